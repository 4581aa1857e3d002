#!/usr/bin/env python3
"""What a multi-voice script costs as one request, against what a client had to do before there was one.

    python tools/script_bench.py [--reps 9] [--out profiles/script_bench.txt]

A 6-piece, 3-voice `[tag]` script whose voices are uploaded clips (new samples every round, so nothing is served from the clip cache), on
F5-TTS Base width with synthetic weights, 32 NFE, Vocos, no batcher, served two ways that alternate in one process:
     (a) pieces   what the parent commit (98dd219) forces a client to do: six `synthesize_clip` calls, one per piece, and a concatenation on
                  the client's side -- six sampler calls, six vocoder calls, the three voices' front-ends and mels one at a time
     (b) script   one `synthesize_script` call: one sampler call, one vocoder call, one ragged front-end call and one ragged mel launch for the
                  three new voices, one join
each with `device_backend` on and off.  Wall clock with a device sync around the whole request, median and min..max of `--reps` (at least 9)
after a warm-up round; per request: device-to-host copies (`infer.backend_stats`), mel launches (`cond_mel` calls + `mel_ragged_launches`) and
join launches (`wave_finish_launches`).

Nothing is decided by this file: no default changes and no threshold is set."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tts_indic_server_f5_amd import _lib, infer, serve, synth  # noqa: E402

VOCAB = {chr(32 + i): i for i in range(96)}
REF_TEXT = "Some call me nature, others call me mother nature."
PIECES = [("main", "I have been a silent spectator for billions of years."), ("town", "We watched every species evolve from the square."),
          ("hill", "Empires rise and fall, and the hill stays where it is."), ("main", "Always remember, I am mighty and enduring."),
          ("town", "Respect me and I will nurture you."), ("hill", "Ignore me and you shall face the consequences.")]
SCRIPT = " ".join(f"[{tag}] {text}" for tag, text in PIECES)
RATES = {"main": 24000, "town": 44100, "hill": 48000}


def _speech_like(n, sr, seed, amp=0.12):
    g = np.random.default_rng(seed)
    t = np.arange(n) / sr
    w = sum(np.sin(2 * np.pi * f * t + p) for f, p in zip(g.uniform(80, 4000, 8), g.uniform(0, 2 * np.pi, 8))) / np.sqrt(8)
    return (amp * w + 0.01 * g.standard_normal(n)).astype(np.float32)


def _voices(seed):
    """three uploaded clips of 5 s at three source rates, new samples for every seed"""
    return {tag: dict(ref_audio=(torch.from_numpy(_speech_like(5 * sr, sr, seed + k)[None]), sr), ref_text=REF_TEXT)
            for k, (tag, sr) in enumerate(RATES.items())}


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _fmt(ts):
    return f"{statistics.median(ts) * 1e3:9.2f} ms  ({min(ts) * 1e3:.2f} .. {max(ts) * 1e3:.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "script_bench.txt"))
    args = ap.parse_args()
    reps = max(args.reps, 9)
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    assert torch.cuda.is_available(), "needs a HIP device"
    from tts_indic_server_f5_amd.model import F5TTS_BASE, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    model = F5HipModel(F5TTS_BASE, synth.dit_state_dict(), vocab_char_map=VOCAB)
    voc = F5HipVocos(synth.vocos_state_dict())
    mel_calls = [0]
    lazy = model.cond_mel

    def counted(audio):
        mel_calls[0] += 1
        return lazy(audio)
    model.cond_mel = counted

    emit(f"tools/script_bench.py: median (min .. max) of {reps}, wall clock with a device sync around the whole request")
    emit(f"workload: a 6-piece, 3-voice script, uploaded clips of 5 s at 24 / 44.1 / 48 kHz (new samples every round); F5-TTS Base width, synthetic "
         f"weights, 32 NFE, Vocos, no batcher; device {torch.cuda.get_device_name(0)}")
    emit("(a) pieces: six synthesize_clip calls and a host concatenation -- all the parent commit 98dd219 offers; (b) script: one synthesize_script call")
    for backend in (False, True):
        mgr = serve.TTSManager(nfe_step=32, device_backend=backend, device_frontend=True).load(model, voc)

        def pieces(voices, seed):
            out = [mgr.synthesize_clip(text, voices[tag]["ref_audio"], REF_TEXT, seed=seed + i) for i, (tag, text) in enumerate(PIECES)]
            return np.concatenate(out)

        def script(voices, seed):
            return mgr.synthesize_script(SCRIPT, voices, seed=seed)

        ways = (("(a) pieces", pieces), ("(b) script", script))
        times, stats = {name: [] for name, _ in ways}, {}
        for rep in range(reps + 1):                      # the first round warms both up (workspaces, tap tables, mel tables, allocator)
            for k, (name, fn) in enumerate(ways):
                voices = _voices(1000 * rep + 100 * k + (50 if backend else 0))
                infer.backend_stats.clear()
                _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")
                mel_calls[0] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                wave = fn(voices, 7 * rep)
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
                stats[name] = (infer.backend_stats["d2h_copies"], mel_calls[0] + _counter("mel_ragged_launches"), _counter("wave_finish_launches"),
                               _counter("ref_frontend_launches"), len(wave) / 24000.0)
        mgr.model = None                                 # (the model objects are shared with the next manager: nothing to close)
        emit(f"device_backend={backend}")
        for name, _ in ways:
            d2h, mels, joins, fe, secs = stats[name]
            emit(f"    {name}  {_fmt(times[name])}   audio {secs:5.2f} s   device-to-host copies {d2h:2d}   mel launches {mels}   "
                 f"join launches {joins}   front-end launches {fe}")
        a, b = statistics.median(times["(a) pieces"]), statistics.median(times["(b) script"])
        emit(f"    (b) / (a) = {b / a:.3f}: the script request {'beats' if b < a else 'does NOT beat'} the six calls here")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
