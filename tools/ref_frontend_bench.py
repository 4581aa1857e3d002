#!/usr/bin/env python3
"""What an uploaded reference clip costs before its request can be sampled: the host front-end against the device one.

    python tools/ref_frontend_bench.py [--reps 9] [--out profiles/ref_frontend_bench.txt]
    python tools/ref_frontend_bench.py --host-only --baseline-audio-prep FILE --baseline-label "parent revision" --out profiles/ref_frontend_prestep_cpu.txt

1. Front-end alone, n = 1 and 8 clips of 12 s (44.1 kHz stereo; 48 kHz mono), each from host fp32 samples to the mel on the device:
     host    per clip `infer._prepare_reference` (torch CPU: mean, square, strided conv1d), upload of the 24 kHz wave, mel
     device  `infer.prepare_voices`: one upload of the packed clips, ONE f5hip_ref_frontend call (two launches), one download of the
             rms values, then the mel per clip
   Wall clock with a device sync, the two alternating in one process, median and min..max of `--reps` (at least 7) after a warm-up.
2. `TTSManager.synthesize_clip` of one request of about 10 s of speech with a fresh 44.1 kHz stereo upload (every repetition uploads
   different samples, so nothing is served from the clip cache), `device_frontend` on and off, alternating.  F5-TTS Base width,
   synthetic weights, 32 NFE, Vocos.
3. The host pre-step `preprocess_ref_audio_text` on a 30 s, 44.1 kHz, mono, 16-bit clip (CPU only; `--baseline-audio-prep FILE` times
   another revision of audio_prep.py on the same clip next to it, named by `--baseline-label`).

Which front-end uploads take by default (`serve.DEVICE_FRONTEND_DEFAULT`) follows from part 1 at n = 1: the device one only where it
beats the host one by more than the spread (max - min) of either in the same run."""
import argparse
import importlib.util
import os
import statistics
import sys
import tempfile
import time
import wave

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tts_indic_server_f5_amd import audio_prep, infer, synth  # noqa: E402

VOCAB = {chr(32 + i): i for i in range(96)}
REF_TEXT = "Some call me nature, others call me mother nature."
TEXT = "I have been a silent spectator for billions of years and watched every species evolve."   # about 10 s of speech after a 6 s prompt


def _speech_like(n, sr, seed, amp=0.12):
    """a sum of eight sines between 80 Hz and 4 kHz plus a little noise (synth.ref_audio's recipe, at any rate)"""
    g = np.random.default_rng(seed)
    t = np.arange(n) / sr
    w = sum(np.sin(2 * np.pi * f * t + p) for f, p in zip(g.uniform(80, 4000, 8), g.uniform(0, 2 * np.pi, 8))) / np.sqrt(8)
    return (amp * w + 0.01 * g.standard_normal(n)).astype(np.float32)


def _clip(seconds, sr, channels, seed):
    return torch.from_numpy(np.stack([_speech_like(int(seconds * sr), sr, seed + 31 * c) for c in range(channels)])), sr


def _stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def _fmt(ts):
    med, lo, hi = _stats(ts)
    return f"{med * 1e3:8.3f} ms  ({lo * 1e3:.3f} .. {hi * 1e3:.3f})"


def front_end(model, reps, emit):
    dev = model.device

    def host(clips):
        mels = []
        for wav, sr in clips:
            audio, _ = infer._prepare_reference(wav, sr, 0.1, dev)
            mels.append(model.cond_mel(audio))
        return mels

    def device(clips):
        return [v.cond(model) for v in infer.prepare_voices(clips, 0.1, device=dev)]

    verdicts = []
    for label, sr, ch in (("12 s, 44.1 kHz stereo", 44100, 2), ("12 s, 48 kHz mono", 48000, 1)):
        for n in (1, 8):
            clips = [_clip(12.0, sr, ch, seed=100 * n + i) for i in range(n)]
            times = {"host": [], "device": []}
            for rep in range(reps + 1):                      # the first round warms both up (tap tables, workspaces, mel tables)
                for name, fn in (("host", host), ("device", device)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(clips)
                    torch.cuda.synchronize()
                    if rep:
                        times[name].append(time.perf_counter() - t0)
            emit(f"  {label:22s} n = {n}:  host {_fmt(times['host'])}   device {_fmt(times['device'])}")
            if n == 1:
                (hm, hl, hh), (dm, dl, dh) = _stats(times["host"]), _stats(times["device"])
                verdicts.append(hm - dm > max(hh - hl, dh - dl))
    return verdicts


def clone_latency(model, voc, reps, emit):
    from tts_indic_server_f5_amd import serve
    mgrs = {flag: serve.TTSManager(nfe_step=32, device_frontend=flag).load(model, voc) for flag in (True, False)}
    times = {True: [], False: []}
    n = 0
    for rep in range(reps + 1):
        for flag, mgr in mgrs.items():
            clip = _clip(6.0, 44100, 2, seed=1000 + rep)     # the same upload for both, a new one every repetition
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = len(mgr.synthesize_clip(TEXT, clip, REF_TEXT, seed=1))
            if rep:
                times[flag].append(time.perf_counter() - t0)
    emit(f"  synthesize_clip, one request, {n / 24000:.1f} s of speech, 6 s 44.1 kHz stereo upload (not cached):")
    emit(f"    device front-end {_fmt(times[True])}")
    emit(f"    host front-end   {_fmt(times[False])}")


def pre_step(reps, emit, baseline, label):
    sr, seconds = 44100, 30.0
    x = _speech_like(int(sr * seconds), sr, seed=7, amp=0.2)
    gate = np.ones_like(x)
    for a, b in ((0.0, 0.4), (4.0, 4.3), (9.5, 10.8), (14.0, 14.2), (21.0, 22.5), (29.5, 30.0)):      # pauses, in seconds
        gate[int(a * sr):int(b * sr)] = 0.0
    pcm = np.clip(np.rint(x * gate * 32768), -32768, 32767).astype("<i2")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "clip.wav")
        with wave.open(path, "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(sr)
            f.writeframes(pcm.tobytes())
        mods = [("this revision", audio_prep)]
        if baseline:
            spec = importlib.util.spec_from_file_location("audio_prep_baseline", baseline)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            mods.append((label or f"baseline ({os.path.basename(baseline)})", mod))
        for name, mod in mods:
            ts = []
            for rep in range(reps + 1):
                t0 = time.perf_counter()
                out, _ = mod.preprocess_ref_audio_text(path, "some words", show_info=lambda *_: None)
                if rep:
                    ts.append(time.perf_counter() - t0)
                os.unlink(out)
            emit(f"  preprocess_ref_audio_text, 30 s 44.1 kHz mono 16-bit, {name}: {_fmt(ts)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ref_frontend_bench.txt"))
    ap.add_argument("--host-only", action="store_true", help="part 3 only (no HIP device needed)")
    ap.add_argument("--baseline-audio-prep", default=None)
    ap.add_argument("--baseline-label", default=None)
    args = ap.parse_args()
    reps = max(args.reps, 7)
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    emit(f"tools/ref_frontend_bench.py: median (min .. max) of {reps}, wall clock" + ("" if args.host_only else " with a device sync"))
    if not args.host_only:
        assert torch.cuda.is_available(), "needs a HIP device (or --host-only)"
        from tts_indic_server_f5_amd.model import F5TTS_BASE, F5HipModel
        from tts_indic_server_f5_amd.vocoder import F5HipVocos
        model = F5HipModel(F5TTS_BASE, synth.dit_state_dict(), vocab_char_map=VOCAB)
        voc = F5HipVocos(synth.vocos_state_dict())
        emit(f"device {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}")
        emit("1. front-end from host samples to the device mel (host: _prepare_reference + upload + mel; device: upload + ref_frontend + mel)")
        verdicts = front_end(model, reps, emit)
        emit(f"   n = 1: the device front-end beats the host one by more than the run's spread in {sum(verdicts)} of {len(verdicts)} cases"
             f" -> uploads default to the {'device' if all(verdicts) else 'host'} front-end")
        emit("2. one cloning request end to end (F5-TTS Base width, synthetic weights, 32 NFE, Vocos)")
        clone_latency(model, voc, reps, emit)
    emit("3. host pre-step (CPU)")
    pre_step(reps, emit, args.baseline_audio_prep, args.baseline_label)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
