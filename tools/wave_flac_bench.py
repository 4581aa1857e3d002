#!/usr/bin/env python3
"""What lossless FLAC delivery costs: from a micro-batch's vocoded chunks to every request's FLAC stream on the host.

    python tools/wave_flac_bench.py [--reps 9] [--out profiles/wave_flac_bench.txt]
    python tools/wave_flac_bench.py --levels 0,1 --out profiles/wave_flac_lpc_bench.txt

The clock starts when the vocoder returns -- a stand-in `decode_ragged` hands out views of one packed fp32 buffer that is already on the
device, as F5HipVocos does -- and stops when every request's stream is on the host.  Two tails, alternating in one process:
     host    `finish_requests(device_backend=False, sample_rate=..., encoding="flac")`: the chunk waves come down, then join, quantisation,
             `resample_pcm16` and `encode_flac` in numpy
     device  `finish_requests(device_backend=True, ...)`: ONE f5hip_wave_finish call, at 44.1 kHz ONE f5hip_wave_encode call, ONE
             f5hip_wave_flac call (three launches) behind them on the same stream, then the streams' lengths, the streams joined on the
             device and one download of exactly their bytes
Cases: a micro-batch of 1 request and of 8 requests of one chunk of about 10 s, at 24 kHz and at 44.1 kHz.  Wall clock with a device sync,
median and min..max of `--reps` (at least 7) after a warm-up round.  Bytes downloaded per batch: on the host path the fp32 chunk waves (from
their shapes), on the device path the size of the stream download as `infer.backend_stats["flac_bytes"]` counted it plus 4 bytes of length per
request, against the same batch delivered as "pcm16" (the sizes of its results).  Then compressed bytes against PCM bytes (host function, 24 kHz): on the stand-in chunk, on an
utterance of the tiny synthetic-weight model the GPU tests use, and on a two-voice script of it with a 1.5 s gap.  The stand-in is a sum of
sines with a little noise and the tiny model's weights are random, so neither is speech: the ratios say what this content gives, and real
speech has to be measured with real weights.

`--levels` (default "0"): the FLAC levels measured, one block of cases per level (the per-request option `flac_level`; 1 adds LPC subframes).
With more than one level the byte table has a column per level and gains a speech-like signal made here -- a pulse train at a wandering
110 Hz through four formant resonators, with a noise floor -- at 8, 24 and 48 kHz.  That is not speech either, and no default follows from
it: `flac_level` stays opt-in.

Nothing is decided by this file: `serve.DEVICE_BACKEND_DEFAULT` stays as it is, and no threshold is set."""
import argparse
import os
import statistics
import sys
import tempfile
import time
import wave

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tts_indic_server_f5_amd import infer, ops, serve, synth  # noqa: E402

HOP, FRAMES = 256, 938          # a chunk of (FRAMES - 1) * HOP = 239 872 samples, about 10 s
ARCH = dict(dim=256, depth=4, heads=4, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=96)
TEXT = ("I do not care what you call me, I have been a silent spectator. Watching species evolve, empires rise and fall. "
        "Always remember, I am mighty and enduring.")


def _speech_like(n, seed, amp=0.12):
    g = np.random.default_rng(seed)
    t = np.arange(n) / 24000.0
    w = sum(np.sin(2 * np.pi * f * t + p) for f, p in zip(g.uniform(80, 4000, 8), g.uniform(0, 2 * np.pi, 8))) / np.sqrt(8)
    return (amp * w + 0.01 * g.standard_normal(n)).astype(np.float32)


class PackedVocoder:
    """`decode_ragged` as F5HipVocos answers it: views of one packed device buffer, which is made before the clock starts"""

    def __init__(self, n_chunks, device):
        self.n = (FRAMES - 1) * HOP
        self.packed = torch.from_numpy(np.concatenate([_speech_like(self.n, 7 + i) for i in range(n_chunks)])).to(device)

    def decode_ragged(self, mels):
        return list(self.packed.split([self.n] * len(mels)))


def _fmt(ts):
    return f"{statistics.median(ts) * 1e3:8.3f} ms  ({min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f})"


def _formant_pulses(rate, seconds=10.0, seed=3):
    """int16 PCM at `rate`: glottal pulses at a wandering 110 Hz through four two-pole formant resonators (700, 1220, 2600, 3300 Hz), with a
    noise floor.  Speech-like in its spectrum's shape and nothing more."""
    g = np.random.default_rng(seed)
    n = int(rate * seconds)
    f0 = 110.0 * (1.0 + 0.15 * np.sin(2 * np.pi * 0.7 * np.arange(n) / rate) + 0.05 * np.sin(2 * np.pi * 2.3 * np.arange(n) / rate))
    phase = np.cumsum(f0 / rate)
    e = np.zeros(n)
    e[np.flatnonzero(np.diff(np.floor(phase)) > 0) + 1] = 1.0
    e += 0.002 * g.standard_normal(n)
    y = np.zeros(n)
    for freq, bw, gain in ((700, 90, 1.0), (1220, 110, 0.6), (2600, 160, 0.35), (3300, 200, 0.2)):
        if freq >= 0.45 * rate:
            continue
        r = np.exp(-np.pi * bw / rate)
        a1, a2 = 2 * r * np.cos(2 * np.pi * freq / rate), -r * r
        v, v1, v2 = np.empty(n), 0.0, 0.0
        for i, x in enumerate(e.tolist()):
            v0 = x + a1 * v1 + a2 * v2
            v[i] = v0
            v2, v1 = v1, v0
        y += gain * v
    y = 0.25 * y / np.abs(y).max() + 0.0005 * g.standard_normal(n)
    return infer.quantise_pcm16(y.astype(np.float32))


def case(n_req, rate, reps, device, emit, level=None):
    voc = PackedVocoder(n_req, device)
    mel = torch.zeros(FRAMES, 100, device=device)
    groups = [([mel], 0, torch.tensor(0.2))] * n_req
    texts = ["x"] * n_req

    def host(enc="flac"):
        waves = [w for w, _ in infer._chunk_waves(groups, voc, "vocos", infer.target_rms, want_specs=False)]
        return infer.finish_requests(waves, texts, infer.cross_fade_duration, want="pcm16", sample_rate=rate, encoding=enc,
                                     **(dict(flac_level=level) if level is not None and enc == "flac" else {}))

    def dev(enc="flac"):
        waves = [w for w, _ in infer._chunk_waves(groups, voc, "vocos", infer.target_rms, on_device=True, want_specs=False)]
        return infer.finish_requests(waves, texts, infer.cross_fade_duration, device_backend=True, want="pcm16", sample_rate=rate, encoding=enc,
                                     **(dict(flac_level=level) if level is not None and enc == "flac" else {}))

    tails = (("host", host), ("device", dev))
    times, copies, results, flac_bytes = {name: [] for name, _ in tails}, {}, {}, {}
    for rep in range(reps + 1):                      # the first round warms both up (workspaces, tap tables, allocator, numpy buffers)
        for name, fn in tails:
            infer.backend_stats.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[name] = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
            copies[name] = infer.backend_stats["d2h_copies"]
            flac_bytes[name] = infer.backend_stats["flac_bytes"]
    same = all(a.dtype == b.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(results["host"], results["device"]))
    pcm = dev("pcm16")
    if level:    # (LPC subframes: the full reader, on the device -- `decode_flac` reads the level-0 subset alone)
        decoded = all(np.array_equal(np.asarray(y[0]).reshape(-1), p) for y, p in zip(ops.flac_decode(results["device"]), pcm))
    else:
        decoded = all(np.array_equal(infer.decode_flac(s)[0], p) for s, p in zip(results["device"], pcm))
    down = {"host": 4 * voc.n * n_req, "device": flac_bytes["device"] + 4 * n_req}      # fp32 chunk waves | the streams as copied, and their lengths
    pcm_bytes = sum(p.nbytes for p in pcm)
    emit(f"  {n_req} x 10 s -> {rate} Hz flac{'' if level is None else f' level {level}'}  (both tails give the same bytes: {same}; the streams decode to the pcm16 path's samples: {decoded})")
    for name, _ in tails:
        emit(f"      {name:7s} {_fmt(times[name])}   device-to-host copies per batch: {copies[name]}   bytes downloaded per batch: {down[name]}")
    emit(f"      the pcm16 path downloads {pcm_bytes} bytes for the same batch: the device path's download is {down['device'] / pcm_bytes:.3f} of it")


def ratios(device, emit, levels=(None,)):
    """Compressed bytes against PCM bytes at 24 kHz, by the host function; with several levels one figure per level, and the last level's
    bytes relative to the first's."""
    def line(what, pcm, rate=24000):
        if levels == (None,):
            stream = infer.encode_flac(pcm, rate)
            emit(f"  {what}: {len(pcm) / rate:.2f} s, {pcm.nbytes} PCM bytes -> {len(stream)} FLAC bytes ({len(stream) / max(pcm.nbytes, 1):.3f})")
            return
        sizes = [len(infer.encode_flac(pcm, rate, lv)) for lv in levels]
        emit(f"  {what}: {len(pcm) / rate:.2f} s at {rate} Hz, {pcm.nbytes} PCM bytes -> "
             + ", ".join(f"level {lv}: {m} ({m / max(pcm.nbytes, 1):.3f})" for lv, m in zip(levels, sizes))
             + f"; level {levels[-1]} is {sizes[-1] / sizes[0]:.3f} of level {levels[0]}")

    if levels != (None,):
        for rate in (8000, 24000, 48000):
            line("formant-filtered pulse train with a noise floor (made here; not speech)", _formant_pulses(rate), rate)

    line("stand-in chunk (8 sines + noise at 0.01)", infer.quantise_pcm16(_speech_like((FRAMES - 1) * HOP, 7)))
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    vocab = {chr(32 + i): i for i in range(96)}
    mgr = serve.TTSManager(nfe_step=8, device_backend=True).load(F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=vocab),
                                                                 F5HipVocos(synth.vocos_state_dict()))
    try:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "prompt.wav")
            with wave.open(path, "wb") as f:
                f.setnchannels(1); f.setsampwidth(2); f.setframerate(24000)
                f.writeframes((synth.ref_audio(24000 * 2, amp=0.15).numpy()[0] * 32767).astype(np.int16).tobytes())
            line("utterance of the tiny synthetic-weight model", mgr.synthesize(TEXT, ref_audio_path=path, ref_text="Hi there.", seed=7))
            voices = {"main": dict(ref_audio_path=path, ref_text="Hi there."),
                      "town": dict(ref_audio=(synth.ref_audio(16000 * 2, seed=77, amp=0.05), 16000), ref_text="Town speaks.")}
            script = f"{TEXT[:64]} [town] I live in town. [main] Always remember, I endure."
            for gap in (0.0, 1.5):
                line(f"script of it, 3 pieces, gap {gap} s", mgr.synthesize_script(script, voices, gap=gap, seed=7))
    finally:
        mgr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--levels", default="0", help='FLAC levels to measure, e.g. "0,1"')
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wave_flac_bench.txt"))
    args = ap.parse_args()
    reps = max(args.reps, 7)
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    assert torch.cuda.is_available(), "needs a HIP device"
    device = torch.device("cuda:0")
    emit(f"tools/wave_flac_bench.py: median (min .. max) of {reps}, wall clock with a device sync, from the vocoder's return to the FLAC streams on the host")
    emit(f"device {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}")
    levels = tuple(infer.check_flac_level(int(v)) for v in args.levels.split(","))
    for level in levels:
        for n_req in (1, 8):
            for rate in (24000, 44100):
                case(n_req, rate, reps, device, emit, None if levels == (0,) else level)
    emit("compressed bytes against PCM bytes (infer.encode_flac; none of this content is speech, and no default follows from it):")
    ratios(device, emit, (None,) if levels == (0,) else levels)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
