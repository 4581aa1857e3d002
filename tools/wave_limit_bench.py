#!/usr/bin/env python3
"""What the true-peak limiter costs: `ops.wave_loudness(..., true_peak=)` (f5hip_wave_loudness_limit) beside `ops.wave_loudness` on the same
waves in the same run, and beside the host definition `wave_codec.limit_pcm16`.

    python tools/wave_limit_bench.py [--reps 21] [--out profiles/wave_limit_bench.txt]

Eight requests of 10 s, and one ragged batch (1 to 10 s), each three ways: nothing over the ceiling (every tile on the fast path), a burst
per second, and the full-scale alternating square (every tile on the slow path); tag {"target": -23, "true_peak": -1}, for the square
{"true_peak": -1} alone (at -23 LUFS it would stand below the ceiling).  The library call
alone in HIP events on PCM that is already on the device (the call works in place, so every repetition first restores the samples with a
device-to-device copy outside the timed stretch): median and min .. max of `--reps` after a warm-up call.  Beside each: the number call
(`ops.wave_loudness`, target -23) on the same waves, and that same number batch through the `true_peak=` entry (all None), which is the
same launches.  The host function is timed once per case.  The device result is compared with the host's before anything is timed.
Nothing is decided by this file."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_args = argparse.ArgumentParser()
_args.add_argument("--reps", type=int, default=21)
_args.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_limit_bench.txt"))
ARGS = _args.parse_args()
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tts_indic_server_f5_amd import infer, ops, wave_codec  # noqa: E402

RATE = 24000
TAG = wave_codec.LoudnessTag(-23.0, -1.0)


def _speech_like(n, seed, db):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    env = (0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 6))) * (np.sin(2 * np.pi * 0.45 * t + rng.uniform(0, 6)) > -0.5)
    x = np.convolve(rng.standard_normal(n), np.ones(6) / 6.0, mode="same")
    return np.clip(np.rint(10.0 ** (db / 20.0) * 2.5 * env * x * 32768.0), -32768, 32767).astype(np.int16)


def _wave(kind, n, seed):
    if kind == "square":
        x = np.empty(n, dtype=np.int16)
        x[0::2], x[1::2] = 32767, -32768
        return x
    x = _speech_like(n, seed, -38.0)                                    # quiet enough that -23 LUFS leaves every peak below -1 dBTP
    if kind == "bursts":
        for at in range(RATE // 2, n - 200, RATE):
            x[at:at + 120] = np.rint(30000 * np.sin(2 * np.pi * 2000 * np.arange(120) / RATE) * np.hanning(120)).astype(np.int16)
    return x


def _events(fn, restore, reps):
    restore(); fn()
    out = []
    for _ in range(reps):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return "%.3f (%.3f .. %.3f)" % (statistics.median(out), min(out), max(out))


def main():
    dev = torch.device("cuda:0")
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    emit(f"# tools/wave_limit_bench.py on {torch.cuda.get_device_name(0)} (the name the driver reports; {torch.cuda.get_device_properties(0).gcnArchName}): "
         f"median ms (min .. max) of {ARGS.reps} after a warm-up call")
    emit("# the library call alone in HIP events, PCM on the device, restored before every repetition outside the timed stretch; tag = target -23 LUFS, -1 dBTP")
    emit("# limit = ops.wave_loudness(..., true_peak=); number = ops.wave_loudness on the same waves; number* = the number batch through the true_peak= entry")
    for batch, lens in (("8 x 10 s", [10 * RATE] * 8), ("ragged 1 .. 10 s", [RATE * s + 17 * s for s in (1, 2, 3, 5, 7, 8, 9, 10)])):
        for kind in ("quiet", "bursts", "square"):
            tag = TAG if kind != "square" else TAG._replace(target=None)
            spec, number_k = infer.WaveSpec(loudness=tag), infer.WaveSpec(loudness=TAG).gain_constant
            waves = [_wave(kind, n, 11 + i) for i, n in enumerate(lens)]
            offsets, off = [], 0
            for x in waves:
                offsets.append(off)
                off += (len(x) + 7) & ~7
            buf = np.zeros(off + 8, dtype=np.int16)
            for o, x in zip(offsets, waves):
                buf[o:o + len(x)] = x
            clean = torch.from_numpy(buf).to(dev)
            pcm = clean.clone()
            restore = lambda: pcm.copy_(clean)   # noqa: E731
            t0 = time.perf_counter()
            want = [wave_codec.limit_pcm16(x, tag) for x in waves]
            host_ms = (time.perf_counter() - t0) * 1e3
            gk, cs, none = [number_k] * len(lens), [spec.ceiling] * len(lens), [None] * len(lens)
            limit = lambda: ops.wave_loudness(pcm, offsets, lens, None, [spec.gain_constant] * len(lens), true_peak=cs)   # noqa: E731
            number = lambda: ops.wave_loudness(pcm, offsets, lens, None, gk)   # noqa: E731
            through = lambda: ops.wave_loudness(pcm, offsets, lens, None, gk, true_peak=none)   # noqa: E731
            restore(); limit()
            got = pcm.cpu().numpy()
            assert all(np.array_equal(got[o:o + len(x)], w) for o, x, w in zip(offsets, waves, want)), (batch, kind)
            slow = sum(not np.array_equal(w, wave_codec.limit_samples(x, wave_codec.limit_gain(*infer.measure_loudness(x)[:2], spec.gain_constant), 1 << 20))
                       for x, w in zip(waves, want))                            # (against the same gain under a ceiling nothing reaches)
            emit(f"{batch:18s} {kind:7s} limit {_events(limit, restore, ARGS.reps)}  number {_events(number, restore, ARGS.reps)}  "
                 f"number* {_events(through, restore, ARGS.reps)}  host limit_pcm16 {host_ms:.1f} ms  (requests the limiter changed: {slow} of {len(lens)})")
    with open(ARGS.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
