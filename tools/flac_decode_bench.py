#!/usr/bin/env python3
"""What a FLAC upload costs before its samples exist: the host definition `wave_codec.read_flac` against the device decoder
`ops.flac_decode`.

    python tools/flac_decode_bench.py [--reps 9] [--seconds 10] [--out profiles/flac_decode_bench.txt]

Workload: 10 s of a speech-like signal, stereo, 44.1 kHz, 16 bit, block 4096, LPC order 8, mid/side, written by the test-side encoder
(tests/flac_ref.py through tests/flac_cases.full_size).
  host     `read_flac` of the clip: serial Python (3 repetitions: it takes seconds)
  device   `ops.flac_decode` of 1 clip and of 8 clips (the clip eight times: nothing is cached between streams or calls), upload and download
           included, wall clock,
           median and min..max of `--reps` after a warm-up
  launches the five kernels of one call for 1 clip and for 8, from torch's profiler (kernel durations on the device)
Whether FLAC uploads are decoded on the device by default (`serve.DEVICE_DECODE_DEFAULT`) follows from the one-clip pair."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import flac_cases  # noqa: E402
from tts_indic_server_f5_amd import ops, serve  # noqa: E402
from tts_indic_server_f5_amd import wave_codec as W  # noqa: E402


def _fmt(ts):
    return f"{statistics.median(ts) * 1e3:10.3f} ms  ({min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f})"


def _timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def _kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rows = {}
    for e in prof.events():
        if "flac_in_" in e.name:
            name = e.name[e.name.index("flac_in_"):].split("(")[0].split("PK")[0]
            rows[name] = rows.get(name, 0.0) + e.device_time
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    clips = [flac_cases.full_size(a.seconds)] * 8
    stream, x, sizes = clips[0]
    say(f"tools/flac_decode_bench.py: median (min .. max), wall clock with a device sync; device {torch.cuda.get_device_name(0)}")
    say(f"clip: {a.seconds:g} s stereo 44.1 kHz 16 bit, block 4096, LPC order 8, mid/side: {len(stream)} bytes in {len(sizes) - 1} frames "
        f"({2 * x.shape[1]} residuals), written in {time.perf_counter() - t0:.1f} s")
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref = W.read_flac(stream)
        host.append(time.perf_counter() - t0)
    assert np.array_equal(ref[0], x)
    say(f"host    read_flac, 1 clip (3 repetitions):      {_fmt(host)}")
    one, eight = [stream], [c[0] for c in clips]
    got = ops.flac_decode(eight)                                 # warm-up: workspace allocations, the operator library
    for g, c in zip(got, clips):
        assert np.array_equal(g[0], c[1]) and g[1:] == (44100, 16)
    ops.flac_decode(one)
    dev1 = _timed(lambda: ops.flac_decode(one), a.reps)
    dev8 = _timed(lambda: ops.flac_decode(eight), a.reps)
    say(f"device  ops.flac_decode, 1 clip (of {a.reps}):         {_fmt(dev1)}")
    say(f"device  ops.flac_decode, 8 clips (of {a.reps}):        {_fmt(dev8)}   = {statistics.median(dev8) / 8 * 1e3:.3f} ms a clip")
    for label, batch in (("1 clip", one), ("8 clips", eight)):
        try:
            rows = _kernels(lambda: ops.flac_decode(batch))
        except Exception as e:                                   # the profiler is a convenience, not a dependency of the numbers above
            rows = {}
            say(f"launches, {label}: torch's profiler is not available here ({type(e).__name__}: {e})")
        if rows:
            say(f"launches, {label}: " + "   ".join(f"{k} {v:.1f} us" for k, v in rows.items()) + f"   sum {sum(rows.values()):.1f} us")
    faster = max(dev1) < min(host)
    say(f"one clip: device {statistics.median(dev1) * 1e3:.3f} ms against host {statistics.median(host) * 1e3:.3f} ms -> "
        f"DEVICE_DECODE_DEFAULT should be {faster} (it is {serve.DEVICE_DECODE_DEFAULT})")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
