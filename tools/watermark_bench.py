#!/usr/bin/env python3
"""What the provenance watermark costs: the host definitions `wave_codec.mark_pcm16` / `detect_watermark` against the device calls
`ops.wave_mark` / `ops.watermark_detect`.

    python tools/watermark_bench.py [--reps 9] [--out profiles/watermark_bench.txt]

     mark     eight requests of 10 s of 24 kHz int16 PCM: `mark_pcm16` of each on the host (numpy) against ONE `ops.wave_mark` call (two
              launches) on PCM that is already on the device, in HIP events -- where `_finish_on_device` calls it, nothing goes up or comes
              down for it
     detect   eight clips of 10 s against four keys: `detect_watermark` of each on the host (fp64 FFTs) against ONE `ops.watermark_detect`
              call (four launches) on clips that are already on the device, in HIP events, and once more with the score rows' download
     dz       the maximum |z_device - z_host(fp64)| over the clips of tests/test_gpu_watermark_detect.py, against one key and against three:
              the figure that test's bound is 8 x of
Median and min .. max of `--reps` after a warm-up round.  The hosts are the test suite's synthetic speech-like signals (tests/denoise_ref.py),
not recordings.  Nothing is decided by this file: no default follows from it and no threshold is set; no earlier commit has this path to
compare with."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_args = argparse.ArgumentParser()
_args.add_argument("--reps", type=int, default=9)
_args.add_argument("--out", default=os.path.join(ROOT, "profiles", "watermark_bench.txt"))
ARGS = _args.parse_args()
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import watermark_ref as ref  # noqa: E402
from tts_indic_server_f5_amd import ops, wave_codec  # noqa: E402

RATE, SECONDS, COUNT = 24000, 10, 8
KEYS = [1, 0xDEADBEEF, 2 ** 47 + 5, 77]


def _stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def _fmt(s):
    return f"{s['median']:9.3f} ({s['min']:.3f} .. {s['max']:.3f})"


def _wall(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return _stats(out)


def _events(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return _stats(out)


def main():
    dev = torch.device("cuda:0")
    n = SECONDS * RATE
    pcms = [np.ascontiguousarray(ref.host(n, s)) for s in range(COUNT)]
    offsets = [i * n for i in range(COUNT)]
    packed = np.concatenate(pcms)
    lines = [f"# tools/watermark_bench.py on {torch.cuda.get_device_name(0)}: median ms (min .. max) of {ARGS.reps} after a warm-up round; "
             f"{COUNT} requests / clips of {SECONDS} s, synthetic speech-like hosts", ""]

    # ---- mark
    marked = [None] * COUNT

    def host_mark():
        marked[:] = [wave_codec.mark_pcm16(x, KEYS[i % 2]) for i, x in enumerate(pcms)]

    h = _wall(host_mark, max(3, min(ARGS.reps, 5)))
    pcm = torch.from_numpy(packed).to(dev)
    keys = [KEYS[i % 2] for i in range(COUNT)]
    ops.wave_mark(pcm, offsets, [n] * COUNT, None, keys)
    assert np.array_equal(pcm.cpu().numpy(), np.concatenate(marked)), "the device call does not equal the host definition"
    d = _events(lambda: ops.wave_mark(pcm, offsets, [n] * COUNT, None, keys), ARGS.reps)   # (marks a marked wave again: the same work)
    lines += ["mark: host mark_pcm16 of each request against ONE ops.wave_mark call, PCM on the device (HIP events; the request table's staged copy included)",
              f"  {'host':>32s} {'device':>32s}   host / device",
              f"  {_fmt(h):>32s} {_fmt(d):>32s}   {h['median'] / d['median']:.0f}", ""]
    print("\n".join(lines[-4:]), flush=True)

    # ---- detect
    clips = [(m.astype(np.float32) / np.float32(32768.0)) for m in marked]
    host_scores = [None] * COUNT

    def host_detect():
        host_scores[:] = [wave_codec.detect_watermark(x, KEYS) for x in clips]

    h = _wall(host_detect, 3)
    wave = torch.from_numpy(np.concatenate(clips)).to(dev)
    carriers = ops.watermark_carriers(KEYS, dev)
    rows = ops.watermark_detect(wave, offsets, [n] * COUNT, carriers).cpu().numpy()
    got = [ops.watermark_scores(r, KEYS) for r in rows]
    assert all(g.detected == s.detected for gs, ss in zip(got, host_scores) for g, s in zip(gs, ss)), "the device's decisions are not the host's"
    d = _events(lambda: ops.watermark_detect(wave, offsets, [n] * COUNT, carriers), ARGS.reps)
    dd = _wall(lambda: ops.watermark_detect(wave, offsets, [n] * COUNT, carriers).cpu(), ARGS.reps)
    lines += [f"detect: host detect_watermark of each clip against ONE ops.watermark_detect call, {len(KEYS)} keys, clips on the device",
              f"  {'host (fp64 FFTs)':>32s} {'device, HIP events':>32s} {'device + rows down, wall':>32s}   host / device",
              f"  {_fmt(h):>32s} {_fmt(d):>32s} {_fmt(dd):>32s}   {h['median'] / d['median']:.0f}",
              f"  z of the marked key, host: {min(s[i % 2].z for i, s in enumerate(host_scores)):.2f} .. {max(s[i % 2].z for i, s in enumerate(host_scores)):.2f}", ""]
    print("\n".join(lines[-5:]), flush=True)

    # ---- dz over the GPU test's clips
    import test_gpu_watermark_detect as t
    tc = t._clips()
    hs = [wave_codec.detect_watermark(x, [t.K1, t.K2, t.K3]) for x in tc]
    worst = 0.0
    lines.append("dz: |z_device - z_host(fp64)| over the clips of tests/test_gpu_watermark_detect.py")
    for ks in ((t.K1,), (t.K1, t.K2, t.K3)):
        r, _, _ = t._device(tc, list(ks))
        for i, x in enumerate(tc):
            for g, key in zip(ops.watermark_scores(r[i], list(ks)), ks):
                hz = hs[i][(t.K1, t.K2, t.K3).index(key)].z
                worst = max(worst, abs(g.z - hz))
                lines.append(f"  {len(ks)} key(s)  clip {i} ({len(x):6d} samples)  key {key:#x}  z_dev {g.z:10.6f}  z_host {hz:10.6f}  dz {abs(g.z - hz):.3e}")
    lines.append(f"  maximum {worst:.3e}")
    print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {ARGS.out}")


if __name__ == "__main__":
    main()
