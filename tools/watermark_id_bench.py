#!/usr/bin/env python3
"""What the watermark's trace ids cost: `ops.wave_mark` with and without ids and `ops.watermark_read_ids` next to `ops.watermark_detect`,
each against the host definitions `wave_codec.mark_pcm16` / `read_watermark`, in the same run.

    python tools/watermark_id_bench.py [--reps 9] [--out profiles/watermark_id_bench.txt]

     mark     eight requests of 10 s of 24 kHz int16 PCM that is already on the device, in HIP events: ONE `ops.wave_mark` call with an id
              on every request (f5hip_wave_mark_ids: two launches), ONE without ids (f5hip_wave_mark), and `mark_pcm16` of each tagged
              request on the host (numpy)
     read     eight clips of 10 s against one key, clips on the device, in HIP events: ONE `ops.watermark_read_ids` call (four launches)
              next to ONE `ops.watermark_detect` call on the same four carrier rows (the key's and its three sub-keys' as four keys), and
              `read_watermark` of each clip on the host (fp64 FFTs); once more with the rows' download
     dz       the maximum |z_d(device) - z_d(host fp64)| over the clips of tests/test_gpu_watermark_id_read.py, against one key and against
              two: the figure that test's bound is 8 x of
Median and min .. max of `--reps` after a warm-up round.  The hosts are the test suite's synthetic speech-like signals (tests/denoise_ref.py),
not recordings.  Nothing is decided by this file: no default follows from it and no threshold is set; no earlier commit has this path to
compare with."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_args = argparse.ArgumentParser()
_args.add_argument("--reps", type=int, default=9)
_args.add_argument("--out", default=os.path.join(ROOT, "profiles", "watermark_id_bench.txt"))
ARGS = _args.parse_args()
sys.argv = sys.argv[:1]                                # (tools/watermark_bench.py parses its own on import)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import watermark_ref as ref  # noqa: E402
from tts_indic_server_f5_amd import ops, wave_codec  # noqa: E402
from watermark_bench import _events, _fmt, _wall  # noqa: E402

RATE, SECONDS, COUNT = 24000, 10, 8
KEY = 1
IDS = [int(v) for v in np.random.default_rng(0).integers(0, 2 ** 30, COUNT)]


def main():
    dev = torch.device("cuda:0")
    n = SECONDS * RATE
    pcms = [np.ascontiguousarray(ref.host(n, s)) for s in range(COUNT)]
    offsets = [i * n for i in range(COUNT)]
    packed = np.concatenate(pcms)
    tags = [wave_codec.WatermarkTag(KEY, i) for i in IDS]
    lines = [f"# tools/watermark_id_bench.py on {torch.cuda.get_device_name(0)}: median ms (min .. max) of {ARGS.reps} after a warm-up round; "
             f"{COUNT} requests / clips of {SECONDS} s, synthetic speech-like hosts (not real speech)", ""]

    # ---- mark
    marked = [None] * COUNT

    def host_mark():
        marked[:] = [wave_codec.mark_pcm16(x, t) for x, t in zip(pcms, tags)]

    h = _wall(host_mark, max(3, min(ARGS.reps, 5)))
    pcm = torch.from_numpy(packed).to(dev)
    ops.wave_mark(pcm, offsets, [n] * COUNT, None, tags)
    assert np.array_equal(pcm.cpu().numpy(), np.concatenate(marked)), "the device call does not equal the host definition"
    d_ids = _events(lambda: ops.wave_mark(pcm, offsets, [n] * COUNT, None, tags), ARGS.reps)   # (marks a marked wave again: the same work)
    d_key = _events(lambda: ops.wave_mark(pcm, offsets, [n] * COUNT, None, [KEY] * COUNT), ARGS.reps)
    lines += ["mark: ONE ops.wave_mark call with an id on every request, ONE without ids, host mark_pcm16 of each tagged request; PCM on the device "
              "(HIP events; the request table's staged copy included)",
              f"  {'device, with ids':>32s} {'device, keys only':>32s} {'host, with ids':>32s}   host / device",
              f"  {_fmt(d_ids):>32s} {_fmt(d_key):>32s} {_fmt(h):>32s}   {h['median'] / d_ids['median']:.0f}", ""]
    print("\n".join(lines[-4:]), flush=True)

    # ---- read
    clips = [(m.astype(np.float32) / np.float32(32768.0)) for m in marked]
    host_reads = [None] * COUNT

    def host_read():
        host_reads[:] = [wave_codec.read_watermark(x, [KEY])[0] for x in clips]

    h = _wall(host_read, 3)
    wave = torch.from_numpy(np.concatenate(clips)).to(dev)
    tagged = ops.watermark_tag_carriers([KEY], dev)
    four = tagged.reshape(4, -1)                                                        # the same rows as four keys of the detector
    rows = ops.watermark_read_ids(wave, offsets, [n] * COUNT, tagged).cpu().numpy()
    got = [ops.watermark_reads(r, [KEY])[0] for r in rows]
    assert [g.id for g in got] == [r.id for r in host_reads] == IDS, "the device's ids are not the host's"
    d_read = _events(lambda: ops.watermark_read_ids(wave, offsets, [n] * COUNT, tagged), ARGS.reps)
    d_det = _events(lambda: ops.watermark_detect(wave, offsets, [n] * COUNT, four), ARGS.reps)
    dd = _wall(lambda: ops.watermark_read_ids(wave, offsets, [n] * COUNT, tagged).cpu(), ARGS.reps)
    lines += ["read: ONE ops.watermark_read_ids call against one key, ONE ops.watermark_detect call on the same four carrier rows, host read_watermark of "
              "each clip; clips on the device",
              f"  {'read_ids, HIP events':>32s} {'detect x 4 rows, HIP events':>32s} {'read_ids + rows down, wall':>32s} {'host (fp64 FFTs)':>32s}   host / device",
              f"  {_fmt(d_read):>32s} {_fmt(d_det):>32s} {_fmt(dd):>32s} {_fmt(h):>32s}   {h['median'] / d_read['median']:.0f}",
              f"  id_z, host: {min(r.id_z for r in host_reads):.2f} .. {max(r.id_z for r in host_reads):.2f}; every id read right on both", ""]
    print("\n".join(lines[-5:]), flush=True)

    # ---- dz over the GPU test's clips
    import test_gpu_watermark_id_read as t
    tc = t._clips()
    hs = [[t._host_symbols(x, k) for k in (t.K1, t.K2)] for x in tc]
    worst = 0.0
    lines.append("dz: |z_d(device) - z_d(host fp64)| over the clips of tests/test_gpu_watermark_id_read.py (symbols on which both agree)")
    for ks in ((t.K1,), (t.K1, t.K2)):
        r, _, _ = t._device(tc, list(ks))
        for i, x in enumerate(tc):
            for j, key in enumerate(ks):
                for dsym, (s, z) in enumerate(hs[i][(t.K1, t.K2).index(key)]):
                    s_dev, z_dev = int(r[i][j][4 + 2 * dsym]), float(r[i][j][5 + 2 * dsym])
                    if s_dev == s:
                        worst = max(worst, abs(z_dev - z))
                    lines.append(f"  {len(ks)} key(s)  clip {i} ({len(x):6d} samples)  key {key:#x}  symbol {dsym}  s_dev {s_dev:4d}  s_host {s:4d}  "
                                 f"z_dev {z_dev:10.6f}  z_host {z:10.6f}  dz {abs(z_dev - z):.3e}")
    lines.append(f"  maximum {worst:.3e}")
    print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {ARGS.out}")


if __name__ == "__main__":
    main()
