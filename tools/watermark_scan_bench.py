#!/usr/bin/env python3
"""What the watermark scan costs: `ops.watermark_scan` against the host definition `wave_codec.scan_watermark`, in the same run.

    python tools/watermark_scan_bench.py [--reps 9] [--out profiles/watermark_scan_bench.txt]

     scan     recordings of 60 s and 600 s (10 s synthetic hosts joined; some of them marked with a trace id, a different phase each)
              against 1 key and against 4, ids read on every span.  Both paths from the fp32 samples on the host to the spans on the host:
              the device path is the upload, ONE `ops.watermark_scan_rows` call over every window, the rows' download, the span rule on
              the host, one more call with ids over the spans and its download (wall clock); the host path is `scan_watermark` (fp64 FFTs)
     dz       the maximum |z(device) - z(host fp64)| over ALL window rows and span rows (the key's z and the symbols' z_d on which both
              agree) of those four cases, and over the rows of tests/test_gpu_watermark_scan.py: the figure that test's bound is 8 x of
Median and min .. max of `--reps` after a warm-up round.  The hosts are the test suite's synthetic speech-like signals (tests/denoise_ref.py),
not recordings.  Nothing is decided by this file: no default follows from it and no threshold is set; no earlier commit has this path to
compare with."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_args = argparse.ArgumentParser()
_args.add_argument("--reps", type=int, default=9)
_args.add_argument("--out", default=os.path.join(ROOT, "profiles", "watermark_scan_bench.txt"))
ARGS = _args.parse_args()
sys.argv = sys.argv[:1]                                # (tools/watermark_bench.py parses its own on import)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import watermark_ref as ref  # noqa: E402
from tts_indic_server_f5_amd import ops, wave_codec  # noqa: E402
from watermark_bench import _fmt, _wall  # noqa: E402

RATE, PART = 24000, 10
KEYS = [1, 2, 3, 4]
P = wave_codec.WATERMARK_PERIOD


def recording(seconds):
    """fp32 [seconds * 24000]: 10 s hosts joined; every third one marked, under KEYS in turn, with an id, cut by 997 i samples (its phase)."""
    parts, marked = [], 0
    for i in range(seconds // PART):
        x = ref.host(PART * RATE + 997 * i, i % 60)
        if i % 3 == 1:
            x = wave_codec.mark_pcm16(x, wave_codec.WatermarkTag(KEYS[marked % len(KEYS)], 1000 + i))
            marked += 1
        parts.append(x[997 * i:])
    return np.concatenate(parts).astype(np.float32) / np.float32(32768.0)


def row_deviation(x, keys, dev):
    """(max |z_dev - z_host|, rows, span ranges) over every window row (ids off) and every span row (ids on) of x, both agreeing on the
    offset and the symbol where a symbol's z_d is compared."""
    import test_gpu_watermark_scan as t
    n = len(x)
    S = -(-n // P)
    windows = [(w, min(w + wave_codec.WATERMARK_SCAN_WINDOW, S) - w) for w in range(wave_codec.watermark_windows(n))]
    wave = torch.from_numpy(x).to(dev)
    got = ops.watermark_scan_rows(wave, windows, ops.watermark_carriers(keys, dev)).cpu().numpy()
    spans = sorted({(g.first, g.count) for g in wave_codec.watermark_spans([ops.watermark_scores(got[w], keys) for w in range(len(windows))], n)})
    seg, _ = wave_codec.scan_window_rows(np.asarray(x, dtype=np.float64))
    worst = 0.0
    for at in range(0, len(windows), 64):                                               # the host rows 64 windows at a time
        for row, hrow in zip(got[at:at + 64], t._host_rows(x, windows[at:at + 64], keys, seg)):
            worst = max([worst] + [abs(float(row[j][0]) - hrow[j][0]) for j in range(len(keys))])
    if spans:
        full = ops.watermark_scan_rows(wave, spans, ops.watermark_tag_carriers(keys, dev), ids=True).cpu().numpy()
        for row, hrow in zip(full, t._host_rows(x, spans, keys, seg)):
            for j in range(len(keys)):
                z, o, symbols = hrow[j]
                worst = max(worst, abs(float(row[j][0]) - z))
                for d, (s, zd) in enumerate(symbols):
                    if int(row[j][1]) == o and int(row[j][4 + 2 * d]) == s:
                        worst = max(worst, abs(float(row[j][5 + 2 * d]) - zd))
    return worst, (len(windows) + len(spans)) * len(keys), len(spans)


def main():
    dev = torch.device("cuda:0")
    lines = [f"# tools/watermark_scan_bench.py on {torch.cuda.get_device_name(0)}: median ms (min .. max) of {ARGS.reps} after a warm-up round; "
             "from the fp32 samples on the host to the spans on the host; synthetic speech-like hosts (not real speech)", "",
             f"  {'recording':>10s} {'keys':>5s} {'spans':>6s} {'device path, wall':>34s} {'host scan_watermark (fp64), wall':>34s}   host / device   launches"]
    import ctypes as C
    from tts_indic_server_f5_amd import _lib

    def counter(name):
        v = C.c_int64(0)
        _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
        return v.value

    dz = []
    for seconds in (60, 600):
        x = recording(seconds)
        for keys in (KEYS[:1], KEYS):
            want = wave_codec.scan_watermark(x, keys)
            _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset")
            got = ops.watermark_scan(torch.from_numpy(x).to(dev), keys)
            launches = counter("watermark_scan_launches")
            assert [(g.key, g.start, g.end, g.offset, g.id) for g in got] == [(w.key, w.start, w.end, w.offset, w.id) for w in want], "the device's spans are not the host's"
            d = _wall(lambda: ops.watermark_scan(torch.from_numpy(x).to(dev), keys), ARGS.reps)
            h = _wall(lambda: wave_codec.scan_watermark(x, keys), ARGS.reps if seconds <= 60 else min(ARGS.reps, 3))
            lines.append(f"  {seconds:>8d} s {len(keys):>5d} {len(got):>6d} {_fmt(d):>34s} {_fmt(h):>34s}   {h['median'] / d['median']:13.1f}   {launches:>8d}")
            print(lines[-1], flush=True)
            worst, rows, spans = row_deviation(x, keys, dev)
            dz.append(f"  {seconds:>4d} s, {len(keys)} key(s): {rows} rows ({spans} span ranges with ids)  max |z_dev - z_host| {worst:.3e}")
            print(dz[-1], flush=True)
    lines += ["  (the host's 600 s cases are the median of 3)" if ARGS.reps > 3 else "", "",
              "dz: |z(device) - z(host fp64)| over every window row and every span row (z, and z_d of the symbols on which both agree)"] + dz
    import test_gpu_watermark_scan as t
    rec = t.recording_a()
    host = t._host_rows(rec, t.RANGES_A, [t.K1, t.K2])
    rows = t._device(rec, t.RANGES_A, [t.K1, t.K2], True)
    worst = 0.0
    lines += ["", "dz over the rows of tests/test_gpu_watermark_scan.py (recording A, its ranges, two keys, with ids):"]
    for i, rng in enumerate(t.RANGES_A):
        for j, key in enumerate((t.K1, t.K2)):
            z, o, symbols = host[i][j]
            worst = max(worst, abs(float(rows[i][j][0]) - z))
            line = f"  range {str(rng):8s} key {key:#10x}  z_dev {rows[i][j][0]:10.6f}  z_host {z:10.6f}  dz {abs(float(rows[i][j][0]) - z):.3e}  symbols"
            for d, (s, zd) in enumerate(symbols):
                s_dev, zd_dev = int(rows[i][j][4 + 2 * d]), float(rows[i][j][5 + 2 * d])
                if int(rows[i][j][1]) == o and s_dev == s:
                    worst = max(worst, abs(zd_dev - zd))
                line += f"  {s_dev}/{s} dz {abs(zd_dev - zd):.3e}"
            lines.append(line)
    lines.append(f"  maximum {worst:.3e}")
    print("\n".join(lines[-2:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {ARGS.out}")


if __name__ == "__main__":
    main()
