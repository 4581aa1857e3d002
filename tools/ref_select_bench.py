#!/usr/bin/env python3
"""What finding the cleanest stretch of a long recording costs: the host definition against the device call, in the same run, from the
samples on the host to the window table on the host.

    python tools/ref_select_bench.py [--reps 5] [--out profiles/ref_select_bench.txt]

Shapes: 60 s and 600 s of mono 24 kHz noisy speech-like content (tests/denoise_ref.py, a minute of it repeated under fresh noise), one
recording and four; 12 s windows (1125 frames) at the default hop.
  host    `audio_prep.select_table` recording by recording, ONE round (it takes seconds to minutes)
  device  upload of the samples, `ops.ref_select` (ONE f5hip_ref_select call, ten launches), download of the rows and the choices
Wall clock (`time.perf_counter`) with a device synchronisation before and after; the device side is the median and min..max of `--reps`
after a warm-up round.  The first round also compares the two: clipped equal, the chosen windows equal, the greatest difference of snr_db
printed.  Then one device call under torch.profiler: each kernel's share of the call's kernel time, rs_window_floor_kernel's first.  What is
measured is reported; no ratio is promised, and nothing is decided by these figures."""
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

import denoise_ref as R  # noqa: E402
from tts_indic_server_f5_amd import audio_prep, ops  # noqa: E402

W = audio_prep.select_window_frames(12.0)


def _fmt(ts):
    return f"{statistics.median(ts):10.3f} ms  ({min(ts):.3f} .. {max(ts):.3f})"


def _recording(seconds, seed):
    minute = R.speechlike(60 * R.RATE, seed)
    s = np.tile(minute, -(-seconds // 60))[:seconds * R.RATE]
    level = np.mean(minute * minute) / 10.0 ** (np.linspace(5.0, 30.0, len(s)) / 10.0)
    return (s + np.random.default_rng(seed + 1).standard_normal(len(s)) * np.sqrt(level)).astype(np.float32)


def _device(recs):
    lens = [len(x) for x in recs]
    at = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    wave = torch.from_numpy(np.concatenate(recs)).to("cuda")
    tables, choices = ops.ref_select([ops.RefSelectClip(wave, o, 1, n, 24000, wave, o, n) for o, n in zip(at, lens)], W)
    return [ops.ref_select_table(t) for t in tables], choices.cpu().numpy()


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _kernel_shares(recs, emit):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            _device(recs)
            torch.cuda.synchronize()
        kernels = {}
        for e in prof.events():
            if e.device_time_total > 0 and ("_kernel" in e.name):
                kernels[e.name.split("(")[0]] = kernels.get(e.name.split("(")[0], 0.0) + e.device_time_total
        total = sum(kernels.values())
        assert total > 0
        for name, us in sorted(kernels.items(), key=lambda kv: (not kv[0].startswith("rs_window_floor"), -kv[1])):
            emit(f"    {name:<28s} {us / 1e3:9.3f} ms  {100.0 * us / total:5.1f} % of the call's kernel time")
    except Exception as e:                                       # noqa: BLE001  (the profiler is a tool of this report, not of the call)
        emit(f"    kernel shares not measured: {type(e).__name__}: {e}")


def shape(label, recs, reps, emit):
    t_h, host = _timed(lambda: [audio_prep.select_table(x[None], 24000, x, W) for x in recs])
    times = []
    for rep in range(reps + 1):                                  # the first round warms up (workspace, tables, allocator)
        t_d, (tables, choices) = _timed(lambda: _device(recs))
        if rep:
            times.append(t_d)
            continue
        frames = [[f for _, f in audio_prep.select_windows(audio_prep.denoise_frames(len(x)), W)] for x in recs]
        assert all(np.array_equal(h[:, 0], d[:, 0]) for h, d in zip(host, tables)), "clipped differs"
        assert [audio_prep.select_choice(h, f) for h, f in zip(host, frames)] == choices.tolist(), "the chosen windows differ"
        diff = max(float(np.max(np.abs(h[:, 4] - d[:, 4]))) for h, d in zip(host, tables))
        emit(f"{label}: {len(recs)} x {len(recs[0]) / 24000:g} s mono 24 kHz, {sum(len(h) for h in host)} windows of {W} frames; clipped and the chosen windows "
             f"{choices.tolist()} equal; max |device - host| snr_db {diff:.3g} dB")
    emit(f"  host    (select_table per recording, one round)             {t_h:10.3f} ms")
    emit(f"  device  (upload, ops.ref_select, 10 launches, rows downloaded) {_fmt(times)}")
    _kernel_shares(recs, emit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"ref_select_bench: {torch.cuda.get_device_name(0)}; wall clock with a device sync; device: median (min .. max) of {args.reps} after one warm-up round")
    for seconds in (60, 600):
        recs = [_recording(seconds, 70 + i) for i in range(4)]
        shape(f"one recording of {seconds} s", recs[:1], args.reps, emit)
        shape(f"four recordings of {seconds} s", recs, args.reps, emit)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
