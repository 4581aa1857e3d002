#!/usr/bin/env python3
"""What measuring an uploaded reference clip costs where its two buffers already lie on the device (behind `ops.ref_frontend`): the host
definition against the device call, in the same run.

    python tools/ref_assess_bench.py [--reps 9] [--out profiles/ref_assess_bench.txt]

Shapes: one 15 s clip, and eight 15 s clips; raw 44.1 kHz stereo, hard-clipped noisy speech-like content (tests/denoise_ref.py), prepared by
the host front-end (mono mix, sinc resampling to 24 kHz).
  host    one download of the two packed buffers, `audio_prep.assess_reference` clip by clip: what a host report behind the device
          front-end would do
  device  `ops.ref_assess`: ONE f5hip_ref_assess call (six launches) and the download of the rows
Wall clock (`time.perf_counter`) with a device synchronisation before and after each side, the two sides alternating in one process, the median
and min..max of `--reps` after a warm-up round.  The first round also compares the two: counts and peak must be equal, and the float measures'
greatest difference is printed.  What is measured is reported; no ratio is promised, and nothing is decided by these figures."""
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
from tts_indic_server_f5_amd import audio_prep, infer, ops  # noqa: E402

SR = 44100


def _fmt(ts):
    return f"{statistics.median(ts):9.3f} ms  ({min(ts):.3f} .. {max(ts):.3f})"


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _clip(seconds, seed):
    x = R.noisy_speech(int(seconds * R.RATE), seed)[1]
    x = np.interp(np.arange(int(seconds * SR)) * (R.RATE / SR), np.arange(len(x)), x)
    raw = np.stack([np.clip(4.0 * x, -1.0, 1.0), np.clip(3.6 * x, -1.0, 1.0)]).astype(np.float32)
    prepared = infer.resample_sinc_hann(torch.from_numpy(raw).mean(dim=0, keepdim=True), SR, infer.target_sample_rate)[0].numpy()
    return raw, prepared


def shape(label, clips, reps, emit):
    raws, waves = [r for r, _ in clips], [w for _, w in clips]
    sizes, lengths = [r.size for r in raws], [len(w) for w in waves]
    raw_at = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    at = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
    raw_dev = torch.from_numpy(np.concatenate([r.reshape(-1) for r in raws])).to("cuda")
    wave_dev = torch.from_numpy(np.concatenate(waves)).to("cuda")
    ch, raw_len = [r.shape[0] for r in raws], [r.shape[1] for r in raws]

    def host():
        a, b = raw_dev.cpu().numpy(), wave_dev.cpu().numpy()
        return [audio_prep.assess_reference(a[o:o + s].reshape(c, -1), SR, b[p:p + n]) for o, s, c, p, n in zip(raw_at, sizes, ch, at, lengths)]

    def device():
        rows = ops.ref_assess(raw_dev, raw_at, ch, raw_len, wave_dev, at, lengths).cpu().numpy()
        return [audio_prep.report_from_row(row, n / SR, None, s) for row, n, s in zip(rows, raw_len, sizes)]

    times = {"host": [], "device": []}
    for rep in range(reps + 1):                                  # the first round warms both up (workspace, tables, allocator)
        t_h, out_h = _timed(host)
        t_d, out_d = _timed(device)
        if rep:
            times["host"].append(t_h)
            times["device"].append(t_d)
            continue
        assert all((h.peak, h.clipped) == (d.peak, d.clipped) for h, d in zip(out_h, out_d)), "counts or peak differ"
        diff = {k: max(abs(getattr(h, k) - getattr(d, k)) for h, d in zip(out_h, out_d)) for k in ("noise_db", "snr_db", "speech_ratio", "bandwidth_hz")}
        emit(f"{label}: {len(clips)} x {raw_len[0] / SR:g} s, raw {SR} Hz x {ch[0]} channels; peak and clipped equal (clipped {[d.clipped for d in out_d][:2]} ...); "
             f"max |device - host|: " + ", ".join(f"{k} {v:.3g}" for k, v in diff.items()))
    emit(f"  host    (download, assess_reference per clip)        {_fmt(times['host'])}")
    emit(f"  device  (ops.ref_assess, 6 launches, rows downloaded) {_fmt(times['device'])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"ref_assess_bench: {torch.cuda.get_device_name(0)}; wall clock with a device sync, median (min .. max) of {args.reps} after one warm-up round")
    one = [_clip(15.0, 51)]
    shape("one clip", one, args.reps, emit)
    shape("eight clips", one + [_clip(15.0, 52 + i) for i in range(7)], args.reps, emit)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
