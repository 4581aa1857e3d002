#!/usr/bin/env python3
"""What denoising an uploaded reference clip costs where the clip already lies on the device (behind `ops.ref_frontend`): the host function
against the device call, in the same run.

    python tools/ref_denoise_bench.py [--reps 11] [--out profiles/ref_denoise_bench.txt]

Shapes: one 10 s clip, and eight 15 s clips, mono at 24 kHz (noisy speech-like content, tests/denoise_ref.py).
  host    one download of the packed clips, `audio_prep.denoise_reference` clip by clip, one upload: what a host denoiser in the middle of
          the device chain would do
  device  `ops.ref_denoise`: ONE f5hip_ref_denoise call (four launches) in place; nothing crosses the bus but the clip table
HIP events around each side (the host side's events enclose its CPU work), the two sides alternating in one process, median and min..max of
`--reps` (at least 10) after a warm-up; the device call's time per launch is its time over its four launches.  The first repetition also
measures parity: the device result against the float64 definition, beside the float32 run of tests/denoise_ref.py on the same clip.
Nothing is decided by these figures: the option is off unless a voice asks for it."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import denoise_ref as R  # noqa: E402
from tts_indic_server_f5_amd import audio_prep, ops  # noqa: E402


def _fmt(ts):
    return f"{statistics.median(ts):9.3f} ms  ({min(ts):.3f} .. {max(ts):.3f})"


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def shape(label, clips, reps, emit):
    lengths = [len(c) for c in clips]
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
    packed_host = torch.from_numpy(np.concatenate(clips))

    def host(dev):
        x = dev.cpu().numpy()
        y = np.concatenate([audio_prep.denoise_reference(x[o:o + n]) for o, n in zip(offsets, lengths)])
        return torch.from_numpy(y).to(dev.device)

    times = {"host": [], "device": []}
    for rep in range(reps + 1):                                  # the first round warms both up (workspace, tables, allocator)
        dev_h, dev_d = packed_host.to("cuda"), packed_host.to("cuda")
        torch.cuda.synchronize()
        t_h, out_h = _timed(lambda: host(dev_h))
        t_d, out_d = _timed(lambda: ops.ref_denoise(dev_d, offsets, lengths))
        if rep:
            times["host"].append(t_h)
            times["device"].append(t_d)
        else:
            got = out_d.cpu().numpy()
            errs, errs32 = [], []
            for o, n, c in zip(offsets, lengths, clips):
                want = R.denoise(c.astype(np.float64), np.float64)
                errs.append(float(np.abs(got[o:o + n] - want).max()))
                errs32.append(float(np.abs(R.denoise(c, np.float32) - want).max()))
            assert np.array_equal(out_h.cpu().numpy(), np.concatenate([audio_prep.denoise_reference(c) for c in clips]))
    emit(f"  {label}:")
    emit(f"    host    download, denoise_reference clip by clip, upload  {_fmt(times['host'])}")
    emit(f"    device  ops.ref_denoise, in place, four launches          {_fmt(times['device'])}   ({statistics.median(times['device']) / 4:.3f} ms per launch)")
    emit(f"    parity  device vs float64 definition: max |err| {max(errs):.3e}; float32 run of the restatement: {max(errs32):.3e} "
         f"(16 x = {16 * max(errs32):.3e})")
    return statistics.median(times["host"]), statistics.median(times["device"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_denoise_bench.txt"))
    args = ap.parse_args()
    reps = max(args.reps, 10)
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    assert torch.cuda.is_available(), "needs a HIP device"
    emit(f"tools/ref_denoise_bench.py: median (min .. max) of {reps} event-timed runs after a warm-up")
    emit(f"device {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}")
    for label, clips in (("one clip, 10 s", [R.clip(10 * R.RATE, 1)]), ("eight clips, 15 s each", [R.clip(15 * R.RATE, 10 + i) for i in range(8)])):
        h, d = shape(label, clips, reps, emit)
        emit(f"    the device call takes {d / h:.3f} of the host path's time ({h / d:.1f} x)")
    emit("nothing is decided by these figures: denoise is per voice and off unless asked for")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
