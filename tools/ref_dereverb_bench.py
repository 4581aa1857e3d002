#!/usr/bin/env python3
"""What dereverberating an uploaded reference clip costs: the host definition against the device call, in the same run, from host samples
to host samples.

    python tools/ref_dereverb_bench.py [--reps 11] [--out profiles/ref_dereverb_bench.txt]
    python tools/ref_dereverb_bench.py --calls 20        # device calls only, nothing timed or written: the run a kernel profiler wraps

Shapes: one 10 s clip, and eight 10 s clips, mono at 24 kHz (reverberant speech-like hosts, tests/dereverb_ref.py, T60 0.3 s).
  host    `audio_prep.dereverb_reference` clip by clip on the host samples
  device  upload of the packed clips, `ops.ref_dereverb` (ONE f5hip_ref_dereverb call, four launches, in place), download
A host clock around each side, the device side ending in its download (a synchronising copy), the two sides alternating in one process,
median and min..max of `--reps` (at least 10) after a warm-up.  The first repetition also measures parity: the device result against the
float64 definition.  Nothing is decided by these figures: the option is off unless a voice asks for it."""
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

import dereverb_ref as R  # noqa: E402
from tts_indic_server_f5_amd import audio_prep, ops  # noqa: E402


def _fmt(ts):
    return f"{statistics.median(ts):9.3f} ms  ({min(ts):.3f} .. {max(ts):.3f})"


def _clips(count):
    return [R.host(10.0, 0.3, 40 + i)[0].astype(np.float32) for i in range(count)]


def _table(clips):
    lengths = [len(c) for c in clips]
    return np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist(), lengths


def shape(label, clips, reps, emit):
    offsets, lengths = _table(clips)
    packed = torch.from_numpy(np.concatenate(clips)).pin_memory()

    def device():
        return ops.ref_dereverb(packed.to("cuda", non_blocking=True), offsets, lengths).cpu().numpy()

    times = {"host": [], "device": []}
    for rep in range(reps + 1):                                  # the first round warms both up (workspace, tables, allocator)
        t0 = time.perf_counter()
        out_h = [audio_prep.dereverb_reference(c) for c in clips]
        t1 = time.perf_counter()
        out_d = device()
        t2 = time.perf_counter()
        if rep:
            times["host"].append(1e3 * (t1 - t0))
            times["device"].append(1e3 * (t2 - t1))
        else:
            want = audio_prep.dereverb_reference_f64(clips[0])
            err, err_h = float(np.abs(out_d[:lengths[0]] - want).max()), float(np.abs(out_h[0] - want).max())
    emit(f"  {label}:")
    emit(f"    host    dereverb_reference clip by clip                     {_fmt(times['host'])}")
    emit(f"    device  upload, ops.ref_dereverb (four launches), download  {_fmt(times['device'])}")
    emit(f"    parity  first clip (peak {np.abs(clips[0]).max():.2f}), device vs float64 definition: max |err| {err:.3e}; the host function's own rounding: {err_h:.3e}")
    return statistics.median(times["host"]), statistics.median(times["device"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_dereverb_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    if args.calls:
        clips = _clips(8)
        offsets, lengths = _table(clips)
        wave = torch.from_numpy(np.concatenate(clips)).to("cuda")
        for _ in range(args.calls):
            ops.ref_dereverb(wave.clone(), offsets, lengths)
        torch.cuda.synchronize()
        return
    reps = max(args.reps, 10)
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    emit(f"tools/ref_dereverb_bench.py: median (min .. max) of {reps} host-clocked runs after a warm-up, host samples to host samples")
    emit(f"device {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}")
    for label, clips in (("one clip, 10 s", _clips(1)), ("eight clips, 10 s each", _clips(8))):
        h, d = shape(label, clips, reps, emit)
        emit(f"    the device path takes {d / h:.4f} of the host path's time ({h / d:.0f} x)")
    emit("nothing is decided by these figures: dereverb is per voice and off unless asked for")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
