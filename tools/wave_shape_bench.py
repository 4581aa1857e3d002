#!/usr/bin/env python3
"""What a per-request formant step costs: `ops.wave_prosody(..., formant=)` (f5hip_wave_prosody_shape) beside the `keep_formants` call on
the same waves in the same run, and beside the host definition `wave_codec.psola_shape_pcm16`.

    python tools/wave_shape_bench.py [--reps 11] [--out profiles/wave_shape_bench.txt]

One request of 10 s and eight, at {"semitones": 0, "formant": 4} and {"semitones": 4, "formant": -2}, no tempo.  The library call alone in
HIP events on PCM that is already on the device (the request tables' copies and their waits included): median and min .. max of `--reps`
after a warm-up call, the `keep_formants` call (pitch +4 kept) measured right beside each shaped call, and their ratio.  The host function
is timed on one request (it is serial: eight cost eight times that).  The device result is compared with the host's before anything is
timed.  Nothing is decided by this file."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_args = argparse.ArgumentParser()
_args.add_argument("--reps", type=int, default=11)
_args.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_shape_bench.txt"))
ARGS = _args.parse_args()
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tts_indic_server_f5_amd import infer, ops, wave_codec  # noqa: E402
_argv, sys.argv = sys.argv, sys.argv[:1]             # (that module parses the command line when it is imported: it gets none of ours)
from wave_formant_bench import _packed, _speech_like  # noqa: E402  (the same speech-like waves as the keep_formants record)
sys.argv = _argv

RATE, SECONDS = 24000, 10
MOVES = ((0, 4), (4, -2))


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
    return statistics.median(out), min(out), max(out)


def main():
    dev = torch.device("cuda:0")
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    emit(f"# tools/wave_shape_bench.py on {torch.cuda.get_device_name(0)} (the name the driver reports; {torch.cuda.get_device_properties(0).gcnArchName}): median ms (min .. max) of {ARGS.reps} after a warm-up call; requests of {SECONDS} s, no tempo")
    emit("# the library call alone in HIP events, PCM on the device; kept = the keep_formants call (pitch +4) on the same waves, measured beside it")
    emit(f"  {'pitch':36s} {'requests':8s} {'shaped call':>28s} {'kept call':>28s}   shaped / kept")
    pcms = [infer.quantise_pcm16(_speech_like(SECONDS * RATE, s)) for s in range(8)]
    for s, f in MOVES:
        for count in (1, 8):
            buf, offsets = _packed(pcms[:count])
            lens, one = [len(x) for x in pcms[:count]], [(1, 1)] * count
            pcm = torch.from_numpy(buf).to(dev)
            shaped = lambda: ops.wave_prosody(pcm, offsets, lens, None, one, [s] * count, formant=[f] * count)   # noqa: E731
            kept = lambda: ops.wave_prosody(pcm, offsets, lens, None, one, [4] * count, keep_formants=[True] * count)   # noqa: E731
            out, _, off2, bounds = shaped()
            down = out.cpu().numpy()
            assert np.array_equal(down[off2[0]:off2[0] + bounds[0]], wave_codec.psola_shape_pcm16(pcms[0], s, f)), "the device call does not equal the host definition"
            a, b = _events(shaped, ARGS.reps), _events(kept, ARGS.reps)
            name = f'{{"semitones": {s}, "formant": {f}}}'
            emit(f"  {name:36s} {count:<8d} {a[0]:9.3f} ({a[1]:.3f} .. {a[2]:.3f}) {b[0]:9.3f} ({b[1]:.3f} .. {b[2]:.3f})   {a[0] / b[0]:.2f}")
    emit()
    emit("the host function wave_codec.psola_shape_pcm16 on one request (numpy, serial), 3 rounds after a warm-up")
    for s, f in MOVES:
        wave_codec.psola_shape_pcm16(pcms[0], s, f)
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            wave_codec.psola_shape_pcm16(pcms[0], s, f)
            ms.append(1e3 * (time.perf_counter() - t0))
        emit(f"  semitones {s:2d}, formant {f:2d}: {statistics.median(ms):9.1f} ms ({min(ms):.1f} .. {max(ms):.1f})")
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"wrote {ARGS.out}")


if __name__ == "__main__":
    main()
