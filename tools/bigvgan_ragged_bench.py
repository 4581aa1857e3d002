#!/usr/bin/env python3
"""BigVGAN over the chunks of a served batch: (a) one `vocoder(mel)` per chunk, the loop `infer._chunk_waves` ran before the ragged call
existed, (b) ONE `decode_ragged` call on the same mels (f5hip_bigvgan_forward_ragged, the slab copy and the table upload included), and, for
equal lengths, (c) the uniform batched `vocoder(mel[n])`.  Full bigvgan_v2_24khz_100band_256x geometry, seeded random weights, the parity
operand mode; n = 1, 2, 4, 8, 16 chunks, all of 10 s or drawn from U(6 s, 14 s) (the README's sampler mix).

    python tools/bigvgan_ragged_bench.py [--repeats 7] [--planes 2]

Per row: 2 warm-up calls of every case at the timed shapes, then `repeats` rounds in which the cases alternate, each call between two
device events; median and [min .. max] in ms.  The verdict column compares (b)'s median with (a)'s: "slower" only when it exceeds (a)'s
median by more than (a)'s own min-to-max spread."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tts_indic_server_f5_amd import synth
from tts_indic_server_f5_amd.vocoder import F5HipBigVGAN

FRAMES_PER_S = 24000 / 256


def timed(fns, repeats):
    """The cases `fns` with their repeats interleaved (a, b, c, a, b, c, ...), so that drift and other load meet all of them alike"""
    for fn in fns:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def fmt(r):
    return f"{r[0]:8.2f} [{r[1]:7.2f} .. {r[2]:7.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--planes", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bigvgan_ragged_bench: no HIP device (nothing is measured without one)")
    voc = F5HipBigVGAN(synth.bigvgan_state_dict(), gemm_planes=args.planes)
    print(f"# {torch.cuda.get_device_name(0)}  gemm_planes {args.planes}  repeats {args.repeats}  ms per call: median [min .. max]")
    print(f"# {'mix':8s} {'n':>2s} {'frames':>6s}  {'(a) per-chunk loop':>30s}  {'(b) one ragged call':>30s}  {'(c) uniform batch':>30s}  (a)/(b)  verdict")
    rng = np.random.default_rng(2024)
    g = torch.Generator().manual_seed(7)
    for mix in ("equal", "U(6,14)s"):
        for n in (1, 2, 4, 8, 16):
            secs = np.full(n, 10.0) if mix == "equal" else rng.uniform(6.0, 14.0, n)
            frames = [int(round(s * FRAMES_PER_S)) for s in secs]
            mels = [(torch.randn(100, t, generator=g) * 1.5 - 1.0).cuda() for t in frames]
            fns = [lambda: [voc(m[None]) for m in mels], lambda: voc.decode_ragged(mels)]
            if mix == "equal":
                batch = torch.stack(mels)
                fns.append(lambda: voc(batch))
            a, b, c = (timed(fns, args.repeats) + [None])[:3]
            verdict = "slower" if b[0] > a[0] + (a[2] - a[1]) else ("faster" if b[0] < a[0] - (a[2] - a[1]) else "same")
            print(f"  {mix:8s} {n:2d} {sum(frames):6d}  {fmt(a):>30s}  {fmt(b):>30s}  {fmt(c) if c else '-':>30s}  {a[0] / b[0]:7.3f}  {verdict}", flush=True)


if __name__ == "__main__":
    main()
