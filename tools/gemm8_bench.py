"""MXFP8 block GEMMs (gemm_planes / prec 4, csrc/gemm8.h) against the fp16 path (prec 3), on the GPU.

Per block-GEMM shape (out, FF1, FF2 of F5-Base) at M = 2808 (one utterance, both CFG branches) and M = 22528 (the C3 share): f5hip_op_gemm
timed with HIP events over `--iters` launches that cycle through a pool of weight copies larger than the Infinity Cache (HBM-cold weights,
as in the forward), prec 3 and prec 4 alternating in one process, `--reps` times each.  Then one whole sampler call (F5-Base, 8 x 1404
frames, CFG 2) in modes 3 and 4, alternating.  Writes profiles/gemm8_bench.txt."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("out", 1024, 1024, dict(mul=True, res=True)), ("FF1", 2048, 1024, dict(act="gelu_tanh", out16=True)), ("FF2", 1024, 2048, dict(mul=True, res=True))]
POOL_BYTES = 320 << 20   # > 256 MiB of Infinity Cache


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--modes", default="3,4", help="comma-separated: a tree without mode 4 can be timed with --modes 3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm8_bench.txt"))
    a = ap.parse_args()
    from tts_indic_server_f5_amd import ops, synth
    from tts_indic_server_f5_amd.model import F5TTS_BASE, F5HipModel
    assert torch.cuda.is_available(), "gemm8_bench needs the GPU: there is no CPU timing"
    modes = [int(m) for m in a.modes.split(",")]
    dev, lines = "cuda:0", [f"# tools/gemm8_bench.py --iters {a.iters} --reps {a.reps} --steps {a.steps} --modes {a.modes}; {torch.cuda.get_device_name(0)}",
                            "# avg us per launch over HBM-cold weight copies; prec 3 = fp16 (gemm5 / gemm6), prec 4 = MXFP8 (gemm8); best of the reps, all reps listed"]
    g = torch.Generator().manual_seed(1)
    for M in (2808, 22528):
        for name, N, K, kw in SHAPES:
            x, w = torch.randn(M, K, generator=g).to(dev), (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
            extra = dict(act=kw.get("act", "none"), out16=kw.get("out16", False), bias=torch.zeros(N),
                         mul=torch.ones(N) if kw.get("mul") else None, res=torch.zeros(M, N) if kw.get("res") else None)
            bias = extra.pop("bias")
            copies = max(2, POOL_BYTES // (N * K * 2))
            t = {p: [] for p in modes}
            for _ in range(a.reps):
                for p in modes:
                    t[p].append(ops.gemm(x, w, bias, prec=p, w_copies=copies, iters=a.iters, **extra)[1])
            line = f"{name:4s} M {M:6d} N {N:5d} K {K:5d} copies {copies:4d}: " + "  ".join(f"prec {p} {min(t[p]):8.2f} us {['%.2f' % v for v in t[p]]}" for p in modes)
            if 3 in t and 4 in t:
                line += f"  prec4 / prec3 = {min(t[4]) / min(t[3]):.3f}"
            print(line, flush=True)
            lines.append(line)
    sd = synth.dit_state_dict()
    gc = torch.Generator().manual_seed(14)
    cond, text = torch.randn(1, 469, 100, generator=gc).expand(8, -1, -1), synth.text_ids().expand(8, -1)
    models = {p: F5HipModel(F5TTS_BASE, sd, gemm_planes=p) for p in modes}
    t = {p: [] for p in modes}
    for rep in range(a.reps + 1):       # the first round warms up
        for p in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            models[p].sample(cond, text, 1404, steps=a.steps, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
            torch.cuda.synchronize()
            if rep:
                t[p].append((time.perf_counter() - t0) * 1e3)
    line = f"sampler call, F5-Base, 8 x 1404 frames (22528 rows), {a.steps} NFE, host clock around a synchronised call: " + \
           "  ".join(f"mode {p} {min(t[p]):8.1f} ms {['%.1f' % v for v in t[p]]}" for p in modes)
    print(line, flush=True)
    lines.append(line)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
