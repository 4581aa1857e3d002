#!/usr/bin/env python3
"""Times the few-tile split-bf16 GEMMs of the flagship call on both gemm3 instances -- 128-row tiles and the thin 32-row tiles -- through
the f5hip_op_gemm unit op (HIP events, 200 launches), forcing the instance with F5HIP_GEMM3_THIN=0|1 (unit op only).  The dispatch rule
(csrc/f5hip.hip kThinMaxTiles128) is read off this table: profiles/thin_tiles_unit_bench.txt.

  python tools/thin_tiles_bench.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tts_indic_server_f5_amd import ops  # noqa: E402

DEV = "cuda:0"
SHAPES = [
    # (what, M, N, K, act, residual)
    ("time MLP (33 points)", 33, 1024, 1024, "silu", False),
    ("proj_out", 2816, 100, 1024, "none", False),
    ("Vocos pwconv2 (937 frames)", 937, 512, 1536, "none", True),
    ("3/4 of a thin round", 1536, 512, 1024, "none", True),
    ("one thin tile per CU", 2048, 512, 1024, "none", True),
    ("text-block pw2", 2816, 512, 1024, "none", True),
    ("Vocos pwconv1 (937 frames)", 937, 1536, 512, "gelu_erf", False),
    ("one 128-row tile per 2 CUs", 2048, 1024, 1024, "none", False),
    ("text-block pw1", 2816, 1024, 512, "gelu_erf", False),
    ("input projection", 2816, 1024, 640, "none", False),
]


def time_one(M, N, K, act, res, thin):
    g = torch.Generator().manual_seed(1)
    a = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    r = torch.randn(M, N, generator=g).to(DEV) if res else None
    os.environ["F5HIP_GEMM3_THIN"] = "1" if thin else "0"
    try:
        _, us = ops.gemm(a, w, torch.zeros(N), prec=2, act=act, res=r, iters=200)
    finally:
        del os.environ["F5HIP_GEMM3_THIN"]
    return us


def main():
    print(f"{'shape':30s} {'M':>5s} {'N':>5s} {'K':>5s}  tiles128  thin WGs   128-row us (2 runs)    thin us (2 runs)   thin / 128-row")
    for what, M, N, K, act, res in SHAPES:
        t128 = -(-M // 128) * -(-N // 128)
        tthin = -(-M // 32) * -(-N // 128)
        us = {0: [], 1: []}
        for _ in range(2):   # alternating, so a clock or cache drift shows as a spread inside a column
            for thin in (0, 1):
                us[thin].append(time_one(M, N, K, act, res, thin))
        print(f"{what:30s} {M:5d} {N:5d} {K:5d}  {t128:8d}  {tthin:8d}   {us[0][0]:8.2f} {us[0][1]:8.2f}      {us[1][0]:8.2f} {us[1][1]:8.2f}"
              f"       {min(us[1]) / min(us[0]):.3f}", flush=True)


if __name__ == "__main__":
    main()
