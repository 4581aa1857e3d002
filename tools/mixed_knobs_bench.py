"""Times one sampler call with per-unit CFG strengths (f5hip_cfm_sample_units) at F5-Base width: 8 units of ~1 400 frames, 32 NFE, Euler.

  A  all 8 units at CFG 2 (one scalar strength: f5hip_cfm_sample_masked)
  B  the same units, half at CFG 2 and half at CFG 0 (per-unit strengths): the CFG-0 units run no unconditional rows
  C  B's two halves as two separate calls (what a server without per-unit strengths would have to do)

Prints the rows each call lays out and the median wall time of `--reps` calls after one warm-up call.

    python tools/mixed_knobs_bench.py [--reps 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tts_indic_server_f5_amd import synth  # noqa: E402
from tts_indic_server_f5_amd.model import F5TTS_BASE, F5HipModel, unit_duration  # noqa: E402

FRAMES = [1380, 1420, 1400, 1350, 1440, 1390, 1410, 1370]
PROMPT, N_TEXT, STEPS = 300, 220, 32


def units(seed=3):
    g = torch.Generator().manual_seed(seed)
    out = []
    for f in FRAMES:
        cond = torch.randn(PROMPT, 100, generator=g)
        text = torch.randint(1, 2545, (N_TEXT,), generator=g)
        out.append((cond, text, f, torch.randn(unit_duration(PROMPT, N_TEXT, f), 100, generator=g)))
    return out


def call(model, us, cfg):
    conds = torch.stack([u[0] for u in us])
    texts = torch.stack([u[1] for u in us])
    out, _ = model.sample(conds, texts, torch.tensor([u[2] for u in us]), y0=[u[3] for u in us], steps=STEPS, cfg_strength=cfg,
                          sway_sampling_coef=-1.0)
    return out


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def rows(us, cfgs):
    # every sequence is padded to a multiple of 128 rows; a unit with CFG >= 1e-5 lays out two sequences
    return sum(((unit_duration(PROMPT, N_TEXT, u[2]) + 127) // 128 * 128) * (2 if c >= 1e-5 else 1) for u, c in zip(us, cfgs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    model = F5HipModel(F5TTS_BASE, synth.dit_state_dict(), attn_shape_invariant=True)
    us = units()
    mixed = [2.0, 0.0] * 4
    lines = [f"F5-Base width (dim 1024, depth 22), {len(us)} units of {min(FRAMES)}-{max(FRAMES)} frames (prompt {PROMPT}), "
             f"{STEPS} NFE Euler, shape-invariant attention, median of {a.reps} calls after 1 warm-up"]
    ta, sa = timed(lambda: call(model, us, 2.0), a.reps)
    tb, sb = timed(lambda: call(model, us, mixed), a.reps)
    half2, half0 = us[0::2], us[1::2]
    tc, sc = timed(lambda: (call(model, half2, 2.0), call(model, half0, 0.0)), a.reps)
    ra, rb = rows(us, [2.0] * 8), rows(us, mixed)
    lines.append(f"A all CFG 2, one call           : rows {ra:6d}  {ta * 1e3:8.1f} ms  (calls {', '.join(f'{t * 1e3:.1f}' for t in sa)})")
    lines.append(f"B half CFG 2 / half CFG 0, mixed: rows {rb:6d}  {tb * 1e3:8.1f} ms  (calls {', '.join(f'{t * 1e3:.1f}' for t in sb)})")
    lines.append(f"C B's halves as two calls       : rows {rb:6d}  {tc * 1e3:8.1f} ms  (pairs {', '.join(f'{t * 1e3:.1f}' for t in sc)})")
    lines.append(f"B vs A: rows -{100 * (1 - rb / ra):.1f} %, time -{100 * (1 - tb / ta):.1f} %;  B vs C: time -{100 * (1 - tb / tc):.1f} %")
    # the mixed call gives each unit what its own-strength call gives it
    ob, o2, o0 = call(model, us, mixed), call(model, half2, 2.0), call(model, half0, 0.0)
    same = all(torch.equal(ob[2 * i, :n], o2[i, :n]) and torch.equal(ob[2 * i + 1, :m], o0[i, :m])
               for i, (n, m) in enumerate(zip([unit_duration(PROMPT, N_TEXT, u[2]) for u in half2],
                                              [unit_duration(PROMPT, N_TEXT, u[2]) for u in half0])))
    lines.append(f"B's units equal C's, bit for bit: {same}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
