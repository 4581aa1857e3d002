"""Times one sampler call with per-unit time grids (f5hip_cfm_sample_grids) at F5-Base width: 8 units of 1 350-1 440 frames, Euler, CFG 2.

  a  4 units at 32 NFE + 4 at 16 NFE: one grids call vs the two per-grid calls a server without per-unit grids makes
  b  all 32 NFE, half at sway -1 and half at sway 0: one grids call vs two calls
  c  one grid for all 8 units (32 NFE, sway -1) through the old entry point (scalar knobs) and through the new one (per-unit lists)

Each row gives the backbone rows of one forward with every unit laid out, the summed rows of the call's forwards (counter "dit_rows") and
the median device-synchronised wall time; the forms of a row are timed in alternation, `--reps` rounds after one warm-up round.

    python tools/mixed_grids_bench.py [--reps 3] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tts_indic_server_f5_amd import _lib, synth  # noqa: E402
from tts_indic_server_f5_amd.model import F5TTS_BASE, F5HipModel, unit_duration  # noqa: E402

FRAMES = [1380, 1420, 1400, 1350, 1440, 1390, 1410, 1370]
PROMPT, N_TEXT = 300, 220


def units(seed=3):
    g = torch.Generator().manual_seed(seed)
    out = []
    for f in FRAMES:
        cond = torch.randn(PROMPT, 100, generator=g)
        text = torch.randint(1, 2545, (N_TEXT,), generator=g)
        out.append((cond, text, f, torch.randn(unit_duration(PROMPT, N_TEXT, f), 100, generator=g)))
    return out


def call(model, us, steps, sway):
    conds = torch.stack([u[0] for u in us])
    texts = torch.stack([u[1] for u in us])
    out, _ = model.sample(conds, texts, torch.tensor([u[2] for u in us]), y0=[u[3] for u in us], steps=steps, cfg_strength=2.0,
                          sway_sampling_coef=sway)
    return out


def counter(name):
    v = C.c_int64()
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def timed_rounds(fns, reps):
    """fns: {name: fn}; one warm-up round, then `reps` rounds that run every form once, in alternation.  -> {name: (median s, [s], dit_rows)}"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    rows = {}
    for _ in range(reps):
        for k, fn in fns.items():
            _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t0)
            rows[k] = counter("dit_rows")
    return {k: (statistics.median(v), v, rows[k]) for k, v in ts.items()}


def layout_rows(us):
    return sum((unit_duration(PROMPT, N_TEXT, u[2]) + 127) // 128 * 128 * 2 for u in us)   # CFG 2: two sequences per unit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    model = F5HipModel(F5TTS_BASE, synth.dit_state_dict(), attn_shape_invariant=True)
    us = units()
    fast, slow = us[1::2], us[0::2]
    ordered = [u for pair in zip(slow, fast) for u in pair]   # units 0, 2, 4, 6 at 32 NFE; 1, 3, 5, 7 at 16 NFE
    steps_a = [32, 16] * 4
    sway_b = [-1.0, 0.0] * 4
    lines = [f"F5-Base width (dim 1024, depth 22), {len(us)} units of {min(FRAMES)}-{max(FRAMES)} frames (prompt {PROMPT}), Euler, CFG 2, "
             f"shape-invariant attention; median of {a.reps} alternating rounds after 1 warm-up round, device-synchronised wall clock",
             f"rows of one forward with all 8 units laid out: {layout_rows(us)}", ""]

    def row(tag, label, res, key):
        t, ts, r = res[key]
        lines.append(f"{tag} {label:<38s}: dit_rows {r:7d}  {t * 1e3:8.1f} ms  ({', '.join(f'{x * 1e3:.1f}' for x in ts)})")

    ra = timed_rounds({"grids": lambda: call(model, ordered, steps_a, -1.0),
                       "two": lambda: (call(model, slow, 32, -1.0), call(model, fast, 16, -1.0))}, a.reps)
    row("a", "32 + 16 NFE, one grids call", ra, "grids")
    row("a", "32 + 16 NFE, two calls (per grid)", ra, "two")
    lines.append(f"a one call vs two: time {100 * (ra['grids'][0] / ra['two'][0] - 1):+.1f} %")
    rb = timed_rounds({"grids": lambda: call(model, ordered, 32, sway_b),
                       "two": lambda: (call(model, slow, 32, -1.0), call(model, fast, 32, 0.0))}, a.reps)
    row("b", "32 NFE, sway -1 / 0, one grids call", rb, "grids")
    row("b", "32 NFE, sway -1 / 0, two calls", rb, "two")
    lines.append(f"b one call vs two: time {100 * (rb['grids'][0] / rb['two'][0] - 1):+.1f} %")
    rc = timed_rounds({"old": lambda: call(model, us, 32, -1.0), "new": lambda: call(model, us, [32] * 8, [-1.0] * 8)}, a.reps)
    row("c", "one grid, scalar knobs (old entry)", rc, "old")
    row("c", "one grid, per-unit lists (new entry)", rc, "new")
    lines.append(f"c new vs old: time {100 * (rc['new'][0] / rc['old'][0] - 1):+.1f} %")
    # the grids call gives every unit what its own grid's call gives it (the GEMM dispatch may differ with the rows: rounding, not bits)
    og, o32, o16 = call(model, ordered, steps_a, -1.0), call(model, slow, 32, -1.0), call(model, fast, 16, -1.0)
    d = 0.0
    for i in range(4):
        n, m = unit_duration(PROMPT, N_TEXT, slow[i][2]), unit_duration(PROMPT, N_TEXT, fast[i][2])
        d = max(d, (og[2 * i, :n] - o32[i, :n]).abs().max().item(), (og[2 * i + 1, :m] - o16[i, :m]).abs().max().item())
    lines.append(f"a: max |grids call - per-grid calls| over all units: {d:.3e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
