"""Times one sampler call whose units use different ODE methods (f5hip_cfm_sample_methods) at F5-Base width: 8 units of 1 350-1 440
frames, CFG 2, sway -1, at equal backbone forwards -- 4 units Euler at 32 steps, 2 midpoint at 16, 2 RK4 at 8 (32 forwards each).

  mixed   ONE call on a Euler handle, `sample(..., ode_method=[...])`
  three   the three one-method calls over the same units through the existing entry points, the handle switched with
          f5hip_dit_set_ode_method in between (the baseline: the path a server without per-unit methods takes, given one handle)

Each row gives the summed backbone rows of the call's forwards (counter "dit_rows"), the kernel launches by class (a profiled run outside
the timing) and the median device-synchronised wall time; the forms are timed in alternation, `--reps` rounds after one warm-up round.

    python tools/mixed_methods_bench.py [--reps 3] [--out FILE]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mixed_grids_bench import FRAMES, N_TEXT, PROMPT, timed_rounds, units  # noqa: E402
from tts_indic_server_f5_amd import _lib, synth  # noqa: E402
from tts_indic_server_f5_amd.model import _ODE_METHODS, F5TTS_BASE, F5HipModel, unit_duration  # noqa: E402

METHODS = ["euler"] * 4 + ["midpoint"] * 2 + ["rk4"] * 2
STEPS = [32] * 4 + [16] * 2 + [8] * 2


def call(model, us, steps, **kw):
    conds = torch.stack([u[0] for u in us])
    texts = torch.stack([u[1] for u in us])
    out, _ = model.sample(conds, texts, torch.tensor([u[2] for u in us]), y0=[u[3] for u in us], steps=steps, cfg_strength=2.0,
                          sway_sampling_coef=-1.0, **kw)
    return out


def set_method(model, name):
    """The handle's own solver, as F5HipModel's constructor sets it"""
    _lib.check(_lib.lib().f5hip_dit_set_ode_method(model._h, _ODE_METHODS[name]), "f5hip_dit_set_ode_method")
    model.odeint_kwargs = dict(method=name)


def three_calls(model, us):
    outs = []
    for name, lo, hi in (("euler", 0, 4), ("midpoint", 4, 6), ("rk4", 6, 8)):
        set_method(model, name)
        outs.append(call(model, us[lo:hi], STEPS[lo]))
    set_method(model, "euler")
    return outs


def launches(model, fn):
    """Kernel launches of fn() by class, from a profiled run"""
    model.set_profiling(True)
    before = model.get_profile()
    fn()
    torch.cuda.synchronize()
    after = model.get_profile()
    model.set_profiling(False)
    return {k: after[k]["launches"] - before[k]["launches"] for k in after}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    model = F5HipModel(F5TTS_BASE, synth.dit_state_dict(), attn_shape_invariant=True)
    us = units()
    forms = {"mixed": lambda: call(model, us, STEPS, ode_method=METHODS), "three": lambda: three_calls(model, us)}
    res = timed_rounds(forms, a.reps)
    n_launch = {k: launches(model, fn) for k, fn in forms.items()}
    lines = [f"F5-Base width (dim 1024, depth 22), {len(us)} units of {min(FRAMES)}-{max(FRAMES)} frames (prompt {PROMPT}), CFG 2, sway -1, "
             f"shape-invariant attention; 4 units Euler x 32 steps, 2 midpoint x 16, 2 RK4 x 8 (32 forwards each); median of {a.reps} "
             "alternating rounds after 1 warm-up round, device-synchronised wall clock", ""]
    for key, label in (("mixed", "one mixed-method call"), ("three", "three one-method calls (baseline)")):
        t, ts, r = res[key]
        n = n_launch[key]
        lines.append(f"{label:<36s}: dit_rows {r:7d}  {t * 1e3:8.1f} ms  ({', '.join(f'{x * 1e3:.1f}' for x in ts)})  launches "
                     f"{sum(n.values())} ({', '.join(f'{k} {v}' for k, v in n.items())})")
    lines.append(f"one call vs three: time {100 * (res['mixed'][0] / res['three'][0] - 1):+.1f} %")
    # every unit gets what its own method's call gives it (the GEMM dispatch may differ with the rows of a launch: rounding, not bits)
    mixed, (o_e, o_m, o_r) = forms["mixed"](), forms["three"]()
    d = 0.0
    for i, (ref, j) in enumerate([(o_e, 0), (o_e, 1), (o_e, 2), (o_e, 3), (o_m, 0), (o_m, 1), (o_r, 0), (o_r, 1)]):
        n = unit_duration(PROMPT, N_TEXT, us[i][2])
        d = max(d, (mixed[i, :n] - ref[j, :n]).abs().max().item())
    lines.append(f"max |mixed call - one-method calls| over all units: {d:.3e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
