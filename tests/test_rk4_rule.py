"""CPU: the fixed-grid RK4 solver (CFM(odeint_kwargs=dict(method="rk4")), torchdiffeq's rk4_alt_step_func).  torchdiffeq is absent, so
the rule restated in tests/rk4_oracle.py is pinned here by closed-form answers, including one that tells the 3/8 rule from the classic
1/6-1/3-1/3-1/6 rule; and the Python layers accept the method name and carry it to the sampler."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import dit_oracle as O  # noqa: E402
from rk4_oracle import rk4_odeint  # noqa: E402
from tts_indic_server_f5_amd import infer, loaders  # noqa: E402

TINY = dict(dim=128, depth=2, heads=2, ff_mult=2, text_dim=64, conv_layers=2)


@pytest.mark.parametrize("a, dt", [(-1.3, 1.0), (0.7, 0.25), (2.0, -0.5)])
def test_linear_field_one_step_is_the_fourth_order_taylor_polynomial(a, dt):
    """dy/dt = a y: one step multiplies y by 1 + z + z^2/2 + z^3/6 + z^4/24 (z = a dt), like every 4-stage fourth-order rule."""
    y0 = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)
    t = torch.tensor([0.1, 0.1 + dt], dtype=torch.float64)
    y1 = rk4_odeint(lambda tt, yy: a * yy, y0, t, keep_trajectory=False)
    z = a * dt
    assert torch.allclose(y1, y0 * (1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24), rtol=1e-14, atol=0)
    # and several steps converge on exp(a) at fourth order: halving dt cuts the error ~16x
    errs = []
    for n in (8, 16):
        tg = torch.linspace(0, 1, n + 1, dtype=torch.float64)
        errs.append(abs(rk4_odeint(lambda tt, yy: a * yy, torch.ones(1, dtype=torch.float64), tg, keep_trajectory=False).item() - math.exp(a)))
    assert 12 < errs[0] / errs[1] < 20


@pytest.mark.parametrize("steps, sway", [(1, None), (5, -1.0), (8, 0.4), (32, -1.0)])
def test_cubic_in_time_is_integrated_exactly_on_any_sway_grid(steps, sway):
    """dy/dt = c3 t^3 + c2 t^2 + c1 t + c0: the 3/8 rule is Simpson's 3/8 quadrature here, exact for cubics on any grid."""
    c3, c2, c1, c0 = 1.7, -2.2, 0.9, 0.3
    t = O.sway_time_grid(steps, sway, dtype=torch.float64)
    traj = rk4_odeint(lambda tt, yy: (c3 * tt ** 3 + c2 * tt ** 2 + c1 * tt + c0) * torch.ones_like(yy), torch.zeros(2, dtype=torch.float64), t)
    exact = lambda s: c3 * s ** 4 / 4 + c2 * s ** 3 / 3 + c1 * s ** 2 / 2 + c0 * s
    for i in range(steps + 1):
        assert abs(traj[i, 0].item() - (exact(t[i].item()) - exact(t[0].item()))) < 1e-14
    assert traj.shape == (steps + 1, 2)


def test_quartic_tells_the_three_eighths_rule_from_the_classic_rule():
    """dy/dt = t^4 on [0, 1], one step: the 3/8 rule gives (0 + 3 (1/81 + 16/81) + 1) / 8 = 11/54 = 0.20370, the classic rule
    (0 + 2 (1/16) + 2 (1/16) + 1) / 6 = 0.208333; the exact value is 0.2.  Both rules are exact for cubics, so only a quartic tells them apart."""
    y1 = rk4_odeint(lambda tt, yy: tt ** 4 * torch.ones_like(yy), torch.zeros(1, dtype=torch.float64),
                    torch.tensor([0.0, 1.0], dtype=torch.float64), keep_trajectory=False).item()
    assert abs(y1 - 11 / 54) < 1e-15
    classic = (0.0 + 2 * 0.5 ** 4 + 2 * 0.5 ** 4 + 1.0) / 6
    assert abs(classic - 0.208333) < 1e-6 and abs(y1 - classic) > 4e-3


def test_stage_times_and_state_in_fp32_follow_torch():
    """The sampler's grid is fp32: the stages are evaluated at t0 + dt * (1/3) and t0 + dt * (2/3) rounded in fp32, and the last stage at
    t1 itself (the same float as the next step's t0) -- what the library's time table holds."""
    t = O.sway_time_grid(4, -1.0)
    seen = []
    rk4_odeint(lambda tt, yy: (seen.append(tt), yy)[1], torch.zeros(1), t)
    assert len(seen) == 16 and all(s.dtype == torch.float32 for s in seen)
    for i in range(4):
        dt = t[i + 1] - t[i]
        assert [s.item() for s in seen[4 * i:4 * i + 4]] == [t[i].item(), (t[i] + dt * (1 / 3)).item(), (t[i] + dt * (2 / 3)).item(),
                                                              t[i + 1].item()]


def test_model_accepts_rk4_and_still_rejects_adaptive_solvers():
    """F5HipModel takes odeint_kwargs=dict(method="rk4") past its method check (here it then stops at the missing device, which the check
    used to precede); an adaptive solver is still refused before anything is built."""
    from tts_indic_server_f5_amd._lib import F5HipError
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    with pytest.raises(F5HipError, match="HIP device"):
        F5HipModel(DiTArch(text_num_embeds=40, **TINY), {}, device="cpu", odeint_kwargs=dict(method="rk4"))
    with pytest.raises(ValueError, match="rk4"):
        F5HipModel(DiTArch(text_num_embeds=40, **TINY), {}, device="cpu", odeint_kwargs=dict(method="dopri5"))


def test_load_model_carries_rk4_to_the_sampler(tmp_path, monkeypatch):
    """load_model(ode_method="rk4") -> UnloadedModel -> load_checkpoint builds the sampler with odeint_kwargs=dict(method="rk4")."""
    built = []
    monkeypatch.setattr(loaders, "F5HipModel", type("F5HipModel", (), {"__init__": lambda self, *a, **k: built.append(k)}))
    from tts_indic_server_f5_amd import synth
    sd = synth.dit_state_dict(text_num_embeds=40, **TINY)
    path = str(tmp_path / "model.pt")
    torch.save({"ema_model_state_dict": {"ema_model." + k: v for k, v in sd.items()}}, path)
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("".join(chr(33 + i) + "\n" for i in range(40)), encoding="utf-8")
    model = infer.load_model(infer.DiT, TINY, vocab_file=str(vocab), ode_method="rk4")
    assert isinstance(model, loaders.UnloadedModel) and model.odeint_kwargs == dict(method="rk4")
    infer.load_checkpoint(model, path, "cuda")
    infer.load_model(infer.DiT, TINY, vocab_file=str(vocab), ode_method="rk4", ckpt_path=path)
    assert [k["odeint_kwargs"] for k in built] == [dict(method="rk4")] * 2
