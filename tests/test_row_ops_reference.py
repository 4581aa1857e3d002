"""CPU: the fp64 references of tests/test_gpu_row_ops.py (tests/row_ops_ref.py) are themselves right -- the four RK4 stage formulas,
chained, are the 3/8-rule step of tests/rk4_oracle.py, and the 16-bit format helpers round known values as csrc/common.h does."""
import torch

from rk4_oracle import rk4_odeint
from row_ops_ref import cfg_velocity, euler_step, fmt_f16, fmt_split, rk4_stage, rk4_stage_abs


def test_chained_stage_formulas_are_the_three_eighths_rule_step():
    g = torch.Generator().manual_seed(11)
    n = 7
    A = torch.randn(n, n, generator=g, dtype=torch.float64) * 0.7
    b = torch.randn(n, generator=g, dtype=torch.float64)
    fn = lambda t, y: y @ A.T + b * t          # a linear field with a time-dependent drive
    y0 = torch.randn(5, n, generator=g, dtype=torch.float64)
    t0, dt = 0.15, 0.21
    t = torch.tensor([t0, t0 + dt], dtype=torch.float64)
    want = rk4_odeint(fn, y0, t)[-1]
    k1 = fn(t[0], y0)
    k2 = fn(t[0] + dt / 3, rk4_stage(1, y0, k1, dt))
    k3 = fn(t[0] + 2 * dt / 3, rk4_stage(2, y0, k2, dt, k1))
    k4 = fn(t[1], rk4_stage(3, y0, k3, dt, k1, k2))
    got = rk4_stage(4, y0, k4, dt, k1, k2, k3)
    assert (got - want).abs().max().item() < 1e-12
    # the term-by-term absolute sums bound the formulas
    for s, v, ks in ((1, k1, ()), (2, k2, (k1,)), (3, k3, (k1, k2)), (4, k4, (k1, k2, k3))):
        assert (rk4_stage(s, y0, v, dt, *ks).abs() <= rk4_stage_abs(s, y0, v.abs(), dt, *ks) * (1 + 1e-15)).all()


def test_cfg_velocity_and_euler_step():
    pc, pu = torch.tensor([1.5, -2.0]), torch.tensor([0.5, 1.0])
    v, s = cfg_velocity(pc, pu, 2.0)
    assert v.tolist() == [3.5, -8.0] and s.tolist() == [5.5, 8.0]
    v, s = cfg_velocity(pc, None, 2.0)
    assert v.tolist() == [1.5, -2.0] and s.tolist() == [1.5, 2.0]
    assert euler_step(torch.tensor([1.0]), torch.tensor([4.0], dtype=torch.float64), 0.25).tolist() == [2.0]


def test_format_helpers_round_known_values():
    # bf16 keeps 8 significand bits, ties to even
    x = torch.tensor([1.0 + 2.0 ** -7, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -9, 1.0 + 3 * 2.0 ** -8, -7.5, 0.0])
    hi = x.bfloat16().float()
    assert hi.tolist() == [1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -7.5, 0.0]
    assert torch.equal(fmt_split(x), x)                       # each is hi + an exactly representable remainder
    y = torch.tensor([1.0 + 2.0 ** -9 + 2.0 ** -20, 3.0 + 2.0 ** -12 + 2.0 ** -21])
    s = fmt_split(y)
    assert s.tolist() == [1.0 + 2.0 ** -9, 3.0 + 2.0 ** -12]              # the remainder is itself rounded to 8 bits
    assert ((s - y).abs() <= 2.0 ** -17 * y.abs()).all()
    assert torch.equal(fmt_split(y.double()), s)              # fp64 input: its fp32 value is what is split
    # fp16: 11 significand bits, ties to even, saturation instead of inf
    h = fmt_f16(torch.tensor([2049.0, 2051.0, 2050.0, 65519.0, 65520.0, 1.0e6, -1.0e6, 2.0 ** -25, 1.5 * 2.0 ** -24]))
    assert h.tolist() == [2048.0, 2052.0, 2050.0, 65504.0, 65504.0, 65504.0, -65504.0, 0.0, 2.0 ** -23]
