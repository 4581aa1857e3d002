"""fp64 references shared by tests/test_gpu_row_ops.py (GPU) and tests/test_row_ops_reference.py (CPU, which pins them): the 16-bit
operand formats of csrc/common.h and the CFG + ODE step formulas written above cfg_step_kernel
(csrc/elementwise.h)."""
import torch


def fmt_split(y):
    """split_bf16 (csrc/common.h) of the fp32 value of y: hi = bf16(y), lo = bf16(y - hi), both round-to-nearest-even; returns hi + lo
    as fp32 (exact: lo's bits lie inside y's 24)."""
    y = y.float()
    hi = y.bfloat16().float()
    return hi + (y - hi).bfloat16().float()


def fmt_f16(y):
    """sat_f16 (csrc/common.h) of the fp32 value of y: clamped to +-65504, then rounded to nearest even; as fp32."""
    return y.float().clamp(-65504.0, 65504.0).half().float()


def cfg_velocity(pc, pu, cfg):
    """v = pc + (pc - pu) cfg in fp64, or pc where the frame has no unconditional row (pu None), and the sum of the absolute values of the
    expression's terms."""
    pc = pc.double()
    if pu is None:
        return pc, pc.abs()
    pu = pu.double()
    return pc + (pc - pu) * cfg, pc.abs() + (pc.abs() + pu.abs()) * abs(cfg)


def euler_step(x, v, dt):
    return x.double() + dt * v


def rk4_stage(stage, y0, v, dt, k1=None, k2=None, k3=None):
    """The input of the next forward after stage 1..3, or y1 after stage 4, of the 3/8 rule over [t0, t0 + dt], in fp64:
        1: y0 + dt k1 / 3   2: y0 + dt (k2 - k1 / 3)   3: y0 + dt (k1 - k2 + k3)   4: y0 + (k1 + 3 (k2 + k3) + k4) dt / 8
    v is the stage's own slope (k_stage); the earlier slopes come in k1..k3."""
    y0 = y0.double()
    if stage == 1:
        return y0 + dt * v / 3
    if stage == 2:
        return y0 + dt * (v - k1.double() / 3)
    if stage == 3:
        return y0 + dt * (k1.double() - k2.double() + v)
    return y0 + (k1.double() + 3 * (k2.double() + k3.double()) + v) * dt / 8


def rk4_stage_abs(stage, y0, sv, dt, k1=None, k2=None, k3=None):
    """rk4_stage with every term replaced by its absolute value (sv: that of the slope's expression): the S of the elementwise bound."""
    a = lambda t: t.double().abs()
    dt = abs(dt)
    if stage == 1:
        return a(y0) + dt * sv / 3
    if stage == 2:
        return a(y0) + dt * (sv + a(k1) / 3)
    if stage == 3:
        return a(y0) + dt * (a(k1) + a(k2) + sv)
    return a(y0) + (a(k1) + 3 * (a(k2) + a(k3)) + sv) * dt / 8
