"""Shared by the GPU parity tests of the BigVGAN kernels (tests/test_gpu_bigvgan_ops.py, test_gpu_bigvgan_ragged_ops.py,
test_gpu_conv1d_geometry.py, the conv1d test of test_gpu_ops.py): the float64 references, the derived error bound of the snake kernel, the
sentinel checks, the dispatch counters and the `[parity]` report line.  Plain torch on the CPU; nothing here touches the device."""
import ctypes as C
import math

import torch

from oracle import bigvgan_oracle as B

DEV = "cuda:0"
U32 = 2.0 ** -24            # fp32 unit roundoff
SENTINEL = -321.5           # exact in fp32, split bf16 and fp16
DELTA_SIN = 2.0 ** -18      # allowance for the absolute error of the hardware sine (v_sin_f32 is not correctly rounded)
CONV_TOL = {2: 4e-5, 3: 4e-3}   # absolute, split bf16 / fp16 operands at unit-variance inputs (derived in test_upsample_vs_fp64's docstring)


def counter(name):
    from tts_indic_server_f5_amd import _lib
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def reset_counters():
    from tts_indic_server_f5_amd import _lib
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def conv_counters():
    """how often each convolution kernel family was dispatched since reset_counters()"""
    return {n: counter(n) for n in ("conv5", "gemm_reg_bn64", "gemm_reg_bn128")}


def report(tag, err):
    mx, rms = err.abs().max().item(), err.pow(2).mean().sqrt().item()
    print(f"[parity] {tag}: max err {mx:.3e} rms err {rms:.3e}")
    return mx, rms


def seq_view(x, batch, P, T):
    """channel-last rows [batch P, C] -> the valid rows as [batch, C, T]"""
    return x.view(batch, P, -1)[:, :T].permute(0, 2, 1)


# ---------------------------------------------------------------------------------------------------------------- convolutions
def conv_ref(x, w, bias, res, batch, P, T, dil):
    """nn.Conv1d on the valid rows of every sequence (zero padding at the sequence bounds), channel-last in / out, float64 -> [batch, T, c_out]"""
    M, ci = x.shape
    k = w.shape[-1]
    xv = x.view(batch, P, ci)[:, :T].transpose(1, 2).double()
    y = torch.nn.functional.conv1d(xv, w.double(), None if bias is None else bias.double(), dilation=dil, padding=dil * (k - 1) // 2)
    y = y.transpose(1, 2)
    if res is not None:
        y = y + res.view(batch, P, -1)[:, :T].double()
    return y


def ups_ref(x, w, bias, batch, P, T, r):
    """nn.ConvTranspose1d(k = 2 r, stride r, padding r / 2) on the valid rows, float64 -> [batch, r T, c_out]"""
    y = torch.nn.functional.conv_transpose1d(seq_view(x, batch, P, T).double(), w.double(), None if bias is None else bias.double(), stride=r,
                                             padding=r // 2)
    return y.permute(0, 2, 1)


# ---------------------------------------------------------------------------------------------------------------- SnakeBeta activation
def snake_ref(x, al, be, batch, P, T, dtype=torch.float64):
    """Activation1d of the oracle in `dtype` over the valid rows -> [batch, T, C]"""
    y = B.activation1d(seq_view(x, batch, P, T).to(dtype), al.to(dtype), be.to(dtype))
    return y.permute(0, 2, 1)


def snake_bound(x_amp, al, be):
    """First-order worst-case error of aa_snake2_kernel's fp32 arithmetic, from |x| <= x_amp and the parameters:
    up-sampled u = sum of 6 taps 2 f_k x: |u| <= F1 x_amp with F1 = max over the two phases of sum |2 f_k|, error du <= 7 u32 F1 x_amp (6 fused
    products plus the filter's own fp32 rounding).  The sine argument in revolutions u e^a / 2 pi carries the rounding of expf, of the 1 / 2 pi
    constant, of their product and of u e^a (<= 4 u32 relative) plus du, and the hardware sine adds DELTA_SIN; d sin^2(theta) <= |d theta|, so
    d sin^2 <= min(e^a du + 4 u32 theta_max + 2 DELTA_SIN, 1).  The snake value a = u + sin^2 / (e^b + 1e-9) then has
    da <= du + ib (d sin^2 + 3 u32) + u32 |a|_max (ib = its reciprocal's rounding, 3 u32), and the 12-tap low-pass adds
    F2 da + 13 u32 F2 |a|_max with F2 = sum |f_k|.  Second-order terms are covered by a factor 2."""
    f = B.aa_filter(torch.float64)
    F1 = max(float((2 * f[0::2]).abs().sum()), float((2 * f[1::2]).abs().sum()))
    F2 = float(f.abs().sum())
    a_max, ib_max = math.exp(float(al.max())), math.exp(-float(be.min()))
    u_max = F1 * x_amp
    du = 7 * U32 * u_max
    theta_max = a_max * u_max
    dsn2 = min(a_max * du + 4 * U32 * theta_max + 2 * DELTA_SIN, 1.0)
    v_max = u_max + ib_max
    da = du + ib_max * (dsn2 + 3 * U32) + U32 * v_max
    return 2 * (F2 * da + 13 * U32 * F2 * v_max)


# format rounding of the snake op's outputs, relative to |y|: fp32 none; split bf16 2^-17 (hi + lo); fp16 2^-11 (11 significant bits)
SNAKE_FORMATS = [(0, "fp32", 0.0), (1, "split-bf16", 2.0 ** -17), (2, "fp16", 2.0 ** -11)]


def snake_nseg(Cc):
    """nseg of bv_snake_launch: cw = the largest divisor of C up to 64 (96 -> 32), nseg = 256 / cw segments of 16 steps per workgroup"""
    cw = min(Cc, 64)
    while Cc % cw:
        cw -= 1
    if Cc == 96:
        cw = 32
    return 256 // cw


# ---------------------------------------------------------------------------------------------------------------- sentinel checks
def check_untouched(out, batch, P, T):
    """no NaN anywhere; padding rows of every sequence and the guard rows still hold the sentinel"""
    assert not torch.isnan(out).any()
    Cc = out.shape[1]
    body = out[: batch * P].view(batch, P, Cc)
    assert (body[:, T:] == SENTINEL).all(), "a padding row was written"
    assert (out[batch * P:] == SENTINEL).all(), "the guard past the last sequence was written"


def check_untouched_items(out, row0, valid):
    """ragged form: no NaN anywhere, and every row outside [row0[i], row0[i] + valid[i]) of all items (padding rows, the rows between items, the
    guard rows) still holds the sentinel"""
    assert not torch.isnan(out).any()
    keep = torch.ones(out.shape[0], dtype=torch.bool)
    for r0, v in zip(row0, valid):
        keep[r0: r0 + v] = False
    assert (out[keep] == SENTINEL).all(), "a row outside every item's valid rows was written"
