"""GPU parity of the BigVGAN generator's own kernels through their unit ops (include/f5hip.h): the anti-aliased SnakeBeta activation
(aa_snake2_kernel, every output format), the up-samplers (ConvTranspose1d as a 3-tap implicit GEMM, conv5.h or gemm.h) and conv_post (the
LDS-tiled and the naive kernel), each against the float64 oracle (oracle/bigvgan_oracle.py on float64 tensors) or torch's float64
conv_transpose1d / conv1d, at the launch-geometry edges: channel counts that change the lane layout, lengths around a segment and a tile,
sequences without padding rows, NaN in the padding rows."""
import math

import pytest
import torch

from bigvgan_ref import DEV, SENTINEL, U32  # noqa: F401
from bigvgan_ref import check_untouched as _check_untouched
from bigvgan_ref import counter as _counter
from bigvgan_ref import report as _report
from bigvgan_ref import reset_counters as _reset_counters
from bigvgan_ref import seq_view as _seq_view
from bigvgan_ref import snake_bound as _snake_bound
from bigvgan_ref import snake_nseg as _nseg
from bigvgan_ref import snake_ref as _snake_ref

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- SnakeBeta activation
def _run_snake(x, al, be, batch, P, T, fmt, guard=64):
    """The op into an output pre-filled with SENTINEL (guard rows past batch P included); returns (valid rows [batch, T, C], the whole buffer)"""
    from tts_indic_server_f5_amd import ops
    Cc = x.shape[1]
    out = torch.full((batch * P + guard, Cc), SENTINEL, dtype=torch.float32, device=DEV)
    ops.bigvgan_snake(x.to(DEV), al, be, batch=batch, valid=T, out_format=fmt, out=out)
    out = out.cpu()
    return out[: batch * P].view(batch, P, Cc)[:, :T].double(), out


SNAKE_C = [768, 96, 48, 24, 16, 4, 40]   # cw 64 / 32 (the 96 case) / 48 (nseg 5) / 24 (nseg 10, 240 of 256 lanes) / 16 / 4 (nseg 64) / 40 (off list)


@pytest.mark.parametrize("T", ["1", "2", "5", "15", "16", "17", "seg-1", "seg+1", "3000"])
@pytest.mark.parametrize("Cc", SNAKE_C)
def test_snake_vs_fp64(Cc, T):
    """aa_snake2_kernel via f5hip_op_bigvgan_snake in all three output formats vs the float64 oracle, batch 3, P = T + 9 with NaN in the
    padding rows, the output pre-filled with a sentinel (padding rows and 64 guard rows must come back unchanged).  x = 2 N(0, 1),
    log alpha / log beta uniform in [-1, 1].  Bound: _snake_bound (fp32 arithmetic) for format 0; the other formats add their rounding of
    the output: split bf16 keeps y to 2^-18 |y| (hi to 2^-9 |y|, lo to 2^-9 of the remainder), allowed 2^-17 |y|; fp16 rounds to nearest
    with 11 significant bits, 2^-11 |y|."""
    nseg = _nseg(Cc)
    T = {"seg-1": nseg * 16 - 1, "seg+1": nseg * 16 + 1}.get(T, None) or int(T)
    batch, P = 3, T + 9
    g = torch.Generator().manual_seed(7000 + Cc * 13 + T)
    x = 2 * torch.randn(batch * P, Cc, generator=g)
    x.view(batch, P, Cc)[:, T:] = float("nan")
    al = torch.rand(Cc, generator=g) * 2 - 1
    be = torch.rand(Cc, generator=g) * 2 - 1
    ref = _snake_ref(x, al, be, batch, P, T)
    b32 = _snake_bound(float(x.view(batch, P, Cc)[:, :T].abs().max()), al, be)
    for fmt, name, rel in [(0, "fp32", 0.0), (1, "split-bf16", 2.0 ** -17), (2, "fp16", 2.0 ** -11)]:
        got, out = _run_snake(x, al, be, batch, P, T, fmt)
        _check_untouched(out, batch, P, T)
        err = got - ref
        _report(f"bigvgan snake C {Cc} T {T} nseg {nseg} {name} (bound {b32:.2e} + {rel:.1e} |y|)", err)
        assert (err.abs() <= b32 + rel * ref.abs()).all()


def test_snake_fp16_saturates():
    """Outputs past the fp16 range saturate at +-65504 like sat_f16 (no inf); the others round to fp16.  x up to 1e5 in amplitude:
    the sine term is O(1) there and the fp32 bound is _snake_bound's."""
    Cc, batch, T = 48, 2, 300
    P = T + 9
    g = torch.Generator().manual_seed(7771)
    x = 1e5 * (torch.rand(batch * P, Cc, generator=g) * 2 - 1)
    x.view(batch, P, Cc)[:, T:] = float("nan")
    al = torch.rand(Cc, generator=g) * 2 - 1
    be = torch.rand(Cc, generator=g) * 2 - 1
    ref = _snake_ref(x, al, be, batch, P, T)
    b32 = _snake_bound(1e5, al, be)
    got, out = _run_snake(x, al, be, batch, P, T, 2)
    _check_untouched(out, batch, P, T)
    assert torch.isfinite(got).all()
    over = ref.abs() > 65504 + b32
    assert over.float().mean() > 0.2 and (over.logical_not() & (ref.abs() < 65504 - b32)).float().mean() > 0.2
    assert (got[over] == 65504 * ref[over].sign()).all()
    inside = ref.abs() <= 65504
    err = (got - ref)[inside]
    _report(f"bigvgan snake fp16 saturation C {Cc} T {T} ({over.float().mean():.2f} saturated)", err)
    assert (err.abs() <= b32 + 2.0 ** -11 * ref[inside].abs()).all()


@pytest.mark.parametrize("Cc", [96, 16])
def test_snake_wide_parameter_spread(Cc):
    """log alpha and log beta uniform in [-2.5, 2.5] (alpha, 1 / beta up to e^2.5 = 12.2) and inputs uniform in [-20, 20]: a stress range
    for the sine, whose argument reaches ~300 rad, not a range measured on a trained checkpoint.  Bound: the kernel's max and rms error
    against float64 are at most 2x those of the same operator computed by PyTorch in fp32 (the oracle on fp32 tensors), measured here on
    the same inputs: the fp32 rounding of the argument (u e^a) is what both make, and the hardware sine must not add more than that."""
    batch, T = 3, 1000
    P = T + 9
    g = torch.Generator().manual_seed(7900 + Cc)
    x = 20 * (torch.rand(batch * P, Cc, generator=g) * 2 - 1)
    x.view(batch, P, Cc)[:, T:] = float("nan")
    al = torch.rand(Cc, generator=g) * 5 - 2.5
    be = torch.rand(Cc, generator=g) * 5 - 2.5
    ref = _snake_ref(x, al, be, batch, P, T)
    ref32 = _snake_ref(x, al, be, batch, P, T, torch.float32).double()
    got, out = _run_snake(x, al, be, batch, P, T, 0)
    _check_untouched(out, batch, P, T)
    mx32, rms32 = _report(f"bigvgan snake wide spread C {Cc} torch fp32", ref32 - ref)
    mx, rms = _report(f"bigvgan snake wide spread C {Cc} kernel", got - ref)
    print(f"[parity] bigvgan snake wide spread C {Cc}: kernel / torch fp32 error ratio max {mx / mx32:.2f} rms {rms / rms32:.2f}")
    assert mx <= 2 * mx32 and rms <= 2 * rms32


# ---------------------------------------------------------------------------------------------------------------- up-samplers
UPS = [(1536, 768, 4), (768, 384, 4), (96, 48, 2), (48, 24, 2), (8, 4, 2), (512, 256, 8), (64, 32, 6)]


@pytest.mark.parametrize("prec,tol", [(2, 4e-5), (3, 4e-3)])
@pytest.mark.parametrize("T,P", [(1, 256), (127, 128), (128, 128), (300, 512)])
@pytest.mark.parametrize("ci,co,r", UPS)
def test_upsample_vs_fp64(ci, co, r, T, P, prec, tol):
    """f5hip_op_bigvgan_upsample (bv_pack_ups + the generator's bv_conv) vs torch conv_transpose1d(stride r, padding r / 2) in float64, batch 3.
    (8, 4, 2): 8 real of 64 padded weight rows, a 64-wide tile; (64, 32, 6): a rate outside the default geometry.  P % 256 == 0 runs conv5.h,
    P = 128 the gemm.h fallback; T = 128 = P has no padding row, so the t + 1 tap of the last row must read zero, not the next sequence.
    Padding rows hold 100 N(0, 1).  Weights N(0, 1 / (2 ci)) (each output sees 2 ci products), inputs N(0, 1), bias N(0, 1).
    Tolerance: the conv1d test's bounds.  A split-bf16 operand is within 2^-18 of its value (hi to 2^-9, lo to 2^-9 of the rest); with the
    dropped lo lo term each product is within 3 2^-18 relative, independently per product, so an output with sum (x w)^2 ~ 1 errs by
    ~2^-18 = 3.8e-6 rms, plus ~sqrt(K) u32 of fp32 accumulation; 4e-5 is ten times that, room for the tail of the largest single products
    at small c_in.  fp16 operands are within 2^-11 of their values: ~2^-11 sqrt(2 / 3) = 4e-4 rms, and 4e-3 is ten times that."""
    from tts_indic_server_f5_amd import ops
    batch = 3
    g = torch.Generator().manual_seed(8000 + ci + r + T)
    x = torch.randn(batch * P, ci, generator=g)
    x.view(batch, P, ci)[:, T:] = 100 * torch.randn(batch, P - T, ci, generator=g)
    w = torch.randn(ci, co, 2 * r, generator=g) / math.sqrt(2 * ci)
    bias = torch.randn(co, generator=g)
    _reset_counters()
    out = ops.bigvgan_upsample(x.to(DEV), w, bias, batch=batch, valid=T, rate=r, prec=prec)
    expect = "conv5" if P % 256 == 0 else ("gemm_reg_bn64" if r * co <= 64 else "gemm_reg_bn128")
    ran = {n: _counter(n) for n in ("conv5", "gemm_reg_bn64", "gemm_reg_bn128")}
    assert ran == {n: int(n == expect) for n in ran}, ran
    ref = torch.nn.functional.conv_transpose1d(_seq_view(x, batch, P, T).double(), w.double(), bias.double(), stride=r, padding=r // 2)
    got = out.cpu().view(batch, P * r, co)[:, : T * r].permute(0, 2, 1).double()
    assert got.shape == ref.shape
    mx, _ = _report(f"bigvgan upsample ci {ci} co {co} r {r} T {T} P {P} prec {prec} ({expect})", got - ref)
    assert mx < tol


# ---------------------------------------------------------------------------------------------------------------- conv_post
@pytest.mark.parametrize("T", [1, 3, 255, 256, 257, 513])
@pytest.mark.parametrize("Cc,variant", [(c, v) for c in (4, 24, 32, 44) for v in (1, 2)] + [(c, 2) for c in (45, 48, 96)] + [(44, 0), (48, 0)])
def test_conv_post_vs_fp64(Cc, variant, T):
    """f5hip_op_bigvgan_conv_post vs torch conv1d(padding 3) + clamp in float64: variant 1 = the LDS kernel (its tile fits up to C = 44),
    2 = the naive kernel, 0 = the generator's choice.  T around the 256-output tile and its 3-row halo; batch 2, P = T + 4 with NaN in the
    padding rows.  Inputs N(0, 1), weights N(0, 1 / (7 C)), so the output is ~N(0, 1) and about a third of it clips.
    Bound: the kernel sums n = 7 C fp32 products in sequence, |error| <= gamma_n sum |w a| with gamma_n = n u32 / (1 - n u32), evaluated per
    output.  Outputs whose exact value lies beyond +-(1 + bound) must come back as exactly +-1; the others within the bound of the clamped
    exact value."""
    from tts_indic_server_f5_amd import ops
    batch, P = 2, T + 4
    g = torch.Generator().manual_seed(9000 + Cc * 7 + T)
    a = torch.randn(batch * P, Cc, generator=g)
    a.view(batch, P, Cc)[:, T:] = float("nan")
    w = torch.randn(Cc, 7, generator=g) / math.sqrt(7 * Cc)
    wave = ops.bigvgan_conv_post(a.to(DEV), w, batch=batch, valid=T, variant=variant).cpu().double()
    av = _seq_view(a, batch, P, T).double()
    ref = torch.nn.functional.conv1d(av, w.double()[None], padding=3)[:, 0]
    mag = torch.nn.functional.conv1d(av.abs(), w.double().abs()[None], padding=3)[:, 0]
    n = 7 * Cc
    bound = n * U32 / (1 - n * U32) * mag
    assert torch.isfinite(wave).all() and wave.shape == ref.shape
    clip = ref.abs() > 1 + bound
    assert (wave[clip] == ref[clip].sign()).all(), "the clamp must give exactly +-1"
    err = wave - ref.clamp(-1, 1)
    kind = {0: "auto", 1: "lds", 2: "naive"}[variant]
    _report(f"bigvgan conv_post {kind} C {Cc} T {T} ({clip.double().mean():.2f} clipped)", err)
    assert (err.abs() <= bound).all()


def test_conv_post_lds_refuses_wide_tile():
    """variant 1 at C = 45: the LDS tile (262 (C + 1) + 7 C floats) would exceed 48 KB, so the op fails instead of launching it."""
    from tts_indic_server_f5_amd import _lib, ops
    a = torch.zeros(128, 45, device=DEV)
    with pytest.raises(_lib.F5HipError):
        ops.bigvgan_conv_post(a, torch.zeros(45, 7), batch=1, valid=100, variant=1)
