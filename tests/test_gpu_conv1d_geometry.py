"""GPU: every tile shape of the sliding-window convolution (conv5.h) and the implicit-GEMM form of gemm.h, through f5hip_op_conv1d in the
uniform (batch, P, T) layout, against torch conv1d in float64.

conv5_kernel is warp-specialised with hand-counted vmcnt waits whose counts depend on the tap count, the channel-chunk count and the depth of
the weight ring, so every instance runs here with one chunk and with several, at all nine (kernel, dilation) pairs of AMPBlock1, and over a
sweep of valid lengths around the halo and the 256-row tile.  Batch 3: the middle sequence has a neighbour on both sides.  The padding rows
of x and of the residual hold NaN: a window row or a residual row taken from outside [0, T) shows as a NaN in a valid output.

Inputs as in tests/test_gpu_ops.py::test_conv1d_vs_torch (x ~ N(0, 1), w ~ N(0, 1 / (c_in k)), bias and res ~ N(0, 1)), so that test's
tolerances carry over: 4e-5 absolute for split bf16, 4e-3 for fp16 (bigvgan_ref.CONV_TOL)."""
import pytest
import torch

from bigvgan_ref import CONV_TOL, DEV, conv_counters, conv_ref, reset_counters

pytestmark = pytest.mark.gpu

BATCH = 3
NAN = float("nan")

# (c_in, c_out, prec) -> the conv5 instance <planes, LDS row bytes, 32-column blocks> and its channel chunks (launch_conv5 in csrc/conv5.h)
INSTANCES = {
    (192, 192, 2): ("<2,64,4>", 6), (192, 192, 3): ("<1,128,4>", 3),
    (96, 96, 2): ("<2,64,4>", 3), (96, 96, 3): ("<1,64,4>", 3),
    (64, 64, 2): ("<2,64,2>", 2), (64, 64, 3): ("<1,128,2>", 1),     # <2,64,2> with 2 chunks: the single-window rewrite
    (24, 24, 2): ("<2,64,2>", 1), (24, 24, 3): ("<1,64,2>", 1),
    (128, 64, 3): ("<1,128,2>", 2),
    (96, 48, 3): ("<1,64,2>", 3),
}
KD = [(k, d) for k in (3, 7, 11) for d in (1, 3, 5)]
EDGE_KD = [(11, 5), (3, 1)]


def _instance(ci, co, prec):
    """the dispatch arithmetic of launch_conv5 for a dense convolution: weights padded to 64 rows (c_out <= 64) or to a multiple of 128,
    channels to a multiple of 32; fp16 takes 64-channel chunks where the padded channel count allows it"""
    cpad = (ci + 31) // 32 * 32
    n_pad = 64 if co <= 64 else (co + 127) // 128 * 128
    nb = 4 if n_pad > 128 else n_pad // 32
    if prec == 2:
        return f"<2,64,{nb}>", cpad // 32
    return (f"<1,128,{nb}>", cpad // 64) if cpad % 64 == 0 else (f"<1,64,{nb}>", cpad // 32)


def _edge_lengths(k, dil):
    halo = (k - 1) // 2 * dil
    return [(512, t) for t in sorted({1, halo, halo + 1, 100, 255, 256, 257, 511, 512})] + [(256, 256)]   # T = 100: the second tile is all padding


def _data(ci, co, k, dil, P, T):
    g = torch.Generator().manual_seed(4000 + 7 * ci + 3 * co + 31 * k + dil + 13 * T + P)
    x = torch.randn(BATCH * P, ci, generator=g)
    w = torch.randn(co, ci, k, generator=g) / (ci * k) ** 0.5
    bias = torch.randn(co, generator=g)
    res = torch.randn(BATCH * P, co, generator=g)
    x.view(BATCH, P, ci)[:, T:] = NAN
    res.view(BATCH, P, co)[:, T:] = NAN
    return x, w, bias, res


def _check(impl, prec, ci, co, k, dil, P, T, expect, tag):
    from tts_indic_server_f5_amd import ops
    x, w, bias, res = _data(ci, co, k, dil, P, T)
    reset_counters()
    out, _, _ = ops.conv1d(x.to(DEV), w, bias, res.to(DEV), batch=BATCH, valid=T, dilation=dil, prec=prec, impl=impl)
    ran = conv_counters()
    assert ran == {n: int(n == expect) for n in ran}, (tag, ran)
    got = out.cpu().view(BATCH, P, co)[:, :T].double()
    assert torch.isfinite(got).all(), f"{tag}: a padding row (NaN) reached a valid output"
    err = (got - conv_ref(x, w, bias, res, BATCH, P, T, dil)).abs().max().item()
    print(f"[parity] conv1d {tag} impl {impl} prec {prec} ci {ci} co {co} k {k} dil {dil} P {P} T {T}: max err {err:.3e} (bound {CONV_TOL[prec]:.0e})")
    assert err < CONV_TOL[prec], tag


def test_instance_table_matches_the_dispatch_arithmetic():
    assert {key: _instance(*key) for key in INSTANCES} == INSTANCES
    # every instance, each with one chunk and with several
    seen = {}
    for inst, chunks in INSTANCES.values():
        seen.setdefault(inst, set()).add(chunks > 1)
    assert set(seen) == {"<2,64,4>", "<2,64,2>", "<1,128,4>", "<1,128,2>", "<1,64,4>", "<1,64,2>"}
    assert all(v == {False, True} for i, v in seen.items() if i.endswith(",2>")), seen   # (a 128-wide tile of 32 channels does not exist: c_out > 64 >= c_in)


@pytest.mark.parametrize("k,dil", KD)
@pytest.mark.parametrize("ci,co,prec", list(INSTANCES))
def test_conv5_every_kernel_and_dilation(ci, co, prec, k, dil):
    """(i) all nine (k, dilation) pairs of AMPBlock1 at T = 300, P = 512: taps 3 / 7 / 11 x the chunk counts of every instance"""
    inst, chunks = INSTANCES[(ci, co, prec)]
    _check(5, prec, ci, co, k, dil, 512, 300, "conv5", f"conv5{inst} {chunks} chunk(s)")


@pytest.mark.parametrize("k,dil", EDGE_KD)
@pytest.mark.parametrize("ci,co,prec", list(INSTANCES))
def test_conv5_length_edges(ci, co, prec, k, dil):
    """(ii) valid lengths 1, halo, halo + 1, 100 (a tile of padding only), 255 / 256 / 257 (around the tile), 511, 512 (no padding row) at
    P = 512, and T = P = 256, at the largest halo (25 rows) and the smallest (1)"""
    inst, chunks = INSTANCES[(ci, co, prec)]
    for P, T in _edge_lengths(k, dil):
        _check(5, prec, ci, co, k, dil, P, T, "conv5", f"conv5{inst} {chunks} chunk(s)")


@pytest.mark.parametrize("k,dil", EDGE_KD)
@pytest.mark.parametrize("prec", [2, 3])
@pytest.mark.parametrize("ci,co,expect", [(192, 192, "gemm_reg_bn128"), (24, 24, "gemm_reg_bn64")])
def test_gemm_form_length_edges(ci, co, expect, prec, k, dil):
    """(iii) the CONV form of gemm_kernel (impl 0) over the same sweep, and at P = 384 (three 128-row tiles per sequence, which conv5 refuses)"""
    for P, T in _edge_lengths(k, dil) + [(384, 384), (384, 257)]:
        _check(0, prec, ci, co, k, dil, P, T, expect, expect)


@pytest.mark.parametrize("batch", [3, 2])
def test_conv5_refuses_a_pitch_of_384(batch):
    """impl 5 at P = 384 (batch 3: M % 256 != 0; batch 2: M fits, the pitch does not): an error, and neither kernel is launched"""
    from tts_indic_server_f5_amd import _lib, ops
    x = torch.zeros(batch * 384, 96, device=DEV)
    reset_counters()
    with pytest.raises(_lib.F5HipError):
        ops.conv1d(x, torch.zeros(96, 96, 3), None, None, batch=batch, valid=300, prec=2, impl=5)
    assert conv_counters() == {"conv5": 0, "gemm_reg_bn64": 0, "gemm_reg_bn128": 0}
