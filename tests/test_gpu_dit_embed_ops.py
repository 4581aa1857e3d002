"""GPU parity of the kernels every backbone runs before its first block, through their unit ops (include/f5hip.h), which run them
through the backbone's own host code (run_conv_pos_embed, run_text_block and the packed row layout of setup_sequences):

- ConvPositionEmbedding: the grouped Conv1d(D, D, 31, groups 16) + Mish, twice, plus the residual, on conv5.h (DiT / MMDiT) and on gemm.h
  (UNetT, plain-bf16 mode), at group widths 64, 48, 24 and 8;
- one ConvNeXtV2 text block: depthwise conv + LayerNorm (ln_kernel's dw prefix), pwconv1 + GELU, GRN (grn_stats_kernel / grn_apply_kernel),
  pwconv2 + residual.

Each stage is compared with float64 torch fed with the op's own previous stage, per sequence, element by element against a bound derived from
the operand precision and the length of the sum, over ragged batches whose lengths sit on the edges of the windows, the 128-row tiles and the
GRN unroll.  NaN in the padding rows, the time-token rows and the slack behind the buffers must not change a real row by one bit."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import dit_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24              # fp32 unit roundoff
U_SPLIT = 2.0 ** -14        # split-bf16 product: hi + lo holds each operand to 2^-16 relative, and lo * lo (<= 2^-16) is dropped: 3 2^-16, with margin
P_SPLIT = 2.0 ** -16        # a value stored as split-bf16 planes: |x - hi - lo| <= 2^-8 |x - hi| <= 2^-16 |x|
P_BF16 = 2.0 ** -8          # a value stored as one bf16 plane (unit roundoff of bf16)
MISH_D = 1.09               # max |mish'(x)|
GELU_D = 1.13               # max |gelu'(x)|


def _counter(name):
    from tts_indic_server_f5_amd import _lib
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset_counters():
    from tts_indic_server_f5_amd import _lib
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _check(tag, got, ref, tol):
    """max |got - ref| / tol <= 1 element-wise; prints the measured error next to the bound"""
    got, ref, tol = got.double(), ref.double(), tol.double()
    err = (got - ref).abs()
    assert torch.isfinite(got).all(), f"{tag}: non-finite output"
    ratio = (err / tol).max().item()
    print(f"[parity] {tag}: max err {err.max().item():.3e} rms err {err.pow(2).mean().sqrt().item():.3e}  max err / bound {ratio:.3f}"
          f"  (bound median {tol.median().item():.2e})")
    assert ratio <= 1.0, f"{tag}: error exceeds its bound by {ratio:.2f}x"
    return ratio


def _split(x, seq_len):
    return list(torch.split(x, list(seq_len), dim=0))


# ---------------------------------------------------------------------------------------------------------------- ConvPositionEmbedding
def _gconv(x, w, b):
    """Conv1d(D, D, 31, padding 15, groups 16) of one sequence x [n, D] in x's dtype (weights [D, D / 16, 31]) -> [n, D]"""
    n, D = x.shape
    gw = D // 16
    win = F.pad(x, (0, 0, 15, 15)).unfold(0, 31, 1).reshape(n, 16, gw, 31)       # [n, group, ci, tap]
    return torch.einsum("ngct,goct->ngo", win, w.reshape(16, gw, gw, 31)).reshape(n, D) + b


def _conv_stage_ref(x, w, b, seq_len, K, bf16):
    """Mish(GConv(x)) per sequence in float64 and its bound.  bf16: the kernel multiplies bf16-rounded operands exactly (fp32 products of
    8-bit mantissas), so the reference does too and only the fp32 accumulation of K products remains; split bf16: the operands' 2^-16
    representation error and the dropped lo * lo term (U_SPLIT), plus the accumulation of 3 K MFMA products.  Mish then adds at most
    MISH_D times that and its own hardware exp / rcp rounding, (2 |pre| + 8) u relative."""
    xd = x.to(DEV, torch.float64)
    wd, bd = w.to(DEV, torch.float64), b.to(DEV, torch.float64)
    if bf16:
        xd, wd = _bf16(xd), _bf16(wd)
    out, tol = [], []
    for xs in _split(xd, seq_len):
        pre = _gconv(xs, wd, bd)
        s = _gconv(xs.abs(), wd.abs(), bd.abs())
        e_pre = s * ((0.0 if bf16 else U_SPLIT) + (1 if bf16 else 3) * K * U) + 2 * U * bd.abs()
        m = F.mish(pre)
        out.append(m)
        tol.append(MISH_D * e_pre + (2 * pre.abs().clamp(max=20) + 8) * U * m.abs() + 1e-30)
    return torch.cat(out), torch.cat(tol)


def _pos_params(D, seed):
    g = torch.Generator().manual_seed(seed)
    gw = D // 16
    sc = 1.0 / (31 * gw) ** 0.5
    return [torch.randn(D, gw, 31, generator=g) * sc * 1.5, torch.randn(D, generator=g) * 0.1,
            torch.randn(D, gw, 31, generator=g) * sc * 1.5, torch.randn(D, generator=g) * 0.1]


SEQS_POS = [1, 15, 129, 16, 31, 128, 127, 1404, 128]   # whole window clipped; window vs sequence; full tiles back to back; a second tile; C2


def _run_pos(x, prm, seq_len, impl, prec, lead=0, pad_nan=False):
    from tts_indic_server_f5_amd import ops
    return ops.conv_pos_embed(x.to(DEV), *prm, seq_len=seq_len, lead=lead, impl=impl, prec=prec, taps=True, pad_nan=pad_nan)


CONV_CASES = [(D, impl, prec, lead) for D in (1024, 768, 384, 128) for impl, prec, lead in ((5, 2, 0), (0, 2, 0), (0, 1, 0))] + \
             [(1024, 0, 2, 1), (768, 0, 1, 1), (128, 0, 2, 1)]


@pytest.mark.parametrize("D,impl,prec,lead", CONV_CASES, ids=[f"D{c[0]}-impl{c[1]}-prec{c[2]}-lead{c[3]}" for c in CONV_CASES])
def test_conv_pos_embed_vs_fp64(D, impl, prec, lead):
    """Both grouped convolutions against float64 per sequence, stage 1 from the op's input and stage 2 from the op's own stage 1, with
    x ~ N(0, 1.5^2) and weights at 1.5x the default init scale (pre-activations of O(3), Mish's curved region).  K = 31 gw: the worst-case
    bound is dominated by the fp32 accumulation, 3 K u sum|a w| (split bf16) resp. K u sum|a w| (bf16).  Measured on an MI355X (split
    bf16, conv5 and gemm.h alike): max error 6e-5 .. 7e-5 (stage 1) and 4e-5 .. 5e-5 (stage 2) at every width, 0.005 .. 0.07 of the
    bound.  In bf16 mode stage 2 measures 3e-6 .. 7e-6 (0.005 .. 0.06 of the bound); stage 1 is read back as the bf16 plane the second
    convolution reads, so its rounding (P_BF16, up to 3e-2 here) is part of the bound and the ratio reaches 0.97 by construction."""
    gw = D // 16
    K = 31 * gw
    g = torch.Generator().manual_seed(1000 + D)
    seq_len = SEQS_POS if D >= 768 else [s for s in SEQS_POS if s != 1404] + [300]
    x = torch.randn(sum(seq_len), D, generator=g) * 1.5
    prm = _pos_params(D, D)
    _reset_counters()
    out, c1 = _run_pos(x, prm, seq_len, impl, prec, lead)
    if impl == 5:
        assert _counter("conv5") == 2
    else:
        assert _counter("gemm_reg_bn64") == 2 and _counter("conv5") == 0
    bf16 = prec == 1
    tag = f"conv_pos D {D} (gw {gw}) impl {impl} prec {prec} lead {lead}"
    ref1, tol1 = _conv_stage_ref(x, prm[0], prm[1], seq_len, K, bf16)
    tol1 = tol1 + (P_BF16 if bf16 else P_SPLIT) * ref1.abs()                 # the tap: stage 1 as stored in the operand planes
    _check(tag + " stage 1", c1, ref1, tol1)
    ref2, tol2 = _conv_stage_ref(c1, prm[2], prm[3], seq_len, K, bf16)
    ref2 = ref2 + x.to(DEV, torch.float64)
    tol2 = tol2 + U * ref2.abs()
    _check(tag + " stage 2 + residual", out, ref2, tol2)


@pytest.mark.parametrize("D", [1024, 768, 384, 128])
def test_conv_pos_embed_nan_padding_is_inert(D):
    """NaN in the padding rows, the time-token rows and the slack behind the operand buffers: every real row comes out finite and
    bit-identical to the run with zero there, on both kernels.  Groups narrower than 64 channels (gw < 64) read 64 channels per tap, the
    last group up to 64 - gw channels into the next row -- a padding row or the buffer's slack behind the last sequence; the kernels
    load those channels as zero."""
    g = torch.Generator().manual_seed(77 + D)
    seq_len = [128, 1, 37, 256, 129]         # full tiles (the next sequence starts on the very next row), the last sequence padded
    x = torch.randn(sum(seq_len), D, generator=g)
    prm = _pos_params(D, 7 * D)
    for impl, prec, lead in ((5, 2, 0), (0, 2, 0), (0, 1, 0), (0, 2, 1)):
        ref = _run_pos(x, prm, seq_len, impl, prec, lead, pad_nan=False)
        got = _run_pos(x, prm, seq_len, impl, prec, lead, pad_nan=True)
        for r, o, name in ((ref[0], got[0], "out"), (ref[1], got[1], "stage 1")):
            bad = (~torch.isfinite(o)).sum().item()
            diff = (o != r).sum().item()
            print(f"[parity] conv_pos NaN padding D {D} impl {impl} prec {prec} lead {lead} {name}: {bad} non-finite, {diff} differing")
            assert bad == 0 and diff == 0


def test_conv_pos_embed_last_row_fills_its_tile():
    """A batch whose LAST sequence ends exactly on a 128-row boundary: the last group of its last row reads into the buffer's slack behind
    all rows (NaN here), not into a padding row."""
    D = 768
    g = torch.Generator().manual_seed(5)
    seq_len = [40, 256]
    x = torch.randn(sum(seq_len), D, generator=g)
    prm = _pos_params(D, 11)
    for impl, prec in ((5, 2), (0, 2), (0, 1)):
        a = _run_pos(x, prm, seq_len, impl, prec, pad_nan=False)[0]
        b = _run_pos(x, prm, seq_len, impl, prec, pad_nan=True)[0]
        assert torch.isfinite(b).all() and torch.equal(a, b), f"impl {impl} prec {prec}"


def test_conv_pos_embed_refuses_conv5_with_time_token():
    from tts_indic_server_f5_amd import ops
    from tts_indic_server_f5_amd._lib import F5HipError
    prm = _pos_params(128, 3)
    with pytest.raises(F5HipError, match="bad argument"):
        ops.conv_pos_embed(torch.zeros(10, 128, device=DEV), *prm, seq_len=[10], lead=1, impl=5, prec=2)


# ---------------------------------------------------------------------------------------------------------------- ConvNeXtV2 text block
def _cnx_params(Td, seed, big_channel=None):
    g = torch.Generator().manual_seed(seed)
    p = {"dwconv.weight": torch.randn(Td, 1, 7, generator=g) * 0.4, "dwconv.bias": torch.randn(Td, generator=g) * 0.1,
         "norm.weight": 1 + 0.2 * torch.randn(Td, generator=g), "norm.bias": 0.1 * torch.randn(Td, generator=g),
         "pwconv1.weight": torch.randn(2 * Td, Td, generator=g) / Td ** 0.5, "pwconv1.bias": 0.1 * torch.randn(2 * Td, generator=g),
         "grn.gamma": 0.5 * torch.randn(1, 1, 2 * Td, generator=g), "grn.beta": 0.1 * torch.randn(1, 1, 2 * Td, generator=g),
         "pwconv2.weight": torch.randn(Td, 2 * Td, generator=g) / (2 * Td) ** 0.5, "pwconv2.bias": 0.1 * torch.randn(Td, generator=g)}
    return p


SEQS_CNX = [1, 2, 3, 7, 8, 9, 15, 17, 129, 4096]   # dw window clipped on both sides; GRN unroll (8) and tail; a second tile; a long sum


def _cnx_input(Td, seq_len, seed):
    """x ~ N(0, 1), and in the sequence of 129 tokens one input channel 40x larger than the rest"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(sum(seq_len), Td, generator=g)
    xs = _split(x, seq_len)
    xs[8][:, 3] *= 40.0
    return torch.cat(xs)


def _run_cnx(x, p, seq_len, pad_nan=False):
    from tts_indic_server_f5_amd import ops
    return ops.convnext_block(x.to(DEV), p, seq_len=seq_len, taps=True, pad_nan=pad_nan)


def _ln_ref(x, p, seq_len):
    """dwconv (k 7, zero padding at the sequence bounds) + LayerNorm(eps 1e-6) per sequence in float64, and the bound: the fp32 7-tap
    sum (8 u sum|w x| + |b|), the wave-sum mean and variance over Td terms (2 Td u relative to the row's deviations), all scaled by the
    row's rstd and |norm.weight|; the output planes hold the result to 2^-16 (P_SPLIT)."""
    Td = x.shape[1]
    d = lambda k: p[k].to(DEV, torch.float64)
    out, tol = [], []
    for xs in _split(x.to(DEV, torch.float64), seq_len):
        y = F.conv1d(xs.t()[None], d("dwconv.weight"), d("dwconv.bias"), padding=3, groups=Td)[0].t()
        s = F.conv1d(xs.abs().t()[None], d("dwconv.weight").abs(), d("dwconv.bias").abs(), padding=3, groups=Td)[0].t()
        e_y = 8 * U * s
        mean, var = y.mean(-1, keepdim=True), y.var(-1, unbiased=False, keepdim=True)
        rstd = (var + 1e-6).rsqrt()
        n = (y - mean) * rstd
        r = n * d("norm.weight") + d("norm.bias")
        e_dev = 2 * e_y.amax(-1, keepdim=True) + Td * U * y.abs().amax(-1, keepdim=True)
        e_n = rstd * e_dev + n.abs() * (e_dev * rstd + Td * U + 4 * U)
        out.append(r)
        tol.append(d("norm.weight").abs() * (e_n + 4 * U * n.abs()) + 2 * U * d("norm.bias").abs() + P_SPLIT * r.abs() + 1e-30)
    return torch.cat(out), torch.cat(tol)


def _linear_bound(a, w, b, K):
    """|a| |w|^T + |b| times the split-bf16 product error and 3 K accumulated MFMA products"""
    return (a.abs() @ w.abs().t() + b.abs()) * (U_SPLIT + 3 * K * U) + 1e-30


@pytest.mark.parametrize("Td", [512, 96, 64])
def test_convnext_block_stages_vs_fp64(Td):
    """Each kernel of the block against float64 fed with the op's own previous stage, per sequence.  The GRN bound: the column norm is an
    fp32 sum of n squares (8 partial sums, the tail into the first), (n + 2) u relative; the channel mean adds 2 Td u; the output's three
    terms add 4 u each; the planes hold the result to 2^-16.  Measured on an MI355X (Td 512 / 96 / 64), max error / bound: dwconv +
    LayerNorm 0.04 / 0.20 / 0.26, pwconv1 + GELU 0.04 / 0.19 / 0.31, pwconv2 + residual 0.04 / 0.39 / 0.41, GRN 0.48 at every width
    (its bound is dominated by the storage of its output in split-bf16 planes, P_SPLIT: the large channel reaches ~1e3)."""
    seq_len = SEQS_CNX
    x = _cnx_input(Td, seq_len, 31 + Td)
    p = _cnx_params(Td, 9 * Td)
    p["pwconv1.weight"][5] = 0.0
    p["pwconv1.bias"][5] = 0.0                                # GELU channel 5 is 0 in every row: Gx = 0 for every sequence
    p["pwconv1.weight"][7] *= 30.0                            # GELU channel 7 dominates the GRN channel mean of every sequence
    out, tp = _run_cnx(x, p, seq_len)
    d = lambda k: p[k].to(DEV, torch.float64).reshape(p[k].shape[0], -1) if p[k].dim() == 2 else p[k].to(DEV, torch.float64).reshape(-1)
    # dwconv + LayerNorm
    ref, tol = _ln_ref(x, p, seq_len)
    _check(f"convnext Td {Td} dwconv + LayerNorm", tp["ln"], ref, tol)
    # pwconv1 + GELU (erf) on the op's own LayerNorm output (the planes, exact in fp32)
    a = tp["ln"].double()
    pre = a @ d("pwconv1.weight").t() + d("pwconv1.bias")
    e = _linear_bound(a, d("pwconv1.weight"), d("pwconv1.bias"), Td)
    ref = F.gelu(pre)
    _check(f"convnext Td {Td} pwconv1 + GELU", tp["ty"], ref, GELU_D * e + 8 * U * ref.abs() + 1e-30)
    # GRN on the op's own GELU output
    ty = tp["ty"].double()
    outs, tols = [], []
    gamma, beta = d("grn.gamma"), d("grn.beta")
    for n, ys in zip(seq_len, _split(ty, seq_len)):
        gx = ys.norm(dim=0, keepdim=True)
        den = gx.mean(-1, keepdim=True) + 1e-6
        nx = gx / den
        r = gamma * (ys * nx) + beta + ys
        rel = (n + 2) * U + 2 * Td * U + 6 * U
        outs.append(r)
        tols.append((gamma * ys * nx).abs() * rel + 4 * U * ((gamma * ys * nx).abs() + beta.abs() + ys.abs()) + P_SPLIT * r.abs() + 1e-30)
    _check(f"convnext Td {Td} GRN", tp["grn"], torch.cat(outs), torch.cat(tols))
    assert (tp["ty"][:, 5] == 0).all()
    # pwconv2 + residual on the op's own GRN output
    a = tp["grn"].double()
    ref = a @ d("pwconv2.weight").t() + d("pwconv2.bias") + x.to(DEV, torch.float64)
    e = _linear_bound(a, d("pwconv2.weight"), d("pwconv2.bias"), 2 * Td) + 2 * U * ref.abs()
    _check(f"convnext Td {Td} pwconv2 + residual", out, ref, e)


@pytest.mark.parametrize("Td", [512, 96])
def test_convnext_block_vs_oracle_block(Td):
    """The whole block against oracle.dit_oracle.convnext_v2_block in float64 per sequence (a batch of one each), max error relative to the
    output scale.  Measured on an MI355X: 6.7e-6 (Td 512) and 6.8e-6 (Td 96) of max|out| at the worst sequence; the bound is 2e-5."""
    seq_len = SEQS_CNX
    x = _cnx_input(Td, seq_len, 5 + Td)
    p = _cnx_params(Td, 3 * Td)
    out = _run_cnx(x, p, seq_len)[0].double().cpu()
    sd = {"b." + k: v.double() for k, v in p.items()}
    worst = 0.0
    for n, xs, os_ in zip(seq_len, _split(x.double(), seq_len), _split(out, seq_len)):
        ref = O.convnext_v2_block(sd, "b.", xs[None])[0]
        err = (os_ - ref).abs().max().item() / ref.abs().max().item()
        worst = max(worst, err)
        assert err < 2e-5, f"len {n}: {err:.3e}"
    print(f"[parity] convnext Td {Td} block vs float64 oracle: worst max err / max|out| {worst:.3e} (bound 2e-5)")


@pytest.mark.parametrize("Td", [512, 64])
def test_convnext_block_nan_padding_is_inert(Td):
    """NaN in the padding rows of every internal buffer: the real rows of every stage are finite and bit-identical to the zero-padding run."""
    seq_len = [7, 128, 3, 129]
    x = _cnx_input(Td, seq_len + [1] * 6, 3)[: sum(seq_len)]
    p = _cnx_params(Td, 17)
    a_out, a_tp = _run_cnx(x, p, seq_len, pad_nan=False)
    b_out, b_tp = _run_cnx(x, p, seq_len, pad_nan=True)
    for name, a, b in [("out", a_out, b_out)] + [(k, a_tp[k], b_tp[k]) for k in ("ln", "ty", "grn")]:
        print(f"[parity] convnext Td {Td} NaN padding {name}: {(~torch.isfinite(b)).sum().item()} non-finite, {(a != b).sum().item()} differing")
        assert torch.isfinite(b).all() and torch.equal(a, b)
