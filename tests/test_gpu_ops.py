"""GPU parity of the per-kernel unit ops (include/f5hip.h "unit ops"): every hot kernel alone, through the C ABI, against a
plain fp64 torch reference of the same op evaluated on the operand values the kernel actually multiplies (fp16 / bf16 /
split-bf16 rounding of the inputs), so the tolerance only has to cover the fp32 accumulation order: 2e-5 relative rms.
Shapes are the transformer-block GEMMs of F5-TTS-Base at the BASELINE configs (M = 2816 rows = one 10 s utterance with both CFG
branches; F/model/modules.py:324-328,409-447) plus ragged / partial-tile / short-K edge cases."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
Q_SCALE = 0.125 * math.log2(math.e)   # csrc/common.h F5_Q_SCALE: softmax scale 1/8 and log2(e), folded into q by the QKV epilogue


def _counter(name):
    from tts_indic_server_f5_amd import _lib
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset_counters():
    from tts_indic_server_f5_amd import _lib
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _operand_values(x, prec):
    """fp64 tensors whose products sum to what the kernel multiplies: [(a_part, w_part_selector)]."""
    if prec == 3:
        return x.half().double(), None
    hi = x.bfloat16()
    if prec == 1:
        return hi.double(), None
    lo = (x - hi.float()).bfloat16()
    return hi.double(), lo.double()


def _ref_matmul(a, w, prec):
    ah, al = _operand_values(a, prec)
    wh, wl = _operand_values(w, prec)
    y = ah @ wh.T
    if prec == 2:   # bf16x3: hi*hi + hi*lo + lo*hi (the lo*lo term is dropped by design)
        y = y + ah @ wl.T + al @ wh.T
    return y


def _act(y, act):
    if act == "gelu_tanh":
        return torch.nn.functional.gelu(y, approximate="tanh")
    if act == "gelu_erf":
        return torch.nn.functional.gelu(y)
    if act == "silu":
        return torch.nn.functional.silu(y)
    if act == "mish":
        return torch.nn.functional.mish(y)
    return y


def _rel(got, ref):
    return ((got.double().cpu() - ref.cpu()).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-30)).item()


# Every launch counter of the GEMM dispatcher (csrc/f5hip.hip run_gemm_n); a row names the ones its single launch must raise to 1, all others stay 0
PATH_COUNTERS = ("gemm5_rb11", "gemm5_rb8", "gemm5_wide", "gemm5_cb12", "gemm3", "gemm3_wide", "gemm6", "gemm6_r176", "gemm6_r256",
                 "gemm_reg_bn64", "gemm_reg_bn128", "conv5")
G5_11_4, G5_11_8, G5_11_12 = ("gemm5_rb11",), ("gemm5_rb11", "gemm5_wide"), ("gemm5_rb11", "gemm5_wide", "gemm5_cb12")
G5_8_4, G5_8_8 = ("gemm5_rb8",), ("gemm5_rb8", "gemm5_wide")
G6_176, G6_256 = ("gemm6", "gemm6_r176"), ("gemm6", "gemm6_r256")
G3, REG64, REG128 = ("gemm3",), ("gemm_reg_bn64",), ("gemm_reg_bn128",)


def _assert_path(expected):
    got = {n: _counter(n) for n in PATH_COUNTERS}
    want = {n: int(n in expected) for n in PATH_COUNTERS}
    assert got == want, f"dispatcher path: got {got}, expected {want}"


# Expected paths follow csrc/gemm_launch.h: t256 / t176 = gemm6 tiles of 256 / 176 rows x 256 columns (gemm6 needs t256 or t176 >= 224; cost
# = rounds of 256 CUs, x 0.85 for 176-row tiles); gemm5_choose = fewest rounds x (16 rb + 16 cb); t128 = 128 x 128 tiles (split-bf16 / bf16
# operands: gemm3 when t128 <= 256, else gemm.h with the call site's bn).
CASES = [
    # (M, N, K, prec, act, bias, mul, res, row_keep, out16, bn, expected counters)
    (2816, 1024, 1024, 3, "none", True, True, True, False, False, 128, G5_11_4),    # attention out-projection, C2 (176 x 64 tiles)
    (2816, 1024, 2048, 3, "none", True, True, True, False, False, 128, G5_11_4),    # FF2, C2
    (2816, 2048, 1024, 3, "gelu_tanh", True, False, False, False, True, 128, G5_11_8),   # FF1, C2: fp16 plane out (176 x 128 tiles)
    (2816, 1024, 1024, 3, "none", True, False, True, True, False, 128, G5_11_4),    # masked rows (padded-batch semantics)
    (1404, 1024, 1024, 3, "none", True, True, True, False, False, 128, G5_8_4),     # M not a multiple of any tile height: partial row slab (11 x 16 = 176 tiles of 128 x 64)
    (1536, 768, 768, 3, "none", True, True, True, False, False, 128, G5_8_4),       # F5-Small widths (C1): 128-row tiles
    (2816, 100, 1024, 3, "none", True, False, False, False, False, 128, G5_8_4),    # N = mel_dim: partial column panel (n_pad 128: rb 8 x cb 4, 44 tiles, cost 192)
    (2816, 1024, 128, 3, "silu", True, False, False, False, False, 128, G5_11_4),   # K shorter than the ring depth
    (22528, 1024, 1024, 3, "none", True, True, True, False, False, 128, G6_176),    # C3 share: 8 utterances x 2 branches (batch mode); t256 = 352 (2 rounds), t176 = 512 (1.7)
    (22528, 2048, 1024, 3, "gelu_tanh", True, False, False, False, True, 128, G6_256),   # FF1 at the C3 share: fp16 plane out; t256 = 704 (3), t176 = 1024 (3.4)
    (22528, 1024, 2048, 3, "none", True, True, True, False, False, 128, G6_176),    # FF2 at the C3 share (32 K-tiles)
    # ragged batch, masked rows: t256 = 352 (2 rounds), t176 = 512 (1.7) -> 176-row tiles; 22400 = 127 x 176 + 48: the last tile has 48 valid rows
    (22400, 1024, 1024, 3, "none", True, True, True, True, False, 128, G6_176),
    (16384, 1024, 64, 3, "silu", True, False, False, False, False, 128, G6_256),    # one K-tile only (prologue without a second tile); t256 = 256 (1), t176 = 376 (1.7)
    (16384, 1024, 128, 3, "none", True, False, True, False, False, 128, G6_256),    # two K-tiles
    (2816, 1024, 1024, 2, "none", True, True, True, False, False, 128, G3),         # bf16x3 (strict mode): t128 = 176
    (2816, 2048, 1024, 1, "gelu_tanh", True, False, False, False, False, 128, REG128),   # plain bf16: t128 = 352
    (200, 512, 1024, 2, "gelu_erf", True, False, False, False, False, 128, G3),     # Vocos-sized, erf GELU: t128 = 8
    # ---- the gemm.h call sites that pass bn = 64 (run_gemm_ln, the UNetT skip, Vocos pwconv2) and the remaining (kernel, template) pairs
    (4864, 1024, 2048, 2, "none", False, False, False, False, False, 64, REG64),    # UNetT skip Linear(2 D -> D), one E2 chunk (C5): t128 = 38 x 8 = 304
    (14592, 1024, 2048, 2, "none", False, False, False, False, False, 64, REG64),   # UNetT skip at the C5 share (3 chunks x 2 branches x 2432 rows): t128 = 912
    (2816, 1024, 2048, 2, "none", True, True, True, False, False, 64, G3),          # strict-mode FF2, C2: t128 = 176 <= 256 -> gemm3 (bn unused)
    (22528, 1024, 1024, 2, "none", True, True, True, False, False, 64, REG64),      # strict-mode out-projection at the C3 share: t128 = 1408
    (22528, 1024, 1024, 1, "none", True, True, True, False, False, 64, REG64),      # plain-bf16 residual GEMM at the C3 share: t128 = 1408
    (2816, 1024, 1024, 1, "none", True, True, True, False, False, 64, G3),          # plain-bf16 residual GEMM, C2: t128 = 176
    (2816, 2048, 1024, 2, "gelu_tanh", True, False, False, False, False, 128, REG128),   # strict-mode FF1, C2: t128 = 352
    (14592, 4096, 1024, 3, "gelu_tanh", True, False, False, False, True, 128, G6_256),   # E2 FF1 at the C5 share: t256 = 912 (4 rounds), t176 = 1328 (5.1)
    (14592, 1024, 4096, 3, "none", True, True, True, False, False, 64, G6_256),     # E2 FF2 at the C5 share, 64 K-tiles: t256 = 228 (1 round), t176 = 332 (1.7)
    # ragged 256-row tile: t256 = 57 x 4 = 228 (1 round), t176 = 332 (1.7); 14500 = 56 x 256 + 164: the last tile has 164 valid rows; masked rows
    (14500, 1024, 1024, 3, "none", True, True, True, True, False, 64, G6_256),
    (14500, 4096, 1024, 3, "gelu_tanh", True, False, False, False, True, 128, G6_256),   # ragged, wide N: t256 = 912 (4), t176 = 1328 (5.1)
    # single E2 chunk FF2, 64 K-tiles: t256 = 76 and t176 = 112 (< 224: no gemm6); gemm5: rb 11 cb 8 = 28 x 8 = 224 tiles (1 round, cost 304)
    # against rb 11 cb 4 = 448 (2 rounds, 480), rb 8 cb 8 = 304 (2, 512), rb 8 cb 4 = 608 (3, 576)
    (4864, 1024, 4096, 3, "none", True, True, True, False, False, 64, G5_11_8),
    # single E2 chunk FF1: t256 = 304 (2 rounds), t176 = 448 (1.7) -> 176-row tiles; 4864 = 27 x 176 + 112: the last tile has 112 valid rows
    (4864, 4096, 1024, 3, "gelu_tanh", True, False, False, False, True, 128, G6_176),
    (2816, 3072, 1024, 3, "none", True, True, True, False, False, 128, G5_11_12),   # QKV width through the generic epilogue: rb 11 cb 12 = 16 x 16 = 256 tiles (1 round)
    # F5-Small FF1 at 1024 frames: rb 8 cb 8 = 16 x 12 = 192 tiles (1 round, cost 256) against rb 11 cb 8 = 144 (1, 304), rb 8 cb 12 = 128 (1, 320)
    (2048, 1536, 768, 3, "gelu_tanh", True, False, False, False, True, 128, G5_8_8),
    # F5-Small FF1, two utterances of 1024 frames: rb 8 cb 12 = 32 x 8 = 256 tiles (1 round, cost 320) against rb 11 cb 12 = 192 (1, 368)
    (4096, 1536, 768, 3, "gelu_tanh", True, False, False, False, True, 128, ("gemm5_rb8", "gemm5_wide", "gemm5_cb12")),
    (2816, 1024, 736, 3, "none", True, True, True, False, False, 128, G3),          # K % 64 == 32: the fp16 gemm3 fallback (t128 = 176, 128 x 128 tiles)
]


@pytest.mark.parametrize("case", CASES, ids=[f"M{c[0]}_N{c[1]}_K{c[2]}_p{c[3]}_{c[4]}{'_keep' if c[8] else ''}{'_f16out' if c[9] else ''}{'_bn64' if c[10] == 64 else ''}"
                                             for c in CASES])
def test_gemm_unit_op(case):
    from tts_indic_server_f5_amd import ops
    M, N, K, prec, act, use_bias, use_mul, use_res, use_keep, out16, bn, counters = case
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + prec)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g) * 0.1 if use_bias else None
    mul = torch.randn(N, generator=g) if use_mul else None
    res = torch.randn(M, N, generator=g) if use_res else None
    keep = (torch.rand(M, generator=g) > 0.3) if use_keep else None
    ref = _ref_matmul(a, w, prec)
    if bias is not None:
        ref = ref + bias.double()
    ref = _act(ref, act)
    if keep is not None:
        ref = ref * keep.double()[:, None]
    if mul is not None:
        ref = ref * mul.double()
    if res is not None:
        ref = ref + res.double()
    _reset_counters()
    out, _ = ops.gemm(a.to(DEV), w.to(DEV), bias, prec=prec, act=act, mul=mul, res=res, row_keep=keep, out16=out16, bn=bn)
    _assert_path(counters)
    assert torch.isfinite(out).all()
    rel = _rel(out.float(), ref)
    print(f"[parity] gemm M{M} N{N} K{K} prec {prec} {act} bn {bn} ({'+'.join(counters)}): rel rms {rel:.3e}")
    if out16:
        # one fp16 rounding of the output on top of the accumulation error
        assert rel < 6e-4
        assert (out.float().cpu() - ref.half().float()).abs().max() <= 2 * torch.finfo(torch.float16).eps * ref.abs().max()
    else:
        assert rel < (3e-4 if act in ("gelu_tanh", "silu", "mish") else 2e-5)   # hardware exp2 / rcp in the activations: ~1 ulp each


def test_gemm_f16_output_saturates():
    """fp16 safety: a pre-activation beyond the fp16 range must come out as +-65504, never inf (a trained checkpoint with FF1 / GELU
    outliers would otherwise poison the next GEMM's whole row with NaN)."""
    from tts_indic_server_f5_amd import ops
    g = torch.Generator().manual_seed(5)
    a = torch.randn(256, 1024, generator=g)
    w = torch.randn(1024, 1024, generator=g) / 32.0
    a[3] *= 40000.0       # rows 3 and 77 produce |y| >> 65504
    a[77] *= -90000.0
    out, _ = ops.gemm(a.to(DEV), w.to(DEV), None, prec=2, act="none", out16=True)
    assert torch.isfinite(out).all()
    ref = (a.double() @ w.double().T).clamp(-65504.0, 65504.0)
    assert out[3].float().abs().max().item() == 65504.0 and out[77].float().abs().max().item() == 65504.0
    ok = torch.ones(256, dtype=torch.bool); ok[3] = ok[77] = False
    assert _rel(out[ok].float(), ref[ok]) < 1e-3
    big = ref[~ok].abs() >= 65504.0
    assert (out[~ok].float().cpu().abs()[big] == 65504.0).all()


QKV_CASES = [
    # (M, D, prec, rotary positions modulo, expected counters): N = 3 D through the QKV epilogue (gemm3 never takes it)
    (2816, 1024, 3, 1405, G5_11_12),   # C2: rb 11 cb 12 = 16 x 16 = 256 tiles (1 round)
    (1404, 1024, 3, 1405, G5_11_8),    # rb 11 cb 8 = 8 x 24 = 192 tiles (1 round, cost 304)
    (1536, 768, 3, 1405, G5_8_8),      # C1 F5-Small: rb 8 cb 8 = 12 x 18 = 216 tiles (1 round, cost 256)
    (1024, 768, 3, 1405, G5_11_4),     # rb 11 cb 4 = 6 x 36 = 216 tiles (1 round, cost 240)
    (256, 768, 3, 1405, G5_8_4),       # rb 8 cb 4 = 2 x 36 = 72 tiles (1 round, cost 192)
    (2560, 768, 3, 1405, ("gemm5_rb8", "gemm5_wide", "gemm5_cb12")),   # rb 8 cb 12 = 20 x 12 = 240 tiles (1 round, cost 320)
    (2816, 1024, 2, 1405, REG128),     # strict mode: split-bf16 QKV always runs gemm.h (t128 = 528)
    (300, 256, 2, 1405, REG128),
    (22528, 1024, 3, 1405, G6_256),    # C3 share: t256 = 1056 (5 rounds), t176 = 1536 (5.1)
    (8320, 768, 3, 1405, G6_176),      # t256 = 297 (2 rounds), t176 = 432 (1.7); 8320 = 47 x 176 + 48
    (14592, 1024, 3, 2341, G6_256),    # E2 at the C5 share (3 chunks x 2 branches x 2432 rows): t256 = 684 (3 rounds), t176 = 996 (3.4)
]


@pytest.mark.parametrize("M,D,prec,npos,counters", QKV_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in QKV_CASES])
def test_qkv_unit_op(M, D, prec, npos, counters):
    """Fused QKV projection + epilogue against a reference that applies x-transformers' interleaved rotary embedding to channels
    0..63 of q and k (head 0 only: F/model/modules.py:414-426), scales q by log2(e) / 8 (the attention kernel works in base-2 exponents) and rounds to fp16 like the kernel's outputs."""
    from oracle import dit_oracle as O
    from tts_indic_server_f5_amd import ops
    g = torch.Generator().manual_seed(M + D + prec)
    a = torch.randn(M, D, generator=g)
    w = torch.randn(3 * D, D, generator=g) / D ** 0.5
    bias = torch.randn(3 * D, generator=g) * 0.1
    pos = torch.arange(M) % npos          # sequences' worth of positions
    y = (_ref_matmul(a, w, prec) + bias.double()).float()
    q, k, v = y[:, :D].clone(), y[:, D:2 * D].clone(), y[:, 2 * D:]
    freqs = O.rotary_freqs(npos, 64)[0][pos]           # [M, 64]
    q[:, :64] = O.apply_rotary(q[None, :, :64], freqs[None])[0]
    k[:, :64] = O.apply_rotary(k[None, :, :64], freqs[None])[0]
    q = q * Q_SCALE
    _reset_counters()
    gq, gk, gv, _ = ops.qkv(a.to(DEV), w.to(DEV), bias, pos.numpy(), prec=prec)
    _assert_path(counters)
    for name, got, ref in (("q", gq, q), ("k", gk, k), ("v", gv, v)):
        err = (got.cpu() - ref.half().float()).abs()
        # fp16 outputs: identical up to accumulation-order flips of the last fp16 bit on some elements
        assert err.max() <= 2.0 ** -10 * ref.abs().max(), name
        assert (err > 0).float().mean() < 0.10, name
        assert _rel(got, ref.double()) < 4e-4, name


def test_qkv_and_attention_operands_saturate():
    """The attention operands are fp16 since round 3 (csrc/attn3.h): a q / k / v value beyond the fp16 range must leave the QKV epilogue as +-65504,
    never as inf (an inf score would make exp2 produce NaN through inf - inf in the next block), and the attention kernel must stay finite on
    operands at that limit (the fixed-offset fast loop overflows its fp16 probabilities there and the workgroup redoes its tile)."""
    from tts_indic_server_f5_amd import ops
    g = torch.Generator().manual_seed(77)
    M, D = 300, 256
    a = torch.randn(M, D, generator=g)
    w = torch.randn(3 * D, D, generator=g) / D ** 0.5
    a[7] *= 3.0e5                                   # row 7: |q|, |k|, |v| far beyond 65504
    gq, gk, gv, _ = ops.qkv(a.to(DEV), w.to(DEV), torch.zeros(3 * D), torch.arange(M).numpy(), prec=2)
    for t in (gq, gk, gv):
        assert torch.isfinite(t).all() and t[7].abs().max().item() == 65504.0
    n, heads = 200, 2
    q = torch.randn(n, 64 * heads, generator=g)
    k = torch.randn(n, 64 * heads, generator=g)
    v = torch.randn(n, 64 * heads, generator=g)
    k[150] = 60000.0                                # one key at the fp16 limit: scores of +-1e5 for every query
    out, _ = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), (n,), None, heads=heads)
    assert torch.isfinite(out).all()
    qs = (q * Q_SCALE).half().double().view(n, heads, 64).transpose(0, 1) * math.log(2.0)
    ks, vs = (t.half().double().view(n, heads, 64).transpose(0, 1) for t in (k, v))
    ref = (torch.softmax(qs @ ks.transpose(1, 2), dim=-1) @ vs).transpose(0, 1).reshape(n, 64 * heads)
    assert (out.double().cpu() - ref).abs().max().item() < 2.5e-3


def _ln_ref(x, scale, shift, mode):
    """fp64 LayerNorm / RMSNorm of the fp32 rows x, with the op's modulation: AdaLN y = n (1 + scale) + shift, affine y = n scale + shift."""
    xd = x.double()
    if mode == "rms":
        return xd / xd.norm(dim=-1, keepdim=True).clamp_min(1e-12) * x.shape[1] ** 0.5 * scale.double()
    mu, var = xd.mean(-1, keepdim=True), xd.var(-1, unbiased=False, keepdim=True)
    return (xd - mu) / (var + 1e-6).sqrt() * ((1.0 if mode == "adaln" else 0.0) + scale.double()) + shift.double()


def _ln_run(x, scale, shift, mode):
    from tts_indic_server_f5_amd import ops
    if mode == "rms":
        return ops.layernorm(x.to(DEV), scale, torch.zeros(x.shape[1]), gain_off=0.0, eps=0.0, rms=True)
    return ops.layernorm(x.to(DEV), scale, shift, gain_off=1.0 if mode == "adaln" else 0.0, eps=1e-6)


# D: every ln_kernel<NV> instantiation (NV = ceil(D / 256) = 1, 2, 3, 4, 6 -- 5 runs the NV = 6 kernel), and 1028 = 4 x 257, a width that
# leaves lanes of the last float4 column group masked; M: the C2 rows, one row past a multiple of the 4 rows per workgroup, and one workgroup
# that is not full (3 rows)
@pytest.mark.parametrize("mode", ["adaln", "affine", "rms"])
@pytest.mark.parametrize("D", [256, 512, 768, 1024, 1028, 1536])
@pytest.mark.parametrize("M", [2816, 2817, 3])
def test_layernorm_unit_op(mode, D, M):
    g = torch.Generator().manual_seed(9 + D + M)
    x = torch.randn(M, D, generator=g) * 3 + 0.5
    scale = torch.randn(D, generator=g) * 0.3 + (1.0 if mode == "affine" else 0.0)
    shift = torch.randn(D, generator=g) * 0.3
    # a constant row (variance 0: the normalised row is 0, so the output is the shift; 2.5 sums exactly in fp32, so the mean is exact),
    # or, under RMSNorm, an all-zero row (norm 0: the 1e-12 clamp keeps it finite and the output is 0)
    x[M // 2] = 0.0 if mode == "rms" else 2.5
    ref = _ln_ref(x, scale, shift, mode)
    out = _ln_run(x, scale, shift, mode)
    assert out.shape == (M, D) and torch.isfinite(out).all()
    rel = _rel(out, ref)
    print(f"[parity] layernorm {mode} M {M} D {D}: rel rms {rel:.3e}")
    assert rel < 2e-6
    assert (out[M // 2].double().cpu() - ref[M // 2]).abs().max().item() <= 1e-6


@pytest.mark.parametrize("mode", ["adaln", "affine"])
@pytest.mark.parametrize("D", [512, 1024, 1028, 1536])
@pytest.mark.parametrize("ratio", [100.0, 1000.0])
def test_layernorm_large_mean(mode, D, ratio):
    """Rows whose mean is 100 / 1000 times their spread (|mu| / sigma), against fp64 on the same fp32 inputs.  The kernel subtracts the mean
    it computed in a first pass (two-pass variance), so its error is that of the fp32 mean: a lane adds 4 NV elements in a row and the wave
    sum adds the 64 lane sums in 6 levels, so (first order) |mean - mu| <= (4 NV + 6 + 1) u |mu| with u = 2^-24 (the +1: the division by D).
    The subtraction x - mean is exact (Sterbenz) and shifts every normalised element by (mean - mu) / sigma, so the relative rms error is at
    most (4 NV + 7) u |mu| / sigma on top of the 2e-6 of the |mu| / sigma <= 1 rows: 1.4e-4 / 1.4e-3 at NV = 4 for ratio 100 / 1000.
    A one-pass variance (E[x^2] - E[x]^2) would be off by ~ u (|mu| / sigma)^2 = 6e-4 / 6e-2 instead."""
    g = torch.Generator().manual_seed(31 + D + int(ratio))
    M, sigma = 2817, 3.0
    sign = torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0)
    x = sign * ratio * sigma * (1.0 + 0.1 * torch.rand(M, 1, generator=g)) + sigma * torch.randn(M, D, generator=g)
    scale = torch.randn(D, generator=g) * 0.3 + (1.0 if mode == "affine" else 0.0)
    shift = torch.randn(D, generator=g) * 0.3
    ref = _ln_ref(x, scale, shift, mode)
    out = _ln_run(x, scale, shift, mode)
    assert torch.isfinite(out).all()
    nv = 6 if D > 1024 else (D + 255) // 256
    bound = 2e-6 + (4 * nv + 7) * 2.0 ** -24 * 1.1 * ratio
    rel = _rel(out, ref)
    print(f"[parity] layernorm {mode} D {D} |mu|/sigma {ratio:g}: rel rms {rel:.3e} (bound {bound:.2e})")
    assert rel < bound


# Every launch counter of the attention dispatcher (csrc/tu_attn.hip f5_launch_attn3): one per attn3 instance, plus two-range launches
ATTN_COUNTERS = ("attn_bal8", "attn_nw8_deep", "attn_nw8", "attn_nw6_deep", "attn_nw6", "attn_nw4", "attn_seg2")


def _attn_counters():
    return {n: _counter(n) for n in ATTN_COUNTERS}


def _assert_attn_path(instance, seg2, got=None):
    got = _attn_counters() if got is None else got
    want = {n: int(n == "attn_" + instance or (seg2 and n == "attn_seg2")) for n in ATTN_COUNTERS}
    assert got == want, f"attention instance: got {got}, expected {want}"


def _attn_ref(q, k, v, lens, kv, heads):
    """fp64 softmax attention per packed sequence on the fp16-rounded operands (q after the log2(e) / 8 scale, undone in fp64)."""
    qb, kb, vb = (q * Q_SCALE).half().double() * math.log(2.0), k.half().double(), v.half().double()
    o, refs = 0, []
    for i, L in enumerate(lens):
        kl = L if kv is None else kv[i]
        qs, ks, vs = (t[o:o + L].view(L, heads, 64).transpose(0, 1) for t in (qb, kb, vb))
        s = qs @ ks.transpose(1, 2)
        s[:, :, kl:] = float("-inf")
        refs.append((torch.softmax(s, dim=-1) @ vs).transpose(0, 1).reshape(L, 64 * heads))
        o += L
    return torch.cat(refs)


def _check_attn_formats(run, ref, instance, seg2, rel_bound, label):
    """run(out_format) -> fp32 output of one attention launch; every output format against the fp64 reference, and the counters of each launch.

    Split-bf16 planes (16 significand bits) carry the kernel's fp32 result o; their bounds, 2.5e-3 max and 5e-4 relative rms, cover the fp16
    P and V operands over up to a few thousand keys.  The fp16 plane (mixed GEMM mode) is o rounded to nearest once: |fl(o) - o| <= 2^-11 |o|,
    half an ulp, in the normal range (below 2^-14 the absolute half ulp, 2^-25, is far inside the bound).  So, elementwise,
    |out - ref| <= 2.5e-3 + 2^-11 (|ref| + 2.5e-3), and over the whole output rel rms <= r + 2^-11 (1 + r) by the triangle inequality, r
    the split planes' rms bound (rel_bound; None: none).
    The bf16 hi plane (bf16 mode) is o rounded to bf16: the same with 2^-8 for 2^-11.  Both narrow formats must also be that rounding of the
    split planes of the same launch shape (the same o): |out - split| <= (h + 2^-16) |split| + 2^-24, h the half ulp above and 2^-16 what
    hi + lo may miss of o (2^-17) with slack."""
    from tts_indic_server_f5_amd import ops
    split = None
    for fmt, h, name in ((ops.ATTN_OUT_SPLIT, 0.0, "split"), (ops.ATTN_OUT_F16, 2.0 ** -11, "fp16"), (ops.ATTN_OUT_BF16, 2.0 ** -8, "bf16")):
        _reset_counters()
        out = run(fmt)
        _assert_attn_path(instance, seg2)
        assert torch.isfinite(out).all(), (label, name)
        out = out.double().cpu()
        err = (out - ref).abs()
        rel = _rel(out, ref)
        print(f"[parity] {label} {instance} {name}: max err {err.max().item():.3e} rel rms {rel:.3e}")
        assert (err <= 2.5e-3 + h * (ref.abs() + 2.5e-3)).all(), (label, name, err.max().item())
        if rel_bound is not None:
            assert rel < rel_bound + h * (1 + rel_bound), (label, name, rel)
        if split is None:
            split = out
        else:
            dev = (out - split).abs() - ((h + 2.0 ** -16) * split.abs() + 2.0 ** -24)
            assert (dev <= 0).all(), (label, name, "not the rounding of the split planes", dev.max().item())


def _hot_block(q, k, hot):
    """Each (q_row, k_row): the 32 queries from q_row on (one query block when q_row is a multiple of 32) point at key k_row, a key that is
    no query block's sample (odd, and not one of the 16 spread over the key range): logits ~360 nats above every other, so exactly those
    blocks overflow the fixed-offset fast loop and take the running-maximum redo, next to blocks of the same workgroup that do not."""
    for qr, kr in hot:
        q[qr:qr + 32] = 20.0 * k[kr]


# The instance table of f5_launch_attn3.  Cost rule: t_NW = ceil(max_len / 32 NW) query tiles per (sequence, head), wgs_NW = t_NW heads n_seq
# workgroups (n_seq counts the 2 pseudo-sequences of a joint sequence), cost_NW = ceil(wgs_NW / 256) NW; the least cost wins, ties in the
# order 8, 6, 4.  NW = 6 runs the balanced 8-wave kernel (bal8) unless the launch is shape-invariant; NW = 6 / 8 take the 9-stage ring
# ("deep") when wgs <= 256.  Each row: wgs_8 / wgs_6 / wgs_4 -> cost_8 / cost_6 / cost_4.  inv: AttnArgs::shape_invariant (-1: the
# process default, 0).  "overhang": the last query tile of a 6- or 8-wave workgroup reaches past the sequence's 128-row padding into the
# next sequence's rows.  kv: key counts that end inside the first (1-32) or second (33-63) half of a 64-key tile, and kv = 1.
N6_LENS = (385,) + tuple(385 - 11 * i for i in range(1, 32)) + (1,)                 # 33 sequences, 385 .. 44 and 1 frames
N6_KV = tuple(L if i % 3 == 0 else max(1, L - 5 * i) for i, L in enumerate(N6_LENS))
N8_LENS = tuple(577 - 37 * i for i in range(13))                                     # 13 sequences, 577 .. 133
N8_KV = tuple(L if i % 2 == 0 else L - 9 * i for i, L in enumerate(N8_LENS))
N8D_LENS = tuple(577 - 50 * i for i in range(11))                                    # 11 sequences, 577 .. 77
N8D_KV = tuple(L if i % 2 == 0 else L - 13 * i for i, L in enumerate(N8D_LENS))
BAL_HOT = ((224, 1001), (704, 701), (1120, 1033))   # blocks 1 (tile 1), 4 (tile 3: key 701 in the key half of waves 6 / 7), 5 (tile 5: key 1033
#                                                      in the half of waves 4 / 5); the other blocks 4 / 5 of those tiles merge their key halves


@pytest.mark.parametrize("impl", [3])
@pytest.mark.parametrize("lens,kv,heads,k_gain,hot,inv,instance", [
    # C2 (1404 x 16 x 2): 192 / 256 / 352 -> 8 / 6 / 8: NW = 6, 256 workgroups: bal8 (the default mode; shape-invariant: nw6_deep)
    pytest.param((1404, 1404), None, 16, 1.0, (), -1, "bal8", id="lens0-None-16-1.0"),
    # 300 x 4 x 3: 24 / 24 / 36 -> 8 / 6 / 4
    pytest.param((300, 50, 257), (300, 41, 200), 4, 1.0, (), -1, "nw4", id="lens1-kv1-4-1.0"),
    # C1 (748 x 12): 36 / 48 / 72 -> 8 / 6 / 4
    pytest.param((748,), None, 12, 1.0, (), -1, "nw4", id="lens2-None-12-1.0"),
    pytest.param((64,), (1,), 2, 1.0, (), -1, "nw4", id="lens3-kv3-2-1.0"),
    # C5 (2341 x 16 x 2): 320 / 416 / 608 -> 16 / 12 / 12: NW = 6 (the tie goes to 6), 416 workgroups: bal8
    pytest.param((2341, 2341), None, 16, 1.0, (), -1, "bal8", id="lens4-None-16-1.0"),
    pytest.param((33,), (33,), 2, 1.0, (), -1, "nw4", id="lens5-kv5-2-1.0"),
    pytest.param((97, 160), (40, 129), 2, 1.0, (), -1, "nw4", id="lens6-kv6-2-1.0"),
    # 1404 x 4 x 2: 48 / 64 / 88 -> 8 / 6 / 4; k_gain: the redo
    pytest.param((1404, 300), (1404, 290), 4, 12.0, (), -1, "nw4", id="lens7-kv7-4-12.0"),
    pytest.param((200,), None, 2, 40.0, (), -1, "nw4", id="lens8-None-2-40.0"),
    # 1404 x 8 x 4: 192 / 256 / 352 -> 8 / 6 / 8: NW = 6, 256 workgroups -- in the default mode the balanced 8-wave kernel with the 9-stage
    # ring (one barrier per two tiles) next to sequences of 2 / 3 / 3 / 5 tiles; overhang: 1404's last tile (1344-1535) covers 70 rows of the next
    pytest.param((1404, 70, 130, 200), (1404, 65, 130, 129), 8, 1.0, (), -1, "bal8", id="lens9-kv9-8-1.0"),
    pytest.param((1404, 320, 130, 200), (1404, 300, 130, 129), 8, 12.0, (), -1, "bal8", id="lens10-kv10-8-12.0"),
    # the balanced 8-wave kernel (C2 arithmetic as in row 0) with key counts inside the first half tile (its key-half waves 6 / 7 then own
    # nothing valid), just past it, and one key; the last one also through the running-maximum redo (1500: 8 / 6 / 8 as 1404)
    pytest.param((1404, 1404), (1404, 20), 16, 1.0, (), -1, "bal8", id="lens11-kv11-16-1.0"),
    pytest.param((1404, 1404), (33, 1), 16, 1.0, (), -1, "bal8", id="lens12-kv12-16-1.0"),
    pytest.param((1500, 1310), (47, 1310), 16, 12.0, (), -1, "bal8", id="lens13-kv13-16-12.0"),
    # bal8: single blocks redone -- one whole-block wave, one block 4 whose overflow only key-half wave 6 sees, one block 5 only wave 5 sees
    pytest.param((1404, 1404), None, 16, 1.0, BAL_HOT, 0, "bal8", id="bal8-hot-blocks"),
    # nw4, shape-invariant, one block redone (1404 x 4 x 2 as row 7)
    pytest.param((1404, 300), None, 4, 1.0, ((640, 701),), 1, "nw4", id="nw4-hot-block"),
    # nw6_deep: the bal8 shapes above in shape-invariant mode (overhang into the next sequence: rows 9 / 10 / hot-blocks)
    pytest.param((1404, 70, 130, 200), (1404, 65, 130, 129), 8, 1.0, (), 1, "nw6_deep", id="nw6_deep-ragged"),
    pytest.param((1404, 1404), (33, 1), 16, 1.0, (), 1, "nw6_deep", id="nw6_deep-kv"),
    pytest.param((1500, 1310), (47, 1310), 16, 12.0, (), 1, "nw6_deep", id="nw6_deep-gain"),
    pytest.param((1404, 1404), None, 16, 1.0, BAL_HOT, 1, "nw6_deep", id="nw6_deep-hot-blocks"),
    # nw6 (5-stage): 385 x 4 x 33: 264 / 396 / 528 -> 16 / 12 / 12 (tie: 6), 396 workgroups; overhang: 385's last tile (384-575) covers 64 rows
    pytest.param(N6_LENS, N6_KV, 4, 1.0, ((64, 201),), 1, "nw6", id="nw6-hot-block"),
    pytest.param(N6_LENS, N6_KV, 4, 12.0, (), 1, "nw6", id="nw6-gain"),
    # nw8 (5-stage): 577 x 12 x 13: 468 / 624 / 780 -> 16 / 18 / 16 (tie: 8), 468 workgroups; overhang: 577's last tile (512-767), 128 rows
    pytest.param(N8_LENS, N8_KV, 12, 1.0, ((288, 101),), -1, "nw8", id="nw8-hot-block"),
    pytest.param(N8_LENS, N8_KV, 12, 12.0, (), 1, "nw8", id="nw8-gain"),
    # nw8_deep: 577 x 6 x 11: 198 / 264 / 330 -> 8 / 12 / 8 (tie: 8), 198 workgroups
    pytest.param(N8D_LENS, N8D_KV, 6, 1.0, ((288, 101),), 0, "nw8_deep", id="nw8_deep-hot-block"),
    pytest.param(N8D_LENS, N8D_KV, 6, 12.0, (), 1, "nw8_deep", id="nw8_deep-gain"),
])
def test_attention_unit_op(impl, lens, kv, heads, k_gain, hot, inv, instance):
    """Attention kernel alone vs fp64 softmax attention on the fp16-rounded operands (q after the log2(e) / 8 scale, undone in fp64), incl. the key-padding mask
    (F/model/modules.py:429-434), ragged sequences, tiles that overhang a sequence, key counts that end inside either half of a 64-key tile,
    and the C2 / C1 / C5 shapes, for every attn3 instance (asserted by the launch counters) in every output format (_check_attn_formats).
    k_gain > 1 multiplies every key at a position = 15 mod 16 from position 47 on (never one of a query block's local sample keys, csrc/attn3.h):
    logits tens to hundreds of nats above each query's maximum over its sample, which sends nearly every query block of attn3 from its
    fixed-offset fast loop to the running-maximum redo; `hot` sends single blocks there (_hot_block)."""
    from tts_indic_server_f5_amd import ops
    g = torch.Generator().manual_seed(sum(lens) + heads)
    n, D = sum(lens), 64 * heads
    q = torch.randn(n, D, generator=g) * 1.5
    k = torch.randn(n, D, generator=g) * 1.5
    v = torch.randn(n, D, generator=g)
    if k_gain != 1.0:
        o = 0
        for L in lens:
            k[o + 47:o + L:16] *= k_gain
            o += L
    _hot_block(q, k, hot)
    ref = _attn_ref(q, k, v, lens, kv, heads)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    _check_attn_formats(lambda fmt: ops.attention(qd, kd, vd, lens, kv, heads=heads, impl=impl, shape_invariant=inv, out_format=fmt)[0],
                        ref, instance, False, 5e-4, f"attention lens {lens[:4]}{'...' if len(lens) > 4 else ''} heads {heads} k_gain {k_gain} hot {hot}")


# ---------------------------------------------------------------------------------------------------------------- conv1d (BigVGAN convolutions)
from bigvgan_ref import conv_ref as _conv_ref  # noqa: E402


@pytest.mark.parametrize("impl", [5, 0])
@pytest.mark.parametrize("prec,tol", [(2, 4e-5), (3, 4e-3)])
@pytest.mark.parametrize("ci,co,k,dil,batch,P,T", [
    (768, 768, 11, 5, 2, 512, 470),     # stage-1 shape, the largest halo (25 rows), 12 channel chunks of 64 / 24 of 32, 6 column tiles
    (192, 192, 3, 1, 3, 256, 256),      # no padding rows at all: the window must stop at the sequence bounds, not read the neighbour
    (96, 96, 7, 3, 2, 512, 300),        # 96 channels: 64-byte rows in fp16 mode (not a multiple of 64), one column tile of 128 with 96 real
    (24, 24, 11, 1, 2, 1024, 1000),     # last stage: one chunk (no window double buffer), 24 of 64 columns real
    (48, 48, 3, 5, 1, 512, 512),        # one chunk of 64 with 48 real channels
    (384, 768, 3, 1, 2, 256, 200),      # c_out != c_in (the 3-tap form of an up-sampler)
])
def test_conv1d_vs_torch(impl, prec, tol, ci, co, k, dil, batch, P, T):
    """f5hip_op_conv1d through both kernels (conv5.h sliding window, gemm.h implicit GEMM) vs torch conv1d in float64.
    Tolerance (absolute, outputs of rms ~1.7): split bf16 carries ~16 mantissa bits per operand -- 2.4e-5 measured at K = 8448,
    i.e. 1.4e-5 relative; fp16 (11 bits) is the documented fast mode."""
    from tts_indic_server_f5_amd import ops
    g = torch.Generator().manual_seed(1000 + ci + k + dil)
    x = torch.randn(batch * P, ci, generator=g)
    w = torch.randn(co, ci, k, generator=g) / (ci * k) ** 0.5
    bias = torch.randn(co, generator=g)
    res = torch.randn(batch * P, co, generator=g)
    _reset_counters()
    out, _, _ = ops.conv1d(x.to(DEV), w, bias, res.to(DEV), batch=batch, valid=T, dilation=dil, prec=prec, impl=impl)
    if impl == 5:
        assert _counter("conv5") == 1
    else:   # gemm.h, 64-wide tiles for weights padded to 64 rows (c_out <= 64), else 128
        assert _counter("conv5") == 0 and _counter("gemm_reg_bn64" if co <= 64 else "gemm_reg_bn128") == 1
    ref = _conv_ref(x, w, bias, res, batch, P, T, dil)
    got = out.cpu().view(batch, P, co)[:, :T].double()
    err = (got - ref).abs().max().item()
    print(f"[parity] conv1d impl {impl} prec {prec} ci {ci} co {co} k {k} dil {dil}: max err {err:.3e} (ref rms {ref.pow(2).mean().sqrt():.3f})")
    assert err < tol


# ---------------------------------------------------------------------------------------------------------------- MMDiT joint attention
def _joint_ref(q, k, v, x_len, c_len, x_kv, heads):
    """fp64 joint attention (audio rows then text rows per sequence, padding masked on the audio keys) on the fp16-rounded operands, in the
    op's row order: all audio frames, then all text tokens."""
    D = 64 * heads
    bf = lambda t: t.to(torch.float16).double()
    ref = torch.empty(q.shape[0], D, dtype=torch.float64)
    ox, oc = 0, sum(x_len)
    for i, (n, nt) in enumerate(zip(x_len, c_len)):
        sel = torch.cat([torch.arange(ox, ox + n), torch.arange(oc, oc + nt)])
        qq = (bf(q[sel] * Q_SCALE) * math.log(2.0)).view(n + nt, heads, 64).transpose(0, 1)
        kk = bf(k[sel]).view(n + nt, heads, 64).transpose(0, 1)
        vv = bf(v[sel]).view(n + nt, heads, 64).transpose(0, 1)
        s = qq @ kk.transpose(1, 2)
        kv = n if x_kv is None else x_kv[i]
        key_ok = torch.cat([torch.arange(n) < kv, torch.ones(nt, dtype=torch.bool)])
        s = s.masked_fill(~key_ok[None, None, :], float("-inf"))
        ref[sel] = (torch.softmax(s, dim=-1) @ vv).transpose(0, 1).reshape(n + nt, D)
        ox += n; oc += nt
    return ref


# The two-range (SEG2) form of every instance; cost arithmetic as for test_attention_unit_op with n_seq = 2 pseudo-sequences per sequence
J6_X, J6_C = tuple(385 - 17 * i for i in range(11)), tuple(1 + (37 * i) % 385 for i in range(11))
J8_X, J8_C = tuple(577 - 41 * i for i in range(13)), tuple(1 + (53 * i) % 577 for i in range(13))
J8D_X, J8D_C = tuple(577 - 50 * i for i in range(11)), tuple(1 + (61 * i) % 577 for i in range(11))


@pytest.mark.parametrize("x_len,c_len,x_kv,heads,k_gain,inv,instance", [
    # 300 x 4 x 2: 16 / 16 / 24 -> 8 / 6 / 4
    pytest.param([300], [21], None, 4, 1.0, -1, "nw4", id="x_len0-c_len0-None"),
    # 1404 x 4 x 6: 144 / 192 / 264 -> 8 / 6 / 8: NW = 6, 192 workgroups: bal8 (shape-invariant: nw6_deep)
    pytest.param([1404, 257, 64], [240, 65, 7], [1404, 200, 33], 4, 1.0, -1, "bal8", id="x_len1-c_len1-x_kv1"),
    # 130 x 4 x 4: 16 / 16 / 32 -> 8 / 6 / 4
    pytest.param([130, 129], [128, 1], [100, 129], 4, 1.0, -1, "nw4", id="x_len2-c_len2-x_kv2"),
    pytest.param([300], [21], None, 4, 12.0, 1, "nw4", id="nw4-gain"),
    pytest.param([1404, 257, 64], [240, 65, 7], [1404, 200, 33], 4, 12.0, 0, "bal8", id="bal8-gain"),
    pytest.param([1404, 257, 64], [240, 65, 7], [1404, 200, 33], 4, 1.0, 1, "nw6_deep", id="nw6_deep"),
    pytest.param([1404, 257, 64], [240, 65, 7], [1404, 200, 33], 4, 12.0, 1, "nw6_deep", id="nw6_deep-gain"),
    # 385 x 6 x 22: 264 / 396 / 528 -> 16 / 12 / 12 (tie: 6), 396 workgroups
    pytest.param(J6_X, J6_C, tuple(L - 3 * i for i, L in enumerate(J6_X)), 6, 1.0, 1, "nw6", id="nw6"),
    pytest.param(J6_X, J6_C, None, 6, 12.0, 1, "nw6", id="nw6-gain"),
    # 577 x 6 x 26: 468 / 624 / 780 -> 16 / 18 / 16 (tie: 8), 468 workgroups
    pytest.param(J8_X, J8_C, tuple(L - 5 * i for i, L in enumerate(J8_X)), 6, 1.0, -1, "nw8", id="nw8"),
    pytest.param(J8_X, J8_C, None, 6, 12.0, 1, "nw8", id="nw8-gain"),
    # 577 x 3 x 22: 198 / 264 / 330 -> 8 / 12 / 8 (tie: 8), 198 workgroups
    pytest.param(J8D_X, J8D_C, tuple(L - 7 * i for i, L in enumerate(J8D_X)), 3, 1.0, 0, "nw8_deep", id="nw8_deep"),
    pytest.param(J8D_X, J8D_C, None, 3, 12.0, 1, "nw8_deep", id="nw8_deep-gain"),
])
def test_joint_attention_vs_torch(x_len, c_len, x_kv, heads, k_gain, inv, instance):
    """attn3's two-range kernels (keys = audio rows then text rows of the same sequence; queries from either) vs fp64 torch SDPA over
    the concatenation, padding masked on the audio keys only (F/model/modules.py:506-514), for the two-range form of every instance in every
    output format.  Same operand rounding and elementwise bounds as the single-range attention test (no rms bound: unit-variance q and k
    give flat rows, outputs of rms ~ 0.05, which the absolute bound already covers); k_gain multiplies the audio keys at positions 47, 63,
    ... of every sequence (the redo)."""
    from tts_indic_server_f5_amd import ops
    D = 64 * heads
    g = torch.Generator().manual_seed(500 + sum(x_len))
    Fx, Fc = sum(x_len), sum(c_len)
    q, k, v = (torch.randn(Fx + Fc, D, generator=g) for _ in range(3))
    if k_gain != 1.0:
        o = 0
        for n in x_len:
            k[o + 47:o + n:16] *= k_gain
            o += n
    ref = _joint_ref(q, k, v, x_len, c_len, x_kv, heads)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    _check_attn_formats(lambda fmt: ops.joint_attention(qd, kd, vd, x_len, c_len, x_kv, heads=heads, shape_invariant=inv, out_format=fmt),
                        ref, instance, True, None, f"joint attention x {list(x_len)[:3]} c {list(c_len)[:3]} heads {heads} k_gain {k_gain}")


def test_attention_random_shapes(monkeypatch):
    """tools/attn_fuzz.py with a fixed seed: 24 random ragged batches (1-16 heads, key counts ending anywhere in a tile, a third of them with
    logits far above the first key block) + 6 two-range cases, each against fp64 attention on the rounded operands, bound 2.5e-3 as above."""
    import importlib.util
    import os
    import sys
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "attn_fuzz.py")
    spec = importlib.util.spec_from_file_location("attn_fuzz", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["attn_fuzz.py", "24", "3"])
    mod.main()   # exits non-zero on the first case out of bounds


# ---------------------------------------------------------------------------------------------------------------- shape invariance
# In shape-invariant mode a sequence's attention output must not depend, bit for bit, on the launch it is part of (conftest.py
# attn_shape_invariant, infer.infer_requests).  One sequence S moves across the invariant instances by its batch size alone (cost arithmetic
# as for test_attention_unit_op; a joint sequence is 2 pseudo-sequences, so 8 heads there give the workgroup counts of 16 here):
#   1404 frames x 16 heads: alone 96 / 128 / 176 -> 8 / 6 / 4: nw4;  + 1: 192 / 256 / 352 -> 8 / 6 / 8: nw6_deep;
#                           + 3: 384 / 512 / 704 -> 16 / 12 / 12: nw6;  + 7: 768 / 1024 / 1408 -> 24 / 24 / 24: nw8 (5-stage)
#   480 frames x 16 heads:  alone 32 / 48 / 64 -> 8 / 6 / 4: nw4;  + 5: 192 / 288 / 384 -> 8 / 12 / 8: nw8_deep
# (companions: n_companions, position of S in the batch, instance)
INV_LAUNCHES = {
    1404: [(0, 0, "nw4"), (1, 0, "nw6_deep"), (1, 1, "nw6_deep"), (3, 0, "nw6"), (3, 2, "nw6"), (3, 3, "nw6"), (7, 0, "nw8"), (7, 4, "nw8"),
           (7, 7, "nw8")],
    480: [(0, 0, "nw4"), (5, 0, "nw8_deep"), (5, 3, "nw8_deep"), (5, 5, "nw8_deep")],
}
# one query block of S aimed at a key no block samples (_hot_block): NW = 4 / 6 / 8 put it into workgroups of 128 / 192 / 256 queries
INV_HOT = {1404: (640, 701), 480: (288, 101)}


def _inv_seq(kind, L, heads, seed):
    """One sequence: (q, k, v) of its audio frames and, for a joint one, of its L // 7 + 1 text tokens (fp32, q and k with std 1.5)."""
    g = torch.Generator().manual_seed(seed)
    D = 64 * heads
    parts = [L] + ([L // 7 + 1] if kind == "joint" else [])
    return [tuple(torch.randn(n, D, generator=g) * s for s in (1.5, 1.5, 1.0)) for n in parts]


def _inv_launch(kind, heads, seqs):
    """One shape-invariant launch of the sequences `seqs` (split-bf16 output): (per-sequence outputs -- audio rows then text rows --,
    the attention counters of the launch)."""
    from tts_indic_server_f5_amd import ops
    lens = [[p[0].shape[0] for p in s] for s in seqs]
    # single range: the sequences back to back; joint: all audio parts, then all text parts
    order = [s[0] for s in seqs] + ([s[1] for s in seqs] if kind == "joint" else [])
    q, k, v = (torch.cat([p[j] for p in order]).to(DEV) for j in range(3))
    _reset_counters()
    if kind == "joint":
        out = ops.joint_attention(q, k, v, [l[0] for l in lens], [l[1] for l in lens], None, heads=heads, shape_invariant=1)
    else:
        out, _ = ops.attention(q, k, v, [l[0] for l in lens], None, heads=heads, shape_invariant=1)
    counters = _attn_counters()
    rows = torch.split(out, [p[0].shape[0] for p in order])
    n = len(seqs)
    per_seq = [torch.cat([rows[i]] + ([rows[n + i]] if kind == "joint" else [])) for i in range(n)]
    return per_seq, counters


def _assert_same(got, want, label):
    if torch.equal(got, want):
        return
    diff = (got - want).abs()
    rows = diff.amax(dim=1).nonzero().flatten().tolist()
    raise AssertionError(f"{label}: {len(rows)} rows differ (rows {rows[0]}..{rows[-1]}), max diff {diff.max().item():.3e}")


def _s_reference(kind, s, heads):
    (qx, kx, vx), *rest = s
    if kind == "joint":
        qc, kc, vc = rest[0]
        ref = _joint_ref(torch.cat([qx, qc]), torch.cat([kx, kc]), torch.cat([vx, vc]), [qx.shape[0]], [qc.shape[0]], None, heads)
    else:
        ref = _attn_ref(qx, kx, vx, [qx.shape[0]], None, heads)
    return ref


@pytest.mark.parametrize("kind", ["single", "joint"])
@pytest.mark.parametrize("L", [1404, 480])
@pytest.mark.parametrize("hot", [False, True])
def test_attention_shape_invariance(kind, L, hot):
    """S's output is bit-identical alone and inside batches that put it on every shape-invariant instance, at first, middle and last position;
    the counters prove the instances differ.  hot: one query block of S takes the running-maximum redo -- which queries are redone must not
    depend on the workgroup size, so S's other rows (and the block itself) still match across instances.  S alone also against fp64."""
    heads = 16 if kind == "single" else 8
    S = _inv_seq(kind, L, heads, 7)
    if hot:
        _hot_block(S[0][0], S[0][1], (INV_HOT[L],))
    comps = [_inv_seq(kind, L - (97 * i) % (L // 2), heads, 100 + i) for i in range(8)]
    first, seen = None, set()
    for n_comp, pos, instance in INV_LAUNCHES[L]:
        batch = comps[:n_comp]
        batch.insert(pos, S)
        outs, counters = _inv_launch(kind, heads, batch)
        _assert_attn_path(instance, kind == "joint", counters)
        seen.add(instance)
        if first is None:
            first = outs[pos]
            ref = _s_reference(kind, S, heads)
            err = (first.double().cpu() - ref).abs().max().item()
            print(f"[invariance] {kind} {L} hot {hot} alone: max err vs fp64 {err:.3e}")
            assert err < 2.5e-3
        else:
            _assert_same(outs[pos], first, f"{kind} S = {L} x {heads} heads, hot block {hot}: {instance} ({n_comp} companions, S at {pos}) vs alone")
    assert seen == {i for _, _, i in INV_LAUNCHES[L]} and len(seen) >= 2


@pytest.mark.parametrize("kind", ["single", "joint"])
def test_attention_neighbour_invariance(kind):
    """The last query tile of a 6- or 8-wave workgroup reaches past S (1404 frames: rows 1344-1535 / 1280-1535) into the first 128 query
    rows of the sequence after it.  Those rows are never stored for S, and their content must not change S's output either: with the
    neighbour's first 128 queries hot (10x: logits far above their sample maximum against S's keys, so they overflow the fast loop in S's
    workgroups) S must match S with a cold neighbour and S alone, on every instance whose tiles overhang."""
    heads = 16 if kind == "single" else 8
    L = 1404
    S = _inv_seq(kind, L, heads, 7)
    comps = [_inv_seq(kind, L - (97 * i) % (L // 2), heads, 100 + i) for i in range(8)]
    hot_nb = [tuple(t.clone() for t in p) for p in comps[0]]
    hot_nb[0][0][:128] *= 10.0
    (alone,), counters = _inv_launch(kind, heads, [S])
    _assert_attn_path("nw4", kind == "joint", counters)
    for n_comp, instance in ((1, "nw6_deep"), (3, "nw6"), (7, "nw8")):
        for nb, what in ((comps[0], "cold"), (hot_nb, "hot")):
            outs, counters = _inv_launch(kind, heads, [S, nb] + comps[1:n_comp])
            _assert_attn_path(instance, kind == "joint", counters)
            _assert_same(outs[0], alone, f"{kind} S = {L} x {heads} heads, {what} neighbour: {instance} ({n_comp} companions) vs alone")


# ---------------------------------------------------------------------------------------------------------------- poisoned neighbours
# A sequence's attention output must not depend on the VALUES of the other sequences of its launch either, whatever they are: the serving
# path packs unrelated requests into one launch and nothing on it rejects a non-finite mel.  Finite neighbours cannot show a leak that is
# masked by multiplication (a probability of exactly 0 times a neighbour's value row changes nothing; times NaN it destroys the row), so
# every other sequence is filled with NaN, or with 1e30 (finite in fp32; the fp16 operands saturate and every score against it overflows).
# What the kernel reads: the op packs q / k / v as the QKV epilogue stores them, through sat_f16 = min(max(x, -65504), 65504), which maps
# 1e30 to +65504 and NaN to -65504 (max(NaN, a) = a) -- attn3's operands are never NaN in this library, a poisoned row is a row at the fp16
# limit, whose scores against finite keys overflow the fp16 probabilities (inf row sums: the redo vote).
# One row per attn3 instance and one two-range row, shapes from the tables above.  "overhang": the finite sequence's last query tile
# covers rows of the poisoned sequence behind it.  hot: one query block of the FIRST sequence takes the running-maximum redo.
POISON_FILLS = [float("nan"), 1e30]
ISO_ATTN = [
    # (lens, kv, heads, hot, inv, instance)
    pytest.param((300, 50, 257), (300, 41, 200), 4, (), -1, "nw4", id="nw4"),                           # 128-query tiles: no overhang
    pytest.param((1404, 300), None, 4, ((640, 701),), 1, "nw4", id="nw4-hot-block"),
    pytest.param(N6_LENS, N6_KV, 4, ((64, 201),), 1, "nw6", id="nw6-hot-block-overhang"),               # 385's last tile: 64 rows of the next
    pytest.param((1404, 70, 130, 200), (1404, 65, 130, 129), 8, (), 1, "nw6_deep", id="nw6_deep-overhang"),   # 1404's last tile: 70 rows
    pytest.param(N8_LENS, N8_KV, 12, ((288, 101),), -1, "nw8", id="nw8-hot-block-overhang"),            # 577's last tile: 128 rows
    pytest.param(N8D_LENS, N8D_KV, 6, ((288, 101),), 0, "nw8_deep", id="nw8_deep-hot-block-overhang"),
    pytest.param((1404, 70, 130, 200), (1404, 65, 130, 129), 8, (), -1, "bal8", id="bal8-overhang"),
    pytest.param((1404, 1404), None, 16, BAL_HOT, 0, "bal8", id="bal8-hot-blocks-overhang"),            # 1404's last tile: 128 rows
]
ATTN_FORMATS = ("ATTN_OUT_SPLIT", "ATTN_OUT_F16", "ATTN_OUT_BF16")


def _poison_rows(ts, bounds, parity, fill):
    """Copies of the tensors `ts` with the rows [a, b) of every range of `bounds` whose index is = parity mod 2 filled with `fill`."""
    out = [t.clone() for t in ts]
    for i, (a, b) in enumerate(bounds):
        if i % 2 == parity:
            for t in out:
                t[a:b] = fill
    return out


def _assert_isolated(run, instance, seg2, keep, poisoned, fill, label):
    """run(poison, out_format) -> fp32 output rows of one launch.  In every output format the rows `keep` (the finite sequences') are
    bit-identical with finite and with poisoned neighbours, the launch took `instance`, and the poisoned sequences' own rows changed (the
    poison went in)."""
    from tts_indic_server_f5_amd import ops
    for name in ATTN_FORMATS:
        fmt, outs = getattr(ops, name), []
        for poison in (False, True):
            _reset_counters()
            outs.append(run(poison, fmt))
            _assert_attn_path(instance, seg2)
        clean, dirty = outs
        assert torch.isfinite(clean).all(), (label, name)
        assert not torch.equal(dirty[poisoned], clean[poisoned]), (label, name, "the poisoned sequences' outputs did not change: the poison never went in")
        _assert_same(dirty[keep], clean[keep], f"{label} {instance} {name}: finite sequences next to {fill} neighbours vs finite neighbours")
    print(f"[isolation] {label} {instance}{' seg2' if seg2 else ''} fill {fill}: {int(keep.sum())} finite rows bit-equal next to {int(poisoned.sum())} "
          f"poisoned rows, formats {', '.join(ATTN_FORMATS)}")


@pytest.mark.parametrize("fill", POISON_FILLS, ids=["nan", "1e30"])
@pytest.mark.parametrize("parity", [1, 0], ids=["odd_poisoned", "even_poisoned"])
@pytest.mark.parametrize("lens,kv,heads,hot,inv,instance", ISO_ATTN)
def test_attention_poisoned_neighbours(lens, kv, heads, hot, inv, instance, parity, fill):
    """The launch of test_attention_unit_op twice, identical but for the q, k and v rows of every other sequence (the odd ones, then the
    even ones), which the second launch fills with NaN / 1e30: the other sequences' outputs are bit-identical in all three output formats.
    With the odd sequences poisoned the first sequence keeps its hot block (the redo runs next to a poisoned neighbour) and its last
    tile overhangs into poisoned rows; with the even ones poisoned a finite sequence sits behind poisoned rows, and the redo vote of a
    poisoned sequence (NaN row sums) must not reach the finite blocks."""
    from tts_indic_server_f5_amd import ops
    g = torch.Generator().manual_seed(sum(lens) + heads)
    n, D = sum(lens), 64 * heads
    q = torch.randn(n, D, generator=g) * 1.5
    k = torch.randn(n, D, generator=g) * 1.5
    v = torch.randn(n, D, generator=g)
    _hot_block(q, k, hot)
    starts = [sum(lens[:i]) for i in range(len(lens))]
    bounds = [(s, s + L) for s, L in zip(starts, lens)]
    keep = torch.zeros(n, dtype=torch.bool)
    for i, (a, b) in enumerate(bounds):
        keep[a:b] = i % 2 != parity
    dev = {False: [t.to(DEV) for t in (q, k, v)], True: [t.to(DEV) for t in _poison_rows((q, k, v), bounds, parity, fill)]}
    run = lambda poison, fmt: ops.attention(*dev[poison], lens, kv, heads=heads, shape_invariant=inv, out_format=fmt)[0].cpu()
    _assert_isolated(run, instance, False, keep, ~keep, fill, f"attention lens {lens[:4]} heads {heads} hot {hot}")


@pytest.mark.parametrize("fill", POISON_FILLS, ids=["nan", "1e30"])
@pytest.mark.parametrize("parity", [1, 0], ids=["odd_poisoned", "even_poisoned"])
@pytest.mark.parametrize("x_len,c_len,x_kv,heads,inv,instance", [
    pytest.param([1404, 257, 64], [240, 65, 7], [1404, 200, 33], 4, -1, "bal8", id="bal8-seg2"),        # 1404's last tile: 128 rows of the next
    pytest.param([130, 129, 300], [128, 1, 21], [100, 129, 300], 4, 1, "nw4", id="nw4-seg2"),           # a text range of exactly 128 rows
])
def test_joint_attention_poisoned_neighbours(x_len, c_len, x_kv, heads, inv, instance, parity, fill):
    """The same for the two-range kernels: every other sequence's audio AND text rows are poisoned; the audio and text rows of the others
    are bit-identical.  A finite sequence's text queries run in pseudo-sequences of their own, between the poisoned ones' text rows."""
    from tts_indic_server_f5_amd import ops
    D = 64 * heads
    g = torch.Generator().manual_seed(500 + sum(x_len))
    Fx, Fc = sum(x_len), sum(c_len)
    q, k, v = (torch.randn(Fx + Fc, D, generator=g) for _ in range(3))
    xb = [(sum(x_len[:i]), sum(x_len[:i + 1])) for i in range(len(x_len))]
    cb = [(Fx + sum(c_len[:i]), Fx + sum(c_len[:i + 1])) for i in range(len(c_len))]
    keep = torch.zeros(Fx + Fc, dtype=torch.bool)
    for i, ((a, b), (c, d)) in enumerate(zip(xb, cb)):
        keep[a:b] = keep[c:d] = i % 2 != parity
    dirty = _poison_rows(_poison_rows((q, k, v), xb, parity, fill), cb, parity, fill)
    dev = {False: [t.to(DEV) for t in (q, k, v)], True: [t.to(DEV) for t in dirty]}
    run = lambda poison, fmt: ops.joint_attention(*dev[poison], x_len, c_len, x_kv, heads=heads, shape_invariant=inv, out_format=fmt).cpu()
    _assert_isolated(run, instance, True, keep, ~keep, fill, f"joint attention x {x_len} c {c_len} heads {heads}")


def test_attention_random_shapes_invariant(monkeypatch):
    """tools/attn_fuzz.py as test_attention_random_shapes, every launch shape-invariant (no balanced 8-wave kernel; NW = 6 launches run
    the 6-wave instances)."""
    import importlib.util
    import os
    import sys
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "attn_fuzz.py")
    spec = importlib.util.spec_from_file_location("attn_fuzz", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["attn_fuzz.py", "24", "3", "1"])
    mod.main()   # exits non-zero on the first case out of bounds
