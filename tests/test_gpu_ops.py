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


@pytest.mark.parametrize("impl", [3])
@pytest.mark.parametrize("lens,kv,heads,k_gain", [((1404, 1404), None, 16, 1.0), ((300, 50, 257), (300, 41, 200), 4, 1.0), ((748,), None, 12, 1.0),
                                                  ((64,), (1,), 2, 1.0), ((2341, 2341), None, 16, 1.0), ((33,), (33,), 2, 1.0), ((97, 160), (40, 129), 2, 1.0),
                                                  ((1404, 300), (1404, 290), 4, 12.0), ((200,), None, 2, 40.0),
                                                  # 6-wave workgroups with the 9-stage ring (one barrier per two tiles) next to sequences of 2 / 3 / 3 / 5 tiles
                                                  ((1404, 70, 130, 200), (1404, 65, 130, 129), 8, 1.0), ((1404, 320, 130, 200), (1404, 300, 130, 129), 8, 12.0),
                                                  # the balanced 8-wave kernel with key counts inside the first half tile (its key-half waves 6 / 7 then own nothing
                                                  # valid), just past it, and one key; the last one also through the running-maximum redo
                                                  ((1404, 1404), (1404, 20), 16, 1.0), ((1404, 1404), (33, 1), 16, 1.0), ((1500, 1310), (47, 1310), 16, 12.0)])
def test_attention_unit_op(impl, lens, kv, heads, k_gain):
    """Attention kernel alone vs fp64 softmax attention on the fp16-rounded operands (q after the log2(e) / 8 scale, undone in fp64), incl. the key-padding mask
    (F/model/modules.py:429-434), ragged sequences, tiles that overhang a sequence, key counts that end inside either half of a 64-key tile,
    and the C2 / C1 / C5 shapes.  k_gain > 1 multiplies every key at a position = 7 mod 16 from position 40 on (never one of a query block's
    sample keys, csrc/attn3.h): logits tens to hundreds of nats above each query's maximum over its sample, which is what sends a workgroup
    of attn3 from its fixed-offset fast loop to the running-maximum redo."""
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
    out, _ = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), lens, kv, heads=heads, impl=impl)
    qb, kb, vb = (q * Q_SCALE).half().double() * math.log(2.0), k.half().double(), v.half().double()
    o, refs = 0, []
    for i, L in enumerate(lens):
        kl = L if kv is None else kv[i]
        qs, ks, vs = (t[o:o + L].view(L, heads, 64).transpose(0, 1) for t in (qb, kb, vb))
        s = qs @ ks.transpose(1, 2)
        s[:, :, kl:] = float("-inf")
        refs.append((torch.softmax(s, dim=-1) @ vs).transpose(0, 1).reshape(L, D))
        o += L
    ref = torch.cat(refs)
    # P is rounded to fp16 before the P V product (11 significand bits); the output planes carry 16 bits
    assert torch.isfinite(out).all()
    err, rel = (out.double().cpu() - ref).abs().max().item(), _rel(out, ref)
    print(f"[parity] attention lens {lens} kv {kv} heads {heads} k_gain {k_gain}: max err {err:.3e} rel rms {rel:.3e}")
    assert err < 2.5e-3
    assert rel < 5e-4


# ---------------------------------------------------------------------------------------------------------------- conv1d (BigVGAN convolutions)
def _conv_ref(x, w, bias, res, batch, P, T, dil):
    """nn.Conv1d on the valid rows of every sequence (zero padding at the sequence bounds), channel-last in / out."""
    M, ci = x.shape
    k = w.shape[-1]
    xv = x.view(batch, P, ci)[:, :T].transpose(1, 2).double()
    y = torch.nn.functional.conv1d(xv, w.double(), None if bias is None else bias.double(), dilation=dil, padding=dil * (k - 1) // 2)
    y = y.transpose(1, 2)
    if res is not None:
        y = y + res.view(batch, P, -1)[:, :T].double()
    return y


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
@pytest.mark.parametrize("x_len,c_len,x_kv", [([300], [21], None), ([1404, 257, 64], [240, 65, 7], [1404, 200, 33]), ([130, 129], [128, 1], [100, 129])])
def test_joint_attention_vs_torch(x_len, c_len, x_kv):
    """attn3's two-range kernels (keys = audio rows then text rows of the same sequence; queries from either) vs fp64 torch SDPA over
    the concatenation, padding masked on the audio keys only (F/model/modules.py:506-514).  Same operand rounding and tolerance as the
    single-range attention test."""
    from tts_indic_server_f5_amd import ops
    heads, D = 4, 256
    g = torch.Generator().manual_seed(500 + sum(x_len))
    Fx, Fc = sum(x_len), sum(c_len)
    q, k, v = (torch.randn(Fx + Fc, D, generator=g) for _ in range(3))
    out = ops.joint_attention(q.to(DEV), k.to(DEV), v.to(DEV), x_len, c_len, x_kv, heads=heads).cpu()
    bf = lambda t: t.to(torch.float16).double()
    ox, oc = 0, Fx
    worst = 0.0
    for i, (n, nt) in enumerate(zip(x_len, c_len)):
        sel = torch.cat([torch.arange(ox, ox + n), torch.arange(oc, oc + nt)])
        qq = (bf(q[sel] * Q_SCALE) * math.log(2.0)).view(n + nt, heads, 64).transpose(0, 1)
        kk = bf(k[sel]).view(n + nt, heads, 64).transpose(0, 1)
        vv = bf(v[sel]).view(n + nt, heads, 64).transpose(0, 1)
        s = qq @ kk.transpose(1, 2)
        kv = n if x_kv is None else x_kv[i]
        key_ok = torch.cat([torch.arange(n) < kv, torch.ones(nt, dtype=torch.bool)])
        s = s.masked_fill(~key_ok[None, None, :], float("-inf"))
        ref = (torch.softmax(s, dim=-1) @ vv).transpose(0, 1).reshape(n + nt, D)
        err = (out[sel].double() - ref).abs().max().item()
        worst = max(worst, err)
        ox += n; oc += nt
    print(f"[parity] joint attention x {x_len} c {c_len} kv {x_kv}: max err {worst:.3e}")
    assert worst < 2.5e-3   # fp16 P and V operands (11 significand bits) over up to ~1.6 k keys; the single-range test uses the same bound


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
