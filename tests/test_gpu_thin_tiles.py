"""The thin (32-row) instance of the warp-specialised GEMM (csrc/gemm3.h gemm3_thin_kernel), which the dispatcher takes for generic-epilogue
launches whose 128-row grid has few workgroups (csrc/f5hip.hip kThinMaxTiles128).

- parity against float64 on the operand values, under test_gpu_ops.test_gemm_unit_op's rules (2e-5 relative rms without activation or with
  the erf GELU, 3e-4 with SiLU / tanh GELU, 6e-4 and two fp16 ulps of the largest value for the fp16 plane), region by region: the full
  32-row tiles, the partial last tile, and the columns of the last 64-column epilogue slab up to the last real column.  K = 32, 96 and 160
  are 1, 3 and 5 k-steps of the 4-stage ring; prec 1 and 3 (one operand plane) take the 10-piece stage that four loader waves do not divide.
- bit equality across instances: the first 145 rows of a launch large enough for the 128-row instance equal the thin launch of those rows.
- the rows behind M, and with them the padding columns of the last real row, keep their sentinel."""
import ctypes as C

import pytest
import torch

from test_gpu_ops import DEV, _act, _counter, _ref_matmul, _rel, _reset_counters

pytestmark = pytest.mark.gpu

SHAPES = [
    # (M, N, K, prec)
    (145, 100, 1024, 2),   # proj_out's width: partial row tile (17 rows), partial column panel
    (33, 512, 1536, 2),    # Vocos pwconv2's K; one row in the second tile
    (1, 128, 32, 2),       # one row, one k-step
    (32, 128, 96, 2),      # exactly one tile, three k-steps (the ring never wraps)
    (65, 256, 160, 2),     # five k-steps: the ring wraps once
    (1, 128, 32, 3), (32, 128, 96, 3), (65, 256, 160, 3),   # fp16 planes (K % 64 != 0 keeps them on gemm3)
    (65, 256, 160, 1),     # plain bf16
]
ACTS = ["none", "silu", "gelu_tanh", "gelu_erf"]
VARIANTS = ["plain", "res", "f16"]   # fp32 out; gated residual (mul + res), fp32 out; one fp16 plane out


def _inputs(M, N, K, prec, seed=0):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + prec + seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g) * 0.1
    mul = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    return a, w, bias, mul, res


def _regions(M, N):
    out = []
    if M >= 32:
        out.append(("full tiles", slice(0, M // 32 * 32), slice(0, N)))
    if M % 32:
        out.append(("partial tile", slice(M // 32 * 32, M), slice(0, N)))
    out.append(("last columns", slice(0, M), slice((N - 1) // 64 * 64, N)))
    return out


@pytest.mark.parametrize("M,N,K,prec", SHAPES, ids=[f"M{s[0]}_N{s[1]}_K{s[2]}_p{s[3]}" for s in SHAPES])
def test_thin_instance_vs_fp64(M, N, K, prec):
    from tts_indic_server_f5_amd import ops
    a, w, bias, mul, res = _inputs(M, N, K, prec)
    pre = _ref_matmul(a, w, prec) + bias.double()
    for act in ACTS:
        for variant in VARIANTS:
            ref = _act(pre, act)
            if variant == "res":
                ref = ref * mul.double() + res.double()
            _reset_counters()
            out, _ = ops.gemm(a.to(DEV), w.to(DEV), bias, prec=prec, act=act, mul=mul if variant == "res" else None,
                              res=res if variant == "res" else None, out16=variant == "f16")
            assert _counter("gemm3") == 1 and _counter("gemm3_thin") == 1, "the launch did not take the thin instance"
            assert torch.isfinite(out).all()
            for name, rs, cs in _regions(M, N):
                got, want = out[rs, cs].float(), ref[rs, cs]
                rel = _rel(got, want)
                print(f"[parity] thin gemm M{M} N{N} K{K} prec {prec} {act} {variant} {name}: rel rms {rel:.3e}")
                if variant == "f16":
                    assert rel < 6e-4, (act, variant, name)
                    assert (got.cpu() - want.half().float()).abs().max() <= 2 * torch.finfo(torch.float16).eps * ref.abs().max(), (act, variant, name)
                else:
                    assert rel < (3e-4 if act in ("gelu_tanh", "silu") else 2e-5), (act, variant, name)


@pytest.mark.parametrize("K,prec", [(1024, 2), (96, 3)], ids=["K1024_p2", "K96_p3"])
def test_rows_have_the_same_bits_on_both_instances(K, prec):
    """145 rows alone (two 128-row tiles: thin) and as the first rows of 3200 (100 tiles of 128 x 128: the 128-row instance)."""
    from tts_indic_server_f5_amd import ops
    M, MB, N = 145, 3200, 512
    a, w, bias, mul, res = _inputs(MB, N, K, prec, seed=1)
    a, w, res = a.to(DEV), w.to(DEV), res.to(DEV)
    for act, variant in [("none", "res"), ("none", "plain"), ("silu", "plain"), ("gelu_tanh", "f16")]:
        kw = dict(prec=prec, act=act, mul=mul if variant == "res" else None, out16=variant == "f16")
        _reset_counters()
        big, _ = ops.gemm(a, w, bias, res=res if variant == "res" else None, **kw)
        assert _counter("gemm3") == 1 and _counter("gemm3_thin") == 0, "the large launch must take the 128-row instance"
        _reset_counters()
        thin, _ = ops.gemm(a[:M].contiguous(), w, bias, res=res[:M].contiguous() if variant == "res" else None, **kw)
        assert _counter("gemm3") == 1 and _counter("gemm3_thin") == 1
        ndiff = (big[:M] != thin).sum().item()
        print(f"[bits] thin vs 128-row instance K{K} prec {prec} {act} {variant}: {ndiff} differing elements")
        assert torch.equal(big[:M], thin), (act, variant)


@pytest.mark.parametrize("out16", [False, True], ids=["f32", "f16"])
def test_thin_partial_tile_stays_inside_its_rows(out16):
    """The output is given M_pad rows of pitch N = 100 filled with a sentinel: the rows behind M survive (the padding columns 100 .. 127 of
    the last real row would land in them), and the real rows have the bits of the plain call."""
    from tts_indic_server_f5_amd import _lib, ops
    M, N, K, prec = 145, 100, 1024, 2
    a, w, bias, _, _ = _inputs(M, N, K, prec, seed=2)
    a, w, bias = a.to(DEV), w.to(DEV), bias.to(DEV)
    want, _ = ops.gemm(a, w, bias, prec=prec, out16=out16)
    M_pad = (M + 127) // 128 * 128
    out = torch.full((M_pad, N), 7.0, device=DEV, dtype=torch.float16 if out16 else torch.float32)
    us = C.c_double(0.0)
    _reset_counters()
    _lib.check(_lib.lib().f5hip_op_gemm(M, N, K, ops._p(a), ops._p(w), ops._p(bias), prec, ops.ACT["none"], None, None, None,
                                        None if out16 else ops._p(out), ops._p(out) if out16 else None, 1, 0, C.byref(us),
                                        _lib.current_stream_ptr(), 128), "f5hip_op_gemm")
    torch.cuda.synchronize()
    assert _counter("gemm3_thin") == 1
    assert (out[M:] == 7.0).all(), "rows behind M were written"
    assert torch.equal(out[:M], want)
