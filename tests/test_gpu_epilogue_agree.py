""""which kernel computed a row cannot change its bits".  gemm6 (batch mode, epilogue straight from the accumulators) and
gemm5 (one utterance, epilogue through an LDS slab) share the k order of every dot product and the per-element epilogue arithmetic
(csrc/gemm_epilogue.h g5_epi_value; the stores and the rotary pair of gemm5.h / gemm6.h), so the same rows through either kernel must be EQUAL, bit for bit.  Each case
runs one launch large enough for gemm6 and one over its first rows that the dispatcher gives to gemm5 (both asserted by the launch counters).
Interior tiles only: ragged last tiles are the fp64 tests' (test_gpu_ops.py); gemm.h / gemm3.h use another k order and are not expected to match."""
import pytest
import torch

from test_gpu_ops import DEV, _counter, _reset_counters

pytestmark = pytest.mark.gpu

M6, M5 = 14336, 1408   # 56 row tiles of 256 x (N / 256 >= 4) = 224 tiles, the fewest gemm6 takes; 1408 = 8 x 176 = 11 x 128 rows of gemm5


def _took(kernel):
    g6, g5 = _counter("gemm6"), _counter("gemm5_rb11") + _counter("gemm5_rb8")
    assert (g6, g5) == ((1, 0) if kernel == "gemm6" else (0, 1)), f"expected one {kernel} launch: gemm6 {g6}, gemm5 {g5}"


def _gemm_pair(N, **kw):
    from tts_indic_server_f5_amd import ops
    K = 128
    g = torch.Generator().manual_seed(N)
    a = torch.randn(M6, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    bias = torch.randn(N, generator=g) * 0.1
    res = kw.pop("res", None)
    if res is not None:
        res = torch.randn(M6, N, generator=g).to(DEV)
    mul = torch.randn(N, generator=g) if kw.pop("mul", False) else None
    _reset_counters()
    big, _ = ops.gemm(a, w, bias, prec=3, mul=mul, res=res, **kw)
    _took("gemm6")
    _reset_counters()
    small, _ = ops.gemm(a[:M5].contiguous(), w, bias, prec=3, mul=mul, res=None if res is None else res[:M5].contiguous(), **kw)
    _took("gemm5")
    return big[:M5], small


def test_residual_epilogue_agrees():
    """bias, AdaLN gate and residual, fp32 out (the out / FF2 projections)."""
    big, small = _gemm_pair(1024, mul=True, res=True)
    assert torch.equal(big, small)


def test_f16_plane_epilogue_agrees():
    """GELU and the saturated fp16 plane (FF1)."""
    big, small = _gemm_pair(2048, act="gelu_tanh", out16=True)
    assert torch.equal(big, small)


def test_qkv_epilogue_agrees():
    """rotary head 0, the softmax scale on q, transposed V: 25 x 9 = 225 gemm6 tiles against the first 1024 rows through gemm5."""
    from tts_indic_server_f5_amd import ops
    M, D, m5 = 6400, 768, 1024
    g = torch.Generator().manual_seed(M + D)
    a = torch.randn(M, D, generator=g).to(DEV)
    w = (torch.randn(3 * D, D, generator=g) / D ** 0.5).to(DEV)
    bias = torch.randn(3 * D, generator=g) * 0.1
    pos = (torch.arange(M) % 1405).numpy()
    _reset_counters()
    q6, k6, v6, _ = ops.qkv(a, w, bias, pos, prec=3)
    _took("gemm6")
    _reset_counters()
    q5, k5, v5, _ = ops.qkv(a[:m5].contiguous(), w, bias, pos[:m5], prec=3)
    _took("gemm5")
    for name, big, small in (("q", q6, q5), ("k", k6, k5), ("v", v6, v5)):
        assert torch.equal(big[:m5], small), name
