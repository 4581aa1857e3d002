"""The DiT's proj_out as a unit-op case: N = mel_dim = 100 (padded to one 128-column tile), K = 1024, no activation, fp32 rows out.

At one utterance this GEMM is a single column of row tiles (22 workgroups at M = 2816), so its row-tile height decides how much of the chip
it uses.  The case is kept small and tile-height agnostic: M = 145 rows = one 128-row tile of today's kernels plus a partial one of 17 rows
(not a multiple of 16, of 4 or of any MFMA block height), against float64 on the operand values the kernel multiplies, under
test_gpu_ops.test_gemm_unit_op's rule for a GEMM without activation: 2e-5 relative rms.  The rows of the full tile, the rows of the partial
tile and the last real columns (96 .. 99, in front of the 28 padding columns) are checked separately."""
import pytest
import torch

from test_gpu_ops import DEV, G3, G5_8_4, _assert_path, _ref_matmul, _rel, _reset_counters

pytestmark = pytest.mark.gpu

M, N, K = 145, 100, 1024


@pytest.mark.parametrize("prec,counters", [(2, G3), (3, G5_8_4)], ids=["split-bf16", "fp16"])
def test_proj_out_shaped_gemm(prec, counters):
    from tts_indic_server_f5_amd import ops
    g = torch.Generator().manual_seed(100 + prec)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g) * 0.1
    ref = _ref_matmul(a, w, prec) + bias.double()
    _reset_counters()
    out, _ = ops.gemm(a.to(DEV), w.to(DEV), bias, prec=prec, act="none")
    _assert_path(counters)
    assert out.shape == (M, N) and torch.isfinite(out).all()
    for name, rs, cs in (("full tile", slice(0, 128), slice(0, N)), ("partial tile", slice(128, M), slice(0, N)),
                         ("last real columns", slice(0, M), slice(96, N)), ("all", slice(0, M), slice(0, N))):
        rel = _rel(out[rs, cs].float(), ref[rs, cs])
        print(f"[parity] proj_out-shaped gemm prec {prec} {name}: rel rms {rel:.3e} (bound 2e-5)")
        assert rel < 2e-5, name
