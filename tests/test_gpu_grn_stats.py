"""GRN column norms of the ConvNeXtV2 text blocks (csrc/elementwise.h grn_stats_kernel), read through the gx tap of the block's unit op.

The kernel sums a column's squares in eight partial sums -- rows r < (n & ~7) into sum r % 8 in ascending order, the tail rows into sum 0 --
one lane per partial sum, combined by the tree ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)).  Sequences of 1, 7, 8, 9 and 1404 tokens: tail
only, the longest tail, no tail, one unrolled step + tail, and the flagship length (175 steps + 4 tail rows, more than one pass of the
8-deep load loop).  Checked against float64 under test_gpu_dit_embed_ops' rule for this sum ((n + 2) u relative), and bit for bit against
that order of fused multiply-adds in fp32."""
import pytest
import torch

from test_gpu_dit_embed_ops import DEV, U, _cnx_params, _split

pytestmark = pytest.mark.gpu

SEQS = [1, 7, 8, 9, 1404]
TD = 512   # F5-TTS-Base text_dim: 1024 GRN columns = 32 workgroups per sequence
_cache = {}


def _run():
    """ty (the GELU output the kernel reads, fp32 as stored) and gx of one block over SEQS: computed once, then only read"""
    if not _cache:
        from tts_indic_server_f5_amd import ops
        g = torch.Generator().manual_seed(77)
        x = torch.randn(sum(SEQS), TD, generator=g)
        _, tp = ops.convnext_block(x.to(DEV), _cnx_params(TD, 5), seq_len=SEQS, taps=True)
        _cache["ty"], _cache["gx"] = tp["ty"], tp["gx"]
    return _cache["ty"], _cache["gx"]


def _fma32(a, t):
    """fp32 fma(t, t, a): the product of two fp32 values is exact in float64"""
    return (a.double() + t.double() * t.double()).float()


def _emulate(ys):
    """the kernel's order on fp32 rows ys [n][C]"""
    n, n8 = ys.shape[0], ys.shape[0] & ~7
    a8 = torch.zeros(8, ys.shape[1], dtype=torch.float32, device=ys.device)
    for r in range(0, n8, 8):
        a8 = _fma32(a8, ys[r:r + 8])
    for r in range(n8, n):
        a8[0] = _fma32(a8[0], ys[r])
    return (((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]))).sqrt()


@pytest.mark.parametrize("i", range(len(SEQS)), ids=[f"n{n}" for n in SEQS])
def test_grn_norms_vs_fp64(i):
    ty, gx = _run()
    n, ys = SEQS[i], _split(ty, SEQS)[i]
    ref = ys.double().norm(dim=0)
    err = (gx[i].double() - ref).abs()
    tol = (n + 2) * U * ref + 1e-30
    print(f"[parity] GRN norms n {n}: max err {err.max().item():.3e}, max err / bound {(err / tol).max().item():.3f}")
    assert torch.isfinite(gx[i]).all() and (err <= tol).all()


@pytest.mark.parametrize("i", range(len(SEQS)), ids=[f"n{n}" for n in SEQS])
def test_grn_norms_have_the_eight_partial_sum_bits(i):
    ty, gx = _run()
    want = _emulate(_split(ty, SEQS)[i])
    ndiff = (gx[i] != want).sum().item()
    print(f"[bits] GRN norms n {SEQS[i]}: {ndiff} of {want.numel()} columns differ from the eight-partial-sum order")
    assert torch.equal(gx[i], want)
