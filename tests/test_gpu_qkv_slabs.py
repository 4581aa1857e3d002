"""Every column-slab kind of the 192-column W-direct QKV kernel (csrc/gemm5.h, EPI_QKV) in one small launch, checked region by region.

A 192-column tile of the fused QKV projection is one of four kinds: its first panel is head 0 of q (rotary), it holds the Q | K boundary with
head 0 of k (rotary) behind it, it straddles K | V (its K columns leave through the row-major slab, its V columns through the transposed one,
side by side in LDS), or it is all V.  D = 256 is the smallest width whose launch has all four (N = 768 = four slabs, K | V at tile column
128); D = 512 puts K | V at tile column 64, the other compact stride.  The dispatcher (csrc/gemm_launch.h gemm5_choose) picks 192-column
tiles for these widths only once the narrower tiles need a second round on the 256 CUs: M = 8193 rows is the smallest count that selects
the 176 x 192 tile at D = 256 (47 row tiles, the last with 97 rows: neither a multiple of 16 nor of the 4-row groups), 4097 at D = 512,
7393 the smallest that selects 128 x 192 at D = 256.  The launch cannot be made smaller than that through the op, so the checks look at
one full row tile (the first) and at the partial one (the last) separately, and at the 64 columns on either side of every boundary.

Reference and tolerance: test_gpu_ops.test_qkv_unit_op's -- float64 products of the fp16-rounded operands, rotary and q scale applied, rounded
to fp16 like the outputs; an element may differ by an accumulation-order flip of its last fp16 bit (2^-10 of the region's largest value), fewer
than one element in ten does, and the relative rms stays under 4e-4.  Positions are not the row index: they restart every 1405 rows and run
backwards, so a tile's rows read scattered rows of the rotary tables."""
import pytest
import torch

from test_gpu_ops import DEV, G5_11_12, Q_SCALE, _assert_path, _ref_matmul, _rel, _reset_counters

pytestmark = pytest.mark.gpu

NPOS = 1405
G5_8_12 = ("gemm5_rb8", "gemm5_wide", "gemm5_cb12")
CASES = [
    # (M, D, tile rows, expected counters)
    (8193, 256, 176, G5_11_12),    # rotary-Q | Q + rotary-K | K + V (boundary at tile column 128) | all V
    (4097, 512, 176, G5_11_12),    # 8 slabs; K | V at tile column 64 of slab 5
    (7393, 256, 128, G5_8_12),     # the 128-row instance of the same kernel: the transposed slab starts right behind the row-major one
]
_cache = {}


def _case(M, D):
    """inputs, reference q / k / v (float, before the fp16 rounding) and the op's outputs: computed once per shape, then only read"""
    if (M, D) not in _cache:
        from oracle import dit_oracle as O
        from tts_indic_server_f5_amd import ops
        g = torch.Generator().manual_seed(3 * M + D)
        a = torch.randn(M, D, generator=g)
        w = torch.randn(3 * D, D, generator=g) / D ** 0.5
        bias = torch.randn(3 * D, generator=g) * 0.1
        pos = (NPOS - 1) - torch.arange(M) % NPOS
        y = (_ref_matmul(a, w, 3) + bias.double()).float()
        q, k, v = y[:, :D].clone(), y[:, D:2 * D].clone(), y[:, 2 * D:]
        freqs = O.rotary_freqs(NPOS, 64)[0][pos]
        q[:, :64] = O.apply_rotary(q[None, :, :64], freqs[None])[0]
        k[:, :64] = O.apply_rotary(k[None, :, :64], freqs[None])[0]
        q = q * Q_SCALE
        _reset_counters()
        gq, gk, gv, _ = ops.qkv(a.to(DEV), w.to(DEV), bias, pos.numpy(), prec=3)
        counters_ok = None
        try:
            _assert_path(_cache_expected[(M, D)])
        except AssertionError as e:   # reported by the test that asks for it, not by whichever test filled the cache
            counters_ok = str(e)
        _cache[(M, D)] = (torch.cat([q, k, v], 1), torch.cat([gq.cpu(), gk.cpu(), gv.cpu()], 1), counters_ok)
    return _cache[(M, D)]


_cache_expected = {(c[0], c[1]): c[3] for c in CASES}


def _check(tag, got, ref):
    err = (got - ref.half().float()).abs()
    frac = (err > 0).float().mean().item()
    rel = _rel(got, ref.double())
    print(f"[parity] qkv slabs {tag}: max err {err.max().item():.3e} (bound {2.0 ** -10 * ref.abs().max().item():.3e}), "
          f"differing {frac:.4f}, rel rms {rel:.3e}")
    assert torch.isfinite(got).all(), tag
    assert err.max() <= 2.0 ** -10 * ref.abs().max(), tag
    assert frac < 0.10, tag
    assert rel < 4e-4, tag


def _regions(D):
    """(name, first column, last column + 1) in the concatenated [q | k | v] columns: every column slab, and the 64 columns on either
    side of every boundary (rotary | plain inside q and k, Q | K, K | V, slab | slab)"""
    N = 3 * D
    out = [(f"slab {s}", s * 192, (s + 1) * 192) for s in range(N // 192)]
    edges = {64: "rotary q | q", D: "q | rotary k", D + 64: "rotary k | k", 2 * D: "k | v"}
    edges.update({s * 192: edges.get(s * 192, f"slab {s - 1} | slab {s}") for s in range(1, N // 192)})
    for c, name in sorted(edges.items()):
        out.append((name + " (left)", c - 64, c))
        out.append((name + " (right)", c, c + 64))
    return out


@pytest.mark.parametrize("M,D,rows,counters", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_qkv_slab_path(M, D, rows, counters):
    """the launch under test is the 192-column kernel of the expected tile height, alone"""
    assert _case(M, D)[2] is None, _case(M, D)[2]
    assert M % rows != 0 and (M % rows) % 4 != 0    # the last row tile is partial, and so is its last 4-row group


@pytest.mark.parametrize("M,D,rows,counters", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
@pytest.mark.parametrize("which", ["full", "partial", "all"])
def test_qkv_slab_regions(M, D, rows, counters, which):
    """every slab and every boundary neighbourhood, over the first (full) row tile, the last (partial) one, and all rows"""
    ref, got, _ = _case(M, D)
    r0, r1 = {"full": (0, rows), "partial": (M - M % rows, M), "all": (0, M)}[which]
    for name, c0, c1 in _regions(D):
        _check(f"M {M} D {D} rows {r0}..{r1 - 1} {name} [{c0}, {c1})", got[r0:r1, c0:c1], ref[r0:r1, c0:c1])


@pytest.mark.parametrize("M,D,rows,counters", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_qkv_partial_tile_stays_inside_its_rows(M, D, rows, counters):
    """The output buffers hold M_pad = ceil128(M) rows (q | k) and token columns (V, transposed): a sentinel in the padding behind row M
    must survive the launch, and the real rows must come out with the bits of the first run."""
    import ctypes as C

    import numpy as np
    from tts_indic_server_f5_amd import _lib, ops
    g = torch.Generator().manual_seed(3 * M + D)
    a = torch.randn(M, D, generator=g).to(DEV)
    w = (torch.randn(3 * D, D, generator=g) / D ** 0.5).to(DEV)
    bias = (torch.randn(3 * D, generator=g) * 0.1).to(DEV)
    pos = np.ascontiguousarray(((NPOS - 1) - np.arange(M) % NPOS).astype(np.int32))
    M_pad = (M + 127) // 128 * 128
    qk = torch.full((M_pad, 2 * D), 7.0, device=DEV, dtype=torch.float16)
    vt = torch.full((D, M_pad), 7.0, device=DEV, dtype=torch.float16)
    us = C.c_double(0.0)
    _lib.check(_lib.lib().f5hip_op_qkv(M, D, ops._p(a), ops._p(w), ops._p(bias), ops._p(pos), 3, ops._p(qk), ops._p(vt), 0, C.byref(us),
                                       _lib.current_stream_ptr()), "f5hip_op_qkv")
    torch.cuda.synchronize()
    assert (qk[M:] == 7.0).all(), "q | k rows behind M were written"
    # V is stored four tokens at a time (a group that starts in front of M is stored whole), and vt_col (csrc/common.h) permutes whole
    # groups of four inside aligned groups of 16: every token column from the next multiple of 4 on must be untouched
    t = torch.arange(M_pad, device=DEV)
    col = (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)
    assert (vt[:, col[(M + 3) // 4 * 4:]] == 7.0).all(), "V token columns behind M were written"
    _, got, _ = _case(M, D)
    assert torch.equal(torch.cat([qk[:M, :D], qk[:M, D:], vt[:, col[:M]].t()], 1).float().cpu(), got)
