"""GPU tests of the MXFP8 block GEMM (csrc/gemm8.h; prec = 4 of the unit ops, gemm_planes = 4 of the model): the kernel against float64 on
the operands tests/mxfp8_ref.py quantises, and the mode end to end against the reference's fixtures."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import mxfp8_ref as R  # noqa: E402
from test_gpu_dit import MMTINY, TINY, UTINY, _load  # noqa: E402
from test_gpu_ops import _counter, _reset_counters  # noqa: E402
from tts_indic_server_f5_amd import synth  # noqa: E402

DEV = "cuda:0"


def _wide(rows, K, g):
    """randn with every 32-wide K block of every row multiplied by 2^u, u in -12 .. 12: the block scales matter"""
    u = torch.randint(-12, 13, (rows, K // 32), generator=g).double()
    return (torch.randn(rows, K, generator=g).double() * (2.0 ** u).repeat_interleave(32, 1)).float()


def _dq(x):
    return torch.from_numpy(R.dequant(*R.quant(x.double().numpy())))


_OPERANDS = {}


def _operands(M, N, K):
    """(a, w, Aq, Wq, bias, mul, res, table, row_mod) per shape, built once: Aq / Wq = what the kernel multiplies"""
    if (M, N, K) not in _OPERANDS:
        g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
        a, w = _wide(M, K, g), _wide(N, K, g) / K ** 0.5
        _OPERANDS[(M, N, K)] = (a, w, _dq(a.half()), _dq(w), torch.randn(N, generator=g) * 0.1, torch.randn(N, generator=g),
                                torch.randn(M, N, generator=g), torch.randn(3, N + 8, generator=g), torch.randint(0, 3, (M,), generator=g))
    return _OPERANDS[(M, N, K)]


# the last: N padded to no multiple of 256 selects the 128-column tile instance (the kernel has no instances chosen by M)
SHAPES = [(40, 1024, 1024), (257, 2048, 1024), (300, 1024, 2048), (1, 1024, 4096), (70, 384, 1024)]
EPILOGUES = ["none", "bias_gelu_f16", "gate_res", "rowmul", "row_keep"]


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M%d_N%d_K%d" % s)
def test_unit_gemm_vs_fp64_of_quantised_operands(shape, epi):
    """|out - ref| <= K 2^-23 (|Aq| @ |Wq|^T) + eps.  The products of two E4M3 values and two power-of-two scales are exact in fp32; what remains
    is fp32 accumulation over at most K terms, unit roundoff taken as 2^-23 (an adder that truncates).  eps, the epilogue's own allowance as in
    tests/test_gpu_ops.py: 2^-22 of every term of the fp32 epilogue (its few roundings), 3e-4 of the activation's value for the hardware
    exp2 / rcp of GELU (whose slope, at most 1.13, also scales the accumulation bound), 2^-10 relative + 2^-24 for the fp16 plane.
    Measured on an MI355X: max err / bound 0.34 - 0.40 at K = 1024, 0.21 at K = 2048, 0.06 at K = 4096 -- an error of ~2^-14.6 of
    |Aq| @ |Wq|^T whatever K is, i.e. the instruction does not keep every product exactly: with these inputs (block scales 2^24 apart inside
    one 128-deep step) it loses what lies ~15 bits below the step's largest product.  The bound holds at every K the block
    GEMMs of Base, Small and E2 have; at K = 128 it would not (2.7 measured), which is why the one-step case below uses exact integers."""
    from tts_indic_server_f5_amd import ops
    M, N, K = shape
    a, w, Aq, Wq, bias, mul, res, table, row_mod = _operands(M, N, K)
    acc = Aq @ Wq.T
    tol = K * 2.0 ** -23 * (Aq.abs() @ Wq.abs().T)
    keep = None
    _reset_counters()
    if epi == "none":
        out, _ = ops.gemm(a.to(DEV), w.to(DEV), None, prec=4)
        ref, tol = acc, tol + 2.0 ** -22 * acc.abs()
    elif epi == "bias_gelu_f16":
        out, _ = ops.gemm(a.to(DEV), w.to(DEV), bias, prec=4, act="gelu_tanh", out16=True)
        ref = torch.nn.functional.gelu(acc + bias.double(), approximate="tanh")
        tol = 1.13 * (tol + 2.0 ** -22 * (acc.abs() + bias.abs())) + 3e-4 * ref.abs() + 2.0 ** -10 * ref.abs() + 2.0 ** -24
        ref = ref.clamp(-65504.0, 65504.0)   # the fp16 plane saturates (include/f5hip.h); clamping moves no value further from its reference
    else:
        if epi == "row_keep":
            keep = torch.ones(M, dtype=torch.bool)
            keep[M // 2] = False
        m = table[row_mod, 4:4 + N].double() if epi == "rowmul" else mul.double()[None].expand(M, N)
        pre = (acc + bias.double()) * (1.0 if keep is None else keep.double()[:, None])
        ref = pre * m + res.double()
        tol = (tol + 2.0 ** -22 * (acc.abs() + bias.abs())) * m.abs() + 2.0 ** -22 * ((pre * m).abs() + res.abs() + ref.abs())
        if epi == "rowmul":
            out = ops.gemm_rowmul(a.to(DEV), w.to(DEV), bias, table.to(DEV), 4, row_mod, res, prec=4)
        else:
            out, _ = ops.gemm(a.to(DEV), w.to(DEV), bias, prec=4, mul=mul, res=res, row_keep=keep)
        if keep is not None:
            assert torch.equal(out[M // 2].cpu(), res[M // 2])
    assert _counter("gemm8") > 0
    err = (out.double().cpu() - ref).abs()
    print(f"[mxfp8] gemm M{M} N{N} K{K} {epi}: max err {err.max():.3e}, max err / bound {(err / tol).max():.3e}")
    assert torch.isfinite(out).all() and (err <= tol).all()


def test_one_k_step_exact_integers():
    """K = 128 (the tiny models' width: fewer k-steps than ring stages), partial row and column tiles: operands of small integers, every code
    and every product exact and within 4 bits of each other, so the output is A @ W^T to the bit"""
    from tts_indic_server_f5_amd import ops
    g = torch.Generator().manual_seed(2)
    a, w = torch.randint(-3, 4, (70, 128), generator=g).float(), torch.randint(-3, 4, (384, 128), generator=g).float()
    out, _ = ops.gemm(a.to(DEV), w.to(DEV), None, prec=4)
    assert torch.equal(out.cpu(), a @ w.T)


def test_rows_do_not_depend_on_their_neighbours():
    from tts_indic_server_f5_amd import ops
    a, w = _operands(300, 1024, 2048)[:2]
    big, _ = ops.gemm(a.to(DEV), w.to(DEV), None, prec=4)
    small, _ = ops.gemm(a[:40].to(DEV), w.to(DEV), None, prec=4)
    assert torch.equal(big[:40], small)


def test_nan_stays_in_its_row():
    from tts_indic_server_f5_amd import ops
    a, w = _operands(257, 2048, 1024)[:2]
    clean, _ = ops.gemm(a.to(DEV), w.to(DEV), None, prec=4)
    bad = a.clone()
    bad[100, 517] = float("nan")
    out, _ = ops.gemm(bad.to(DEV), w.to(DEV), None, prec=4)
    ok = torch.arange(257) != 100
    assert torch.isnan(out[100]).all() and torch.equal(out[ok], clean[ok])


def test_uncovered_shape_takes_the_fp16_path():
    from tts_indic_server_f5_amd import ops
    g = torch.Generator().manual_seed(11)
    a, w = torch.randn(200, 96, generator=g).to(DEV), torch.randn(1024, 96, generator=g).to(DEV)
    _reset_counters()
    out4, _ = ops.gemm(a, w, None, prec=4)
    assert _counter("gemm8") == 0
    out3, _ = ops.gemm(a, w, None, prec=3)
    assert torch.equal(out4, out3)


# ---------------------------------------------------------------- gemm_planes = 4 end to end
# rms error against the reference's fixtures: 1.5 x the value measured on an MI355X, rounded up to two digits (DESIGN.md "MXFP8 block GEMMs")
# measured: dit_tiny 2.934e-2, dit_small 4.486e-2, cfm_tiny 2.299e-2, unett_tiny 6.141e-2, mmdit_tiny 3.688e-2
CAPS = {"dit_tiny": 4.5e-2, "dit_small": 6.8e-2, "cfm_tiny": 3.5e-2, "unett_tiny": 9.3e-2, "mmdit_tiny": 5.6e-2}


def _rms(tag, got, ref):
    e = (got.float().cpu() - ref.float().cpu()).pow(2).mean().sqrt().item()
    print(f"[mxfp8] {tag}: rms err {e:.3e} (cap {CAPS[tag]:.1e})")
    return e


def _model(name):
    from tts_indic_server_f5_amd import model as Mo
    if name in ("dit_tiny", "cfm_tiny"):
        return Mo.F5HipModel(Mo.DiTArch(**TINY), synth.dit_state_dict(**TINY), gemm_planes=4)
    if name == "dit_small":
        return Mo.F5HipModel(Mo.F5TTS_SMALL, synth.dit_state_dict(dim=768, depth=18, heads=12), gemm_planes=4)
    if name == "unett_tiny":
        return Mo.F5HipModel(Mo.UNetTArch(**UTINY), synth.unett_state_dict(**UTINY), gemm_planes=4)
    return Mo.F5HipModel(Mo.MMDiTArch(**MMTINY), synth.mmdit_state_dict(**MMTINY), gemm_planes=4)


@pytest.mark.parametrize("name", sorted(CAPS))
def test_mode_4_end_to_end(golden_dir, name, attn_shape_invariant):
    m = _model(name)
    _reset_counters()
    if name == "cfm_tiny":
        g = _load(golden_dir, "cfm_sample_tiny")
        out, _ = m.sample(g["cond1"], g["text1"], 48, steps=16, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=7)
        ref = g["s16_swm1_cfg2_b1_out"]
        assert torch.equal(out[:, :17].cpu(), ref[:, :17])   # conditioning frames are copied exactly
        out, ref = out[:, 17:], ref[:, 17:]
    else:
        g = _load(golden_dir, {"dit_tiny": "dit_tiny_forward", "dit_small": "dit_small_forward"}.get(name, name))
        x, cond, text = g["x"][:1], g["cond"][:1], g["text"][:1]
        t = 0.5 if name == "dit_small" else float(g["time"])
        ref = g[{"dit_tiny": "out_b1_cond", "mmdit_tiny": "out_b1_cond"}.get(name, "out_cond")][:1]
        out = m.transformer_forward(x, cond, text, t, False, False)
        two = m.transformer_forward(x.repeat(2, 1, 1), cond.repeat(2, 1, 1), text.repeat(2, 1), t, False, False)
        assert torch.equal(two[0], out[0]) and torch.equal(two[1], out[0])   # copies == single
    assert _counter("gemm8") > 0
    assert torch.isfinite(out).all()
    assert _rms(name, out, ref) < CAPS[name]
