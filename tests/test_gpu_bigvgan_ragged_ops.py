"""GPU: the ragged forms of the BigVGAN generator's kernels, alone, through the ragged unit ops (include/f5hip.h): the convolutions reading
their sequence bounds from per-block tables (conv5_kernel, the CONV form of gemm_kernel), aa_snake2_kernel and the two conv_post kernels
taking `items` / `scale`, and the two kernels without a uniform op of their own (bv_mean3_kernel, bv_mel_rows(_ragged)_kernel).

Every item of a ragged launch is compared (1) bit for bit with the uniform op on that item alone at its own pitch -- the same kernel instance
and the same summation order, which the whole-generator test tests/test_gpu_bigvgan_ragged.py relies on -- and (2) with float64 under the
bound of the uniform test of the same kernel.  Padding rows hold NaN, neighbouring items hold different data, outputs the kernel must not
write are pre-filled with a sentinel."""
import math

import pytest
import torch

from bigvgan_ref import (CONV_TOL, DEV, SENTINEL, SNAKE_FORMATS, U32, check_untouched_items, conv_counters, conv_ref, report, reset_counters,
                         snake_bound, snake_ref, ups_ref)
from row_ops_ref import fmt_f16, fmt_split

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _layout(frames, scale, pitch_align=128):
    """rows of the ragged forward at the stage of up-sampling `scale`: item pitch ceil(frames / pitch_align) pitch_align scale, frames scale valid"""
    row0, rows, valid, r = [], [], [], 0
    for f in frames:
        p = (f + pitch_align - 1) // pitch_align * pitch_align * scale
        row0.append(r); rows.append(p); valid.append(f * scale)
        r += p
    return row0, rows, valid, r


def _nan_padding(t, row0, rows, valid):
    for r0, p, v in zip(row0, rows, valid):
        t[r0 + v: r0 + p] = NAN
    return t


# ---------------------------------------------------------------------------------------------------------------- convolutions
CONV_FRAMES = [1, 127, 128, 129, 300, 37]


def _check_conv_items(tag, prec, got, row0, rows, valid, alone, ref64):
    """got [M, co] of the ragged op; per item: alone(i) = the uniform op's valid rows, ref64(i) = float64"""
    for i, (r0, v) in enumerate(zip(row0, valid)):
        g = got[r0: r0 + v]
        assert torch.isfinite(g).all(), f"{tag} item {i}: a padding row (NaN) reached a valid output"
        if alone is not None:
            a = alone(i)
            assert torch.equal(g, a), f"{tag} item {i} (rows {r0} + {v}): differs from the uniform op, max {(g - a).abs().max().item():.3e}"
        err = (g.double() - ref64(i)).abs().max().item()
        print(f"[parity] {tag} item {i} rows {r0}+{v}/{rows[i]}: max err {err:.3e} (bound {CONV_TOL[prec]:.0e}), "
              f"{'bit-equal to the uniform op' if alone is not None else 'no uniform op of this impl'}")
        assert err < CONV_TOL[prec], f"{tag} item {i}"


def _conv_case(tag, frames, scale, blk, ci, co, k, dil, prec, impl, pitch_align=128):
    from tts_indic_server_f5_amd import ops
    row0, rows, valid, M = _layout(frames, scale, pitch_align)
    g = torch.Generator().manual_seed(5000 + 7 * ci + 31 * k + dil + scale)
    x = _nan_padding(torch.randn(M, ci, generator=g), row0, rows, valid)
    w = torch.randn(co, ci, k, generator=g) / (ci * k) ** 0.5
    bias = torch.randn(co, generator=g)
    res = _nan_padding(torch.randn(M, co, generator=g), row0, rows, valid)
    expect = "conv5" if impl == 5 else ("gemm_reg_bn64" if co <= 64 else "gemm_reg_bn128")
    reset_counters()
    got = ops.conv1d_ragged(x.to(DEV), w, bias, res.to(DEV), row0=row0, rows=rows, valid=valid, blk=blk, dilation=dil, prec=prec, impl=impl).cpu()
    ran = conv_counters()
    assert ran == {n: int(n == expect) for n in ran}, (tag, ran)

    def alone(i):
        sl = slice(row0[i], row0[i] + rows[i])
        out, _, _ = ops.conv1d(x[sl].to(DEV), w, bias, res[sl].to(DEV), batch=1, valid=valid[i], dilation=dil, prec=prec, impl=impl)
        return out.cpu()[: valid[i]]

    def ref64(i):
        sl = slice(row0[i], row0[i] + rows[i])
        return conv_ref(x[sl], w, bias, res[sl], 1, rows[i], valid[i], dil)[0]

    _check_conv_items(f"conv1d ragged {tag} scale {scale} blk {blk} ci {ci} co {co} k {k} dil {dil} prec {prec} impl {impl}", prec, got, row0, rows, valid,
                      alone, ref64)


@pytest.mark.parametrize("impl", [5, 0])
@pytest.mark.parametrize("prec", [2, 3])
@pytest.mark.parametrize("k,dil", [(11, 5), (7, 3), (3, 1)])
@pytest.mark.parametrize("scale,blk,ch", [(2, 256, 96), (8, 1024, 48), (8, 1024, 24)])
def test_conv_ragged_stage(scale, blk, ch, k, dil, prec, impl):
    """the AMPBlock1 convolutions of a later stage: one table entry per 128 scale rows, items of 1 ... 300 first-stage frames"""
    _conv_case("stage", CONV_FRAMES, scale, blk, ch, ch, k, dil, prec, impl)


@pytest.mark.parametrize("prec", [2, 3])
@pytest.mark.parametrize("impl,frames", [(5, [129, 256, 300, 200]), (0, [129, 256, 300, 200])])
def test_conv_ragged_first_stage_aligned(impl, frames, prec):
    """conv_pre's shape (c_in 100, k 7, c_out 256) over first-stage rows, blk 128, items of 256-aligned pitch: a 256-row tile of conv5 spans
    two table entries"""
    _conv_case("first stage, 256-aligned items", frames, 1, 128, 100, 256, 7, 1, prec, impl, pitch_align=256)


@pytest.mark.parametrize("prec", [2, 3])
def test_conv_ragged_first_stage_pitch_128(prec):
    """the items the generator leaves to gemm.h: pitch 128 and 384 beside the 256-aligned ones (impl 0 only)"""
    _conv_case("first stage, pitch-128 items", [129, 1, 256, 127, 300, 128, 200], 1, 128, 100, 256, 7, 1, prec, 0)


@pytest.mark.parametrize("impl", [5, 0])
@pytest.mark.parametrize("prec", [2, 3])
def test_upsample_ragged(prec, impl):
    """ups (96 -> 48, r = 2) in its 3-tap form at scale 2.  The uniform op takes the generator's dispatch, conv5.h at these pitches, so the
    bit comparison is made for impl 5; impl 0 is compared with float64 only."""
    from tts_indic_server_f5_amd import ops
    ci, co, r, scale, blk = 96, 48, 2, 2, 256
    row0, rows, valid, M = _layout(CONV_FRAMES, scale)
    g = torch.Generator().manual_seed(5100 + prec)
    x = _nan_padding(torch.randn(M, ci, generator=g), row0, rows, valid)
    w = torch.randn(ci, co, 2 * r, generator=g) / math.sqrt(2 * ci)
    bias = torch.randn(co, generator=g)
    expect = "conv5" if impl == 5 else "gemm_reg_bn128"   # r co = 96 columns: weights padded to 128 rows
    reset_counters()
    got = ops.conv1d_ragged(x.to(DEV), w, bias, row0=row0, rows=rows, valid=valid, blk=blk, prec=prec, impl=impl, ups_rate=r).cpu()
    ran = conv_counters()
    assert ran == {n: int(n == expect) for n in ran}, ran
    assert got.shape == (M * r, co)

    def alone(i):
        sl = slice(row0[i], row0[i] + rows[i])
        reset_counters()
        out = ops.bigvgan_upsample(x[sl].to(DEV), w, bias, batch=1, valid=valid[i], rate=r, prec=prec).cpu()
        assert conv_counters()["conv5"] == 1
        return out[: valid[i] * r]

    def ref64(i):
        sl = slice(row0[i], row0[i] + rows[i])
        return ups_ref(x[sl], w, bias, 1, rows[i], valid[i], r)[0]

    up = lambda v: [e * r for e in v]
    _check_conv_items(f"upsample ragged ci {ci} co {co} r {r} scale {scale} prec {prec} impl {impl}", prec, got, up(row0), up(rows), up(valid),
                      alone if impl == 5 else None, ref64)


def test_conv_ragged_refuses_excluded_layouts():
    """the rules of include/f5hip.h: nothing is launched for a layout the kernels' contracts exclude"""
    from tts_indic_server_f5_amd import _lib, ops
    x = torch.zeros(1024, 32, device=DEV)
    w = torch.zeros(32, 32, 3)
    ok = dict(row0=[0, 256], rows=[256, 768], valid=[200, 700], blk=256)
    reset_counters()
    ops.conv1d_ragged(x, w, **ok, impl=5)
    assert conv_counters()["conv5"] == 1
    bad = [
        dict(ok, row0=[0, 384], rows=[256, 512]),                 # an item start that is not a multiple of blk
        dict(ok, rows=[256, 512]),                                # the last block belongs to no item
        dict(ok, row0=[256, 512], rows=[256, 512]),               # the first block belongs to no item
        dict(ok, row0=[0, 0]),                                    # a block that belongs to two items
        dict(ok, valid=[257, 700]),                               # more valid rows than the item has
        dict(ok, valid=[0, 700]),
        dict(ok, rows=[256, 1024]),                               # past the last row
        dict(ok, blk=192),                                        # blk is not a multiple of 128
        dict(row0=[0, 128], rows=[128, 896], valid=[100, 800], blk=128, impl=5),   # conv5: a 256-row tile would span two items
    ]
    reset_counters()
    for kw in bad:
        with pytest.raises(_lib.F5HipError):
            ops.conv1d_ragged(x, w, **{"impl": 5, **kw})
    with pytest.raises(_lib.F5HipError, match="does not fit"):   # conv5: a blk of 384 rows does not fit the 256-row tile (M = 768 does)
        ops.conv1d_ragged(x[:768], w, row0=[0, 384], rows=[384, 384], valid=[300, 384], blk=384, impl=5)
    assert conv_counters() == {"conv5": 0, "gemm_reg_bn64": 0, "gemm_reg_bn128": 0}
    reset_counters()   # what conv5 refuses, gemm.h takes
    ops.conv1d_ragged(x, w, row0=[0, 128], rows=[128, 896], valid=[100, 800], blk=128, impl=0)
    assert conv_counters()["gemm_reg_bn64"] == 1


# ---------------------------------------------------------------------------------------------------------------- SnakeBeta activation
ITEM_FRAMES = [1, 5, 129, 37]
GUARD = 64


@pytest.mark.parametrize("Cc", [96, 24, 4])
@pytest.mark.parametrize("scale", [1, 2, 256])
def test_snake_ragged(scale, Cc):
    """aa_snake2_kernel with items / scale in all three output formats, inputs and bounds of test_snake_vs_fp64 (x = 2 N(0, 1), log alpha /
    log beta uniform in [-1, 1], _snake_bound plus the format's rounding).  The output is pre-filled with the sentinel: in the launch over all
    items every row outside the items' valid rows must keep it, and in a launch that lists ONE item (at its place in the same buffer) every
    other item's rows too, while that item's rows equal the full launch's.  Each item also equals the uniform op on the item alone, to the bit."""
    from tts_indic_server_f5_amd import ops
    row0, rows, valid, M = _layout(ITEM_FRAMES, scale)
    g = torch.Generator().manual_seed(7300 + Cc * 13 + scale)
    x = _nan_padding(2 * torch.randn(M, Cc, generator=g), row0, rows, valid)
    al = torch.rand(Cc, generator=g) * 2 - 1
    be = torch.rand(Cc, generator=g) * 2 - 1
    xd = x.to(DEV)
    refs = [snake_ref(x[r0: r0 + p], al, be, 1, p, v)[0] for r0, p, v in zip(row0, rows, valid)]
    b32 = snake_bound(max(float(x[r0: r0 + v].abs().max()) for r0, v in zip(row0, valid)), al, be)

    def run(r0s, vs, fmt):
        out = torch.full((M + GUARD, Cc), SENTINEL, dtype=torch.float32, device=DEV)
        ops.bigvgan_snake_ragged(xd, al, be, row0=r0s, valid=vs, scale=scale, out_format=fmt, out=out)
        return out.cpu()

    for fmt, name, rel in SNAKE_FORMATS:
        out = run(row0, valid, fmt)
        check_untouched_items(out, row0, valid)
        for i, (r0, p, v) in enumerate(zip(row0, rows, valid)):
            got = out[r0: r0 + v]
            err = got.double() - refs[i]
            report(f"bigvgan snake ragged C {Cc} scale {scale} item {i} rows {r0}+{v} {name} (bound {b32:.2e} + {rel:.1e} |y|)", err)
            assert (err.abs() <= b32 + rel * refs[i].abs()).all(), (name, i)
            one = run([r0], [v], fmt)
            check_untouched_items(one, [r0], [v])
            assert torch.equal(one[r0: r0 + v], got), f"{name} item {i}: the item alone in the ragged layout differs"
            uni = torch.full((p + GUARD, Cc), SENTINEL, dtype=torch.float32, device=DEV)
            ops.bigvgan_snake(xd[r0: r0 + p], al, be, batch=1, valid=v, out_format=fmt, out=uni)
            assert torch.equal(uni.cpu()[:v], got), f"{name} item {i}: differs from the uniform op"


def test_snake_ragged_refuses_bad_items():
    from tts_indic_server_f5_amd import _lib, ops
    x = torch.zeros(512, 24, device=DEV)
    p = torch.zeros(24)
    for kw in (dict(row0=[0, 257], valid=[100, 100], scale=2), dict(row0=[0, 256], valid=[100, 101], scale=2),
               dict(row0=[0, 256], valid=[100, 258], scale=2), dict(row0=[0, 256], valid=[100, 0], scale=1), dict(row0=[-2, 256], valid=[100, 100], scale=2)):
        with pytest.raises(_lib.F5HipError):
            ops.bigvgan_snake_ragged(x, p, p, **kw)


# ---------------------------------------------------------------------------------------------------------------- conv_post
WAVE_ORDER = [2, 0, 3, 1]   # the order in which the items get their place in the packed wave: not the row order


def _conv_post_data(Cc, scale):
    row0, rows, valid, M = _layout(ITEM_FRAMES, scale)
    g = torch.Generator().manual_seed(9300 + Cc * 7 + scale)
    a = _nan_padding(torch.randn(M, Cc, generator=g), row0, rows, valid)
    w = torch.randn(Cc, 7, generator=g) / math.sqrt(7 * Cc)
    off, o = [0] * len(valid), 0
    for i in WAVE_ORDER:
        off[i] = o
        o += valid[i]
    refs, bounds = [], []
    n = 7 * Cc
    for r0, v in zip(row0, valid):
        av = a[r0: r0 + v].t()[None].double()
        refs.append(torch.nn.functional.conv1d(av, w.double()[None], padding=3)[0, 0])
        bounds.append(n * U32 / (1 - n * U32) * torch.nn.functional.conv1d(av.abs(), w.double().abs()[None], padding=3)[0, 0])
    return row0, rows, valid, off, o, a, w, refs, bounds


@pytest.mark.parametrize("Cc,scale", [(c, s) for c in (24, 44, 48) for s in (256, 1)])
def test_conv_post_ragged_inputs_clip_a_third(Cc, scale):
    """the seeds of test_conv_post_ragged give what test_conv_post_vs_fp64 asks for: outputs ~N(0, 1), about a third of them beyond +-1.
    P(|z| > 1) = 0.317 at unit variance; the variance is sum w^2 of the 7 C weights drawn, 1 +- sqrt(2 / (7 C)) = +-11 % at C = 24, which
    moves the fraction by +-0.03, and the 172 samples of scale 1 scatter by another +-0.04 around it."""
    *_, refs, bounds = _conv_post_data(Cc, scale)
    clip = torch.cat([r.abs() > 1 + b for r, b in zip(refs, bounds)]).double().mean().item()
    print(f"[parity] conv_post ragged inputs C {Cc} scale {scale}: {clip:.3f} of the outputs clip")
    assert 0.22 < clip < 0.42


@pytest.mark.parametrize("scale", [256, 1])
@pytest.mark.parametrize("Cc,variant", [(24, 1), (44, 1), (24, 2), (44, 2), (48, 2)])
def test_conv_post_ragged(Cc, variant, scale):
    """bv_conv_post_kernel (variant 1, while its tile fits: C <= 44) and bv_conv_post_naive_kernel (2) with items / scale: bound and exact +-1
    rule of test_conv_post_vs_fp64 per item, the wave offsets handed out in another order than the rows, 64 guard samples behind the packed
    wave, and every item bit-equal to the uniform op on the item alone."""
    from tts_indic_server_f5_amd import ops
    row0, rows, valid, off, total, a, w, refs, bounds = _conv_post_data(Cc, scale)
    ad = a.to(DEV)
    wave = torch.full((total + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    ops.bigvgan_conv_post_ragged(ad, w, wave, row0=row0, valid=valid, wave_off=off, scale=scale, variant=variant)
    wave = wave.cpu()
    assert (wave[total:] == SENTINEL).all(), "the guard behind the packed wave was written"
    assert torch.isfinite(wave).all()
    kind = {1: "lds", 2: "naive"}[variant]
    for i, (r0, p, v, o) in enumerate(zip(row0, rows, valid, off)):
        got = wave[o: o + v]
        ref, bound = refs[i], bounds[i]
        clip = ref.abs() > 1 + bound
        assert (got.double()[clip] == ref[clip].sign()).all(), "the clamp must give exactly +-1"
        err = got.double() - ref.clamp(-1, 1)
        mx, _ = report(f"bigvgan conv_post ragged {kind} C {Cc} scale {scale} item {i} rows {r0}+{v} wave {o} ({clip.double().mean():.2f} clipped)", err)
        print(f"[parity] bigvgan conv_post ragged {kind} C {Cc} scale {scale} item {i}: max err / bound {(err.abs() / bound.clamp_min(1e-30)).max().item():.3f} (<= 1)")
        assert (err.abs() <= bound).all()
        uni = ops.bigvgan_conv_post(ad[r0: r0 + p], w, batch=1, valid=v, variant=variant).cpu()[0]
        assert torch.equal(uni, got), f"item {i}: differs from the uniform op"


def test_conv_post_ragged_refuses_bad_items():
    from tts_indic_server_f5_amd import _lib, ops
    a = torch.zeros(512, 24, device=DEV)
    w = torch.zeros(24, 7)
    wave = torch.zeros(200, device=DEV)
    for kw in (dict(row0=[0, 256], valid=[100, 100], wave_off=[0, 101], scale=1),    # past the end of the wave
               dict(row0=[0, 256], valid=[100, 100], wave_off=[1, 100], scale=2),    # an offset that is no multiple of scale
               dict(row0=[0, 256], valid=[100, 300], wave_off=[0, 100], scale=1)):   # past the last row
        with pytest.raises(_lib.F5HipError):
            ops.bigvgan_conv_post_ragged(a, w, wave, **kw)
    with pytest.raises(_lib.F5HipError):   # variant 1 where its tile does not fit
        ops.bigvgan_conv_post_ragged(torch.zeros(512, 48, device=DEV), torch.zeros(48, 7), wave, row0=[0], valid=[100], wave_off=[0], scale=1, variant=1)


# ---------------------------------------------------------------------------------------------------------------- mean3
M3_ROWS = 1037            # rows C / 4 lanes: 1037, 6222, 24888 -- none a multiple of the 256 lanes of a workgroup
M3_SENTINEL = -320.0      # exact in bf16 too (the plain-bf16 mode rounds the planes it loads)
# plane mode -> (name, the format's conversion of an fp32 value, its rounding relative to |y|, absolute floor)
M3_MODES = {
    1: ("split-bf16", fmt_split, 2.0 ** -17, 0.0),
    2: ("fp16", fmt_f16, 2.0 ** -11, 2.0 ** -25),            # (below 2^-14 fp16 is subnormal: spacing 2^-24)
    3: ("bf16", lambda y: y.float().bfloat16().float(), 2.0 ** -8, 0.0),
}
# The bf16 plane: bf16 carries 8 significant bits, so within a binade [2^e, 2^(e+1)) its values are 2^(e-7) apart and round-to-nearest errs by
# up to half of that, 2^(e-8) <= 2^-8 |y| -- not 2^-9 |y|, which no conversion can meet (test_bf16_rounding_bound_on_the_cpu shows both on the
# CPU).  The split pair does reach 2^-17 |y|: the remainder y - hi is below 2^(e-8), so lo is within 2^(e-17) of it.


def _mean3_inputs(Cc):
    g = torch.Generator().manual_seed(6100 + Cc)
    ys = [3 * torch.randn(M3_ROWS, Cc, generator=g) for _ in range(3)]
    for y in ys:   # a few means beyond the fp16 range, both signs
        y[5::97, 1] = 9e4
        y[6::97, 2] = -9e4
    return ys


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("Cc", [4, 24, 96])
def test_mean3_vs_fp64(Cc, mode):
    """bv_mean3_kernel, n_in = 3, against (y0 + y1 + y2) / 3 in float64.  fp32 bound: two fp32 additions and the product with the rounded
    1 / 3, 4 u32 (|y0| + |y1| + |y2|) / 3.  A plane mode adds its rounding of the fp32 result: 2^-17 |y| split bf16, 2^-11 |y| fp16 (2^-25
    in its subnormal range; saturating at +-65504), 2^-8 |y| for the round-to-nearest bf16 plane (M3_MODES).  Planes of pitch ceil32(C): the
    padding channels keep the sentinel."""
    from tts_indic_server_f5_amd import ops
    ys = _mean3_inputs(Cc)
    ref = (ys[0].double() + ys[1].double() + ys[2].double()) / 3
    b32 = 4 * U32 * (ys[0].double().abs() + ys[1].double().abs() + ys[2].double().abs()) / 3
    ldo = (Cc + 31) // 32 * 32
    planes = torch.full((M3_ROWS, ldo), M3_SENTINEL, dtype=torch.float32, device=DEV) if mode else None
    out, planes = ops.bigvgan_mean3([y.to(DEV) for y in ys], mode=mode, planes=planes)
    err = out.cpu().double() - ref
    report(f"bigvgan mean3 C {Cc} mode {mode} fp32 rows (max err / bound {(err.abs() / b32).max().item():.3f})", err)
    assert (err.abs() <= b32).all()
    if not mode:
        return
    name, _, rel, floor = M3_MODES[mode]
    pl = planes.cpu()
    assert (pl[:, Cc:] == M3_SENTINEL).all(), "a padding channel was written"
    got = pl[:, :Cc].double()
    assert torch.isfinite(got).all()
    want = ref.clamp(-65504, 65504) if mode == 2 else ref
    bound = b32 + rel * ref.abs() + floor
    err = got - want
    report(f"bigvgan mean3 C {Cc} mode {mode} {name} planes (max err / bound {(err.abs() / bound).max().item():.3f})", err)
    assert (err.abs() <= bound).all()
    if mode == 2:
        over = ref.abs() > 65504 + b32
        assert over.any() and (got[over] == 65504 * ref[over].sign()).all()


def test_bf16_rounding_bound_on_the_cpu():
    """The float64 reference of test_mean3_vs_fp64, rounded to each plane format by torch on the CPU (round to nearest even), stays inside
    the format bounds of M3_MODES -- and the bf16 plane does NOT stay inside 2^-9 |y|: that figure is half of what 8 significant bits give."""
    ys = _mean3_inputs(96)
    ref = (ys[0].double() + ys[1].double() + ys[2].double()) / 3
    r32 = ref.float()
    for mode, (name, conv, rel, floor) in M3_MODES.items():
        want = ref.clamp(-65504, 65504) if mode == 2 else ref
        ratio = ((conv(r32).double() - want).abs() / (U32 * ref.abs() + rel * ref.abs() + floor)).max().item()
        print(f"[parity] mean3 reference rounded to {name} on the CPU: max err / bound {ratio:.3f} (<= 1)")
        assert ratio <= 1
    worst = ((r32.bfloat16().double() - ref).abs() / (2.0 ** -9 * ref.abs())).max().item()
    print(f"[parity] mean3 reference rounded to bf16 on the CPU: max err / (2^-9 |y|) {worst:.3f} (> 1: the bound 2^-9 |y| cannot hold)")
    assert 1.5 < worst <= 2.0


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("Cc", [4, 24, 96])
def test_mean3_single_input_is_the_exact_conversion(Cc, mode):
    """n_in = 1: the fp32 rows are y0 itself and the planes its conversion to the format (round to nearest even, fp16 saturating), bit for bit"""
    from tts_indic_server_f5_amd import ops
    y = _mean3_inputs(Cc)[0]
    ldo = (Cc + 31) // 32 * 32
    planes = torch.full((M3_ROWS, ldo), M3_SENTINEL, dtype=torch.float32, device=DEV) if mode else None
    out, planes = ops.bigvgan_mean3([y.to(DEV)], mode=mode, planes=planes)
    assert torch.equal(out.cpu(), y)
    if mode:
        name, conv, _, _ = M3_MODES[mode]
        pl = planes.cpu()
        assert (pl[:, Cc:] == M3_SENTINEL).all(), "a padding channel was written"
        err = pl[:, :Cc].double() - conv(y).double()
        report(f"bigvgan mean3 C {Cc} n_in 1 {name} vs the exact conversion (bound 0)", err)
        assert torch.equal(pl[:, :Cc], conv(y))


# ---------------------------------------------------------------------------------------------------------------- mel rows
MELS = 100


def _check_mel_rows(tag, got, mel_items, row0, f16):
    """got fp32 [M0, 128]; mel_items[i] [MELS, T_i] from row row0[i]; every other entry must be exactly zero"""
    assert not torch.isnan(got).any(), f"{tag}: a column past an item's frames, or a plane the kernel left unwritten, shows"
    want = torch.zeros_like(got, dtype=torch.float64)
    for m, r0 in zip(mel_items, row0):
        want[r0: r0 + m.shape[1], :MELS] = m.t().double()
    zero = want == 0
    assert (got[zero] == 0).all(), f"{tag}: rows past T and channels past num_mels must be zero"
    if f16:
        bound, name = 2.0 ** -11 * want.abs() + 2.0 ** -25, "fp16"
        over = want.abs() > 65504
        assert over.any() and (got.double()[over] == 65504 * want[over].sign()).all()
        want = want.clamp(-65504, 65504)
    else:
        bound, name = 2.0 ** -17 * want.abs(), "split-bf16"
    err = got.double() - want
    report(f"bigvgan mel_rows {tag} {name} (max err / bound {(err.abs() / bound.clamp_min(1e-300)).max().item():.3f})", err)
    assert (err.abs() <= bound).all()


def _mel(t, g):
    m = torch.randn(MELS, t, generator=g) * 1.5 - 1.0
    m[3, 0] = 1e5      # beyond the fp16 range
    m[MELS - 1, t - 1] = -1e5
    return m


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("T", [1, 127, 128, 129])
def test_mel_rows_uniform(T, f16):
    from tts_indic_server_f5_amd import ops
    batch, P = 3, (T + 127) // 128 * 128
    g = torch.Generator().manual_seed(6500 + T)
    mels = [_mel(T, g) for _ in range(batch)]
    got = ops.bigvgan_mel_rows(torch.stack(mels).to(DEV), rows=batch * P, f16=f16).cpu()
    _check_mel_rows(f"uniform batch {batch} T {T} P {P}", got, mels, [b * P for b in range(batch)], f16)


@pytest.mark.parametrize("f16", [False, True])
def test_mel_rows_ragged(f16):
    """items in another order than the rows (the generator puts the 256-aligned pitches first); the columns past an item's frames hold NaN"""
    from tts_indic_server_f5_amd import ops
    frames = [1, 127, 128, 129, 300, 37]
    order = [3, 4, 0, 1, 2, 5]
    row0, r = [0] * len(frames), 0
    for i in order:
        row0[i] = r
        r += (frames[i] + 127) // 128 * 128
    g = torch.Generator().manual_seed(6600)
    mels = [_mel(t, g) for t in frames]
    slab = torch.full((len(frames), MELS, max(frames)), NAN)
    for i, m in enumerate(mels):
        slab[i, :, : m.shape[1]] = m
    got = ops.bigvgan_mel_rows(slab.to(DEV), rows=r, row0=row0, frames=frames, f16=f16).cpu()
    _check_mel_rows(f"ragged frames {frames} rows {row0}", got, mels, row0, f16)
