"""GPU: every stage of the Vocos decoder (csrc/vocos.h: vocos_decode_items) against the float64 references of tests/vocos_ref.py, through
the parity taps of f5hip_vocos_decode_taps (F5HipVocos.decode_taps): the residual stream behind the embed conv + norm and behind each of
the 8 ConvNeXt blocks, the head output y, the windowed frames fw and the wave.

Stage k's reference starts from the GPU's OWN tap of stage k - 1 (upcast), so nothing accumulates and a failure names the stage, the item
and the row.  The GPU is compared with vocos_ref.EXACT only; the tolerances are those of tests/test_vocos_reference.py, which shows on the
CPU what they catch:
  backbone stages and head   rms(GPU - exact) <= 3 rms(model - exact) per item, over all its rows and on its worst row, model = the same
                             float64 arithmetic on the mode's operand formats (split bf16 for gemm_planes 2, one bf16 plane for 1);
  istft_frame_kernel         per frame, rms(GPU - exact) / rms(exact) <= 4 x the same figure of torch's fp32 irfft on the same y;
  istft_ola_kernel           per sample, |GPU - exact| <= 10 x 2^-24 x sum|terms| / envelope;
  whole decode               max and rms of GPU - float64 <= 3 x those of the chained model.

The case: real geometry (dim 512, intermediate 1536, 8 layers), one ragged call of frames (2, 129, 5, 128, 7, 3) -- 896 padded rows; items
shorter than the 7-tap kernels, one exactly as long, one an exact 128-row slab, one a row over -- and one batched call of (77, 77, 77),
f5hip_vocos_decode's layout.  Every valid row of every item is compared."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_vocos_reference as T  # noqa: E402
import vocos_ref as R  # noqa: E402
from mel_ref import LOG_CLAMP  # noqa: E402
from tts_indic_server_f5_amd import synth  # noqa: E402

RAGGED = (2, 129, 5, 128, 7, 3)
BATCHED = (77, 77, 77)
LAYERS = 8
_PLANES = pytest.mark.parametrize("planes", [2, 1], ids=["split_bf16", "bf16"])


def _mels(frames, seed):
    g = torch.Generator().manual_seed(seed)
    mels = [torch.randn(100, t, generator=g) * 1.5 - 1.0 for t in frames]
    if frames == RAGGED:                      # digital silence at the head and the tail of the item that is one row over a slab
        mels[1][:, :9] = LOG_CLAMP
        mels[1][:, -11:] = LOG_CLAMP
    return mels


def _packed(mels, fill=0.0):
    """[n, C, T_max] with `fill` behind every item's last frame"""
    mel = torch.full((len(mels), 100, max(m.shape[1] for m in mels)), fill)
    for i, m in enumerate(mels):
        mel[i, :, :m.shape[1]] = m
    return mel


def _vocos(planes, sd=None):
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipVocos(synth.vocos_state_dict() if sd is None else sd, gemm_planes=planes)


class _Run:
    """All taps of one case on one handle, on the CPU: xs[k] behind k blocks, and y / fw / wave of the whole decode"""

    def __init__(self, vocos, frames, seed, fill=0.0):
        self.frames, self.mels = frames, _mels(frames, seed)
        mel = _packed(self.mels, fill)
        self.xs = [vocos.decode_taps(mel, frames, k)["x"].cpu() for k in range(LAYERS + 1)]
        full = vocos.decode_taps(mel, frames, -1)
        self.x_full, self.y, self.fw, self.wave = (full[k].cpu() for k in ("x", "y", "fw", "wave"))

    def rows(self, i):
        r0 = sum(self.frames[:i])
        return slice(r0, r0 + self.frames[i])

    def samples(self, i):
        s0 = 256 * sum(t - 1 for t in self.frames[:i])
        return slice(s0, s0 + 256 * (self.frames[i] - 1))

    def tensors(self):
        return self.xs + [self.x_full, self.y, self.fw, self.wave]


@pytest.fixture(scope="module")
def weights():
    return R.Weights(synth.vocos_state_dict())


@pytest.fixture(scope="module", params=[2, 1], ids=["split_bf16", "bf16"])
def ragged(request):
    planes = request.param
    vocos = _vocos(planes)
    return planes, vocos, _Run(vocos, RAGGED, 500)


class _Report:
    """Prints one [parity] line per comparison and collects the ones above the factor; the test asserts on them at its end, so one run
    shows every figure."""

    def __init__(self, label):
        self.label, self.bad, self.worst = label, [], (0.0, 0.0)

    def check(self, tag, got, exact, model):
        g, m = R.row_stats(got.double() - exact), R.row_stats(model - exact)
        ratio = (g[0] / m[0], g[1] / m[1])
        print(f"[parity] {self.label} {tag}: gpu_err rms {g[0]:.3e} worst row {g[1]:.3e}   model_err rms {m[0]:.3e} worst row {m[1]:.3e}   "
              f"gpu_err / model_err {ratio[0]:.2f} / {ratio[1]:.2f}   (ref rms {exact.pow(2).mean().sqrt():.3f})")
        self.worst = (max(self.worst[0], ratio[0]), max(self.worst[1], ratio[1]))
        if not (ratio[0] <= T.FACTOR and ratio[1] <= T.FACTOR):
            self.bad.append((tag, ratio))

    def finish(self):
        print(f"[parity] {self.label}: largest gpu_err / model_err {self.worst[0]:.2f} (rms) {self.worst[1]:.2f} (worst row)")
        assert not self.bad, self.bad


def _check_stages(W, run, planes, label):
    F, rep = R.MODES[planes], _Report(f"{label} gemm_planes {planes}")
    assert all(torch.isfinite(t).all() for t in run.tensors())
    assert torch.equal(run.x_full, run.xs[LAYERS]), "the whole decode's stream tap differs from the one stopped behind the last block"
    for i, t in enumerate(run.frames):
        rows = run.rows(i)
        rep.check(f"item {i} (T {t}) embed + norm", run.xs[0][rows], R.embed(W, run.mels[i]), R.embed(W, run.mels[i], F))
        for l in range(LAYERS):
            xin = run.xs[l][rows]
            rep.check(f"item {i} (T {t}) block {l}", run.xs[l + 1][rows], R.block(W, l, xin), R.block(W, l, xin, F))
        xin = run.xs[LAYERS][rows]
        rep.check(f"item {i} (T {t}) final norm + head", run.y[rows], R.head(W, xin), R.head(W, xin, F))
    rep.finish()


def test_stage_chain_ragged(weights, ragged):
    """Embed conv + norm, the 8 blocks and the final norm + head of the ragged case, every row of every item.
    Measured on an MI355X, largest gpu_err / model_err (rms / worst row): gemm_planes 2 1.33 / 1.35, gemm_planes 1 1.00 / 1.00.  In split
    bf16 every stage of every item sits at 1.19 .. 1.35 (a split-bf16 GEMM sums hi x hi + hi x lo + lo x hi in fp32, the operand model
    multiplies hi + lo by hi + lo in float64): embed + norm 4.2e-6 rms on a stream of rms 1.0 (K = 7 x 100 mel values of rms 1.8), the
    blocks 5.3e-7, the head 2.2e-6 on y of rms 0.5.  In plain bf16 the operands' own rounding (2.3e-3 / 2.8e-4 / 1.2e-3) is all there is."""
    planes, _, run = ragged
    _check_stages(weights, run, planes, "Vocos ragged")


@_PLANES
def test_stage_chain_batched(weights, planes):
    """The same for three items of 77 frames: f5hip_vocos_decode's layout (channel stride = frames, equal slabs).
    Measured on an MI355X, largest gpu_err / model_err (rms / worst row): gemm_planes 2 1.29 / 1.34, gemm_planes 1 1.00 / 1.00."""
    vocos = _vocos(planes)
    run = _Run(vocos, BATCHED, 501)
    _check_stages(weights, run, planes, "Vocos batched")
    mel = torch.stack(run.mels)
    assert torch.equal(vocos.decode(mel).reshape(-1).cpu(), run.wave), "decode_taps(-1) and decode differ"


@pytest.mark.parametrize("fill", [1e30, float("nan")], ids=["1e30", "nan"])
def test_columns_behind_an_item_are_not_read(ragged, fill):
    """The mel tensor's columns behind an item's last frame hold 1e30 / NaN instead of zeros: every tap has the same bits"""
    _, vocos, run = ragged
    other = _Run(vocos, RAGGED, 500, fill=fill)
    for k, (a, b) in enumerate(zip(run.tensors(), other.tensors())):
        assert torch.equal(a, b), f"tap {k} changed with {fill} behind the items"


def test_taps_wave_equals_decode_ragged(ragged):
    """decode_taps(-1) returns decode_ragged's wave bit for bit, and each item's equals its own decode"""
    _, vocos, run = ragged
    waves = vocos.decode_ragged(run.mels)
    assert torch.equal(torch.cat(waves).cpu(), run.wave)
    for i in (0, 1, 4):
        assert torch.equal(vocos.decode(run.mels[i][None])[0].cpu(), run.wave[run.samples(i)]), i


def _gemm_launches():
    from tts_indic_server_f5_amd import _lib
    total = 0
    for name in ("gemm3", "gemm_reg_bn64", "gemm_reg_bn128"):
        v = C.c_int64(0)
        _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
        total += v.value
    return total


def test_taps_entry_refuses_bad_arguments(ragged):
    """n_blocks outside -1 .. 8, null pointers and an item of one frame are refused before any launch (the GEMM launch counters stay)"""
    from tts_indic_server_f5_amd import _lib
    _, vocos, _ = ragged
    mel = torch.zeros(2, 100, 5)
    n0 = _gemm_launches()
    vocos.decode_taps(mel, (5, 4), 0)
    assert _gemm_launches() == n0 + 1                                      # the embed conv alone
    n0 = _gemm_launches()
    for k in (LAYERS + 1, -2):
        with pytest.raises(_lib.F5HipError, match="n_blocks"):
            vocos.decode_taps(mel, (5, 4), k)
    with pytest.raises(_lib.F5HipError):
        vocos.decode_taps(mel, (5, 1), 0)
    with pytest.raises(_lib.F5HipError):
        vocos.decode_taps(mel, (5, 4, 3), 0)
    dev = mel.cuda()
    f = torch.tensor([5, 4], dtype=torch.int32)
    x, y, fw, wave = (torch.empty(n, device="cuda") for n in (9 * 512, 9 * 1026, 9 * 1024, 256 * 7))
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda *a: _lib.lib().f5hip_vocos_decode_taps(vocos._h, 2, *a, _lib.current_stream_ptr())
    assert call(p(f), p(dev), -1, p(x), p(y), p(fw), p(wave)) == 0
    n0 = _gemm_launches()
    for args in ((None, p(dev), 0, p(x), None, None, None), (p(f), None, 0, p(x), None, None, None), (p(f), p(dev), 0, None, None, None, None),
                 (p(f), p(dev), -1, p(x), None, p(fw), p(wave)), (p(f), p(dev), -1, p(x), p(y), None, p(wave)),
                 (p(f), p(dev), -1, p(x), p(y), p(fw), None)):
        assert call(*args) == -1
    assert _lib.lib().f5hip_vocos_decode_taps(None, 2, p(f), p(dev), 0, p(x), None, None, None, _lib.current_stream_ptr()) == -1
    assert _gemm_launches() == n0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- iSTFT head
def _head_state(which):
    sd = synth.vocos_state_dict()
    if which == "phases":          # phases of some tens of radians: the argument reduction of sinf / cosf
        w = sd["head.out.weight"].clone()
        w[513:] *= 20.0
        sd["head.out.weight"] = w
    elif which == "clip":          # log-magnitudes raised by ln 100: part of the bins exceed the clip
        b = sd["head.out.bias"].clone()
        b[:513] += math.log(100.0)
        sd["head.out.bias"] = b
    return sd


@pytest.mark.parametrize("which", ["plain", "phases", "clip"])
def test_istft_frames(which):
    """istft_frame_kernel against vocos_ref.frames in float64 on the GPU's own y, every frame of the ragged case, in three states: the
    synthetic one (phases within +-2.4 rad), phases scaled by 20, magnitudes raised past the clip of 100.
    Measured on an MI355X, largest (GPU figure / fp32 CPU figure) over the 274 frames: plain 1.21, phases (up to 46.8 rad) 0.84, clip
    (50 % of the bins) 1.33; medians 0.81 / 0.74 / 0.85, the GPU figure itself 1.1e-7 .. 3.0e-7."""
    run = _Run(_vocos(2, _head_state(which)), RAGGED, 500)
    assert torch.isfinite(run.fw).all()
    mag, ph = run.y[:, :513], run.y[:, 513:]
    print(f"[parity] frames {which}: max |phase| {ph.abs().max():.1f} rad, {100 * (mag > math.log(100.0)).float().mean():.1f} % of the bins clipped")
    if which == "phases":
        assert ph.abs().max().item() > 20.0
    if which == "clip":
        assert 0.1 < (mag > math.log(100.0)).float().mean().item() < 0.9
    exact = R.frames(run.y)
    gpu, cpu = T.frame_rel(run.fw, exact), T.frame_rel(R.frames(run.y, dtype=torch.float32), exact)
    ratio = gpu / cpu
    k = int(ratio.argmax())
    print(f"[parity] frames {which}: gpu rel err median {gpu.median():.3e} max {gpu.max():.3e}; fp32 cpu median {cpu.median():.3e} max {cpu.max():.3e}; "
          f"gpu / cpu median {ratio.median():.2f} max {ratio.max():.2f} (frame {k})")
    assert (ratio <= T.FRAME_FACTOR).all(), (k, ratio[k].item())


def test_istft_overlap_add(ragged):
    """istft_ola_kernel against vocos_ref.ola in float64 on the GPU's own fw, every sample of every item (the bisection over the items'
    first samples, the first and last 512 samples where fewer than 4 frames overlap, the 256-sample item).  The bound is derived, not
    measured: val sums <= 4 terms (3 roundings), env <= 4 squares of the fp32 window (2 roundings each against the float64 window, 3 for
    the sum), one division: <= 10 x 2^-24 x sum|terms| / env.  (An MI355X uses at most 0.41 of it.)"""
    _, _, run = ragged
    worst = 0.0
    for i, t in enumerate(run.frames):
        fw = run.fw[run.rows(i)]
        err = (run.wave[run.samples(i)].double() - R.ola(fw)).abs()
        frac = (err / T.ola_bound(fw)).max().item()
        print(f"[parity] overlap-add item {i} (T {t}): max err {err.max():.3e}, {frac:.3f} of the bound")
        worst = max(worst, frac)
    assert worst <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------- whole decode
def test_whole_decode_ragged(weights, ragged):
    """The ragged case end to end against float64: max and rms within 3 x the chained model's (and the north-star 1e-4 in the split-bf16
    mode).  Measured on an MI355X, gpu_err / model_err (max / rms): gemm_planes 2 1.14 / 1.29 (6.5e-7 max against the model's 5.7e-7),
    gemm_planes 1 0.94 / 1.00 (3.3e-4 against 3.5e-4)."""
    planes, _, run = ragged
    waves = [run.wave[run.samples(i)] for i in range(len(run.frames))]
    (g_max, g_rms), (m_max, m_rms) = R.decode_errors(weights, run.mels, waves, planes)
    print(f"[parity] whole decode ragged gemm_planes {planes}: gpu_err max {g_max:.3e} rms {g_rms:.3e}   model_err max {m_max:.3e} rms {m_rms:.3e}   "
          f"gpu_err / model_err {g_max / m_max:.2f} / {g_rms / m_rms:.2f}")
    if planes == 2:
        assert g_max < 1e-4
    assert g_max <= T.FACTOR * m_max and g_rms <= T.FACTOR * m_rms
