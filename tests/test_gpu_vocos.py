"""GPU parity (through the C ABI) of the Vocos decoder and the mel front-end vs the CPU oracle.
Tolerances from BASELINE.json north_star: 1e-4 on waveform samples, 1e-3 RMS on mel frames."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import vocos_ref as R  # noqa: E402
from mel_ref import LOG_CLAMP, float64 as _float64  # noqa: E402
from oracle import vocos_oracle as V  # noqa: E402
from tts_indic_server_f5_amd import synth  # noqa: E402


def _report(tag, got, ref):
    d = got.float().cpu() - ref.float().cpu()
    print(f"[parity] {tag}: rms_err {d.pow(2).mean().sqrt():.3e} max_err {d.abs().max():.3e} ref_rms {ref.float().pow(2).mean().sqrt():.3e}")
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


def _within_model(tag, sd, mel, got):
    """The whole decode against float64 by the rule of tests/test_gpu_vocos_stages.py: max and rms of GPU - float64 within 3 x those of
    the split-bf16 operand model chained over all stages (tests/vocos_ref.py) on the same mel [b, 100, t].  Measured on an MI355X over the
    cases of this file: gpu_err / model_err 1.19 .. 1.29 (max) and 1.20 .. 1.30 (rms); the model is 3.8e-7 .. 5.8e-7 max off float64 at
    the synthetic level, 2.6e-6 with the log-magnitudes raised by ln 5 and 3.2e-5 by ln 100."""
    (g_max, g_rms), (m_max, m_rms) = R.decode_errors(R.Weights(sd), list(mel), list(got), 2)
    print(f"[parity] {tag}: gpu_err max {g_max:.3e} rms {g_rms:.3e}   model_err max {m_max:.3e} rms {m_rms:.3e}   "
          f"gpu_err / model_err {g_max / m_max:.2f} / {g_rms / m_rms:.2f}")
    assert g_max <= 3.0 * m_max and g_rms <= 3.0 * m_rms


@pytest.fixture(scope="module")
def vocos():
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipVocos(synth.vocos_state_dict())


@pytest.mark.parametrize("b,t", [(1, 936), (3, 77), (1, 2), (2, 129)])
def test_vocos_decode(vocos, b, t):
    g = torch.Generator().manual_seed(100 + t)
    mel = torch.randn(b, 100, t, generator=g) * 1.5 - 1.0
    ref = V.vocos_decode(synth.vocos_state_dict(), mel)
    got = vocos.decode(mel)
    assert got.shape == ref.shape == (b, 256 * (t - 1))
    mx, rms = _report(f"vocos b{b} t{t}", got, ref)
    assert mx < 1e-4
    _within_model(f"vocos b{b} t{t}", synth.vocos_state_dict(), mel, got)


def _shifted_vocos_decode(shift):
    """The synthetic Vocos state with its log-magnitude bias (head.out.bias[:513]) raised by `shift`, decoded by the HIP path and by the
    float64 oracle (mel [2, 100, 200])."""
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    sd = synth.vocos_state_dict()
    bias = sd["head.out.bias"].clone()
    bias[:513] += shift
    sd["head.out.bias"] = bias
    g = torch.Generator().manual_seed(300)
    mel = torch.randn(2, 100, 200, generator=g) * 1.5 - 1.0
    ref = _float64(V.vocos_decode, {k: v.double() for k, v in sd.items()}, mel.double())
    got = F5HipVocos(sd).decode(mel)
    assert got.shape == ref.shape == (2, 256 * 199) and torch.isfinite(got).all()
    _within_model(f"vocos log-magnitudes + {shift:.2f}", sd, mel, got)
    return got, ref


def test_vocos_decode_realistic_level():
    """Log-magnitudes raised by ln 5: rms 0.104 and peak 0.51, the level of the reference's target_rms = 0.1 (F/infer/utils_infer.py:48),
    where the synthetic state alone gives rms 0.021.  The north-star bound holds absolutely; relative to the peak the error must stay at the
    level of fp32 arithmetic through the split-bf16 GEMMs: 3.1e-6 max, 6.1e-6 of the peak measured on an MI355X, bound 2e-5 (~3x).  (The fp32
    CPU oracle itself is 3.8e-7 off the float64 one here.)"""
    got, ref = _shifted_vocos_decode(math.log(5.0))
    mx, rms = _report("vocos x5 level", got, ref)
    peak = ref.abs().max().item()
    print(f"[parity] vocos x5 level: peak {peak:.3f}, max err / peak {mx / peak:.3e}")
    assert mx < 1e-4
    assert mx / peak < 2e-5


def test_vocos_decode_magnitude_clip():
    """Log-magnitudes raised by ln 100: half the bins exceed the clip of exp(mag) at 100 (istft_frame_kernel's fminf(expf(.), 100)),
    rms 1.15 and peak 5.4.  Same bounds: 1e-4 absolute (3.9e-5 measured on an MI355X), and the error relative to the peak at the fp32 level
    (7.2e-6 measured, bound 2e-5).  (The fp32 CPU oracle itself is 5.8e-6 off the float64 one here.)"""
    got, ref = _shifted_vocos_decode(math.log(100.0))
    mx, rms = _report("vocos x100 level (magnitude clip)", got, ref)
    peak = ref.abs().max().item()
    print(f"[parity] vocos x100 level: peak {peak:.3f}, max err / peak {mx / peak:.3e}")
    assert mx < 1e-4
    assert mx / peak < 2e-5


# 513: the shortest wave the host accepts (n_samples > n_fft / 2): reflect padding folds at both ends inside one frame;
# 256 x 94: an exact multiple of the hop; 256 x 94 + 255: one sample short of the next multiple
@pytest.mark.parametrize("b,nw", [(1, 120_000), (2, 24_000 + 77), (1, 1024), (1, 513), (2, 256 * 94), (1, 256 * 94 + 255)])
def test_mel_spectrogram(b, nw):
    from tts_indic_server_f5_amd.mel import mel_spectrogram
    wave = torch.cat([synth.ref_audio(nw, seed=1234 + i) for i in range(b)], dim=0)
    ref = _float64(V.vocos_mel_spectrogram, wave.double())
    got = mel_spectrogram(wave.cuda())
    assert got.shape == ref.shape == (b, 100, 1 + nw // 256)
    mx, rms = _report(f"mel b{b} nw{nw}", got, ref)
    assert rms < 1e-3 and mx < 5e-3


def test_vocos_decode_silence_frames(vocos):
    """What the decoder sees after the front-end on a clip with digital silence: half the frames of a [2, 100, 64] mel hold log(1e-5) in
    every channel (a run in the middle of item 0, the head and the tail of item 1), the others the random level of test_vocos_decode.
    Against the float64 oracle under the same 1e-4 bound (6.9e-7 max measured on an MI355X)."""
    sd = synth.vocos_state_dict()
    g = torch.Generator().manual_seed(164)
    mel = torch.randn(2, 100, 64, generator=g) * 1.5 - 1.0
    mel[0, :, 16:48] = LOG_CLAMP
    mel[1, :, :20] = LOG_CLAMP
    mel[1, :, 52:] = LOG_CLAMP
    assert (mel == mel.new_tensor(LOG_CLAMP)).all(1).sum().item() == 64          # half of the 128 frames
    ref = _float64(V.vocos_decode, {k: v.double() for k, v in sd.items()}, mel.double())
    got = vocos.decode(mel)
    assert got.shape == ref.shape == (2, 256 * 63) and torch.isfinite(got).all()
    mx, rms = _report("vocos silence frames b2 t64", got, ref)
    assert mx < 1e-4
    _within_model("vocos silence frames b2 t64", sd, mel, got)


def test_decode_ragged_ctypes_and_torch_op_paths_agree(vocos):
    """`decode_ragged` through the TORCH_LIBRARY operator and through ctypes: the same C entry point, so the same bits.  Items of 2 frames (the
    minimum), 129 (one past a 128-row slab) and 5 (a short one behind it)."""
    from tts_indic_server_f5_amd import torch_ops
    g = torch.Generator().manual_seed(7)
    mels = [torch.randn(100, t, generator=g) * 1.5 - 1.0 for t in (2, 129, 5)]
    via_op = vocos.decode_ragged(mels)
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        via_ctypes = vocos.decode_ragged(mels)
    finally:
        torch_ops._loaded = True
    assert [tuple(w.shape) for w in via_op] == [(256 * (m.shape[1] - 1),) for m in mels]
    assert len(via_ctypes) == len(via_op) and all(torch.equal(a, b) for a, b in zip(via_op, via_ctypes))


def test_mel_then_vocos_roundtrip_lengths(vocos):
    from tts_indic_server_f5_amd.mel import mel_spectrogram
    wave = synth.ref_audio(24_000).cuda()
    mel = mel_spectrogram(wave)
    out = vocos.decode(mel)
    assert out.shape[-1] == 256 * (mel.shape[-1] - 1) and torch.isfinite(out).all()
