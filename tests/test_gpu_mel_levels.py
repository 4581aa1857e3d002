"""GPU: mel_frame_kernel (csrc/vocos.h), through mel.mel_spectrogram and mel.mel_spectrogram_bigvgan, against the float64 oracles on clean,
silent and band-limited audio, where bins sit at or near log(clamp(., 1e-5)): the linear-domain bound and the signals of tests/mel_ref.py
(tests/test_mel_bound_reference.py fixes its constants on the CPU), exact log(1e-5) on all-zero frames, batch independence, the geometries
the wrappers accept besides 100 channels / 24 kHz / hop 256, the rebuild of the device tables between geometries, and the arguments the
library refuses."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import mel_ref as M  # noqa: E402
from oracle import vocos_oracle as V  # noqa: E402


def _run(front, wave, n_fft=1024, hop=256, n_mels=100, sr=24000):
    from tts_indic_server_f5_amd import mel
    fn = mel.mel_spectrogram if front == "vocos" else mel.mel_spectrogram_bigvgan
    return fn(wave.cuda(), n_fft=n_fft, hop_length=hop, n_mel_channels=n_mels, target_sample_rate=sr)


@functools.lru_cache(maxsize=None)
def _signals():
    return M.signals()


@functools.lru_cache(maxsize=None)
def _ref(front, name):
    return M.ref64(front, _signals()[name])


def _check(front, tag, got, wave, ref, hop=256):
    r, a = M.BOUND[front]
    assert got.shape == ref.shape
    parts = M.check_linear(got, ref, r, a, tag=tag)
    M.check_exact_frames(got, M.zero_frames(front, wave, hop=hop), tag=tag)
    return parts


LEVEL_CASES = [(f, k) for f in M.FRONTS for k in M.signals_for(f)]


@pytest.mark.parametrize("front,name", LEVEL_CASES)
def test_mel_levels(front, name):
    """Every signal of mel_ref.signals(), one launch each: |E - E_ref| <= r E_ref + a P_t on every bin, all-zero frames at log(1e-5) to 1e-6,
    and the log-domain bounds of the older mel tests wherever the float64 reference keeps every bin 1e3 above the clamp."""
    wave, ref = _signals()[name], _ref(front, name)
    got = _run(front, wave)
    _check(front, f"{front} {name}", got, wave, ref)
    if name in ("zeros", "impulse", "tones_then_zeros"):
        assert M.zero_frames(front, wave).any()
    if M.far_above_floor(ref):
        d = got.cpu().double() - ref
        mx, rms = d.abs().max().item(), d.pow(2).mean().sqrt().item()
        print(f"[parity] {front} {name}: every bin 1e3 above the clamp: log-mel rms_err {rms:.3e} max_err {mx:.3e}")
        assert rms < 1e-3 and mx < 5e-3
    else:
        assert name not in ("dc_tones_noise", "clipped")


@pytest.mark.parametrize("front", M.FRONTS)
def test_mel_batch_independence(front):
    """A batch of three different signals is the three single calls, bit for bit (one block per (frame, item): nothing is shared)."""
    names = ("tones_then_zeros", "impulse", "loud_low_tone")
    waves = [_signals()[k] for k in names]
    batch = _run(front, torch.cat(waves, 0))
    for i, (k, w) in enumerate(zip(names, waves)):
        assert torch.equal(batch[i:i + 1], _run(front, w)), (front, k)
        _check(front, f"{front} batch item {k}", batch[i:i + 1], w, _ref(front, k))


def _geometry_waves(hop):
    """[3, n]: tones, tones running into exact zeros, the control; 24 000 samples, or the 12 000 around the start of the zeros at hop 128,
    so that no case has more than 94 frames."""
    s = _signals()
    w = torch.cat([s["tones"], s["tones_then_zeros"], s["control"]], 0)
    return w if hop >= 256 else w[:, 6_000:18_000].contiguous()


@pytest.mark.parametrize("geom", list(M.GEOMETRIES))
@pytest.mark.parametrize("front", M.FRONTS)
def test_mel_geometries(front, geom):
    """The wrappers' own n_mel_channels / target_sample_rate / hop_length against the oracle called with the same values; the bound's
    constants are those of the default geometry."""
    g = M.GEOMETRIES[geom]
    hop = g.get("hop", 256)
    wave = _geometry_waves(hop)
    ref = M.ref64(front, wave, **g)
    got = _run(front, wave, **g)
    n_frames = 1 + wave.shape[1] // hop if front == "vocos" else wave.shape[1] // hop
    assert got.shape == (3, g.get("n_mels", 100), n_frames) and n_frames <= 94
    _check(front, f"{front} {geom}", got, wave, ref, hop=hop)
    assert M.zero_frames(front, wave, hop=hop)[1].any()
    if front == "vocos" and geom == "mels256":
        # 256 HTK channels over 12 kHz: the lowest filters are narrower than a bin (23.4 Hz) and some hold none; those channels are empty
        empty = M.float64(V.melscale_fbanks_htk, 513, 0.0, 12000.0, 256).sum(0) == 0
        assert 0 < empty.sum().item() < 40
        err = (got.cpu()[:, empty].double() - M.LOG_CLAMP).abs().max().item()
        print(f"[parity] vocos mels256: {int(empty.sum())} empty HTK channels, max |log-mel - log(1e-5)| {err:.3e}")
        assert err <= 1e-6


@pytest.mark.parametrize("front", M.FRONTS)
def test_mel_table_rebuild(front):
    """Geometry A, then B, then A again: the device tables (window, twiddles, filterbank) are rebuilt twice; the two A results are
    bit-identical and B matches its own float64 reference."""
    wave = _signals()["tones_then_zeros"]
    b_geom = dict(n_mels=80, sr=16000)
    a1 = _run(front, wave)
    b = _run(front, wave, **b_geom)
    a2 = _run(front, wave)
    assert torch.equal(a1, a2)
    _check(front, f"{front} rebuild A", a2, wave, _ref(front, "tones_then_zeros"))
    _check(front, f"{front} rebuild B", b, wave, M.ref64(front, wave, **b_geom))


BAD_ARGS = [
    ("n_fft_512", dict(n_fft=512), "n_fft"),
    ("n_mels_257", dict(n_mels=257), "n_mels"),
    ("n_mels_0", dict(n_mels=0), "n_mels"),
    ("sample_rate_0", dict(sr=0), "sample_rate"),
    ("too_short", dict(), "bad argument"),              # 512 samples (Vocos), 1023 (BigVGAN)
    ("hop_0", dict(hop=0), "hop_length"),
    ("hop_negative", dict(hop=-256), "hop_length"),
    ("hop_above_n_fft", dict(hop=1025), "hop_length"),
]


@pytest.mark.parametrize("case,kw,word", BAD_ARGS, ids=[c[0] for c in BAD_ARGS])
@pytest.mark.parametrize("front", M.FRONTS)
def test_mel_refused_arguments(front, case, kw, word):
    """Each is the library's own error (F5HipError with its text), through the wrapper and through the C entry point, where an output buffer
    of the default size keeps its sentinel: nothing was launched."""
    from tts_indic_server_f5_amd import _lib
    n = 4096 if case != "too_short" else (512 if front == "vocos" else 1023)
    wave = _signals()["tones"][:, :4096].cuda()
    with pytest.raises(_lib.F5HipError, match=word):
        _run(front, wave[:, :n].contiguous(), **kw)
    g = M._geom(**kw)
    out = torch.full((1, 256, 64), 7.0, device="cuda")
    fn = _lib.lib().f5hip_mel_spectrogram if front == "vocos" else _lib.lib().f5hip_mel_spectrogram_bigvgan
    rc = fn(1, n, C.c_void_p(wave.data_ptr()), C.c_void_p(out.data_ptr()), g["n_fft"], g["hop"], g["n_mels"], g["sr"], _lib.current_stream_ptr())
    assert rc != 0 and word in _lib.lib().f5hip_last_error().decode()
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    # the next valid call is unaffected
    _check(front, f"{front} after {case}", _run(front, _signals()["tones_1024"]), _signals()["tones_1024"], _ref(front, "tones_1024"))
