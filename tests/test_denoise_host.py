"""CPU: the per-voice `denoise` option of uploaded reference clips on the host -- the definition `audio_prep.denoise_reference` against its
independent restatement (tests/denoise_ref.py), its laws, its effect on a synthetic speech-like signal in white noise, and the plumbing
through `infer.PreparedVoice`, `infer.prepare_voices(device=None)`, `serve.TTSManager` (clip cache, script voices) and the routes, on CPU
stand-in models."""
import base64
import io
import os
import sys
import wave

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import denoise_ref as R  # noqa: E402
from tts_indic_server_f5_amd import audio_prep as AP  # noqa: E402
from tts_indic_server_f5_amd import infer, serve  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------------ the definition
def test_constants():
    assert (AP.DENOISE_N_FFT, AP.DENOISE_HOP, AP.DENOISE_PAD, AP.DENOISE_RANK_DIV) == (1024, 256, 768, 5)
    assert (AP.DENOISE_SUBTRACT, AP.DENOISE_MIN_GAIN, AP.DENOISE_MAX_SAMPLES) == (6.75, 0.125, 1_440_000)
    assert [R.n_frames(n) for n in R.LENGTHS] == [4, 4, 4, 5, 7, 7, 20, 50, 238]
    assert [R.rank(R.n_frames(n)) for n in R.LENGTHS] == [0, 0, 0, 0, 1, 1, 3, 9, 47]
    assert [AP.denoise_frames(n) for n in R.LENGTHS] == [R.n_frames(n) for n in R.LENGTHS]
    w = np.sin(np.pi * np.arange(1024) / 1024) ** 2
    assert np.abs(w[:256] + w[256:512] + w[512:768] + w[768:] - 2.0).max() < 1e-15      # four shifts of w^2 by the hop sum to 2


@pytest.mark.parametrize("n", R.LENGTHS)
def test_definition_equals_the_restatement(n):
    x = R.clip(n)
    want = R.denoise(x, np.float64)
    got64 = AP.denoise_reference_f64(x)
    got = AP.denoise_reference(x)
    err = np.abs(got64 - want).max()
    print(f"[denoise] n={n} F={R.n_frames(n)} r={R.rank(R.n_frames(n))}: definition vs restatement max |diff| {err:.3e}")
    assert got64.dtype == np.float64 and got64.shape == (n,) and err <= 1e-12
    assert got.dtype == np.float32 and got.shape == (n,) and np.array_equal(got, got64.astype(np.float32))   # its one rounding
    assert np.array_equal(AP.denoise_reference(x[None]), got)                                                # [1, n] as a prepared voice holds it


def test_laws():
    for n in (1, 700, 5000, 30000):
        assert AP.denoise_reference(R.clip(n)).shape == (n,)                     # the length is preserved
        z = AP.denoise_reference(np.zeros(n, dtype=np.float32))
        assert z.shape == (n,) and not z.any()                                   # zeros stay zeros
    s = R.speechlike(6 * R.RATE, 11)                                             # clean, gated: floor = 0 in every bin, G = 1
    back = AP.denoise_reference_f64(s)
    rel = np.abs(back - s).max() / np.abs(s).max()
    print(f"[denoise] clean gated clip comes back within {rel:.3e} relative")
    assert rel <= 1e-9
    noisy = R.noisy_speech(3 * R.RATE, 12)[1]
    for peak in (1.0, 1e-6):
        y = AP.denoise_reference((noisy * (peak / np.abs(noisy).max())).astype(np.float32))
        assert np.isfinite(y).all() and np.abs(y).max() <= 2 * peak
    with pytest.raises(ValueError):
        AP.denoise_reference(np.zeros(0, dtype=np.float32))
    with pytest.raises(ValueError, match="DENOISE_MAX_SAMPLES"):
        AP.denoise_reference(np.zeros(AP.DENOISE_MAX_SAMPLES + 1, dtype=np.float32))


def test_rank_rule_against_sort():
    rng = np.random.default_rng(5)
    for F in (4, 5, 6, 7, 10, 11, 20, 50, 238, 1001):
        P = rng.exponential(1.0, (F, 513))
        P[rng.integers(0, F, 40), rng.integers(0, 513, 40)] = 0.0                # ties
        assert np.array_equal(AP.denoise_floor(P), np.sort(P, axis=0)[(F - 1) // 5])


def test_effect_on_speechlike_signal_in_white_noise():
    """6 s of the speech-like generator in seed-fixed white noise at 15 dB.  The bounds are the figures of the definition's prototype on its
    own generator (+9.1 dB, 14.4 dB in the pauses) less 3 dB and 2.4 dB of room for generator detail; 18.06 dB is what a gain of 1/8 gives."""
    n = 6 * R.RATE
    s, x = R.noisy_speech(n, 3, 15.0)
    y = AP.denoise_reference(x.astype(np.float32)).astype(np.float64)
    snr = lambda e: 10 * np.log10(np.sum(s * s) / np.sum(e * e))     # noqa: E731
    snr_in, snr_out = snr(x - s), snr(y - s)
    pm = R.pause_mask(n)
    att = 10 * np.log10(np.sum(x[pm] ** 2) / np.sum(y[pm] ** 2))
    print(f"[denoise] white noise at {snr_in:.2f} dB -> {snr_out:.2f} dB (+{snr_out - snr_in:.2f} dB); noise in the pauses -{att:.2f} dB "
          f"over {pm.mean():.0%} of the clip")
    assert abs(snr_in - 15.0) < 1e-9 and pm.mean() > 0.2
    assert snr_out - snr_in >= 6.0
    assert 12.0 <= att < 18.06


# ------------------------------------------------------------------------------------------------------------------------ plumbing
def _upload(seconds=3.0, seed=21, sr=24000, channels=1):
    """A noisy speech-like upload as (wave [ch, n] float32 torch, sr)."""
    n = int(seconds * sr)
    x = R.noisy_speech(int(seconds * R.RATE), seed)[1]
    if sr != R.RATE:
        x = np.interp(np.arange(n) * (R.RATE / sr), np.arange(len(x)), x)
    w = np.stack([x * (1.0 - 0.1 * c) for c in range(channels)]).astype(np.float32)
    return torch.from_numpy(w), sr


@pytest.mark.parametrize("sr,channels", [(24000, 1), (16000, 2)])
def test_prepared_voice_denoise(sr, channels):
    clip = _upload(2.0, 22, sr, channels)
    plain = infer.PreparedVoice(clip)
    den = infer.PreparedVoice(clip, denoise=True)
    want = torch.from_numpy(AP.denoise_reference(plain.audio[0].numpy()))[None]
    assert den.denoise and not plain.denoise
    assert torch.equal(den.audio, want) and not torch.equal(den.audio, plain.audio)
    assert torch.equal(den.rms, plain.rms) and den.seconds == plain.seconds and den.ref_frames == plain.ref_frames
    before = dict(infer.DENOISE_COUNTS)
    lazy = infer.PreparedVoice.deferred(clip, denoise=True)
    other = infer.PreparedVoice.deferred(clip)
    assert lazy.audio is None and lazy.denoise and lazy.ref_frames == plain.ref_frames and lazy.seconds == plain.seconds
    infer.prepare_voices([other], device=None)
    assert dict(infer.DENOISE_COUNTS) == before                                  # a batch with no flagged voice: no denoise call
    infer.prepare_voices([lazy, other], device=None)
    assert infer.DENOISE_COUNTS["host_clips"] == before.get("host_clips", 0) + 1
    assert torch.equal(lazy.audio, want) and torch.equal(lazy.rms, plain.rms) and torch.equal(other.audio, plain.audio)


def test_over_long_clips_are_refused_at_both_constructors():
    limit = AP.DENOISE_MAX_SAMPLES
    for n, sr in ((limit + 1, 24000), (2 * limit + 2, 48000)):
        clip = (torch.zeros(1, n), sr)
        with pytest.raises(ValueError, match=f"DENOISE_MAX_SAMPLES = {limit}"):
            infer.PreparedVoice(clip, denoise=True)
        with pytest.raises(ValueError, match=f"DENOISE_MAX_SAMPLES = {limit}"):
            infer.PreparedVoice.deferred(clip, denoise=True)
        assert infer.PreparedVoice.deferred(clip).pending is not None           # without the flag the length is nobody's business
    assert infer.PreparedVoice.deferred((torch.zeros(1, limit), 24000), denoise=True).denoise


# ------------------------------------------------------------------------------------------------------------------------ serving
class NoiseModel:
    """Stand-in with F5HipModel's batch interface: a unit's mel is its noise plus a closed form of its own prompt and tokens."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def cond_mel(self, audio):
        n = audio.shape[-1] // 256
        return audio[0, : n * 256].reshape(n, 256).abs().mean(1, keepdim=True).repeat(1, 100)[None]

    def sample_units(self, cond, units, *, steps, cfg_strength, sway_sampling_coef, generators=None, ode_method=None):
        conds = list(cond) if isinstance(cond, (list, tuple)) else [cond] * len(units)
        gens = generators if generators is not None else [None] * len(units)
        self.calls.append(len(units))
        return [torch.randn(frames, 100, generator=g) * 0.05 + float(c.sum()) * 1e-4 + sum(map(ord, "".join(tokens))) * 1e-5
                for c, (tokens, frames), g in zip(conds, units, gens)]


class Vocoder:
    def _wave(self, mel):
        return torch.repeat_interleave(mel.mean(0), 256) * 0.5 + 0.1 * torch.sin(torch.arange(256 * mel.shape[-1], dtype=torch.float32) * 0.01)

    def decode(self, mel):
        return self._wave(mel[0])[None]

    def decode_ragged(self, mels):
        return [self._wave(m) for m in mels]


def _wav(clip):
    x, sr = clip
    buf = io.BytesIO()
    with wave.open(buf, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(sr)
        f.writeframes(infer.quantise_pcm16(x[0].numpy()).tobytes())
    return buf.getvalue()


UP = _wav(_upload(3.0, 23))
OTHER = _wav(_upload(2.5, 24))
RT, TEXT = "some reference words", "Hello there, this is the text."


@pytest.mark.parametrize("device_frontend", [False, True])
def test_clip_cache_keeps_the_flag_apart(device_frontend):
    mgr = serve.TTSManager(nfe_step=4, device_frontend=device_frontend).load(NoiseModel(), Vocoder())
    plain, _ = mgr._clip_voice(UP, RT)
    den, _ = mgr._clip_voice(UP, RT, True, True)
    assert len(mgr._clip_cache) == 2 and plain is not den and den.denoise and not plain.denoise
    assert mgr._clip_voice(UP, RT, denoise=True)[0] is den and mgr._clip_voice(UP, RT, denoise=False)[0] is plain and len(mgr._clip_cache) == 2
    if device_frontend:
        assert den.pending is not None                                          # deferred: denoised with the batch it first rides in
        infer.prepare_voices([den, plain], device=None)
    assert torch.equal(den.audio, torch.from_numpy(AP.denoise_reference(plain.audio[0].numpy()))[None])
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="denoise"):
            mgr._clip_voice(UP, RT, True, bad)
        with pytest.raises(ValueError, match="denoise"):
            mgr.synthesize_clip(TEXT, UP, RT, denoise=bad)
    assert len(mgr._clip_cache) == 2 and mgr.model_obj.calls == []
    a = mgr.synthesize_clip(TEXT, UP, RT, seed=3)
    b = mgr.synthesize_clip(TEXT, UP, RT, seed=3, denoise=True)
    assert a.shape == b.shape and not np.array_equal(a, b)
    assert np.array_equal(np.concatenate(list(mgr.synthesize_clip_stream(TEXT, UP, RT, seed=3, denoise=True))), b)


def test_script_voices_take_denoise_on_uploads_only(tmp_path):
    p = tmp_path / "prompt.wav"
    p.write_bytes(OTHER)
    mgr = serve.TTSManager(nfe_step=4).load(NoiseModel(), Vocoder())
    script = "First the main voice. [town] Then the one from town."
    voices = dict(main=dict(ref_audio_path=str(p), ref_text=RT), town=dict(ref_audio=UP, ref_text=RT))
    plain = mgr.synthesize_script(script, voices, seed=5)
    den = mgr.synthesize_script(script, dict(voices, town=dict(voices["town"], denoise=True)), seed=5)
    assert plain.shape == den.shape and not np.array_equal(plain, den)
    assert np.array_equal(mgr.synthesize_script(script, dict(voices, town=dict(voices["town"], denoise=False)), seed=5), plain)
    assert mgr._clip_voice(UP, RT, True, True)[0].denoise and len(mgr._clip_cache) == 2
    calls = len(mgr.model_obj.calls)
    for bad, word in [(dict(voices, main=dict(voices["main"], denoise=True)), "registered"), (dict(voices, main=dict(voices["main"], denoise=False)), "registered"),
                      (dict(voices, town=dict(voices["town"], denoise="yes")), "true or false"), (dict(voices, town=dict(voices["town"], denoise=1)), "true or false"),
                      (dict(voices, town=dict(voices["town"], denoised=True)), "denoise")]:
        with pytest.raises(ValueError, match=word):
            mgr.synthesize_script(script, bad, seed=5)
        with pytest.raises(ValueError, match=word):
            mgr.synthesize_script_stream(script, bad, seed=5)
    assert len(mgr.model_obj.calls) == calls


def _pcm(r):
    assert r.status_code == 200, r.text
    return r.content


def test_routes(tmp_path):
    from fastapi.testclient import TestClient
    p = tmp_path / "prompt.wav"
    p.write_bytes(OTHER)
    reg = serve.VoiceRegistry()
    reg.add("KAN_F (Happy)", str(p), RT)
    mgr = serve.TTSManager(nfe_step=4).load(NoiseModel(), Vocoder())
    c = TestClient(serve.create_app(mgr, reg))
    up = base64.b64encode(UP).decode()
    # the clone route
    body = dict(text=TEXT, ref_audio=up, ref_text=RT, seed=6, response_format="pcm")
    plain, den = _pcm(c.post("/v1/audio/speech/clone", json=body)), _pcm(c.post("/v1/audio/speech/clone", json=dict(body, denoise=True)))
    assert plain == infer.quantise_pcm16(mgr.synthesize_clip(TEXT, UP, RT, seed=6)).tobytes()
    assert den == infer.quantise_pcm16(mgr.synthesize_clip(TEXT, UP, RT, seed=6, denoise=True)).tobytes() and den != plain
    assert _pcm(c.post("/v1/audio/speech/clone", json=dict(body, denoise=False))) == plain
    assert _pcm(c.post("/v1/audio/speech/clone", json=dict(body, denoise=True, stream=True))) == den
    # the script route
    script = "First the main voice. [town] Then the one from town."
    sbody = dict(text=script, voices=dict(main=dict(ref_audio_name="KAN_F (Happy)"), town=dict(ref_audio=up, ref_text=RT)), seed=6, response_format="pcm")
    flagged = dict(sbody, voices=dict(sbody["voices"], town=dict(sbody["voices"]["town"], denoise=True)))
    voices = dict(main=dict(ref_audio_path=str(p), ref_text=RT), town=dict(ref_audio=UP, ref_text=RT, denoise=True))
    sden = _pcm(c.post("/v1/audio/speech/script", json=flagged))
    assert sden == infer.quantise_pcm16(mgr.synthesize_script(script, voices, seed=6)).tobytes() and sden != _pcm(c.post("/v1/audio/speech/script", json=sbody))
    assert _pcm(c.post("/v1/audio/speech/script", json=dict(flagged, stream=True))) == sden
    calls = len(mgr.model_obj.calls)
    r = c.post("/v1/audio/speech/script", json=dict(sbody, voices=dict(sbody["voices"], main=dict(ref_audio_name="KAN_F (Happy)", denoise=True))))
    assert r.status_code == 400 and "registered" in r.json()["detail"]
    # the edit route keeps the recording
    for value in (True, False):
        r = c.post("/v1/audio/edit", json=dict(audio=up, text="new words here", parts_to_edit=[[0.5, 1.0]], denoise=value))
        assert r.status_code == 400 and "denoise" in r.json()["detail"], r.text
    assert len(mgr.model_obj.calls) == calls
    fields = serve.request_models()
    assert fields.CloneRequest.model_fields["denoise"].default is False
    for bad in ("yes", 1, None):                                                 # a script voice's flag is true or false
        r = c.post("/v1/audio/speech/script", json=dict(sbody, voices=dict(sbody["voices"], town=dict(sbody["voices"]["town"], denoise=bad))))
        assert r.status_code == 400 and "true or false" in r.json()["detail"], r.text
    assert len(mgr.model_obj.calls) == calls
    assert "denoise" not in fields.SynthesizeRequest.model_fields and "denoise" not in fields.KannadaSynthesizeRequest.model_fields
