"""CPU: the per-voice `dereverb` option of uploaded reference clips on the host -- the definition `audio_prep.dereverb_reference` (single-channel
WPE) against its independent restatement (tests/dereverb_ref.py), its laws, its effect on synthetic reverberant hosts, the float32 run's error
on the clips the device test uses, and the plumbing through `infer.PreparedVoice`, `infer.prepare_voices(device=None)`, `serve.TTSManager`
(clip cache, script voices) and the routes, on the denoiser tests' CPU stand-in models.

Measured with the float64 definition when this was written (3.5 s hosts, seeds 1, 2, 3): the late-to-early ratio falls by 1.55, 2.44 and
1.17 dB at T60 0.3 s and by 1.33, 1.28 and 0.80 dB at T60 0.6 s; a dry clip changes at -37.1, -32.7 and -29.4 dB relative to itself.  The
thresholds below are half the smallest improvement (0.40 dB) and the worst dry change plus 3 dB (-26.4 dB)."""
import base64

import numpy as np
import pytest
import torch

import dereverb_ref as R
from test_denoise_host import RT, TEXT, NoiseModel, Vocoder, _pcm, _wav
from tts_indic_server_f5_amd import audio_prep as AP
from tts_indic_server_f5_amd import infer, ops, serve

SECONDS, SEEDS = 3.5, (1, 2, 3)


# ------------------------------------------------------------------------------------------------------------------------ the definition
def test_constants():
    assert (AP.DEREVERB_DELAY, AP.DEREVERB_TAPS, AP.DEREVERB_ITERATIONS) == (R.DELAY, R.TAPS, R.ITERATIONS) == (4, 16, 3)
    assert (AP.DEREVERB_FLOOR, AP.DEREVERB_LOAD, AP.DEREVERB_TINY) == (R.FLOOR, R.LOAD, R.TINY)
    assert AP.DEREVERB_MAX_SAMPLES == AP.DENOISE_MAX_SAMPLES


@pytest.fixture(scope="module")
def device_clips():
    return R.device_clips(ops.ref_dereverb_chunk())


@pytest.mark.parametrize("name", ["short_one_tap", "line_short_by_one", "line_full", "seconds_1p5", "dc"])
def test_definition_equals_the_restatement(device_clips, name):
    x = device_clips[name]
    want, got64 = R.dereverb(x, np.float64), AP.dereverb_reference_f64(x)
    err = np.abs(got64 - want).max()
    print(f"[dereverb] {name}: definition vs restatement max |diff| {err:.3e}")
    assert err < 1e-12                                                           # float64 sums in another order
    assert AP.dereverb_reference(x).dtype == np.float32 and np.array_equal(AP.dereverb_reference(x), got64.astype(np.float32))
    assert np.abs(got64 - x).max() > 1e-4                                        # and the taps did something


def test_laws():
    x = R.device_clips(128)
    for name in ("one_sample", "no_tap"):                                        # F <= D: no tap, the STFT round trip
        assert R.n_frames(len(x[name])) <= AP.DEREVERB_DELAY
        assert np.abs(AP.dereverb_reference_f64(x[name]) - x[name]).max() < 1e-15
    assert not AP.dereverb_reference_f64(x["zeros"]).any()                       # zeros stay zero
    for clip in x.values():                                                      # the length is kept
        assert AP.dereverb_reference(clip).shape == clip.shape
    assert np.array_equal(AP.dereverb_reference(x["line_full"][None]), AP.dereverb_reference(x["line_full"]))
    with pytest.raises(ValueError, match="empty"):
        AP.dereverb_reference(np.zeros(0))
    with pytest.raises(ValueError, match=f"DEREVERB_MAX_SAMPLES = {AP.DEREVERB_MAX_SAMPLES}"):
        AP.dereverb_reference(np.zeros(AP.DEREVERB_MAX_SAMPLES + 1))


@pytest.mark.parametrize("t60", [0.3, 0.6])
@pytest.mark.parametrize("seed", SEEDS)
def test_late_to_early_ratio_falls(t60, seed):
    rev, early = R.host(SECONDS, t60, seed)
    before, after = R.late_to_early_db(rev, early), R.late_to_early_db(AP.dereverb_reference_f64(rev), early)
    print(f"[dereverb] T60 {t60} s seed {seed}: late-to-early {before:.2f} dB -> {after:.2f} dB, improvement {before - after:.2f} dB")
    assert before - after >= 0.40


@pytest.mark.parametrize("seed", SEEDS)
def test_a_dry_clip_is_left_nearly_alone(seed):
    dry = R.dry_speech(int(SECONDS * R.RATE), seed)
    out = AP.dereverb_reference_f64(dry)
    change = 10.0 * np.log10(np.sum((out - dry) ** 2) / np.sum(dry ** 2))
    print(f"[dereverb] dry clip seed {seed}: changed at {change:.1f} dB relative to itself")
    assert change < -26.4


def test_the_float32_run_stays_under_the_device_tolerance_cap(device_clips):
    """What `min(16 x float32 error, 1e-4)` of tests/test_gpu_ref_dereverb.py rests on: at a peak of at most 0.5 the float32 run alone is under
    1e-4 / 16 on every clip of the device test, so the cap never widens a clip's tolerance."""
    for name, x in device_clips.items():
        err32 = np.abs(R.dereverb(x, np.float32).astype(np.float64) - R.dereverb(x, np.float64)).max()
        print(f"[dereverb] {name}: n={len(x)} F={R.n_frames(len(x))} peak {np.abs(x).max():.3f} float32 run max |err| {err32:.3e}")
        assert np.abs(x).max() <= 0.5 and err32 <= 1e-4 / 16


# ------------------------------------------------------------------------------------------------------------------------ plumbing
def _upload(seconds, seed, sr=24000):
    x = R.host(seconds, 0.3, seed)[0]
    if sr != R.RATE:
        x = np.interp(np.arange(int(seconds * sr)) * (R.RATE / sr), np.arange(len(x)), x)
    return torch.from_numpy((0.2 * x).astype(np.float32))[None], sr


UP, OTHER = _wav(_upload(1.5, 23)), _wav(_upload(1.2, 24))


def test_prepared_voice_dereverb_runs_in_front_of_denoise():
    clip = _upload(1.2, 22, 16000)
    plain = infer.PreparedVoice(clip)
    want = torch.from_numpy(AP.dereverb_reference(plain.audio[0].numpy()))[None]
    rev, both = infer.PreparedVoice(clip, dereverb=True), infer.PreparedVoice(clip, dereverb=True, denoise=True)
    assert rev.dereverb and not plain.dereverb and torch.equal(rev.audio, want) and not torch.equal(want, plain.audio)
    assert torch.equal(both.audio, torch.from_numpy(AP.denoise_reference(want[0].numpy()))[None])
    assert torch.equal(rev.rms, plain.rms) and rev.seconds == plain.seconds and rev.ref_frames == plain.ref_frames
    before = dict(infer.DEREVERB_COUNTS)
    lazy, lazy_both, other = (infer.PreparedVoice.deferred(clip, **kw) for kw in (dict(dereverb=True), dict(dereverb=True, denoise=True), {}))
    infer.prepare_voices([other], device=None)
    assert dict(infer.DEREVERB_COUNTS) == before                                 # a batch with no flagged voice: no call
    infer.prepare_voices([lazy, lazy_both, other], device=None)
    assert infer.DEREVERB_COUNTS["host_clips"] == before.get("host_clips", 0) + 2
    assert torch.equal(lazy.audio, want) and torch.equal(lazy_both.audio, both.audio) and torch.equal(other.audio, plain.audio)
    long = (torch.zeros(1, AP.DEREVERB_MAX_SAMPLES + 1), 24000)
    for make in (infer.PreparedVoice, infer.PreparedVoice.deferred):
        with pytest.raises(ValueError, match="DEREVERB_MAX_SAMPLES"):
            make(long, dereverb=True)


@pytest.mark.parametrize("device_frontend", [False, True])
def test_clip_cache_keeps_the_flag_apart(device_frontend):
    mgr = serve.TTSManager(nfe_step=4, device_frontend=device_frontend).load(NoiseModel(), Vocoder())
    plain, _ = mgr._clip_voice(UP, RT)
    rev, _ = mgr._clip_voice(UP, RT, dereverb=True)
    assert len(mgr._clip_cache) == 2 and plain is not rev and rev.dereverb and not plain.dereverb and not rev.denoise
    assert mgr._clip_voice(UP, RT, dereverb=True)[0] is rev and mgr._clip_voice(UP, RT, True, False, False)[0] is plain and len(mgr._clip_cache) == 2
    if device_frontend:
        assert rev.pending is not None                                           # deferred: dereverberated with the batch it first rides in
        infer.prepare_voices([rev, plain], device=None)
    assert torch.equal(rev.audio, torch.from_numpy(AP.dereverb_reference(plain.audio[0].numpy()))[None])
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="dereverb"):
            mgr.synthesize_clip(TEXT, UP, RT, dereverb=bad)
    assert len(mgr._clip_cache) == 2 and mgr.model_obj.calls == []
    a, b = mgr.synthesize_clip(TEXT, UP, RT, seed=3), mgr.synthesize_clip(TEXT, UP, RT, seed=3, dereverb=True)
    assert a.shape == b.shape and not np.array_equal(a, b)
    assert np.array_equal(np.concatenate(list(mgr.synthesize_clip_stream(TEXT, UP, RT, seed=3, dereverb=True))), b)


def test_routes_and_script_voices(tmp_path):
    from fastapi.testclient import TestClient
    p = tmp_path / "prompt.wav"
    p.write_bytes(OTHER)
    reg = serve.VoiceRegistry()
    reg.add("KAN_F (Happy)", str(p), RT)
    mgr = serve.TTSManager(nfe_step=4).load(NoiseModel(), Vocoder())
    c = TestClient(serve.create_app(mgr, reg))
    up = base64.b64encode(UP).decode()
    body = dict(text=TEXT, ref_audio=up, ref_text=RT, seed=6, response_format="pcm")
    plain, rev = _pcm(c.post("/v1/audio/speech/clone", json=body)), _pcm(c.post("/v1/audio/speech/clone", json=dict(body, dereverb=True)))
    assert plain == infer.quantise_pcm16(mgr.synthesize_clip(TEXT, UP, RT, seed=6)).tobytes()
    assert rev == infer.quantise_pcm16(mgr.synthesize_clip(TEXT, UP, RT, seed=6, dereverb=True)).tobytes() and rev != plain
    assert _pcm(c.post("/v1/audio/speech/clone", json=dict(body, dereverb=False))) == plain
    assert _pcm(c.post("/v1/audio/speech/clone", json=dict(body, dereverb=True, stream=True))) == rev
    script = "First the main voice. [town] Then the one from town."
    sbody = dict(text=script, voices=dict(main=dict(ref_audio_name="KAN_F (Happy)"), town=dict(ref_audio=up, ref_text=RT)), seed=6, response_format="pcm")
    flagged = dict(sbody, voices=dict(sbody["voices"], town=dict(sbody["voices"]["town"], dereverb=True)))
    voices = dict(main=dict(ref_audio_path=str(p), ref_text=RT), town=dict(ref_audio=UP, ref_text=RT, dereverb=True))
    srev = _pcm(c.post("/v1/audio/speech/script", json=flagged))
    assert srev == infer.quantise_pcm16(mgr.synthesize_script(script, voices, seed=6)).tobytes() and srev != _pcm(c.post("/v1/audio/speech/script", json=sbody))
    assert _pcm(c.post("/v1/audio/speech/script", json=dict(flagged, stream=True))) == srev
    calls = len(mgr.model_obj.calls)
    r = c.post("/v1/audio/speech/script", json=dict(sbody, voices=dict(sbody["voices"], main=dict(ref_audio_name="KAN_F (Happy)", dereverb=True))))
    assert r.status_code == 400 and "dereverb" in r.json()["detail"] and "registered" in r.json()["detail"]
    r = c.post("/v1/audio/speech/script", json=dict(sbody, voices=dict(sbody["voices"], town=dict(sbody["voices"]["town"], dereverb="yes"))))
    assert r.status_code == 400 and "true or false" in r.json()["detail"], r.text
    for value in (True, False):                                                  # the edit route keeps the recording
        r = c.post("/v1/audio/edit", json=dict(audio=up, text="new words here", parts_to_edit=[[0.5, 1.0]], dereverb=value))
        assert r.status_code == 400 and "dereverb" in r.json()["detail"], r.text
    assert len(mgr.model_obj.calls) == calls
    fields = serve.request_models()
    assert fields.CloneRequest.model_fields["dereverb"].default is False and "dereverb" not in fields.SynthesizeRequest.model_fields
