"""CPU: the reference-clip report's host definition (audio_prep.assess_reference) against its plain-loop restatement (tests/assess_ref.py):
the clipping rule's cases, the degenerate clips, the bandwidth of band-limited and full-band hosts, the SNR calibration against SNRs known
from the hosts' clean and noise parts, then the gate (`TTSManager(reference_limits=...)`), `check_reference` and its route on CPU stand-ins.

Calibration hosts: `denoise_ref.speechlike` (40 % pauses) plus white noise at 5, 15 and 25 dB.  The reading must order the hosts and lie
within 3 dB of the in-band SNR of the known parts.  Measured with ASSESS_FLOOR_TO_MEAN = -1 / ln(0.8) as derived (no tuning): errors of
-1.03, -1.53 and -2.22 dB (seed 11); the noise floor reads 0.8 to 2.2 dB high because the speech's own frames raise each bin's 20 % quantile,
the more the cleaner the clip."""
import base64
import io
import math
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import assess_ref as A  # noqa: E402
import denoise_ref as R  # noqa: E402
from tts_indic_server_f5_amd import audio_prep as AP  # noqa: E402
from tts_indic_server_f5_amd import infer, serve  # noqa: E402


def test_constants():
    assert (AP.ASSESS_HOT, AP.ASSESS_MIN_PEAK, AP.ASSESS_MIN_RUN) == (A.HOT, A.MIN_PEAK, A.MIN_RUN) == (1 - 2.0 ** -10, 0.25, 3)
    assert np.float32(AP.ASSESS_HOT) == AP.ASSESS_HOT                            # exact in float32
    assert AP.ASSESS_BAND == (A.BAND[0], A.BAND[-1]) == (3, 341)
    assert AP.ASSESS_FLOOR_TO_MEAN == A.FLOOR_TO_MEAN == -1.0 / math.log(0.8)
    assert abs(1.0 / AP.ASSESS_FLOOR_TO_MEAN - 0.2231) < 5e-5                    # the 20 % quantile of an exponential power over its mean
    assert (AP.ASSESS_SPEECH_FACTOR, AP.ASSESS_MEAN_BINS, AP.ASSESS_BANDWIDTH_REL) == (A.SPEECH_FACTOR, A.MEAN_BINS, A.BANDWIDTH_REL)
    assert AP.ASSESS_MAX_SAMPLES == 1_440_000 and len(AP.ASSESS_ROW) == 10
    assert AP.REFERENCE_LIMITS == ("min_seconds", "max_clip_ratio", "min_snr_db", "min_speech_ratio", "min_bandwidth_hz")


@pytest.mark.parametrize("name", list(A.run_cases()))
def test_run_rule(name):
    x, want = A.run_cases()[name]
    peak, clipped = AP.assess_clipping(x)
    assert (peak, clipped) == A.clipping(x) and clipped == want
    assert peak.dtype == np.float32 and peak == np.abs(x).max()
    report = AP.assess_reference(x, 8000, np.zeros(16))
    assert report.clipped == want and report.clip_ratio == want / x.size and report.seconds == x.shape[1] / 8000


def test_run_rule_on_random_clips():
    rng = np.random.default_rng(3)
    for _ in range(40):
        ch, n = int(rng.integers(1, 4)), int(rng.integers(1, 60))
        x = rng.choice(np.array([1.0, -1.0, 32767 / 32768, 0.999, 0.5, 0.0], dtype=np.float32), size=(ch, n), p=[.3, .2, .1, .1, .2, .1])
        assert AP.assess_clipping(x) == A.clipping(x)


@pytest.mark.parametrize("name,x", [("zeros", np.zeros(5000)), ("dc", np.full(3000, 0.25)), ("one_sample", np.full(1, 0.7))])
def test_degenerate_clips_have_defined_values(name, x):
    r = AP.assess_reference(x.astype(np.float32)[None], 24000, x, rms=0.1)
    s = AP.assess_spectrum(x)
    assert r.clipped == 0 and r.clip_ratio == 0.0 and r.rms == 0.1 and r.peak == float(np.float32(x[0]))
    if name == "zeros":
        assert (r.noise_db, r.snr_db, r.speech_ratio, r.bandwidth_hz) == (-math.inf, math.inf, 0.0, 0.0)
        assert r.as_json()["noise_db"] is None and r.as_json()["snr_db"] is None and r.as_json()["clipped"] == 0
    if name == "one_sample":
        assert s["F"] == 4 and R.rank(4) == 0                                    # the sample sits under w[0] = 0 in one of its four frames: the floor is 0 in every bin
        assert (r.noise_db, r.snr_db, r.speech_ratio) == (-math.inf, math.inf, 0.75)
    ref = A.spectrum(x)
    for key in A.FLOAT_MEASURES:
        assert s[key] == ref[key] or abs(s[key] - ref[key]) <= 1e-9 * abs(ref[key]), key


@pytest.mark.parametrize("n", R.LENGTHS)
def test_definition_equals_the_restatement(n):
    x = R.clip(n)
    s, ref = AP.assess_spectrum(x), A.spectrum(x)
    assert s["F"] == ref["F"] == R.n_frames(n)
    assert s["k_star"] == ref["k_star"] and s["speech_frames"] == ref["speech_frames"]
    for key in A.FLOAT_MEASURES:
        assert s[key] == ref[key] or abs(s[key] - ref[key]) <= 1e-9 * max(abs(ref[key]), 1e-30), (key, s[key], ref[key])


def test_only_the_first_sixty_seconds_are_read():
    x = np.zeros(AP.ASSESS_MAX_SAMPLES + 5000)
    x[-5000:] = 0.5                                                              # content past the limit: not seen
    assert AP.assess_spectrum(x)["S"] == 0.0 and AP.assess_spectrum(x)["F"] == AP.denoise_frames(AP.ASSESS_MAX_SAMPLES)
    assert AP.assess_reference(x.astype(np.float32)[None], 24000, x).peak == 0.5  # the raw side reads the whole upload


def test_bandwidth_of_band_limited_and_full_band_hosts():
    clean, noise = A.calibration_host(15.0)
    full = AP.assess_spectrum(clean + noise)["bandwidth_hz"]
    # an 8 kHz recording's anti-alias filter: -6 dB at 3.8 kHz, 100 dB down from 3.95 kHz (`assess_ref.lowpass`)
    narrow = AP.assess_spectrum(A.lowpass(clean + noise, 3800.0))["bandwidth_hz"]
    print(f"[ref_assess] bandwidth_hz: full band {full:.1f}, 4 kHz low-pass {narrow:.1f}")
    assert full > 10000.0
    assert 3900.0 <= narrow <= 4100.0
    # the same host played from 16 kHz and from 44.1 kHz files: the reading is the content's, not the container's
    for sr in (16000, 44100):
        up = infer.resample_sinc_hann(torch.from_numpy(A.lowpass(clean + noise, 3800.0).astype(np.float32))[None], 24000, sr)
        back = infer.resample_sinc_hann(up, sr, 24000)[0].numpy()
        assert 3900.0 <= AP.assess_spectrum(back)["bandwidth_hz"] <= 4100.0, sr


def test_snr_calibration_against_the_known_parts():
    readings = []
    for snr in (5.0, 15.0, 25.0):
        clean, noise = A.calibration_host(snr)
        true = A.true_snr_db(clean, noise)                                       # from the parts, inside the band: nominal + 1.76 dB
        s = AP.assess_spectrum(clean + noise)
        true_noise = 10.0 * math.log10(A.spectrum(noise)["S"])
        print(f"[ref_assess] host at {snr:g} dB: in-band SNR of the parts {true:.2f} dB, snr_db {s['snr_db']:.2f} (error {s['snr_db'] - true:+.2f}); "
              f"noise of the part {true_noise:.2f} dB, noise_db {s['noise_db']:.2f}; speech_ratio {s['speech_ratio']:.3f}")
        assert abs(true - (snr + 10.0 * math.log10(1.5))) < 0.2                  # white noise: two thirds of it lie in the band
        assert abs(s["snr_db"] - true) <= 3.0
        assert abs(s["noise_db"] - true_noise) <= 3.0
        readings.append(s["snr_db"])
    assert readings[0] < readings[1] < readings[2]


def test_weak_case_a_voice_without_pauses_reads_low():
    n = 6 * R.RATE
    t = np.arange(n) / R.RATE
    buzz = sum(np.sin(2 * np.pi * 120.0 * h * t + h) / h for h in range(1, 30)) * (0.8 + 0.2 * np.sin(2 * np.pi * 3.0 * t))
    s = AP.assess_spectrum(0.1 * buzz)                                           # no noise at all, yet:
    assert s["snr_db"] < 10.0 or s["snr_db"] == -math.inf


# ------------------------------------------------------------------------------------------------------------------------ limits
def test_limits_are_checked_at_construction():
    assert AP.check_reference_limits(None) is None
    assert AP.check_reference_limits(dict(min_snr_db=10, max_clip_ratio=0.001)) == dict(min_snr_db=10.0, max_clip_ratio=0.001)
    for bad, word in ((dict(min_snr=3), "unknown limit 'min_snr'"), (dict(min_snr_db="3"), "min_snr_db"), (dict(min_seconds=True), "min_seconds"),
                      (dict(min_seconds=math.nan), "finite"), ([("min_seconds", 1)], "dict")):
        with pytest.raises(ValueError, match=word):
            serve.TTSManager(reference_limits=bad)
        with pytest.raises(ValueError, match=word):
            infer.PreparedVoice.deferred((torch.zeros(1, 100), 24000), limits=bad)
    assert serve.TTSManager().reference_limits is None


def test_gate_messages_name_measure_value_and_limit():
    r = AP.ReferenceReport(seconds=2.0, rms=0.1, peak=1.0, clipped=50, clip_ratio=0.01, noise_db=-30.0, snr_db=8.0, speech_ratio=0.3, bandwidth_hz=3984.375)
    limits = AP.check_reference_limits(dict(min_seconds=3, max_clip_ratio=0.001, min_snr_db=15, min_speech_ratio=0.2, min_bandwidth_hz=6000))
    got = AP.reference_problems(r, limits)
    assert got == ["the reference clip's seconds is 2, below the limit min_seconds = 3",
                   "the reference clip's clip_ratio is 0.01, above the limit max_clip_ratio = 0.001",
                   "the reference clip's snr_db is 8, below the limit min_snr_db = 15",
                   "the reference clip's bandwidth_hz is 3984.38, below the limit min_bandwidth_hz = 6000"]
    assert [p for p in got if "snr_db" not in p] == AP.reference_problems(r, limits, denoise=True)      # the denoiser is the remedy
    assert AP.reference_problems(r, None) == [] and AP.reference_problems(r, {}) == []
    assert AP.reference_problems(r._replace(snr_db=-math.inf), dict(min_snr_db=-100.0)) != []           # an infinity compares like any value
    assert AP.reference_problems(r._replace(snr_db=math.inf), dict(min_snr_db=100.0)) == []


# ------------------------------------------------------------------------------------------------------------------------ plumbing
def _upload(seconds=3.0, seed=21, sr=24000, channels=1, snr_db=15.0, clip_at=None):
    """A noisy speech-like upload as (wave [ch, n] float32 torch, sr); `clip_at`: hard-clipped at that level and scaled to full scale."""
    n = int(seconds * sr)
    x = R.noisy_speech(int(seconds * R.RATE), seed, snr_db)[1]
    if sr != R.RATE:
        x = np.interp(np.arange(n) * (R.RATE / sr), np.arange(len(x)), x)
    if clip_at is not None:
        x = np.clip(x, -clip_at, clip_at) / clip_at
    w = np.stack([x * (1.0 - 0.1 * c) for c in range(channels)]).astype(np.float32)
    return torch.from_numpy(w), sr


@pytest.mark.parametrize("sr,channels", [(24000, 1), (16000, 2)])
def test_prepared_voice_report(sr, channels):
    clip = _upload(2.0, 22, sr, channels)
    before = dict(infer.ASSESS_COUNTS)
    plain = infer.PreparedVoice(clip)
    assert plain.report is None and not plain.assess and dict(infer.ASSESS_COUNTS) == before
    v = infer.PreparedVoice(clip, assess=True)
    want = AP.assess_reference(clip[0].numpy(), sr, plain.audio[0].numpy(), rms=float(plain.rms))
    assert v.report == want and v.report.seconds == plain.seconds and v.report.rms == float(plain.rms)
    assert torch.equal(v.audio, plain.audio) and torch.equal(v.rms, plain.rms)  # measuring changes nothing
    lazy, other = infer.PreparedVoice.deferred(clip, assess=True), infer.PreparedVoice.deferred(clip)
    assert lazy.report is None and lazy.assess and not other.assess
    infer.prepare_voices([lazy, other], device=None)
    assert lazy.report == want and other.report is None and torch.equal(lazy.audio, plain.audio)
    assert infer.ASSESS_COUNTS["host_clips"] == before.get("host_clips", 0) + 2 and infer.ASSESS_COUNTS["device_calls"] == before.get("device_calls", 0)
    # limits imply the report; a violated one is refused by both constructors' paths, min_snr_db not with denoise
    low = dict(min_snr_db=want.snr_db + 1.0)
    with pytest.raises(ValueError, match="snr_db is .* below the limit min_snr_db"):
        infer.PreparedVoice(clip, limits=low)
    gated = infer.PreparedVoice.deferred(clip, limits=low)
    with pytest.raises(ValueError, match="snr_db"):
        infer.prepare_voices([gated], device=None)
    assert gated.pending is not None and gated.audio is None                     # a refused voice stays deferred
    passed = infer.PreparedVoice(clip, limits=low, denoise=True)
    assert passed.report == want and passed.denoise                              # measured before the denoiser, and let through
    assert infer.PreparedVoice(clip, limits=dict(min_snr_db=want.snr_db - 1.0)).report == want


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
        f.setnchannels(x.shape[0]); f.setsampwidth(2); f.setframerate(sr)
        f.writeframes(np.ascontiguousarray(infer.quantise_pcm16(x.numpy().T)).tobytes())
    return buf.getvalue()


CLEAN = _wav(_upload(3.0, 23, snr_db=25.0))
NOISY = _wav(_upload(3.0, 23, snr_db=5.0))
CLIPPED = _wav(_upload(3.0, 23, snr_db=25.0, clip_at=0.08))
RT, TEXT = "some reference words", "Hello there, this is the text."
LIMITS = dict(max_clip_ratio=0.001, min_snr_db=12.0)


@pytest.mark.parametrize("device_frontend", [False, True])
def test_manager_refuses_before_cache_and_sampler(device_frontend):
    mgr = serve.TTSManager(nfe_step=4, device_frontend=device_frontend, reference_limits=LIMITS).load(NoiseModel(), Vocoder())
    with pytest.raises(ValueError, match="clip_ratio is .* above the limit max_clip_ratio = 0.001"):
        mgr.synthesize_clip(TEXT, CLIPPED, RT, seed=3)
    with pytest.raises(ValueError, match="snr_db is .* below the limit min_snr_db = 12"):
        mgr.synthesize_clip(TEXT, NOISY, RT, seed=3)
    assert len(mgr._clip_cache) == 0 and mgr.model_obj.calls == []               # neither cached nor sampled
    before = infer.ASSESS_COUNTS["host_clips"]
    with pytest.raises(ValueError, match="snr_db"):                              # refused again: a refused upload was not cached
        mgr.synthesize_clip(TEXT, NOISY, RT, seed=3)
    assert infer.ASSESS_COUNTS["host_clips"] == before + 1
    den = mgr.synthesize_clip(TEXT, NOISY, RT, seed=3, denoise=True)             # min_snr_db is not applied with denoise
    with pytest.raises(ValueError, match="clip_ratio"):                          # ... the other limits are
        mgr.synthesize_clip(TEXT, CLIPPED, RT, seed=3, denoise=True)
    ok = mgr.synthesize_clip(TEXT, CLEAN, RT, seed=3)
    count = infer.ASSESS_COUNTS["host_clips"]
    assert np.array_equal(mgr.synthesize_clip(TEXT, CLEAN, RT, seed=3), ok) and infer.ASSESS_COUNTS["host_clips"] == count   # once per upload
    voice = mgr._clip_voice(CLEAN, RT)[0]
    assert voice.report is not None and voice.report.snr_db >= 12.0 and voice.report.clipped == 0
    # a script's upload is gated the same way, a registered voice is not
    script = "First the main voice. [town] Then the one from town."
    with pytest.raises(ValueError, match="snr_db"):
        mgr.synthesize_script(script, dict(main=dict(ref_audio=CLEAN, ref_text=RT), town=dict(ref_audio=NOISY, ref_text=RT)), seed=5)
    assert len(den) > 0 and len(mgr._clip_cache) == 2


@pytest.mark.parametrize("device_frontend", [False, True])
def test_no_limits_measure_nothing_and_change_nothing(device_frontend, tmp_path):
    p = tmp_path / "prompt.wav"
    p.write_bytes(NOISY)
    before = dict(infer.ASSESS_COUNTS)
    plain = serve.TTSManager(nfe_step=4, device_frontend=device_frontend).load(NoiseModel(), Vocoder())
    gated = serve.TTSManager(nfe_step=4, device_frontend=device_frontend, reference_limits=dict(min_snr_db=-50.0)).load(NoiseModel(), Vocoder())
    script = "First the main voice. [town] Then the one from town."
    voices = dict(main=dict(ref_audio_path=str(p), ref_text=RT), town=dict(ref_audio=CLIPPED, ref_text=RT))
    a = [plain.synthesize_clip(TEXT, NOISY, RT, seed=3), plain.synthesize_clip(TEXT, CLEAN, RT, seed=4, denoise=True), plain.synthesize_script(script, voices, seed=5)]
    assert dict(infer.ASSESS_COUNTS) == before and plain._clip_voice(NOISY, RT)[0].report is None
    b = [gated.synthesize_clip(TEXT, NOISY, RT, seed=3), gated.synthesize_clip(TEXT, CLEAN, RT, seed=4, denoise=True), gated.synthesize_script(script, voices, seed=5)]
    assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))       # a gate that passes serves the same bytes
    assert infer.ASSESS_COUNTS["host_clips"] == before.get("host_clips", 0) + 3          # the three uploads, not the registered voice


def test_check_reference_and_route():
    from fastapi.testclient import TestClient
    mgr = serve.TTSManager(nfe_step=4, reference_limits=LIMITS).load(NoiseModel(), Vocoder())
    c = TestClient(serve.create_app(mgr, serve.VoiceRegistry()))
    report = mgr.check_reference(NOISY)
    assert isinstance(report, infer.ReferenceReport) and report == mgr.check_reference(NOISY) and len(mgr._clip_cache) == 0
    # ... exactly as a clone upload would be measured
    free = serve.TTSManager(nfe_step=4, reference_limits=dict(min_seconds=0.0)).load(NoiseModel(), Vocoder())
    assert free._clip_voice(NOISY, RT)[0].report == report
    r = c.post("/v1/audio/reference/check", json=dict(audio=base64.b64encode(NOISY).decode()))
    assert r.status_code == 200, r.text
    assert r.json()["report"] == report.as_json() and set(r.json()["report"]) == set(infer.ReferenceReport._fields)
    assert r.json()["problems"] == mgr.reference_problems(report) and len(r.json()["problems"]) == 1 and "min_snr_db = 12" in r.json()["problems"][0]
    r = c.post("/v1/audio/reference/check", json=dict(audio=base64.b64encode(CLIPPED).decode(), clip_short=False))
    assert r.status_code == 200 and r.json()["report"]["clipped"] > 0 and "max_clip_ratio" in r.json()["problems"][0]
    # a clip with digital silence between its words has a floor of zero: the infinities are null
    x = R.speechlike(3 * R.RATE, 7)
    r = c.post("/v1/audio/reference/check", json=dict(audio=base64.b64encode(_wav((torch.from_numpy(x.astype(np.float32))[None], 24000))).decode()))
    assert r.status_code == 200 and r.json()["report"]["noise_db"] is None and r.json()["report"]["snr_db"] is None and r.json()["problems"] == []
    # without limits: a report and no problems
    c2 = TestClient(serve.create_app(serve.TTSManager(nfe_step=4).load(NoiseModel(), Vocoder()), serve.VoiceRegistry()))
    r = c2.post("/v1/audio/reference/check", json=dict(audio=base64.b64encode(NOISY).decode()))
    assert r.status_code == 200 and r.json()["problems"] == [] and r.json()["report"] == report.as_json()
    # a bad upload is the clone route's 400
    clone = c.post("/v1/audio/speech/clone", json=dict(text=TEXT, ref_audio="@@@", ref_text=RT))
    r = c.post("/v1/audio/reference/check", json=dict(audio="@@@"))
    assert r.status_code == clone.status_code == 400 and r.json() == clone.json()
    junk = base64.b64encode(b"RIFFxxxxjunk").decode()
    clone = c.post("/v1/audio/speech/clone", json=dict(text=TEXT, ref_audio=junk, ref_text=RT))
    r = c.post("/v1/audio/reference/check", json=dict(audio=junk))
    assert r.status_code == clone.status_code == 400 and r.json() == clone.json()
    silent = base64.b64encode(_wav((torch.zeros(1, 24000), 24000))).decode()
    r = c.post("/v1/audio/reference/check", json=dict(audio=silent))
    assert r.status_code == 400 and "empty or silent" in r.json()["detail"]
    assert mgr.model_obj.calls == []
    # the existing routes' models are what they were
    fields = serve.request_models()
    assert set(fields.ReferenceCheckRequest.model_fields) == {"audio", "clip_short"}
    assert not any(name.startswith(("assess", "limits", "reference_limits")) for m in (fields.CloneRequest, fields.ScriptVoice, fields.SynthesizeRequest)
                   for name in m.model_fields)
    assert "assess" not in infer.REQUEST_OPTIONS and "reference_limits" not in infer.REQUEST_OPTIONS
