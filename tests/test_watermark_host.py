"""The provenance watermark on the host (CPU): `wave_codec.mark_pcm16` / `detect_watermark` against their known answers, their plain
restatement (tests/watermark_ref.py) and their laws; the detection figures on the suite's synthetic speech-like hosts; robustness through the
delivery chain; the option through the planner, `finish_requests`, the manager and the routes over stand-in models; `reject_marked`.

The mark is compared as bytes.  The detector's bounds are the issue's: z >= 10 on clean and z >= 9 on 25 dB-noise hosts of 1 s, z < 6 for
unmarked and wrong-key clips (the threshold is 7), z >= 10 after each robustness step; definition against restatement |dz| <= 1e-9 (both
fp64: an FFT correlation against direct sums)."""
import base64
import dataclasses
import os

import numpy as np
import pytest
import torch

import watermark_ref as ref
from tts_indic_server_f5_amd import _lib, infer, serve, wave_codec

from test_script_host import RA, RB, SCRIPT, NoiseModel, Vocoder, _wav, B  # noqa: E402
from test_script_host import client as script_client  # noqa: E402,F401  (a manager without a model behind a TestClient)
from test_wave_encode_host import TEXT, _voice, client  # noqa: E402,F401  (the stand-in manager behind a TestClient)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 24000
KEY = 1
WRONG_KEYS = [2, 3, 0xDEADBEEF, 2 ** 47 + 5]
DEFAULTS = dict(speed=1.0, nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=None)


def _z(wave, key=KEY):
    return wave_codec.detect_watermark(wave, [key])[0]


# ------------------------------------------------------------------------------------------------ constants and known answers
def test_constants():
    assert (wave_codec.WATERMARK_PERIOD, wave_codec.WATERMARK_BLOCK, wave_codec.WATERMARK_TAPS, wave_codec.WATERMARK_SHIFT) == (16384, 240, 129, 23)
    assert wave_codec.WATERMARK_BAND == (22, 136) and wave_codec.WATERMARK_THRESHOLD == 7.0
    assert (wave_codec.WATERMARK_MIN_SAMPLES, wave_codec.WATERMARK_MAX_SAMPLES, wave_codec.WATERMARK_KEYS_MAX) == (12000, 1_440_000, 16)
    assert (ref.P, ref.BLOCK, ref.TAPS, ref.SHIFT, ref.BAND, ref.THRESHOLD, ref.MIN_SAMPLES, ref.MAX_SAMPLES) == (
        16384, 240, 129, 23, (22, 136), 7.0, 12000, 1_440_000)
    lo, hi = (k * RATE / 1024 for k in wave_codec.WATERMARK_BAND)
    assert round(lo) == 516 and round(hi) == 3188
    assert infer.mark_pcm16 is wave_codec.mark_pcm16 and infer.detect_watermark is wave_codec.detect_watermark


def test_generator_and_chip_known_answers():
    assert wave_codec.splitmix64(0)[1] == 0xE220A8397B1DCDAF == ref.splitmix_outputs(0, 1)[0]
    chips = wave_codec.watermark_chips(1)
    assert chips[:16].tolist() == [1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, 1, 1, -1, 1, -1]
    assert len(chips) == 16384 and set(chips.tolist()) == {1, -1} and int(chips.sum()) == -80
    for key in (1, 0xDEADBEEF, 2 ** 48 - 1):
        assert wave_codec.watermark_chips(key).tolist() == ref.chips(key)


def test_tap_file_is_the_formula():
    g = wave_codec.watermark_taps()
    assert g[62:67].tolist() == [1914, 3193, 3686, 3193, 1914] and int(g.sum()) == 28 and int(np.abs(g).sum()) == 34684
    assert g.tolist() == ref.taps() and np.array_equal(g, g[::-1])
    text = open(os.path.join(ROOT, "tts-indic-server-f5_amd", "csrc", "watermark_taps.inc")).read()
    body = "".join(line for line in text.splitlines() if not line.startswith("//"))
    assert [int(v) for v in body.replace(",", " ").split()] == g.tolist()
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_watermark_taps", os.path.join(ROOT, "tools", "gen_watermark_taps.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.text() == text


def test_carrier_known_answers():
    c = wave_codec.watermark_carrier(1)
    assert c.dtype == np.int16 and c.shape == (16384,) and not c.flags.writeable
    assert c[:8].tolist() == [-63, -441, -793, -936, -768, -311, 305, 899]
    c64 = c.astype(np.int64)
    assert int(c64.sum()) == -6412 and int((c64 * c64).sum()) == 14_442_340_954 and (int(c.min()), int(c.max())) == (-2863, 3113)
    assert wave_codec.watermark_carrier(1) is c                                        # cached
    for key in (1, 3, 2 ** 47 + 5):
        assert np.array_equal(wave_codec.watermark_carrier(key), ref.carrier(key))


def test_the_library_builds_the_same_carrier():
    lib = _lib.lib()                                                                   # loads without a GPU
    for key in (1, 0xDEADBEEF, 2 ** 48 - 1):
        out = np.zeros(16384, dtype=np.int16)
        assert lib.f5hip_watermark_carrier(key, out.ctypes.data) == 0
        assert np.array_equal(out, wave_codec.watermark_carrier(key))
    assert lib.f5hip_watermark_carrier(0, out.ctypes.data) != 0 and lib.f5hip_watermark_carrier(2 ** 48, out.ctypes.data) != 0
    assert lib.f5hip_wave_mark_tile() == 32 * 240 and lib.f5hip_watermark_detect_launches() == 4


def test_key_checks():
    assert wave_codec.check_watermark(None) is None and wave_codec.check_watermark(np.int64(7)) == 7
    assert wave_codec.check_watermark(2 ** 48 - 1) == 2 ** 48 - 1
    for bad in (True, False, 1.0, "1", 0, -1, 2 ** 48, [1], np.bool_(True)):
        with pytest.raises(ValueError) as e:
            wave_codec.check_watermark(bad)
        assert str(e.value) == f"watermark must be an integer key from 1 to 2^48 - 1 (got {bad!r})"
    assert wave_codec.check_watermark_keys(5) == [5] and wave_codec.check_watermark_keys((1, 2)) == [1, 2]
    for bad in ([], list(range(1, 18)), "12", None, [1, None]):
        with pytest.raises(ValueError, match="watermark keys must be a list of 1 to 16 keys"):
            wave_codec.check_watermark_keys(bad)
    with pytest.raises(ValueError, match="watermark must be an integer key"):
        wave_codec.check_watermark_keys([1, 2.0])


# ------------------------------------------------------------------------------------------------ the mark
MARK_LENGTHS = (1, 239, 240, 241, 481, 7680, 16385, 40000)


def _content(kind, n):
    if kind == "speech":
        return ref.host(max(n, 2), n)[:n]
    if kind == "full":                                                                 # full-scale square: the clip binds
        return np.where((np.arange(n) // 37) % 2 == 0, 32767, -32768).astype(np.int16)
    rng = np.random.default_rng(n)
    x = rng.integers(-3000, 3000, n).astype(np.int16)
    x[n // 3:n // 3 + 700] = 0                                                         # silence across blocks
    return x


@pytest.mark.parametrize("n", MARK_LENGTHS)
def test_mark_equals_the_restatement(n):
    for kind, key in (("speech", 1), ("full", 0xDEADBEEF), ("noise", 2 ** 47 + 5)):
        x = _content(kind, n)
        y = wave_codec.mark_pcm16(x, key)
        assert y.dtype == np.int16 and len(y) == n and np.array_equal(y, ref.mark(x, key)), (kind, n)


def test_mark_laws():
    zeros = np.zeros(50000, dtype=np.int16)
    assert not wave_codec.mark_pcm16(zeros, 1).any()                                   # zeros stay zeros
    x = ref.host(50000, 3)
    assert wave_codec.mark_pcm16(x, None) is x                                         # no key: the array itself
    assert len(wave_codec.mark_pcm16(np.zeros(0, dtype=np.int16), 1)) == 0
    y = wave_codec.mark_pcm16(x, 1)
    assert not np.array_equal(y, x) and not np.array_equal(y, wave_codec.mark_pcm16(x, 2))
    for wave in (x, _content("full", 40000), np.full(40000, 32767, dtype=np.int16)):
        for key in (1, 2, 0xDEADBEEF):
            assert np.abs(wave_codec.mark_pcm16(wave, key).astype(np.int64) - wave).max() <= 4064
    # locality: output block b depends on input blocks b - 1 .. b + 1 only
    rng = np.random.default_rng(0)
    for b in (0, 7, 100, 207):
        x2 = x.copy()
        x2[240 * b:240 * (b + 1)] = rng.integers(-20000, 20000, len(x2[240 * b:240 * (b + 1)]))
        y2 = wave_codec.mark_pcm16(x2, 1)
        lo, hi = 240 * max(b - 1, 0), 240 * (b + 2)
        assert np.array_equal(y2[:lo], y[:lo]) and np.array_equal(y2[hi:], y[hi:]) and not np.array_equal(y2[lo:hi], y[lo:hi])
        window = slice(240 * max(b - 2, 0), 240 * (b + 3))                             # ... and is what the blocks around it give alone
        alone = wave_codec.mark_pcm16(np.concatenate([np.zeros(window.start % 16384, dtype=np.int16), x2[window]]), 1)[window.start % 16384:]
        if window.start < 16384:                                                       # (the carrier index is kept by the zeros in front)
            assert np.array_equal(alone[240 * (b - max(b - 2, 0)):][:240], y2[240 * b:240 * (b + 1)])
    # a silent stretch keeps its zeros away from its edges
    quiet = x.copy()
    quiet[10000:20000] = 0
    yq = wave_codec.mark_pcm16(quiet, 1)
    assert not yq[240 * 43:240 * 82].any() and yq[:9000].any()


# ------------------------------------------------------------------------------------------------ the detector
def test_detect_equals_the_restatement():
    clips = [wave_codec.mark_pcm16(ref.host(20000, 1), 1), ref.host(16385, 2, noisy=True),
             (wave_codec.mark_pcm16(ref.host(30000, 3), 3)[5000:].astype(np.float32) / 32768.0)]
    for clip in clips:
        got = wave_codec.detect_watermark(clip, [1, 3])
        for g, (key, z, offset, detected) in zip(got, ref.detect(clip, [1, 3])):
            assert g.key == key and abs(g.z - z) <= 1e-9 and g.detected == detected, (g, z)
            if z >= wave_codec.WATERMARK_THRESHOLD:
                assert g.offset == offset
    assert [g.detected for g in wave_codec.detect_watermark(clips[0], [1, 3])] == [True, False]
    assert [g.detected for g in wave_codec.detect_watermark(clips[2], [1, 3])] == [False, True]
    assert wave_codec.detect_watermark(clips[2], [3])[0].offset == 5000


def test_detect_input_rules():
    y = wave_codec.mark_pcm16(ref.host(24000, 0), 1)
    short = wave_codec.detect_watermark(y[:11999], [1, 2])
    assert short == [wave_codec.WatermarkScore(1, 0.0, 0, False), wave_codec.WatermarkScore(2, 0.0, 0, False)] == [
        wave_codec.WatermarkScore(*s) for s in ref.detect(y[:11999], [1, 2])]
    assert _z(y[:12000]).detected
    a, b, c = _z(y), _z(y.astype(np.float64) / 32768.0), _z(torch.from_numpy(y.astype(np.float32) / 32768.0))
    assert a == b == c                                                                  # int16 is scaled by 1 / 32768 and scored in fp64
    # scale-invariant up to the 1e-10 under the square root, which only tells in bins 100 dB below full scale (|X|^2 near 1e-10): a bin with
    # |X|^2 >= 1e-7 moves by under 1e-3 of its unit modulus, so z (a ratio of sums over such bins) by far less than 1e-3 of itself
    scaled = _z(y.astype(np.float64) / 32768.0 * 3.7)
    assert abs(scaled.z - a.z) < 1e-3 * a.z and scaled.offset == a.offset
    assert _z(np.zeros(24000, dtype=np.int16)) == wave_codec.WatermarkScore(1, 0.0, 0, False)   # sigma = 0
    with pytest.raises(ValueError, match="int16 PCM or floating-point"):
        wave_codec.detect_watermark(y.astype(np.int32), [1])
    with pytest.raises(ValueError, match="not finite"):
        wave_codec.detect_watermark(np.array([np.nan] * 20000), [1])
    with pytest.raises(ValueError, match="watermark keys"):
        wave_codec.detect_watermark(y, [])
    # only the first WATERMARK_MAX_SAMPLES samples are read
    assert len(wave_codec._watermark_samples(np.zeros(wave_codec.WATERMARK_MAX_SAMPLES + 5, dtype=np.int16))) == wave_codec.WATERMARK_MAX_SAMPLES
    # float32 against float64 arithmetic of the same clip: the detector is not ill-conditioned
    assert abs(_z(y.astype(np.float32) / np.float32(32768.0)).z - a.z) < 1e-5


def test_detection_figures_on_the_synthetic_hosts():
    """Seeds 0 .. 11, key 1, hosts of 1 s at peak 12 000: every clean clip z >= 10, every clip in 25 dB white noise z >= 9, offset 0 in
    both; the same hosts unmarked, and marked but scored with four other keys: every z < 6."""
    for seed in range(12):
        for noisy, floor in ((False, 10.0), (True, 9.0)):
            x = ref.host(RATE, seed, noisy)
            assert int(np.abs(x).max()) == 12000
            y = wave_codec.mark_pcm16(x, KEY)
            scores = wave_codec.detect_watermark(y, [KEY] + WRONG_KEYS)
            assert scores[0].z >= floor and scores[0].offset == 0 and scores[0].detected, (seed, noisy, scores[0])
            assert all(s.z < 6.0 and not s.detected for s in scores[1:]), (seed, noisy, scores[1:])
            plain = _z(x)
            assert plain.z < 6.0 and not plain.detected, (seed, noisy, plain)


def _to_24k(pcm8):
    return infer.resample_sinc_hann(torch.from_numpy(pcm8.astype(np.float32) / 32768.0)[None], 8000, RATE)[0].numpy()


def test_robustness_through_the_delivery_chain():
    x = ref.host(3 * RATE, 0)
    y = wave_codec.mark_pcm16(x, KEY)
    assert _z(y).z >= 10 and _z(y).offset == 0
    cut = _z(y[7001:])
    assert cut.z >= 10 and cut.offset == 7001
    assert _z(infer.decode_g711(infer.encode_g711(y, "mulaw"), "mulaw")).z >= 10
    narrow = infer.decode_g711(infer.encode_g711(infer.resample_pcm16(y, 8000), "alaw"), "alaw")
    assert _z(_to_24k(narrow)).z >= 10
    loud = infer.normalise_loudness_pcm16(y, -30.0)
    assert not np.array_equal(loud, y) and _z(loud).z >= 10
    spec = infer.WaveSpec.of(dict(tempo=1.25, sample_rate=8000, encoding="mulaw"))
    sent = infer.finish_pcm16(x, dataclasses.replace(spec, watermark=KEY))                                         # tempo in front of the mark, 8 kHz mu-law behind it
    assert sent.dtype == np.uint8 and abs(len(sent) - len(x) / 1.25 / 3) <= 2
    got = _z(_to_24k(infer.decode_g711(sent, "mulaw")))
    assert got.z >= 10 and got.detected
    assert not _z(_to_24k(infer.decode_g711(infer.finish_pcm16(x, spec), "mulaw"))).detected


# ------------------------------------------------------------------------------------------------ plumbing
def test_request_options_layout():
    assert infer.REQUEST_OPTIONS.index("watermark") == 11 and infer.WATERMARK_OPTIONS == ("watermark",)
    assert infer.REQUEST_OPTIONS[-2:] == ("tempo", "pitch") and set(infer.REQUEST_OPTIONS[6:11]) == set(infer.DELIVERY_OPTIONS)
    assert infer.REQUEST_OPTIONS[6:11] == ("remove_silence", "sample_rate", "encoding", "loudness", "flac_level")
    assert infer.DELIVERY_OPTIONS == ("remove_silence", "loudness", "sample_rate", "encoding", "flac_level") and infer.PROSODY_OPTIONS == ("tempo", "pitch")
    assert serve.EDIT_DELIVERY == ("sample_rate", "encoding", "loudness", "flac_level") and serve.EDIT_MARK == ("watermark",)
    assert [f.name for f in dataclasses.fields(infer.WaveSpec)] == ["remove_silence", "loudness", "sample_rate", "encoding", "flac_level", "tempo", "pitch", "watermark", "keep_formants"]
    models = serve.request_models()
    for name in ("KannadaSynthesizeRequest", "SynthesizeRequest", "CloneRequest", "ScriptRequest", "EditRequest"):
        assert "watermark" in getattr(models, name).model_fields, name


def test_refusal_messages_and_whole_wave_rule():
    assert infer.needs_whole_wave(dict(watermark=5)) and infer.needs_whole_wave(dict(watermark=5), streamed=True)
    assert not infer.needs_whole_wave(dict(watermark=None))
    assert infer.whole_wave_message(dict(watermark=5)) == infer.WHOLE_WAVE_WATERMARK == wave_codec.WHOLE_WAVE_WATERMARK
    assert infer.whole_wave_message(dict(watermark=5, loudness=-20.0)) == infer.WHOLE_WAVE_LOUDNESS
    assert serve.stream_refusal(dict(watermark=5)) == serve.STREAM_WATERMARK
    assert serve.stream_refusal(dict(watermark=5, tempo=1.25)) == serve.STREAM_PROSODY
    assert serve.stream_refusal(dict(sample_rate=8000)) is None
    assert "whole wave" in serve.STREAM_WATERMARK and "streaming" in serve.STREAM_WATERMARK and "join=False" in infer.WHOLE_WAVE_WATERMARK
    check = serve.check_request_options
    assert check(dict(watermark=77)) == dict(watermark=77) and check(dict(watermark=None)) == {}
    for bad in (True, 1.5, "7", 0, 2 ** 48):
        with pytest.raises(ValueError, match="watermark must be an integer key"):
            check(dict(watermark=bad))
    with pytest.raises(ValueError, match="unknown option 'watermark'"):
        check(dict(watermark=1), allowed=serve.EDIT_OPTIONS)


def test_finish_pcm16_marks_between_prosody_and_loudness():
    x = ref.host(2 * RATE, 4)
    pause = np.concatenate([x, np.zeros(int(2.5 * RATE), dtype=np.int16), x[::-1]])
    for opts in (dict(), dict(tempo=1.25), dict(loudness=-20.0), dict(remove_silence=True, pitch=2, loudness=-23.0, sample_rate=8000, encoding="mulaw"),
                 dict(encoding="flac", flac_level=1)):
        spec = infer.WaveSpec.of(opts)
        pcm = infer.remove_silence_pcm(pause, RATE) if spec.remove_silence else pause
        marked = wave_codec.mark_pcm16(wave_codec.shift_pcm16(pcm, spec.tempo, spec.pitch), 9)
        want = infer.deliver_pcm16(infer.normalise_loudness_pcm16(marked, spec.loudness), *spec.format, flac_level=spec.flac_level if spec.flac else None)
        got = infer.finish_pcm16(pause, dataclasses.replace(spec, watermark=9))
        assert got.dtype == want.dtype and np.array_equal(got, want), opts
        assert np.array_equal(infer.finish_pcm16(pause, dataclasses.replace(spec, watermark=None)), infer.finish_pcm16(pause, spec))   # no key: as before
    # the loudness target and the peak cap are measured on the marked samples
    spec = infer.WaveSpec.of(dict(loudness=-20.0))
    assert not np.array_equal(infer.finish_pcm16(pause, dataclasses.replace(spec, watermark=9)), wave_codec.mark_pcm16(infer.normalise_loudness_pcm16(pause, -20.0), 9))


def test_finish_requests_takes_the_key_per_request():
    fade = infer.cross_fade_duration
    rng = np.random.default_rng(9)
    reqs = [[(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens] for lens in ([20000], [15000, 14000], [9000])]
    texts, flags = ["x"] * 3, [False] * 3
    plain = infer.finish_requests(reqs, texts, fade, flags, want="pcm16")
    got = infer.finish_requests(reqs, texts, fade, flags, watermark=[5, None, 6], loudness=[None, None, -20.0])
    assert got[0].dtype == np.int16 and np.array_equal(got[0], wave_codec.mark_pcm16(plain[0], 5))
    assert got[1].dtype == np.float32 and np.array_equal(got[1], infer.finish_requests(reqs, texts, fade, flags)[1])   # no key: today's bytes
    assert np.array_equal(got[2], infer.normalise_loudness_pcm16(wave_codec.mark_pcm16(plain[2], 6), -20.0))
    one = infer.finish_requests(reqs, texts, fade, flags, watermark=5)                  # one key for all
    assert all(np.array_equal(g, wave_codec.mark_pcm16(x, 5)) for g, x in zip(one, plain))
    waves = infer.SegmentedWaves([reqs[1], reqs[2]], RATE // 2)                        # a script is marked as one joined wave
    joined = infer.quantise_pcm16(infer.join_segments([reqs[1], reqs[2]], fade, RATE // 2))
    assert np.array_equal(infer.finish_requests([waves], ["x"], fade, [False], watermark=7)[0], wave_codec.mark_pcm16(joined, 7))
    with pytest.raises(ValueError, match="watermark must be an integer key"):
        infer.finish_requests(reqs, texts, fade, flags, watermark=1.5)
    with pytest.raises(ValueError) as e:
        infer.finish_requests([reqs[0]], [["head"]], fade, watermark=5)                 # a list of chunk texts
    assert str(e.value) == infer.WHOLE_WAVE_WATERMARK


def test_planner_carries_the_key_and_refuses_chunk_texts_and_join_false(tmp_path):
    voice = infer.PreparedVoice(_voice(tmp_path))
    plan = lambda text, opts: infer.plan_request((voice, "reference words", text, opts), DEFAULTS, target_rms=0.1, fix_duration=None, device=None,   # noqa: E731
                                                 tokenizer=infer.text_to_tokens)
    for text in (["one chunk.", "another chunk."], ("one chunk.",)):
        with pytest.raises(ValueError) as e:
            plan(text, dict(watermark=5))
        assert str(e.value) == infer.WHOLE_WAVE_WATERMARK
    p = plan("some text.", dict(watermark=5))
    assert p.spec.watermark == 5 and p.spec == infer.WaveSpec(watermark=5) and plan("some text.", {}).spec.watermark is None
    assert dataclasses.replace(p.spec, watermark=None) == infer.WaveSpec() == plan("some text.", {}).spec   # the key leaves every other field at its default
    with pytest.raises(ValueError, match="watermark must be an integer key"):
        plan("text.", dict(watermark="5"))
    from test_serve import FakeModel, FakeVocoder
    with pytest.raises(ValueError) as e:
        infer.infer_requests([(voice, "reference words", "some text.", dict(watermark=5))], FakeModel(), FakeVocoder(), nfe_step=4, join=False)
    assert str(e.value) == infer.WHOLE_WAVE_WATERMARK


def test_span_scheduler_carries_the_key():
    import test_spans as spans
    voice = spans._voice()
    text = "This is sentence one, quite long. And here is the second sentence, also long. A third one follows. " * 3
    _, sched = spans._scheduler(span_steps=2, nfe_step=4)
    plain, marked = sched.admit(spans._request(voice, text, seed=1)), sched.admit(spans._request(voice, text, seed=1, watermark=17))
    assert plain.spec.watermark is None and marked.spec.watermark == 17
    with pytest.raises(ValueError) as e:
        sched.admit(spans._request(voice, ["One.", "Two."], watermark=17))
    assert str(e.value) == infer.WHOLE_WAVE_WATERMARK
    while sched.busy:
        sched.step()
    assert plain.result.dtype == np.float32 and marked.result.dtype == np.int16
    assert np.array_equal(marked.result, wave_codec.mark_pcm16(infer.quantise_pcm16(plain.result), 17))


def test_manager_and_speech_routes(client, tmp_path):
    c, mgr, reg = client
    voice = reg.get("KAN_F (Happy)")
    plain = mgr.synthesize(TEXT, voice.audio_path, voice.ref_text)
    pcm = infer.quantise_pcm16(plain)
    want = wave_codec.mark_pcm16(pcm, 41)
    got = mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, watermark=41)
    assert got.dtype == np.int16 and np.array_equal(got, want) and not np.array_equal(want, pcm)
    again = mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, watermark=None)
    assert again.dtype == plain.dtype and np.array_equal(again, plain)                  # without the option: byte for byte as before
    raw = open(_voice(tmp_path), "rb").read()
    clip_pcm = infer.quantise_pcm16(mgr.synthesize_clip(TEXT, raw, "reference words"))
    assert np.array_equal(mgr.synthesize_clip(TEXT, raw, "reference words", watermark=41), wave_codec.mark_pcm16(clip_pcm, 41))
    for stream in (mgr.synthesize_stream, lambda *a, **kw: mgr.synthesize_clip_stream(TEXT, raw, "reference words", **kw)):
        with pytest.raises(ValueError) as e:
            stream(TEXT, voice.audio_path, voice.ref_text, watermark=41)
        assert str(e.value) == serve.STREAM_WATERMARK
    body = dict(text=TEXT, watermark=41)
    clone = dict(body, ref_audio=base64.b64encode(raw).decode(), ref_text="reference words")
    before = c.post("/v1/audio/speech", json=dict(text=TEXT)).content
    for route, extra in (("/v1/audio/speech", body), ("/v1/audio/speech/voice", dict(body, ref_audio_name="KAN_F (Happy)")), ("/v1/audio/speech/clone", clone)):
        r = c.post(route, json=dict(extra, response_format="pcm"))
        assert r.status_code == 200 and r.content == (want if "clone" not in route else wave_codec.mark_pcm16(clip_pcm, 41)).tobytes(), route
        r = c.post(route, json=dict(extra, stream=True))
        assert r.status_code == 400 and r.json()["detail"] == serve.STREAM_WATERMARK, route
        for bad in (True, 1.0, "41", 0, 2 ** 48):
            r = c.post(route, json=dict(extra, watermark=bad))
            assert r.status_code == 400 and "watermark must be an integer key" in r.json()["detail"], (route, bad)
    r = c.post("/v1/audio/speech", json=dict(body, sample_rate=8000, encoding="mulaw", loudness=-20.0, response_format="pcm"))
    assert r.status_code == 200 and r.content == infer.deliver_pcm16(infer.normalise_loudness_pcm16(want, -20.0), 8000, "mulaw").tobytes()
    assert c.post("/v1/audio/speech", json=dict(text=TEXT)).content == before           # a request without the option: the same body


def test_manager_default_key(client):
    c, mgr, reg = client
    voice = reg.get("KAN_F (Happy)")
    pcm = infer.quantise_pcm16(mgr.synthesize(TEXT, voice.audio_path, voice.ref_text))
    marked = serve.TTSManager(nfe_step=4, watermark=99).load(mgr.model_obj, mgr.vocoder)
    assert np.array_equal(marked.synthesize(TEXT, voice.audio_path, voice.ref_text), wave_codec.mark_pcm16(pcm, 99))
    assert np.array_equal(marked.synthesize(TEXT, voice.audio_path, voice.ref_text, watermark=5), wave_codec.mark_pcm16(pcm, 5))   # the request's own key wins
    with pytest.raises(ValueError) as e:
        marked.synthesize_stream(TEXT, voice.audio_path, voice.ref_text)
    assert str(e.value) == serve.STREAM_WATERMARK                                       # never an unmarked stream
    for bad in (True, "99", 0):
        with pytest.raises(ValueError, match="watermark must be an integer key"):
            serve.TTSManager(watermark=bad)
    with pytest.raises(ValueError, match="watermark keys"):
        serve.TTSManager(reject_marked=[])


def test_script_route_and_method(script_client):
    c, mgr, path = script_client
    mgr.load(NoiseModel(), Vocoder())
    voices = dict(main=dict(ref_audio_path=path, ref_text=RA), town=dict(ref_audio=_wav(B), ref_text=RB))
    pcm = infer.quantise_pcm16(mgr.synthesize_script(SCRIPT, voices, gap=0.5, seed=4))
    want = wave_codec.mark_pcm16(pcm, 12)
    got = mgr.synthesize_script(SCRIPT, voices, gap=0.5, seed=4, watermark=12)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    with pytest.raises(ValueError) as e:
        mgr.synthesize_script_stream(SCRIPT, voices, watermark=12)
    assert str(e.value) == serve.STREAM_WATERMARK
    town = dict(ref_audio=base64.b64encode(_wav(B)).decode(), ref_text=RB)
    body = dict(text=SCRIPT, voices=dict(main=dict(ref_audio_name="KAN_F (Happy)"), town=town), seed=4, gap=0.5, watermark=12)
    r = c.post("/v1/audio/speech/script", json=dict(body, response_format="pcm"))
    assert r.status_code == 200 and r.content == want.tobytes()
    calls = len(mgr.model_obj.calls)
    r = c.post("/v1/audio/speech/script", json=dict(body, stream=True))
    assert r.status_code == 400 and r.json()["detail"] == serve.STREAM_WATERMARK
    r = c.post("/v1/audio/speech/script", json=dict(body, watermark="12"))
    assert r.status_code == 400 and "watermark must be" in r.json()["detail"]
    assert len(mgr.model_obj.calls) == calls                                            # neither reached the sampler


def test_edit_route_and_method(client, tmp_path, monkeypatch):
    c, mgr, _ = client
    raw = open(_voice(tmp_path), "rb").read()
    edited = (ref.host(30011, 5).astype(np.float32) / 32768.0)
    monkeypatch.setattr(infer, "speech_edit_batch", lambda edits, *a, **kw: [(edited, RATE, None)] * len(edits))
    want = wave_codec.mark_pcm16(infer.quantise_pcm16(edited), 8)                      # the whole returned recording
    plain = mgr.edit(raw, "new words", [[0.2, 0.5]])
    assert plain.dtype == np.float32 and np.array_equal(plain, edited)
    got = mgr.edit(raw, "new words", [[0.2, 0.5]], watermark=8)
    assert got.dtype == np.int16 and np.array_equal(got, want) and _z(got, 8).detected
    got = mgr.edit(raw, "new words", [[0.2, 0.5]], watermark=8, sample_rate=16000, encoding="alaw")
    assert np.array_equal(got, infer.deliver_pcm16(want, 16000, "alaw"))
    body = dict(audio=base64.b64encode(raw).decode(), text="new words", parts_to_edit=[[0.2, 0.5]], watermark=8)
    r = c.post("/v1/audio/edit", json=dict(body, response_format="pcm"))
    assert r.status_code == 200 and r.content == want.tobytes()
    r = c.post("/v1/audio/edit", json=dict(body, watermark=1.5))
    assert r.status_code == 400 and "watermark must be" in r.json()["detail"]


def _wav24(pcm):
    return serve.wav_bytes(pcm, RATE).getvalue()


def test_detect_method_and_route(client):
    c, mgr, _ = client
    y = wave_codec.mark_pcm16(ref.host(2 * RATE, 6), 31)
    scores = mgr.detect_watermark(_wav24(y), [31, 32])
    assert scores == wave_codec.detect_watermark(y.astype(np.float32) / np.float32(32768.0), [31, 32])
    assert [s.detected for s in scores] == [True, False] and scores[0].offset == 0
    flac = infer.encode_flac(y, RATE).tobytes()                                        # a FLAC upload is read like a reference upload
    assert [s.detected for s in mgr.detect_watermark(flac, [31])] == [True]
    stereo16k = infer.resample_pcm16(y, 16000).astype(np.float32) / 32768.0             # stereo at another rate: mono mix, sinc resampling
    got = mgr.detect_watermark((torch.from_numpy(np.stack([stereo16k, stereo16k])), 16000), [31])
    assert got[0].detected and got[0].z >= 10
    with pytest.raises(ValueError, match="needs keys"):
        mgr.detect_watermark(_wav24(y))
    own = serve.TTSManager(watermark=31)
    assert own.detect_watermark(_wav24(y)) == scores[:1]                                # keys=None: the manager's own; no model needed
    body = dict(audio=base64.b64encode(_wav24(y)).decode(), keys=[31, 32])
    r = c.post("/v1/audio/watermark/detect", json=body)
    assert r.status_code == 200
    results = r.json()["results"]
    assert [(d["key"], d["detected"], d["offset"]) for d in results] == [(31, True, 0), (32, False, scores[1].offset)]
    assert results[0]["score"] == pytest.approx(scores[0].z, abs=1e-12) and set(results[0]) == {"key", "detected", "score", "offset"}
    for bad, words in ((dict(body, keys=[]), "watermark keys"), (dict(body, keys=list(range(1, 18))), "watermark keys"), (dict(body, keys=[1.5]), "integer key"),
                       (dict(audio=body["audio"]), "needs keys"), (dict(body, audio="!!"), "base64"), (dict(body, audio=base64.b64encode(b"nonsense").decode()), "Invalid audio")):
        r = c.post("/v1/audio/watermark/detect", json=bad)
        assert r.status_code == 400 and words in r.json()["detail"], (bad.get("keys"), r.json())


def test_reject_marked_uploads(tmp_path):
    from fastapi.testclient import TestClient
    from test_serve import FakeModel, FakeVocoder
    reg = serve.VoiceRegistry()
    reg.add("KAN_F (Happy)", _voice(tmp_path), "reference words")
    clean = ref.host(3 * RATE, 7)
    marked = wave_codec.mark_pcm16(clean, 21)
    for frontend in (True, False):                                                     # deferred voices (host front-end here) and eager ones
        mgr = serve.TTSManager(nfe_step=4, reject_marked=[20, 21], device_frontend=frontend).load(FakeModel(), FakeVocoder())
        c = TestClient(serve.create_app(mgr, reg))
        infer.WATERMARK_COUNTS.clear()
        body = dict(text=TEXT, ref_text="reference words")
        r = c.post("/v1/audio/speech/clone", json=dict(body, ref_audio=base64.b64encode(_wav24(marked)).decode()))
        assert r.status_code == 400 and r.json()["detail"] == serve.MARKED_REFERENCE == "the reference clip carries this service's watermark"
        assert not mgr._clip_cache and infer.WATERMARK_COUNTS["host_clips"] == 1           # refused before it is cached
        r = c.post("/v1/audio/speech/clone", json=dict(body, ref_audio=base64.b64encode(_wav24(marked)).decode(), denoise=True))
        assert r.status_code == 400 and r.json()["detail"] == serve.MARKED_REFERENCE       # checked in front of the denoiser
        r = c.post("/v1/audio/speech/clone", json=dict(body, ref_audio=base64.b64encode(_wav24(clean)).decode()))
        assert r.status_code == 200 and len(mgr._clip_cache) == 1 and infer.WATERMARK_COUNTS["host_clips"] == 3
        r = c.post("/v1/audio/speech/clone", json=dict(body, ref_audio=base64.b64encode(_wav24(clean)).decode()))
        assert r.status_code == 200 and infer.WATERMARK_COUNTS["host_clips"] == 3           # the cached voice is not scored again
        with pytest.raises(ValueError) as e:
            mgr.synthesize_clip(TEXT, _wav24(marked), "reference words")
        assert str(e.value) == serve.MARKED_REFERENCE
        voices = dict(main=dict(ref_audio_path=reg.get("KAN_F (Happy)").audio_path, ref_text="reference words"),
                      town=dict(ref_audio=_wav24(marked), ref_text="second voice says"))
        with pytest.raises(ValueError) as e:
            mgr.synthesize_script("[main] hello there. [town] and hello.", voices)
        assert str(e.value) == serve.MARKED_REFERENCE
    other = serve.TTSManager(nfe_step=4, reject_marked=[20]).load(FakeModel(), FakeVocoder())   # another service's mark is not this one's
    assert len(other.synthesize_clip(TEXT, _wav24(marked), "reference words")) > 0
    infer.WATERMARK_COUNTS.clear()
    off = serve.TTSManager(nfe_step=4).load(FakeModel(), FakeVocoder())                          # default: no call
    assert len(off.synthesize_clip(TEXT, _wav24(marked), "reference words")) > 0 and not infer.WATERMARK_COUNTS
