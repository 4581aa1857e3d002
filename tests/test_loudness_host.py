"""CPU: the loudness target on the host -- the integer BS.1770 meter (`infer.measure_loudness`, `loudness_lufs`) against known answers and
against the float64 meter of tests/loudness_ref.py, gating, `normalise_loudness_pcm16`, the bit budget, the tap table the library builds in,
and the `loudness` option through `check_request_options`, `finish_requests`, the manager and the routes."""
import base64
import os
import re

import numpy as np
import pytest

import loudness_ref as ref
from tts_indic_server_f5_amd import infer, serve

from test_script_host import RA, RB, SCRIPT, NoiseModel, Vocoder, _wav, A, B  # noqa: E402
from test_script_host import client as script_client  # noqa: E402,F401  (a manager without a model behind a TestClient)
from test_wave_encode_host import TEXT, _voice, client  # noqa: E402,F401  (the stand-in manager behind a TestClient)

RATE = 24000
SUB = 2400


def _pcm(x):
    return np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def _sine(n, freq, db, phase=0.0):
    return _pcm(10.0 ** (db / 20.0) * np.sin(2 * np.pi * freq * np.arange(n) / RATE + phase))


def _noise(n, seed, db):
    return _pcm(10.0 ** (db / 20.0) * np.random.default_rng(seed).standard_normal(n))


def _bursts(n, seed, db):
    """Speech-like: noise through a slow syllable envelope with pauses between phrases."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    env = (0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 6))) * (np.sin(2 * np.pi * 0.45 * t + rng.uniform(0, 6)) > -0.5)
    x = np.convolve(rng.standard_normal(n), np.ones(6) / 6.0, mode="same")          # most of the energy below 4 kHz
    return _pcm(10.0 ** (db / 20.0) * 2.5 * env * x)


def _lufs(pcm):
    n2, S2, _ = infer.measure_loudness(pcm)
    return infer.loudness_lufs(n2, S2)


def _ref_lufs(pcm):
    return ref.integrated_loudness(pcm.astype(np.float64) / 32768.0, RATE)


# lengths that are no multiple of a sub-block; levels from about -55 to -10 LUFS
SIGNALS = {
    "tone 997 Hz -10": lambda: _sine(3 * RATE + 17, 997, -7.0),
    "tone 250 Hz -30": lambda: _sine(2 * RATE + 1234, 250, -27.0),
    "tone 3 kHz -50": lambda: _sine(2 * RATE + 999, 3000, -52.0),
    "noise -14": lambda: _noise(3 * RATE + 5, 1, -14.0),
    "noise -40": lambda: _noise(2 * RATE + 2399, 2, -40.0),
    "noise -55": lambda: _noise(2 * RATE + 1, 3, -57.0),
    "speech -16": lambda: _bursts(4 * RATE + 777, 4, -12.0),
    "speech -33": lambda: _bursts(4 * RATE + 1201, 5, -29.0),
    "speech -50": lambda: _bursts(3 * RATE + 31, 6, -46.0),
}
_cache = {}


def _signal(name):
    """(pcm, integer LUFS, float64 LUFS) of a named signal, computed once for the tests that share it."""
    if name not in _cache:
        x = SIGNALS[name]()
        _cache[name] = (x, _lufs(x), _ref_lufs(x))
    return _cache[name]


# ------------------------------------------------------------------------------------------------ the definition
def test_taps_and_constants():
    h = infer.loudness_taps()
    assert h.dtype == np.int64 and len(h) == infer.LOUDNESS_TAPS == 1024 and h is infer.loudness_taps() and not h.flags.writeable
    assert int(np.flatnonzero(h)[-1]) == 915 and int(np.abs(h).sum()) == 212915
    assert infer.LOUDNESS_GATE_ABS == int(np.floor(10.0 ** ((-70 + 0.691) / 10) * 9600 * 2.0 ** 26)) == 75535
    assert infer.LOUDNESS_PEAK_CEILING == int(np.floor(32767 * 10.0 ** (-1 / 20))) == 29203
    # the taps are the impulse response of the float meter's own biquads at 24 kHz, at 2^16
    imp = np.zeros(1024)
    imp[0] = 1.0
    assert np.array_equal(h, np.rint(ref.k_weight(imp, RATE) * 65536.0).astype(np.int64))


def test_the_library_builds_in_the_same_taps():
    path = os.path.join(os.path.dirname(os.path.abspath(infer.__file__)), "csrc", "loudness_taps.inc")
    body = "".join(line for line in open(path, encoding="utf-8") if not line.startswith("//"))
    assert [int(v) for v in re.findall(r"-?\d+", body)] == [int(v) for v in infer.loudness_taps()]
    header = open(os.path.join(os.path.dirname(path), "wave_out.h"), encoding="utf-8").read()
    assert f"kLdGateAbs = {infer.LOUDNESS_GATE_ABS};" in header and f"kLdTapAbsSum = {int(np.abs(infer.loudness_taps()).sum())};" in header
    assert f"kLdPeakCeiling = {infer.LOUDNESS_PEAK_CEILING}.0;" in header


def test_known_answers():
    """EBU Tech 3341's meter tolerance, 0.1 LU: a full-scale 997 Hz sine reads -3.01 LUFS (the 24 kHz design: -2.98); 20 dB down, 20 LU less."""
    full = _lufs(_pcm(np.sin(2 * np.pi * 997 * np.arange(4 * RATE) / RATE) * (32767.0 / 32768.0)))
    low = _lufs(_sine(4 * RATE, 997, -20.0))
    print(f"997 Hz sine: full scale {full:.4f} LUFS, -20 dBFS {low:.4f} LUFS")
    assert abs(full - (-3.01)) <= 0.1
    assert abs((full - low) - 20.0) <= 0.01


def test_integer_meter_equals_the_float_meter():
    worst = 0.0
    assert len(SIGNALS) >= 8
    for name in SIGNALS:
        x, got, want = _signal(name)
        assert len(x) % SUB != 0 and got is not None and want is not None, name
        worst = max(worst, abs(got - want))
        print(f"{name:18s} integer {got:9.4f}  float64 {want:9.4f}  diff {got - want:+.2e}")
    levels = [_signal(name)[2] for name in SIGNALS]
    print(f"largest difference: {worst:.2e} LU over {min(levels):.1f} .. {max(levels):.1f} LUFS")
    assert min(levels) < -50 and max(levels) > -15
    assert worst <= 0.01


# ------------------------------------------------------------------------------------------------ gating
def test_quiet_parts_do_not_count():
    loud, quiet = _noise(2 * RATE, 7, -20.0), _noise(3 * RATE, 8, -46.0)                 # 26 dB apart: the quiet blocks fall to the relative gate
    x = np.concatenate([quiet, loud, quiet[:2 * RATE + 500]])
    got, want = _lufs(x), _ref_lufs(x)
    assert abs(got - want) <= 0.01
    # the blocks that straddle an edge hold one to three loud sub-blocks (-6 to -1.2 LU: above the relative gate), so the reading lies a
    # little under the loud part's own, and nowhere near the quiet part's
    assert 0 < _lufs(loud) - got < 1.0 and got - _lufs(np.concatenate([quiet, quiet])) > 20
    n2, _, _ = infer.measure_loudness(x)
    assert n2 < (len(loud) // SUB) + 4                                                  # only the blocks that touch the loud part


def test_nothing_to_measure_comes_back_unchanged():
    zeros = np.zeros(3 * RATE, dtype=np.int16)
    assert infer.measure_loudness(zeros) == (0, 0, 0) and infer.loudness_lufs(0, 0) is None
    assert infer.normalise_loudness_pcm16(zeros, -16.0) is zeros
    short = _noise(9599, 9, -20.0)
    assert infer.measure_loudness(short)[0] == 0 and infer.normalise_loudness_pcm16(short, -16.0) is short
    one = _noise(9600, 9, -20.0)
    assert infer.measure_loudness(one)[0] == 1 and infer.measure_loudness(_noise(9600 + SUB - 1, 9, -20.0))[0] == 1
    assert infer.measure_loudness(_noise(9600 + SUB, 9, -20.0))[0] == 2
    below = _noise(2 * RATE, 10, -75.0)                                                 # everything under the absolute gate
    assert infer.measure_loudness(below)[0] == 0 and infer.normalise_loudness_pcm16(below, -16.0) is below
    empty = np.zeros(0, dtype=np.int16)
    assert infer.measure_loudness(empty) == (0, 0, 0) and infer.normalise_loudness_pcm16(empty, -16.0) is empty
    assert infer.normalise_loudness_pcm16(one, None) is one
    with pytest.raises(ValueError):
        infer.measure_loudness(one.astype(np.float32))


def test_dc_is_judged_by_its_transient():
    x = np.full(3 * RATE, 8000, dtype=np.int16)                                          # -12 dBFS of DC: the high-pass leaves the step at the start
    n2, S2, peak = infer.measure_loudness(x)
    assert peak == 8000 and 1 <= n2 <= 4                                                # only the blocks over the first sub-block
    got, want = infer.loudness_lufs(n2, S2), _ref_lufs(x)
    assert abs(got - want) <= 0.01 and got < -25
    tail = x.copy()
    tail[:RATE] = 0                                                                     # the same step one second later: the same reading
    assert abs(_lufs(tail) - got) <= 0.01


# ------------------------------------------------------------------------------------------------ normalisation
@pytest.mark.parametrize("target", [-16.0, -23.0, -30.0])
def test_normalised_waves_read_the_target(target):
    """No block of these inputs lies within 3 LU of either gate, before or after the gain: the gated set is the same and the re-measured
    loudness is the target up to the rounding of the samples."""
    for name in ("noise -14", "tone 250 Hz -30", "noise -40"):                          # steady signals at three levels
        x, before, _ = _signal(name)
        blocks = ref.block_loudness(x.astype(np.float64) / 32768.0, RATE)
        rel = before - 10.0
        assert all(abs(b - rel) > 3.0 and abs(b + 70.0) > 3.0 and abs(b + (target - before) + 70.0) > 3.0 for b in blocks if np.isfinite(b)), name
        n2, S2, peak = infer.measure_loudness(x)
        g = infer.loudness_gain(n2, S2, peak, infer.loudness_gain_constant(target))
        y = infer.normalise_loudness_pcm16(x, target)
        assert y.dtype == np.int16 and len(y) == len(x)
        assert np.array_equal(y, np.clip(np.rint(x.astype(np.float64) * g), -32768, 32767).astype(np.int16))
        if g < infer.LOUDNESS_PEAK_CEILING / peak:                                      # the ceiling did not bind
            after = _lufs(y)
            print(f"{name:18s} {before:8.3f} -> {after:9.4f} LUFS (target {target}, g = {g:.5f})")
            assert abs(after - target) <= 0.01, (name, after)
        else:
            assert int(np.abs(y.astype(np.int32)).max()) == infer.LOUDNESS_PEAK_CEILING and _lufs(y) < target, name


def test_the_peak_ceiling_binds():
    x, before, _ = _signal("speech -33")
    n2, S2, peak = infer.measure_loudness(x)
    target = -5.0                                                                       # 28 LU up: the peaks would clip
    assert infer.loudness_gain(n2, S2, peak, infer.loudness_gain_constant(target)) == infer.LOUDNESS_PEAK_CEILING / peak
    y = infer.normalise_loudness_pcm16(x, target)
    assert int(np.abs(y.astype(np.int32)).max()) == infer.LOUDNESS_PEAK_CEILING == 29203
    assert before < _lufs(y) < target


def test_already_at_the_target():
    x, before, _ = _signal("noise -14")
    n2, S2, peak = infer.measure_loudness(x)
    g = infer.loudness_gain(n2, S2, peak, infer.loudness_gain_constant(before))
    assert abs(g - 1.0) <= 1e-3
    y = infer.normalise_loudness_pcm16(x, before)
    assert np.abs(y.astype(np.int32) - x.astype(np.int32)).max() <= 1


# ------------------------------------------------------------------------------------------------ bit budget
def test_bit_budget():
    h = infer.loudness_taps()
    total = int(np.abs(h).sum())
    assert (total * 32768) >> 14 < 2 ** 19 and total * 32768 < 2 ** 53
    assert SUB * ((total * 32768) >> 14) ** 2 < 2 ** 50
    # the worst case: every sample at full scale with the sign of its tap, so that one output collects sum |h| * 32768
    nz = int(np.flatnonzero(h)[-1]) + 1
    x = np.zeros(9600, dtype=np.int16)
    x[:nz] = np.where(h[:nz][::-1] >= 0, 32767, -32768)
    y = np.convolve(x.astype(np.float64), h[:nz].astype(np.float64))[:len(x)]
    exact = sum(int(a) * int(b) for a, b in zip(x[:nz].tolist(), h[:nz][::-1].tolist()))
    assert int(y[nz - 1]) == exact and total * 32767 <= abs(exact) <= total * 32768
    n2, S2, peak = infer.measure_loudness(x)
    assert peak == 32768 and n2 == 1 and 0 < S2 < 2 ** 63
    square = np.where(np.arange(3 * RATE) % 2 == 0, 32767, -32768).astype(np.int16)     # the alternating square: a steady |y| near its bound
    n2, S2, _ = infer.measure_loudness(square)
    assert n2 == 3 * RATE // SUB - 3 and S2 < 2 ** 63 and abs(infer.loudness_lufs(n2, S2) - _ref_lufs(square)) <= 0.01


# ------------------------------------------------------------------------------------------------ the option
def test_option_checks():
    assert "loudness" in infer.REQUEST_OPTIONS and "loudness" not in serve.EDIT_OPTIONS
    check = serve.check_request_options
    assert check(dict(loudness=-16)) == dict(loudness=-16.0) and isinstance(check(dict(loudness=-16))["loudness"], float)
    assert check(dict(loudness=None)) == {} and check(dict(loudness=-40.0)) == dict(loudness=-40.0) and check(dict(loudness=-5)) == dict(loudness=-5.0)
    for bad in (-40.5, -4.9, 0, 3.0, True, False, float("nan"), float("inf"), -float("inf"), "-16", [-16.0]):
        with pytest.raises(ValueError, match="loudness must be"):
            check(dict(loudness=bad))
        with pytest.raises(ValueError, match="loudness must be"):
            infer.check_loudness(bad)
    assert infer.needs_whole_wave(dict(loudness=-16.0)) and infer.needs_whole_wave(dict(loudness=-16.0), streamed=True)
    assert not infer.needs_whole_wave(dict(loudness=None))
    models = serve.request_models()
    for name in ("KannadaSynthesizeRequest", "SynthesizeRequest", "CloneRequest", "ScriptRequest", "EditRequest"):
        assert "loudness" in getattr(models, name).model_fields, name


def test_finish_requests_on_the_host():
    fade = infer.cross_fade_duration
    rng = np.random.default_rng(11)
    reqs = [[(amp * rng.standard_normal(n)).astype(np.float32) for n in lens]
            for amp, lens in ((0.3, [19000]), (0.02, [18000, 17300]), (0.1, [22000]), (0.05, [9000]))]
    texts, flags = ["x"] * 4, [False, False, False, False]
    plain = infer.finish_requests(reqs, texts, fade, flags, want="pcm16")
    targets = [-16.0, -23.0, None, -30.0]
    for want in ("float", "pcm16"):
        got = infer.finish_requests(reqs, texts, fade, flags, want=want, loudness=targets)
        for i, t in enumerate(targets):
            if t is None:                                                               # left alone: exactly what it gets today
                today = infer.finish_requests(reqs[i:i + 1], ["x"], fade, [False], want=want)[0]
                assert got[i].dtype == today.dtype and np.array_equal(got[i], today)
            else:
                assert got[i].dtype == np.int16 and np.array_equal(got[i], infer.normalise_loudness_pcm16(plain[i], t)), (want, i)
    assert abs(_lufs(got[0]) - (-16.0)) <= 0.01 and abs(_lufs(got[1]) - (-23.0)) <= 0.01
    assert np.array_equal(got[3], plain[3])                                             # 9000 samples: no block
    one = infer.finish_requests(reqs, texts, fade, flags, want="pcm16", loudness=-20.0)  # one value for all
    assert all(np.array_equal(g, infer.normalise_loudness_pcm16(p, -20.0)) for g, p in zip(one, plain))
    # before the delivery format, after silence removal
    pause = np.concatenate([reqs[0][0], np.zeros(int(2.5 * RATE), np.float32), reqs[2][0]])
    cut = infer.finish_requests([[pause]], ["x"], fade, [True], want="pcm16")[0]
    assert len(cut) < len(pause)
    got = infer.finish_requests([[pause]], ["x"], fade, [True], sample_rate=8000, encoding="mulaw", loudness=-23.0)[0]
    assert np.array_equal(got, infer.deliver_pcm16(infer.normalise_loudness_pcm16(cut, -23.0), 8000, "mulaw"))
    with pytest.raises(ValueError):
        infer.finish_requests(reqs, texts, fade, flags, loudness=[-16.0, -16.0])
    with pytest.raises(ValueError, match="loudness must be"):
        infer.finish_requests(reqs, texts, fade, flags, loudness=-50.0)
    with pytest.raises(ValueError) as e:
        infer.finish_requests([reqs[0]], [["head"]], fade, loudness=-16.0)               # a list of chunk texts
    assert str(e.value) == infer.WHOLE_WAVE_LOUDNESS


def test_a_script_is_normalised_after_the_join():
    fade = infer.cross_fade_duration
    rng = np.random.default_rng(3)
    loud = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in (15000, 14000)]
    quiet = [(0.03 * rng.standard_normal(16000)).astype(np.float32)]
    gap = RATE // 2
    waves = infer.SegmentedWaves([loud, quiet], gap)
    joined = infer.quantise_pcm16(infer.join_segments([loud, quiet], fade, gap))
    got = infer.finish_requests([waves], ["x"], fade, [False], loudness=-18.0)[0]
    assert got.dtype == np.int16 and np.array_equal(got, infer.normalise_loudness_pcm16(joined, -18.0))
    # one gain for the whole script: the quiet voice stays 20 dB below the loud one
    n2, S2, peak = infer.measure_loudness(joined)
    g = infer.loudness_gain(n2, S2, peak, infer.loudness_gain_constant(-18.0))
    tail = slice(len(joined) - 12000, len(joined))
    assert np.abs(got[tail].astype(np.float64) - joined[tail].astype(np.float64) * g).max() <= 0.5


def test_chunk_texts_and_join_false_are_refused(tmp_path):
    voice = infer.PreparedVoice(_voice(tmp_path))
    for text in (["one chunk.", "another chunk."], ("one chunk.",)):
        with pytest.raises(ValueError) as e:
            infer.plan_request((voice, "reference words", text, dict(loudness=-16.0)), dict(speed=1.0, nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0,
                                                                                            seed=None), target_rms=0.1, fix_duration=None, device=None,
                               tokenizer=infer.text_to_tokens)
        assert str(e.value) == infer.WHOLE_WAVE_LOUDNESS
    with pytest.raises(ValueError, match="loudness must be"):
        infer.plan_request((voice, "reference words", "text.", dict(loudness=True)), dict(speed=1.0, nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0,
                                                                                         seed=None), target_rms=0.1, fix_duration=None, device=None,
                           tokenizer=infer.text_to_tokens)
    assert infer.WHOLE_WAVE_LOUDNESS != infer.WHOLE_WAVE and serve.STREAM_LOUDNESS != serve.STREAM_REMOVE_SILENCE


def test_manager_and_speech_routes(client, tmp_path):
    c, mgr, reg = client
    voice = reg.get("KAN_F (Happy)")
    pcm = infer.quantise_pcm16(mgr.synthesize(TEXT, voice.audio_path, voice.ref_text))
    want = infer.normalise_loudness_pcm16(pcm, -20.0)
    assert infer.measure_loudness(pcm)[0] > 0 and not np.array_equal(want, pcm)          # (the stand-in's wave can be measured)
    got = mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, loudness=-20.0)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    raw = open(_voice(tmp_path), "rb").read()
    clip_pcm = infer.quantise_pcm16(mgr.synthesize_clip(TEXT, raw, "reference words"))
    assert np.array_equal(mgr.synthesize_clip(TEXT, raw, "reference words", loudness=-20), infer.normalise_loudness_pcm16(clip_pcm, -20.0))
    for stream in (mgr.synthesize_stream, lambda *a, **kw: mgr.synthesize_clip_stream(TEXT, raw, "reference words", **kw)):
        with pytest.raises(ValueError) as e:
            stream(TEXT, voice.audio_path, voice.ref_text, loudness=-20.0)
        assert str(e.value) == serve.STREAM_LOUDNESS
    body = dict(text=TEXT, loudness=-20.0)
    clone = dict(body, ref_audio=base64.b64encode(raw).decode(), ref_text="reference words")
    for route, extra in (("/v1/audio/speech", body), ("/v1/audio/speech/voice", dict(body, ref_audio_name="KAN_F (Happy)")), ("/v1/audio/speech/clone", clone)):
        r = c.post(route, json=dict(extra, response_format="pcm"))
        assert r.status_code == 200 and r.content == (want if "clone" not in route else infer.normalise_loudness_pcm16(clip_pcm, -20.0)).tobytes(), route
        r = c.post(route, json=dict(extra, stream=True))
        assert r.status_code == 400 and r.json()["detail"] == serve.STREAM_LOUDNESS, route
        for bad in (-41, -4, True):
            r = c.post(route, json=dict(extra, loudness=bad))
            assert r.status_code in (400, 422) and "loudness" in r.text, (route, bad)
    r = c.post("/v1/audio/speech", json=dict(body, sample_rate=8000, encoding="mulaw", response_format="pcm"))
    assert r.status_code == 200 and r.content == infer.deliver_pcm16(want, 8000, "mulaw").tobytes()
    r = c.post("/v1/audio/speech", json=dict(text=TEXT, stream=True, remove_silence=True, loudness=-20.0))
    assert r.status_code == 400 and r.json()["detail"] == serve.STREAM_REMOVE_SILENCE


def test_script_route_and_method(script_client):
    c, mgr, path = script_client
    mgr.load(NoiseModel(), Vocoder())
    voices = dict(main=dict(ref_audio_path=path, ref_text=RA), town=dict(ref_audio=_wav(B), ref_text=RB))
    pcm = infer.quantise_pcm16(mgr.synthesize_script(SCRIPT, voices, gap=0.5, seed=4))
    want = infer.normalise_loudness_pcm16(pcm, -18.0)
    assert infer.measure_loudness(pcm)[0] > 0 and not np.array_equal(want, pcm)
    got = mgr.synthesize_script(SCRIPT, voices, gap=0.5, seed=4, loudness=-18.0)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    with pytest.raises(ValueError) as e:
        mgr.synthesize_script_stream(SCRIPT, voices, loudness=-18.0)
    assert str(e.value) == serve.STREAM_LOUDNESS
    town = dict(ref_audio=base64.b64encode(_wav(B)).decode(), ref_text=RB)
    body = dict(text=SCRIPT, voices=dict(main=dict(ref_audio_name="KAN_F (Happy)"), town=town), seed=4, gap=0.5, loudness=-18.0)
    r = c.post("/v1/audio/speech/script", json=dict(body, response_format="pcm"))
    assert r.status_code == 200 and r.content == want.tobytes()
    calls = len(mgr.model_obj.calls)
    r = c.post("/v1/audio/speech/script", json=dict(body, stream=True))
    assert r.status_code == 400 and r.json()["detail"] == serve.STREAM_LOUDNESS
    r = c.post("/v1/audio/speech/script", json=dict(body, loudness=-60))
    assert r.status_code == 400 and "loudness must be" in r.json()["detail"]
    assert len(mgr.model_obj.calls) == calls                                            # neither reached the sampler


def test_edit_route_and_method(client, tmp_path, monkeypatch):
    c, mgr, _ = client
    raw = open(_voice(tmp_path), "rb").read()
    edited = (0.4 * np.sin(np.arange(30011) * 0.03)).astype(np.float32)
    monkeypatch.setattr(infer, "speech_edit_batch", lambda edits, *a, **kw: [(edited, RATE, None)] * len(edits))
    want = infer.normalise_loudness_pcm16(infer.quantise_pcm16(edited), -23.0)
    got = mgr.edit(raw, "new words", [[0.2, 0.5]], loudness=-23.0)
    assert got.dtype == np.int16 and np.array_equal(got, want) and abs(_lufs(got) - (-23.0)) <= 0.01
    got = mgr.edit(raw, "new words", [[0.2, 0.5]], loudness=-23.0, sample_rate=16000, encoding="alaw")
    assert np.array_equal(got, infer.deliver_pcm16(want, 16000, "alaw"))
    body = dict(audio=base64.b64encode(raw).decode(), text="new words", parts_to_edit=[[0.2, 0.5]], loudness=-23.0)
    r = c.post("/v1/audio/edit", json=dict(body, response_format="pcm"))
    assert r.status_code == 200 and r.content == want.tobytes()
    r = c.post("/v1/audio/edit", json=dict(body, loudness=-3))
    assert r.status_code == 400 and "loudness must be" in r.json()["detail"]
