"""CPU: `loudness` as `{"target": L, "true_peak": C}` on the host: `wave_codec.limit_pcm16` against tests/limit_ref.py, its laws, the accuracy
of the 4x reading and the overshoot against a 16x fp64 meter, the loudness it reaches, the option's normal form and refusals, and its way
through the layers."""
import base64
import math
import os
import re

import limit_ref
import numpy as np
import pytest
from tts_indic_server_f5_amd import infer, serve, wave_codec

from test_loudness_host import RATE, _lufs, _signal, _sine
from test_script_host import RA, RB, SCRIPT, NoiseModel, Vocoder, _wav, B  # noqa: E402
from test_script_host import client as script_client  # noqa: E402,F401
from test_wave_encode_host import TEXT, _voice, client  # noqa: E402,F401

Tag, M, UNITY = wave_codec.LoudnessTag, wave_codec.LIMIT_HOLD, wave_codec.LIMIT_UNITY
# measured below against the 16x meter, rounded up to 0.05 dB: properties of the tap table and of the 10 ms window (DESIGN "True-peak limiter")
UNDER_READ_DB, OVERSHOOT_DB = 0.15, 0.20


def _content(kind, n):
    rng = np.random.default_rng(n)
    x = np.zeros(n, dtype=np.int16)
    if kind == "square":
        x[:] = 32767
        x[1::2] = -32768
    elif kind == "sine":
        x = _sine(n, RATE / 4, -0.5, math.pi / 4)
    elif kind == "click" and n:
        x[[0, n // 2, n - 1]] = (30000, -32768, 32767)
    elif kind == "noise":
        x = np.clip(rng.standard_normal(n) * 9000, -32768, 32767).astype(np.int16)
    return x


@pytest.mark.parametrize("kind,n", [(k, n) for n in (0, 1, 7, M + 1, 2 * M + 1, 1500) for k in ("zeros", "square", "sine", "click", "noise")])
def test_limit_equals_the_restatement_and_keeps_its_laws(kind, n):
    x = _content(kind, n)
    for G, c in ((UNITY, 29203), (3 * UNITY + 12345, 11626), (UNITY // 3, 32767), (wave_codec.LIMIT_GAIN_MAX, 23197)):
        y, m, a = limit_ref.limit(x.tolist(), G, c)
        assert wave_codec.true_peak_pcm16(x).tolist() == m and wave_codec.limit_envelope(np.asarray(m, np.int64), G, c).tolist() == a
        assert all(mi * G * ai <= c << 46 for mi, ai in zip(m, a))                         # the law, with no tolerance
        assert all(yi == 0 for xi, yi in zip(x.tolist(), y) if xi == 0)
        got = wave_codec.limit_samples(x, G, c)
        assert got.dtype == np.int16 and got.tolist() == y
        assert G != UNITY or c != 29203 or np.array_equal(wave_codec.limit_pcm16(x, Tag(None, -1.0)), got)   # (too short for the meter: unity)


def test_the_tables_equal_their_formulas():
    csrc = os.path.join(os.path.dirname(os.path.abspath(infer.__file__)), "csrc")
    read = lambda name: [int(v) for v in re.findall(r"-?\d+", "".join(l for l in open(os.path.join(csrc, name), encoding="utf-8") if not l.startswith("//")))]  # noqa: E731
    assert read("truepeak_taps.inc") == wave_codec.truepeak_taps().reshape(-1).tolist() == sum(limit_ref.taps(), [])
    assert read("limit_window.inc") == wave_codec.limit_window().tolist() == limit_ref.window()
    core = open(os.path.join(csrc, "wave_limit.h"), encoding="utf-8").read()
    assert f"kLmHold = {M};" in core and f"kLmCeilingMin = {wave_codec.true_peak_ceiling(-9.0)}, kLmCeilingMax = {wave_codec.true_peak_ceiling(0.0)};" in core
    assert wave_codec.true_peak_ceiling(-1.0) == wave_codec.LOUDNESS_PEAK_CEILING


def test_below_the_ceiling_the_limiter_is_the_plain_gain():
    x = _signal("speech -33")[0]
    assert np.array_equal(wave_codec.limit_pcm16(x, {"true_peak": -1.0}), x)               # unity gain, nothing over: byte for byte
    G = wave_codec.limit_gain(*infer.measure_loudness(x)[:2], infer.loudness_gain_constant(-30.0))
    want = np.clip(np.rint(x.astype(np.float64) * G / 65536.0), -32768, 32767).astype(np.int16)
    assert G != UNITY and np.array_equal(wave_codec.limit_pcm16(x, {"target": -30.0, "true_peak": -1.0}), want)
    for number in (-16.0, -30, None):                                                      # a number is the call as it stands
        assert np.array_equal(wave_codec.limit_pcm16(x, number), infer.normalise_loudness_pcm16(x, number))
        assert np.array_equal(infer.finish_pcm16(x, infer.WaveSpec.of(dict(loudness=number))), infer.normalise_loudness_pcm16(x, number))


def _meter16(pcm):
    """The reference meter: dBTP (re 32767) of the largest of 16 points a sample, each an fp64 Kaiser-windowed sinc of 64 taps a side."""
    x, top = pcm.astype(np.float64), float(np.abs(pcm.astype(np.float64)).max())
    for p in range(1, 16):
        d = np.arange(-63, 65) - p / 16.0
        h = np.sinc(d) * np.i0(12.0 * np.sqrt(1.0 - (d / 64.5) ** 2)) / np.i0(12.0)
        top = max(top, float(np.abs(np.convolve(x, h[::-1])).max()))
    return 20.0 * math.log10(top / 32767.0)


def _hosts():
    burst = _sine(3 * RATE, 220, -33.0).astype(np.int32)                                   # a steady host with one plosive 18 dB above its loudness
    amp = 32768.0 * 10.0 ** ((_lufs(burst.astype(np.int16)) + 18.0) / 20.0)
    burst[40000:40120] += np.rint(amp * np.sin(2 * np.pi * 2000 * np.arange(120) / RATE) * np.hanning(120)).astype(np.int32)
    return {"fs/4": _sine(RATE, RATE / 4, -0.5, math.pi / 4), "fs/8": _sine(RATE, RATE / 8, -0.5, math.pi / 8),
            "speech -16": _signal("speech -16")[0], "speech -33": _signal("speech -33")[0], "burst": burst.astype(np.int16)}


def test_reading_overshoot_and_reached_loudness_against_the_16x_meter():
    """Measured on this host function (printed with -s).  The 16x meter minus the 4x reading: fs/4 -0.039 dB, fs/8 -0.022 dB (over-reads), the
    speech-like hosts +0.015 and +0.137 dB, the burst host 0.000 dB: the largest under-read is 0.137 dB, asserted as 0.15.  With the limiter
    acting (the sines at unity gain, the others towards -10 LUFS; -1 and -3 dBTP) the 16x reading of the output stands -0.014, -0.004, +0.245,
    +0.309 and 0.000 dB above C: 0.159 dB beyond the recorded under-read on the noise-like hosts, asserted as an overshoot of 0.20.  The
    reached loudness falls short of -10 LUFS by 3.05 / 4.63 and 2.71 / 4.30 LU on the speech-like hosts (whose crests the limiter holds down
    all the time at that target) and by 0.18 / 0.19 LU on the burst host, and is never above it.  The burst host, 18 dB of crest, asked for
    -16 LUFS: the number reaches -20.33 LUFS, the tag -16.12."""
    hosts, under, over, short = _hosts(), [], [], []
    for name, x in hosts.items():
        under.append(_meter16(x) - wave_codec.true_peak_db(wave_codec.true_peak_pcm16(x)))
        target = None if name.startswith("fs") else -10.0                                  # (a full-scale sine is over the ceiling at unity gain)
        for C in (-1.0, -3.0):
            y = wave_codec.limit_pcm16(x, Tag(target, C))
            G = UNITY if target is None else wave_codec.limit_gain(*infer.measure_loudness(x)[:2], infer.loudness_gain_constant(target))
            assert not np.array_equal(y, np.clip(np.rint(x * (G / 65536.0)), -32768, 32767)), name   # the limiter acts
            over.append(_meter16(y) - C)
            short.append(0.0 if target is None else target - _lufs(y))
        print(name, "under-read %.3f dB, over C %.3f %.3f dB, short %.2f %.2f LU" % (under[-1], *over[-2:], *short[-2:]))
    assert max(under) <= UNDER_READ_DB and max(over) <= UNDER_READ_DB + OVERSHOOT_DB and min(short) >= -0.01
    x = hosts["burst"]                                                                     # the point of the feature
    number, tag = _lufs(infer.normalise_loudness_pcm16(x, -16.0)), _lufs(wave_codec.limit_pcm16(x, {"target": -16.0, "true_peak": -1.0}))
    print("burst: the number reaches %.2f LUFS, the tag %.2f" % (number, tag))
    assert number < -17.0 and tag - number > 1.0 and tag <= -16.0 + 0.01


def test_the_option_normalises_and_refuses():
    of = lambda v, **kw: infer.WaveSpec.of(dict(loudness=v, **kw))   # noqa: E731
    check = lambda v: serve.check_request_options(dict(loudness=v))   # noqa: E731
    assert of({"target": -16}) == of(-16.0) == infer.WaveSpec(loudness=-16.0) and isinstance(of({"target": -16}).loudness, float)
    assert of({"target": -16, "true_peak": -1}).loudness == Tag(-16.0, -1.0) == wave_codec.check_loudness(Tag(-16.0, -1.0))
    assert of({"true_peak": -0.3}).loudness == Tag(None, -0.3) and of({"true_peak": 0, "target": None}).ceiling == 32767 and of(-16.0).ceiling is None
    assert of({"true_peak": -1.0}).gain_constant is None and of({"target": -20, "true_peak": -9.0}).gain_constant == infer.loudness_gain_constant(-20.0)
    assert check({"target": -16.0}) == dict(loudness=-16.0) and check({"true_peak": -2}) == dict(loudness=Tag(None, -2.0))
    assert infer.REQUEST_OPTIONS.count("loudness") == 1 and serve.stream_refusal(dict(loudness={"true_peak": -1.0})) == serve.STREAM_LOUDNESS
    refusals = [({}, "loudness must be a number of LUFS or a mapping with target or true_peak (got {})"),
                ({"true_peak": -1, "lra": 7}, "loudness must be a number of LUFS or {\"target\": L, \"true_peak\": C} (unknown entry 'lra')"),
                ({"true_peak": -1.05}, "loudness must have a true_peak that is a multiple of 0.1 dBTP from -9 to 0 (got -1.05)"),
                ({"true_peak": 0.1}, "loudness must have a true_peak that is a multiple of 0.1 dBTP from -9 to 0 (got 0.1)"),
                ({"target": -16, "true_peak": -9.1}, "loudness must have a true_peak that is a multiple of 0.1 dBTP from -9 to 0 (got -9.1)"),
                ({"true_peak": True}, "loudness must have a true_peak that is a multiple of 0.1 dBTP from -9 to 0 (got True)"),
                ({"target": True, "true_peak": -1}, "loudness must be a number of LUFS (got True)"),
                ({"target": -4, "true_peak": -1}, "loudness must be between -40 and -5 LUFS (got -4.0).")]
    for bad, text in refusals:
        for call in (wave_codec.check_loudness, of, check):
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(e.value) == text
    with pytest.raises(ValueError) as e:                                                   # a list of chunk texts: the loudness message
        infer.finish_requests([[np.zeros(9000, dtype=np.float32)]], [["head"]], loudness={"true_peak": -1.0})
    assert str(e.value) == infer.WHOLE_WAVE_LOUDNESS


def test_finish_requests_compose_in_the_written_order():
    rng = np.random.default_rng(5)
    reqs = [[(amp * rng.standard_normal(n)).astype(np.float32)] for amp, n in ((0.3, 19000), (0.02, 18000), (0.1, 22000))]
    plain = infer.finish_requests(reqs, ["x"] * 3, want="pcm16")
    options = [{"target": -12.0, "true_peak": -2.0}, -23.0, None]
    got = infer.finish_requests(reqs, ["x"] * 3, want="pcm16", watermark=99, loudness=options)
    for g, p, o in zip(got, plain, options):
        assert np.array_equal(g, wave_codec.limit_pcm16(wave_codec.mark_pcm16(p, 99), o))
    assert not np.array_equal(got[0], infer.normalise_loudness_pcm16(wave_codec.mark_pcm16(plain[0], 99), -12.0))
    one = infer.finish_requests(reqs, ["x"] * 3, loudness={"true_peak": -6.0}, sample_rate=8000, encoding="mulaw")   # one mapping for all
    assert all(np.array_equal(g, infer.deliver_pcm16(wave_codec.limit_pcm16(p, Tag(None, -6.0)), 8000, "mulaw")) for g, p in zip(one, plain))


def test_manager_and_routes(client, script_client, tmp_path, monkeypatch):  # noqa: F811
    c, mgr, reg = client
    voice, tag = reg.get("KAN_F (Happy)"), {"target": -14.0, "true_peak": -3.0}
    raw = open(_voice(tmp_path), "rb").read()
    pcm = infer.quantise_pcm16(mgr.synthesize(TEXT, voice.audio_path, voice.ref_text))
    want = wave_codec.limit_pcm16(pcm, tag)
    assert not np.array_equal(want, infer.normalise_loudness_pcm16(pcm, -14.0))            # (the limiter acts on the stand-in's wave)
    assert np.array_equal(mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, loudness=tag), want)
    clip = wave_codec.limit_pcm16(infer.quantise_pcm16(mgr.synthesize_clip(TEXT, raw, "reference words")), tag)
    assert np.array_equal(mgr.synthesize_clip(TEXT, raw, "reference words", loudness=tag), clip)
    with pytest.raises(ValueError) as e:
        mgr.synthesize_stream(TEXT, voice.audio_path, voice.ref_text, loudness=tag)
    assert str(e.value) == serve.STREAM_LOUDNESS
    body = dict(text=TEXT, loudness=tag)
    clone = dict(body, ref_audio=base64.b64encode(raw).decode(), ref_text="reference words")
    for route, extra in (("/v1/audio/speech", body), ("/v1/audio/speech/voice", dict(body, ref_audio_name="KAN_F (Happy)")), ("/v1/audio/speech/clone", clone)):
        r = c.post(route, json=dict(extra, response_format="pcm"))
        assert r.status_code == 200 and r.content == (clip if "clone" in route else want).tobytes(), route
        r = c.post(route, json=dict(extra, stream=True))
        assert r.status_code == 400 and r.json()["detail"] == serve.STREAM_LOUDNESS, route
        r = c.post(route, json=dict(extra, loudness={"true_peak": 1}))
        assert r.status_code == 400 and r.json()["detail"].startswith("loudness must have a true_peak"), route
    edited = (0.4 * np.sin(np.arange(30011) * 0.03)).astype(np.float32)
    monkeypatch.setattr(infer, "speech_edit_batch", lambda edits, *a, **kw: [(edited, RATE, None)] * len(edits))
    want = wave_codec.limit_pcm16(infer.quantise_pcm16(edited), tag)
    assert np.array_equal(mgr.edit(raw, "new words", [[0.2, 0.5]], loudness=tag), want)
    r = c.post("/v1/audio/edit", json=dict(audio=base64.b64encode(raw).decode(), text="new words", parts_to_edit=[[0.2, 0.5]], loudness=tag, response_format="pcm"))
    assert r.status_code == 200 and r.content == want.tobytes()
    c, mgr, path = script_client
    mgr.load(NoiseModel(), Vocoder())
    voices = dict(main=dict(ref_audio_path=path, ref_text=RA), town=dict(ref_audio=_wav(B), ref_text=RB))
    want = wave_codec.limit_pcm16(infer.quantise_pcm16(mgr.synthesize_script(SCRIPT, voices, gap=0.5, seed=4)), tag)
    assert np.array_equal(mgr.synthesize_script(SCRIPT, voices, gap=0.5, seed=4, loudness=tag), want)
    town = dict(ref_audio=base64.b64encode(_wav(B)).decode(), ref_text=RB)
    r = c.post("/v1/audio/speech/script", json=dict(text=SCRIPT, voices=dict(main=dict(ref_audio_name="KAN_F (Happy)"), town=town), seed=4, gap=0.5,
                                                    loudness=tag, response_format="pcm"))
    assert r.status_code == 200 and r.content == want.tobytes()
