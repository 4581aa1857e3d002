"""CPU: FLAC level 1 on the host (`wave_codec.encode_flac(pcm, rate, level=1)`, the definition the device encoder is held to): level 0
unchanged, the round trip through the full reader `read_flac`, every frame's size against a brute-force minimum written a second time
from the rule (flac_lpc_ref.py: Python ints and floats), never larger than level 0, LPC where the fixed predictors cannot follow, the
streaming form, STREAMINFO, the guard, the option's refusals, and every route's body."""
import base64

import numpy as np
import pytest

import flac_lpc_ref as R
from tts_indic_server_f5_amd import infer, serve, wave_codec as W

from test_wave_encode_host import TEXT, client  # noqa: F401  (the stand-in manager behind a TestClient)
from test_serve import _voice

RATES = infer.OUTPUT_SAMPLE_RATES


@pytest.fixture(scope="module")
def signals():
    return R.signals()


@pytest.fixture(scope="module")
def streams(signals):
    """{(name, length): (level-0 stream, level-1 stream)} at 24 kHz, encoded once for the tests below."""
    return {(name, n): (W.encode_flac(x[:n], 24000, 0), W.encode_flac(x[:n], 24000, 1)) for name, x in signals.items() for n in R.LENGTHS}


def test_level_zero_is_todays_stream(signals, streams):
    for (name, n), (s0, _) in streams.items():
        assert np.array_equal(s0, W.encode_flac(signals[name][:n], 24000)), (name, n)
    x = signals["resonance"]
    for rate in RATES:
        assert np.array_equal(W.encode_flac(x, rate, level=0), W.encode_flac(x, rate))


def test_round_trip_through_the_full_reader(signals, streams):
    for (name, n), (_, s1) in streams.items():
        y, rate, bits = W.read_flac(s1.tobytes())
        assert (rate, bits) == (24000, 16) and y.shape == (1, n) and np.array_equal(y[0], signals[name][:n]), (name, n)


@pytest.mark.parametrize("rate", RATES)
def test_round_trip_at_every_rate(signals, rate):
    for name in ("square", "sine041", "resonance", "edges", "noise"):
        x = signals[name][:4097]
        y, r, _ = W.read_flac(W.encode_flac(x, rate, 1).tobytes())
        assert r == rate and np.array_equal(y[0], x), name


def test_every_frame_is_the_brute_force_minimum_and_never_larger(signals, streams):
    chosen = set()
    for (name, n), (s0, s1) in streams.items():
        x = signals[name][:n]
        f0, f1 = R.frames_of(s0), R.frames_of(s1)
        assert len(f0) == len(f1) == -(-n // 4096)
        for f, ((kind0, size0), (kind1, size1)) in enumerate(zip(f0, f1)):
            block = x[4096 * f:4096 * (f + 1)]
            assert size1 == R.frame_bytes(block, f, 1) and kind1 == R.best(block, 1)[1], (name, n, f, kind1, R.best(block, 1))
            assert size0 == R.frame_bytes(block, f, 0) and kind0 == R.best(block, 0)[1], (name, n, f)
            assert size1 <= size0, (name, n, f)
            assert len(block) == 4096 or not kind1.startswith("lpc")                  # the short last block takes the level-0 rule
            chosen.add(kind1)
    assert {"constant", "verbatim"} <= chosen and any(k.startswith("fixed") for k in chosen) and any(k.startswith("lpc") for k in chosen)


def test_lpc_is_chosen_where_it_must_be(streams):
    for name in ("square", "sine041"):
        s0, s1 = streams[(name, 4096)]
        (kind0, size0), = R.frames_of(s0)
        (kind1, size1), = R.frames_of(s1)
        assert kind1.startswith("lpc") and not kind0.startswith("lpc") and size1 < size0 // 3, (name, kind0, size0, kind1, size1)
    assert R.best(R.signals(4096)["square"], 1)[0] == 4399                            # the bits the rule's first prototype gave


@pytest.mark.parametrize("piece", [1, 4095, 4096, 4097, None])
def test_streaming_gives_the_same_frames(signals, piece):
    x = np.concatenate([signals["resonance"], signals["square"][:4096], signals["sine041"][:5000]])
    want = W.encode_flac(x, 16000, 1).tobytes()
    for level in ((1,) if piece == 1 else (0, 1)):
        enc = W.StreamFlacEncoder(16000, level)
        rng, at, out = np.random.default_rng(3), 0, [enc.header()]
        if piece == 1:                                                               # sample by sample over the first block's seam only
            cuts = list(range(1, 4200)) + [len(x)]
        else:
            cuts = []
            while at < len(x):
                at = min(len(x), at + (piece or int(rng.integers(1, 6000))))
                cuts.append(at)
        at = 0
        for c in cuts:
            out.append(enc.feed(x[at:c]))
            at = c
        out.append(enc.flush())
        got = b"".join(out)
        ref = want if level else W.encode_flac(x, 16000).tobytes()
        assert got[:42] == W.flac_stream_header(16000) and got[42:] == ref[42:], (piece, level)
    with pytest.raises(ValueError, match="flac_level"):
        W.StreamFlacEncoder(16000, 2)


def test_streaminfo_names_the_true_frame_sizes(streams):
    for (name, n), (_, s1) in streams.items():
        sizes = [size for _, size in R.frames_of(s1)] or [0]
        data = s1.tobytes()
        assert data[8:12] == bytes([0x10, 0x00, 0x10, 0x00])
        assert int.from_bytes(data[12:15], "big") == min(sizes) and int.from_bytes(data[15:18], "big") == max(sizes), (name, n)
        assert int.from_bytes(data[18:26], "big") & ((1 << 36) - 1) == n and data[26:42] == bytes(16)
        assert len(data) == 42 + sum(sizes if n else [])


def test_the_guard_drops_an_order():
    """No block was found that reaches the guard through Levinson (smooth and alternating tones with full-scale bursts stayed near 1.3e5
    against 2^21), so the host residual helper is fed hand-made coefficients: q = [2047] * 12 at shift 0 on a loud block."""
    rng = np.random.default_rng(5)
    loud = np.where(rng.random(4096) < 0.5, 32767, -32768).astype(np.int64)
    loud[:64] = 32767
    q = np.full((1, 12), 2047, dtype=np.int64)
    u, inside = W.flac_lpc_residual(loud[None], q, np.array([0]))
    assert not inside[0] and u.max() >= W.FLAC_LPC_GUARD and u.max() == max(R.lpc_u([int(v) for v in loud], [2047] * 12, 0))
    u, inside = W.flac_lpc_residual(loud[None], q, np.array([15]))
    assert inside[0] and u.max() < W.FLAC_LPC_GUARD
    assert 12 * 2048 * 32768 < 2 ** 31                                               # the residual's sum stays inside int32
    # what Levinson does reach on the matrix stays far below the guard
    for name, x in R.signals(4096).items():
        for o, (valid, shift, qq, ok) in R.lpc_orders(x).items():
            assert not valid or ok, (name, o)


def test_the_level_is_zero_or_one_as_an_int():
    assert W.check_flac_level(None) == 0 and W.check_flac_level(0) == 0 and W.check_flac_level(1) == 1 and W.check_flac_level(np.int32(1)) == 1
    for bad in (True, False, 2, -1, "1", 1.0, [1]):
        with pytest.raises(ValueError, match="flac_level must be one of") as e:
            W.check_flac_level(bad)
        assert repr(bad) in str(e.value)
        with pytest.raises(ValueError):
            W.encode_flac(np.zeros(4, dtype=np.int16), 24000, bad)
    pcm = R.signals(5000)["resonance"]
    assert np.array_equal(W.deliver_pcm16(pcm, 8000, "flac", 1), W.encode_flac(W.resample_pcm16(pcm, 8000), 8000, 1))
    assert np.array_equal(W.deliver_pcm16(pcm, 8000, "flac"), W.encode_flac(W.resample_pcm16(pcm, 8000), 8000))
    for enc in ("mulaw", "pcm16", None):
        for level in (0, 1):
            with pytest.raises(ValueError, match="flac_level needs encoding 'flac'"):
                W.deliver_pcm16(pcm, 8000, enc, level)
    assert "flac_level" in infer.REQUEST_OPTIONS and "flac_level" in serve.EDIT_OPTIONS
    assert serve.check_request_options(dict(encoding="flac", flac_level=1)) == dict(encoding="flac", flac_level=1)
    assert serve.check_request_options(dict(encoding="flac", flac_level=0)) == dict(encoding="flac")
    for bad in (True, 2, "1"):
        with pytest.raises(ValueError, match="flac_level must be one of"):
            serve.check_request_options(dict(encoding="flac", flac_level=bad))
    for other in (dict(encoding="mulaw"), dict(encoding="pcm16"), {}):
        with pytest.raises(ValueError, match="flac_level needs encoding 'flac'"):
            serve.check_request_options(dict(other, flac_level=1))


def test_finish_requests_on_the_host_with_levels():
    fade = infer.cross_fade_duration
    rng = np.random.default_rng(11)
    reqs = [[(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lens] for lens in ([9000], [8000, 7300], [12000])]
    pcm = infer.finish_requests(reqs, ["x"] * 3, fade, want="pcm16")
    got = infer.finish_requests(reqs, ["x"] * 3, fade, want="pcm16", sample_rate=[None, 8000, 44100], encoding=["flac", "flac", "mulaw"],
                                flac_level=[1, 0, None])
    assert np.array_equal(got[0], infer.encode_flac(pcm[0], 24000, 1)) and np.array_equal(got[1], infer.deliver_pcm16(pcm[1], 8000, "flac"))
    assert np.array_equal(got[2], infer.deliver_pcm16(pcm[2], 44100, "mulaw"))
    with pytest.raises(ValueError, match="flac_level needs encoding 'flac'"):
        infer.finish_requests(reqs, ["x"] * 3, fade, want="pcm16", encoding=["flac", "flac", "mulaw"], flac_level=1)
    with pytest.raises(ValueError, match="flac_level must be one of"):
        infer.finish_requests(reqs[:1], ["x"], fade, want="pcm16", encoding="flac", flac_level=2)


# ------------------------------------------------------------------------------------------------ routes
def _flac_of(wave24, rate, level=1):
    return infer.encode_flac(infer.deliver_pcm16(infer.quantise_pcm16(wave24), rate, "pcm16"), rate, level=level)


def test_speech_routes_answer_level_one(client):  # noqa: F811
    c, mgr, reg = client
    voice = reg.get("KAN_F (Happy)")
    wave24 = mgr.synthesize(TEXT, voice.audio_path, voice.ref_text)
    for rate in (None, 8000):
        want = _flac_of(wave24, rate or 24000)
        assert len(want) <= len(_flac_of(wave24, rate or 24000, 0))
        body = dict(text=TEXT, encoding="flac", flac_level=1, **(dict(sample_rate=rate) if rate else {}))
        got = mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, encoding="flac", sample_rate=rate, flac_level=1)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        for route, extra in (("/v1/audio/speech", {}), ("/v1/audio/speech/voice", dict(ref_audio_name="KAN_F (Happy)"))):
            r = c.post(route, json=dict(body, **extra))
            assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content == want.tobytes(), route
            zero = c.post(route, json=dict(body, flac_level=0, **extra))
            assert zero.status_code == 200 and zero.content == _flac_of(wave24, rate or 24000, 0).tobytes()
        s = c.post("/v1/audio/speech", json=dict(body, stream=True))
        assert s.status_code == 200 and s.content[:42] == infer.StreamFlacEncoder(rate or 24000, 1).header() and s.content[42:] == want.tobytes()[42:]
        pieces = list(mgr.synthesize_stream(TEXT, voice.audio_path, voice.ref_text, encoding="flac", sample_rate=rate, flac_level=1))
        assert np.concatenate(pieces).tobytes() == s.content
        y, r, _ = W.read_flac(s.content)
        assert r == (rate or 24000) and np.array_equal(y[0], W.read_flac(want.tobytes())[0][0])


def test_every_route_refuses_a_bad_level(client, tmp_path):  # noqa: F811
    c, mgr, reg = client
    voice = reg.get("KAN_F (Happy)")
    b64 = base64.b64encode(open(_voice(tmp_path), "rb").read()).decode()
    routes = (("/v1/audio/speech", dict(text=TEXT)),
              ("/v1/audio/speech", dict(text=TEXT, stream=True)),
              ("/v1/audio/speech/voice", dict(text=TEXT, ref_audio_name="KAN_F (Happy)")),
              ("/v1/audio/speech/clone", dict(text=TEXT, ref_audio=b64, ref_text="reference words")),
              ("/v1/audio/speech/script", dict(text="[main] " + TEXT, voices=dict(main=dict(ref_audio=b64, ref_text="reference words")))),
              ("/v1/audio/edit", dict(audio=b64, text="new words", parts_to_edit=[[0.2, 0.5]])))
    for route, body in routes:
        for bad in (True, 2, "1"):
            r = c.post(route, json=dict(body, encoding="flac", flac_level=bad))
            assert r.status_code == 400 and "flac_level must be one of" in r.json()["detail"], (route, bad, r.text)
        for other in (dict(encoding="mulaw"), {}):
            r = c.post(route, json=dict(body, flac_level=1, **other))
            assert r.status_code == 400 and "flac_level needs encoding 'flac'" in r.json()["detail"], (route, other, r.text)
    for bad, message in ((True, "must be one of"), (2, "must be one of"), ("1", "must be one of")):
        with pytest.raises(ValueError, match=message):
            mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, encoding="flac", flac_level=bad)
    with pytest.raises(ValueError, match="needs encoding 'flac'"):
        mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, encoding="mulaw", flac_level=1)
    with pytest.raises(ValueError, match="needs encoding 'flac'"):
        next(mgr.synthesize_stream(TEXT, voice.audio_path, voice.ref_text, flac_level=1))
    with pytest.raises(ValueError, match="needs encoding 'flac'"):
        infer.plan_request((None, "", "x", dict(flac_level=1, encoding="alaw")), {}, target_rms=0.1, fix_duration=None, device=None, tokenizer=None)


def test_clone_script_and_edit_routes_answer_level_one(client, tmp_path, monkeypatch):  # noqa: F811
    c, mgr, _ = client
    raw = open(_voice(tmp_path), "rb").read()
    b64 = base64.b64encode(raw).decode()
    # clone
    want = _flac_of(mgr.synthesize_clip(TEXT, raw, "reference words"), 16000)
    assert np.array_equal(mgr.synthesize_clip(TEXT, raw, "reference words", sample_rate=16000, encoding="flac", flac_level=1), want)
    body = dict(text=TEXT, ref_audio=b64, ref_text="reference words", sample_rate=16000, encoding="flac", flac_level=1)
    r = c.post("/v1/audio/speech/clone", json=body)
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content == want.tobytes()
    s = c.post("/v1/audio/speech/clone", json=dict(body, stream=True))
    assert s.status_code == 200 and s.content[42:] == want.tobytes()[42:]
    pieces = list(mgr.synthesize_clip_stream(TEXT, raw, "reference words", sample_rate=16000, encoding="flac", flac_level=1))
    assert np.concatenate(pieces).tobytes() == s.content
    # script, with a gap and silence removal
    voices = dict(main=dict(ref_audio=raw, ref_text="reference words"))
    text = "[main] hello world, this is a test. [main] And one more sentence."
    pcm = mgr.synthesize_script(text, voices, gap=1.5, remove_silence=True)
    got = mgr.synthesize_script(text, voices, gap=1.5, remove_silence=True, encoding="flac", flac_level=1)
    assert np.array_equal(got, infer.encode_flac(pcm, 24000, 1))
    body = dict(text=text, voices=dict(main=dict(ref_audio=b64, ref_text="reference words")), gap=1.5, encoding="flac", flac_level=1)
    r = c.post("/v1/audio/speech/script", json=dict(body, remove_silence=True))
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content == got.tobytes()
    whole = c.post("/v1/audio/speech/script", json=body)
    s = c.post("/v1/audio/speech/script", json=dict(body, stream=True))
    assert whole.status_code == s.status_code == 200 and s.content[42:] == whole.content[42:]
    assert whole.content == infer.encode_flac(infer.quantise_pcm16(mgr.synthesize_script(text, voices, gap=1.5)), 24000, 1).tobytes()
    assert np.concatenate(list(mgr.synthesize_script_stream(text, voices, gap=1.5, encoding="flac", flac_level=1))).tobytes() == s.content
    # edit
    edited = (0.4 * np.sin(np.arange(30011) * 0.03)).astype(np.float32)
    monkeypatch.setattr(infer, "speech_edit_batch", lambda edits, *a, **kw: [(edited, 24000, None)] * len(edits))
    want = _flac_of(edited, 44100)
    assert np.array_equal(mgr.edit(raw, "new words", [[0.2, 0.5]], sample_rate=44100, encoding="flac", flac_level=1), want)
    r = c.post("/v1/audio/edit", json=dict(audio=b64, text="new words", parts_to_edit=[[0.2, 0.5]], sample_rate=44100, encoding="flac", flac_level=1))
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content == want.tobytes()
