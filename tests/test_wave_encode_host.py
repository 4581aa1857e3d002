"""The delivery format on the host (CPU): `infer.resample_pcm16`, `encode_g711` / `decode_g711`, `StreamResampler`, the WAV headers of
`serve.wav_bytes` / `wav_stream_header`, the routes' three fields over a stand-in manager, and `finish_requests` on mixed batches.

Every comparison is `np.array_equal` or equality of bytes, except the cross-check of `resample_pcm16` against the fp32 resampler, whose bound
of one LSB is derived in that test."""
import io
import math
import struct
import wave

import numpy as np
import pytest
import torch

from tts_indic_server_f5_amd import infer, serve

from test_serve import FakeModel, FakeVocoder, _voice

RATE = 24000
RATES = [r for r in infer.OUTPUT_SAMPLE_RATES if r != RATE]
ALL_PCM = np.arange(-32768, 32768).astype(np.int16)


# ------------------------------------------------------------------------------------------------ G.711
def _ilog2(m):
    return m.bit_length() - 1


def _mulaw_closed_form(s):
    """The issue's closed form, one Python int at a time.  Its magnitude clip is 8158 here, not the 8159 the issue's text gives: with 8159 the
    biased magnitude reaches 8192 and the segment 8, which gives 0x7F / 0xFF for the 268 loudest inputs -- against the issue's own known
    answers (32767 -> 0x80, -32768 -> 0x00) and against audioop, which the issue names as the definition (test_encoders_equal_audioop)."""
    x = s >> 2
    sign = 0x7F if x < 0 else 0xFF
    m = min(abs(x), 8158) + 0x21
    seg = _ilog2(m) - 5
    return ((seg << 4) | ((m >> (seg + 1)) & 15)) ^ sign


def _alaw_closed_form(s):
    x = s >> 3
    mask = 0xD5 if x >= 0 else 0x55
    m = x if x >= 0 else -x - 1
    seg = max(_ilog2(max(m, 1)) - 4, 0)
    return ((seg << 4) | ((m >> (1 if seg < 2 else seg)) & 15)) ^ mask


def test_encoders_equal_the_closed_forms_on_every_input():
    for law, form in (("mulaw", _mulaw_closed_form), ("alaw", _alaw_closed_form)):
        got = infer.encode_g711(ALL_PCM, law)
        assert got.dtype == np.uint8
        want = np.array([form(int(s)) for s in ALL_PCM], dtype=np.int64)
        assert want.min() >= 0 and want.max() <= 255 and np.array_equal(got, want), law


def test_known_answers():
    mu = {0: 0xFF, -1: 0x7E, 4: 0xFE, 1000: 0xCE, -1000: 0x4E, 32767: 0x80, -32768: 0x00}
    al = {0: 0xD5, -1: 0x55, 1000: 0xFA, -1000: 0x7A, 32767: 0xAA, -32768: 0x2A}
    for law, table in (("mulaw", mu), ("alaw", al)):
        s = np.array(list(table), dtype=np.int16)
        assert infer.encode_g711(s, law).tolist() == list(table.values()), law


def test_round_trips():
    mu = infer.encode_g711(ALL_PCM, "mulaw")
    assert len(set(mu.tolist())) == 255 and 0x7F not in set(mu.tolist())
    codes = np.arange(256).astype(np.uint8)
    assert np.array_equal(infer.encode_g711(infer.decode_g711(codes, "alaw"), "alaw"), codes)
    back = infer.encode_g711(infer.decode_g711(codes, "mulaw"), "mulaw")          # 0x7F decodes to 0, which encodes as 0xFF
    assert np.array_equal(np.delete(back, 0x7F), np.delete(codes, 0x7F)) and back[0x7F] == 0xFF
    for law in ("mulaw", "alaw"):
        assert infer.decode_g711(codes, law).dtype == np.int16
        with pytest.raises(ValueError):
            infer.encode_g711(ALL_PCM, "mp3")
        with pytest.raises(ValueError):
            infer.encode_g711(ALL_PCM.astype(np.float32), law)


def test_encoders_equal_audioop():
    audioop = pytest.importorskip("audioop")
    raw = ALL_PCM.astype("<i2").tobytes()
    assert infer.encode_g711(ALL_PCM, "mulaw").tobytes() == audioop.lin2ulaw(raw, 2)
    assert infer.encode_g711(ALL_PCM, "alaw").tobytes() == audioop.lin2alaw(raw, 2)
    codes = bytes(range(256))
    assert infer.decode_g711(np.frombuffer(codes, np.uint8), "mulaw").astype("<i2").tobytes() == audioop.ulaw2lin(codes, 2)
    assert infer.decode_g711(np.frombuffer(codes, np.uint8), "alaw").astype("<i2").tobytes() == audioop.alaw2lin(codes, 2)


# ------------------------------------------------------------------------------------------------ resample_pcm16
def _noise(n, seed, amp=0.3):
    return infer.quantise_pcm16(amp * np.random.default_rng(seed).standard_normal(n))


def _square(n):
    return np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)


def test_table_shapes_and_lengths():
    shapes = {8000: (1, 41), 16000: (2, 23), 22050: (147, 174), 32000: (4, 17), 44100: (147, 94), 48000: (2, 15)}
    assert set(shapes) | {RATE} == set(infer.OUTPUT_SAMPLE_RATES)
    for rate, shape in shapes.items():
        of, nf, width, taps = infer.resample_taps(RATE, rate)
        assert tuple(taps.shape) == shape == (nf, 2 * width + of) and taps.dtype == torch.float32
        for n in (0, 1, 2, of - 1, of, of + 1, width, 4801, 30011):
            out = infer.resample_pcm16(_noise(n, n), rate)
            assert out.dtype == np.int16 and len(out) == infer.resampled_length(n, RATE, rate) == math.ceil(n * rate / RATE), (rate, n)
    x = _noise(5000, 1)
    assert infer.resample_pcm16(x, RATE) is x
    for bad in (44101, 11025, True):
        with pytest.raises(ValueError):
            infer.resample_pcm16(x, bad)
    with pytest.raises(ValueError):
        infer.resample_pcm16(x.astype(np.float32), 8000)


@pytest.mark.parametrize("rate", RATES)
def test_within_one_lsb_of_the_fp32_resampler(rate):
    """`resample_sinc_hann` sums the same taps times the same samples in fp32.  Its sum differs from the fp64 one by its own rounding, a small
    fraction of an LSB (0.005 measured for these tables), so after rint the two can disagree only where the exact sum lies next to a tie, and
    then by one."""
    x = _noise(30011, rate)
    ref = np.rint(infer.resample_sinc_hann(torch.from_numpy(x.astype(np.float32))[None], RATE, rate)[0].numpy().astype(np.float64))
    got = infer.resample_pcm16(x, rate).astype(np.float64)
    assert len(got) == len(ref) and np.abs(got - np.clip(ref, -32768, 32767)).max() <= 1


def _exact(x, rate):
    """Every output's sum in fp64 straight from the definition, one dot product per output"""
    of, nf, width, taps = infer.resample_taps(RATE, rate)
    t = taps.numpy().astype(np.float64)
    xpad = np.concatenate([np.zeros(width), x.astype(np.float64), np.zeros(2 * width + 2 * of)])
    m = infer.resampled_length(len(x), RATE, rate)
    return np.array([t[j % nf] @ xpad[(j // nf) * of:(j // nf) * of + t.shape[1]] for j in range(m)])


@pytest.mark.parametrize("rate", RATES)
def test_full_scale_square_waves_clip_without_wraparound(rate):
    """Two full-scale inputs.  The alternating 32767 / -32768 one sits at the band edge, where the filter halves it: it never reaches the rails
    (31 611 at most at these rates), so on its own it cannot show clipping.  The slow square (24 samples up, 24 down) does: its edges
    overshoot full scale on both sides at every rate (Gibbs), and the result must stick to the rails there instead of wrapping."""
    fast = _square(4801)
    slow = np.where(np.arange(4801) // 24 % 2 == 0, 32767, -32768).astype(np.int16)
    for name, x in (("fast", fast), ("slow", slow)):
        exact, got = _exact(x, rate), infer.resample_pcm16(x, rate)
        far = np.abs(exact - np.floor(exact) - 0.5) > 1e-6   # (a dot product adds in another order: compare away from ties)
        assert np.array_equal(got[far], np.clip(np.rint(exact), -32768, 32767).astype(np.int16)[far]), (rate, name)
        over, under = exact > 32767.5, exact < -32768.5
        assert (got[over] == 32767).all() and (got[under] == -32768).all(), (rate, name)
        loud = np.abs(exact) > 1
        assert np.array_equal(np.sign(got[loud].astype(np.int32)), np.sign(exact[loud])), (rate, name)      # no sample changed sides
        if name == "slow":
            assert over.any() and under.any(), rate


# ------------------------------------------------------------------------------------------------ StreamResampler
@pytest.mark.parametrize("rate", infer.OUTPUT_SAMPLE_RATES)
def test_stream_resampler_equals_the_whole(rate):
    of, nf, width, _ = infer.resample_taps(RATE, rate) if rate != RATE else (1, 1, 0, None)
    # 3 of + width + 5: long enough for several blocks to leave from `feed` and for the tail to be cut more than once, short enough to feed
    # the 147-phase tables sample by sample too; 9 700 for the larger pieces (and sample by sample where the table is small)
    for n, sizes in ((1, (1,)), (max(width, 1), (1, 7, of)), (3 * of + width + 5, (1, 7, 240, of, 4801)), (9700, ((1,) if nf < 100 else ()) + (7, 240, of, 4801))):
        x = _noise(n, 7 * n + rate)
        whole = infer.resample_pcm16(x, rate)
        for size in sizes + (n,):
            sr = infer.StreamResampler(rate)
            parts = [sr.feed(x[i:i + size]) for i in range(0, n, size)] + [sr.flush()]
            assert all(p.dtype == np.int16 for p in parts)
            got = np.concatenate(parts)
            assert np.array_equal(got, whole), (rate, n, size)
            assert len(sr.flush()) == 0
    sr = infer.StreamResampler(rate)
    assert len(sr.flush()) == 0                             # nothing fed: nothing comes out


# ------------------------------------------------------------------------------------------------ WAV headers
def _parse_g711(raw):
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE" and raw[12:16] == b"fmt "
    riff, = struct.unpack_from("<I", raw, 4)
    fmt_size, tag, ch, rate, byte_rate, align, bits, cb = struct.unpack_from("<IHHIIHHH", raw, 16)
    assert raw[38:42] == b"fact"
    fact_size, count = struct.unpack_from("<II", raw, 42)
    assert raw[50:54] == b"data"
    data_size, = struct.unpack_from("<I", raw, 54)
    return dict(riff=riff, fmt_size=fmt_size, tag=tag, ch=ch, rate=rate, byte_rate=byte_rate, align=align, bits=bits, cb=cb, fact_size=fact_size,
                count=count, data_size=data_size, body=raw[58:])


def test_g711_wav_headers():
    for law, tag in (("mulaw", 7), ("alaw", 6)):
        for n in (480, 481):
            codes = infer.encode_g711(_noise(n, n), law)
            raw = serve.wav_bytes(codes, 8000, law).getvalue()
            h = _parse_g711(raw)
            assert (h["fmt_size"], h["tag"], h["ch"], h["rate"], h["byte_rate"], h["align"], h["bits"], h["cb"]) == (18, tag, 1, 8000, 8000, 1, 8, 0)
            assert h["fact_size"] == 4 and h["count"] == n and h["data_size"] == n and h["riff"] == len(raw) - 8
            assert h["body"][:n] == codes.tobytes() and len(h["body"]) == n + (n & 1)
            # PCM that is not encoded yet is encoded on the way
            assert serve.wav_bytes(_noise(n, n), 8000, law).getvalue() == raw
        s = _parse_g711(serve.wav_stream_header(8000, law) + b"")
        assert (s["fmt_size"], s["tag"], s["rate"], s["byte_rate"], s["align"], s["bits"], s["cb"]) == (18, tag, 8000, 8000, 1, 8, 0)
        assert s["riff"] == s["count"] == s["data_size"] == 0xFFFFFFFF and len(serve.wav_stream_header(8000, law)) == 58


def test_pcm16_wav_bytes_are_what_they_were():
    x = _noise(1001, 3)
    buf = io.BytesIO()
    with wave.open(buf, "wb") as f:                         # what wav_bytes wrote before it learnt the rate and the encoding
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(24000)
        f.writeframes(x.astype("<i2").tobytes())
    assert serve.wav_bytes(x).getvalue() == buf.getvalue() == serve.wav_bytes(x, 24000, "pcm16").getvalue()
    assert serve.wav_bytes(x.astype(np.float32) / 32768.0).getvalue() == buf.getvalue()
    assert serve.wav_stream_header() == serve.wav_stream_header(24000, "pcm16") and len(serve.wav_stream_header()) == 44
    with wave.open(serve.wav_bytes(infer.resample_pcm16(x, 44100), 44100), "rb") as f:
        assert f.getframerate() == 44100 and f.getsampwidth() == 2 and f.getnframes() == infer.resampled_length(1001, RATE, 44100)
    assert struct.unpack_from("<IHHIIHH", serve.wav_stream_header(16000), 16) == (16, 1, 1, 16000, 32000, 2, 16)


# ------------------------------------------------------------------------------------------------ options and routes
def test_request_options():
    assert {"sample_rate", "encoding"} <= set(infer.REQUEST_OPTIONS) and not {"sample_rate", "encoding"} & set(serve.EDIT_OPTIONS)
    check = serve.check_request_options
    assert check(dict(sample_rate=8000, encoding="mulaw")) == dict(sample_rate=8000, encoding="mulaw")
    assert check(dict(sample_rate=24000, encoding="pcm16")) == {} == check(dict(sample_rate=None, encoding=None))
    for bad in (44101, True, 8000.0, "8000"):
        with pytest.raises(ValueError, match="8000, 16000, 22050, 24000, 32000, 44100, 48000"):
            check(dict(sample_rate=bad))
    for bad in ("mp3", True, 1):
        with pytest.raises(ValueError, match="'pcm16', 'mulaw', 'alaw'"):
            check(dict(encoding=bad))


@pytest.fixture()
def client(tmp_path):
    from fastapi.testclient import TestClient
    reg = serve.VoiceRegistry()
    reg.add("KAN_F (Happy)", _voice(tmp_path), "reference words")
    mgr = serve.TTSManager(nfe_step=4).load(FakeModel(), FakeVocoder())
    return TestClient(serve.create_app(mgr, reg)), mgr, reg


TEXT = "hello world, this is a test. And one more sentence, to have a second chunk; and a third one, why not."


def test_routes_refuse_bad_formats(client):
    c, _, _ = client
    for body, word in ((dict(sample_rate=44101), "sample_rate must be one of"), (dict(encoding="mp3"), "encoding must be one of"),
                       (dict(sample_rate=True), "sample_rate must be one of"), (dict(response_format="flac"), "response_format must be one of")):
        for route, extra in (("/v1/audio/speech", {}), ("/v1/audio/speech/voice", dict(ref_audio_name="KAN_F (Happy)")),
                             ("/v1/audio/speech", dict(stream=True))):
            r = c.post(route, json=dict(text="hello", **extra, **body))
            assert r.status_code == 400 and word in r.json()["detail"], (route, body, r.status_code, r.text)


@pytest.mark.parametrize("rate,enc,fmt", [(8000, "mulaw", "wav"), (16000, "pcm16", "pcm"), (48000, "alaw", "wav")])
def test_route_bodies_equal_the_host_pipeline(client, rate, enc, fmt):
    c, mgr, reg = client
    voice = reg.get("KAN_F (Happy)")
    wave24 = mgr.synthesize(TEXT, voice.audio_path, voice.ref_text)                       # today's result: float32 at 24 kHz
    assert wave24.dtype == np.float32
    samples = infer.deliver_pcm16(infer.quantise_pcm16(wave24), rate, enc)
    payload = samples.astype("<i2").tobytes() if enc == "pcm16" else samples.tobytes()
    want = payload if fmt == "pcm" else serve.wav_bytes(samples, rate, enc).getvalue()
    body = dict(text=TEXT, sample_rate=rate, encoding=enc, response_format=fmt)
    r = c.post("/v1/audio/speech", json=body)
    assert r.status_code == 200 and r.headers["content-type"] == ("audio/pcm" if fmt == "pcm" else "audio/wav")
    assert r.content == want
    r = c.post("/v1/audio/speech/voice", json=dict(body, ref_audio_name="KAN_F (Happy)"))
    assert r.status_code == 200 and r.content == want
    # streamed: the same samples behind the streaming header (or behind nothing, with "pcm")
    s = c.post("/v1/audio/speech", json=dict(body, stream=True))
    header = b"" if fmt == "pcm" else serve.wav_stream_header(rate, enc)
    assert s.status_code == 200 and s.content[:len(header)] == header and s.content[len(header):] == payload
    # the manager's own stream gives the pieces in the delivery format
    pieces = list(mgr.synthesize_stream(TEXT, voice.audio_path, voice.ref_text, sample_rate=rate, encoding=enc))
    assert len(pieces) > 1 and all(p.dtype == samples.dtype for p in pieces) and np.array_equal(np.concatenate(pieces), samples)


def test_clone_route_and_clip_methods_carry_the_format(client, tmp_path):
    import base64
    c, mgr, _ = client
    raw = open(_voice(tmp_path), "rb").read()
    wave24 = mgr.synthesize_clip(TEXT, raw, "reference words")
    assert wave24.dtype == np.float32
    samples = infer.deliver_pcm16(infer.quantise_pcm16(wave24), 8000, "mulaw")
    assert np.array_equal(mgr.synthesize_clip(TEXT, raw, "reference words", sample_rate=8000, encoding="mulaw"), samples)
    pieces = list(mgr.synthesize_clip_stream(TEXT, raw, "reference words", sample_rate=8000, encoding="mulaw"))
    assert len(pieces) > 1 and all(p.dtype == np.uint8 for p in pieces) and np.array_equal(np.concatenate(pieces), samples)
    body = dict(text=TEXT, ref_audio=base64.b64encode(raw).decode(), ref_text="reference words", sample_rate=8000, encoding="mulaw")
    r = c.post("/v1/audio/speech/clone", json=body)
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and r.content == serve.wav_bytes(samples, 8000, "mulaw").getvalue()
    assert "synthesized_speech.wav" in r.headers["content-disposition"]
    r = c.post("/v1/audio/speech/clone", json=dict(body, response_format="pcm"))
    assert r.status_code == 200 and r.headers["content-type"] == "audio/pcm" and r.content == samples.tobytes()
    assert "synthesized_speech.pcm" in r.headers["content-disposition"]
    r = c.post("/v1/audio/speech/clone", json=dict(body, stream=True))
    assert r.status_code == 200 and r.content == serve.wav_stream_header(8000, "mulaw") + samples.tobytes()
    for bad, word in ((dict(sample_rate=44101), "sample_rate must be one of"), (dict(encoding="mp3"), "encoding must be one of"),
                      (dict(response_format="mp3"), "response_format must be one of")):
        r = c.post("/v1/audio/speech/clone", json=dict(body, **bad))
        assert r.status_code == 400 and word in r.json()["detail"], bad


def test_edit_route_and_method_carry_the_format(client, tmp_path, monkeypatch):
    """`TTSManager.edit` itself (the sampler call behind it replaced by a known wave): the host functions on its int16 PCM."""
    import base64
    c, mgr, _ = client
    raw = open(_voice(tmp_path), "rb").read()
    edited = (0.4 * np.sin(np.arange(30011) * 0.03)).astype(np.float32)
    monkeypatch.setattr(infer, "speech_edit_batch", lambda edits, *a, **kw: [(edited, RATE, None)] * len(edits))
    plain = mgr.edit(raw, "new words", [[0.2, 0.5]])
    assert plain.dtype == np.float32 and np.array_equal(plain, edited)
    assert np.array_equal(mgr.edit(raw, "new words", [[0.2, 0.5]], sample_rate=24000, encoding="pcm16"), edited)
    samples = infer.deliver_pcm16(infer.quantise_pcm16(edited), 16000, "alaw")
    got = mgr.edit(raw, "new words", [[0.2, 0.5]], sample_rate=16000, encoding="alaw")
    assert got.dtype == np.uint8 and np.array_equal(got, samples)
    body = dict(audio=base64.b64encode(raw).decode(), text="new words", parts_to_edit=[[0.2, 0.5]])
    r = c.post("/v1/audio/edit", json=body)
    assert r.status_code == 200 and r.content == serve.wav_bytes(edited).getvalue() and "edited_speech.wav" in r.headers["content-disposition"]
    r = c.post("/v1/audio/edit", json=dict(body, sample_rate=16000, encoding="alaw"))
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and r.content == serve.wav_bytes(samples, 16000, "alaw").getvalue()
    pcm44 = infer.resample_pcm16(infer.quantise_pcm16(edited), 44100)
    r = c.post("/v1/audio/edit", json=dict(body, sample_rate=44100, response_format="pcm"))
    assert r.status_code == 200 and r.headers["content-type"] == "audio/pcm" and r.content == pcm44.astype("<i2").tobytes()
    assert "edited_speech.pcm" in r.headers["content-disposition"]
    for bad, word in ((dict(sample_rate=True), "sample_rate must be one of"), (dict(encoding="mp3"), "encoding must be one of")):
        r = c.post("/v1/audio/edit", json=dict(body, **bad))
        assert r.status_code == 400 and word in r.json()["detail"], bad


def test_default_route_body_is_unchanged(client):
    c, mgr, reg = client
    voice = reg.get("KAN_F (Happy)")
    want = serve.wav_bytes(mgr.synthesize(TEXT, voice.audio_path, voice.ref_text)).getvalue()
    for body in (dict(), dict(sample_rate=24000, encoding="pcm16", response_format="wav")):
        r = c.post("/v1/audio/speech", json=dict(text=TEXT, **body))
        assert r.status_code == 200 and r.content == want and r.headers["content-type"] == "audio/wav"


# ------------------------------------------------------------------------------------------------ finish_requests
def test_finish_requests_mixed_batches():
    fade = infer.cross_fade_duration
    rng = np.random.default_rng(11)
    reqs = [[(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lens] for lens in ([9000], [8000, 7300], [12000], [7200, 9001, 7777], [5000])]
    texts = ["x"] * len(reqs)
    flags = [False, True, False, False, True]
    plain_float = infer.finish_requests(reqs, texts, fade, flags)
    plain_pcm = infer.finish_requests(reqs, texts, fade, flags, want="pcm16")
    rates, encs = [None, 8000, 24000, 44100, 16000], [None, "mulaw", "pcm16", None, "alaw"]
    for want, plain in (("float", plain_float), ("pcm16", plain_pcm)):
        got = infer.finish_requests(reqs, texts, fade, flags, want=want, sample_rate=rates, encoding=encs)
        for i in (0, 2):                                    # set nothing, or name the defaults: exactly what they get today
            assert got[i].dtype == plain[i].dtype and np.array_equal(got[i], plain[i]), (want, i)
        for i in (1, 3, 4):
            w = infer.deliver_pcm16(plain_pcm[i], rates[i], encs[i])
            assert got[i].dtype == w.dtype == (np.int16 if encs[i] in (None, "pcm16") else np.uint8) and np.array_equal(got[i], w), (want, i)
    one = infer.finish_requests(reqs, texts, fade, flags, want="pcm16", sample_rate=8000, encoding="alaw")     # one value for all
    for g, p in zip(one, plain_pcm):
        assert np.array_equal(g, infer.encode_g711(infer.resample_pcm16(p, 8000), "alaw"))
    with pytest.raises(ValueError):
        infer.finish_requests(reqs, texts, fade, flags, sample_rate=[8000, 8000])
    with pytest.raises(ValueError):
        infer.finish_requests(reqs, texts, fade, flags, sample_rate=12345)
    with pytest.raises(ValueError):
        infer.finish_requests([reqs[0]], [["head"]], fade, sample_rate=8000)
