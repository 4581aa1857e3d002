"""FLAC delivery on the host (CPU): `infer.encode_flac`, `decode_flac`, `StreamFlacEncoder`, `delivery_format` / `deliver_pcm16` with
encoding "flac", and the routes over the stand-in manager of tests/test_wave_encode_host.py.

The judge is a decoder written in this file: a plain bit reader over the stream's bits that shares no code with `wave_codec` and is anchored
on the CRC vectors and the frame of the format specification's first example file.  Every comparison is equality of samples, bytes or bit
counts.  There is no third-party FLAC decoder to ask, so interoperability rests on the specification (RFC 9639) and these anchors."""
import base64

import numpy as np
import pytest

from tts_indic_server_f5_amd import infer, serve

from test_wave_encode_host import TEXT, client  # noqa: F401  (the stand-in manager behind a TestClient)
from test_serve import _voice

RATE = 24000
RATES = list(infer.OUTPUT_SAMPLE_RATES)
RATE_CODES = {8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10}
LENGTHS = [0, 1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8192, 30011]
BLOCK = 4096


# ------------------------------------------------------------------------------------------------ the independent decoder
def crc(data, poly, bits):
    """Bit-serial CRC, initial value 0, not reflected."""
    c, top, mask = 0, 1 << (bits - 1), (1 << bits) - 1
    for byte in data:
        for i in range(7, -1, -1):
            fed = ((byte >> i) & 1) ^ (1 if c & top else 0)
            c = ((c << 1) & mask) ^ (poly if fed else 0)
    return c


class Bits:
    """The stream as a string of '0' and '1'."""

    def __init__(self, data):
        self.s = "".join(f"{b:08b}" for b in data)
        self.i = 0

    def u(self, n):
        assert self.i + n <= len(self.s), "ran off the stream"
        v = int(self.s[self.i:self.i + n], 2) if n else 0
        self.i += n
        return v

    def s16(self):
        v = self.u(16)
        return v - 65536 if v >= 32768 else v

    def unary(self):
        j = self.s.index("1", self.i)
        n, self.i = j - self.i, j + 1
        return n


PREDICT = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}


def parse(stream):
    """(info, frames) of a stream in the subset: info = the STREAMINFO fields, frames = [dict(number, b, kind, order, ks, porder, samples,
    subframe_bits, size, rate_code)].  Asserts everything the format fixes on the way."""
    data = bytes(stream)
    assert data[:4] == b"fLaC" and data[4] == 0x80 and data[5:8] == b"\x00\x00\x22"
    rd = Bits(data[8:42])
    info = dict(min_block=rd.u(16), max_block=rd.u(16), min_frame=rd.u(24), max_frame=rd.u(24), rate=rd.u(20), channels=rd.u(3) + 1,
                bits=rd.u(5) + 1, total=rd.u(36), md5=rd.u(128))
    frames, pos = [], 42
    while pos < len(data):
        rd = Bits(data[pos:pos + 2 * BLOCK + 64])
        assert rd.u(16) == 0xFFF8
        bs_code, rate_code = rd.u(4), rd.u(4)
        assert rd.u(4) == 0 and rd.u(3) == 4 and rd.u(1) == 0       # mono, 16 bits, reserved
        lead = rd.u(8)
        if lead < 0x80:
            number, nbytes = lead, 1
        else:
            nbytes = 8 - (lead ^ 0xFF).bit_length()
            assert 2 <= nbytes <= 7
            number = lead & (0x7F >> nbytes)
            for _ in range(nbytes - 1):
                cont = rd.u(8)
                assert cont >> 6 == 2
                number = (number << 6) | (cont & 0x3F)
        # the shortest coding of the number
        assert nbytes == (1 if number < 128 else 2 if number < 2048 else 3 if number < 65536 else 4 if number < 1 << 21 else 5)
        if bs_code == 12:
            b = BLOCK
        else:
            assert bs_code == 7
            b = rd.u(16) + 1
            assert b < BLOCK
        hlen = rd.i // 8
        assert rd.u(8) == crc(data[pos:pos + hlen], 0x07, 8), "CRC-8"
        start = rd.i
        assert rd.u(1) == 0
        typ = rd.u(6)
        assert rd.u(1) == 0                                         # no wasted bits
        frame = dict(number=number, b=b, rate_code=rate_code, order=None, ks=None, porder=None)
        if typ == 0:
            frame["kind"], x = "constant", [rd.s16()] * b
        elif typ == 1:
            frame["kind"], x = "verbatim", [rd.s16() for _ in range(b)]
        else:
            assert 8 <= typ <= 12
            o = typ - 8
            assert o < b
            x = [rd.s16() for _ in range(o)]
            assert rd.u(2) == 0                                     # 4-bit Rice parameters
            porder = rd.u(4)
            assert porder == (4 if b == BLOCK else 0)
            ks = []
            for p in range(1 << porder):
                k = rd.u(4)
                assert k <= 14                                      # never the escape code
                ks.append(k)
                for _ in range((b >> porder) - (o if p == 0 else 0)):
                    u = (rd.unary() << k) | rd.u(k)
                    r = u >> 1 if u % 2 == 0 else -((u + 1) >> 1)
                    x.append(r + sum(c * x[-1 - j] for j, c in enumerate(PREDICT[o])))
            frame.update(kind="fixed", order=o, ks=ks, porder=porder)
        frame["subframe_bits"] = rd.i - start
        pad = -rd.i % 8
        assert rd.u(pad) == 0
        end = pos + rd.i // 8
        assert int.from_bytes(data[end:end + 2], "big") == crc(data[pos:end], 0x8005, 16), "CRC-16"
        frame["samples"], frame["size"] = np.array(x, dtype=np.int64), end + 2 - pos
        assert len(x) == b
        frames.append(frame)
        pos = end + 2
    assert pos == len(data)
    return info, frames


def decode(stream):
    info, frames = parse(stream)
    x = np.concatenate([f["samples"] for f in frames]) if frames else np.zeros(0, dtype=np.int64)
    assert x.min(initial=0) >= -32768 and x.max(initial=0) <= 32767
    return x.astype(np.int16), info["rate"]


def brute_force(x):
    """The rule of the format's section 1 on one block, from the samples alone: (kind, order, ks, bits)."""
    b = len(x)
    if (x == x[0]).all():
        return "constant", None, None, 8 + 16
    parts = 16 if b == BLOCK else 1
    best = None
    r = x.astype(np.int64)
    for o in range(min(5, b)):
        if o:
            r = r[1:] - r[:-1]
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        bits, ks = 8 + 16 * o + 2 + 4, []
        for p in range(parts):
            lo, hi = max(p * (b // parts) - o, 0), (p + 1) * (b // parts) - o
            seg = u[lo:hi]
            costs = [int((seg >> k).sum()) + len(seg) * (1 + k) for k in range(15)]
            k = min(range(15), key=lambda k: (costs[k], k))
            ks.append(k)
            bits += 4 + costs[k]
        if best is None or bits < best[3]:
            best = ("fixed", o, ks, bits)
    if 8 + 16 * b < best[3]:
        return "verbatim", None, None, 8 + 16 * b
    return best


def check_stream(x, rate):
    """Everything a stream must satisfy: decodes to x, right header, every frame the brute-force winner.  Returns the frames."""
    stream = infer.encode_flac(x, rate)
    assert stream.dtype == np.uint8 and stream.ndim == 1
    info, frames = parse(stream)
    got = np.concatenate([f["samples"] for f in frames]) if frames else np.zeros(0, dtype=np.int64)
    assert np.array_equal(got, x.astype(np.int64))
    sizes = [f["size"] for f in frames] or [0]
    assert info == dict(min_block=BLOCK, max_block=BLOCK, min_frame=min(sizes), max_frame=max(sizes), rate=rate, channels=1, bits=16,
                        total=len(x), md5=0)
    assert len(stream) == 42 + sum(f["size"] for f in frames)
    assert [f["number"] for f in frames] == list(range(len(frames))) and all(f["rate_code"] == RATE_CODES[rate] for f in frames)
    assert [f["b"] for f in frames] == [BLOCK] * (len(x) // BLOCK) + ([len(x) % BLOCK] if len(x) % BLOCK else [])
    for f in frames:
        kind, order, ks, bits = brute_force(f["samples"])
        assert (f["kind"], f["order"], f["ks"], f["subframe_bits"]) == (kind, order, ks, bits), (f["number"], f["kind"], f["order"], kind, order)
    return frames


# ------------------------------------------------------------------------------------------------ contents
def _noise(n, seed=0, amp=0.3):
    return infer.quantise_pcm16(amp * np.random.default_rng(seed).standard_normal(n))


def _walk(n, seed=1):
    return np.clip(np.cumsum(200.0 * np.random.default_rng(seed).standard_normal(n)), -32768, 32767).astype(np.int16)


def _sine(n, freq, amp, noise=0.0, seed=2):
    x = amp * np.sin(2 * np.pi * freq * np.arange(n) / RATE) * 32768.0
    if noise:
        x = x + noise * np.random.default_rng(seed).standard_normal(n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


CONTENTS = {   # name -> (samples of n, the subframe a full block of it gets, bits per sample of that block)
    "zeros": (lambda n: np.zeros(n, dtype=np.int16), ("constant", None), None),
    "constant": (lambda n: np.full(n, 1234, dtype=np.int16), ("constant", None), None),
    "noise": (lambda n: _noise(n), ("fixed", 0), 15.5),
    "walk": (lambda n: _walk(n), ("fixed", 1), 9.8),
    "low sine": (lambda n: _sine(n, 100, 0.01), ("fixed", 2), 1.95),
    "noisy sine": (lambda n: _sine(n, 1000, 0.3, noise=30.0), ("fixed", 3), 9.7),
    "sine": (lambda n: _sine(n, 300, 0.5), ("fixed", 4), 3.8),
    "square": (lambda n: np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16), ("verbatim", None), 16.0),
}


def test_anchors_of_the_format():
    """The two CRCs on the usual check string, and the single frame of the specification's first example file -- for this file's bit-serial
    CRCs and for the package's table-driven ones."""
    header, frame = bytes.fromhex("fff869180000"), bytes.fromhex("fff869180000bf0358fd03128b")
    for crc8, crc16 in ((lambda d: crc(d, 0x07, 8), lambda d: crc(d, 0x8005, 16)), (infer.flac_crc8, infer.flac_crc16)):
        assert crc8(b"123456789") == 0xF4 and crc16(b"123456789") == 0xFEE8
        assert crc8(header) == 0xBF and crc16(frame) == 0xAA9A


@pytest.mark.parametrize("rate", RATES)
def test_every_length_round_trips_at_every_rate(rate):
    for n in LENGTHS:
        x = _walk(n, seed=n)
        check_stream(x, rate)
        y, r = decode(infer.encode_flac(x, rate))
        assert r == rate and np.array_equal(y, x)
    empty = infer.encode_flac(np.zeros(0, dtype=np.int16), rate)
    assert len(empty) == 42 and parse(empty)[0]["total"] == 0 and parse(empty)[0]["min_frame"] == parse(empty)[0]["max_frame"] == 0


@pytest.mark.parametrize("name", list(CONTENTS))
def test_contents_get_the_subframe_they_should(name):
    make, (kind, order), bps = CONTENTS[name]
    for n in (5, 257, 4095, 4096, 2 * BLOCK + 3):
        frames = check_stream(make(n), RATE)
        if n >= BLOCK:
            first = frames[0]
            assert (first["kind"], first["order"]) == (kind, order), (name, n, first["kind"], first["order"])
            if bps is not None:
                # the figures are a probe's, on other random draws and rounded to two or three digits: 6 % covers the rounding (at most
                # 0.5 % at 9.8) and the spread between draws of 4096 samples, and still tells each content's neighbours apart (the orders
                # next to the expected one cost 10 % or more on these signals); the exact size is held to `brute_force` above
                assert abs(first["subframe_bits"] / BLOCK - bps) < 0.06 * bps, (name, first["subframe_bits"] / BLOCK)
    if name == "square":       # the best fixed order would need 18 bits per sample
        x = make(BLOCK).astype(np.int64)
        r = x[1:] - x[:-1]
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        assert min(int((u >> k).sum()) + len(u) * (1 + k) for k in range(15)) / BLOCK > 16


def test_all_seven_kinds_occur():
    seen = set()
    x = np.concatenate([CONTENTS[name][0](BLOCK) for name in CONTENTS])
    for f in check_stream(x, RATE):
        seen.add((f["kind"], f["order"]))
    assert seen == {("constant", None), ("verbatim", None)} | {("fixed", o) for o in range(5)}


def test_short_blocks_take_orders_below_their_length():
    rng = np.random.default_rng(5)
    for b in range(1, 12):
        for _ in range(20):
            x = (rng.integers(-3, 4, b) * rng.integers(1, 9000)).astype(np.int16)
            for f in check_stream(x, RATE):
                assert f["order"] is None or f["order"] < b


@pytest.mark.parametrize("frames", [127, 128, 129, 2047, 2048, 2049])
def test_frame_number_seams(frames):
    x = np.zeros(frames * BLOCK - 100, dtype=np.int16)
    for f in (0, 126, 127, 128, 2046, 2047, 2048):                  # noise at the seams, silence elsewhere
        if f < frames - 1:
            x[f * BLOCK:(f + 1) * BLOCK] = _noise(BLOCK, seed=f, amp=0.001)
    x[-50:] = 77
    stream = infer.encode_flac(x, RATE)
    info, parsed = parse(stream)
    assert len(parsed) == frames and [f["number"] for f in parsed] == list(range(frames)) and info["total"] == len(x)
    assert np.array_equal(np.concatenate([f["samples"] for f in parsed]), x)
    assert info["min_frame"] == min(f["size"] for f in parsed) and info["max_frame"] == max(f["size"] for f in parsed)
    assert np.array_equal(infer.decode_flac(stream)[0], x)


@pytest.mark.parametrize("piece", [1, 4095, 4096, 4097, None])
def test_stream_encoder_equals_the_whole(piece):
    n = 3 * BLOCK + 1234 if piece != 1 else BLOCK + 7
    x = np.concatenate([_walk(n // 2, seed=3), np.zeros(n - n // 2, dtype=np.int16)])
    whole = infer.encode_flac(x, 44100).tobytes()
    enc = infer.StreamFlacEncoder(44100)
    assert enc.header() == whole[:4] + infer.encode_flac(np.zeros(0, dtype=np.int16), 44100).tobytes()[4:] and len(enc.header()) == 42
    info = parse(enc.header())[0]
    assert (info["total"], info["min_frame"], info["max_frame"], info["rate"]) == (0, 0, 0, 44100)
    rng, pos, out = np.random.default_rng(9), 0, []
    while pos < n:
        step = piece if piece else int(rng.integers(0, 6000))
        out.append(enc.feed(x[pos:pos + step]))
        pos += step
    out.append(enc.flush())
    assert b"".join(out) == whole[42:]
    assert enc.flush() == b""
    y, r = decode(enc.header() + b"".join(out))
    assert r == 44100 and np.array_equal(y, x)


def test_decode_flac_round_trips_and_refuses():
    for name in CONTENTS:
        x = CONTENTS[name][0](BLOCK + 301)
        y, r = infer.decode_flac(infer.encode_flac(x, 16000))
        assert r == 16000 and y.dtype == np.int16 and np.array_equal(y, x)
    y, r = infer.decode_flac(infer.encode_flac(np.zeros(0, dtype=np.int16), 8000).tobytes())
    assert len(y) == 0 and r == 8000
    good = infer.encode_flac(_walk(300), RATE)
    _, (frame,) = parse(good)
    hlen = 4 + 1 + 2                                                # sync and codes, the frame number, b - 1
    for byte in (42 + hlen, len(good) - 1, len(good) - 2):          # a bit of the CRC-8, and of either byte of the CRC-16
        bad = good.copy()
        bad[byte] ^= 0x10
        with pytest.raises(ValueError, match="CRC"):
            infer.decode_flac(bad)
    bad = good.copy()
    bad[42 + hlen + 5] ^= 0x01                                      # a bit of the subframe: the CRC-16 no longer holds
    with pytest.raises(ValueError):
        infer.decode_flac(bad)
    stereo, deep = good.copy(), good.copy()
    stereo[8 + 12] |= 0x02                                          # channels - 1 = 1
    deep[8 + 12] |= 0x01; deep[8 + 13] = (deep[8 + 13] & 0x0F) | 0x70   # bits - 1 = 23
    with pytest.raises(ValueError, match="mono 16-bit"):
        infer.decode_flac(stereo)
    with pytest.raises(ValueError, match="mono 16-bit"):
        infer.decode_flac(deep)
    for junk in (b"", b"RIFF....WAVE", good[:60].tobytes()):
        with pytest.raises(ValueError):
            infer.decode_flac(junk)


def test_decode_flac_reads_what_other_encoders_write():
    """A hand-built stream outside our subset but inside the decoder's: variable block size code, partition order 1, a wasted bit."""
    x = (2 * np.arange(-8, 8)).astype(np.int16)                     # 16 samples, all even: one wasted bit
    half = x.astype(np.int64) >> 1
    bits = "0" + "001001" + "1" + "1"                               # FIXED order 1, wasted-bits flag, unary 1 wasted bit
    bits += f"{half[0] & 0x7FFF:015b}" + "00" + "0001"              # warm-up at 15 bits, method 0, partition order 1
    res = half[1:] - half[:-1]
    for part in (res[:7], res[7:]):
        bits += "0001"                                              # k = 1
        for r in part:
            u = 2 * int(r) if r >= 0 else -2 * int(r) - 1
            bits += "0" * (u >> 1) + "1" + str(u & 1)
    bits += "0" * (-len(bits) % 8)
    head = bytes([0xFF, 0xF8, 0x67, 0x08, 0x00, 15])                # block-size code 0110: an 8-bit b - 1
    head += bytes([crc(head, 0x07, 8)])
    frame = head + int(bits, 2).to_bytes(len(bits) // 8, "big")
    frame += crc(frame, 0x8005, 16).to_bytes(2, "big")
    info = (16 << 16 | 16).to_bytes(4, "big") + bytes(6) + ((RATE << 44) | (15 << 36) | 16).to_bytes(8, "big") + bytes(16)
    y, r = infer.decode_flac(b"fLaC" + bytes([0x80, 0, 0, 34]) + info + frame)
    assert r == RATE and np.array_equal(y, x)


# ------------------------------------------------------------------------------------------------ delivery format and options
def test_delivery_format_and_options():
    assert infer.OUTPUT_ENCODINGS == ("pcm16", "mulaw", "alaw") and infer.FLAC_ENCODINGS == ("flac",)
    assert infer.delivery_format(44100, "flac") == (44100, "flac") and infer.delivery_format(None, "flac") == (RATE, "flac")
    assert serve.check_request_options(dict(encoding="flac")) == dict(encoding="flac")
    with pytest.raises(ValueError, match="'pcm16', 'mulaw', 'alaw', 'flac'"):
        infer.delivery_format(None, "mp3")
    with pytest.raises(ValueError, match="sample_rate must be one of"):
        infer.encode_flac(np.zeros(4, dtype=np.int16), 11025)
    pcm = _walk(9000)
    for rate in (8000, RATE, 44100):
        got = infer.deliver_pcm16(pcm, rate, "flac")
        assert got.dtype == np.uint8 and np.array_equal(got, infer.encode_flac(infer.resample_pcm16(pcm, rate), rate))
        y, r = decode(got)
        assert r == rate and np.array_equal(y, infer.resample_pcm16(pcm, rate))
    assert serve.delivery_bytes(got, "flac") == got.tobytes()


def test_finish_requests_on_the_host_with_flac():
    fade = infer.cross_fade_duration
    rng = np.random.default_rng(11)
    reqs = [[(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lens] for lens in ([9000], [8000, 7300], [12000])]
    flags = [False, True, False]
    pcm = infer.finish_requests(reqs, ["x"] * 3, fade, flags, want="pcm16")
    for want in ("float", "pcm16"):
        got = infer.finish_requests(reqs, ["x"] * 3, fade, flags, want=want, sample_rate=[None, 8000, 44100], encoding=["flac", "flac", "mulaw"])
        assert np.array_equal(got[0], infer.encode_flac(pcm[0], RATE)) and np.array_equal(got[1], infer.deliver_pcm16(pcm[1], 8000, "flac"))
        assert np.array_equal(got[2], infer.deliver_pcm16(pcm[2], 44100, "mulaw"))
    with pytest.raises(ValueError):
        infer.finish_requests([reqs[0]], [["head"]], fade, encoding="flac")


# ------------------------------------------------------------------------------------------------ routes
def _flac_of(wave24, rate):
    return infer.encode_flac(infer.deliver_pcm16(infer.quantise_pcm16(wave24), rate, "pcm16"), rate)


@pytest.mark.parametrize("rate", [None, 8000, 44100])
def test_speech_routes_answer_flac(client, rate):  # noqa: F811
    c, mgr, reg = client
    voice = reg.get("KAN_F (Happy)")
    wave24 = mgr.synthesize(TEXT, voice.audio_path, voice.ref_text)
    want = _flac_of(wave24, rate or RATE)
    body = dict(text=TEXT, encoding="flac", **(dict(sample_rate=rate) if rate else {}))
    got = mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, encoding="flac", sample_rate=rate)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    for route, extra in (("/v1/audio/speech", {}), ("/v1/audio/speech/voice", dict(ref_audio_name="KAN_F (Happy)"))):
        r = c.post(route, json=dict(body, **extra))
        assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content == want.tobytes(), route
        assert ".flac" in r.headers["content-disposition"] and ".wav" not in r.headers["content-disposition"]
    samples, _ = decode(want)
    # streamed: the header with the totals unknown, then the same frames
    s = c.post("/v1/audio/speech", json=dict(body, stream=True))
    assert s.status_code == 200 and s.headers["content-type"] == "audio/flac"
    assert s.content[:42] == infer.StreamFlacEncoder(rate or RATE).header() and s.content[42:] == want.tobytes()[42:]
    y, r = infer.decode_flac(s.content)
    assert r == (rate or RATE) and np.array_equal(y, samples)
    pieces = list(mgr.synthesize_stream(TEXT, voice.audio_path, voice.ref_text, encoding="flac", sample_rate=rate))
    assert len(pieces) > 1 and all(p.dtype == np.uint8 for p in pieces) and np.concatenate(pieces).tobytes() == s.content


def test_a_failing_first_chunk_of_a_flac_stream_is_a_status_code(tmp_path):
    """The streaming routes synthesize the first piece before the response exists.  The flac header must not go out ahead of that piece: a
    head request that fails is an error status as with every other encoding, never a 200 whose body is a bare header."""
    from fastapi.testclient import TestClient
    from test_serve import FakeModel, FakeVocoder

    class FailingModel(FakeModel):
        def sample(self, *args, **kw):
            raise RuntimeError("the device is gone")

    reg = serve.VoiceRegistry()
    reg.add("KAN_F (Happy)", _voice(tmp_path), "reference words")
    mgr = serve.TTSManager(nfe_step=4).load(FailingModel(), FakeVocoder())
    voice = reg.get("KAN_F (Happy)")
    for enc in ("flac", "mulaw", None):
        opts = dict(encoding=enc) if enc else {}
        stream = mgr.synthesize_stream(TEXT, voice.audio_path, voice.ref_text, **opts)
        with pytest.raises(RuntimeError, match="the device is gone"):
            next(stream)                                            # the first `next` runs the head request, whatever the encoding
    c = TestClient(serve.create_app(mgr, reg), raise_server_exceptions=False)
    raw = base64.b64encode(open(_voice(tmp_path), "rb").read()).decode()
    bodies = (("/v1/audio/speech", dict(text=TEXT)),
              ("/v1/audio/speech/clone", dict(text=TEXT, ref_audio=raw, ref_text="reference words")),
              ("/v1/audio/speech/script", dict(text="[main] " + TEXT, voices=dict(main=dict(ref_audio=raw, ref_text="reference words")))))
    for route, body in bodies:
        plain = c.post(route, json=dict(body, stream=True))
        flac = c.post(route, json=dict(body, stream=True, encoding="flac"))
        assert plain.status_code >= 500 and flac.status_code == plain.status_code, (route, plain.status_code, flac.status_code)
        assert flac.headers.get("content-type") != "audio/flac" and b"fLaC" not in flac.content, route


def test_flac_is_its_own_container(client):  # noqa: F811
    c, _, _ = client
    for route, extra in (("/v1/audio/speech", {}), ("/v1/audio/speech/voice", dict(ref_audio_name="KAN_F (Happy)")), ("/v1/audio/speech", dict(stream=True))):
        for fmt in ("wav", "pcm"):
            r = c.post(route, json=dict(text="hello", encoding="flac", response_format=fmt, **extra))
            assert r.status_code == 400 and "flac" in r.json()["detail"] and "response_format" in r.json()["detail"], (route, fmt, r.text)
        r = c.post(route, json=dict(text="hello", response_format="flac", **extra))
        assert r.status_code == 400 and "response_format must be one of" in r.json()["detail"]
        r = c.post(route, json=dict(text="hello", encoding="mp3", **extra))
        assert r.status_code == 400 and "'pcm16', 'mulaw', 'alaw', 'flac'" in r.json()["detail"]


def test_clone_script_and_edit_routes_answer_flac(client, tmp_path, monkeypatch):  # noqa: F811
    c, mgr, _ = client
    raw = open(_voice(tmp_path), "rb").read()
    b64 = base64.b64encode(raw).decode()
    # clone
    want = _flac_of(mgr.synthesize_clip(TEXT, raw, "reference words"), 16000)
    assert np.array_equal(mgr.synthesize_clip(TEXT, raw, "reference words", sample_rate=16000, encoding="flac"), want)
    body = dict(text=TEXT, ref_audio=b64, ref_text="reference words", sample_rate=16000, encoding="flac")
    r = c.post("/v1/audio/speech/clone", json=body)
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content == want.tobytes()
    assert "synthesized_speech.flac" in r.headers["content-disposition"]
    s = c.post("/v1/audio/speech/clone", json=dict(body, stream=True))
    assert s.status_code == 200 and s.content[42:] == want.tobytes()[42:] and np.array_equal(decode(s.content)[0], decode(want)[0])
    pieces = list(mgr.synthesize_clip_stream(TEXT, raw, "reference words", sample_rate=16000, encoding="flac"))
    assert np.concatenate(pieces).tobytes() == s.content
    assert c.post("/v1/audio/speech/clone", json=dict(body, response_format="wav")).status_code == 400
    # script, with a gap and silence removal
    voices = dict(main=dict(ref_audio=raw, ref_text="reference words"))
    text = "[main] hello world, this is a test. [main] And one more sentence."
    pcm = mgr.synthesize_script(text, voices, gap=1.5, remove_silence=True)
    assert pcm.dtype == np.int16
    got = mgr.synthesize_script(text, voices, gap=1.5, remove_silence=True, encoding="flac")
    assert np.array_equal(got, infer.encode_flac(pcm, RATE))
    body = dict(text=text, voices=dict(main=dict(ref_audio=b64, ref_text="reference words")), gap=1.5, encoding="flac")
    r = c.post("/v1/audio/speech/script", json=dict(body, remove_silence=True))
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content == got.tobytes()
    assert "synthesized_script.flac" in r.headers["content-disposition"]
    whole = c.post("/v1/audio/speech/script", json=body)
    s = c.post("/v1/audio/speech/script", json=dict(body, stream=True))
    assert whole.status_code == s.status_code == 200 and s.content[42:] == whole.content[42:]
    assert np.array_equal(decode(s.content)[0], decode(whole.content)[0])
    kinds = {f["kind"] for f in parse(whole.content)[1]}
    assert "constant" in kinds                                      # the gap's exact zeros cost 3 bytes a frame
    assert np.concatenate(list(mgr.synthesize_script_stream(text, voices, gap=1.5, encoding="flac"))).tobytes() == s.content
    assert c.post("/v1/audio/speech/script", json=dict(body, response_format="pcm")).status_code == 400
    # edit
    edited = (0.4 * np.sin(np.arange(30011) * 0.03)).astype(np.float32)
    monkeypatch.setattr(infer, "speech_edit_batch", lambda edits, *a, **kw: [(edited, RATE, None)] * len(edits))
    want = _flac_of(edited, 44100)
    assert np.array_equal(mgr.edit(raw, "new words", [[0.2, 0.5]], sample_rate=44100, encoding="flac"), want)
    body = dict(audio=b64, text="new words", parts_to_edit=[[0.2, 0.5]], sample_rate=44100, encoding="flac")
    r = c.post("/v1/audio/edit", json=body)
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content == want.tobytes()
    assert "edited_speech.flac" in r.headers["content-disposition"]
    r = c.post("/v1/audio/edit", json=dict(body, response_format="wav"))
    assert r.status_code == 400 and "flac" in r.json()["detail"]
