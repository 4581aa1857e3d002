"""CPU: `wave_codec.read_flac` (the whole native FLAC format, the definition the device decoder equals) against the test-side writer
`flac_ref`, against anchors that do not depend on the two agreeing with each other (numpy.diff, `encode_flac` / `decode_flac`, mid/side by
hand), its refusals one by one, `load_audio`, and the routes with a FLAC upload."""
import base64
import io
import wave

import numpy as np
import pytest
import torch

import flac_cases as C
import flac_ref as R
from test_ref_frontend_host import TEXT, StandInModel, StandInVocoder, _pcm, _tone16, _wav
from tts_indic_server_f5_amd import infer, serve
from tts_indic_server_f5_amd import wave_codec as W

REQUIRED = (["constant", "verbatim"] + [f"fixed_{o}" for o in range(5)] + ["lpc_order_1", "lpc_order_8", "lpc_order_32", "lpc_precision_2_shift_0",
            "lpc_precision_15_shift_14", "rice_0", "rice_14", "rice_method1_30", "escape_0", "escape_17", "partition_0", "partition_largest", "wasted_1",
            "wasted_7"] + [f"bits_{b}" for b in (8, 12, 16, 20, 24, 32)] + [f"channels_{c}" for c in (1, 2, 3, 8)] +
            ["stereo_left_side", "stereo_side_right", "stereo_mid_side", "variable_blocking", "short_last_frame", "frames_130_of_16"] +
            [f"block_code_{c}_{b}" for b, c in R.BLOCK_CODES.items()] + ["block_form_8bit", "block_form_16bit"] +
            [f"rate_table_{r}" for r in R.RATE_CODES] + ["rate_from_streaminfo", "rate_khz", "rate_hz", "rate_dahz", "padding_and_seektable", C.FULL])


def test_no_case_is_left_out():
    cases = C.cases()
    assert not [k for k in REQUIRED if k not in cases]
    assert len(cases["frames_130_of_16"]["sizes"]) == 131 and cases["frames_130_of_16"]["stream"].count(b"\xff\xf8") >= 130
    assert cases[C.FULL]["x"].shape == (2, 44100) and len(cases[C.FULL]["sizes"]) == 12


@pytest.mark.parametrize("name", list(C.cases()))
def test_case_matrix(name):
    v = C.cases()[name]
    samples, rate, bits = W.read_flac(v["stream"])
    assert samples.dtype == np.int32 and samples.shape == v["x"].shape and np.array_equal(samples, v["x"])
    assert (rate, bits) == (v["rate"], v["bits"])
    assert np.array_equal(W.read_flac(np.frombuffer(v["stream"], dtype=np.uint8))[0], samples)      # an array of bytes reads the same


# ------------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize("coefs", [[2, -1], [3, -3, 1], [4, -6, 4, -1]])
@pytest.mark.parametrize("shift", [0, 3, 9])
def test_lpc_coefficient_order_and_sign_against_numpy_diff(coefs, shift):
    rng = np.random.default_rng(len(coefs) + shift)
    x = np.cumsum(rng.integers(-300, 301, size=96))
    o = len(coefs)
    scaled = [c << shift for c in coefs]
    assert R.lpc_residuals(x, scaled, shift) == np.diff(x, o).tolist()
    stream, _ = R.write_flac(x, 16000, 16, block=48, subs=[R.sub("lpc", coefs=scaled, precision=4 + shift, shift=shift)])
    assert np.array_equal(W.read_flac(stream)[0][0], x)
    fixed, _ = R.write_flac(x, 16000, 16, block=48, subs=[R.sub("fixed", order=o)])
    assert np.array_equal(W.read_flac(fixed)[0][0], x)
    # the same residuals either way: the LPC subframe is the fixed one plus its coefficient table
    assert len(stream) == len(fixed) + 2 * ((4 + 5 + o * (4 + shift) + 7) // 8) or len(stream) > len(fixed)


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 9000])
def test_every_encode_flac_output_reads_the_same(n):
    rng = np.random.default_rng(n)
    for pcm in ((rng.standard_normal(n) * 3000).astype(np.int16), np.full(n, 77, dtype=np.int16), rng.integers(-32768, 32768, n).astype(np.int16)):
        s = W.encode_flac(pcm, 24000)
        old, rate = W.decode_flac(s)
        samples, r, bits = W.read_flac(s)
        assert np.array_equal(samples[0], old) and np.array_equal(old, pcm) and (r, bits) == (rate, 16) and samples.shape == (1, n)


def test_mid_side_by_hand():
    assert [v.tolist() for v in W.flac_unstereo(10, np.array([3]), np.array([3]))] == [[5], [2]]
    assert [v.tolist() for v in W.flac_unstereo(10, np.array([0]), np.array([-7]))] == [[-3], [4]]
    assert [v.tolist() for v in W.flac_unstereo(8, np.array([5]), np.array([3]))] == [[5], [2]]
    assert [v.tolist() for v in W.flac_unstereo(9, np.array([3]), np.array([2]))] == [[5], [2]]
    # the same through a stream whose coded planes are written as given: (mid, side) = (3, 3), (0, -7)
    frame = R.frame([[3, 0] * 8, [3, -7] * 8], 0, 24000, 16, [R.sub()] * 2, stereo=10, coded=True)
    samples, _, _ = W.read_flac(R.stream_header(24000, 2, 16, 16) + frame)
    assert samples.tolist() == [[5, -3] * 8, [2, 4] * 8]
    # and the writer's own forward transform agrees
    assert R.frame([[5, -3] * 8, [2, 4] * 8], 0, 24000, 16, [R.sub()] * 2, stereo=10) == frame


# ------------------------------------------------------------------------------------------------ refusals
def _frames(x=None, **kw):
    x = np.cumsum(np.random.default_rng(1).integers(-50, 51, size=(1, 96)), axis=1) if x is None else x
    kw.setdefault("subs", [R.sub("fixed", order=2)] * np.atleast_2d(x).shape[0])
    return R.write_flac(x, 24000, 16, block=32, **kw)


def _patched(at, fn, **kw):
    """A stream whose first frame has byte `at` (counted from the frame's start) changed by fn, with both checksums made right again."""
    s, sizes = _frames(**kw)
    s = bytearray(s)
    s[sizes[0] + at] = fn(s[sizes[0] + at]) & 0xFF
    return C._repair(s, sizes)


def _refused(stream, match):
    with pytest.raises(ValueError, match=match):
        W.read_flac(stream)


def test_refusals_of_the_metadata():
    s, _ = _frames()
    _refused(b"fLaX" + s[4:], "not a FLAC stream")
    _refused(s[:4] + b"\x81" + s[5:], "first metadata block is not STREAMINFO")
    _refused(s[:7] + b"\x21" + s[8:], "first metadata block is not STREAMINFO")
    _refused(s[:30], "truncated FLAC stream: metadata")
    _refused(s[:4] + b"\x00" + s[5:], "truncated FLAC stream: metadata")                 # not the last block, and nothing follows the frames
    _refused(R.stream_header(24000, 1, 3, 0), "3 bits per sample")
    _refused(R.stream_header(0, 1, 16, 0), "sample rate 0")


def test_refusals_of_the_checksums():
    s, sizes = _frames()
    for frame in range(3):
        at = sum(sizes[:frame + 1])
        _refused(s[:at + 2] + bytes([s[at + 2] ^ 0x10]) + s[at + 3:], f"header CRC-8 of the frame at byte {at}")
        end = at + sizes[frame + 1]
        _refused(s[:end - 1] + bytes([s[end - 1] ^ 0x01]) + s[end:], f"CRC-16 of the frame at byte {at}")
        _refused(s[:at + 12] + bytes([s[at + 12] ^ 0x40]) + s[at + 13:], "corrupt FLAC stream|truncated FLAC stream")   # (the parser or the CRC-16, whichever meets it)


def test_refusals_of_reserved_codes():
    _refused(_patched(1, lambda b: b | 0x02), "reserved bit after the sync")
    _refused(_patched(0, lambda b: 0xFE), "no frame sync at byte 42")
    _refused(_patched(2, lambda b: b & 0x0F), "reserved block-size code 0")
    _refused(_patched(2, lambda b: b | 0x0F), "invalid sample-rate code 15")
    _refused(_patched(3, lambda b: 0xB0 | (b & 0x0F)), "reserved channel code 11")
    _refused(_patched(3, lambda b: 0xF0 | (b & 0x0F)), "reserved channel code 15")
    _refused(_patched(3, lambda b: (b & 0xF1) | 0x06), "reserved sample-size code 3")
    _refused(_patched(3, lambda b: b | 0x01), "reserved bit in the header")
    _refused(_patched(4, lambda b: 0x80), "coded number of the frame at byte 42 .lead byte 0x80")
    _refused(_patched(4, lambda b: 0xFF), "coded number of the frame at byte 42 .lead byte 0xff")
    _refused(_patched(4, lambda b: 0xFE), "coded number")                                 # 36 bits belong to variable blocking alone
    hlen = 7                                                                               # sync 2, codes 2, number 1, 8-bit block size 1, CRC-8 1
    _refused(_patched(hlen, lambda b: b | 0x80), "subframe padding bit")
    _refused(_patched(hlen, lambda b: 0x04), "reserved subframe type 0x02")
    _refused(_patched(hlen, lambda b: 0x1A), "reserved subframe type 0x0d")
    _refused(_patched(hlen, lambda b: 0x3E), "reserved subframe type 0x1f")
    _refused(_patched(hlen + 5, lambda b: b | 0x80), "residual coding method [23]")
    lpc = dict(subs=[R.sub("lpc", coefs=[2, -1], precision=3, shift=0)])
    _refused(_patched(hlen + 5, lambda b: b | 0xF0, **lpc), "invalid LPC precision code 1111")
    _refused(_patched(hlen + 5, lambda b: b | 0x08, **lpc), "negative LPC shift")
    # a continuation byte that is none
    s, sizes = R.write_flac(np.zeros(16 * 130, dtype=np.int64), 24000, 16, block=16, subs=[R.sub("constant")])
    at = sum(sizes[:129])
    assert s[at + 4] == 0xC2 and s[at + 5] == 0x80                                         # frame 128: two bytes
    _refused(C._repair(s[:at + 5] + b"\x40" + s[at + 6:], sizes), "continuation byte 0x40")


def test_refusals_of_the_subframe_layout():
    hlen = 7
    _refused(_patched(hlen, lambda b: b | 0x01), "wasted bits leave no sample bits|samples outside|CRC|truncated|partition order")
    s, sizes = _frames(x=np.zeros((1, 96), dtype=np.int64), subs=[R.sub("verbatim")])
    s = bytearray(s)
    s[sizes[0] + hlen] |= 0x01                                                             # wasted-bits flag, then 16 zero bits and a one: k = 17
    s[sizes[0] + hlen + 3] = 0x80
    _refused(C._repair(s, sizes), "17 wasted bits leave no sample bits")
    short, sizes = R.write_flac(np.arange(3), 24000, 16, blocks=[3], subs=[R.sub("fixed", order=3)])
    s = bytearray(short)
    s[sizes[0] + hlen] = (12 << 1)                                                         # FIXED order 4 in a block of 3
    _refused(C._repair(s, sizes), "predictor order 4 in a block of 3")
    _refused(C.refusals()["a partition order too large for the block"], "partition order does not fit the block")
    big = R.write_flac(np.zeros(32, dtype=np.int64), 24000, 16, block=32, md5=False,
                       subs=[R.sub("fixed", order=0, method=1, params=30, residuals=[0] * 31 + [1 << 31])])[0]
    _refused(big, "a residual outside 32 bits")


def test_refusals_of_numbering_and_sizes():
    x = np.arange(96)
    sub = [R.sub("fixed", order=1)]
    head = R.stream_header(24000, 1, 16, 96, min_block=32, max_block=32)
    f = [R.frame([x[i * 32:(i + 1) * 32]], i, 24000, 16, sub) for i in range(3)]
    assert np.array_equal(W.read_flac(head + b"".join(f))[0][0], x)
    _refused(head + f[0] + f[2] + f[1], "numbered 2, expected 1")
    _refused(head + f[1] + f[2], "numbered 1, expected 0")
    v = [R.frame([x[i * 32:(i + 1) * 32]], n, 24000, 16, sub, variable=True) for i, n in enumerate((0, 32, 65))]
    _refused(head + b"".join(v), "numbered 65, expected 64")
    _refused(head + f[0] + v[1], "blocking strategy changes")
    _refused(R.stream_header(24000, 1, 16, 96, min_block=16, max_block=31) + b"".join(f), "block of 32 at byte 42, STREAMINFO's largest is 31")
    _refused(R.stream_header(24000, 1, 16, 96, min_block=33, max_block=64) + b"".join(f), "block of 32 at byte 42, STREAMINFO's smallest is 33")
    odd = [R.frame([x[:32]], 0, 24000, 16, sub), R.frame([x[32:48]], 1, 24000, 16, sub), R.frame([x[48:80]], 2, 24000, 16, sub)]
    _refused(R.stream_header(24000, 1, 16, 80, min_block=16, max_block=32) + b"".join(odd), "block of 16 at byte .* in a fixed-blocking stream of 32")
    _refused(R.stream_header(24000, 1, 8, 96, min_block=32, max_block=32) + b"".join(f), "has 1 channel.s. at 16 bits")
    _refused(R.stream_header(24000, 2, 16, 96, min_block=32, max_block=32) + b"".join(f), "has 1 channel.s. at 16 bits")
    _refused(R.stream_header(16000, 1, 16, 96, min_block=32, max_block=32) + b"".join(f), "24000 Hz, STREAMINFO 1 at 16 and 16000")
    _refused(R.stream_header(24000, 1, 16, 95, min_block=32, max_block=32) + b"".join(f), "STREAMINFO names 95 samples, the frames hold 96")
    _refused(head + b"".join(f) + b"\x00\x00", "no frame sync at byte 117")
    _refused(head + b"".join(f) + b"\x00", "truncated FLAC stream: header of the frame at byte 117")
    _refused(R.stream_header(24000, 1, 16, 96, md5=bytes(15) + b"\x01", min_block=32, max_block=32) + b"".join(f), "STREAMINFO's MD5 is 0{30}01, the samples'")
    good = R.stream_header(24000, 1, 16, 96, md5=R.md5_of(x[None], 16), min_block=32, max_block=32) + b"".join(f)
    assert np.array_equal(W.read_flac(good)[0][0], x)


def test_refusals_of_samples_outside_their_depth():
    top = [R.sub("fixed", order=1, residuals=[0] * 30 + [1])]
    _refused(R.write_flac(np.full(32, 32767), 24000, 16, block=32, subs=top, md5=False)[0], "samples outside 16 bits")
    low = [R.sub("lpc", coefs=[1], precision=2, shift=0, wasted=2, residuals=[0] * 30 + [-1])]
    _refused(R.write_flac(np.full(32, -32768), 24000, 16, block=32, subs=low, md5=False)[0], "samples outside 14 bits")
    # a side channel may use its extra bit; the channel it reconstructs may not leave the sample size
    frame = R.frame([[32767] * 16, [-40000] * 16], 0, 24000, 16, [R.sub()] * 2, stereo=8, coded=True)
    _refused(R.stream_header(24000, 2, 16, 16) + frame, "samples outside 16 bits")
    frame = R.frame([[40000] * 16, [32767] * 16], 0, 24000, 16, [R.sub()] * 2, stereo=9, coded=True)
    _refused(R.stream_header(24000, 2, 16, 16) + frame, "samples outside 16 bits")
    frame = R.frame([[32767] * 16, [65535] * 16], 0, 24000, 16, [R.sub()] * 2, stereo=10, coded=True)
    _refused(R.stream_header(24000, 2, 16, 16) + frame, "samples outside 16 bits")
    frame = R.frame([[32767] * 16, [65535] * 16], 0, 24000, 16, [R.sub()] * 2, stereo=8, coded=True)
    assert W.read_flac(R.stream_header(24000, 2, 16, 16) + frame)[0].tolist() == [[32767] * 16, [-32768] * 16]


def test_truncation_at_every_frame_boundary():
    for name in ("fixed_2", "stereo_mid_side", "variable_blocking", "unknown_total_and_no_md5"):
        v = C.cases()[name]
        s, bounds = v["stream"], np.cumsum(v["sizes"]).tolist()
        for b in bounds:
            for cut in (b - 1, b + 1):
                if cut < len(s):
                    with pytest.raises(ValueError, match="truncated|STREAMINFO names|MD5|no frame sync"):
                        W.read_flac(s[:cut])
    # a stream that names no total and no MD5 may end at any frame boundary -- and only there
    v = C.cases()["unknown_total_and_no_md5"]
    assert W.read_flac(v["stream"][:v["sizes"][0] + v["sizes"][1]])[0].shape == (1, 32)


def test_the_cap():
    assert W.FLAC_MAX_SECONDS == 600
    _refused(R.stream_header(8000, 1, 16, 600 * 8000 + 1), "FLAC stream too long: STREAMINFO names 4800001 samples")
    assert W.read_flac(R.stream_header(8000, 1, 16, 0))[0].shape == (1, 0)
    # a few bytes of CONSTANT frames that declare no total: the running count stops them (1 Hz: 600 samples)
    frames = [R.frame([[5] * 256], i, 1, 16, [R.sub("constant")], rate_form="info") for i in range(3)]
    head = R.stream_header(1, 1, 16, 0, min_block=256, max_block=256)
    assert W.read_flac(head + frames[0] + frames[1])[0].shape == (1, 512)
    _refused(head + b"".join(frames), "FLAC stream too long: more than 600 s at 1 Hz")
    big = R.frame([[0] * 16], (1 << 36) - 16, 24000, 16, [R.sub("constant")], variable=True)
    assert len(big) < 20
    _refused(R.stream_header(24000, 1, 16, 0) + big, "numbered 68719476720, expected 0")


# ------------------------------------------------------------------------------------------------ load_audio
def _wav_of(x, rate, bits):
    """x int [ch, n] as a PCM WAV of `bits` (8: unsigned)."""
    ch, n = x.shape
    width = bits // 8
    if bits == 8:
        raw = (x.T + 128).astype(np.uint8).tobytes()
    else:
        raw = b"".join(int(v).to_bytes(width, "little", signed=True) for v in x.T.reshape(-1))
    return (b"RIFF" + (36 + len(raw)).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") + (1).to_bytes(2, "little") +
            ch.to_bytes(2, "little") + rate.to_bytes(4, "little") + (rate * ch * width).to_bytes(4, "little") + (ch * width).to_bytes(2, "little") +
            bits.to_bytes(2, "little") + b"data" + len(raw).to_bytes(4, "little") + raw)


@pytest.mark.parametrize("bits", [8, 16, 24])
@pytest.mark.parametrize("ch", [1, 2])
def test_load_audio_of_flac_equals_load_wav_of_the_same_samples(bits, ch, tmp_path):
    rng = np.random.default_rng(bits + ch)
    x = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(ch, 200))
    x[:, 0], x[:, 1] = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    flac, _ = R.write_flac(x, 22050, bits, block=64, stereo=10 if ch == 2 else None)
    a, ra = W.load_audio(flac)
    b, rb = W.load_wav(_wav_of(x, 22050, bits))
    assert ra == rb == 22050 and a.dtype == b.dtype == torch.float32 and torch.equal(a, b)
    assert infer.load_audio is W.load_audio and infer.read_flac is W.read_flac
    p = tmp_path / "clip.flac"
    p.write_bytes(flac)
    assert torch.equal(W.load_audio(str(p))[0], a) and torch.equal(W.load_audio(io.BytesIO(flac))[0], a)
    # WAV goes where it went, and a reader handed in replaces read_flac
    assert torch.equal(W.load_audio(_wav_of(x, 22050, bits))[0], b)
    seen = []
    W.load_audio(flac, flac=lambda d: (seen.append(d), W.read_flac(d))[1])
    assert seen == [flac]


def test_load_audio_sniffs_streaminfo_not_the_magic_alone():
    with pytest.raises(ValueError, match="not a WAV file: FLAC stream"):
        W.load_audio(b"fLaC" + bytes(40))
    with pytest.raises(ValueError, match="not a WAV file: FLAC stream"):
        W.load_wav(C.cases()["verbatim"]["stream"])
    with pytest.raises(ValueError, match="not a RIFF/WAVE file"):
        W.load_audio(b"OggS" + bytes(40))
    assert not W.is_flac(b"fLaC" + bytes(40)) and W.is_flac(b"fLaC\x00\x00\x00\x22") and W.is_flac(b"fLaC\x80\x00\x00\x22")
    with pytest.raises(ValueError, match="truncated FLAC stream: metadata"):
        W.load_audio(b"fLaC\x80\x00\x00\x22" + bytes(10))


# ------------------------------------------------------------------------------------------------ the routes
def _b64(raw):
    return base64.b64encode(raw).decode()


def _flac_upload(frames, rate):
    x = frames.T.astype(np.int64)
    return R.write_flac(x, rate, 16, block=4096, subs=lambda i, c: R.sub("fixed", order=2, porder=4 if (i + 1) * 4096 <= x.shape[1] else 0),
                        stereo=8 if x.shape[0] == 2 else None)[0]


@pytest.fixture()
def served(tmp_path):
    from fastapi.testclient import TestClient
    frames = _tone16(seconds=1.5)
    wav_path, flac_path = tmp_path / "prompt.wav", tmp_path / "prompt.flac"
    wav_path.write_bytes(_wav(frames, 24000))
    flac_path.write_bytes(_flac_upload(frames, 24000))
    reg = serve.VoiceRegistry()
    reg.add("wav voice", str(wav_path), "reference words")
    reg.add("flac voice", str(flac_path), "reference words")
    mgr = serve.TTSManager(nfe_step=4).load(StandInModel(), StandInVocoder())
    return TestClient(serve.create_app(mgr, reg)), mgr, frames


def test_routes_take_a_flac_upload_like_the_wav_of_the_same_samples(served, monkeypatch):
    c, mgr, frames = served
    stereo = np.stack([frames[:, 0], (frames[:, 0] // 2)], axis=1)
    for clip in (frames, stereo):
        wav, flac = _wav(clip, 24000), _flac_upload(clip, 24000)
        assert torch.equal(W.load_audio(flac)[0], W.load_wav(wav)[0])
        got = []
        for raw in (wav, flac):
            r = c.post("/v1/audio/speech/clone", json=dict(text=TEXT, ref_audio=_b64(raw), ref_text="reference words"))
            assert r.status_code == 200, r.text
            got.append(_pcm(r.content))
        assert len(got[0]) > 0 and np.array_equal(got[0], got[1])
        got = []
        for raw in (wav, flac):
            body = dict(text="[main] " + TEXT + " [other] And a reply.", voices=dict(main=dict(ref_audio=_b64(raw), ref_text="reference words"),
                                                                                    other=dict(ref_audio_name="wav voice")))
            r = c.post("/v1/audio/speech/script", json=body)
            assert r.status_code == 200, r.text
            got.append(_pcm(r.content))
        assert len(got[0]) > 0 and np.array_equal(got[0], got[1])
        assert np.array_equal(mgr.synthesize_clip(TEXT, flac, "reference words"), mgr.synthesize_clip(TEXT, wav, "reference words"))
    # a registered voice whose file is FLAC
    a = c.post("/v1/audio/speech/voice", json=dict(text=TEXT, ref_audio_name="wav voice"))
    b = c.post("/v1/audio/speech/voice", json=dict(text=TEXT, ref_audio_name="flac voice"))
    assert a.status_code == 200 and b.status_code == 200 and np.array_equal(_pcm(a.content), _pcm(b.content)) and len(_pcm(a.content)) > 0
    # refusals keep their texts
    r = c.post("/v1/audio/speech/clone", json=dict(text=TEXT, ref_audio=_b64(b"fLaC" + bytes(40)), ref_text="reference words"))
    assert r.status_code == 400 and r.json()["detail"].startswith("Invalid audio: not a WAV file")
    r = c.post("/v1/audio/speech/clone", json=dict(text=TEXT, ref_audio="not base64 !!", ref_text="reference words"))
    assert r.status_code == 400 and r.json()["detail"] == "Audio must be a base64-encoded WAV file."
    r = c.post("/v1/audio/speech/clone", json=dict(text=TEXT, ref_audio=_b64(_flac_upload(frames, 24000)[:-3]), ref_text="reference words"))
    assert r.status_code == 400 and r.json()["detail"].startswith("Invalid audio: truncated FLAC stream")


def test_edit_route_takes_flac_and_its_own_flac_answer(served, monkeypatch):
    c, mgr, frames = served
    seen = []

    def fake_edit(edits, *a, **kw):
        seen.append([np.asarray(e.cond_wave if hasattr(e, "cond_wave") else 0) for e in edits])
        return [((0.4 * np.sin(np.arange(30011) * 0.03)).astype(np.float32), 24000, None)] * len(edits)

    preps = []
    real = infer.prepare_edit
    monkeypatch.setattr(infer, "prepare_edit", lambda audio, *a, **kw: (preps.append(audio), real(audio, *a, **kw))[1])
    monkeypatch.setattr(infer, "speech_edit_batch", fake_edit)
    body = dict(text="new words", parts_to_edit=[[0.2, 0.5]])
    wav, flac = _wav(frames, 24000), _flac_upload(frames, 24000)
    a = c.post("/v1/audio/edit", json=dict(body, audio=_b64(wav)))
    b = c.post("/v1/audio/edit", json=dict(body, audio=_b64(flac)))
    assert a.status_code == 200 and b.status_code == 200, (a.text, b.text)
    assert a.content == b.content and len(_pcm(a.content)) == 30011
    assert torch.equal(preps[0][0], preps[1][0]) and preps[0][1] == preps[1][1] == 24000     # the recording reaches the edit as the same samples
    # the route's own FLAC answer posted back to it
    r = c.post("/v1/audio/edit", json=dict(body, audio=_b64(wav), encoding="flac"))
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac"
    back = c.post("/v1/audio/edit", json=dict(body, audio=_b64(r.content)))
    assert back.status_code == 200, back.text
    assert torch.equal(preps[-1][0], torch.from_numpy(W.decode_flac(r.content)[0].astype(np.float32) / 32768.0)[None])
    assert np.array_equal(mgr.edit(flac, "new words", [[0.2, 0.5]]), mgr.edit(wav, "new words", [[0.2, 0.5]]))
    r = c.post("/v1/audio/edit", json=dict(body, audio=_b64(flac[:-5])))
    assert r.status_code == 400 and r.json()["detail"].startswith("Invalid audio: truncated FLAC stream")
    r = c.post("/v1/audio/edit", json=dict(body, audio=_b64(b"fLaC" + bytes(40))))
    assert r.status_code == 400 and r.json()["detail"].startswith("Invalid audio: not a WAV file")
    r = c.post("/v1/audio/edit", json=dict(body, audio="not base64 !!"))
    assert r.status_code == 400 and r.json()["detail"] == "Audio must be a base64-encoded WAV file."


def test_manager_switch_and_default():
    assert serve.DEVICE_DECODE_DEFAULT in (True, False)
    assert serve.TTSManager().device_decode == serve.DEVICE_DECODE_DEFAULT
    assert serve.TTSManager(device_decode=True).device_decode is True and serve.TTSManager(device_decode=False).device_decode is False
    # without a device model the manager decodes on the host, whatever the switch says: nothing here touches a GPU
    flac = C.cases()["stereo_mid_side"]
    wave_, rate = serve.TTSManager(device_decode=True).load(StandInModel(), StandInVocoder()).decode_audio(flac["stream"])
    assert rate == flac["rate"] and np.array_equal(np.rint(wave_.numpy() * 32768).astype(np.int64), flac["x"])
