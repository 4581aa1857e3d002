"""GPU: the device FLAC decoder (f5hip_flac_decode, torch.ops.f5hip.flac_decode, `ops.flac_decode`) against its definition,
`wave_codec.read_flac`.  Equality only: the same samples, rate and bits, or the same ValueError.  The bounds of the core are not tested here
but on the CPU (tests/test_flac_in_core.py); the refusals below are the short list that has passed that run."""
import io
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import flac_cases as C  # noqa: E402
import flac_ref as R  # noqa: E402
from tts_indic_server_f5_amd import _lib, ops, serve, synth, torch_ops  # noqa: E402
from tts_indic_server_f5_amd import wave_codec as W  # noqa: E402

LAUNCHES = 5           # include/f5hip.h f5hip_flac_decode: scan, offsets, frame, chain, pack -- whatever the batch


def _counter(name):
    import ctypes
    v = ctypes.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), ctypes.byref(v)), "get_counter")
    return v.value


def _same(got, v):
    samples, rate, bits = got
    assert samples.dtype == np.int32 and samples.shape == v["x"].shape and np.array_equal(samples, v["x"])
    assert (rate, bits) == (v["rate"], v["bits"])


@pytest.fixture(params=["torch_op", "ctypes"])
def path(request, monkeypatch):
    if request.param == "ctypes":
        monkeypatch.setattr(torch_ops, "_loaded", False)
    else:
        assert torch_ops.load()
    return request.param


def _packed(streams, rng):
    """The streams in one buffer with a loud filler between them (sync-like bytes included), starting at offsets 0, 1, 3 and 7 mod 8."""
    buf, spans = bytearray(), []
    for i, s in enumerate(streams):
        want = (0, 1, 3, 7)[i % 4]
        pad = (want - len(buf)) % 8 + (8 * int(rng.integers(0, 3)) if i else 0)
        filler = (b"\xff\xf8\xc9\x08\x00\xc2" + rng.integers(0, 256, size=pad + 8, dtype=np.uint8).tobytes())[:pad]
        buf += filler
        assert len(buf) % 8 == want
        spans.append((len(buf), len(buf) + len(s)))
        buf += s
    buf += b"\xff\xf8\xc9\x08\x00"
    return bytes(buf), spans


def test_case_matrix_in_one_call(path):
    cases = C.device_cases()
    names = list(cases)
    buf, spans = _packed([cases[k]["stream"] for k in names], np.random.default_rng(3))
    assert {a % 8 for a, _ in spans} == {0, 1, 3, 7}
    got = ops.flac_decode_packed(buf, spans)
    for k, g in zip(names, got):
        _same(g, cases[k])
    for batch in (1, 7):
        _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset")
        got = ops.flac_decode([cases[k]["stream"] for k in names[3:3 + batch]])
        assert _counter("flac_decode_launches") == LAUNCHES and _counter("flac_decode_streams") == batch
        for k, g in zip(names[3:3 + batch], got):
            _same(g, cases[k])


def test_a_false_sync_is_never_visited(path):
    stream, x = C.false_sync()
    ref = W.read_flac(stream)
    assert np.array_equal(ref[0], x)
    samples, rate, bits = ops.flac_decode([stream])[0]
    assert np.array_equal(samples, x) and (rate, bits) == (44100, 16)


def test_number_seam_and_variable_blocking(path):
    cases = C.cases()
    names = ["frames_130_of_16", "variable_blocking", "variable_number_seam"]
    for k, g in zip(names, ops.flac_decode([cases[k]["stream"] for k in names])):
        _same(g, cases[k])


def test_streams_outside_the_limits_come_back_through_the_host(path):
    cases = C.cases()
    names = ["channels_3", "bits_32", "block_code_15_32768", "channels_8", "stereo_mid_side"]
    assert [cases[k]["device"] for k in names] == [False, False, False, False, True]
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset")
    for k, g in zip(names, ops.flac_decode([cases[k]["stream"] for k in names])):
        _same(g, cases[k])
    assert _counter("flac_decode_launches") == LAUNCHES


def test_refusals_are_the_definitions(path):
    good = C.cases()["stereo_left_side"]
    for name, stream in C.refusals().items():
        with pytest.raises(ValueError) as want:
            W.read_flac(stream)
        with pytest.raises(ValueError) as got:
            ops.flac_decode([good["stream"], stream])
        assert str(got.value) == str(want.value), name
        _same(ops.flac_decode([good["stream"]])[0], good)         # the next call on good streams is correct


def test_full_size_case(path):
    v = C.cases()[C.FULL]
    assert len(v["sizes"]) - 1 == 11
    _same(ops.flac_decode([v["stream"]])[0], v)
    two = ops.flac_decode([v["stream"], C.cases()["bits_24"]["stream"], v["stream"]])
    _same(two[0], v), _same(two[1], C.cases()["bits_24"]), _same(two[2], v)


ARCH = dict(dim=256, depth=4, heads=4, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=96)
VOCAB = {chr(32 + i): i for i in range(96)}


@pytest.mark.parametrize("device_decode", [True, False])
def test_synthesize_clip_takes_flac_like_wav(device_decode):
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    x = (synth.ref_audio(24000 * 2, amp=0.15).numpy()[0] * 32767).astype(np.int16)
    buf = io.BytesIO()
    with wave.open(buf, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(24000)
        f.writeframes(x.tobytes())
    flac, _ = R.write_flac(x, 24000, 16, block=4096, subs=lambda i, c: R.sub("fixed", order=2, porder=4 if (i + 1) * 4096 <= len(x) else 0))
    model = F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB)
    mgr = serve.TTSManager(nfe_step=4, device_decode=device_decode).load(model, F5HipVocos(synth.vocos_state_dict()))
    try:
        _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset")
        a = mgr.synthesize_clip("Always remember, I endure.", buf.getvalue(), "Hi there.", seed=3)
        assert _counter("flac_decode_launches") == 0
        b = mgr.synthesize_clip("Always remember, I endure.", flac, "Hi there.", seed=3)
        assert _counter("flac_decode_launches") == (5 if device_decode else 0)
        assert len(a) > 0 and np.array_equal(a, b)
    finally:
        mgr.close()
