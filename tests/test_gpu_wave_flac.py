"""FLAC delivery on the device (csrc/wave_out.h, f5hip_wave_flac: the int16 PCM of a ragged batch of requests -> each request's complete
native FLAC stream in at most three launches) against the host definition `infer.encode_flac`, alone, chained behind `ops.wave_finish` /
`ops.wave_encode`, and through `infer_requests` with the device back-end on a tiny model.

Every comparison is equality of bytes and lengths: there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, ops, serve, synth, torch_ops  # noqa: E402

from test_gpu_request_knobs import ARCH, REF_TEXT, TEXT, VOCAB, _prompt  # noqa: E402

RATE = 24000
BLOCK = 4096
FADE_S = infer.cross_fade_duration
F = int(FADE_S * RATE)
LENGTHS = [0, 1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 2 * BLOCK + 3, 30011, 2 * BLOCK]      # 15: batches of 1, 2, 3, 4 and 5 requests


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _sine(n, freq, amp, noise=0.0, seed=2):
    x = amp * np.sin(2 * np.pi * freq * np.arange(n) / RATE) * 32768.0
    if noise:
        x = x + noise * np.random.default_rng(seed).standard_normal(n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _content(n, kind, seed):
    """The eight contents: one per subframe kind (CONSTANT twice, the five fixed orders, VERBATIM)."""
    rng = np.random.default_rng(seed)
    return [lambda: np.zeros(n, dtype=np.int16),
            lambda: np.full(n, 1234, dtype=np.int16),
            lambda: infer.quantise_pcm16(0.3 * rng.standard_normal(n)),
            lambda: np.clip(np.cumsum(200.0 * rng.standard_normal(n)), -32768, 32767).astype(np.int16),
            lambda: _sine(n, 100, 0.01),
            lambda: _sine(n, 1000, 0.3, noise=30.0, seed=seed),
            lambda: _sine(n, 300, 0.5),
            lambda: np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)][kind % 8]()


def _batches(turn):
    """The 15 lengths dealt into batches of 1 to 5 requests; request j of the deal takes content (j + turn) mod 8."""
    out, k = [], 0
    for size in (1, 2, 3, 4, 5):
        out.append([_content(n, k + j + turn, 100 * turn + k + j) for j, n in enumerate(LENGTHS[k:k + size])])
        k += size
    return out


def _device(pcms, rate, packed=True, cut=None):
    """ops.wave_flac on device copies of the requests -> [bytes per request].  `packed`: ONE buffer with the requests at `wave_finish`'s
    8-sample offsets and a loud filler between them (a read past a request's end would show); else one allocation per request.  `cut`: the
    actual lengths, on the device alone (the requests' arrays are then the upper bounds)."""
    dev = torch.device("cuda:0")
    lens = [len(x) for x in pcms]
    if packed:
        offsets, off = [], 0
        for n in lens:
            offsets.append(off)
            off += (n + 7) & ~7
        buf = np.full(off + 8, 23456, dtype=np.int16)
        for o, x in zip(offsets, pcms):
            buf[o:o + len(x)] = x
        src = torch.from_numpy(buf).to(dev)
    else:
        offsets, src = [0] * len(pcms), [torch.from_numpy(x.copy()).to(dev) for x in pcms]
    len_dev = None if cut is None else torch.tensor(cut, dtype=torch.int32, device=dev)
    data, out_len, out_off = ops.wave_flac(src, offsets, lens, len_dev, rate)
    assert data.dtype == torch.uint8 and out_len.dtype == torch.int32 and all(o % 16 == 0 for o in out_off)
    host, counts = data.cpu().numpy(), out_len.cpu().tolist()
    assert all(o + m <= (out_off[i + 1] if i + 1 < len(out_off) else len(host)) for i, (o, m) in enumerate(zip(out_off, counts)))
    return [host[o:o + m].tobytes() for o, m in zip(out_off, counts)]


def _check(got, want, where):
    assert len(got) == len(want), (where, len(got), len(want))
    if got != want:
        g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        raise AssertionError((where, "first differing byte", int(np.flatnonzero(g != w)[0])))


@pytest.mark.parametrize("turn", range(8))
def test_kernel_equals_the_host_definition_byte_for_byte(turn):
    """Each length meets each content over the eight turns, at 24 kHz; packed and in separate allocations."""
    for b, batch in enumerate(_batches(turn)):
        want = [infer.encode_flac(x, RATE).tobytes() for x in batch]
        for packed in (True, False):
            for i, (g, w) in enumerate(zip(_device(batch, RATE, packed), want)):
                _check(g, w, (turn, b, i, packed, len(batch[i])))


@pytest.mark.parametrize("rate", [8000, 44100])
def test_other_rates_change_the_rate_fields_alone(rate):
    for b, batch in enumerate(_batches(3)):
        for i, (g, x) in enumerate(zip(_device(batch, rate), batch)):
            _check(g, infer.encode_flac(x, rate).tobytes(), (rate, b, i))


def test_device_side_lengths():
    """len_dev shorter than max_len, as silence removal leaves it: the stream is that of the shorter request, whatever lies behind it."""
    batch = [_content(n, k + 2, k) for k, n in enumerate([30011, 2 * BLOCK, 4097, 300, 5000])]
    cut = [2 * BLOCK + 5, BLOCK, 0, 299, 4096]
    got = _device(batch, RATE, cut=cut)
    for i, (g, x, n) in enumerate(zip(got, batch, cut)):
        _check(g, infer.encode_flac(x[:n], RATE).tobytes(), (i, n))
    assert len(got[2]) == 42
    over = _device(batch[:2], RATE, cut=[10 ** 9, -5])                                  # clamped to [0, max_len]
    _check(over[0], infer.encode_flac(batch[0], RATE).tobytes(), "clamped above")
    _check(over[1], infer.encode_flac(batch[1][:0], RATE).tobytes(), "clamped below")


def test_frame_number_seams_in_one_long_request():
    frames = 2050
    x = np.zeros(frames * BLOCK - 100, dtype=np.int16)
    for f in (0, 126, 127, 128, 2046, 2047, 2048):
        x[f * BLOCK:(f + 1) * BLOCK] = infer.quantise_pcm16(0.001 * np.random.default_rng(f).standard_normal(BLOCK))
    x[-50:] = 77
    got, = _device([x], RATE, packed=False)
    _check(got, infer.encode_flac(x, RATE).tobytes(), "2050 frames")


def test_a_request_does_not_depend_on_its_call():
    batch = _batches(5)[4]
    first, again, reverse = _device(batch, RATE), _device(batch, RATE), _device(batch[::-1], RATE)[::-1]
    assert first == again == reverse
    for i in range(len(batch)):
        solo, = _device(batch[i:i + 1], RATE, packed=False)
        assert solo == first[i], i


def test_at_most_three_launches_per_call():
    _device(_batches(0)[0], RATE)                                                       # (the first call of a process also allocates)
    for idx, requests in ((0, 1), (4, 5)):
        _reset()
        _device(_batches(2)[idx], RATE)
        assert 1 <= _counter("wave_flac_launches") <= 3 and _counter("wave_flac_requests") == requests
        assert _counter("wave_encode_launches") == 0 and _counter("wave_finish_launches") == 0
    _reset()
    _device([np.zeros(0, dtype=np.int16)], RATE, packed=False)                          # nothing to encode: the header alone, one launch
    assert _counter("wave_flac_launches") == 1


def test_ctypes_and_torch_op_paths_agree():
    batch = _batches(6)[3]
    via_op = _device(batch, 44100)
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        for packed in (True, False):
            assert _device(batch, 44100, packed) == via_op
    finally:
        torch_ops._loaded = True


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    pcm = torch.zeros(4096, device=dev, dtype=torch.int16)
    out = torch.zeros(65536, device=dev, dtype=torch.uint8)
    out_len = torch.zeros(4, device=dev, dtype=torch.int32)

    def call(max_len=(100,), out_off=(0,), n=None, rate=8000, pcm_p=pcm.data_ptr(), out_p=out.data_ptr(), in_p=True, ml_p=True, oo_p=True,
             ol_p=out_len.data_ptr()):
        ml, oo = np.asarray(max_len, dtype=np.int32), np.asarray(out_off, dtype=np.int64)
        io = np.zeros(len(ml), dtype=np.int64)
        p = lambda a, on: C.c_void_p(a.ctypes.data) if on else None   # noqa: E731
        return lib.f5hip_wave_flac(len(ml) if n is None else n, C.c_void_p(pcm_p), p(io, in_p), p(ml, ml_p), None, rate, C.c_void_p(out_p), p(oo, oo_p),
                                   C.c_void_p(ol_p), _lib.current_stream_ptr())

    _reset()
    assert call(n=0) != 0 and b"bad argument" in lib.f5hip_last_error()
    for null in (dict(pcm_p=None), dict(in_p=False), dict(ml_p=False), dict(out_p=None), dict(oo_p=False), dict(ol_p=None)):
        assert call(**null) != 0 and b"bad argument" in lib.f5hip_last_error(), null
    for rate in (0, -8000, 11025, 96000):
        assert call(rate=rate) != 0 and b"sample rate must be one of" in lib.f5hip_last_error(), rate
    assert call(out_off=(8,)) != 0 and b"multiple of 16" in lib.f5hip_last_error()
    assert call(out_p=out.data_ptr() + 8) != 0 and b"aligned" in lib.f5hip_last_error()
    assert call(pcm_p=pcm.data_ptr() + 1) != 0 and b"aligned" in lib.f5hip_last_error()
    assert call(ol_p=out_len.data_ptr() + 2) != 0 and b"aligned" in lib.f5hip_last_error()
    assert call(max_len=(-1,)) != 0 and b"negative" in lib.f5hip_last_error()
    assert call(max_len=(2 ** 31 - 1, 2 ** 31 - 1), out_off=(0, 0)) != 0 and b"2^31" in lib.f5hip_last_error()      # samples in (refused unread)
    assert call(max_len=(2 ** 30 + 5,)) != 0 and b"2^31" in lib.f5hip_last_error()                                  # bytes out
    assert lib.f5hip_wave_flac_bound(-1) == 0 and lib.f5hip_wave_flac_bound(0) == 42 and lib.f5hip_wave_flac_bound(4097) == 42 + 2 * 4097 + 32
    with pytest.raises(_lib.F5HipError, match="sample rate"):
        ops.wave_flac(pcm, [0], [100], None, 11025)
    with pytest.raises(_lib.F5HipError):
        ops.wave_flac(pcm, [4000], [100], None, RATE)                                   # reads past the tensor
    with pytest.raises(_lib.F5HipError, match="int16"):
        ops.wave_flac(pcm.to(torch.int32), [0], [100], None, RATE)
    with pytest.raises(RuntimeError, match="sample rate"):
        torch.ops.f5hip.wave_flac([pcm], torch.zeros(1, dtype=torch.int64), torch.tensor([100], dtype=torch.int32), None, 12345)
    assert _counter("wave_flac_launches") == 0 and _counter("wave_flac_requests") == 0
    assert call() == 0 and _counter("wave_flac_launches") == 3 and _counter("wave_flac_requests") == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ behind wave_finish and wave_encode
def _silence_requests():
    """The "pause" and "all quiet" constructions of tests/test_gpu_wave_backend.py, and a plain request of two chunks"""
    noise = lambda n, s, amp: (amp * np.random.default_rng(s).standard_normal(n)).astype(np.float32)   # noqa: E731
    plateau = (np.sign(np.random.default_rng(4).standard_normal(3 * RATE) + 1e-9) * (50 / 32768.0)).astype(np.float32)
    pause = np.concatenate([noise(2 * RATE, 1, 0.1), np.zeros(int(2.5 * RATE), np.float32), noise(2 * RATE, 2, 0.1)])
    return [[pause], [plateau], [noise(9003, 5, 0.3), noise(7201, 6, 0.3)]], [True, True, False]


def test_finish_requests_takes_flac_on_the_device():
    """A mixed batch on the device path: one wave_flac call per distinct rate (behind one wave_encode call where the rate is not 24 kHz), the
    other formats as before, every result the host pipeline's bytes."""
    dev = torch.device("cuda:0")
    reqs, flags = _silence_requests()
    reqs = reqs + [reqs[2], reqs[0], reqs[2], reqs[2]]
    flags = flags + [False, True, False, False]
    rates = [None, 44100, None, 44100, 8000, None, 24000]
    encs = ["flac", "flac", "flac", "flac", "mulaw", None, "flac"]
    on_dev = [[torch.from_numpy(c).to(dev) for c in r] for r in reqs]
    want = infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16", sample_rate=rates, encoding=encs)
    pcm = infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16")
    infer.backend_stats.clear()
    _reset()
    got = infer.finish_requests(on_dev, ["x"] * len(reqs), FADE_S, flags, device_backend=True, want="pcm16", sample_rate=rates, encoding=encs)
    stats = dict(infer.backend_stats)
    assert stats["device_requests"] == len(reqs) and stats["device_calls"] == 1 and stats.get("host_requests", 0) == 0
    assert stats["flac_calls"] == 2 and stats["flac_requests"] == 5 and _counter("wave_flac_requests") == 5
    assert _counter("wave_flac_launches") <= 6 and _counter("wave_encode_launches") == 2        # 44100 for flac, (8000, mulaw)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and len(g) == len(w) and np.array_equal(g, w), i
    for i in (0, 1, 2, 3, 6):
        y, r = infer.decode_flac(got[i])
        assert r == (rates[i] or RATE) and np.array_equal(y, infer.resample_pcm16(pcm[i], r)), i
    assert len(got[1]) == 42                                                                     # "all quiet": the header alone
    # what came down of the flac requests is their streams and not the room between them that the VERBATIM bound leaves
    assert stats["flac_bytes"] == sum(len(got[i]) for i in (0, 1, 2, 3, 6))


# ------------------------------------------------------------------------------------------------ end to end on a tiny model
@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


def test_infer_requests_mixed_encodings_in_one_micro_batch(hip_objects, tmp_path):
    """pcm16, mulaw and flac requests, one flac request with `remove_silence` and a script with a gap, in ONE micro-batch with the device
    back-end: each flac result is the host pipeline's stream and decodes to the request's own PCM."""
    path = _prompt(tmp_path)
    text = TEXT[:110]                                                                   # one chunk: the test is about the tail of the pipeline
    script = f"{TEXT[:64]} [town] I live in town."
    voices = {"main": dict(ref_audio_path=path, ref_text=REF_TEXT), "town": dict(ref_audio=(synth.ref_audio(16000 * 2, seed=77, amp=0.05), 16000),
                                                                                  ref_text="Town speaks.")}
    opts = [dict(seed=7), dict(seed=7, sample_rate=8000, encoding="mulaw"), dict(seed=7, encoding="flac"),
            dict(seed=7, encoding="flac", sample_rate=44100, remove_silence=True), dict(seed=7, remove_silence=True)]
    out = {}
    for backend in (True, False):
        mgr = serve.TTSManager(nfe_step=8, device_backend=backend).load(*hip_objects)
        try:
            voice, ref_text_n = mgr._voice(path, REF_TEXT)
            batch = [(voice, ref_text_n, text, o) for o in opts]
            segments = mgr._script_segments(script, voices, 1.5)
            batch += [infer.ScriptRequest(segments, dict(seed=7, encoding="flac"), 1.5), infer.ScriptRequest(segments, dict(seed=7), 1.5)]
            _reset()
            infer.backend_stats.clear()
            out[backend] = mgr._run_batch(batch)
            if backend:
                assert infer.backend_stats["device_requests"] == len(batch) and infer.backend_stats.get("host_requests", 0) == 0
                assert infer.backend_stats["flac_calls"] == 2 and infer.backend_stats["flac_requests"] == 3
                assert _counter("wave_flac_requests") == 3 and _counter("wave_flac_launches") <= 6
            else:
                assert _counter("wave_flac_launches") == 0
        finally:
            mgr.close()
    dev, host = out[True], out[False]
    for i in (2, 3, 5):                                                                 # the host pipeline's bytes
        assert dev[i].dtype == host[i].dtype == np.uint8 and dev[i].tobytes() == host[i].tobytes(), i
    assert dev[0].dtype == np.int16 and np.array_equal(dev[1], infer.deliver_pcm16(dev[0], 8000, "mulaw"))
    assert dev[2].tobytes() == infer.encode_flac(dev[0], RATE).tobytes()
    for i, pcm, rate in ((2, dev[0], RATE), (3, infer.resample_pcm16(dev[4], 44100), 44100), (5, dev[6], RATE)):
        y, r = infer.decode_flac(dev[i])
        assert r == rate and np.array_equal(y, pcm), i
    gap = int(1.5 * RATE)
    assert len(dev[6]) > gap and len(dev[5]) < 2 * len(dev[6])                           # (the script is there, and its stream is smaller than its PCM)


def test_continuous_batcher_delivers_flac(hip_objects, tmp_path):
    """`SpanScheduler` hands its finished requests to `finish_requests` with their formats: a flac request through the continuous batcher is
    the stream of the same request's PCM, with the device back-end on and off, and a streamed one carries the same frames."""
    path, text = _prompt(tmp_path), TEXT[:110]
    got = {}
    for backend in (True, False):
        mgr = serve.TTSManager(nfe_step=8, micro_batch=dict(span_steps=3), device_backend=backend).load(*hip_objects)
        try:
            _reset()
            pcm = mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, seed=7)
            pcm = pcm if pcm.dtype == np.int16 else infer.quantise_pcm16(pcm)       # (int16 already with the device back-end)
            got[backend] = mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, seed=7, encoding="flac", sample_rate=8000)
            assert got[backend].dtype == np.uint8 and got[backend].tobytes() == infer.deliver_pcm16(pcm, 8000, "flac").tobytes(), backend
            assert _counter("wave_flac_requests") == (1 if backend else 0)
            if backend:
                pieces = list(mgr.synthesize_stream(text, ref_audio_path=path, ref_text=REF_TEXT, seed=7, encoding="flac", sample_rate=8000))
                assert pieces[0].tobytes() == infer.StreamFlacEncoder(8000).header()
                assert np.concatenate(pieces).tobytes()[42:] == got[backend].tobytes()[42:]
        finally:
            mgr.close()
    assert got[True].tobytes() == got[False].tobytes()
