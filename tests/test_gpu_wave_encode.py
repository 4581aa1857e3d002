"""The delivery format on the device (csrc/wave_out.h, f5hip_wave_encode: the 24 kHz int16 PCM of a ragged batch of requests resampled to
another rate and G.711-encoded in one launch) against the host definition `infer.resample_pcm16` / `infer.encode_g711`, alone and chained
behind `ops.wave_finish`, and `TTSManager(device_backend=True)` end to end on a tiny model.

Every comparison is `np.array_equal` on samples / code bytes and lengths, or equality of WAV bytes: there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, ops, serve, synth, torch_ops  # noqa: E402

from test_gpu_request_knobs import ARCH, REF_TEXT, TEXT, VOCAB, _prompt  # noqa: E402

RATE = 24000
FADE_S = infer.cross_fade_duration
F = int(FADE_S * RATE)
RATES = [r for r in infer.OUTPUT_SAMPLE_RATES if r != RATE]
ENCODINGS = infer.OUTPUT_ENCODINGS
FORMATS = [(8000, "mulaw"), (22050, "pcm16"), (48000, "alaw")]


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _content(n, kind, seed):
    """int16 PCM: noise at 0.3, all zeros, or the full-scale square wave 32767, -32768, ..."""
    if kind == 0:
        return infer.quantise_pcm16(0.3 * np.random.default_rng(seed).standard_normal(n))
    if kind == 1:
        return np.zeros(n, dtype=np.int16)
    return np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)


def _lengths(rate):
    """Request lengths around the kernel's seams at `rate`, 15 of them: dealt into batches of 1, 2, 3, 4 and 5 requests"""
    of, nf, width, _ = infer.resample_taps(RATE, rate)
    tile = ops.wave_encode_tile(rate)
    assert tile > 0 and tile % of == 0
    return [30011, 1, 2, of - 1, of, of + 1, width, 2 * width + of - 1, 2 * width + of + 1, tile - 1, tile, tile + 1, 2 * tile + 3, 29989, 0]


def _batches(rate):
    """Ten batches: the 15 lengths dealt into batches of 1 to 5 requests with the three contents in turn, then the same batches with noise in
    every request (zeros give one constant code whatever the taps and the window: every seam length must also run with content that tells)"""
    lens, out = _lengths(rate), []
    for turn in (True, False):
        k = 0
        for size in (1, 2, 3, 4, 5):
            out.append([_content(n, (k + j) % 3 if turn else 0, 1000 * rate + k + j) for j, n in enumerate(lens[k:k + size])])
            k += size
    return out


@pytest.fixture(scope="module")
def host_results():
    """{rate: [[resample_pcm16 of request] per batch]}: the host definition of every request, computed once and shared"""
    return {rate: [[infer.resample_pcm16(x, rate) for x in batch] for batch in _batches(rate)] for rate in RATES}


def _taps(rate):
    return None if rate == RATE else infer._device_taps(RATE, rate, torch.device("cuda:0"))


def _device(pcms, rate, enc, packed=True):
    """ops.wave_encode on device copies of the requests -> [numpy per request].  `packed`: ONE buffer with the requests at `wave_finish`'s
    8-sample offsets and a loud filler between them (a read past a request's end would show); else one allocation per request."""
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
    data, out_len, out_off = ops.wave_encode(src, offsets, lens, None, rate, enc, _taps(rate))
    assert data.dtype == torch.uint8 and out_len.dtype == torch.int32 and all(o % 16 == 0 for o in out_off)
    host, counts = data.cpu().numpy(), out_len.cpu().tolist()
    bps = 2 if enc == "pcm16" else 1
    return [host[o:o + m * bps].copy().view(np.int16 if enc == "pcm16" else np.uint8) for o, m in zip(out_off, counts)]


def _want(resampled, enc):
    return resampled if enc == "pcm16" else infer.encode_g711(resampled, enc)


@pytest.mark.parametrize("rate", RATES)
def test_kernel_equals_the_host_definition_bit_for_bit(host_results, rate):
    for b, (batch, res) in enumerate(zip(_batches(rate), host_results[rate])):
        for enc in ENCODINGS:
            for packed in (True, False):
                got = _device(batch, rate, enc, packed)
                for i, (g, r) in enumerate(zip(got, res)):
                    w = _want(r, enc)
                    assert len(w) == infer.resampled_length(len(batch[i]), RATE, rate)
                    assert g.dtype == w.dtype and len(g) == len(w), (rate, enc, b, i, packed, len(g), len(w))
                    assert np.array_equal(g, w), (rate, enc, b, i, packed, int(np.flatnonzero(g != w)[0]))


def test_identity_rate_encodes_without_resampling():
    batch = [_content(n, k % 3, k) for k, n in enumerate([4097, 1, 8192, 30011])]
    for enc in ENCODINGS:
        for packed in (True, False):
            for g, x in zip(_device(batch, RATE, enc, packed), batch):
                assert np.array_equal(g, _want(x, enc)), (enc, packed)


def test_a_request_does_not_depend_on_its_batch():
    for rate, enc in FORMATS:
        batch = _batches(rate)[4]
        together = _device(batch, rate, enc)
        for i in range(len(batch)):
            solo, = _device(batch[i:i + 1], rate, enc)
            assert solo.tobytes() == together[i].tobytes(), (rate, enc, i)


def test_one_launch_per_call_and_wave_finish_counters_stay():
    dev = torch.device("cuda:0")
    ops.wave_finish([torch.zeros(2 * F, device=dev)], [1], F, [False], RATE)
    before = (_counter("wave_finish_launches"), _counter("wave_finish_requests"))
    enc_before = (_counter("wave_encode_launches"), _counter("wave_encode_requests"))
    for k, idx in enumerate((0, 4)):                       # 1 request, 5 requests
        batch = _batches(22050)[idx]
        _device(batch, 22050, "alaw")
        assert _counter("wave_encode_launches") - enc_before[0] == k + 1
        assert _counter("wave_encode_requests") - enc_before[1] == (1, 6)[k]
    assert (_counter("wave_finish_launches"), _counter("wave_finish_requests")) == before


def _silence_requests():
    """The "pause" and "all quiet" constructions of tests/test_gpu_wave_backend.py, and a plain request of two chunks"""
    noise = lambda n, s, amp: (amp * np.random.default_rng(s).standard_normal(n)).astype(np.float32)   # noqa: E731
    plateau = (np.sign(np.random.default_rng(4).standard_normal(3 * RATE) + 1e-9) * (50 / 32768.0)).astype(np.float32)
    pause = np.concatenate([noise(2 * RATE, 1, 0.1), np.zeros(int(2.5 * RATE), np.float32), noise(2 * RATE, 2, 0.1)])
    return [[pause], [plateau], [noise(9003, 5, 0.3), noise(7201, 6, 0.3)]], [True, True, False]


@pytest.mark.parametrize("rate,enc", [(8000, "mulaw"), (44100, "pcm16"), (RATE, "alaw")])
def test_chained_behind_wave_finish_without_a_download(rate, enc):
    """wave_finish's packed PCM and its device lengths go straight into wave_encode: a flagged request's length never visits the host."""
    reqs, flags = _silence_requests()
    want = [infer.deliver_pcm16(p, rate, enc) for p in infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16")]
    assert len(want[1]) == 0 and 0 < len(want[0]) < infer.resampled_length(len(reqs[0][0]), RATE, rate)      # "all quiet", "pause"
    dev = torch.device("cuda:0")
    chunks = [torch.from_numpy(c).to(dev) for r in reqs for c in r]
    joined = [sum(len(c) for c in r) - (len(r) - 1) * F for r in reqs]
    pcm, lengths, offsets = ops.wave_finish(chunks, [len(r) for r in reqs], F, flags, RATE)
    data, out_len, out_off = ops.wave_encode(pcm, offsets, joined, lengths, rate, enc, _taps(rate))
    host, counts = data.cpu().numpy(), out_len.cpu().tolist()
    bps = 2 if enc == "pcm16" else 1
    for i, (o, m, w) in enumerate(zip(out_off, counts, want)):
        assert m == len(w), (i, m, len(w))
        assert host[o:o + m * bps].tobytes() == w.tobytes(), i


def test_ctypes_and_torch_op_paths_agree():
    batch = _batches(16000)[3]
    via_op = _device(batch, 16000, "mulaw")
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        for packed in (True, False):
            via_ctypes = _device(batch, 16000, "mulaw", packed)
            assert [a.tobytes() for a in via_ctypes] == [a.tobytes() for a in via_op]
    finally:
        torch_ops._loaded = True


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    pcm = torch.zeros(4096, device=dev, dtype=torch.int16)
    out = torch.zeros(65536, device=dev, dtype=torch.uint8)
    out_len = torch.zeros(4, device=dev, dtype=torch.int32)
    taps = _taps(8000)

    def call(max_len=(100,), out_off=(0,), n=None, rate=8000, enc=1, pcm_p=pcm.data_ptr(), taps_p=taps.data_ptr(), out_p=out.data_ptr(),
             in_p=True, ml_p=True, oo_p=True, ol_p=out_len.data_ptr()):
        ml, oo = np.asarray(max_len, dtype=np.int32), np.asarray(out_off, dtype=np.int64)
        io = np.zeros(len(ml), dtype=np.int64)
        p = lambda a, on: C.c_void_p(a.ctypes.data) if on else None   # noqa: E731
        return lib.f5hip_wave_encode(len(ml) if n is None else n, C.c_void_p(pcm_p), p(io, in_p), p(ml, ml_p), None, rate, enc, C.c_void_p(taps_p),
                                     C.c_void_p(out_p), p(oo, oo_p), C.c_void_p(ol_p), _lib.current_stream_ptr())

    _reset()
    assert call(n=0) != 0 and b"bad argument" in lib.f5hip_last_error()
    for null in (dict(pcm_p=None), dict(in_p=False), dict(ml_p=False), dict(out_p=None), dict(oo_p=False), dict(ol_p=None)):
        assert call(**null) != 0 and b"bad argument" in lib.f5hip_last_error(), null
    assert call(enc=3) != 0 and b"unknown encoding" in lib.f5hip_last_error() and call(enc=-1) != 0
    assert call(taps_p=None) != 0 and b"tap table" in lib.f5hip_last_error()
    assert call(out_off=(8,)) != 0 and b"multiple of 16" in lib.f5hip_last_error()
    assert call(out_p=out.data_ptr() + 8) != 0 and b"aligned" in lib.f5hip_last_error()
    assert call(max_len=(-1,)) != 0
    assert call(max_len=(2 ** 31 - 1, 2 ** 31 - 1), out_off=(0, 0)) != 0 and b"2^31" in lib.f5hip_last_error()            # in (refused unread)
    assert call(max_len=(2 ** 30 + 5,), rate=48000, taps_p=_taps(48000).data_ptr()) != 0 and b"2^31" in lib.f5hip_last_error()   # out
    with pytest.raises(_lib.F5HipError, match="encoding"):
        ops.wave_encode(pcm, [0], [100], None, 8000, "mp3", taps)
    with pytest.raises(_lib.F5HipError, match="taps"):
        ops.wave_encode(pcm, [0], [100], None, 8000, "mulaw", None)
    with pytest.raises(_lib.F5HipError):
        ops.wave_encode(pcm, [4000], [100], None, 8000, "mulaw", taps)                      # reads past the tensor
    with pytest.raises(_lib.F5HipError, match="does not fit"):                              # 320 : 147, a 204 KB table: more than the LDS holds
        ops.wave_encode(pcm, [0], [100], None, 11025, "pcm16", infer._device_taps(RATE, 11025, dev))
    with pytest.raises(RuntimeError, match="encoding"):
        torch.ops.f5hip.wave_encode([pcm], torch.zeros(1, dtype=torch.int64), torch.tensor([100], dtype=torch.int32), None, 8000, 3, taps)
    with pytest.raises(RuntimeError, match="tap table"):
        torch.ops.f5hip.wave_encode([pcm], torch.zeros(1, dtype=torch.int64), torch.tensor([100], dtype=torch.int32), None, 8000, 1, None)
    assert _counter("wave_encode_launches") == 0 and _counter("wave_encode_requests") == 0
    assert call() == 0 and _counter("wave_encode_launches") == 1 and _counter("wave_encode_requests") == 1
    torch.cuda.synchronize()


def test_finish_requests_groups_formats_and_counts_copies():
    """Mixed batch on the device path: one wave_encode call per distinct (rate, encoding), at most two copies per group, and the requests that
    set no format get exactly what they get without the others."""
    dev = torch.device("cuda:0")
    reqs, flags = _silence_requests()
    reqs = reqs + [reqs[2], reqs[0], reqs[2]]
    flags = flags + [False, True, False]
    rates = [8000, 8000, None, 44100, 8000, 24000]
    encs = ["mulaw", "mulaw", None, None, "mulaw", "pcm16"]
    on_dev = [[torch.from_numpy(c).to(dev) for c in r] for r in reqs]
    want = infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16", sample_rate=rates, encoding=encs)
    infer.backend_stats.clear()
    _reset()
    got = infer.finish_requests(on_dev, ["x"] * len(reqs), FADE_S, flags, device_backend=True, want="pcm16", sample_rate=rates, encoding=encs)
    stats = dict(infer.backend_stats)
    assert stats["device_requests"] == len(reqs) and stats["device_calls"] == 1 and stats.get("host_requests", 0) == 0
    assert stats["encode_calls"] == 2 and stats["encode_requests"] == 4 and _counter("wave_encode_launches") == 2
    assert stats["d2h_copies"] <= 2 * 3                    # the plain group, (8000, mulaw), (44100, pcm16)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), i
    plain = infer.finish_requests([on_dev[2], on_dev[5]], ["x", "x"], FADE_S, [False, False], device_backend=True, want="pcm16")
    assert np.array_equal(plain[0], got[2]) and np.array_equal(plain[1], got[5])


# ------------------------------------------------------------------------------------------------ end to end on a tiny model
@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


@pytest.mark.parametrize("micro_batch", [None, dict(span_steps=3)], ids=["direct", "continuous_batcher"])
def test_manager_bytes_do_not_depend_on_the_back_end(hip_objects, tmp_path, micro_batch):
    """`wav_bytes(synthesize(...))` with a fixed seed in three delivery formats, with and without `remove_silence`: byte-identical for
    device_backend on and off, one wave_encode launch per request with it on and none with it off."""
    path = _prompt(tmp_path)
    out = {}
    for backend in (False, True):
        mgr = serve.TTSManager(nfe_step=8, micro_batch=micro_batch, device_backend=backend).load(*hip_objects)
        try:
            for rate, enc in FORMATS:
                for cut in (False, True):
                    _reset()
                    infer.backend_stats.clear()
                    wave = mgr.synthesize(TEXT, ref_audio_path=path, ref_text=REF_TEXT, seed=7, remove_silence=cut, sample_rate=rate, encoding=enc)
                    assert wave.dtype == (np.int16 if enc == "pcm16" else np.uint8)
                    assert _counter("wave_encode_launches") == (1 if backend else 0), (backend, rate, enc, cut)
                    if backend:
                        assert infer.backend_stats["d2h_copies"] <= 2 and infer.backend_stats["encode_requests"] == 1
                    out[backend, rate, enc, cut] = serve.wav_bytes(wave, rate, enc).getvalue()
            if backend and micro_batch is None:            # a mixed batch: one call per format, at most two copies per group
                voice, ref_text_n = mgr._voice(path, REF_TEXT)
                opts = [dict(seed=7, sample_rate=8000, encoding="mulaw"), dict(seed=7), dict(seed=7, sample_rate=8000, encoding="mulaw", remove_silence=True),
                        dict(seed=7, sample_rate=48000, encoding="alaw")]
                _reset()
                infer.backend_stats.clear()
                res = mgr._run_batch([(voice, ref_text_n, TEXT, o) for o in opts])
                assert _counter("wave_encode_launches") == 2 and infer.backend_stats["d2h_copies"] <= 2 * 3
                assert serve.wav_bytes(res[0], 8000, "mulaw").getvalue() == out[True, 8000, "mulaw", False]
                assert serve.wav_bytes(res[2], 8000, "mulaw").getvalue() == out[True, 8000, "mulaw", True]
                assert serve.wav_bytes(res[3], 48000, "alaw").getvalue() == out[True, 48000, "alaw", False]
                assert res[1].dtype == np.int16
        finally:
            mgr.close()
    for rate, enc in FORMATS:
        for cut in (False, True):
            assert out[True, rate, enc, cut] == out[False, rate, enc, cut], (rate, enc, cut)
        assert len(out[True, rate, enc, True]) <= len(out[True, rate, enc, False])
