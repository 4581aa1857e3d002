"""The waveform back-end on the device (csrc/wave_out.h, f5hip_wave_finish: cross-fade join, int16 quantisation and silence removal of a
ragged batch of requests in one call) against the host path `infer.finish_requests` -- the project's existing numpy arithmetic plus
`audio_prep.remove_silence_pcm` -- and `TTSManager(device_backend=True)` end to end on a tiny model.

Every comparison is `np.array_equal` on int16 samples and lengths, or equality of WAV bytes: there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, ops, serve, synth  # noqa: E402

from test_gpu_request_knobs import ARCH, REF_TEXT, TEXT, VOCAB, _prompt  # noqa: E402

RATE = 24000
FADE_S = infer.cross_fade_duration
F = int(FADE_S * RATE)                                   # 3600: a chunk of 7200 samples is exactly 2 F
LAUNCHES = {False: 1, True: 3}                           # per call: the join alone, or join + silence + compaction


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _noise(n, seed, amp=0.3):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _plateau(n, level, seed):
    """float32 samples that quantise to +-level exactly (level / 32768 is a float32)"""
    return (np.sign(np.random.default_rng(seed).standard_normal(n) + 1e-9) * (level / 32768.0)).astype(np.float32)


def _silence_cases():
    """The CPU list (tests/test_wave_backend_host.py) as float chunk waves: [(chunks, name)]"""
    loud = lambda n, s: _noise(n, s, 0.1)   # noqa: E731
    cases = [([np.concatenate([loud(2 * RATE, 1), np.zeros(int(2.5 * RATE), np.float32), loud(2 * RATE, 2)])], "pause"),
             ([loud(24 * 3000 + 5, 3)], "no pause"),
             ([_plateau(3 * RATE, 50, 4)], "all quiet"),
             ([_plateau(RATE // 2, 50, 5)], "under 1 s"),
             ([np.concatenate([loud(2 * RATE, 6), _plateau(int(2.5 * RATE), 103, 7), loud(2 * RATE, 8)])], "plateau 103"),
             ([np.concatenate([loud(2 * RATE, 9), _plateau(int(2.5 * RATE), 104, 10), loud(2 * RATE, 11)])], "plateau 104"),
             # silent head and tail, N mod 24 == 12 with odd and even whole milliseconds, (len_ms - 1000) % 10 == 8
             ([np.concatenate([np.zeros(30000, np.float32), loud(24 * 3001 + 12 - 60000, 12), np.zeros(30000, np.float32)])], "edges, odd half"),
             ([np.concatenate([loud(30000, 13), np.zeros(24 * 3000 + 12 - 60000, np.float32), loud(30000, 14)])], "even half"),
             ([np.concatenate([loud(40000, 15), _plateau(26000, 60, 16), loud(24 * 4007 + 13 - 66000 - 25000, 17), np.zeros(25000, np.float32)])], "unaligned last"),
             # pauses inside and across the chunks of a request that is joined first
             ([np.concatenate([loud(20000, 18), np.zeros(30000, np.float32)]), np.concatenate([np.zeros(9000, np.float32), loud(21011, 19)]),
               np.concatenate([loud(8000, 20), _plateau(40000, 103, 21), loud(9001, 22)])], "three chunks")]
    return cases


def _batches():
    """[(requests = [[chunk, ...]], flags)]: 1 to 5 requests of 1 to 4 chunks; lengths 2 F, 2 F + 1, 9 000 + r and about 30 000"""
    lens = [[7200], [7200, 7201], [9003, 7200, 30011], [30000, 9017, 7201, 7200], [29989, 9001]]
    plain = [[_noise(n, 100 * i + j) for j, n in enumerate(ls)] for i, ls in enumerate(lens)]
    sil = [c for c, _ in _silence_cases()]
    return [(plain[:1], [False]), (plain[3:4], [True]), (plain, [False] * 5), (plain, [True, False, True, False, True]),
            (sil[:5], [True] * 5), (sil[5:], [True] * 5), ([sil[0], plain[2], sil[9], plain[1]], [True, False, True, True]),
            ([sil[0], sil[4], sil[9]], [False, False, False])]


@pytest.fixture(scope="module")
def host_results():
    """The host path's int16 PCM of every batch, computed once and shared"""
    return [infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16") for reqs, flags in _batches()]


def _device(reqs, flags, packed=True):
    """ops.wave_finish on device copies of the chunk waves -> [int16 numpy per request].  `packed`: the chunks are views of ONE buffer, back to
    back like `decode_ragged` leaves them (odd lengths then shift the later chunks off 16-byte alignment); else separate allocations."""
    dev = torch.device("cuda:0")
    flat = [c for r in reqs for c in r]
    if packed:
        chunks = list(torch.from_numpy(np.concatenate(flat)).to(dev).split([len(c) for c in flat]))
    else:
        chunks = [torch.from_numpy(c).to(dev) for c in flat]
    pcm, lengths, offsets = ops.wave_finish(chunks, [len(r) for r in reqs], F, flags, RATE)
    assert pcm.dtype == torch.int16 and lengths.dtype == torch.int32
    host, lengths = pcm.cpu().numpy(), lengths.cpu().tolist()
    return [host[o:o + n].copy() for o, n in zip(offsets, lengths)]


def test_kernel_equals_the_host_path_bit_for_bit(host_results):
    for b, ((reqs, flags), want) in enumerate(zip(_batches(), host_results)):
        for packed in (True, False):
            got = _device(reqs, flags, packed)
            for i, (g, w) in enumerate(zip(got, want)):
                assert w.dtype == np.int16 and len(g) == len(w), (b, i, packed, len(g), len(w))
                assert np.array_equal(g, w), (b, i, packed, int(np.flatnonzero(g != w)[0]))


def test_silence_cases_do_what_their_names_say(host_results):
    """The host results the kernel was held to are the known answers, not merely something both sides agree on."""
    cases, (a, b) = _silence_cases(), host_results[4:6]
    got = dict(zip([name for _, name in cases], a + b))
    n = {name: sum(len(c) for c in chunks) - (len(chunks) - 1) * F for chunks, name in cases}
    assert n["pause"] - len(got["pause"]) == 24 * 1500 and len(got["no pause"]) == 24 * 3000
    assert len(got["all quiet"]) == 0 and len(got["under 1 s"]) == n["under 1 s"]
    assert n["plateau 103"] - len(got["plateau 103"]) == 24 * 1500 and len(got["plateau 104"]) == n["plateau 104"]
    assert 0 < len(got["three chunks"]) < n["three chunks"] and 0 < len(got["unaligned last"]) < n["unaligned last"]


def test_a_request_does_not_depend_on_its_batch(host_results):
    reqs, flags = _batches()[3]
    batch = _device(reqs, flags)
    for i in range(len(reqs)):
        solo, = _device(reqs[i:i + 1], flags[i:i + 1])
        assert solo.tobytes() == batch[i].tobytes(), i
    sreqs, sflags = _batches()[6]
    batch = _device(sreqs, sflags)
    for i in (0, 2):
        solo, = _device(sreqs[i:i + 1], sflags[i:i + 1])
        assert solo.tobytes() == batch[i].tobytes(), i


def test_launches_per_call_do_not_depend_on_the_batch():
    for idx in (0, 2, 1, 3):                              # 1 and 5 requests without a flag, 1 and 5 requests with flags
        reqs, flags = _batches()[idx]
        _reset()
        _device(reqs, flags)
        assert _counter("wave_finish_launches") == LAUNCHES[any(flags)], (idx, flags)
        assert _counter("wave_finish_requests") == len(reqs)


def test_plain_concatenation_with_fade_0():
    reqs = [[_noise(5000, 1), _noise(101, 2), _noise(7, 3)], [_noise(9000, 4)]]
    dev = torch.device("cuda:0")
    pcm, lengths, offsets = ops.wave_finish([torch.from_numpy(c).to(dev) for r in reqs for c in r], [3, 1], 0, [False, False], RATE)
    host, lengths = pcm.cpu().numpy(), lengths.cpu().tolist()
    want = infer.finish_requests(reqs, ["x", "y"], 0, want="pcm16")
    for o, n, w in zip(offsets, lengths, want):
        assert np.array_equal(host[o:o + n], w)


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    wave = torch.zeros(4 * F, device=dev)
    pcm, lens_dev = torch.zeros(8 * F, device=dev, dtype=torch.int16), torch.zeros(4, device=dev, dtype=torch.int32)

    def call(k, chunk_len, fade, rate, n=None, ptr=None):
        k, cl = np.asarray(k, dtype=np.int32), np.asarray(chunk_len, dtype=np.int32)
        ptrs = np.full(len(cl), wave.data_ptr() if ptr is None else ptr, dtype=np.uint64)
        flags = np.zeros(len(k), dtype=np.uint8)
        return lib.f5hip_wave_finish(len(k) if n is None else n, C.c_void_p(k.ctypes.data), C.c_void_p(ptrs.ctypes.data), C.c_void_p(cl.ctypes.data), fade,
                                     C.c_void_p(flags.ctypes.data), rate, C.c_void_p(pcm.data_ptr()), C.c_void_p(lens_dev.data_ptr()), _lib.current_stream_ptr())

    _reset()
    assert call([2], [2 * F, 2 * F - 1], F, RATE) != 0 and b"2 x fade" in lib.f5hip_last_error()      # a chunk shorter than 2 F, several chunks
    assert call([2], [2 * F, 2 * F], -1, RATE) != 0                                                    # a negative fade
    assert call([1], [2 * F], F, 22050) != 0 and b"24000" in lib.f5hip_last_error()                    # another rate
    assert call([1, 1], [2 ** 31 - 1, 2 ** 31 - 1], F, RATE) != 0 and b"2^31" in lib.f5hip_last_error()   # totals beyond 2^31 - 1 (refused unread)
    assert call([1], [2 * F], F, RATE, n=0) != 0 and call([0], [], F, RATE) != 0 and call([1], [0], F, RATE) != 0
    with pytest.raises(_lib.F5HipError, match="2 x fade"):
        ops.wave_finish([wave[:2 * F], wave[2 * F:4 * F - 1]], [2], F, [False], RATE)
    with pytest.raises(_lib.F5HipError, match="24000"):
        ops.wave_finish([wave[:2 * F]], [1], F, [False], 16000)
    with pytest.raises(_lib.F5HipError):
        ops.wave_finish([wave[:2 * F]], [1], -3, [False], RATE)
    with pytest.raises(RuntimeError, match="2 x fade"):
        torch.ops.f5hip.wave_finish([wave[:2 * F], wave[2 * F:4 * F - 1]], torch.tensor([2], dtype=torch.int32), F, torch.zeros(1, dtype=torch.uint8), RATE)
    assert _counter("wave_finish_launches") == 0 and _counter("wave_finish_requests") == 0
    assert call([1], [F], F, RATE) == 0 and _counter("wave_finish_launches") == 1                      # one short chunk alone is fine: nothing to fade
    torch.cuda.synchronize()


def test_finish_requests_device_path_counts_and_falls_back(host_results):
    """One call and at most two downloads for the eligible requests; a request with a chunk below 2 F and a list text take the host path."""
    dev = torch.device("cuda:0")
    reqs, flags = _batches()[3]
    short = [_noise(3 * F, 50), _noise(F + 100, 51), _noise(3 * F, 52)]
    head = [_noise(8000, 53)]
    all_reqs = [[torch.from_numpy(c).to(dev) for c in r] for r in reqs + [short, head]]
    texts, all_flags = ["x"] * len(reqs) + ["y", ["head"]], flags + [True, False]
    infer.backend_stats.clear()
    _reset()
    got = infer.finish_requests(all_reqs, texts, FADE_S, all_flags, device_backend=True, want="pcm16")
    stats = dict(infer.backend_stats)
    assert stats["device_requests"] == len(reqs) and stats["host_requests"] == 2 and stats["device_calls"] == 1
    assert stats["d2h_copies"] == 2 + 3 + 1               # lengths + samples; the short request's three chunks and the head's one
    assert _counter("wave_finish_launches") == 3
    for g, w in zip(got[:len(reqs)], host_results[3]):
        assert np.array_equal(g, w)
    want_short, = infer.finish_requests([short], ["y"], FADE_S, [True], want="pcm16")
    assert np.array_equal(got[len(reqs)], want_short) and np.array_equal(got[-1][0], head[0])
    infer.backend_stats.clear()
    infer.finish_requests(all_reqs[:2], texts[:2], FADE_S, [False, False], device_backend=True, want="pcm16")
    assert infer.backend_stats["d2h_copies"] == 1         # without silence removal the lengths are known: the samples only


# ------------------------------------------------------------------------------------------------ end to end on a tiny model
@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


@pytest.mark.parametrize("micro_batch", [None, dict(max_requests=4, max_wait_ms=2.0), dict(span_steps=3)], ids=["direct", "micro_batcher", "span_steps"])
def test_manager_bytes_do_not_depend_on_the_back_end(hip_objects, tmp_path, micro_batch):
    """`wav_bytes(synthesize(...))` with a fixed seed, with and without `remove_silence`: byte-identical for device_backend on and off; the
    library's launch counter grows by the fixed number per batch with the back-end on and stays put with it off."""
    path = _prompt(tmp_path)
    texts = [TEXT, "Always remember, I endure."]           # several chunks, one chunk
    out = {}
    for backend in (False, True):
        mgr = serve.TTSManager(nfe_step=8, micro_batch=micro_batch, device_backend=backend).load(*hip_objects)
        try:
            for text in texts:
                for cut in (False, True):
                    _reset()
                    infer.backend_stats.clear()
                    wave = mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, seed=7, remove_silence=cut)
                    assert wave.dtype == (np.int16 if backend or cut else np.float32)
                    assert _counter("wave_finish_launches") == (LAUNCHES[cut] if backend else 0), (backend, text[:12], cut)
                    assert infer.backend_stats["device_requests"] == (1 if backend else 0)
                    out[backend, text, cut] = serve.wav_bytes(wave).getvalue()
        finally:
            mgr.close()
    for text in texts:
        for cut in (False, True):
            assert out[True, text, cut] == out[False, text, cut], (text[:12], cut)
        assert len(out[True, text, True]) <= len(out[True, text, False])
