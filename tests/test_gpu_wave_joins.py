"""The segment-aware join on the device (csrc/wave_out.h, f5hip_wave_finish_joins: a request's chunks cross-fade inside a segment and butt
between segments -- a multi-voice script) against the host definition `infer.join_segments` + `infer.quantise_pcm16`
(+ `audio_prep.remove_silence_pcm`), alone, chained into `ops.wave_encode`, and through `infer.finish_requests`.

Every comparison is `np.array_equal` on int16 samples / code bytes and lengths: there is no tolerance anywhere.

Layout (iii) is the one the slow path's chunk walk exists for: single-chunk segments of 1, 2, 3, 1 and 5 samples between two long ones.  With
those lengths an 8-sample group covers at most five chunks (six would need four whole chunks inside six samples; 1 + 2 + 3 + 1 = 7), so the
first long chunk is run at all eight lengths mod 8: every alignment of the short chunks against the groups, the five-chunk ones included."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, ops, torch_ops  # noqa: E402

RATE = 24000
FADE_S = infer.cross_fade_duration
F = int(FADE_S * RATE)                                   # 3600
TILE = 3840                                              # joined samples per block of the join kernel


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _content(n, kind, seed):
    """float32 chunk: noise at 0.3, zeros, or the full-scale square wave +1, -1, ... (32767, -32768 once quantised)"""
    if kind == 0:
        return (0.3 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)
    if kind == 1:
        return np.zeros(n, dtype=np.float32)
    return np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)


def _layouts():
    """[request] with request = [segment] and segment = [chunk length | ("z", length): a gap, a chunk of zeros whatever the turn]"""
    out = [[[7200, 7201, 9003]]]                                                                  # (i) one segment: wave_finish itself
    for j in (7200, 7201, 7207, TILE - 1, TILE, TILE + 1):                                        # (ii) 2 + 1 chunks, the butt join at joined sample j
        a = F if j < 2 * F else 2 * F
        out.append([[a, j + F - a], [5000]])
    for r in range(8):                                                                            # (iii) see the module docstring
        out.append([[4000 + r], [1], [2], [3], [1], [5], [4100]])
    out.append([[4000, F], [4001]])                                                               # (iv) a fading chunk of exactly F, successor butts
    out.append([[F, 2 * F, F + 3]])                                                               #      exactly 2 F between two fades (and F, first)
    out.append([[4003], [("z", 1)], [4005]])                                                      # (v) zero gaps of 1 and of 12 000 samples
    out.append([[7200, 7300], [("z", 12000)], [3700, 3600]])
    out.append([[1]])                                                                             # (vi) a single one-sample request
    return out


def _requests(turn):
    """The layouts with content: `turn` True deals noise / zeros / square wave over the chunks in turn, False is noise everywhere"""
    reqs, k = [], 0
    for layout in _layouts():
        segs = []
        for seg in layout:
            chunks = []
            for n in seg:
                gap = isinstance(n, tuple)
                chunks.append(_content(n[1] if gap else n, 1 if gap else (k % 3 if turn else 0), 7000 + k))
                k += 1
            segs.append(chunks)
        reqs.append(segs)
    return reqs


def _calls():
    """The 20 requests of each turn dealt into calls of 1, 2, 3, 4, 5 and 5 requests: [[request]]"""
    out = []
    for turn in (True, False):
        reqs, k = _requests(turn), 0
        for size in (1, 2, 3, 4, 5, 5):
            out.append(reqs[k:k + size])
            k += size
        assert k == len(reqs)
    return out


def _host(segs, flag=False):
    pcm = infer.quantise_pcm16(infer.join_segments(segs, FADE_S))
    return infer.remove_silence_pcm(pcm, RATE) if flag else pcm


@pytest.fixture(scope="module")
def host_results():
    """The host definition of every request of every call, computed once and shared"""
    return [[_host(segs) for segs in call] for call in _calls()]


def _flat(reqs):
    chunks = [c for segs in reqs for seg in segs for c in seg]
    fades = [i > 0 for segs in reqs for seg in segs for i in range(len(seg))]
    return chunks, [sum(len(seg) for seg in segs) for segs in reqs], fades


def _device(reqs, flags=None, packed=True, fades="own", raw=False):
    """ops.wave_finish_joins on device copies of the chunk waves -> [int16 numpy per request].  `packed`: the chunks are views of ONE buffer, back
    to back like `decode_ragged` leaves them; else separate allocations."""
    dev = torch.device("cuda:0")
    flat, counts, own = _flat(reqs)
    if packed:
        chunks = list(torch.from_numpy(np.concatenate(flat)).to(dev).split([len(c) for c in flat]))
    else:
        chunks = [torch.from_numpy(c).to(dev) for c in flat]
    pcm, lengths, offsets = ops.wave_finish_joins(chunks, counts, F, own if fades == "own" else fades, flags, RATE)
    assert pcm.dtype == torch.int16 and lengths.dtype == torch.int32 and all(o % 8 == 0 for o in offsets)
    if raw:
        return pcm, lengths, offsets
    host, lengths = pcm.cpu().numpy(), lengths.cpu().tolist()
    return [host[o:o + n].copy() for o, n in zip(offsets, lengths)]


def test_kernel_equals_join_segments_bit_for_bit(host_results):
    for b, (call, want) in enumerate(zip(_calls(), host_results)):
        for packed in (True, False):
            got = _device(call, packed=packed)
            for i, (g, w, segs) in enumerate(zip(got, want, call)):
                n = sum(len(c) for seg in segs for c in seg) - F * sum(len(seg) - 1 for seg in segs)
                assert w.dtype == np.int16 and len(g) == len(w) == n, (b, i, packed, len(g), len(w), n)
                assert np.array_equal(g, w), (b, i, packed, int(np.flatnonzero(g != w)[0]))


def test_one_segment_is_wave_finish_and_null_chunk_fade_is_wave_finish():
    dev = torch.device("cuda:0")
    reqs = [_requests(False)[0], [[_content(7200, 0, 1), _content(9000, 2, 2)]], [[_content(5, 0, 3)]]]      # one segment each
    flat, counts, _ = _flat(reqs)
    chunks = [torch.from_numpy(c).to(dev) for c in flat]
    _reset()
    pcm0, len0, off0 = ops.wave_finish(chunks, counts, F, None, RATE)
    assert _counter("wave_finish_launches") == 1 and _counter("wave_finish_requests") == 3
    _reset()
    pcm1, len1, off1 = ops.wave_finish_joins(chunks, counts, F, None, None, RATE)                             # chunk_fade == NULL
    assert _counter("wave_finish_launches") == 1 and _counter("wave_finish_requests") == 3
    _reset()
    pcm2, len2, off2 = _device(reqs, packed=False, raw=True)                                                  # every later chunk fades
    assert _counter("wave_finish_launches") == 1 and _counter("wave_finish_requests") == 3
    assert off0 == off1 == off2 and torch.equal(len0, len1) and torch.equal(len0, len2)
    for o, n in zip(off0, len0.cpu().tolist()):
        assert torch.equal(pcm0[o:o + n], pcm1[o:o + n]) and torch.equal(pcm0[o:o + n], pcm2[o:o + n])
    # the flagged launches: three, as wave_finish's
    _reset()
    ops.wave_finish_joins(chunks, counts, F, None, [True, False, True], RATE)
    assert _counter("wave_finish_launches") == 3


def _pause_script():
    """The "pause" construction of tests/test_gpu_wave_backend.py (2 s of noise, 2.5 s of zeros, 2 s of noise) split into two segments inside
    the pause, the first of two chunks"""
    noise = lambda n, s: (0.1 * np.random.default_rng(s).standard_normal(n)).astype(np.float32)   # noqa: E731
    return [[noise(RATE, 1), np.concatenate([noise(RATE + F, 2), np.zeros(30000, np.float32)])], [np.concatenate([np.zeros(30000, np.float32), noise(2 * RATE, 3)])]]


def test_flagged_script_and_the_chain_into_wave_encode():
    script, plain = _pause_script(), _requests(False)[1]
    reqs, flags = [script, plain, script], [True, False, False]
    want = [_host(segs, f) for segs, f in zip(reqs, flags)]
    assert len(want[2]) - len(want[0]) == 24 * 1500                                # the 2.5 s pause shrinks to 2 x 500 ms
    _reset()
    got = _device(reqs, flags)
    assert _counter("wave_finish_launches") == 3 and _counter("wave_finish_requests") == 3
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) and np.array_equal(g, w), i
    # chained into wave_encode at (8000, "mulaw"): the flagged request's length never visits the host
    pcm, lengths, offsets = _device(reqs, flags, raw=True)
    joined = [sum(len(c) for seg in segs for c in seg) - F * sum(len(seg) - 1 for seg in segs) for segs in reqs]
    data, out_len, out_off = ops.wave_encode(pcm, offsets, joined, lengths, 8000, "mulaw", infer._device_taps(RATE, 8000, pcm.device))
    host, counts = data.cpu().numpy(), out_len.cpu().tolist()
    for i, (o, m, w) in enumerate(zip(out_off, counts, want)):
        enc = infer.deliver_pcm16(w, 8000, "mulaw")
        assert m == len(enc) and host[o:o + m].tobytes() == enc.tobytes(), i


def test_a_request_does_not_depend_on_its_call():
    call = _calls()[4]                                                             # five requests, mixed content
    together = _device(call)
    for i in range(len(call)):
        solo, = _device(call[i:i + 1])
        assert solo.tobytes() == together[i].tobytes(), i
        moved, = _device(call[i:i + 1], packed=False)
        assert moved.tobytes() == together[i].tobytes(), i
    reqs, flags = [_pause_script(), call[0], _pause_script()], [True, False, True]
    both = _device(reqs, flags)
    solo, = _device(reqs[:1], flags[:1])
    assert solo.tobytes() == both[0].tobytes() == both[2].tobytes()


def test_ctypes_and_torch_op_paths_agree():
    call = _calls()[5]
    via_op = _device(call)
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        for packed in (True, False):
            via_ctypes = _device(call, packed=packed)
            assert [a.tobytes() for a in via_ctypes] == [a.tobytes() for a in via_op]
    finally:
        torch_ops._loaded = True
    flat, counts, fades = _flat(call)
    dev = torch.device("cuda:0")
    pcm, lengths = torch.ops.f5hip.wave_finish_joins([torch.from_numpy(c).to(dev) for c in flat], torch.tensor(counts, dtype=torch.int32), F,
                                                     torch.tensor(fades, dtype=torch.uint8), torch.zeros(len(call), dtype=torch.uint8), RATE)
    host, off = pcm.cpu().numpy(), 0
    for n, w in zip(lengths.cpu().tolist(), via_op):
        assert host[off:off + n].tobytes() == w.tobytes()
        off += (n + 7) & ~7


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    wave = torch.zeros(6 * F, device=dev)
    pcm, lens_dev = torch.zeros(16 * F, device=dev, dtype=torch.int16), torch.zeros(4, device=dev, dtype=torch.int32)

    def call(k, chunk_len, fades, fade=F, rate=RATE, n=None, ptr=None):
        k, cl, cf = np.asarray(k, dtype=np.int32), np.asarray(chunk_len, dtype=np.int32), np.asarray(fades, dtype=np.uint8)
        ptrs = np.full(len(cl), wave.data_ptr() if ptr is None else ptr, dtype=np.uint64)
        flags = np.zeros(len(k), dtype=np.uint8)
        return lib.f5hip_wave_finish_joins(len(k) if n is None else n, C.c_void_p(k.ctypes.data), C.c_void_p(ptrs.ctypes.data), C.c_void_p(cl.ctypes.data),
                                           fade, C.c_void_p(cf.ctypes.data), C.c_void_p(flags.ctypes.data), rate, C.c_void_p(pcm.data_ptr()),
                                           C.c_void_p(lens_dev.data_ptr()), _lib.current_stream_ptr())

    _reset()
    assert call([3], [F, 2 * F - 1, F], [0, 1, 1]) != 0 and b"fewer than its fades" in lib.f5hip_last_error()   # fades in and out: needs 2 F
    assert call([2], [F - 1, F], [0, 1]) != 0 and b"fewer than its fades" in lib.f5hip_last_error()             # fades out only: needs F
    assert call([3], [F, F - 1, F], [0, 1, 0]) != 0 and b"fewer than its fades" in lib.f5hip_last_error()       # fades in, successor butts: needs F
    assert call([2, 2], [F, F, F, F - 1], [0, 0, 0, 1]) != 0 and b"request 1" in lib.f5hip_last_error()         # the second request's last chunk
    assert call([2], [F, 0], [0, 0]) != 0 and b"empty" in lib.f5hip_last_error()                                # what wave_finish refuses
    assert call([2], [F, F], [0, 0], fade=-1) != 0 and call([1], [F], [0], rate=22050) != 0 and call([1], [F], [0], n=0) != 0 and call([0], [], []) != 0
    assert call([1, 1], [2 ** 31 - 1, 2 ** 31 - 1], [0, 0]) != 0 and b"2^31" in lib.f5hip_last_error()
    assert call([1], [F], [0], ptr=0) != 0
    with pytest.raises(_lib.F5HipError, match="fewer than its fades"):
        ops.wave_finish_joins([wave[:F], wave[F:3 * F - 1], wave[3 * F:4 * F]], [3], F, [False, True, True], None, RATE)
    with pytest.raises(_lib.F5HipError, match="one value per chunk"):
        ops.wave_finish_joins([wave[:F], wave[F:3 * F]], [2], F, [False], None, RATE)
    with pytest.raises(_lib.F5HipError, match="24000"):
        ops.wave_finish_joins([wave[:F]], [1], F, [False], None, 16000)
    with pytest.raises(RuntimeError, match="fewer than its fades"):
        torch.ops.f5hip.wave_finish_joins([wave[:F - 1], wave[F:2 * F]], torch.tensor([2], dtype=torch.int32), F, torch.tensor([0, 1], dtype=torch.uint8),
                                          torch.zeros(1, dtype=torch.uint8), RATE)
    with pytest.raises(RuntimeError, match="one value per chunk"):
        torch.ops.f5hip.wave_finish_joins([wave[:F]], torch.tensor([1], dtype=torch.int32), F, torch.zeros(2, dtype=torch.uint8),
                                          torch.zeros(1, dtype=torch.uint8), RATE)
    assert _counter("wave_finish_launches") == 0 and _counter("wave_finish_requests") == 0
    # what the 2 F rule refuses and this one takes: butt-joined chunks shorter than the fade, with the fade set
    assert call([3], [5, 1, F - 1], [0, 0, 0]) == 0 and _counter("wave_finish_launches") == 1 and _counter("wave_finish_requests") == 1
    torch.cuda.synchronize()


def test_finish_requests_takes_a_script_in_the_batch_s_one_call():
    """A script (with a gap) between plain requests: one device call for all of them and at most two copies; a script with a chunk shorter than
    its fades is finished on the host in the same call.  Each request gets the host definition's samples."""
    dev = torch.device("cuda:0")
    on_dev = lambda segs: [[torch.from_numpy(c).to(dev) for c in seg] for seg in segs]   # noqa: E731
    plain = [_content(7200, 0, 1), _content(9003, 0, 2)]
    script = [[_content(8000, 0, 3), _content(7300, 0, 4)], [_content(50, 2, 5)], [_content(7201, 0, 6)]]
    short = [[_content(8000, 0, 7), _content(F - 1, 0, 8)], [_content(4000, 0, 9)]]
    waves = [[torch.from_numpy(c).to(dev) for c in plain], infer.SegmentedWaves(on_dev(script), 4801), infer.SegmentedWaves(on_dev(_pause_script())),
             infer.SegmentedWaves(on_dev(short), 7)]
    host = [plain, infer.SegmentedWaves(script, 4801), infer.SegmentedWaves(_pause_script()), infer.SegmentedWaves(short, 7)]
    flags, rates, encs = [False, False, True, False], [None, None, 8000, None], [None, None, "mulaw", None]
    want = infer.finish_requests(host, ["x"] * 4, FADE_S, flags, want="pcm16", sample_rate=rates, encoding=encs)
    z = np.zeros(4801, dtype=np.float32)
    assert np.array_equal(want[1], infer.quantise_pcm16(np.concatenate([infer.cross_fade_concat(script[0], FADE_S), z, script[1][0], z, script[2][0]])))
    infer.backend_stats.clear()
    _reset()
    got = infer.finish_requests(waves, ["x"] * 4, FADE_S, flags, device_backend=True, want="pcm16", sample_rate=rates, encoding=encs)
    stats = dict(infer.backend_stats)
    assert stats["device_calls"] == 1 and stats["device_requests"] == 3 and stats["host_requests"] == 1 and stats["encode_calls"] == 1
    assert _counter("wave_finish_launches") == 3 and _counter("wave_finish_requests") == 3 and _counter("wave_encode_launches") == 1
    assert stats["d2h_copies"] <= 2 * 2 + 3                # two format groups; the short script's three chunks come down for the host
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), i
