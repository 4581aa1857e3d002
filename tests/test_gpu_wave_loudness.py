"""The loudness target on the device (csrc/wave_out.h, f5hip_wave_loudness: the 24 kHz int16 PCM of a ragged batch of requests, normalised
in place to each flagged request's BS.1770 target in three launches) against the host definition `infer.measure_loudness` /
`infer.normalise_loudness_pcm16`, alone, chained between `ops.wave_finish` and `ops.wave_encode` / `ops.wave_flac`, and through
`infer_requests` with the device back-end on a tiny model.

Every comparison is equality of bytes and of the stats integers: there is no tolerance anywhere."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, ops, serve, synth, torch_ops  # noqa: E402

from test_gpu_request_knobs import ARCH, REF_TEXT, TEXT, VOCAB, _prompt  # noqa: E402

RATE = 24000
T = infer.LOUDNESS_TAPS
TILE = 4800                                            # f5hip_wave_loudness_tile(): checked below
FADE_S = infer.cross_fade_duration
LENGTHS = [0, 1, 2399, 2400, 9599, 9600, 9601, 11999, 12000, T - 1, T, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 30011, 5 * RATE]
SIZES = (1, 2, 3, 4, 5, 2)                             # the 17 lengths dealt into batches
TARGETS = [-16.0, None, -23.0, -30.0, -5.0, -40.0, -26.0]
FILLER = 23456
_host_cache = {}


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _sine(n, freq, db):
    return np.clip(np.rint(10.0 ** (db / 20.0) * 32768.0 * np.sin(2 * np.pi * freq * np.arange(n) / RATE)), -32768, 32767).astype(np.int16)


def _content(n, kind, seed):
    """The eight contents: zeros, a constant, the alternating full-scale square (the accumulator's worst case), sines at -6, -30 and -60
    dBFS, noise, a loud burst in silence."""
    rng = np.random.default_rng(seed)

    def burst():
        x = np.zeros(n, dtype=np.int16)
        a, b = n // 3, max(2 * n // 3, n // 3 + 1)
        x[a:b] = infer.quantise_pcm16(0.5 * rng.standard_normal(b - a))[:len(x[a:b])]
        return x
    return [lambda: np.zeros(n, dtype=np.int16),
            lambda: np.full(n, 1234, dtype=np.int16),
            lambda: np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16),
            lambda: _sine(n, 997, -6.0),
            lambda: _sine(n, 440, -30.0),
            lambda: _sine(n, 1500, -60.0),
            lambda: infer.quantise_pcm16(0.05 * rng.standard_normal(n)),
            burst][kind % 8]()


def _batches(turn):
    """The 17 lengths dealt into batches of 1 to 5 requests; request j of the deal takes content (j + turn) mod 8 and target (j + turn) mod 7
    (one of them None: unflagged)."""
    out, k = [], 0
    for size in SIZES:
        out.append([(_content(n, k + j + turn, 100 * turn + k + j), TARGETS[(k + j + turn) % len(TARGETS)]) for j, n in enumerate(LENGTHS[k:k + size])])
        k += size
    return out


def _bits(g):
    return struct.unpack("<q", struct.pack("<d", g))[0]


def _host(x, target):
    """(normalised PCM, stats row) by the host definition; cached: several tests meet the same request."""
    key = (x.tobytes(), target)
    if key not in _host_cache:
        if target is None:
            _host_cache[key] = (x, (0, 0, 0, 0))
        else:
            n2, S2, peak = infer.measure_loudness(x)
            g = infer.loudness_gain(n2, S2, peak, infer.loudness_gain_constant(target))
            _host_cache[key] = (infer.normalise_loudness_pcm16(x, target), (n2, S2, peak, _bits(g)))
    return _host_cache[key]


def _device(batch, cut=None):
    """ops.wave_loudness on ONE packed buffer with the requests at `wave_finish`'s 8-sample offsets and a loud filler between them ->
    (the whole buffer afterwards, its offsets, the stats rows).  `cut`: the actual lengths, on the device alone."""
    dev = torch.device("cuda:0")
    offsets, off = [], 0
    for x, _ in batch:
        offsets.append(off)
        off += (len(x) + 7) & ~7
    buf = np.full(off + 8, FILLER, dtype=np.int16)
    for o, (x, _) in zip(offsets, batch):
        buf[o:o + len(x)] = x
    pcm = torch.from_numpy(buf.copy()).to(dev)
    len_dev = None if cut is None else torch.tensor(cut, dtype=torch.int32, device=dev)
    ks = [None if t is None else infer.loudness_gain_constant(t) for _, t in batch]
    stats = ops.wave_loudness(pcm, offsets, [len(x) for x, _ in batch], len_dev, ks)
    assert stats.dtype == torch.int64 and tuple(stats.shape) == (len(batch), 4)
    return pcm.cpu().numpy(), buf, offsets, [tuple(int(v) for v in row) for row in stats.cpu().tolist()]


def _expect(batch, buf, offsets, cut=None):
    """The buffer and the stats rows the host definition gives: a request's (cut) samples normalised, everything else as it was."""
    want, rows = buf.copy(), []
    for i, (o, (x, t)) in enumerate(zip(offsets, batch)):
        n = len(x) if cut is None else min(max(cut[i], 0), len(x))
        y, row = _host(x[:n], t)
        want[o:o + n] = y
        rows.append(row)
    return want, rows


def _compare(got, want, rows, want_rows, where):
    assert rows == want_rows, (where, rows, want_rows)
    if not np.array_equal(got, want):
        raise AssertionError((where, "first differing sample", int(np.flatnonzero(got != want)[0])))


@pytest.mark.parametrize("turn", range(8))
def test_kernel_equals_the_host_definition_bit_for_bit(turn):
    """Each length meets each content over the eight turns; the filler between the requests and every unflagged request stay as they were."""
    assert ops.wave_loudness_tile() == TILE
    for b, batch in enumerate(_batches(turn)):
        got, buf, offsets, rows = _device(batch)
        want, want_rows = _expect(batch, buf, offsets)
        _compare(got, want, rows, want_rows, (turn, b, [len(x) for x, _ in batch]))


def test_the_deal_covers_gated_ceiling_and_untouched_requests():
    """What the turns above meet, counted on the host: requests whose gain is set by the target, by the peak ceiling, and requests that come
    back unchanged (no block, or nothing above the gates)."""
    by_target = ceiling = unchanged = 0
    for turn in range(8):
        for batch in _batches(turn):
            for x, t in batch:
                if t is None:
                    continue
                n2, S2, peak = infer.measure_loudness(x)
                if not n2:
                    unchanged += 1
                elif infer.loudness_gain(n2, S2, peak, infer.loudness_gain_constant(t)) == infer.LOUDNESS_PEAK_CEILING / peak:
                    ceiling += 1
                else:
                    by_target += 1
    assert by_target >= 8 and ceiling >= 3 and unchanged >= 8, (by_target, ceiling, unchanged)


def test_device_side_lengths():
    """len_dev shorter than max_len, as silence removal leaves it: the result is the host function's on the cut samples, and the samples
    beyond the cut are untouched."""
    batch = [(_content(n, k + 3, k), t) for k, (n, t) in enumerate(zip([30011, 2 * TILE, 12000, 9700, 5 * RATE], [-16.0, -23.0, -20.0, -30.0, -18.0]))]
    cut = [2 * TILE + 5, 9600, 0, 9599, 3 * RATE + 1]
    got, buf, offsets, rows = _device(batch, cut)
    want, want_rows = _expect(batch, buf, offsets, cut)
    _compare(got, want, rows, want_rows, "cut")
    assert any(r[0] > 0 for r in rows)
    got, buf, offsets, rows = _device(batch[:2], [10 ** 9, -5])                          # clamped to [0, max_len]
    want, want_rows = _expect(batch[:2], buf, offsets, [10 ** 9, -5])
    _compare(got, want, rows, want_rows, "clamped")


def test_a_request_does_not_depend_on_its_call():
    batch = [(_content(n, k + 3, 7 + k), t) for k, (n, t) in enumerate(zip([30011, 9601, 2 * TILE + 3, 5 * RATE, 12000], [-16.0, -23.0, -30.0, -20.0, -12.0]))]
    got, _, offsets, rows = _device(batch)
    again, _, _, rows2 = _device(batch)
    assert np.array_equal(got, again) and rows == rows2
    back, _, boff, brows = _device(batch[::-1])
    for i, (x, _) in enumerate(batch):
        solo, _, _, srows = _device(batch[i:i + 1])
        assert np.array_equal(solo[:len(x)], got[offsets[i]:offsets[i] + len(x)]) and srows[0] == rows[i], i
        j = len(batch) - 1 - i
        assert np.array_equal(back[boff[j]:boff[j] + len(x)], got[offsets[i]:offsets[i] + len(x)]) and brows[j] == rows[i], i


def test_three_launches_per_call_and_none_without_a_flag():
    one = [(_content(30011, 6, 1), -16.0)]
    five = [(_content(n, k + 2, k), -20.0 - k) for k, n in enumerate([30011, 9601, 0, 5 * RATE, 100])]
    _device(one)                                                                        # (the first call of a process also allocates)
    for batch, requests in ((one, 1), (five, 5), (five + [(_content(9700, 6, 9), None)], 5)):
        _reset()
        _device(batch)
        assert _counter("wave_loudness_launches") == 3 and _counter("wave_loudness_requests") == requests
        assert _counter("wave_encode_launches") == 0 and _counter("wave_finish_launches") == 0 and _counter("wave_flac_launches") == 0
    _reset()
    none = [(x, None) for x, _ in five]
    got, buf, _, rows = _device(none)
    assert np.array_equal(got, buf) and rows == [(0, 0, 0, 0)] * 5
    # the library itself, without the binding's shortcut: a call without a flagged request returns 0 and launches nothing
    dev = torch.device("cuda:0")
    pcm, stats = torch.full((256,), FILLER, device=dev, dtype=torch.int16), torch.zeros(4, device=dev, dtype=torch.int64)
    io, ml, gk = np.zeros(1, dtype=np.int64), np.array([200], dtype=np.int32), np.array([0.0])
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    assert _lib.lib().f5hip_wave_loudness(1, C.c_void_p(pcm.data_ptr()), p(io), p(ml), None, p(gk), C.c_void_p(stats.data_ptr()), _lib.current_stream_ptr()) == 0
    assert _counter("wave_loudness_launches") == 0 and _counter("wave_loudness_requests") == 0


def test_ctypes_and_torch_op_paths_agree():
    batch = _batches(6)[4]
    got, _, _, rows = _device(batch)
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        again, _, _, rows2 = _device(batch)
    finally:
        torch_ops._loaded = True
    assert np.array_equal(got, again) and rows == rows2


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    pcm = torch.zeros(4096, device=dev, dtype=torch.int16)
    stats = torch.zeros(16, device=dev, dtype=torch.int64)
    lens = torch.zeros(4, device=dev, dtype=torch.int32)
    k16 = infer.loudness_gain_constant(-16.0)

    def call(max_len=(100,), gain=(k16,), n=None, pcm_p=pcm.data_ptr(), st_p=stats.data_ptr(), len_p=None, in_p=True, ml_p=True, gk_p=True):
        ml, gk = np.asarray(max_len, dtype=np.int32), np.asarray(gain, dtype=np.float64)
        io = np.zeros(len(ml), dtype=np.int64)
        p = lambda a, on: C.c_void_p(a.ctypes.data) if on else None   # noqa: E731
        return lib.f5hip_wave_loudness(len(ml) if n is None else n, C.c_void_p(pcm_p), p(io, in_p), p(ml, ml_p), C.c_void_p(len_p) if len_p else None,
                                       p(gk, gk_p), C.c_void_p(st_p), _lib.current_stream_ptr())

    _reset()
    assert call(n=0) != 0 and b"bad argument" in lib.f5hip_last_error()
    for null in (dict(pcm_p=None), dict(in_p=False), dict(ml_p=False), dict(gk_p=False), dict(st_p=None)):
        assert call(**null) != 0 and b"bad argument" in lib.f5hip_last_error(), null
    assert call(max_len=(-1,)) != 0 and b"negative" in lib.f5hip_last_error()
    assert call(pcm_p=pcm.data_ptr() + 1) != 0 and b"aligned" in lib.f5hip_last_error()
    assert call(st_p=stats.data_ptr() + 4) != 0 and b"aligned" in lib.f5hip_last_error()
    assert call(len_p=lens.data_ptr() + 2) != 0 and b"aligned" in lib.f5hip_last_error()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(gain=(bad,)) != 0 and b"not finite" in lib.f5hip_last_error(), bad
    assert call(max_len=(2 ** 31 - 1, 2 ** 31 - 1), gain=(k16, k16)) != 0 and b"2^31" in lib.f5hip_last_error()       # (refused unread)
    with pytest.raises(_lib.F5HipError):
        ops.wave_loudness(pcm, [4000], [100], None, [k16])                              # covers samples past the tensor
    with pytest.raises(_lib.F5HipError, match="int16"):
        ops.wave_loudness(pcm.to(torch.int32), [0], [100], None, [k16])
    with pytest.raises(_lib.F5HipError, match="finite"):
        ops.wave_loudness(pcm, [0], [100], None, [float("nan")])
    with pytest.raises(RuntimeError, match="one value per request"):
        torch.ops.f5hip.wave_loudness(pcm, torch.zeros(1, dtype=torch.int64), torch.tensor([100], dtype=torch.int32), None, torch.zeros(2, dtype=torch.float64))
    assert _counter("wave_loudness_launches") == 0 and _counter("wave_loudness_requests") == 0
    assert call() == 0 and _counter("wave_loudness_launches") == 3 and _counter("wave_loudness_requests") == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ between wave_finish and the encoders
def _chunk_requests():
    """A request with a pause (silence removal shortens it), a loud one of two chunks, a quiet one of one chunk, one that stays as it is."""
    noise = lambda n, s, amp: (amp * np.random.default_rng(s).standard_normal(n)).astype(np.float32)   # noqa: E731
    pause = np.concatenate([noise(2 * RATE, 1, 0.1), np.zeros(int(2.5 * RATE), np.float32), noise(2 * RATE, 2, 0.1)])
    return ([[pause], [noise(19003, 5, 0.3), noise(17201, 6, 0.3)], [noise(30011, 7, 0.004)], [noise(20000, 8, 0.1)]], [True, False, False, False],
            [-23.0, -16.0, -30.0, None])


def test_chains_behind_wave_finish_equal_the_host_pipeline():
    """wave_finish -> wave_loudness -> wave_encode (8 kHz mu-law), and -> wave_flac, on the same stream with the lengths on the device:
    `deliver_pcm16(normalise_loudness_pcm16(...))` byte for byte, with `remove_silence` on one request."""
    dev = torch.device("cuda:0")
    reqs, flags, targets = _chunk_requests()
    F = int(FADE_S * RATE)
    host_pcm = infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16")
    assert len(host_pcm[0]) < len(reqs[0][0])                                           # (the pause was cut: the length is the device's alone)
    want = [infer.normalise_loudness_pcm16(x, t) for x, t in zip(host_pcm, targets)]
    assert not np.array_equal(want[0], host_pcm[0]) and np.array_equal(want[3], host_pcm[3])
    chunks = [torch.from_numpy(c).to(dev) for r in reqs for c in r]
    joined = [sum(len(c) for c in r) - (len(r) - 1) * F for r in reqs]
    ks = [None if t is None else infer.loudness_gain_constant(t) for t in targets]
    for kind in ("mulaw", "flac"):
        pcm, lengths, offsets = ops.wave_finish(chunks, [len(r) for r in reqs], F, flags, RATE)
        ops.wave_loudness(pcm, offsets, joined, lengths, ks)
        if kind == "mulaw":
            data, out_len, out_off = ops.wave_encode(pcm, offsets, joined, lengths, 8000, "mulaw", infer._device_taps(RATE, 8000, dev))
        else:
            data, out_len, out_off = ops.wave_flac(pcm, offsets, joined, lengths, RATE)
        host, counts = data.cpu().numpy(), out_len.cpu().tolist()
        for i, (o, m, y) in enumerate(zip(out_off, counts, want)):
            assert host[o:o + m].tobytes() == infer.deliver_pcm16(y, 8000 if kind == "mulaw" else RATE, kind).tobytes(), (kind, i)


def test_finish_requests_makes_one_loudness_call_and_no_copy_for_it():
    dev = torch.device("cuda:0")
    reqs, flags, targets = _chunk_requests()
    reqs, flags, targets = reqs + [reqs[1], reqs[2]], flags + [False, False], targets + [-20.0, -26.0]
    rates, encs = [None, 8000, None, None, None, 44100], [None, "mulaw", None, None, "flac", "flac"]
    on_dev = [[torch.from_numpy(c).to(dev) for c in r] for r in reqs]
    want = infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16", sample_rate=rates, encoding=encs, loudness=targets)
    copies = {}
    for with_option in (False, True):
        infer.backend_stats.clear()
        _reset()
        got = infer.finish_requests(on_dev, ["x"] * len(reqs), FADE_S, flags, device_backend=True, want="pcm16", sample_rate=rates, encoding=encs,
                                    loudness=targets if with_option else None)
        stats = dict(infer.backend_stats)
        copies[with_option] = stats["d2h_copies"]
        assert stats["device_requests"] == len(reqs) and stats["device_calls"] == 1 and stats.get("host_requests", 0) == 0
        if with_option:
            assert stats["loudness_calls"] == 1 and stats["loudness_requests"] == 5
            assert _counter("wave_loudness_launches") == 3 and _counter("wave_loudness_requests") == 5
        else:
            assert "loudness_calls" not in stats and _counter("wave_loudness_launches") == 0
    assert copies[True] == copies[False]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and len(g) == len(w) and np.array_equal(g, w), i
    plain = infer.finish_requests(reqs[:1], ["x"], FADE_S, flags[:1], want="pcm16")[0]
    assert np.array_equal(got[0], infer.normalise_loudness_pcm16(plain, targets[0])) and not np.array_equal(got[0], plain)


# ------------------------------------------------------------------------------------------------ end to end on a tiny model
@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


def test_infer_requests_with_loudness_in_one_micro_batch(hip_objects, tmp_path):
    """Plain requests with two targets, a script whose two voices have different prompt levels, and a request without the option, in ONE
    micro-batch: the device back-end's results are the host's, with one `ops.wave_loudness` call and no further copy."""
    path = _prompt(tmp_path)
    text = TEXT[:110]
    script = f"{TEXT[:64]} [town] I live in town."
    voices = {"main": dict(ref_audio_path=path, ref_text=REF_TEXT), "town": dict(ref_audio=(synth.ref_audio(16000 * 2, seed=77, amp=0.02), 16000),
                                                                                  ref_text="Town speaks.")}
    opts = [dict(seed=7, loudness=-16.0), dict(seed=7, loudness=-30.0, sample_rate=8000, encoding="mulaw"), dict(seed=7),
            dict(seed=7, loudness=-23.0, remove_silence=True)]
    out, copies = {}, {}
    for backend, with_option in ((True, True), (False, True), (True, False)):
        mgr = serve.TTSManager(nfe_step=8, device_backend=backend).load(*hip_objects)
        try:
            voice, ref_text_n = mgr._voice(path, REF_TEXT)
            strip = (lambda o: {k: v for k, v in o.items() if k != "loudness"}) if not with_option else (lambda o: o)
            batch = [(voice, ref_text_n, text, strip(o)) for o in opts]
            segments = mgr._script_segments(script, voices, 0.5)
            batch += [infer.ScriptRequest(segments, strip(dict(seed=7, loudness=-20.0)), 0.5)]
            _reset()
            infer.backend_stats.clear()
            out[backend, with_option] = mgr._run_batch(batch)
            copies[backend, with_option] = infer.backend_stats["d2h_copies"]
            if backend and with_option:
                assert infer.backend_stats["device_requests"] == len(batch) and infer.backend_stats.get("host_requests", 0) == 0
                assert infer.backend_stats["loudness_calls"] == 1 and infer.backend_stats["loudness_requests"] == 4
                assert _counter("wave_loudness_launches") == 3 and _counter("wave_loudness_requests") == 4
            else:
                assert _counter("wave_loudness_launches") == 0
        finally:
            mgr.close()
    dev, host, before = out[True, True], out[False, True], out[True, False]
    assert copies[True, True] <= copies[True, False]
    for i, (d, h) in enumerate(zip(dev, host)):
        h = h if h.dtype != np.float32 else infer.quantise_pcm16(h)                     # (the host back-end leaves a request without options as float32)
        assert d.dtype == h.dtype and len(d) == len(h) and np.array_equal(d, h), i
    assert np.array_equal(dev[2], before[2])                                            # the request without the option: as without the feature
    for i, target in ((0, -16.0), (4, -20.0)):                                          # the host function of the PCM the batch gives without the option
        assert np.array_equal(dev[i], infer.normalise_loudness_pcm16(before[i], target)), i
    n2, S2, _ = infer.measure_loudness(before[0])
    assert n2 > 0 and not np.array_equal(dev[0], before[0])                             # (the tiny model's wave is loud enough to be measured)
