"""Tempo and pitch on the device (csrc/wave_out.h, f5hip_wave_prosody: the 24 kHz int16 PCM of a ragged batch of requests, time-scale
modified per request in two launches, one without a pitch) against the host definition `infer.shift_pcm16`, alone, chained between
`ops.wave_finish` and `ops.wave_loudness` / `ops.wave_encode` / `ops.wave_flac`, and through `infer_requests` with the device back-end on a
tiny model.

Every comparison is equality of bytes and of lengths: there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, ops, serve, synth, torch_ops, wave_codec  # noqa: E402

from test_gpu_request_knobs import ARCH, REF_TEXT, TEXT, VOCAB, _prompt  # noqa: E402

RATE = 24000
FADE_S = infer.cross_fade_duration
LENGTHS = [0, 1, 2, 239, 479, 480, 481, 959, 960, 961, 1441, 5000, 30011, 3 * RATE]
SIZES = (1, 2, 3, 5, 3)                                # the 14 lengths dealt into batches
# (tempo, pitch) per request: neutral, tempo only, pitch only, both; the stretches 4/5, 5/4, 1/2, 2/1, 46/41, 17/18, 400/399, ...
OPTIONS = [(1.0, 0), (1.25, 0), (1.0, 2), (0.8, 0), (1.0, -1), (2.0, 0), (1.1, 3), (0.5, 0), (0.9, -6), (1.33, 5), (1.0, 6)]
FILLER = 23456
_host_cache = {}


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _content(n, kind, seed):
    """Zeros, a constant -32768, the alternating full-scale square, a 100 Hz square (its period of 240 samples makes exact ties), noise,
    a voiced-like sum of harmonics."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return [lambda: np.zeros(n, dtype=np.int16),
            lambda: np.full(n, -32768, dtype=np.int16),
            lambda: np.where(t % 2 == 0, 32767, -32768).astype(np.int16),
            lambda: np.where((t // 120) % 2 == 0, 12000, -12000).astype(np.int16),
            lambda: infer.quantise_pcm16(0.2 * rng.standard_normal(n)),
            lambda: infer.quantise_pcm16(sum(0.2 / h * np.sin(2 * np.pi * 131.0 * h * t / RATE + h) for h in range(1, 6)))][kind % 6]()


def _batches(turn):
    """The 14 lengths dealt into batches of 1 to 5 requests; request j of the deal takes content (j + turn) mod 6 and options (j + 3 turn) mod 11."""
    out, k = [], 0
    for size in SIZES:
        out.append([(_content(n, k + j + turn, 100 * turn + k + j), OPTIONS[(k + j + 3 * turn) % len(OPTIONS)]) for j, n in enumerate(LENGTHS[k:k + size])])
        k += size
    return out


def _host(x, opt):
    key = (x.tobytes(), opt)
    if key not in _host_cache:
        _host_cache[key] = infer.shift_pcm16(x, *opt)
    return _host_cache[key]


def _spec(opt):
    return infer.WaveSpec.of(dict(tempo=opt[0], pitch=opt[1]))


def _device(batch, cut=None):
    """ops.wave_prosody on ONE packed buffer with the requests at `wave_finish`'s 8-sample offsets and a loud filler between them -> (each
    request's samples, the input buffer afterwards and before, the bounds)."""
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
    pcm2, lengths2, offsets2, bounds2 = ops.wave_prosody(pcm, offsets, [len(x) for x, _ in batch], len_dev, [_spec(o).stretch for _, o in batch],
                                                         [o[1] for _, o in batch])
    assert pcm2.dtype == torch.int16 and lengths2.dtype == torch.int32 and all(o % 8 == 0 for o in offsets2)
    host, counts = pcm2.cpu().numpy(), lengths2.cpu().tolist()
    assert all(0 <= m <= b for m, b in zip(counts, bounds2)) and all(o + b <= len(host) for o, b in zip(offsets2, bounds2))
    return [host[o:o + m].copy() for o, m in zip(offsets2, counts)], pcm.cpu().numpy(), buf, bounds2


def _compare(got, want, where):
    assert len(got) == len(want), (where, len(got), len(want))
    if not np.array_equal(got, want):
        raise AssertionError((where, "first differing sample", int(np.flatnonzero(got != want)[0]), "of", len(want)))


@pytest.mark.parametrize("turn", range(4))
def test_kernels_equal_the_host_definition_bit_for_bit(turn):
    """Each length meets several contents and option sets over the turns; the input, the filler between the requests included, is not written,
    and a request's bound is its length."""
    for b, batch in enumerate(_batches(turn)):
        got, after, before, bounds = _device(batch)
        assert np.array_equal(after, before)
        for i, (x, opt) in enumerate(batch):
            want = _host(x, opt)
            assert bounds[i] == len(want) == wave_codec.shifted_length(len(x), _spec(opt).stretch, opt[1])
            _compare(got[i], want, (turn, b, i, len(x), opt))


def test_device_side_lengths():
    """len_dev shorter than max_len, as silence removal leaves it: the result is the host function's on the cut samples."""
    opts = [(1.25, 0), (0.8, 2), (1.0, 0), (1.0, -3), (1.5, 0)]
    batch = [(_content(n, k + 3, k), o) for k, (n, o) in enumerate(zip([30011, 9600, 12000, 9700, 2 * RATE], opts))]
    cut = [20005, 481, 0, 9599, RATE + 1]
    got, _, _, _ = _device(batch, cut)
    for i, ((x, o), n) in enumerate(zip(batch, cut)):
        _compare(got[i], _host(x[:n], o), ("cut", i))
    got, _, _, _ = _device(batch[:2], [10 ** 9, -5])                                     # clamped to [0, max_len]
    _compare(got[0], _host(batch[0][0], opts[0]), "clamped high")
    assert len(got[1]) == 0


def test_a_request_does_not_depend_on_its_call():
    opts = [(1.25, 0), (1.0, 2), (0.8, -1), (1.0, 0), (2.0, 0)]
    batch = [(_content(n, k + 3, 7 + k), o) for k, (n, o) in enumerate(zip([30011, 961, 5000, 12000, 20000], opts))]
    got, _, _, _ = _device(batch)
    again, _, _, _ = _device(batch)
    back, _, _, _ = _device(batch[::-1])
    for i in range(len(batch)):
        solo, _, _, _ = _device(batch[i:i + 1])
        assert np.array_equal(solo[0], got[i]) and np.array_equal(again[i], got[i]) and np.array_equal(back[len(batch) - 1 - i], got[i]), i


def test_two_launches_per_call_and_one_without_a_pitch():
    x = _content(5000, 5, 1)
    _device([(x, (1.25, 2))])                                                           # (the first call of a process also allocates)
    for opts, launches, requests in (([(1.25, 0)], 1, 1), ([(1.25, 2)], 2, 1), ([(1.25, 0), (1.0, 0), (0.8, 0), (1.1, 0), (2.0, 0)], 1, 4),
                                     ([(1.25, 0), (1.0, 0), (1.0, -4), (1.1, 3), (0.5, 0)], 2, 4), ([(1.0, 0), (1.0, 0)], 1, 0)):
        _reset()
        got, _, _, _ = _device([(x, o) for o in opts])
        assert _counter("wave_prosody_launches") == launches and _counter("wave_prosody_requests") == requests, opts
        assert _counter("wave_encode_launches") == 0 and _counter("wave_finish_launches") == 0 and _counter("wave_loudness_launches") == 0
        for g, o in zip(got, opts):
            _compare(g, _host(x, o), o)


def test_ctypes_and_torch_op_paths_agree():
    batch = _batches(1)[3]
    got, _, _, bounds = _device(batch)
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        again, _, _, bounds2 = _device(batch)
    finally:
        torch_ops._loaded = True
    assert bounds == bounds2 and all(np.array_equal(a, b) for a, b in zip(got, again))


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    pcm = torch.zeros(4096, device=dev, dtype=torch.int16)
    out = torch.zeros(8192, device=dev, dtype=torch.int16)
    lens = torch.zeros(4, device=dev, dtype=torch.int32)
    taps = ops.wave_prosody_taps(dev)
    assert taps.numel() == lib.f5hip_wave_prosody_tap_offset(0) and lib.f5hip_wave_prosody_tap_offset(7) == -1 and lib.f5hip_wave_prosody_tap_offset(-6) == 0

    def call(max_len=(100,), P=(5,), Q=(4,), pitch=(0,), n=None, in_off=None, out_off=None, pcm_p=pcm.data_ptr(), out_p=out.data_ptr(), len_p=None,
             taps_p=taps.data_ptr(), outlen_p=lens.data_ptr(), null=()):
        arrays = dict(ml=np.asarray(max_len, dtype=np.int32), P=np.asarray(P, dtype=np.int32), Q=np.asarray(Q, dtype=np.int32),
                      pitch=np.asarray(pitch, dtype=np.int32))
        k = len(arrays["ml"])
        arrays["io"] = np.zeros(k, dtype=np.int64) if in_off is None else np.asarray(in_off, dtype=np.int64)
        arrays["oo"] = 2048 * np.arange(k, dtype=np.int64) if out_off is None else np.asarray(out_off, dtype=np.int64)
        p = lambda name: None if name in null else C.c_void_p(arrays[name].ctypes.data)   # noqa: E731
        v = lambda a: C.c_void_p(a) if a else None                                         # noqa: E731
        return lib.f5hip_wave_prosody(k if n is None else n, v(pcm_p), p("io"), p("ml"), v(len_p), p("P"), p("Q"), p("pitch"), v(taps_p), v(out_p), p("oo"),
                                      v(outlen_p), _lib.current_stream_ptr())

    _reset()
    assert call(n=0) != 0 and b"bad argument" in lib.f5hip_last_error()
    for null in (dict(pcm_p=None), dict(out_p=None), dict(outlen_p=None), dict(null=("io",)), dict(null=("ml",)), dict(null=("P",)), dict(null=("Q",)),
                 dict(null=("pitch",)), dict(null=("oo",))):
        assert call(**null) != 0 and b"bad argument" in lib.f5hip_last_error(), null
    assert call(max_len=(-1,)) != 0 and b"negative" in lib.f5hip_last_error()
    assert call(in_off=(-8,)) != 0 and b"negative" in lib.f5hip_last_error()
    assert call(out_off=(-8,)) != 0 and b"multiple of 8" in lib.f5hip_last_error()
    assert call(out_off=(4,)) != 0 and b"multiple of 8" in lib.f5hip_last_error()
    assert call(pcm_p=pcm.data_ptr() + 1) != 0 and b"aligned" in lib.f5hip_last_error()
    assert call(out_p=out.data_ptr() + 8) != 0 and b"aligned" in lib.f5hip_last_error()
    assert call(len_p=lens.data_ptr() + 2) != 0 and b"aligned" in lib.f5hip_last_error()
    assert call(taps_p=taps.data_ptr() + 4, pitch=(1,), P=(18,), Q=(17,)) != 0 and b"aligned" in lib.f5hip_last_error()
    for P, Q in ((0, 1), (1, 0), (-2, -1)):
        assert call(P=(P,), Q=(Q,)) != 0 and b"positive" in lib.f5hip_last_error(), (P, Q)
    for P, Q in ((201, 100), (100, 201), (3, 1), (1 << 21, 1 << 21)):
        assert call(P=(P,), Q=(Q,)) != 0 and b"outside 1/2 to 2" in lib.f5hip_last_error(), (P, Q)
    for s in (7, -7):
        assert call(pitch=(s,)) != 0 and b"semitones" in lib.f5hip_last_error()
    assert call(pitch=(1,), P=(18,), Q=(17,), taps_p=None) != 0 and b"tap table" in lib.f5hip_last_error()
    assert call(max_len=(2 ** 31 - 1, 2 ** 31 - 1), P=(1, 1), Q=(1, 1), pitch=(0, 0)) != 0 and b"2^31" in lib.f5hip_last_error()   # (refused unread)
    assert call(max_len=(2 ** 31 - 1,), P=(2,), Q=(1,)) != 0 and b"2^31" in lib.f5hip_last_error()
    with pytest.raises(_lib.F5HipError):
        ops.wave_prosody(pcm, [4000], [100], None, [(5, 4)], [0])                       # reads samples past the tensor
    with pytest.raises(_lib.F5HipError, match="int16"):
        ops.wave_prosody(pcm.to(torch.int32), [0], [100], None, [(5, 4)], [0])
    with pytest.raises(_lib.F5HipError, match="1/2 to 2"):
        ops.wave_prosody(pcm, [0], [100], None, [(3, 1)], [0])
    with pytest.raises(_lib.F5HipError, match="semitones"):
        ops.wave_prosody(pcm, [0], [100], None, [(1, 1)], [2.0])
    with pytest.raises(_lib.F5HipError, match="-6 to 6"):
        ops.wave_prosody(pcm, [0], [100], None, [(1, 1)], [7])
    one = lambda v, dt: torch.tensor([v], dtype=dt)   # noqa: E731
    with pytest.raises(RuntimeError, match="one value per request"):
        torch.ops.f5hip.wave_prosody(pcm, one(0, torch.int64), one(100, torch.int32), None, one(5, torch.int32), one(4, torch.int32),
                                     torch.zeros(2, dtype=torch.int32), None)
    with pytest.raises(RuntimeError, match="needs taps"):
        torch.ops.f5hip.wave_prosody(pcm, one(0, torch.int64), one(100, torch.int32), None, one(18, torch.int32), one(17, torch.int32),
                                     one(1, torch.int32), None)
    with pytest.raises(RuntimeError, match="HIP device"):
        torch.ops.f5hip.wave_prosody(pcm.cpu(), one(0, torch.int64), one(100, torch.int32), None, one(5, torch.int32), one(4, torch.int32),
                                     one(0, torch.int32), None)
    assert _counter("wave_prosody_launches") == 0 and _counter("wave_prosody_requests") == 0
    assert call() == 0 and _counter("wave_prosody_launches") == 1 and _counter("wave_prosody_requests") == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ between wave_finish and what follows it
def _chunk_requests():
    """A request with a pause (silence removal shortens it), one of two chunks, a short one, one that stays as it is."""
    noise = lambda n, s, amp: (amp * np.random.default_rng(s).standard_normal(n)).astype(np.float32)   # noqa: E731
    pause = np.concatenate([noise(RATE, 1, 0.1), np.zeros(int(2.5 * RATE), np.float32), noise(RATE, 2, 0.1)])
    return ([[pause], [noise(19003, 5, 0.3), noise(17201, 6, 0.3)], [noise(12011, 7, 0.05)], [noise(20000, 8, 0.1)]], [True, False, False, False],
            [(1.25, 0), (0.9, 2), (1.0, -5), (1.0, 0)], [-23.0, -16.0, None, -20.0])


def test_chains_behind_wave_finish_equal_the_host_pipeline():
    """wave_finish (silence removal: the length is on the device alone, below the bound) -> wave_prosody -> wave_loudness -> wave_encode
    (8 kHz mu-law), and -> wave_flac: `deliver_pcm16(normalise_loudness_pcm16(shift_pcm16(...)))` byte for byte."""
    dev = torch.device("cuda:0")
    reqs, flags, opts, targets = _chunk_requests()
    F = int(FADE_S * RATE)
    host_pcm = infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16")
    assert len(host_pcm[0]) < len(reqs[0][0])                                           # (the pause was cut)
    want = [infer.normalise_loudness_pcm16(infer.shift_pcm16(x, *o), t) for x, o, t in zip(host_pcm, opts, targets)]
    chunks = [torch.from_numpy(c).to(dev) for r in reqs for c in r]
    joined = [sum(len(c) for c in r) - (len(r) - 1) * F for r in reqs]
    ks = [None if t is None else infer.loudness_gain_constant(t) for t in targets]
    for kind in ("mulaw", "flac"):
        pcm, lengths, offsets = ops.wave_finish(chunks, [len(r) for r in reqs], F, flags, RATE)
        pcm2, lengths2, offsets2, bounds2 = ops.wave_prosody(pcm, offsets, joined, lengths, [_spec(o).stretch for o in opts], [o[1] for o in opts])
        assert lengths2.cpu().tolist() == [len(infer.shift_pcm16(x, *o)) for x, o in zip(host_pcm, opts)] and lengths2[0].item() < bounds2[0]
        ops.wave_loudness(pcm2, offsets2, bounds2, lengths2, ks)
        if kind == "mulaw":
            data, out_len, out_off = ops.wave_encode(pcm2, offsets2, bounds2, lengths2, 8000, "mulaw", infer._device_taps(RATE, 8000, dev))
        else:
            data, out_len, out_off = ops.wave_flac(pcm2, offsets2, bounds2, lengths2, RATE)
        host, counts = data.cpu().numpy(), out_len.cpu().tolist()
        for i, (o, m, y) in enumerate(zip(out_off, counts, want)):
            assert host[o:o + m].tobytes() == infer.deliver_pcm16(y, 8000 if kind == "mulaw" else RATE, kind).tobytes(), (kind, i)


def test_finish_requests_makes_one_prosody_call_for_the_batch():
    dev = torch.device("cuda:0")
    reqs, flags, opts, targets = _chunk_requests()
    reqs, flags, opts, targets = reqs + [reqs[1], reqs[2]], flags + [False, False], opts + [(1.5, 0), (0.75, -2)], targets + [None, -26.0]
    rates, encs = [None, 8000, None, None, None, 44100], [None, "mulaw", None, None, "flac", "flac"]
    on_dev = [[torch.from_numpy(c).to(dev) for c in r] for r in reqs]
    keywords = dict(sample_rate=rates, encoding=encs, loudness=targets, tempo=[o[0] for o in opts], pitch=[o[1] for o in opts])
    want = infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16", **keywords)
    for with_option in (False, True):
        infer.backend_stats.clear()
        _reset()
        kw = keywords if with_option else dict(keywords, tempo=None, pitch=None)
        got = infer.finish_requests(on_dev, ["x"] * len(reqs), FADE_S, flags, device_backend=True, want="pcm16", **kw)
        stats = dict(infer.backend_stats)
        assert stats["device_requests"] == len(reqs) and stats["device_calls"] == 1 and stats.get("host_requests", 0) == 0
        if with_option:
            assert stats["prosody_calls"] == 1 and stats["prosody_requests"] == 5
            assert _counter("wave_prosody_launches") == 2 and _counter("wave_prosody_requests") == 5
            for i, (g, w) in enumerate(zip(got, want)):
                assert g.dtype == w.dtype and len(g) == len(w) and np.array_equal(g, w), i
        else:
            assert "prosody_calls" not in stats and _counter("wave_prosody_launches") == 0


# ------------------------------------------------------------------------------------------------ end to end on a tiny model
@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


def test_infer_requests_with_tempo_and_pitch_in_one_micro_batch(hip_objects, tmp_path):
    """Plain requests with a tempo, a pitch and both, one without the options and a script, in ONE micro-batch: the device back-end's
    results are the host's, with one `ops.wave_prosody` call, and each is `shift_pcm16` of what the batch gives without the options."""
    path = _prompt(tmp_path)
    text = TEXT[:110]
    script = f"{TEXT[:64]} [town] I live in town."
    voices = {"main": dict(ref_audio_path=path, ref_text=REF_TEXT), "town": dict(ref_audio=(synth.ref_audio(16000 * 2, seed=77, amp=0.02), 16000),
                                                                                  ref_text="Town speaks.")}
    opts = [dict(seed=7, tempo=1.25), dict(seed=7, pitch=-2, sample_rate=8000, encoding="mulaw"), dict(seed=7), dict(seed=7, tempo=0.9, pitch=3, loudness=-20.0)]
    out = {}
    for backend, with_option in ((True, True), (False, True), (True, False)):
        mgr = serve.TTSManager(nfe_step=8, device_backend=backend).load(*hip_objects)
        try:
            voice, ref_text_n = mgr._voice(path, REF_TEXT)
            strip = (lambda o: {k: v for k, v in o.items() if k not in infer.PROSODY_OPTIONS}) if not with_option else (lambda o: o)
            batch = [(voice, ref_text_n, text, strip(o)) for o in opts]
            segments = mgr._script_segments(script, voices, 0.5)
            batch += [infer.ScriptRequest(segments, strip(dict(seed=7, tempo=1.1, pitch=1)), 0.5)]
            _reset()
            infer.backend_stats.clear()
            out[backend, with_option] = mgr._run_batch(batch)
            if backend and with_option:
                assert infer.backend_stats["device_requests"] == len(batch) and infer.backend_stats.get("host_requests", 0) == 0
                assert infer.backend_stats["prosody_calls"] == 1 and infer.backend_stats["prosody_requests"] == 4
                assert _counter("wave_prosody_launches") == 2 and _counter("wave_prosody_requests") == 4
            else:
                assert _counter("wave_prosody_launches") == 0
        finally:
            mgr.close()
    dev, host, before = out[True, True], out[False, True], out[True, False]
    for i, (d, h) in enumerate(zip(dev, host)):
        h = h if h.dtype != np.float32 else infer.quantise_pcm16(h)                     # (the host back-end leaves a request without options as float32)
        assert d.dtype == h.dtype and len(d) == len(h) and np.array_equal(d, h), i
    assert np.array_equal(dev[2], before[2])                                            # the request without the options: as without the feature
    assert np.array_equal(dev[0], infer.shift_pcm16(before[0], 1.25)) and len(dev[0]) == -(-len(before[0]) * 4 // 5)
    assert np.array_equal(dev[4], infer.shift_pcm16(before[4], 1.1, 1)) and not np.array_equal(dev[4], before[4])
