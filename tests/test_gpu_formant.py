"""The formant-preserving pitch shift on the device (csrc/wave_formant.h, f5hip_wave_prosody_formants: `ops.wave_prosody(...,
keep_formants=...)`, three launches behind the WSOLA launch whatever the batch) against the host definition `infer.shift_pcm16(...,
keep_formants=True)` = `wsola_pcm16` by the tempo alone, then `psola_pcm16`: the case matrix of tests/test_formant_host.py in ragged
batches with mixed options, device-side lengths, a request alone and in a batch, both bindings, the launch counts, the refusals, the chain
between `ops.wave_finish` and `ops.wave_mark` / `ops.wave_loudness` / `ops.wave_encode`, and `infer_requests` on a tiny model.

Every comparison is equality of bytes and of lengths: there is no tolerance anywhere."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, ops, serve, synth, torch_ops, wave_codec  # noqa: E402

from test_formant_host import CONTENTS, LENGTHS, content, vowel  # noqa: E402
from test_gpu_request_knobs import ARCH, REF_TEXT, TEXT, VOCAB, _prompt  # noqa: E402

RATE = 24000
FADE_S = infer.cross_fade_duration
SIZES = (1, 2, 3, 5, 3)                                # the 7 lengths, twice, dealt into batches
# (tempo, pitch, keep_formants) per request: neutral, tempo only, plain pitch, kept pitch, kept pitch with a tempo
OPTIONS = [(1.0, 0, False), (1.25, 0, False), (1.0, 2, False), (1.0, 4, True), (1.25, -6, True), (0.8, 3, True), (1.0, -1, True), (0.9, -3, False),
           (1.0, 6, True)]
FILLER = 23456
_host_cache = {}


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _batches(turn):
    """The 7 lengths, twice, dealt into batches of 1 to 5 requests; request j of the deal takes content (j + turn) mod 5 and options
    (j + 2 turn) mod 9: over the five turns every length meets every content."""
    lengths = LENGTHS + LENGTHS
    out, k = [], 0
    for size in SIZES:
        out.append([(content(CONTENTS[(k + j + turn) % len(CONTENTS)], n), OPTIONS[(k + j + 2 * turn) % len(OPTIONS)]) for j, n in enumerate(lengths[k:k + size])])
        k += size
    return out


def _host(x, opt):
    key = (x.tobytes(), opt)
    if key not in _host_cache:
        _host_cache[key] = infer.shift_pcm16(x, opt[0], opt[1], keep_formants=opt[2])
    return _host_cache[key]


def _stretch(opt):
    return wave_codec.formant_stretch(round(100 * opt[0])) if opt[2] else infer.WaveSpec.of(dict(tempo=opt[0], pitch=opt[1])).stretch


def _device(batch, cut=None, flags=True):
    """ops.wave_prosody on ONE packed buffer with the requests at `wave_finish`'s 8-sample offsets and a loud filler between them -> (each
    request's samples, the input buffer afterwards and before, the bounds).  flags=False: the call without the keyword."""
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
    keyword = dict(keep_formants=[o[2] for _, o in batch]) if flags else {}
    pcm2, lengths2, offsets2, bounds2 = ops.wave_prosody(pcm, offsets, [len(x) for x, _ in batch], len_dev, [_stretch(o) for _, o in batch],
                                                         [o[1] for _, o in batch], **keyword)
    assert pcm2.dtype == torch.int16 and lengths2.dtype == torch.int32 and all(o % 8 == 0 for o in offsets2)
    host, counts = pcm2.cpu().numpy(), lengths2.cpu().tolist()
    assert all(0 <= m <= b for m, b in zip(counts, bounds2)) and all(o + b <= len(host) for o, b in zip(offsets2, bounds2))
    return [host[o:o + m].copy() for o, m in zip(offsets2, counts)], pcm.cpu().numpy(), buf, bounds2


def _compare(got, want, where):
    assert len(got) == len(want), (where, len(got), len(want))
    if not np.array_equal(got, want):
        raise AssertionError((where, "first differing sample", int(np.flatnonzero(got != want)[0]), "of", len(want)))


@pytest.mark.parametrize("turn", range(5))
def test_kernels_equal_the_host_definition_bit_for_bit(turn):
    """The case matrix in ragged batches with mixed options: every request's bytes and length are the host function's; the input, the filler
    between the requests included, is not written; a kept request's bound is the length of its tempo's stretch alone."""
    for b, batch in enumerate(_batches(turn)):
        got, after, before, bounds = _device(batch)
        assert np.array_equal(after, before)
        for i, (x, opt) in enumerate(batch):
            want = _host(x, opt)
            assert bounds[i] == len(want)
            if opt[2]:
                assert len(want) == -(-len(x) * 100 // round(100 * opt[0]))
            _compare(got[i], want, (turn, b, i, len(x), opt))


def test_device_side_lengths():
    """len_dev shorter than max_len, as silence removal leaves it: the result is the host function's on the cut samples, whatever lies
    behind the cut in the buffer."""
    opts = [(1.0, 4, True), (0.8, -2, True), (1.0, 5, True), (1.0, -3, False), (1.5, 1, True)]
    batch = [(content(kind, n), o) for kind, n, o in zip(("vowel", "mixed", "square", "vowel", "mixed"), (30011, 24000, 12000, 9700, 2 * RATE), opts)]
    cut = [20005, 481, 0, 9599, RATE + 1]
    got, _, _, _ = _device(batch, cut)
    for i, ((x, o), n) in enumerate(zip(batch, cut)):
        _compare(got[i], _host(x[:n], o), ("cut", i))
    got, _, _, _ = _device(batch[:2], [10 ** 9, -5])                                     # clamped to [0, max_len]
    _compare(got[0], _host(batch[0][0], opts[0]), "clamped high")
    assert len(got[1]) == 0


def test_a_request_does_not_depend_on_its_call():
    opts = [(1.0, 4, True), (1.0, 2, False), (0.8, -6, True), (1.0, 0, False), (1.25, 6, True)]
    batch = [(content(kind, n), o) for kind, n, o in zip(("vowel", "mixed", "mixed", "noise", "vowel"), (30011, 1000, 24000, 12000, 20000), opts)]
    got, _, _, _ = _device(batch)
    again, _, _, _ = _device(batch)
    back, _, _, _ = _device(batch[::-1])
    for i in range(len(batch)):
        solo, _, _, _ = _device(batch[i:i + 1])
        assert np.array_equal(solo[0], got[i]) and np.array_equal(again[i], got[i]) and np.array_equal(back[len(batch) - 1 - i], got[i]), i
        _compare(got[i], _host(*batch[i]), i)


def test_launch_counts_per_kind_of_call():
    """No flagged request: exactly today's launches (the keyword absent, or all false).  A flagged one: WSOLA, the three new launches, and
    the resampler only when another request has a plain pitch."""
    assert ops.wave_prosody_formants_launches() == 3
    x = content("vowel", 5000)
    _device([(x, (1.25, 2, True))])                                                     # (the first call of a process also allocates)
    K, P, T, N = (1.0, 4, True), (1.0, -4, False), (1.25, 0, False), (1.0, 0, False)
    for opts, flags, prosody, formant, kept, changed in (([T], False, 1, 0, 0, 1), ([T, P], False, 2, 0, 0, 2), ([T, P, N], True, 2, 0, 0, 2), ([N], True, 1, 0, 0, 0),
                                                         ([K], True, 1, 3, 1, 1), ([K, T, N], True, 1, 3, 1, 2), ([K, P], True, 2, 3, 1, 2),
                                                         ([(0.8, 6, True)] * 5, True, 1, 3, 5, 5), ([K, P, T, N, (1.25, -6, True)], True, 2, 3, 2, 4)):
        _reset()
        got, _, _, _ = _device([(x, o) for o in opts], flags=flags)
        assert _counter("wave_prosody_launches") == prosody and _counter("wave_prosody_requests") == changed, opts
        assert _counter("wave_formant_launches") == formant and _counter("wave_formant_requests") == kept, opts
        assert _counter("wave_encode_launches") == 0 and _counter("wave_finish_launches") == 0 and _counter("wave_mark_launches") == 0
        for g, o in zip(got, opts):
            _compare(g, _host(x, o), o)


def test_ctypes_and_torch_op_paths_agree():
    batch = _batches(2)[3]
    assert any(o[2] for _, o in batch) and any(o[1] and not o[2] for _, o in batch)
    got, _, _, bounds = _device(batch)
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        again, _, _, bounds2 = _device(batch)
    finally:
        torch_ops._loaded = True
    assert bounds == bounds2 and all(np.array_equal(a, b) for a, b in zip(got, again))
    for g, (x, o) in zip(got, batch):
        _compare(g, _host(x, o), o)


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    pcm = torch.zeros(4096, device=dev, dtype=torch.int16)
    out = torch.zeros(8192, device=dev, dtype=torch.int16)
    lens = torch.zeros(4, device=dev, dtype=torch.int32)
    taps = ops.wave_prosody_taps(dev)

    def call(max_len=(100,), P=(5,), Q=(4,), pitch=(3,), keep=(1,), n=None, in_off=None, out_off=None, pcm_p=pcm.data_ptr(), out_p=out.data_ptr(),
             taps_p=taps.data_ptr(), outlen_p=lens.data_ptr(), null=()):
        arrays = dict(ml=np.asarray(max_len, dtype=np.int32), P=np.asarray(P, dtype=np.int32), Q=np.asarray(Q, dtype=np.int32),
                      pitch=np.asarray(pitch, dtype=np.int32), keep=np.asarray(keep, dtype=np.uint8))
        k = len(arrays["ml"])
        arrays["io"] = np.zeros(k, dtype=np.int64) if in_off is None else np.asarray(in_off, dtype=np.int64)
        arrays["oo"] = 2048 * np.arange(k, dtype=np.int64) if out_off is None else np.asarray(out_off, dtype=np.int64)
        p = lambda name: None if name in null else C.c_void_p(arrays[name].ctypes.data)   # noqa: E731
        v = lambda a: C.c_void_p(a) if a else None                                         # noqa: E731
        return lib.f5hip_wave_prosody_formants(k if n is None else n, v(pcm_p), p("io"), p("ml"), None, p("P"), p("Q"), p("pitch"), p("keep"), v(taps_p),
                                               v(out_p), p("oo"), v(outlen_p), _lib.current_stream_ptr())

    _reset()
    assert call(n=0) != 0 and b"bad argument" in lib.f5hip_last_error()
    for null in (dict(null=("keep",)), dict(pcm_p=None), dict(out_p=None), dict(outlen_p=None), dict(null=("io",)), dict(null=("ml",)), dict(null=("P",)),
                 dict(null=("pitch",)), dict(null=("oo",))):
        assert call(**null) != 0 and b"bad argument" in lib.f5hip_last_error(), null
    assert call(pitch=(0,)) != 0 and b"keeps its formants without a pitch" in lib.f5hip_last_error()
    assert call(max_len=(100, 100), P=(1, 1), Q=(1, 1), pitch=(2, 0), keep=(1, 1)) != 0 and b"request 1 keeps its formants" in lib.f5hip_last_error()
    assert call(max_len=(-1,)) != 0 and b"negative" in lib.f5hip_last_error()
    assert call(out_off=(4,)) != 0 and b"multiple of 8" in lib.f5hip_last_error()
    assert call(pcm_p=pcm.data_ptr() + 1) != 0 and b"aligned" in lib.f5hip_last_error()
    assert call(P=(3,), Q=(1,)) != 0 and b"outside 1/2 to 2" in lib.f5hip_last_error()
    assert call(pitch=(7,)) != 0 and b"semitones" in lib.f5hip_last_error()
    assert call(max_len=(100, 100), P=(1, 1), Q=(1, 1), pitch=(2, 2), keep=(1, 0), taps_p=None) != 0 and b"tap table" in lib.f5hip_last_error()
    assert call(max_len=(2 ** 31 - 1,), P=(2,), Q=(1,)) != 0 and b"2^31" in lib.f5hip_last_error()
    with pytest.raises(_lib.F5HipError, match="without a pitch"):
        ops.wave_prosody(pcm, [0], [100], None, [(1, 1)], [0], keep_formants=[True])
    with pytest.raises(_lib.F5HipError, match="one bool per request"):
        ops.wave_prosody(pcm, [0], [100], None, [(1, 1)], [2], keep_formants=[1])
    with pytest.raises(_lib.F5HipError, match="one value per request"):
        ops.wave_prosody(pcm, [0], [100], None, [(1, 1)], [2], keep_formants=[True, False])
    with pytest.raises(_lib.F5HipError, match="1/2 to 2"):
        ops.wave_prosody(pcm, [0], [100], None, [(3, 1)], [2], keep_formants=[True])
    one = lambda v, dt: torch.tensor([v], dtype=dt)   # noqa: E731
    with pytest.raises(RuntimeError, match="one value per request"):
        torch.ops.f5hip.wave_prosody_formants(pcm, one(0, torch.int64), one(100, torch.int32), None, one(1, torch.int32), one(1, torch.int32),
                                              one(2, torch.int32), torch.zeros(2, dtype=torch.uint8), None)
    with pytest.raises(RuntimeError, match="without a pitch"):
        torch.ops.f5hip.wave_prosody_formants(pcm, one(0, torch.int64), one(100, torch.int32), None, one(1, torch.int32), one(1, torch.int32),
                                              one(0, torch.int32), one(1, torch.uint8), None)
    with pytest.raises(RuntimeError, match="needs taps"):                               # a plain pitch beside a kept one
        torch.ops.f5hip.wave_prosody_formants(pcm, torch.tensor([0, 2048]), torch.tensor([100, 100], dtype=torch.int32), None,
                                              torch.ones(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32), torch.tensor([2, 2], dtype=torch.int32),
                                              torch.tensor([1, 0], dtype=torch.uint8), None)
    for name in ("wave_prosody_launches", "wave_prosody_requests", "wave_formant_launches", "wave_formant_requests"):
        assert _counter(name) == 0, name
    assert call(taps_p=None) == 0 and _counter("wave_prosody_launches") == 1 and _counter("wave_formant_launches") == 3   # a kept pitch needs no tap table
    assert _counter("wave_formant_requests") == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ between wave_finish and what follows it
def _chunk_requests():
    """A voiced request with a pause (silence removal shortens it), one of two chunks, a short one, one that stays as it is."""
    f = lambda x: (x.astype(np.float32) / 32768.0)   # noqa: E731
    pause = np.concatenate([f(vowel(RATE, 110)), np.zeros(int(2.5 * RATE), np.float32), f(content("mixed", RATE))])
    return ([[pause], [f(vowel(19003, 140)), f(vowel(17201, 140))], [f(content("mixed", 12011))], [f(vowel(20000, 180))]], [True, False, False, False],
            [(1.0, 4, True), (0.9, -5, True), (1.0, -5, False), (1.0, 0, False)], [-23.0, -16.0, None, -20.0], [None, 77, 5, None])


def test_chain_behind_wave_finish_equals_the_host_pipeline():
    """wave_finish (silence removal: the length is on the device alone, below the bound) -> wave_prosody with the flag -> wave_mark ->
    wave_loudness -> wave_encode (8 kHz mu-law): `infer.finish_pcm16` byte for byte."""
    dev = torch.device("cuda:0")
    reqs, flags, opts, targets, keys = _chunk_requests()
    F = int(FADE_S * RATE)
    joined_pcm = infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, want="pcm16")
    specs = [infer.WaveSpec.of(dict(remove_silence=flag, tempo=o[0], pitch=o[1], loudness=t, sample_rate=8000, encoding="mulaw"))
             for flag, o, t in zip(flags, opts, targets)]
    want = [infer.finish_pcm16(x, dataclasses.replace(spec, watermark=key, keep_formants=o[2])) for x, spec, key, o in zip(joined_pcm, specs, keys, opts)]
    cut = infer.remove_silence_pcm(joined_pcm[0], RATE)
    assert len(cut) < len(joined_pcm[0]) and not np.array_equal(infer.shift_pcm16(cut, 1.0, 4, keep_formants=True), cut)   # (cut, and voiced)
    chunks = [torch.from_numpy(c).to(dev) for r in reqs for c in r]
    joined = [sum(len(c) for c in r) - (len(r) - 1) * F for r in reqs]
    pcm, lengths, offsets = ops.wave_finish(chunks, [len(r) for r in reqs], F, flags, RATE)
    pcm2, lengths2, offsets2, bounds2 = ops.wave_prosody(pcm, offsets, joined, lengths, [_stretch(o) for o in opts], [o[1] for o in opts],
                                                         keep_formants=[o[2] for o in opts])
    assert lengths2[0].item() == len(cut) < bounds2[0]
    ops.wave_mark(pcm2, offsets2, bounds2, lengths2, keys)
    ops.wave_loudness(pcm2, offsets2, bounds2, lengths2, [spec.gain_constant for spec in specs])
    data, out_len, out_off = ops.wave_encode(pcm2, offsets2, bounds2, lengths2, 8000, "mulaw", infer._device_taps(RATE, 8000, dev))
    host, counts = data.cpu().numpy(), out_len.cpu().tolist()
    for i, (o, m, y) in enumerate(zip(out_off, counts, want)):
        assert host[o:o + m].tobytes() == y.tobytes(), i


def test_finish_requests_makes_one_prosody_call_for_the_batch():
    dev = torch.device("cuda:0")
    reqs, flags, opts, targets, keys = _chunk_requests()
    on_dev = [[torch.from_numpy(c).to(dev) for c in r] for r in reqs]
    keywords = dict(loudness=targets, tempo=[o[0] for o in opts], pitch=[o[1] for o in opts], keep_formants=[o[2] for o in opts], watermark=keys,
                    sample_rate=[None, 8000, None, None], encoding=[None, "mulaw", "flac", None])
    want = infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16", **keywords)
    infer.backend_stats.clear()
    _reset()
    got = infer.finish_requests(on_dev, ["x"] * len(reqs), FADE_S, flags, device_backend=True, want="pcm16", **keywords)
    stats = dict(infer.backend_stats)
    assert stats["device_requests"] == len(reqs) and stats["device_calls"] == 1 and stats.get("host_requests", 0) == 0
    assert stats["prosody_calls"] == 1 and stats["prosody_requests"] == 3 and stats["formant_requests"] == 2
    assert _counter("wave_prosody_launches") == 2 and _counter("wave_formant_launches") == 3 and _counter("wave_formant_requests") == 2
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and len(g) == len(w) and np.array_equal(g, w), i
    # without the flag the same batch is today's call
    _reset()
    plain = infer.finish_requests(on_dev, ["x"] * len(reqs), FADE_S, flags, device_backend=True, want="pcm16", **dict(keywords, keep_formants=None))
    assert _counter("wave_formant_launches") == 0 and _counter("wave_prosody_launches") == 2
    assert np.array_equal(plain[2], got[2]) and np.array_equal(plain[3], got[3]) and not np.array_equal(plain[0], got[0])


# ------------------------------------------------------------------------------------------------ end to end on a tiny model
@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


def test_infer_requests_with_kept_formants_in_one_micro_batch(hip_objects, tmp_path):
    """Plain requests with a kept pitch, a plain pitch, no option and a kept pitch with a tempo, and a script, in ONE micro-batch: the device
    back-end's results are the host's, with one `ops.wave_prosody` call, and each is `shift_pcm16` of what the batch gives without the
    options."""
    path = _prompt(tmp_path)
    text = TEXT[:110]
    script = f"{TEXT[:64]} [town] I live in town."
    voices = {"main": dict(ref_audio_path=path, ref_text=REF_TEXT), "town": dict(ref_audio=(synth.ref_audio(16000 * 2, seed=77, amp=0.02), 16000),
                                                                                  ref_text="Town speaks.")}
    opts = [dict(seed=7, pitch=4, keep_formants=True), dict(seed=7, pitch=-2, sample_rate=8000, encoding="mulaw"), dict(seed=7),
            dict(seed=7, tempo=0.9, pitch=-3, keep_formants=True, loudness=-20.0)]
    drop = infer.PROSODY_OPTIONS + infer.FORMANT_OPTIONS
    out = {}
    for backend, with_option in ((True, True), (False, True), (True, False)):
        mgr = serve.TTSManager(nfe_step=8, device_backend=backend).load(*hip_objects)
        try:
            voice, ref_text_n = mgr._voice(path, REF_TEXT)
            strip = (lambda o: {k: v for k, v in o.items() if k not in drop}) if not with_option else (lambda o: o)
            batch = [(voice, ref_text_n, text, strip(o)) for o in opts]
            segments = mgr._script_segments(script, voices, 0.5)
            batch += [infer.ScriptRequest(segments, strip(dict(seed=7, tempo=1.1, pitch=2, keep_formants=True)), 0.5)]
            _reset()
            infer.backend_stats.clear()
            out[backend, with_option] = mgr._run_batch(batch)
            if backend and with_option:
                assert infer.backend_stats["device_requests"] == len(batch) and infer.backend_stats.get("host_requests", 0) == 0
                assert infer.backend_stats["prosody_calls"] == 1 and infer.backend_stats["prosody_requests"] == 4 and infer.backend_stats["formant_requests"] == 3
                assert _counter("wave_prosody_launches") == 2 and _counter("wave_formant_launches") == 3 and _counter("wave_formant_requests") == 3
            else:
                assert _counter("wave_prosody_launches") == 0 and _counter("wave_formant_launches") == 0
        finally:
            mgr.close()
    dev, host, before = out[True, True], out[False, True], out[True, False]
    for i, (d, h) in enumerate(zip(dev, host)):
        h = h if h.dtype != np.float32 else infer.quantise_pcm16(h)                     # (the host back-end leaves a request without options as float32)
        assert d.dtype == h.dtype and len(d) == len(h) and np.array_equal(d, h), i
    assert np.array_equal(dev[2], before[2])                                            # the request without the options: as without the feature
    assert np.array_equal(dev[0], infer.shift_pcm16(before[0], 1.0, 4, keep_formants=True)) and len(dev[0]) == len(before[0])
    assert np.array_equal(dev[4], infer.shift_pcm16(before[4], 1.1, 2, keep_formants=True)) and len(dev[4]) == -(-len(before[4]) * 10 // 11)
