"""The provenance watermark's mark on the device (csrc/wave_mark.h, f5hip_wave_mark: the 24 kHz int16 PCM of a ragged batch of requests,
each flagged request marked in place with its key's carrier in two launches) against the host definition `wave_codec.mark_pcm16`, alone,
through `infer.finish_requests` with the device back-end, and through `TTSManager(device_backend=True)` on a tiny model.

Every comparison is equality of bytes: there is no tolerance anywhere."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, ops, serve, synth, torch_ops, wave_codec  # noqa: E402

import watermark_ref as ref  # noqa: E402
from test_gpu_request_knobs import ARCH, REF_TEXT, TEXT, VOCAB, _prompt  # noqa: E402

RATE = 24000
TILE = 32 * 240                                        # f5hip_wave_mark_tile(): checked below
FADE_S = infer.cross_fade_duration
FILLER = 23456
K1, K2 = 1, 0xDEADBEEF
# (length, key, device length or None): every length of the issue, an all-zero request, two unflagged requests in between, two keys, device
# lengths below the bound
BATCH = [(1, K1, None), (239, K2, None), (240, K1, None), (241, K1, 240), (480, K2, None), (3000, None, None), (TILE - 1, K1, None), (TILE, K2, None),
         (TILE + 1, K1, TILE), (5000, "zeros", None), (16383, K2, None), (9000, None, 4000), (16384, K1, None), (16385, K2, 16384), (40000, K1, 33001),
         (0, K1, None)]


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _requests():
    out = []
    for i, (n, key, cut) in enumerate(BATCH):
        if key == "zeros":
            out.append((np.zeros(n, dtype=np.int16), K1, cut))
        else:
            x = ref.host(max(n, 2), i)[:n] if i % 3 else np.random.default_rng(i).integers(-30000, 30000, n).astype(np.int16)
            out.append((np.ascontiguousarray(x), key, cut))
    return out


def _device(requests, misalign=0):
    """ops.wave_mark on ONE packed buffer with the requests at `wave_finish`'s 8-sample offsets (plus `misalign` samples) and a loud filler
    between them -> (the whole buffer afterwards, the buffer before, its offsets)."""
    dev = torch.device("cuda:0")
    offsets, off = [], misalign
    for x, _, _ in requests:
        offsets.append(off)
        off += (len(x) + 7) & ~7
    buf = np.full(off + 8, FILLER, dtype=np.int16)
    for o, (x, _, _) in zip(offsets, requests):
        buf[o:o + len(x)] = x
    pcm = torch.from_numpy(buf.copy()).to(dev)
    cuts = [len(x) if cut is None else cut for x, _, cut in requests]
    len_dev = None if all(cut is None for _, _, cut in requests) else torch.tensor(cuts, dtype=torch.int32, device=dev)
    assert ops.wave_mark(pcm, offsets, [len(x) for x, _, _ in requests], len_dev, [key for _, key, _ in requests]) is pcm
    return pcm.cpu().numpy(), buf, offsets


def _expect(requests, buf, offsets):
    """The buffer the host definition gives: a flagged request's (cut) samples marked, everything else as it was."""
    want = buf.copy()
    for o, (x, key, cut) in zip(offsets, requests):
        n = len(x) if cut is None else min(max(cut, 0), len(x))
        want[o:o + n] = wave_codec.mark_pcm16(x[:n], key)
    return want


def _compare(got, want, where):
    if not np.array_equal(got, want):
        raise AssertionError((where, "first differing sample", int(np.flatnonzero(got != want)[0])))


@pytest.fixture(scope="module")
def batch_run():
    requests = _requests()
    got, buf, offsets = _device(requests)
    return requests, got, buf, offsets


def test_ragged_batch_equals_the_host_definition_bit_for_bit(batch_run):
    """Marked bytes = `mark_pcm16`; the sentinel gaps, the unflagged requests and the samples past a device length keep their bits."""
    assert ops.wave_mark_tile() == TILE
    requests, got, buf, offsets = batch_run
    want = _expect(requests, buf, offsets)
    _compare(got, want, "batch")
    changed = [not np.array_equal(got[o:o + len(x)], x) for o, (x, _, _) in zip(offsets, requests)]
    assert changed == [key is not None and len(x) > 0 and bool(x.any()) for x, key, _ in requests]
    assert not got[offsets[9]:offsets[9] + 5000].any()                                  # zeros stay zeros
    for o, (x, key, cut) in zip(offsets, requests):
        if cut is not None:
            assert np.array_equal(got[o + cut:o + len(x)], x[cut:])                     # past the device length: not written


def test_each_request_equals_its_single_request_call(batch_run):
    requests, got, _, offsets = batch_run
    for i, (o, (x, key, cut)) in enumerate(zip(offsets, requests)):
        if key is None:
            continue
        solo, _, _ = _device([requests[i]])
        assert np.array_equal(solo[:len(x)], got[o:o + len(x)]), i
    back, _, boff = _device(requests[::-1])
    for i, (o, (x, _, _)) in enumerate(zip(offsets, requests)):
        j = len(requests) - 1 - i
        assert np.array_equal(back[boff[j]:boff[j] + len(x)], got[o:o + len(x)]), i


def test_misaligned_samples_take_the_scalar_path():
    """Requests that do not start at a multiple of 8 samples (the C ABI asks for 2-byte alignment only): the same bytes."""
    requests = [r for r in _requests() if r[1] is not None][:9]
    for shift in (1, 3):
        got, buf, offsets = _device(requests, misalign=shift)
        _compare(got, _expect(requests, buf, offsets), ("misaligned", shift))


def test_two_launches_per_call_and_none_without_a_flag():
    requests = _requests()
    _device(requests[:1])                                                               # (the first call of a process also allocates)
    flagged = sum(key is not None for _, key, _ in requests)
    for batch, marked in ((requests[:1], 1), (requests, flagged), (requests[5:6] + requests[14:15], 1)):
        _reset()
        _device(batch)
        assert _counter("wave_mark_launches") == 2 and _counter("wave_mark_requests") == marked
        assert _counter("wave_loudness_launches") == 0 and _counter("wave_finish_launches") == 0 and _counter("wave_encode_launches") == 0
    _reset()
    none = [(x, None, cut) for x, _, cut in requests]
    got, buf, _ = _device(none)
    assert np.array_equal(got, buf)
    # the library itself, without the binding's shortcut: a call without a flagged request returns 0 and launches nothing
    pcm = torch.full((256,), FILLER, device="cuda:0", dtype=torch.int16)
    io, ml, ki = np.zeros(1, dtype=np.int64), np.array([200], dtype=np.int32), np.array([-1], dtype=np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    assert _lib.lib().f5hip_wave_mark(1, C.c_void_p(pcm.data_ptr()), p(io), p(ml), None, p(ki), None, 0, _lib.current_stream_ptr()) == 0
    assert _counter("wave_mark_launches") == 0 and _counter("wave_mark_requests") == 0
    assert (pcm == FILLER).all()


def test_ctypes_and_torch_op_paths_agree(batch_run):
    requests, got, _, _ = batch_run
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        again, _, _ = _device(requests)
    finally:
        torch_ops._loaded = True
    assert np.array_equal(got, again)


def test_carriers_are_uploaded_once_per_key_and_device():
    dev = torch.device("cuda:0")
    a = ops.watermark_carriers([K1], dev)
    assert a.dtype == torch.int16 and tuple(a.shape) == (1, 16384) and a.data_ptr() == ops.watermark_carriers([K1], dev).data_ptr()
    both = ops.watermark_carriers([K1, K2], dev)
    assert np.array_equal(both.cpu().numpy(), np.stack([wave_codec.watermark_carrier(K1), wave_codec.watermark_carrier(K2)]))
    assert len(wave_codec._carriers_on_device) <= wave_codec.TAP_TABLE_CACHE


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    pcm = torch.zeros(4096, device=dev, dtype=torch.int16)
    lens = torch.zeros(4, device=dev, dtype=torch.int32)
    carriers = ops.watermark_carriers([K1, K2], dev)

    def call(max_len=(100,), key=(0,), n=None, pcm_p=pcm.data_ptr(), car_p=carriers.data_ptr(), n_keys=2, len_p=None, in_p=True, ml_p=True, ki_p=True, in_off=None):
        ml, ki = np.asarray(max_len, dtype=np.int32), np.asarray(key, dtype=np.int32)
        io = np.zeros(len(ml), dtype=np.int64) if in_off is None else np.asarray(in_off, dtype=np.int64)
        p = lambda a, on: C.c_void_p(a.ctypes.data) if on else None   # noqa: E731
        return lib.f5hip_wave_mark(len(ml) if n is None else n, C.c_void_p(pcm_p), p(io, in_p), p(ml, ml_p), C.c_void_p(len_p) if len_p else None,
                                   p(ki, ki_p), C.c_void_p(car_p) if car_p else None, n_keys, _lib.current_stream_ptr())

    _reset()
    assert call(n=0) != 0 and b"bad argument" in lib.f5hip_last_error()
    for null in (dict(pcm_p=None), dict(in_p=False), dict(ml_p=False), dict(ki_p=False)):
        assert call(**null) != 0 and b"bad argument" in lib.f5hip_last_error(), null
    assert call(car_p=None) != 0 and b"carriers" in lib.f5hip_last_error()
    assert call(car_p=carriers.data_ptr() + 8) != 0 and b"aligned" in lib.f5hip_last_error()
    assert call(max_len=(-1,)) != 0 and b"negative" in lib.f5hip_last_error()
    assert call(in_off=(-8,)) != 0 and b"negative" in lib.f5hip_last_error()
    assert call(pcm_p=pcm.data_ptr() + 1) != 0 and b"aligned" in lib.f5hip_last_error()
    assert call(len_p=lens.data_ptr() + 2) != 0 and b"aligned" in lib.f5hip_last_error()
    for bad in (2, -2):
        assert call(key=(bad,)) != 0 and b"names key" in lib.f5hip_last_error(), bad
    for bad in (-1, 17):
        assert call(n_keys=bad) != 0 and b"keys in a call" in lib.f5hip_last_error(), bad
    assert call(max_len=(2 ** 31 - 1, 2 ** 31 - 1), key=(0, 1)) != 0 and b"2^31" in lib.f5hip_last_error()              # (refused unread)
    with pytest.raises(_lib.F5HipError):
        ops.wave_mark(pcm, [4000], [100], None, [K1])                                   # covers samples past the tensor
    with pytest.raises(_lib.F5HipError, match="int16"):
        ops.wave_mark(pcm.to(torch.int32), [0], [100], None, [K1])
    with pytest.raises(_lib.F5HipError, match="integer key"):
        ops.wave_mark(pcm, [0], [100], None, [1.5])
    with pytest.raises(_lib.F5HipError, match="one value per request"):
        ops.wave_mark(pcm, [0], [100], None, [K1, K2])
    with pytest.raises(_lib.F5HipError, match="distinct keys"):
        ops.wave_mark(pcm, [0] * 17, [8] * 17, None, list(range(1, 18)))
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)   # noqa: E731
    with pytest.raises(RuntimeError, match="one value per request"):
        torch.ops.f5hip.wave_mark(pcm, torch.zeros(1, dtype=torch.int64), i32(100), None, i32(0, 0), carriers)
    with pytest.raises(RuntimeError, match="names key"):
        torch.ops.f5hip.wave_mark(pcm, torch.zeros(1, dtype=torch.int64), i32(100), None, i32(2), carriers)
    with pytest.raises(RuntimeError, match="carriers must be"):
        torch.ops.f5hip.wave_mark(pcm, torch.zeros(1, dtype=torch.int64), i32(100), None, i32(0), carriers[:, :100].contiguous())
    assert _counter("wave_mark_launches") == 0 and _counter("wave_mark_requests") == 0
    assert call() == 0 and _counter("wave_mark_launches") == 2 and _counter("wave_mark_requests") == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ between wave_prosody and wave_loudness
def _chunk_requests():
    noise = lambda n, s, amp: (amp * np.random.default_rng(s).standard_normal(n)).astype(np.float32)   # noqa: E731
    speech = lambda n, s: (ref.host(n, s).astype(np.float32) / 32768.0)   # noqa: E731
    pause = np.concatenate([speech(2 * RATE, 1), np.zeros(int(2.5 * RATE), np.float32), speech(2 * RATE, 2)])
    return [[pause], [speech(19003, 5), speech(17201, 6)], [noise(30011, 7, 0.004)], [speech(20000, 8)], [speech(19003, 5), speech(17201, 6)], [noise(30011, 7, 0.1)]]


def test_finish_requests_makes_one_mark_call_and_no_copy_for_it():
    """A mixed batch -- marked with silence removal, with a tempo, with a loudness target, as 8 kHz mu-law and as FLAC, between unmarked
    neighbours -- equals the host `finish_pcm16` byte for byte, in one `ops.wave_mark` call, with the copies of the same batch unmarked."""
    dev = torch.device("cuda:0")
    reqs = _chunk_requests()
    flags = [True, False, False, False, False, False]
    keys = [K1, K2, None, K1, K1, None]
    options = dict(sample_rate=[None, 8000, None, None, None, 44100], encoding=[None, "mulaw", None, None, "flac", "flac"],
                   loudness=[-23.0, None, -30.0, -16.0, None, None], tempo=[None, 1.25, None, None, 0.8, None], pitch=[None, None, None, 2, None, None])
    on_dev = [[torch.from_numpy(c).to(dev) for c in r] for r in reqs]
    want = infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16", watermark=keys, **options)
    unmarked = infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16", **options)
    copies = {}
    for with_option in (False, True):
        infer.backend_stats.clear()
        _reset()
        got = infer.finish_requests(on_dev, ["x"] * len(reqs), FADE_S, flags, device_backend=True, want="pcm16", watermark=keys if with_option else None,
                                    **options)
        stats = dict(infer.backend_stats)
        copies[with_option] = stats["d2h_copies"]
        assert stats["device_requests"] == len(reqs) and stats["device_calls"] == 1 and stats.get("host_requests", 0) == 0
        if with_option:
            assert stats["mark_calls"] == 1 and stats["mark_requests"] == 4
            assert _counter("wave_mark_launches") == 2 and _counter("wave_mark_requests") == 4
        else:
            assert "mark_calls" not in stats and _counter("wave_mark_launches") == 0
            for i, (g, w) in enumerate(zip(got, unmarked)):
                assert g.dtype == w.dtype and np.array_equal(g, w), i
    assert copies[True] == copies[False]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and len(g) == len(w) and np.array_equal(g, w), i
    for i, key in enumerate(keys):
        assert np.array_equal(want[i], unmarked[i]) == (key is None), i
    spec = infer.WaveSpec.of(dict(loudness=-16.0, pitch=2))
    assert np.array_equal(got[3], infer.finish_pcm16(infer.quantise_pcm16(reqs[3][0]), dataclasses.replace(spec, watermark=K1)))
    assert wave_codec.detect_watermark(got[3], [K1])[0].detected


# ------------------------------------------------------------------------------------------------ end to end on a tiny model
@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


def test_manager_batch_with_marks_in_one_micro_batch(hip_objects, tmp_path):
    """Through `TTSManager(device_backend=True)`: marked requests (plain, with a tempo and a loudness target, as 8 kHz mu-law, as FLAC, a
    script) and unmarked neighbours in ONE micro-batch equal the host back-end byte for byte, with one `ops.wave_mark` call and no device-
    to-host copy more than the same batch unmarked."""
    path = _prompt(tmp_path)
    text = TEXT[:110]
    script = f"{TEXT[:64]} [town] I live in town."
    voices = {"main": dict(ref_audio_path=path, ref_text=REF_TEXT), "town": dict(ref_audio=(synth.ref_audio(16000 * 2, seed=77, amp=0.02), 16000),
                                                                                  ref_text="Town speaks.")}
    opts = [dict(seed=7, watermark=K1), dict(seed=7), dict(seed=7, watermark=K2, tempo=1.25, loudness=-20.0), dict(seed=7, watermark=K1, sample_rate=8000, encoding="mulaw"),
            dict(seed=7, sample_rate=8000, encoding="mulaw"), dict(seed=7, watermark=K1, encoding="flac")]
    out, copies = {}, {}
    for backend, with_option in ((True, True), (False, True), (True, False)):
        mgr = serve.TTSManager(nfe_step=8, device_backend=backend).load(*hip_objects)
        try:
            voice, ref_text_n = mgr._voice(path, REF_TEXT)
            strip = (lambda o: {k: v for k, v in o.items() if k != "watermark"}) if not with_option else (lambda o: o)
            batch = [(voice, ref_text_n, text, strip(o)) for o in opts]
            segments = mgr._script_segments(script, voices, 0.5)
            batch += [infer.ScriptRequest(segments, strip(dict(seed=7, watermark=K2)), 0.5)]
            _reset()
            infer.backend_stats.clear()
            out[backend, with_option] = mgr._run_batch(batch)
            copies[backend, with_option] = infer.backend_stats["d2h_copies"]
            if backend and with_option:
                assert infer.backend_stats["device_requests"] == len(batch) and infer.backend_stats.get("host_requests", 0) == 0
                assert infer.backend_stats["mark_calls"] == 1 and infer.backend_stats["mark_requests"] == 5
                assert _counter("wave_mark_launches") == 2 and _counter("wave_mark_requests") == 5
            else:
                assert _counter("wave_mark_launches") == 0
        finally:
            mgr.close()
    dev, host, before = out[True, True], out[False, True], out[True, False]
    assert copies[True, True] == copies[True, False]
    for i, (d, h) in enumerate(zip(dev, host)):
        h = h if h.dtype != np.float32 else infer.quantise_pcm16(h)                     # (the host back-end leaves a request without options as float32)
        assert d.dtype == h.dtype and len(d) == len(h) and np.array_equal(d, h), i
    for i in (1, 4):
        assert np.array_equal(dev[i], before[i]), i                                     # the unmarked neighbours: as without the feature
    assert np.array_equal(dev[0], wave_codec.mark_pcm16(before[0], K1)) and not np.array_equal(dev[0], before[0])
    assert np.array_equal(dev[6], wave_codec.mark_pcm16(before[6], K2))                 # the script: marked as one joined wave
    assert np.array_equal(infer.decode_flac(dev[5])[0], wave_codec.mark_pcm16(before[0], K1))   # the FLAC stream holds the marked samples
