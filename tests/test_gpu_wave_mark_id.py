"""The watermark's trace ids on the device, embedding (csrc/wave_mark.h, f5hip_wave_mark_ids: the 24 kHz int16 PCM of a ragged batch of
requests, each flagged request marked in place with its key's carrier and, with an id, its three rotated sub-key carriers, in two launches)
against the host definition `wave_codec.mark_pcm16` of a `WatermarkTag`, alone, through `infer.finish_requests` with the device back-end, and
through `TTSManager(device_backend=True)` on a tiny model.

Every comparison is equality of bytes: there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, ops, serve, synth, torch_ops, wave_codec  # noqa: E402
from tts_indic_server_f5_amd.wave_codec import WatermarkTag  # noqa: E402

import watermark_ref as ref  # noqa: E402
from test_gpu_request_knobs import REF_TEXT, TEXT, _prompt  # noqa: E402
from test_gpu_wave_mark import FADE_S, FILLER, K1, K2, TILE, _chunk_requests, _compare, _counter, _reset, hip_objects  # noqa: E402,F401

S = lambda s0, s1, s2: s0 | s1 << 10 | s2 << 20   # noqa: E731  (an id from its three symbols)
MIXED = 0x2A5F3C91
# (length, key, id or None, device length or None): every length of the issue, an all-zero request, requests with an id, with a key only and
# with neither, two keys, symbols 0, 1 and 1023 in each position, device lengths below the bound
BATCH = [(1, K1, S(0, 1, 1023), None), (239, K2, S(1, 1023, 0), None), (240, K1, S(1023, 0, 1), None), (241, K1, MIXED, 240), (480, K2, None, None),
         (3000, None, None, None), (TILE - 1, K1, 0, None), (TILE, K2, 2 ** 30 - 1, None), (TILE + 1, K1, S(1, 1, 1), TILE), (5000, "zeros", MIXED, None),
         (16383, K2, S(0, 0, 1023), None), (9000, None, None, 4000), (16384, K1, None, None), (16385, K2, S(1023, 1, 0), 16384), (40000, K1, MIXED, 33001),
         (0, K1, 5, None)]


def _mark(key, tag):
    return key if key is None or tag is None else WatermarkTag(key, tag)


def _requests():
    out = []
    for i, (n, key, tag, cut) in enumerate(BATCH):
        if key == "zeros":
            out.append((np.zeros(n, dtype=np.int16), _mark(K1, tag), cut))
        else:
            x = ref.host(max(n, 2), i)[:n] if i % 3 else np.random.default_rng(i).integers(-30000, 30000, n).astype(np.int16)
            out.append((np.ascontiguousarray(x), _mark(key, tag), cut))
    return out


def _device(requests, misalign=None):
    """ops.wave_mark on ONE packed buffer with the requests at `wave_finish`'s 8-sample offsets and a loud filler between them; request
    `misalign` starts one sample late (an odd sample offset: the scalar path) -> (the whole buffer afterwards, the buffer before, its offsets)."""
    dev = torch.device("cuda:0")
    offsets, off = [], 0
    for i, (x, _, _) in enumerate(requests):
        offsets.append(off + (i == misalign))
        off += ((len(x) + 7) & ~7) + 8 * (i == misalign)
    buf = np.full(off + 8, FILLER, dtype=np.int16)
    for o, (x, _, _) in zip(offsets, requests):
        buf[o:o + len(x)] = x
    pcm = torch.from_numpy(buf.copy()).to(dev)
    cuts = [len(x) if cut is None else cut for x, _, cut in requests]
    len_dev = None if all(cut is None for _, _, cut in requests) else torch.tensor(cuts, dtype=torch.int32, device=dev)
    assert ops.wave_mark(pcm, offsets, [len(x) for x, _, _ in requests], len_dev, [mark for _, mark, _ in requests]) is pcm
    return pcm.cpu().numpy(), buf, offsets


def _expect(requests, buf, offsets):
    """The buffer the host definition gives: a flagged request's (cut) samples marked, everything else as it was."""
    want = buf.copy()
    for o, (x, mark, cut) in zip(offsets, requests):
        n = len(x) if cut is None else min(max(cut, 0), len(x))
        want[o:o + n] = wave_codec.mark_pcm16(x[:n], mark)
    return want


@pytest.fixture(scope="module")
def batch_run():
    requests = _requests()
    _reset()
    got, buf, offsets = _device(requests, misalign=6)                                  # the request of TILE - 1 samples starts at an odd offset
    return requests, got, buf, offsets, (_counter("wave_mark_id_launches"), _counter("wave_mark_id_requests"), _counter("wave_mark_launches"))


def test_ragged_batch_equals_the_host_definition_bit_for_bit(batch_run):
    """Marked bytes = `mark_pcm16` of the request's tag or key; the sentinel gaps, the unflagged requests and the samples past a device length
    keep their bits; two launches for the call, counted on the id counters."""
    assert ops.wave_mark_tile() == TILE
    requests, got, buf, offsets, counters = batch_run
    assert offsets[6] % 2 == 1
    _compare(got, _expect(requests, buf, offsets), "batch")
    changed = [not np.array_equal(got[o:o + len(x)], x) for o, (x, _, _) in zip(offsets, requests)]
    assert changed == [mark is not None and len(x) > 0 and bool(x.any()) for x, mark, _ in requests]
    assert not got[offsets[9]:offsets[9] + 5000].any()                                  # zeros stay zeros
    for o, (x, _, cut) in zip(offsets, requests):
        if cut is not None:
            assert np.array_equal(got[o + cut:o + len(x)], x[cut:])                     # past the device length: not written
    assert counters == (2, sum(mark is not None for _, mark, _ in requests), 0)
    x, mark, _ = requests[14]                                                           # an id changes the bytes, and a key alone is `wave_mark`'s
    assert not np.array_equal(got[offsets[14]:offsets[14] + 33001], wave_codec.mark_pcm16(x[:33001], K1))
    assert np.array_equal(got[offsets[12]:offsets[12] + 16384], wave_codec.mark_pcm16(requests[12][0], K1))


def test_each_request_equals_its_single_request_call(batch_run):
    requests, got, _, offsets, _ = batch_run
    for i, (o, (x, mark, _)) in enumerate(zip(offsets, requests)):
        if mark is None:
            continue
        solo, _, _ = _device([requests[i]])
        assert np.array_equal(solo[:len(x)], got[o:o + len(x)]), i
    back, _, boff = _device(requests[::-1])
    for i, (o, (x, _, _)) in enumerate(zip(offsets, requests)):
        j = len(requests) - 1 - i
        assert np.array_equal(back[boff[j]:boff[j] + len(x)], got[o:o + len(x)]), i


def test_ctypes_and_torch_op_paths_agree(batch_run):
    requests, got, _, _, _ = batch_run
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        again, _, _ = _device(requests, misalign=6)
    finally:
        torch_ops._loaded = True
    assert np.array_equal(got, again)


def test_a_call_without_an_id_is_wave_mark(batch_run):
    """Keys only: `ops.wave_mark`'s bytes and only its counters; the library's id entry with every id -1 likewise."""
    requests = [(x, wave_codec.watermark_key(mark), cut) for x, mark, cut in batch_run[0]]
    _reset()
    got, buf, offsets = _device(requests)
    _compare(got, _expect(requests, buf, offsets), "keys only")
    flagged = sum(key is not None for _, key, _ in requests)
    assert (_counter("wave_mark_launches"), _counter("wave_mark_requests")) == (2, flagged)
    assert (_counter("wave_mark_id_launches"), _counter("wave_mark_id_requests")) == (0, 0)
    dev = torch.device("cuda:0")
    keys = [k for k in (K1, K2)]
    pcm = torch.from_numpy(buf.copy()).to(dev)
    io, ml = np.asarray(offsets, dtype=np.int64), np.asarray([len(x) for x, _, _ in requests], dtype=np.int32)
    ki = np.asarray([-1 if key is None else keys.index(key) for _, key, _ in requests], dtype=np.int32)
    ids = np.full(len(requests), -1, dtype=np.int32)
    cuts = torch.tensor([len(x) if cut is None else cut for x, _, cut in requests], dtype=torch.int32, device=dev)
    carriers = ops.watermark_tag_carriers(keys, dev)
    assert tuple(carriers.shape) == (2, 4, 16384) and np.array_equal(carriers[1, 2].cpu().numpy(), wave_codec.watermark_carrier(wave_codec.watermark_subkey(K2, 1)))
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    _reset()
    rc = _lib.lib().f5hip_wave_mark_ids(len(requests), C.c_void_p(pcm.data_ptr()), p(io), p(ml), C.c_void_p(cuts.data_ptr()), p(ki), p(ids),
                                        C.c_void_p(carriers.data_ptr()), 2, _lib.current_stream_ptr())
    assert rc == 0, _lib.lib().f5hip_last_error()
    assert np.array_equal(pcm.cpu().numpy(), got)
    assert (_counter("wave_mark_launches"), _counter("wave_mark_requests")) == (2, flagged)
    assert (_counter("wave_mark_id_launches"), _counter("wave_mark_id_requests")) == (0, 0)


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    pcm = torch.full((4096,), FILLER, device=dev, dtype=torch.int16)
    carriers = ops.watermark_tag_carriers([K1, K2], dev)

    def call(key=(0,), tag=(5,), ids=True, n_keys=2):
        ml, ki, it = np.full(len(key), 100, dtype=np.int32), np.asarray(key, dtype=np.int32), np.asarray(tag, dtype=np.int32)
        io = np.zeros(len(ml), dtype=np.int64)
        p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        return lib.f5hip_wave_mark_ids(len(ml), C.c_void_p(pcm.data_ptr()), p(io), p(ml), None, p(ki), p(it) if ids else None,
                                       C.c_void_p(carriers.data_ptr()), n_keys, _lib.current_stream_ptr())

    _reset()
    assert call(ids=False) != 0 and b"bad argument" in lib.f5hip_last_error()
    assert call(key=(-1,)) != 0 and b"an id and no key" in lib.f5hip_last_error()      # an id on a request that is left alone
    for bad in (-2, 2 ** 30):
        assert call(tag=(bad,)) != 0 and b"has id" in lib.f5hip_last_error(), bad
    assert call(key=(2,)) != 0 and b"names key" in lib.f5hip_last_error()
    assert call(n_keys=17) != 0 and b"keys in a call" in lib.f5hip_last_error()
    with pytest.raises(_lib.F5HipError, match="watermark id must be"):
        ops.wave_mark(pcm, [0], [100], None, [{"key": K1, "id": 2 ** 30}])
    with pytest.raises(_lib.F5HipError, match="id without a key"):
        ops.wave_mark(pcm, [0], [100], None, [{"id": 1}])
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)   # noqa: E731
    zero = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="an id and no key"):
        torch.ops.f5hip.wave_mark_ids(pcm, zero, i32(100), None, i32(-1), i32(5), carriers)
    with pytest.raises(RuntimeError, match="has id"):
        torch.ops.f5hip.wave_mark_ids(pcm, zero, i32(100), None, i32(0), i32(2 ** 30), carriers)
    with pytest.raises(RuntimeError, match="one value per request"):
        torch.ops.f5hip.wave_mark_ids(pcm, zero, i32(100), None, i32(0), i32(1, 2), carriers)
    with pytest.raises(RuntimeError, match="carriers must be"):
        torch.ops.f5hip.wave_mark_ids(pcm, zero, i32(100), None, i32(0), i32(1), carriers.reshape(8, 16384))
    assert _counter("wave_mark_id_launches") == 0 and _counter("wave_mark_launches") == 0
    assert (pcm == FILLER).all()
    assert call() == 0 and _counter("wave_mark_id_launches") == 2 and _counter("wave_mark_id_requests") == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ between wave_prosody and wave_loudness
def test_finish_requests_makes_one_mark_call_and_no_copy_more_than_keys_alone():
    """A mixed batch -- tagged, key-only and unmarked requests with silence removal, a tempo, a loudness target, as 8 kHz mu-law and as
    FLAC -- equals the host `finish_pcm16` byte for byte, in one `ops.wave_mark` call, with the copies of the same batch marked by keys alone."""
    dev = torch.device("cuda:0")
    reqs = _chunk_requests()
    flags = [True, False, False, False, False, False]
    marks = [WatermarkTag(K1, MIXED), {"key": K2, "id": 1023}, None, K1, WatermarkTag(K1, 0), None]
    keys = [wave_codec.watermark_key(wave_codec.check_watermark(m)) for m in marks]
    options = dict(sample_rate=[None, 8000, None, None, None, 44100], encoding=[None, "mulaw", None, None, "flac", "flac"],
                   loudness=[-23.0, None, -30.0, -16.0, None, None], tempo=[None, 1.25, None, None, 0.8, None], pitch=[None, None, None, 2, None, None])
    on_dev = [[torch.from_numpy(c).to(dev) for c in r] for r in reqs]
    want = infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16", watermark=marks, **options)
    keyed = infer.finish_requests(reqs, ["x"] * len(reqs), FADE_S, flags, want="pcm16", watermark=keys, **options)
    copies = {}
    for tagged in (False, True):
        infer.backend_stats.clear()
        _reset()
        got = infer.finish_requests(on_dev, ["x"] * len(reqs), FADE_S, flags, device_backend=True, want="pcm16", watermark=marks if tagged else keys, **options)
        stats = dict(infer.backend_stats)
        copies[tagged] = stats["d2h_copies"]
        assert stats["device_requests"] == len(reqs) and stats["device_calls"] == 1 and stats.get("host_requests", 0) == 0
        assert stats["mark_calls"] == 1 and stats["mark_requests"] == 4
        assert (_counter("wave_mark_id_launches"), _counter("wave_mark_id_requests")) == ((2, 4) if tagged else (0, 0))
        assert (_counter("wave_mark_launches"), _counter("wave_mark_requests")) == ((0, 0) if tagged else (2, 4))
        for i, (g, w) in enumerate(zip(got, want if tagged else keyed)):
            assert g.dtype == w.dtype and len(g) == len(w) and np.array_equal(g, w), (tagged, i)
    assert copies[True] == copies[False]
    for i, mark in enumerate(marks):
        assert np.array_equal(want[i], keyed[i]) == (not isinstance(wave_codec.check_watermark(mark), WatermarkTag)), i
    got0 = wave_codec.read_watermark(got[0], [K1])[0]
    assert got0.detected and got0.id == MIXED


# ------------------------------------------------------------------------------------------------ end to end on a tiny model
def test_manager_batch_with_tags_in_one_micro_batch(hip_objects, tmp_path):  # noqa: F811
    """Through `TTSManager(device_backend=True)` with a key of its own: requests with an id of their own, with the manager's key alone, with
    another key and a script in ONE micro-batch equal the host back-end byte for byte, with one `ops.wave_mark` call and no device-to-host
    copy more than the same batch marked by keys alone."""
    path = _prompt(tmp_path)
    text = TEXT[:110]
    script = f"{TEXT[:64]} [town] I live in town."
    voices = {"main": dict(ref_audio_path=path, ref_text=REF_TEXT), "town": dict(ref_audio=(synth.ref_audio(16000 * 2, seed=77, amp=0.02), 16000),
                                                                                  ref_text="Town speaks.")}
    opts = [dict(seed=7, watermark={"id": 77}), dict(seed=7), dict(seed=7, watermark={"key": K2, "id": MIXED}, tempo=1.25, loudness=-20.0),
            dict(seed=7, watermark={"id": 1023}, sample_rate=8000, encoding="mulaw"), dict(seed=7, watermark=K2, encoding="flac")]
    key_only = lambda o: dict(o, watermark=wave_codec.watermark_key(o["watermark"])) if "watermark" in o else o   # noqa: E731
    out, copies = {}, {}
    for backend, tagged in ((True, True), (False, True), (True, False)):
        mgr = serve.TTSManager(nfe_step=8, device_backend=backend, watermark=K1).load(*hip_objects)
        try:
            voice, ref_text_n = mgr._voice(path, REF_TEXT)
            checked = [mgr.request_options(**o) for o in opts] + [mgr.request_options(seed=7, watermark={"id": 5})]
            assert [o["watermark"] for o in checked] == [WatermarkTag(K1, 77), K1, WatermarkTag(K2, MIXED), WatermarkTag(K1, 1023), K2, WatermarkTag(K1, 5)]
            checked = checked if tagged else [key_only(o) for o in checked]
            batch = [(voice, ref_text_n, text, o) for o in checked[:-1]]
            batch += [infer.ScriptRequest(mgr._script_segments(script, voices, 0.5), checked[-1], 0.5)]
            _reset()
            infer.backend_stats.clear()
            out[backend, tagged] = mgr._run_batch(batch)
            copies[backend, tagged] = infer.backend_stats["d2h_copies"]
            if backend:
                assert infer.backend_stats["device_requests"] == len(batch) and infer.backend_stats.get("host_requests", 0) == 0
                assert infer.backend_stats["mark_calls"] == 1 and infer.backend_stats["mark_requests"] == len(batch)
                assert (_counter("wave_mark_id_launches"), _counter("wave_mark_id_requests")) == ((2, len(batch)) if tagged else (0, 0))
                assert (_counter("wave_mark_launches"), _counter("wave_mark_requests")) == ((0, 0) if tagged else (2, len(batch)))
            else:
                assert _counter("wave_mark_launches") == 0 and _counter("wave_mark_id_launches") == 0
        finally:
            mgr.close()
    dev, host, keyed = out[True, True], out[False, True], out[True, False]
    assert copies[True, True] == copies[True, False]
    for i, (d, h) in enumerate(zip(dev, host)):
        assert d.dtype == h.dtype and len(d) == len(h) and np.array_equal(d, h), i
    for i in (1, 4):
        assert np.array_equal(dev[i], keyed[i]), i                                      # the key-only neighbours: `wave_mark`'s bytes
    assert not np.array_equal(dev[0], keyed[0]) and not np.array_equal(dev[5], keyed[5])      # an id changes the bytes (the tiny model's output is not speech: nothing is read back here)
