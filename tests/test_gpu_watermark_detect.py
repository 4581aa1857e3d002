"""The provenance watermark's detector on the device (csrc/wave_mark.h, f5hip_watermark_detect: a ragged batch of mono 24 kHz fp32 clips
scored against every key in four launches) against the host definition `wave_codec.detect_watermark` (fp64), and `reject_marked` through a
manager with the device front-end.

A clip's rows equal its single-clip call's bit for bit and the input is never written: equality of bytes.  Against the fp64 host the
decision `detected` must be the host's for every clip (all chosen with the host's z outside 7 +- 0.5), the offset wherever the host's z >= 10,
and |z_dev - z_host| stays within 8 x the maximum measured over these clips on the first run on an MI355X (DZ_MEASURED; room for another
FFT and summation order), never above 0.05: a difference beyond that is not rounding."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, ops, serve, synth, wave_codec  # noqa: E402

import watermark_ref as ref  # noqa: E402
from test_gpu_request_knobs import ARCH, VOCAB  # noqa: E402

RATE = 24000
K1, K2, K3 = 1, 0xDEADBEEF, 2 ** 47 + 5
DZ_MEASURED = 3.37e-5                                  # max |z_dev - z_host| over CLIPS x (1 key, 3 keys), MI355X: profiles/watermark_bench.txt
DZ_BOUND = min(8 * DZ_MEASURED, 0.05)
FILLER = 0.123


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _clips():
    """11 999 (below the minimum), 12 000, 16 384, 16 385, 24 000 and 50 000 samples: marked, unmarked or marked with another key; one cut
    out of a longer marked wave (offset 5000), two in 25 dB white noise."""
    m = lambda n, s, k: wave_codec.mark_pcm16(ref.host(n, s), k)   # noqa: E731
    pcm = [m(11999, 1, K1), m(12000, 2, K1), ref.host(16384, 3), m(16385, 4, K2), m(40000, 5, K1)[5000:29000],
           wave_codec.mark_pcm16(ref.host(50000, 6, True), K3), ref.host(24000, 7, True)]
    return [(x.astype(np.float32) / np.float32(32768.0)) for x in pcm]


@pytest.fixture(scope="module")
def clips():
    return _clips()


@pytest.fixture(scope="module")
def host_scores(clips):
    """The fp64 definition, once: [clip][key] over the three keys (a key's score does not depend on the other keys of the call)."""
    return [wave_codec.detect_watermark(x, [K1, K2, K3]) for x in clips]


def _device(clips, keys):
    """ops.watermark_detect on ONE packed buffer with a filler between the clips -> (score rows [n, n_keys, 4], the buffer afterwards, the
    buffer before)."""
    dev = torch.device("cuda:0")
    offsets, off = [], 3
    for x in clips:
        offsets.append(off)
        off += len(x) + 5
    buf = np.full(off, FILLER, dtype=np.float32)
    for o, x in zip(offsets, clips):
        buf[o:o + len(x)] = x
    wave = torch.from_numpy(buf.copy()).to(dev)
    rows = ops.watermark_detect(wave, offsets, [len(x) for x in clips], ops.watermark_carriers(keys, dev))
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (len(clips), len(keys), 4)
    return rows.cpu().numpy(), wave.cpu().numpy(), buf


@pytest.fixture(scope="module")
def runs(clips):
    return {keys: _device(clips, list(keys)) for keys in ((K1,), (K1, K2, K3))}


@pytest.mark.parametrize("keys", [(K1,), (K1, K2, K3)], ids=["one_key", "three_keys"])
def test_decisions_offsets_and_scores_against_the_host(clips, host_scores, runs, keys):
    rows, after, before = runs[keys]
    assert after.tobytes() == before.tobytes()                                          # the input is never written
    worst = 0.0
    for i, x in enumerate(clips):
        got = ops.watermark_scores(rows[i], list(keys))
        for g, key in zip(got, keys):
            h = host_scores[i][(K1, K2, K3).index(key)]
            assert abs(h.z - wave_codec.WATERMARK_THRESHOLD) > 0.5 or h.z == 0.0
            print(f"clip {i} ({len(x)} samples) key {key:#x}: z_dev {g.z:.6f} z_host {h.z:.6f} dz {abs(g.z - h.z):.3e} offsets {g.offset} {h.offset}")
            worst = max(worst, abs(g.z - h.z))
            assert g.detected == h.detected, (i, key, g, h)
            if h.z >= 10:
                assert g.offset == h.offset, (i, key, g, h)
    print(f"max |z_dev - z_host| = {worst:.3e} (bound {DZ_BOUND:.3e})")
    assert worst <= DZ_BOUND, worst
    assert rows[0].tolist() == [[0.0] * 4] * len(keys)                                  # below WATERMARK_MIN_SAMPLES: zeros
    r_peak, sigma = rows[4][0][2], rows[4][0][3]
    assert sigma > 0 and r_peak / sigma > 10                                            # (r at the offset and the deviation come down too)


def test_a_key_does_not_depend_on_the_other_keys_of_the_call(runs):
    assert np.array_equal(runs[(K1,)][0][:, 0], runs[(K1, K2, K3)][0][:, 0])


def test_each_row_equals_its_single_clip_call(clips, runs):
    keys = (K1, K2, K3)
    rows = runs[keys][0]
    for i, x in enumerate(clips):
        solo, _, _ = _device([x], list(keys))
        assert solo[0].tobytes() == rows[i].tobytes(), i
    back, _, _ = _device(clips[::-1], list(keys))                                       # another order: other clip groups in the correlation launch
    assert back[::-1].tobytes() == rows.tobytes()
    five, _, _ = _device(clips[:5], list(keys))                                         # a last group that is not full
    assert five.tobytes() == rows[:5].tobytes()


def test_launch_count_as_declared(clips):
    lib = _lib.lib()
    assert lib.f5hip_watermark_detect_launches() == 4
    for batch, keys in ((clips[1:2], [K1]), (clips, [K1, K2, K3]), (clips[:5], [K2])):
        _reset()
        _device(batch, keys)
        assert _counter("watermark_detect_launches") == 4 and _counter("watermark_detect_clips") == len(batch)
        assert _counter("ref_denoise_launches") == 0 and _counter("wave_mark_launches") == 0


def test_both_bindings_agree(clips, runs):
    from tts_indic_server_f5_amd import torch_ops
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        again, _, _ = _device(clips, [K1, K2, K3])
    finally:
        torch_ops._loaded = True
    assert again.tobytes() == runs[(K1, K2, K3)][0].tobytes()


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    wave = torch.zeros(40000, device=dev, dtype=torch.float32)
    scores = torch.zeros(64, device=dev, dtype=torch.float32)
    carriers = ops.watermark_carriers([K1, K2], dev)

    def call(n_samples=(20000,), offset=None, n=None, n_keys=2, wave_p=wave.data_ptr(), car_p=carriers.data_ptr(), sc_p=scores.data_ptr(), off_p=True, ns_p=True):
        ns = np.asarray(n_samples, dtype=np.int32)
        off = np.zeros(len(ns), dtype=np.int64) if offset is None else np.asarray(offset, dtype=np.int64)
        p = lambda a, on: C.c_void_p(a.ctypes.data) if on else None   # noqa: E731
        return lib.f5hip_watermark_detect(len(ns) if n is None else n, C.c_void_p(wave_p) if wave_p else None, p(off, off_p), p(ns, ns_p), n_keys,
                                          C.c_void_p(car_p) if car_p else None, C.c_void_p(sc_p) if sc_p else None, _lib.current_stream_ptr())

    _reset()
    assert call(n=0) != 0 and b"at least one clip" in lib.f5hip_last_error()
    for null in (dict(wave_p=None), dict(car_p=None), dict(sc_p=None), dict(off_p=False), dict(ns_p=False)):
        assert call(**null) != 0 and b"bad argument" in lib.f5hip_last_error(), null
    for bad in (0, 17, -1):
        assert call(n_keys=bad) != 0 and b"keys in a call" in lib.f5hip_last_error(), bad
    for bad in (0, -5, wave_codec.WATERMARK_MAX_SAMPLES + 1):
        assert call(n_samples=(bad,)) != 0 and b"samples (1 .." in lib.f5hip_last_error(), bad
    assert call(offset=(-1,)) != 0 and b"starts at" in lib.f5hip_last_error()
    assert call(n_samples=(20000, 20000), offset=(0, 19999)) != 0 and b"overlaps" in lib.f5hip_last_error()
    assert call(car_p=carriers.data_ptr() + 8) != 0 and b"aligned" in lib.f5hip_last_error()
    assert call(wave_p=wave.data_ptr() + 2) != 0 and b"aligned" in lib.f5hip_last_error()
    c2 = ops.watermark_carriers([K1, K2], dev)
    with pytest.raises(_lib.F5HipError, match="samples"):
        ops.watermark_detect(wave, [30000], [20000], c2)                                # past the tensor
    with pytest.raises(_lib.F5HipError, match="fp32"):
        ops.watermark_detect(wave.double(), [0], [20000], c2)
    with pytest.raises(_lib.F5HipError, match="carriers must be"):
        ops.watermark_detect(wave, [0], [20000], c2.to(torch.int32))
    with pytest.raises(_lib.F5HipError, match="one value per clip"):
        ops.watermark_detect(wave, [0, 1], [20000], c2)
    with pytest.raises(RuntimeError, match="carriers must be"):
        torch.ops.f5hip.watermark_detect(wave, torch.zeros(1, dtype=torch.int64), torch.tensor([20000], dtype=torch.int32), c2[:, :64].contiguous())
    assert _counter("watermark_detect_launches") == 0 and _counter("watermark_detect_clips") == 0
    assert call() == 0 and _counter("watermark_detect_launches") == 4 and _counter("watermark_detect_clips") == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ reject_marked with the device front-end
@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


def test_reject_marked_uploads_are_scored_in_one_call_per_front_end_call(hip_objects):
    """The decisions of the host path, made on the front-end's device buffer: one `ops.watermark_detect` call for the new uploads of a
    front-end call, nothing for a cached voice, nothing without the option."""
    as_clip = lambda pcm, sr=RATE: (torch.from_numpy(pcm.astype(np.float32) / 32768.0)[None], sr)   # noqa: E731
    clean, marked = ref.host(3 * RATE, 7), wave_codec.mark_pcm16(ref.host(3 * RATE, 8), K2)
    uploads = dict(clean=as_clip(clean), marked=as_clip(marked), marked16k=as_clip(infer.resample_pcm16(marked, 16000), 16000),
                   other=as_clip(wave_codec.mark_pcm16(clean, K3)), clean2=as_clip(ref.host(2 * RATE, 9)))
    decisions = {}
    for frontend in (False, True):
        mgr = serve.TTSManager(nfe_step=8, device_frontend=frontend, reject_marked=[K1, K2]).load(*hip_objects)
        try:
            for name, clip in uploads.items():
                _reset()
                infer.WATERMARK_COUNTS.clear()
                try:
                    voice, _ = mgr._clip_voice(clip, "reference words")
                    decisions[frontend, name] = True
                    assert voice.pending is None and voice.audio is not None
                except ValueError as e:
                    assert str(e) == serve.MARKED_REFERENCE
                    decisions[frontend, name] = False
                if frontend:
                    assert infer.WATERMARK_COUNTS == {"device_calls": 1} and _counter("watermark_detect_launches") == 4 and _counter("watermark_detect_clips") == 1
                else:
                    assert infer.WATERMARK_COUNTS == {"host_clips": 1} and _counter("watermark_detect_launches") == 0
            if frontend:
                _reset()
                infer.WATERMARK_COUNTS.clear()
                mgr._clip_voice(uploads["clean"], "reference words")                    # cached: it has already passed
                assert not infer.WATERMARK_COUNTS and _counter("watermark_detect_launches") == 0
                fresh = [(as_clip(ref.host(2 * RATE, 20 + k)), "reference words", True) for k in range(3)]
                assert len(mgr._clip_voices(fresh)) == 3                                # three new uploads of one rate: ONE front-end call, ONE detect call
                assert infer.WATERMARK_COUNTS == {"device_calls": 1} and _counter("watermark_detect_launches") == 4 and _counter("watermark_detect_clips") == 3
                with pytest.raises(ValueError) as e:                                    # a script's marked upload refuses the call; nothing of it is cached
                    mgr._clip_voices([(as_clip(ref.host(2 * RATE, 30)), "reference words", True), (as_clip(wave_codec.mark_pcm16(ref.host(2 * RATE, 31), K1)), "words", True)])
                assert str(e.value) == serve.MARKED_REFERENCE and len(mgr._clip_cache) == 6
        finally:
            mgr.close()
    assert [decisions[True, name] for name in uploads] == [decisions[False, name] for name in uploads] == [True, False, False, True, True]
    off = serve.TTSManager(nfe_step=8, device_frontend=True).load(*hip_objects)         # default None: no call, no change
    try:
        _reset()
        voice, _ = off._clip_voice(uploads["marked"], "reference words")
        assert voice.pending is not None and _counter("watermark_detect_launches") == 0
    finally:
        off.close()
