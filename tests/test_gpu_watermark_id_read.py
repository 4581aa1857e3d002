"""The watermark's trace ids on the device, reading (csrc/wave_mark.h, f5hip_watermark_read_ids: a ragged batch of mono 24 kHz fp32 clips
scored against 1 .. 4 keys and read for the three symbols of each key's id in four launches) against the host definition
`wave_codec.read_watermark` (fp64), and `TTSManager.read_watermark` with the device front-end.

A clip's rows equal its single-clip call's bit for bit, their first four words equal `ops.watermark_detect`'s bit for bit, and the input is
never written: equality of bytes.  Against the fp64 host every symbol must be the host's wherever the host's z_d >= 5, the id decision the
host's for every clip and key, and |z_d(dev) - z_d(host)| stays within 8 x the maximum measured over these clips on the first run on an
MI355X (DZ_ID_MEASURED; room for another FFT and summation order), never above 0.05: a difference beyond that is not rounding."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, ops, serve, synth, torch_ops, wave_codec  # noqa: E402
from tts_indic_server_f5_amd.wave_codec import WatermarkTag  # noqa: E402

import watermark_ref as ref  # noqa: E402
from test_gpu_request_knobs import ARCH, VOCAB  # noqa: E402
from test_gpu_watermark_detect import FILLER, _counter, _reset  # noqa: E402

RATE = 24000
K1, K2 = 1, 0xDEADBEEF
MIXED = 0x2A5F3C91
DZ_ID_MEASURED = 1.891e-5                              # max |z_d(dev) - z_d(host)| over CLIPS x (1 key, 2 keys), MI355X: profiles/watermark_id_bench.txt
DZ_ID_BOUND = min(8 * DZ_ID_MEASURED, 0.05)


def _clips():
    """0.4 s (below the minimum), 0.5 s, 1 s, 3 s, 16 383, 16 384 and 16 385 samples and one cut by 7001 out of a 3 s wave: tagged under
    either key, key-only or unmarked."""
    t = lambda n, s, k, i: wave_codec.mark_pcm16(ref.host(n, s), WatermarkTag(k, i))   # noqa: E731
    pcm = [t(9600, 1, K1, 5), t(12000, 2, K1, MIXED), t(RATE, 3, K2, 1023), t(3 * RATE, 4, K1, 2 ** 30 - 1), t(16383, 5, K1, 1 << 10),
           wave_codec.mark_pcm16(ref.host(16384, 6), K1), ref.host(16385, 7), t(3 * RATE, 8, K2, MIXED)[7001:], t(RATE, 9, K1, 0)]
    return [(x.astype(np.float32) / np.float32(32768.0)) for x in pcm]


@pytest.fixture(scope="module")
def clips():
    return _clips()


def _host_symbols(clip, key):
    """[(s_d, z_d)] of the fp64 definition."""
    if len(clip) < wave_codec.WATERMARK_MIN_SAMPLES:
        return [(0, 0.0)] * 3
    FZ = np.conj(np.fft.rfft(wave_codec.watermark_fold(clip)))
    corr = lambda k: np.fft.irfft(FZ * np.fft.rfft(wave_codec.watermark_carrier(k).astype(np.float64)), n=wave_codec.WATERMARK_PERIOD)   # noqa: E731
    offset = wave_codec.watermark_score(corr(key), key).offset
    return [wave_codec.watermark_symbol(corr(sub), offset) for sub in wave_codec.watermark_subkeys(key)]


@pytest.fixture(scope="module")
def host(clips):
    """The fp64 definition, once: [clip][key] -> (WatermarkRead, [(s_d, z_d)])."""
    return [[(wave_codec.read_watermark(x, [k])[0], _host_symbols(x, k)) for k in (K1, K2)] for x in clips]


def _device(clips, keys, detect=False):
    """ops.watermark_read_ids (or ops.watermark_detect on the same buffer) on ONE packed buffer with a filler between the clips -> (rows, the
    buffer afterwards, the buffer before)."""
    dev = torch.device("cuda:0")
    offsets, off = [], 3
    for x in clips:
        offsets.append(off)
        off += len(x) + 5
    buf = np.full(off, FILLER, dtype=np.float32)
    for o, x in zip(offsets, clips):
        buf[o:o + len(x)] = x
    wave = torch.from_numpy(buf.copy()).to(dev)
    if detect:
        rows = ops.watermark_detect(wave, offsets, [len(x) for x in clips], ops.watermark_carriers(keys, dev))
    else:
        rows = ops.watermark_read_ids(wave, offsets, [len(x) for x in clips], ops.watermark_tag_carriers(keys, dev))
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (len(clips), len(keys), 10)
    return rows.cpu().numpy(), wave.cpu().numpy(), buf


@pytest.fixture(scope="module")
def runs(clips):
    return {keys: _device(clips, list(keys)) for keys in ((K1,), (K1, K2))}


@pytest.mark.parametrize("keys", [(K1,), (K1, K2)], ids=["one_key", "two_keys"])
def test_symbols_decisions_and_scores_against_the_host(clips, host, runs, keys):
    rows, after, before = runs[keys]
    assert after.tobytes() == before.tobytes()                                          # the input is never written
    worst = 0.0
    for i, x in enumerate(clips):
        got = ops.watermark_reads(rows[i], list(keys))
        for j, (g, key) in enumerate(zip(got, keys)):
            h, symbols = host[i][(K1, K2).index(key)]
            for d, (s, z) in enumerate(symbols):
                s_dev, z_dev = int(rows[i][j][4 + 2 * d]), float(rows[i][j][5 + 2 * d])
                print(f"clip {i} ({len(x)} samples) key {key:#x} symbol {d}: s_dev {s_dev} s_host {s} z_dev {z_dev:.6f} z_host {z:.6f} dz {abs(z_dev - z):.3e}")
                if z >= 5:
                    assert s_dev == s, (i, key, d)
                if s_dev == s:                                                          # (another candidate of a flat grid is another number)
                    worst = max(worst, abs(z_dev - z))
            assert abs(h.id_z - wave_codec.WATERMARK_ID_THRESHOLD) > 0.05 and (abs(h.z - wave_codec.WATERMARK_THRESHOLD) > 0.5 or h.z == 0.0)
            assert (g.id, g.detected) == (h.id, h.detected), (i, key, g, h)
    print(f"max |z_d(dev) - z_d(host)| = {worst:.3e} (bound {DZ_ID_BOUND:.3e})")
    assert worst <= DZ_ID_BOUND, worst
    assert rows[0].tolist() == [[0.0] * 10] * len(keys)                                 # below WATERMARK_MIN_SAMPLES: zeros
    ids = [ops.watermark_reads(rows[i], list(keys))[0].id for i in range(len(clips))]   # key 1's: the 0.5 s clip's third symbol stays below 6
    assert ids == [None, None, None, 2 ** 30 - 1, 1 << 10, None, None, None, 0]
    assert [int(rows[1][0][4 + 2 * d]) for d in range(3)] == wave_codec.watermark_id_symbols(MIXED)
    if len(keys) == 2:
        assert [ops.watermark_reads(rows[i], list(keys))[1].id for i in (2, 7)] == [1023, MIXED]
        assert ops.watermark_reads(rows[7], list(keys))[1].offset == 7001


def test_the_first_four_words_are_watermark_detect(clips, runs):
    for keys in ((K1,), (K1, K2)):
        scores, _, _ = _device(clips, list(keys), detect=True)
        assert runs[keys][0][..., :4].tobytes() == np.ascontiguousarray(scores).tobytes(), keys


def test_a_key_does_not_depend_on_the_other_keys_of_the_call(runs):
    assert np.array_equal(runs[(K1,)][0][:, 0], runs[(K1, K2)][0][:, 0])


def test_each_row_equals_its_single_clip_call(clips, runs):
    keys = (K1, K2)
    rows = runs[keys][0]
    for i, x in enumerate(clips):
        solo, _, _ = _device([x], list(keys))
        assert solo[0].tobytes() == rows[i].tobytes(), i
    back, _, _ = _device(clips[::-1], list(keys))                                       # another order: other clip groups in the correlation launch
    assert back[::-1].tobytes() == rows.tobytes()
    five, _, _ = _device(clips[:5], list(keys))                                         # a last group that is not full
    assert five.tobytes() == rows[:5].tobytes()


def test_launch_count_and_both_bindings(clips, runs):
    assert ops.watermark_read_ids_launches() == 4
    for batch, keys in ((clips[1:2], [K1]), (clips, [K1, K2])):
        _reset()
        _device(batch, keys)
        assert _counter("watermark_read_ids_launches") == 4 and _counter("watermark_read_ids_clips") == len(batch)
        assert _counter("watermark_detect_launches") == 0 and _counter("wave_mark_launches") == 0
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        again, _, _ = _device(clips, [K1, K2])
    finally:
        torch_ops._loaded = True
    assert again.tobytes() == runs[(K1, K2)][0].tobytes()


def test_refusals_come_before_any_launch(clips):
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    wave = torch.zeros(40000, device=dev)
    carriers = ops.watermark_tag_carriers([K1, K2], dev)
    rows = torch.zeros(2, 2, 10, device=dev)

    def call(n_samples=(20000,), offset=(0,), n_keys=2, car_p=carriers.data_ptr()):
        ns, off = np.asarray(n_samples, dtype=np.int32), np.asarray(offset, dtype=np.int64)
        return lib.f5hip_watermark_read_ids(len(ns), C.c_void_p(wave.data_ptr()), C.c_void_p(off.ctypes.data), C.c_void_p(ns.ctypes.data), n_keys,
                                            C.c_void_p(car_p) if car_p else None, C.c_void_p(rows.data_ptr()), _lib.current_stream_ptr())

    _reset()
    for bad in (0, 5):
        assert call(n_keys=bad) != 0 and b"watermark_read_ids: 1 .. 4 keys" in lib.f5hip_last_error(), bad
    assert call(n_samples=(0,)) != 0 and b"watermark_read_ids: clip 0 has 0 samples" in lib.f5hip_last_error()
    assert call(n_samples=(20000, 20000), offset=(0, 10000)) != 0 and b"overlaps" in lib.f5hip_last_error()
    assert call(car_p=None) != 0 and b"bad argument" in lib.f5hip_last_error()
    assert call(car_p=carriers.data_ptr() + 8) != 0 and b"aligned" in lib.f5hip_last_error()
    with pytest.raises(_lib.F5HipError, match="carriers must be"):
        ops.watermark_read_ids(wave, [0], [20000], ops.watermark_carriers([K1, K2], dev))               # the detector's layout
    with pytest.raises(_lib.F5HipError, match="carriers must be"):
        ops.watermark_read_ids(wave, [0], [20000], ops.watermark_tag_carriers([1, 2, 3, 4, 5], dev))    # more than four keys
    with pytest.raises(_lib.F5HipError, match="tensor of 40000"):
        ops.watermark_read_ids(wave, [30000], [20000], carriers)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)   # noqa: E731
    with pytest.raises(RuntimeError, match="carriers must be"):
        torch.ops.f5hip.watermark_read_ids(wave, torch.zeros(1, dtype=torch.int64), i32(20000), carriers.reshape(8, 16384))
    with pytest.raises(RuntimeError, match="one value per clip"):
        torch.ops.f5hip.watermark_read_ids(wave, torch.zeros(2, dtype=torch.int64), i32(20000), carriers)
    assert _counter("watermark_read_ids_launches") == 0
    assert call() == 0 and _counter("watermark_read_ids_launches") == 4
    torch.cuda.synchronize()


def test_manager_reads_on_the_device(clips):
    """`TTSManager.read_watermark` with the device front-end and a model on the GPU: one `ops.watermark_read_ids` call, the host's ids."""
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    y = wave_codec.mark_pcm16(ref.host(3 * RATE, 4), WatermarkTag(K1, 2 ** 30 - 1))
    want = wave_codec.read_watermark(y.astype(np.float32) / np.float32(32768.0), [K1, K2])
    mgr = serve.TTSManager(nfe_step=8, device_frontend=True, watermark={"key": K1, "id": 3}).load(
        F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict()))
    try:
        _reset()
        got = mgr.read_watermark((torch.from_numpy(y.astype(np.float32) / np.float32(32768.0))[None], RATE), [K1, K2])
        assert _counter("watermark_read_ids_launches") == 4 and _counter("watermark_read_ids_clips") == 1
        assert [(g.key, g.id, g.detected, g.offset) for g in got] == [(w.key, w.id, w.detected, w.offset) for w in want] and got[0].id == 2 ** 30 - 1
        assert abs(got[0].id_z - want[0].id_z) <= DZ_ID_BOUND and abs(got[0].z - want[0].z) <= 0.05
        assert mgr.read_watermark((torch.from_numpy(y.astype(np.float32) / np.float32(32768.0))[None], RATE))[0].id == 2 ** 30 - 1   # the manager's own key
        host_mgr = serve.TTSManager(device_frontend=False)
        assert host_mgr.read_watermark((torch.from_numpy(y.astype(np.float32) / np.float32(32768.0))[None], RATE), [K1, K2]) == want
    finally:
        mgr.close()
