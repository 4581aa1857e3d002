"""The watermark scan on the device (csrc/wave_mark.h, f5hip_watermark_scan: segment ranges of ONE mono 24 kHz fp32 recording folded by
their absolute sample index, correlated with 1 .. 16 keys and scored, with or without the trace-id symbols) against the host definition
`wave_codec.scan_watermark` (fp64), `ops.watermark_scan` and `TTSManager.scan_watermark` with the device front-end.

A range's rows equal its single-range call's bit for bit -- with other ranges, in another order, with the keys swapped, in a second slab --,
the first four words of a row with ids equal the row without, a range of every segment equals `ops.watermark_detect` of the recording, and
the input is never written: equality of bytes.  Against the fp64 host the decisions, offsets and symbols must be the host's away from the
thresholds, and |z_dev - z_host| over all window and span rows stays within 8 x the maximum measured over these rows on the first run on an
MI355X (DZ_SCAN_MEASURED; room for another FFT and summation order), never above 0.05: a difference beyond that is not rounding.  The
shapes are the smallest at which each path can go wrong: a recording of 5 periods and 1000 samples (a last segment below the minimum), one
short window, exactly one and two periods plus a sample, and 257 ranges against 16 carrier rows (the first size that takes a second slab)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, ops, serve, synth, torch_ops, wave_codec  # noqa: E402
from tts_indic_server_f5_amd.wave_codec import WatermarkTag  # noqa: E402

import watermark_ref as ref  # noqa: E402
from test_gpu_request_knobs import ARCH, VOCAB  # noqa: E402
from test_gpu_watermark_detect import _counter, _reset  # noqa: E402

P = wave_codec.WATERMARK_PERIOD
K1, K2 = 1, 0xDEADBEEF
TAG = 0x2A5F3C91
N_A = 5 * P + 1000
RANGES_A = [(0, 2), (1, 2), (2, 2), (3, 2), (4, 2), (5, 1), (2, 1), (0, 6), (0, 4)]     # the five windows, the last partial segment, one segment, all, a span
EDGES = (12000, 11999, P, 2 * P + 1)
DZ_SCAN_MEASURED = 4.586e-5                             # max |z_dev - z_host| over the window and span rows below, MI355X: profiles/watermark_scan_bench.txt
DZ_SCAN_BOUND = min(8 * DZ_SCAN_MEASURED, 0.05)


def _f32(pcm):
    return pcm.astype(np.float32) / np.float32(32768.0)


def recording_a():
    """Recording A: 82 920 samples of host material with K1's tagged mark on samples [P / 2, 3.5 P)."""
    x = np.array(ref.host(N_A, 11))
    x[P // 2:7 * P // 2] = wave_codec.mark_pcm16(x[P // 2:7 * P // 2], WatermarkTag(K1, TAG))
    return _f32(x)


@pytest.fixture(scope="module")
def recording():
    return recording_a()


def _host_rows(x, ranges, keys, seg=None):
    """The fp64 definition of the device rows, [range][key] -> (z, offset, [(s_d, z_d)] x 3); zeros for a range below the minimum.
    `seg`: the recording's segment rows when the caller has them already."""
    if seg is None:
        seg, _ = wave_codec.scan_window_rows(np.asarray(x, dtype=np.float64))
    out = []
    for first, count in ranges:
        if min(len(x), (first + count) * P) - first * P < wave_codec.WATERMARK_MIN_SAMPLES:
            out.append([(0.0, 0, [(0, 0.0)] * 3) for _ in keys])
            continue
        Z = seg[first].copy()
        for s in range(first + 1, first + count):
            Z += seg[s]
        row = []
        for k in keys:
            r = wave_codec._scan_correlations(Z[None], [wave_codec.watermark_carrier(c) for c in [k] + wave_codec.watermark_subkeys(k)])[:, 0]
            score = wave_codec.watermark_score(r[0], k)
            row.append((score.z, score.offset, [wave_codec.watermark_symbol(r[1 + d], score.offset) for d in range(3)]))
        out.append(row)
    return out


def _device(x, ranges, keys, ids):
    dev = torch.device("cuda:0")
    wave = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    carriers = ops.watermark_tag_carriers(keys, dev) if ids else ops.watermark_carriers(keys, dev)
    rows = ops.watermark_scan_rows(wave, ranges, carriers, ids=ids)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (len(ranges), len(keys), 10 if ids else 4)
    assert wave.cpu().numpy().tobytes() == np.ascontiguousarray(x).tobytes()            # the input is never written
    return rows.cpu().numpy()


@pytest.fixture(scope="module")
def runs(recording):
    return {ids: _device(recording, RANGES_A, [K1, K2], ids) for ids in (False, True)}


def test_window_and_span_rows_against_the_host(recording, runs):
    host = _host_rows(recording, RANGES_A, [K1, K2])
    worst = 0.0
    for i, rng in enumerate(RANGES_A):
        for j, key in enumerate((K1, K2)):
            z, o, symbols = host[i][j]
            plain, full = runs[False][i][j], runs[True][i][j]
            print(f"range {rng} key {key:#x}: z_dev {plain[0]:.6f} z_host {z:.6f} dz {abs(plain[0] - z):.3e} offset {int(plain[1])} / {o}")
            worst = max(worst, abs(float(plain[0]) - z))
            if abs(z - wave_codec.WATERMARK_THRESHOLD) > DZ_SCAN_BOUND:
                assert bool(plain[0] >= wave_codec.WATERMARK_THRESHOLD) == bool(z >= wave_codec.WATERMARK_THRESHOLD), (rng, key)
            if z >= 10:
                assert int(plain[1]) == o, (rng, key)
            for d, (s, zd) in enumerate(symbols):
                s_dev, zd_dev = int(full[4 + 2 * d]), float(full[5 + 2 * d])
                print(f"    symbol {d}: s_dev {s_dev} s_host {s} z_dev {zd_dev:.6f} z_host {zd:.6f} dz {abs(zd_dev - zd):.3e}")
                if z >= 10 and zd >= 10:
                    assert s_dev == s, (rng, key, d)
                if int(plain[1]) == o and s_dev == s:                                   # (another candidate of a flat grid is another number)
                    worst = max(worst, abs(zd_dev - zd))
                if z >= 10 and abs(zd - wave_codec.WATERMARK_ID_THRESHOLD) > DZ_SCAN_BOUND:
                    assert bool(zd_dev >= wave_codec.WATERMARK_ID_THRESHOLD) == bool(zd >= wave_codec.WATERMARK_ID_THRESHOLD), (rng, key, d)
    print(f"max |z_dev - z_host| = {worst:.3e} (bound {DZ_SCAN_BOUND:.3e})")
    assert worst <= DZ_SCAN_BOUND, worst
    assert runs[False][5].tolist() == [[0.0] * 4] * 2 and runs[True][5].tolist() == [[0.0] * 10] * 2   # 1000 samples: below the minimum, zeros
    # the marked stretch: windows 0 .. 2 carry K1 at one offset, the range (0, 4) reads the id; K2 is nowhere
    assert [bool(runs[False][w][0][0] >= 7.0) for w in range(5)] == [host[w][0][0] >= 7.0 for w in range(5)]
    assert host[8][0][0] >= 10 and int(runs[False][1][0][1]) == (-(P // 2)) % P
    assert ops.watermark_reads(runs[True][8], [K1, K2])[0].id == wave_codec.scan_watermark(recording, [K1])[0].id == TAG
    assert all(runs[False][i][1][0] < 7.0 for i in range(len(RANGES_A)))


def test_the_first_four_words_are_the_row_without_ids(runs):
    assert runs[True][..., :4].tobytes() == np.ascontiguousarray(runs[False]).tobytes()


def test_a_whole_range_is_watermark_detect(recording, runs):
    dev = torch.device("cuda:0")
    wave = torch.from_numpy(recording).to(dev)
    scores = ops.watermark_detect(wave, [0], [len(recording)], ops.watermark_carriers([K1, K2], dev)).cpu().numpy()
    assert scores[0].tobytes() == runs[False][7].tobytes()


def test_each_range_is_bit_identical_alone_reversed_and_with_the_keys_swapped(recording, runs):
    for ids in (False, True):
        rows = runs[ids]
        for i, rng in enumerate(RANGES_A):
            assert _device(recording, [rng], [K1, K2], ids)[0].tobytes() == rows[i].tobytes(), (ids, rng)
        assert _device(recording, RANGES_A[::-1], [K1, K2], ids)[::-1].tobytes() == rows.tobytes(), ids
        swapped = _device(recording, RANGES_A, [K2, K1], ids)
        assert np.ascontiguousarray(swapped[:, ::-1]).tobytes() == rows.tobytes(), ids
        assert _device(recording, RANGES_A, [K1], ids).tobytes() == np.ascontiguousarray(rows[:, :1]).tobytes(), ids


def test_a_second_slab_changes_no_row(recording, runs):
    keys = [K1, K2, 3, 4]                                                               # 16 carrier rows with ids: 256 ranges per slab
    ranges = [RANGES_A[i % len(RANGES_A)] for i in range(257)]
    assert ops.watermark_scan_launches(257, 4, True) == 6 and ops.watermark_scan_launches(256, 4, True) == 4
    assert ops.watermark_scan_launches(878, 4) == 4 and ops.watermark_scan_launches(878, 16) == 10 and ops.watermark_scan_launches() == 4
    _reset()
    rows = _device(recording, ranges, keys, True)
    assert _counter("watermark_scan_launches") == 6 and _counter("watermark_scan_ranges") == 257
    for i in range(257):
        assert rows[i][:2].tobytes() == runs[True][i % len(RANGES_A)].tobytes(), i      # rows 256 (slab 2) and 0 .. 255 (slab 1) alike


def test_launch_count_and_both_bindings(recording, runs):
    for ids, counted in ((False, "watermark_detect_launches"), (True, "watermark_read_ids_launches")):
        _reset()
        _device(recording, RANGES_A, [K1, K2], ids)
        assert _counter("watermark_scan_launches") == _lib.lib().f5hip_watermark_scan_launches() == 4
        assert _counter("watermark_scan_ranges") == len(RANGES_A) and _counter(counted) == 0
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        again = {ids: _device(recording, RANGES_A, [K1, K2], ids) for ids in (False, True)}
    finally:
        torch_ops._loaded = True
    assert all(again[ids].tobytes() == runs[ids].tobytes() for ids in (False, True))


def test_refusals_come_before_any_launch(recording):
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    wave = torch.from_numpy(recording).to(dev)
    plain, tagged = ops.watermark_carriers([K1, K2], dev), ops.watermark_tag_carriers([K1, K2], dev)
    rows = torch.zeros(4, 2, 10, device=dev)

    def call(n=N_A, first=(0,), count=(2,), n_keys=2, with_ids=0, wave_p=wave.data_ptr(), car_p=None, rows_p=rows.data_ptr(), n_ranges=None):
        f, c = np.asarray(first, dtype=np.int32), np.asarray(count, dtype=np.int32)
        car_p = (tagged if with_ids else plain).data_ptr() if car_p is None else car_p
        return lib.f5hip_watermark_scan(C.c_void_p(wave_p) if wave_p else None, n, len(f) if n_ranges is None else n_ranges, C.c_void_p(f.ctypes.data),
                                        C.c_void_p(c.ctypes.data), n_keys, with_ids, C.c_void_p(car_p) if car_p else None,
                                        C.c_void_p(rows_p) if rows_p else None, _lib.current_stream_ptr())

    _reset()
    for bad in (0, -1, wave_codec.WATERMARK_SCAN_MAX_SAMPLES + 1):
        assert call(n=bad) != 0 and b"watermark_scan: the recording has" in lib.f5hip_last_error(), bad
    for bad in (0, -1, 4097):
        assert call(n_ranges=bad) != 0 and b"ranges in a call" in lib.f5hip_last_error(), bad
    for first, count in (((5,), (2,)), ((6,), (1,)), ((0,), (0,)), ((-1,), (2,)), ((0, 0), (2, 7)), ((0,), (-3,))):
        assert call(first=first, count=count) != 0 and b"segments from segment" in lib.f5hip_last_error(), (first, count)
    for n_keys, with_ids in ((0, 0), (17, 0), (0, 1), (5, 1)):
        assert call(n_keys=n_keys, with_ids=with_ids) != 0 and b"keys in a call" in lib.f5hip_last_error(), (n_keys, with_ids)
    assert call(with_ids=2) != 0 and b"with_ids is 0 or 1" in lib.f5hip_last_error()
    for null in (dict(wave_p=0), dict(car_p=0), dict(rows_p=0)):
        assert call(**null) != 0 and b"bad argument" in lib.f5hip_last_error(), null
    for off in (dict(wave_p=wave.data_ptr() + 2), dict(car_p=plain.data_ptr() + 8), dict(rows_p=rows.data_ptr() + 2)):
        assert call(**off) != 0 and b"aligned" in lib.f5hip_last_error(), off
    with pytest.raises(_lib.F5HipError, match="carriers must be"):
        ops.watermark_scan_rows(wave, [(0, 2)], plain, ids=True)                        # the detector's layout with ids
    with pytest.raises(_lib.F5HipError, match="carriers must be"):
        ops.watermark_scan_rows(wave, [(0, 2)], ops.watermark_tag_carriers([1, 2, 3, 4, 5], dev), ids=True)
    with pytest.raises(_lib.F5HipError, match="2 segments from segment 5 of a recording of 6"):
        ops.watermark_scan_rows(wave, [(0, 2), (5, 2)], plain)
    with pytest.raises(_lib.F5HipError, match="ranges are 1 .. 4096"):
        ops.watermark_scan_rows(wave, [], plain)
    with pytest.raises(_lib.F5HipError, match="contiguous 1-D fp32"):
        ops.watermark_scan_rows(wave.double(), [(0, 2)], plain)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)   # noqa: E731
    with pytest.raises(RuntimeError, match="segments from segment"):
        torch.ops.f5hip.watermark_scan(wave, i32(4), i32(3), plain)
    with pytest.raises(RuntimeError, match="one value per range"):
        torch.ops.f5hip.watermark_scan(wave, i32(0, 1), i32(2), plain)
    with pytest.raises(RuntimeError, match="carriers must be"):
        torch.ops.f5hip.watermark_scan(wave, i32(0), i32(2), tagged.reshape(8, P)[:, :P // 2].contiguous())
    with pytest.raises(_lib.F5HipError, match="at most 14400000"):
        ops.watermark_scan(torch.zeros(1, device=dev).expand(wave_codec.WATERMARK_SCAN_MAX_SAMPLES + 1), [K1])   # (no storage behind it: refused by its size)
    assert ops.watermark_scan(wave[:11999], [K1]) == []                                 # below the minimum: no call
    assert _counter("watermark_scan_launches") == 0 and _counter("watermark_scan_ranges") == 0
    assert call() == 0 and _counter("watermark_scan_launches") == 4
    torch.cuda.synchronize()


def _same_spans(got, want, what):
    assert [(g.key, g.start, g.end, g.offset, g.id) for g in got] == [(w.key, w.start, w.end, w.offset, w.id) for w in want], (what, got, want)
    for g, w in zip(got, want):
        assert abs(g.z - w.z) <= DZ_SCAN_BOUND and abs(g.id_z - w.id_z) <= DZ_SCAN_BOUND, (what, g, w)


def test_ops_watermark_scan_returns_the_hosts_spans(recording):
    dev = torch.device("cuda:0")
    want = wave_codec.scan_watermark(recording, [K1, K2])
    assert [(w.key, w.start, w.id) for w in want] == [(K1, 0, TAG)] and want[0].end in (4 * P, 5 * P)
    _reset()
    got = ops.watermark_scan(torch.from_numpy(recording).to(dev), [K1, K2])
    assert _counter("watermark_scan_launches") == 8 and _counter("watermark_scan_ranges") == 5 + 1   # every window, then the one span
    _same_spans(got, want, "recording A")
    five = [K2, 3, 4, 5, K1]                                                            # a fifth key: its spans take a second call with ids
    _same_spans(ops.watermark_scan(torch.from_numpy(recording).to(dev), five), wave_codec.scan_watermark(recording, five), "five keys")
    for n in EDGES:
        y = _f32(wave_codec.mark_pcm16(ref.host(n, 12), WatermarkTag(K1, 77)))
        _reset()
        got = ops.watermark_scan(torch.from_numpy(y).to(dev), [K1, K2])
        _same_spans(got, wave_codec.scan_watermark(y, [K1, K2]), n)
        assert (_counter("watermark_scan_launches") == 0 and got == []) if n < wave_codec.WATERMARK_MIN_SAMPLES else len(got) == 1, (n, got)
    silent = ops.watermark_scan(torch.zeros(3 * P, device=dev), [K1])                   # nothing detected: no second call
    assert silent == [] and wave_codec.scan_watermark(np.zeros(3 * P, dtype=np.float32), [K1]) == []


def test_manager_scans_on_the_device(recording):
    """`TTSManager.scan_watermark` with the device front-end and a model on the GPU: `ops.watermark_scan` under the device lock."""
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    want = wave_codec.scan_watermark(recording, [K1, K2])
    mgr = serve.TTSManager(nfe_step=8, device_frontend=True, watermark={"key": K1, "id": 3}).load(
        F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict()))
    try:
        audio = (torch.from_numpy(recording)[None], 24000)
        _reset()
        _same_spans(mgr.scan_watermark(audio, [K1, K2]), want, "manager")
        assert _counter("watermark_scan_launches") == 8
        _same_spans(mgr.scan_watermark(audio), want, "the manager's own key")
        for n in EDGES:
            y = _f32(wave_codec.mark_pcm16(ref.host(n, 12), WatermarkTag(K1, 77)))
            _same_spans(mgr.scan_watermark((torch.from_numpy(y)[None], 24000), [K1, K2]), wave_codec.scan_watermark(y, [K1, K2]), n)
        _reset()
        assert mgr.scan_watermark((torch.from_numpy(recording[:11999])[None], 24000), [K1]) == [] and _counter("watermark_scan_launches") == 0
        bad = recording.copy()
        bad[5] = np.nan
        with pytest.raises(ValueError, match="not finite"):
            mgr.scan_watermark((torch.from_numpy(bad)[None], 24000), [K1])
        assert serve.TTSManager(device_frontend=False).scan_watermark(audio, [K1, K2]) == want
    finally:
        mgr.close()
