"""The reference-stretch selection on the device (csrc/ref_select.h, f5hip_ref_select: the report's measures over every window of a ragged
batch of recordings, ten launches) against its definition (audio_prep.select_reference; tests/ref_select_ref.py in float64 is the reference)
at the smallest shapes where the kernels can go wrong: a recording of exactly W frames, of W - 1 (the single short window), of W + hop - 1 and
W + hop (one window against two), of exactly one workgroup's run of windows and one more, rank 0 (W = 1), a silent recording (every column
equal, all zeros) and one that ends in digital silence (columns with exact zeros beside live values: radix ties), raw sides of one, two and
three channels at 24, 48 and 11.025 kHz.

The floors are compared EXACTLY with np.partition on the device's own downloaded fp32 band power, which isolates the select from the STFT.
clipped is an integer and must equal the definition's.  N, S and snr_db take tests/test_gpu_ref_assess.py's rule, per clip and measure 16
times the error of the float32 run of the restatement against its float64 run; a recording's float32 error is the largest over its windows.
speech is a threshold decision: it may differ by the frames that lie, in float64, within a relative 1e-3 of their window's threshold, and
at most 1 % of a recording's (window, frame) pairs do (asserted; measured on the CPU: at most 0.3 %, one pair of 340, none in most).

The chosen window is compared on the recordings with more than one window.  Their noise level falls by 24 dB along the recording, so the
best and the second-best key differ by far more than rounding: measured on the CPU in float64, they differ by at least one whole clipped
sample, or by equal infinities that the window index settles exactly, or in snr_db by 0.062 dB (W 20, 17 windows), 0.77 dB (W 1125, 17
windows), 1.29 dB and 15.8 dB; the manager's recording by 38 clipped samples.  Asserted below as at least 0.05 dB: the float32 run of the
restatement is within 3e-5 dB of the float64 one."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_select_ref as S  # noqa: E402
from tts_indic_server_f5_amd import audio_prep, ops, serve  # noqa: E402

DEV = "cuda:0"
GAP = 37
CASES = [(20, 4), (93, 48), (1125, 48), (1, 1)]
MARGIN_DB = 0.05


def _recordings(W, hop):
    """[(raw [ch, n], sr, prepared [len])] of one case."""
    run = ops.ref_select_run(W, hop)
    frames = sorted({F for F in (W, W - 1, W + hop - 1, W + hop, W + hop * (run - 1), W + hop * run) if F >= 4} | ({4, 20} if W == 1 else set()))
    recs = []
    for i, F in enumerate(frames):
        x = S.staged(F, 100 + i, quiet_from=0.6 if i == 1 else None)
        hard = np.clip(3.0 * x, -1.0, 1.0)
        n = len(x) * 11025 // 24000 + 5
        recs.append([(hard[None], 24000, x), (np.stack([np.repeat(hard, 2), np.repeat(x, 2)]), 48000, x), (np.stack([hard[:n], hard[-n:], x[:n]]), 11025, x)][i % 3])
    if (W, hop) == (20, 4):
        recs.append((np.zeros((1, 9000), dtype=np.float32), 24000, np.zeros(9000, dtype=np.float32)))
    return recs


def _call(recs, W, hop, taps=False):
    """One call over the recordings, both buffers packed with gaps of sentinel samples -> the outputs as numpy."""
    raw_at = np.cumsum([GAP] + [raw.size + GAP for raw, _, _ in recs])
    at = np.cumsum([GAP] + [len(x) + GAP for _, _, x in recs])
    raw_host, wave_host = np.full(raw_at[-1], 7.5, dtype=np.float32), np.full(at[-1], 7.5, dtype=np.float32)
    for ro, wo, (raw, _, x) in zip(raw_at, at, recs):
        raw_host[ro:ro + raw.size] = raw.reshape(-1)
        wave_host[wo:wo + len(x)] = x
    raw_dev, wave_dev = torch.from_numpy(raw_host).to(DEV), torch.from_numpy(wave_host).to(DEV)
    clips = [ops.RefSelectClip(raw_dev, int(ro), raw.shape[0], raw.shape[1], sr, wave_dev, int(wo), len(x)) for ro, wo, (raw, sr, x) in zip(raw_at, at, recs)]
    return [[t.cpu().numpy() for t in part] if isinstance(part, list) else part.cpu().numpy() for part in ops.ref_select(clips, W, hop, taps=taps)]


_CACHE = {}


def case(W, hop):
    """One ragged call of the case and its references, computed once, shared, never written."""
    if (W, hop) not in _CACHE:
        recs = _recordings(W, hop)
        rows, choices, floors, powers = _call(recs, W, hop, taps=True)
        refs = [(*S.table(raw, sr, x, W, hop, np.float64), S.table(raw, sr, x, W, hop, np.float32)[0]) for raw, sr, x in recs]
        _CACHE[(W, hop)] = dict(recs=recs, rows=rows, choices=choices, floors=floors, powers=powers, refs=refs)
    return _CACHE[(W, hop)]


@pytest.mark.parametrize("W,hop", CASES)
def test_every_floor_is_the_windows_order_statistic_exactly(W, hop):
    c = case(W, hop)
    for (raw, sr, x), floors, P in zip(c["recs"], c["floors"], c["powers"]):
        wins = S.windows(P.shape[1], W, hop)
        assert floors.shape == (len(wins), 339) and P.shape == (339, (len(x) + 768 + 255) // 256)
        for w, (f0, Ww) in enumerate(wins):
            want = np.partition(P[:, f0:f0 + Ww], (Ww - 1) // 5, axis=1)[:, (Ww - 1) // 5]
            assert np.array_equal(floors[w].view(np.uint32), want.view(np.uint32)), (len(x), w)


def _errors(a, b):
    """|a - b| per value: 0 where they are equal (infinities too), inf where only one is infinite."""
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(np.where(a == b, 0.0, np.abs(a - b)), nan=np.inf)


@pytest.mark.parametrize("W,hop", CASES)
def test_rows_against_the_float64_definition(W, hop):
    c = case(W, hop)
    for i, (rows, (want, E, f32)) in enumerate(zip(c["rows"], c["refs"])):
        got, wins = ops.ref_select_table(rows), S.windows(len(E), W, hop)
        assert got.shape == want.shape and np.array_equal(got[:, 0], want[:, 0]), f"clipped of recording {i}"
        near = [int(np.count_nonzero(np.abs(E[f0:f0 + Ww] - 4.0 * N) <= 4e-3 * N)) if N > 0 else 0 for (f0, Ww), N in zip(wins, want[:, 2])]
        assert sum(near) <= 0.01 * sum(Ww for _, Ww in wins)                     # the inputs' property, checked on the CPU
        assert (np.abs(got[:, 1] - want[:, 1]) <= near).all(), f"speech frames of recording {i}"
        err, bound = _errors(got[:, 2:], want[:, 2:]).max(axis=0), 16.0 * _errors(f32[:, 2:], want[:, 2:]).max(axis=0)
        print(f"[ref_select] W {W} hop {hop} recording {i} ({len(want)} windows): |err| of N, S, snr_db {err}; bounds {bound}")
        assert (err <= bound).all(), f"recording {i}"


@pytest.mark.parametrize("W,hop", CASES)
def test_the_chosen_window_is_the_definitions(W, hop):
    c = case(W, hop)
    many = [i for i, (want, _, _) in enumerate(c["refs"]) if len(want) > 1]
    assert len(many) >= 2 and all(c["choices"][i] == 0 for i in range(len(c["refs"])) if i not in many)
    for i in many:
        by_clipped, by_snr = S.key_margin(c["refs"][i][0])
        assert by_clipped >= 1 or by_snr >= MARGIN_DB, f"recording {i}: the reference's best two keys are {by_snr} dB apart"
        assert c["choices"][i] == S.ranked(c["refs"][i][0])[0], f"recording {i}"


@pytest.mark.parametrize("W,hop", [(20, 4), (93, 48)])
def test_a_recordings_rows_do_not_depend_on_the_batch(W, hop):
    c = case(W, hop)
    picks = [0, len(c["recs"]) - 2]                                   # the shortest and one of many windows: different lengths
    both = _call([c["recs"][i] for i in picks], W, hop)
    flipped = _call([c["recs"][i] for i in reversed(picks)], W, hop)
    for at, i in enumerate(picks):
        alone = _call([c["recs"][i]], W, hop)
        for (rows, choices), k in ((alone, 0), (both, at), (flipped, 1 - at)):
            assert np.array_equal(rows[k], c["rows"][i]) and choices[k] == c["choices"][i]


def test_the_managers_device_path_selects_what_its_host_path_selects():
    x = S.staged(1878, 31)                                                       # 20 s; stereo at 48 kHz, one channel hard-clipped
    wave = torch.from_numpy(np.stack([np.repeat(np.clip(3.0 * x, -1.0, 1.0), 2), np.repeat(x, 2)]))
    host = serve.TTSManager(device_frontend=False).select_reference((wave, 48000), 3.0, 0.2)
    by_clipped, by_snr = S.key_margin(host.windows[host.windows[:, 1] >= 0.2 * audio_prep.select_window_frames(3.0)])
    assert by_clipped >= 1 or by_snr >= MARGIN_DB
    mgr = serve.TTSManager(device_frontend=True)
    mgr.model_obj = types.SimpleNamespace(device=torch.device(DEV))              # (all the branch asks of a loaded model: where it lives)
    got = mgr.select_reference((wave, 48000), 3.0, 0.2)
    assert got[:3] == host[:3] and np.array_equal(got.windows[:, 0], host.windows[:, 0]) and got.report == host.report
