"""CPU: `audio_prep.preprocess_ref_ranges`, the reference-clip pre-step restated as frame ranges of the source (what the device call
mirrors), against its definition `audio_prep.preprocess_ref_segment` -- frame for frame on the case matrix of tests/ref_prestep_cases.py
and on 200 seeded random layouts; its integer comparisons against the fp64 / dBFS ones they replace; and `TTSManager(device_prestep=True)`
on a CPU stand-in, which must fall back to the host path."""
import io
import math
import wave
from fractions import Fraction

import numpy as np
import pytest
import torch

import ref_prestep_cases as RC
from tts_indic_server_f5_amd import audio_prep as AP
from tts_indic_server_f5_amd import serve

QUIET = lambda *_: None


def _by_ranges(x, rate, clip):
    seg = AP.PcmSegment(x, rate)
    ranges, tail = AP.preprocess_ref_ranges(seg, clip)
    assert all(0 <= a < b <= seg.frames.shape[0] for a, b in ranges) and tail == int(rate * 50 / 1000.0)
    return np.concatenate([seg.frames[a:b] for a, b in ranges] + [np.zeros((tail, seg.frames.shape[1]), dtype=np.int16)])


@pytest.mark.parametrize("name", list(RC.cases()))
def test_ranges_reproduce_the_segment_on_the_matrix(name):
    x, rate, clip = RC.cases()[name]
    got, want = _by_ranges(x, rate, clip), RC.expected(name)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_ranges_reproduce_the_segment_on_200_random_layouts():
    kinds = set()
    for seed in range(200):
        x, rate, clip = RC.random_layout(seed)
        want = AP.preprocess_ref_segment(AP.PcmSegment(x, rate), clip, show_info=QUIET).frames
        got = _by_ranges(x, rate, clip)
        assert got.shape == want.shape and np.array_equal(got, want), seed
        kinds.add((len(AP.preprocess_ref_ranges(AP.PcmSegment(x, rate), clip)[0]) > 1, clip))
    assert {(True, True), (False, True), (False, False)} <= kinds      # several ranges, one range, not clipped: all occur


def test_the_matrix_covers_what_it_names():
    """Each pair of threshold cases differs, the stop / pass 2 / hard cut cases end where they should, and in the two trailing-silence
    cases the running subtraction's rounding decides the cut."""
    n = lambda name: RC.expected(name).shape[0]
    t1, t2, te = RC.thresholds()
    for a, b in ((f"thresh_pass1_{t1}", f"thresh_pass1_{t1 + 1}"), (f"thresh_pass2_{t2}", f"thresh_pass2_{t2 + 1}"), (f"thresh_edges_{te}", f"thresh_edges_{te + 1}")):
        assert n(a) < n(b), (a, b)                                     # amplitude T is silent and is cut, T + 1 is not
    tail = int(11025 * 50 / 1000.0)
    assert n("hard_cut") - tail == int(15000 * (11025 / 1000.0))
    assert n("pass1_stop") < n("hard_cut") and n("pass2_short_pauses") < n("hard_cut") and n("pass1_first_chunk_long") == n("hard_cut")
    for name in ("pass1_stop", "pass1_first_chunk_long", "pass2_short_pauses", "hard_cut"):
        assert n(name + "_noclip") > n(name)
    for name in ("extra_window_pass1", "extra_window_pass2"):
        L = len(RC.segment(name)[0])
        assert (L - 1000) % 10 != 0 and (L - 100) % 10 != 0, name
    for name, (rate, body_ms, quiet_ms) in RC.TRAIL_ROUNDING.items():
        frames = RC.cases()[name][0].shape[0]
        exact = int((Fraction(frames, rate) - Fraction(quiet_ms, 1000)) * 1000)
        assert exact == body_ms and n(name) - int(rate * 50 / 1000.0) == int((body_ms - 1) * (rate / 1000.0)), name
    assert len(AP.preprocess_ref_ranges(*RC.segment("edges_two_ranges"))[0]) == 2


def test_integer_thresholds_agree_with_the_scalar_rule():
    lead, trail = AP.edge_rms_thresholds()
    for r in range(32769):
        db = AP._dbfs_of_rms(r)
        assert (db < AP.REF_EDGE_DBFS) == (r < lead) and (db > AP.REF_EDGE_DBFS) == (r >= trail), r
    for _, db in AP.REF_CLIP_PASSES:
        thresh = (10 ** (db / 20.0)) * 32768.0
        for r in range(32769):
            assert (r <= thresh) == (r * r < AP.silence_square(db)), (db, r)


def test_integer_window_comparison_agrees_with_fp64_on_every_window():
    lead, trail = AP.edge_rms_thresholds()
    windows = 0
    for name, (x, rate, _) in RC.cases().items():
        seg = AP.PcmSegment(x, rate)
        L, c, ch = len(seg), seg._cum_squares(), seg.frames.shape[1]
        plans = [(msl, 10, AP.silence_square(db)) for msl, db in AP.REF_CLIP_PASSES] + [(10, 10, lead * lead), (1, 1, trail * trail)]
        for msl, step, square in plans:
            if L < msl:
                continue
            starts = np.arange(0, L - msl + 1, step, dtype=np.int64)
            if (L - msl) % step:
                starts = np.append(starts, L - msl)
            a, b = seg._frames(starts), seg._frames(starts + msl)
            n, S = (b - a) * ch, c[b] - c[a]
            ok = n > 0
            rms = seg.rms_windows(starts, starts + msl)                       # floor(sqrt(S / n)) in fp64
            r = math.isqrt(square)
            assert np.array_equal(rms[ok] >= r, S[ok] >= square * n[ok]), (name, msl)
            assert int(S.max(initial=0)) < 2 ** 53
            windows += int(ok.sum())
    assert windows > 100000


# ------------------------------------------------------------------------------------------------ the manager without a GPU
class _CpuModel:
    """A stand-in model object on the CPU: no `device` on a GPU, so `device_prestep` must fall back to the host path."""
    device = torch.device("cpu")


def _wav_bytes(frames, sr):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as f:
        f.setnchannels(frames.shape[1]); f.setsampwidth(2); f.setframerate(sr)
        f.writeframes(np.ascontiguousarray(frames, dtype="<i2").tobytes())
    return buf.getvalue()


@pytest.mark.parametrize("name", ["edges_two_ranges", "short_22050_stereo"])
def test_manager_on_a_cpu_stand_in_falls_back_to_the_host_path(name, monkeypatch):
    from tts_indic_server_f5_amd import ops

    def never(*a, **k):
        raise AssertionError("ops.ref_prestep called without a GPU")

    monkeypatch.setattr(ops, "ref_prestep", never)
    x, rate, clip = RC.cases()[name]
    raw = _wav_bytes(x, rate)
    assert serve.DEVICE_PRESTEP_DEFAULT is False and serve.TTSManager().device_prestep is False
    voices = []
    for kwargs in (dict(device_frontend=True, device_prestep=True), dict(device_frontend=True), dict(device_frontend=False, device_prestep=True)):
        mgr = serve.TTSManager(**kwargs)
        mgr.model_obj = _CpuModel()
        assert mgr._prestep_device() is None
        voice, ref_text = mgr._clip_voice(raw, "Some call me nature", clip)
        assert ref_text == "Some call me nature. "
        voices.append(voice)
    want = torch.from_numpy(np.ascontiguousarray((RC.expected(name).astype(np.float32) / 32768.0).T))
    for v in voices[:2]:                                                  # deferred: the clip as the host pre-step left it, bit for bit
        wav, sr, _ = v.pending
        assert sr == rate and not wav.is_cuda and torch.equal(wav, want)
    assert voices[2].pending is None and voices[2].seconds == voices[0].seconds
    with pytest.raises(ValueError, match="Invalid audio: the clip is empty or silent."):
        mgr._clip_voice(_wav_bytes(RC.cases()["zeros_2s"][0], 11025), "Some call me nature", True)
