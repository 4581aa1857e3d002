"""CPU: the reference-stretch selection's definition (audio_prep.select_reference) against the plain-loop restatement in
tests/ref_select_ref.py, the key rule on hand-written tables, the recording it is for (a noisy start, a clean later stretch), its refusals,
and `TTSManager.select_reference` with its route on a manager without a device."""
import base64
import io
import math
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import denoise_ref as R  # noqa: E402
import ref_select_ref as S  # noqa: E402
from tts_indic_server_f5_amd import audio_prep as AP, serve  # noqa: E402

INF = math.inf


def _long_recording():
    """40 s at 24 kHz: speech-like throughout, white noise at 3 dB over the first 15 s (a door, a fan), at 35 dB behind."""
    n = 40 * R.RATE
    s = R.speechlike(n, 5)
    p = np.mean(s * s)
    noise = np.random.default_rng(6).standard_normal(n) * np.sqrt(np.where(np.arange(n) < 15 * R.RATE, p / 10 ** 0.3, p / 10 ** 3.5))
    return (s + noise).astype(np.float32)


LONG = _long_recording()


def _wav(x, sr=24000):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(sr)
        f.writeframes(np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2").tobytes())
    return buf.getvalue()


@pytest.mark.parametrize("W,hop,n,sr", [(20, 4, 5359, 24000), (20, 4, 20719, 11025), (93, 48, 35311, 48000), (1, 1, 1000, 24000)])
def test_definition_equals_the_restatement(W, hop, n, sr):
    x = S.staged(R.n_frames(n), n)
    raw = np.clip(3.0 * x, -1.0, 1.0)
    raw = np.stack([raw, x])[:, :len(x) * sr // 24000] if sr != 48000 else np.repeat(raw, 2)[None]
    got, (want, _) = AP.select_table(raw, sr, x, W, hop), S.table(raw, sr, x, W, hop)
    assert got.shape == want.shape == (len(S.windows(R.n_frames(len(x)), W, hop)), 5)
    assert np.array_equal(got[:, :2], want[:, :2]) and np.allclose(got[:, 2:4], want[:, 2:4], rtol=1e-12, atol=0)
    fin = np.isfinite(want[:, 4])
    assert np.array_equal(got[~fin, 4], want[~fin, 4]) and np.allclose(got[fin, 4], want[fin, 4], rtol=0, atol=1e-9)
    frames = [f for _, f in AP.select_windows(R.n_frames(len(x)), W, hop)]
    assert AP.select_choice(got, frames) == S.ranked(want)[0]


def test_a_short_recording_is_one_window_with_the_reports_measures():
    x = R.clip(60000)                                                            # 238 frames, below any window
    sel = AP.select_reference(x[None], 24000, x, seconds=3.0)
    s = AP.assess_spectrum(x)
    assert sel.windows.shape == (1, 5) and sel.window == 0 and (sel.start, sel.end) == (0, 60000)
    assert (sel.windows[0, 2], sel.windows[0, 3], sel.windows[0, 1]) == (s["N"], s["S"], s["speech_frames"])
    assert sel.report == AP.assess_reference(x[None], 24000, x)


@pytest.mark.parametrize("rows,want", [
    ([[3, 40.0], [0, 2.0], [0, 1.0]], 1),               # clipped beats snr_db
    ([[0, 10.0], [0, INF], [0, INF]], 1),               # +inf first, the earlier of two
    ([[1, -INF], [1, -5.0], [2, INF]], 1),              # -inf last among equals in clipped
    ([[0, 7.0], [0, 7.0], [0, 6.0]], 0),                # the earliest wins a tie
    ([[5, -INF]], 0),
])
def test_the_key_rule(rows, want):
    table = np.array([[c, 10, 1.0, 2.0, snr] for c, snr in rows], dtype=np.float64)
    assert AP.select_choice(table, [20] * len(rows)) == want == S.ranked(table)[0]


def test_a_long_upload_with_a_noisy_start_selects_the_clean_stretch():
    sel = AP.select_reference(LONG[None], 24000, LONG, seconds=12.0)
    assert sel.windows.shape[0] == (R.n_frames(len(LONG)) - 1125) // 48 + 1 and sel.end - sel.start == 1125 * 256 + 768
    assert sel.start >= 15 * R.RATE and sel.report.snr_db > 25.0                 # inside the clean stretch
    # ... where the pre-step keeps the noisy start: its crop begins at 0 and reads the noise
    pcm = np.clip(np.rint(LONG * 32768.0), -32768, 32767).astype(np.int16)[:, None]
    kept = AP.preprocess_ref_segment(AP.PcmSegment(pcm, 24000), True, show_info=lambda *_: None).frames[:, 0].astype(np.float32) / 32768.0
    # (15 s and the 50 ms of silence the pre-step appends)
    assert len(kept) <= 15 * R.RATE + 1200 and np.array_equal(kept[:1000], (pcm[:1000, 0] / 32768.0).astype(np.float32))
    assert AP.assess_reference(kept[None], 24000, kept).snr_db < 10.0 < sel.report.snr_db - 15.0


def test_refusals_and_min_speech_ratio():
    assert (AP.SELECT_MAX_SAMPLES, AP.SELECT_HOP) == (600 * 24000, S.HOP) and [AP.select_window_frames(s) for s in (3, 12.0, 15, 7.5)] == [281, 1125, 1406, 703]
    for bad in (2.5, 15.5, 12.3, "12", True, math.nan, None):
        with pytest.raises(ValueError, match="multiple of 0.5 from 3 to 15"):
            AP.select_window_frames(bad)
    with pytest.raises(ValueError, match="at most SELECT_MAX_SAMPLES = 14400000"):
        AP.select_table(np.zeros((1, 8), dtype=np.float32), 24000, np.zeros(AP.SELECT_MAX_SAMPLES + 1, dtype=np.float32), 1125)
    with pytest.raises(ValueError, match="from 0 to 1"):
        AP.select_reference(LONG[None], 24000, LONG, min_speech_ratio=1.5)
    table = np.array([[0, 2, 0.0, 0.0, INF], [0, 12, 1.0, 9.0, 9.0], [0, 15, 1.0, 5.0, 6.0]])
    assert AP.select_choice(table, [20, 20, 20]) == 0                             # the silent window wins on +inf: the documented weak case
    assert AP.select_choice(table, [20, 20, 20], min_speech_ratio=0.5) == 1 and AP.select_choice(table, [20, 20, 20], min_speech_ratio=0.7) == 2
    with pytest.raises(ValueError, match=r"no window has a speech_ratio of at least 0.9 \(the best of 3 is 0.75\)"):
        AP.select_choice(table, [20, 20, 20], min_speech_ratio=0.9)


def test_manager_and_route():
    from fastapi.testclient import TestClient
    mgr = serve.TTSManager()
    x16 = np.clip(np.rint(LONG * 32768.0), -32768, 32767).astype(np.float32) / 32768.0          # what the WAV holds
    sel = mgr.select_reference(_wav(LONG), 12.0)
    pair = mgr.select_reference((torch.from_numpy(x16)[None], 24000))
    assert sel.start >= 15 * R.RATE and sel[:3] == pair[:3] and sel.report == pair.report and np.array_equal(sel.windows, pair.windows)
    assert sel.report.rms is not None and sel.report.seconds == (sel.end - sel.start) / 24000
    c = TestClient(serve.create_app(mgr, serve.VoiceRegistry()))
    r = c.post("/v1/audio/reference/select", json=dict(audio=base64.b64encode(_wav(LONG)).decode()))
    assert r.status_code == 200, r.text
    body = r.json()
    assert set(body) == {"seconds", "start", "end", "window", "report", "windows"} and body["seconds"] == 40.0
    assert (body["start"], body["end"], body["window"]) == (sel.start / 24000, sel.end / 24000, sel.window) and body["report"] == sel.report.as_json()
    assert len(body["windows"]) == len(sel.windows) and set(body["windows"][0]) == {"start", "clipped", "speech_frames", "snr_db"}
    for payload, word in ((dict(audio="@@@"), "base64"), (dict(audio=base64.b64encode(b"RIFFxxxx").decode()), "Invalid audio"),
                          (dict(audio=base64.b64encode(_wav(LONG[:48000])).decode(), seconds=2), "multiple of 0.5"),
                          (dict(audio=base64.b64encode(_wav(LONG[:120000])).decode(), seconds=3, min_speech_ratio=1.0), "no window has a speech_ratio"),
                          (dict(audio=base64.b64encode(_wav(np.full(601 * 4000, 0.1, dtype=np.float32), 4000)).decode()), "600 s")):
        r = c.post("/v1/audio/reference/select", json=payload)
        assert r.status_code == 400 and word in r.json()["detail"], r.text
    with pytest.raises(ValueError, match="channels"):
        mgr.select_reference((torch.full((9, 100), 0.1), 24000))
    assert "select" not in " ".join(serve.request_models().CloneRequest.model_fields)
