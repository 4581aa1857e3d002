"""CPU: the watermark scan (`wave_codec.scan_watermark`, written down above it) -- where a long or spliced recording carries a key's mark
and which trace id each stretch holds.  Constants and geometry, the span rule on hand-written scores, equality with the plain-loop
restatement `tests/watermark_scan_ref.py`, a recording spliced from seven parts (clean, through mu-law and through 8 kHz A-law), a mark that
starts after the detector's 60 s, unmarked recordings, and `TTSManager.scan_watermark` / `POST /v1/audio/watermark/scan` over the suite's
stand-in model.  Every figure comes from synthetic speech-like hosts (`watermark_ref.host`), not real speech."""
import base64
import functools
import json

import numpy as np
import pytest
import torch

import watermark_ref as ref
import watermark_scan_ref as sref
from tts_indic_server_f5_amd import infer, serve, wave_codec
from tts_indic_server_f5_amd.wave_codec import WatermarkRange, WatermarkScore, WatermarkSpan, WatermarkTag

from test_watermark_host import _to_24k, _wav24  # noqa: E402
from test_wave_encode_host import client  # noqa: E402,F401  (the stand-in manager behind a TestClient)

R = 24000
P = wave_codec.WATERMARK_PERIOD
KEY = 1
IDS = (123456789, 987654321)


@functools.lru_cache(maxsize=1)
def spliced():
    """(pcm int16 [n], [(first, last + 1) sample of each marked stretch], [the offset each stretch must report]) of the issue's recording."""
    parts = [(ref.host(6 * R, 0), None, 0),
             (wave_codec.mark_pcm16(ref.host(5 * R, 1), WatermarkTag(KEY, IDS[0]))[7001:], IDS[0], 7001),
             (ref.host(4 * R, 2), None, 0),
             (wave_codec.mark_pcm16(ref.host(5 * R, 3), WatermarkTag(KEY, IDS[1])), IDS[1], 0),
             (ref.host(3 * R, 4, True), None, 0),
             (wave_codec.mark_pcm16(ref.host(2 * R, 5), KEY), -1, 0),
             (ref.host(5 * R, 6), None, 0)]
    at, stretches, offsets = 0, [], []
    for pcm, tag, cut in parts:
        if tag is not None:
            stretches.append((at, at + len(pcm)))
            offsets.append((cut - at) % P)                                             # (-start of the uncut marked wave) mod P
        at += len(pcm)
    pcm = np.concatenate([p for p, _, _ in parts])
    pcm.setflags(write=False)
    return pcm, stretches, offsets


def _check_spliced(spans, stretches, offsets, what):
    """Exactly the three spans of key 1, each around its stretch by less than two periods, with the ids and the issue's floors."""
    for s in spans:
        print(f"{what}: {s.start / R:.2f} .. {s.end / R:.2f} s z {s.z:.1f} offset {s.offset} id {s.id} id_z {s.id_z:.1f}")
    assert [s.key for s in spans] == [KEY] * 3, (what, spans)
    assert [s.offset for s in spans] == offsets and [s.id for s in spans] == [IDS[0], IDS[1], None], (what, spans)
    for s, (a, b) in zip(spans, stretches):
        assert s.start % P == 0
        assert 0 <= a - s.start < 2 * P and 0 <= s.end - b < 2 * P, (what, s, a, b)
        assert s.z >= 12.0, (what, s)
    assert min(spans[0].id_z, spans[1].id_z) >= 7.5 and spans[2].id_z < 6.0, (what, spans)


# ------------------------------------------------------------------------------------------------ constants and geometry
def test_constants_and_exports():
    assert (wave_codec.WATERMARK_SCAN_WINDOW, wave_codec.WATERMARK_SCAN_SLACK, wave_codec.WATERMARK_SCAN_MAX_SAMPLES) == (2, 2, 14_400_000)
    assert wave_codec.WATERMARK_SCAN_MAX_SAMPLES == wave_codec.FLAC_MAX_SECONDS * R
    assert WatermarkSpan._fields == ("key", "start", "end", "z", "offset", "id", "id_z")
    for name in ("WATERMARK_SCAN_WINDOW", "WATERMARK_SCAN_SLACK", "WATERMARK_SCAN_MAX_SAMPLES", "WatermarkSpan", "scan_watermark", "watermark_spans"):
        assert getattr(infer, name) is getattr(wave_codec, name), name
    assert wave_codec.WATERMARK_MAX_SAMPLES == 1_440_000                                # the detector's 60 s stay


def test_window_counts_and_short_recordings():
    assert [wave_codec.watermark_windows(n) for n in (12000, P, P + 1, 2 * P, 2 * P + 1)] == [1, 1, 1, 1, 2]
    assert wave_codec.watermark_windows(wave_codec.WATERMARK_SCAN_MAX_SAMPLES) == 878
    y = wave_codec.mark_pcm16(ref.host(12000, 3), KEY)
    assert wave_codec.scan_watermark(y[:11999], [KEY]) == []
    for n in (12000, P, P + 1, 2 * P, 2 * P + 1):                                      # the windows the scan really scores
        x = np.asarray(ref.host(2 * P + 1, 4)[:n], dtype=np.float64) / 32768.0
        seg, rows = wave_codec.scan_window_rows(x)
        assert rows.shape == (wave_codec.watermark_windows(n), P) and seg.shape == (-(-n // P), P)


def test_input_rules():
    over = np.zeros(wave_codec.WATERMARK_SCAN_MAX_SAMPLES + 1, dtype=np.int16)
    with pytest.raises(ValueError, match="14400001 samples.*14400000"):
        wave_codec.scan_watermark(over, [KEY])
    x = ref.host(R, 0).astype(np.float32) / 32768.0
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[100] = bad
        with pytest.raises(ValueError) as mine:
            wave_codec.scan_watermark(y, [KEY])
        with pytest.raises(ValueError) as theirs:
            wave_codec.detect_watermark(y, [KEY])
        assert str(mine.value) == str(theirs.value)
    with pytest.raises(ValueError) as mine:
        wave_codec.scan_watermark(ref.host(R, 0).astype(np.int32), [KEY])
    with pytest.raises(ValueError) as theirs:
        wave_codec.detect_watermark(ref.host(R, 0).astype(np.int32), [KEY])
    assert str(mine.value) == str(theirs.value)
    for bad in ([], [0], list(range(1, 18)), [True], "1"):
        with pytest.raises(ValueError):
            wave_codec.scan_watermark(ref.host(R, 0), bad)
    assert wave_codec.scan_watermark(torch.from_numpy(np.array(ref.host(R, 0))), KEY) == wave_codec.scan_watermark(ref.host(R, 0), [KEY])   # a tensor, one key


# ------------------------------------------------------------------------------------------------ the span rule on hand-written scores
def _rows(*columns, keys=None):
    """scores[w][k] from one column per key: None for an undetected window, an offset for a detected one."""
    keys = keys or list(range(1, len(columns) + 1))
    return [[WatermarkScore(k, 0.0 if col[w] is None else 9.0, 77 if col[w] is None else col[w], col[w] is not None) for k, col in zip(keys, columns)]
            for w in range(len(columns[0]))]


def test_spans_a_run_split_by_an_undetected_window():
    n = 8 * P                                                                           # 8 segments, 7 windows
    got = wave_codec.watermark_spans(_rows([None, 5, 5, None, 5, 5, 5]), n)
    assert got == [WatermarkRange(1, 1, 3, P, 4 * P), WatermarkRange(1, 4, 4, 4 * P, 8 * P)]


def test_spans_split_by_a_jump_of_three_and_kept_across_two_and_the_wrap():
    n = 9 * P
    got = wave_codec.watermark_spans(_rows([10, 12, 15, 17, 19, None, 16383, 1]), n)
    assert got == [WatermarkRange(1, 0, 3, 0, 3 * P), WatermarkRange(1, 2, 4, 2 * P, 6 * P), WatermarkRange(1, 6, 3, 6 * P, 9 * P)]
    assert wave_codec.watermark_spans(_rows([1, 16383, 16382, 0, 3, None, None, None]), n) == [
        WatermarkRange(1, 0, 5, 0, 5 * P), WatermarkRange(1, 4, 2, 4 * P, 6 * P)]      # 16382 -> 0 is two; 0 -> 3 is three
    # the slack is against the PREVIOUS window, not the run's first: a slow drift stays one run
    assert wave_codec.watermark_spans(_rows([0, 2, 4, 6, 8, 10, 12, 14]), n) == [WatermarkRange(1, 0, 9, 0, 9 * P)]


def test_spans_single_window_clipped_end_and_one_window_recordings():
    n = 5 * P + 1000                                                                    # 6 segments, 5 windows
    assert wave_codec.watermark_spans(_rows([None, None, 9, None, None]), n) == [WatermarkRange(1, 2, 2, 2 * P, 4 * P)]
    assert wave_codec.watermark_spans(_rows([None, None, None, None, 9]), n) == [WatermarkRange(1, 4, 2, 4 * P, n)]      # end clipped to n
    assert wave_codec.watermark_spans(_rows([9]), 12000) == [WatermarkRange(1, 0, 1, 0, 12000)]                          # S = 1 < W
    assert wave_codec.watermark_spans(_rows([9]), 2 * P) == [WatermarkRange(1, 0, 2, 0, 2 * P)]
    assert wave_codec.watermark_spans(_rows([None] * 5), n) == []
    with pytest.raises(ValueError, match="5 windows"):
        wave_codec.watermark_spans(_rows([9, 9]), n)


def test_spans_two_keys_interleaved_and_sorted():
    n = 8 * P
    got = wave_codec.watermark_spans(_rows([None, 5, 5, None, None, 7, None], [3, 3, None, None, 4, None, 8], keys=[40, 30]), n)
    assert got == [WatermarkRange(30, 0, 3, 0, 3 * P), WatermarkRange(40, 1, 3, P, 4 * P), WatermarkRange(30, 4, 2, 4 * P, 6 * P),
                   WatermarkRange(40, 5, 2, 5 * P, 7 * P), WatermarkRange(30, 6, 2, 6 * P, 8 * P)]
    same = wave_codec.watermark_spans(_rows([5, None, None, None, None, None, None], [5, None, None, None, None, None, None], keys=[40, 30]), n)
    assert [g.key for g in same] == [40, 30]                                            # equal starts: the keys' order


# ------------------------------------------------------------------------------------------------ the restatement
def _same_as_restatement(pcm, keys):
    got, want = wave_codec.scan_watermark(pcm, keys), sref.scan(pcm, keys)
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        assert (g.key, g.start, g.end, g.offset, g.id) == (w[0], w[1], w[2], w[4], w[5]), (g, w)
        assert g.z == pytest.approx(w[3], abs=1e-9) and g.id_z == pytest.approx(w[6], abs=1e-9), (g, w)
    return got


def test_scan_equals_the_restatement():
    pcm, _, _ = spliced()
    assert len(_same_as_restatement(pcm, [KEY, 2])) == 3
    y = wave_codec.mark_pcm16(ref.host(2 * P + 1, 8), WatermarkTag(KEY, 4242))          # three segments, the last of one sample
    got = _same_as_restatement(y, [2, KEY])
    assert [(s.key, s.start, s.end, s.offset, s.id) for s in got] == [(KEY, 0, 2 * P + 1, 0, 4242)]
    u = wave_codec.watermark_whitened(np.asarray(y, dtype=np.float64) / 32768.0)       # the slabs change nothing: `watermark_fold`'s Z to the bit
    Z = np.zeros(3 * P)
    Z[:len(u)] = u
    assert np.array_equal(Z.reshape(3, P).sum(axis=0), wave_codec.watermark_fold(y))


# ------------------------------------------------------------------------------------------------ the spliced recording
def test_the_spliced_recording():
    pcm, stretches, offsets = spliced()
    assert len(pcm) == 30 * R - 7001 and offsets == [10457, 7449, 12057]
    spans = wave_codec.scan_watermark(pcm, [KEY, 2])
    _check_spliced(spans, stretches, offsets, "clean")
    # what the detector makes of it: one offset, no place, at most one of the two ids
    one = wave_codec.detect_watermark(pcm, [KEY])
    assert len(one) == 1 and one[0].offset in offsets
    assert wave_codec.read_watermark(pcm, [KEY])[0].id in (None,) + IDS


def test_the_spliced_recording_through_g711():
    pcm, stretches, offsets = spliced()
    clean = wave_codec.scan_watermark(pcm, [KEY, 2])
    mulaw = wave_codec.scan_watermark(infer.decode_g711(infer.encode_g711(pcm, "mulaw"), "mulaw"), [KEY, 2])
    _check_spliced(mulaw, stretches, offsets, "mu-law")                                 # (a span may end a segment earlier: containment, not equal edges)
    back = _to_24k(infer.decode_g711(infer.encode_g711(infer.resample_pcm16(pcm, 8000), "alaw"), "alaw"))
    alaw = wave_codec.scan_watermark(back, [KEY, 2])
    _check_spliced(alaw, [(a, min(b, len(back))) for a, b in stretches], offsets, "8 kHz A-law and back")
    assert [(s.start, min(s.end, len(back))) for s in clean] == [(s.start, s.end) for s in alaw]


# ------------------------------------------------------------------------------------------------ past the detector's 60 s
def test_a_mark_after_sixty_seconds():
    tail = wave_codec.mark_pcm16(ref.host(5 * R, 24), WatermarkTag(KEY, 31337))
    pcm = np.concatenate([ref.host(20 * R, 20 + i) for i in range(4)] + [tail])
    assert len(pcm) == 85 * R
    assert wave_codec.detect_watermark(pcm, [KEY])[0].detected is False                 # it reads 60 s
    spans = wave_codec.scan_watermark(pcm, [KEY])
    assert len(spans) == 1, spans
    s = spans[0]
    print(f"85 s: {s.start / R:.2f} .. {s.end / R:.2f} s z {s.z:.1f} id_z {s.id_z:.1f}")
    assert 0 <= 80 * R - s.start < 2 * P and s.end == 85 * R and s.id == 31337 and s.offset == (-80 * R) % P and s.z >= 12.0, s


def test_unmarked_recordings_return_nothing():
    for i in range(3):
        pcm = np.concatenate([ref.host(10 * R, 100 + 6 * i + j) for j in range(6)])
        assert len(pcm) == 60 * R
        assert wave_codec.scan_watermark(pcm, [1, 2, 3, 4]) == [], i


# ------------------------------------------------------------------------------------------------ the manager and the route
def test_manager_and_route(client):
    c, mgr, _ = client
    pcm, stretches, offsets = spliced()
    wav = _wav24(pcm)
    spans = mgr.scan_watermark(wav, [KEY, 2])                                           # no model on a GPU: the host, fp64
    assert spans == wave_codec.scan_watermark(pcm.astype(np.float32) / np.float32(32768.0), [KEY, 2])
    _check_spliced(spans, stretches, offsets, "manager")
    with pytest.raises(ValueError, match="scan_watermark needs keys"):
        mgr.scan_watermark(wav)
    for default in (KEY, {"key": KEY, "id": 5}):                                        # keys=None: the manager's own key
        assert serve.TTSManager(watermark=default).scan_watermark(wav) == mgr.scan_watermark(wav, [KEY])
    body = dict(audio=base64.b64encode(wav).decode(), keys=[KEY, 2])
    r = c.post("/v1/audio/watermark/scan", json=body)
    assert r.status_code == 200, r.text
    out = r.json()
    assert set(out) == {"seconds", "spans"} and out["seconds"] == pytest.approx(len(pcm) / R)
    assert [set(d) for d in out["spans"]] == [{"key", "start", "end", "score", "offset", "id", "id_score"}] * 3
    for d, s in zip(out["spans"], spans):
        assert (d["key"], d["offset"], d["id"]) == (s.key, s.offset, s.id)
        assert d["start"] == s.start / R and d["end"] == s.end / R                      # seconds
        assert d["score"] == pytest.approx(s.z, abs=1e-12) and d["id_score"] == pytest.approx(s.id_z, abs=1e-12)
    assert out["spans"][2]["id"] is None


def test_route_refusals_and_other_uploads(client):
    c, mgr, _ = client
    y = wave_codec.mark_pcm16(ref.host(3 * R, 6), WatermarkTag(31, 424242))
    audio = base64.b64encode(_wav24(y)).decode()
    for body, words in ((dict(audio=audio, keys=[0]), "integer key"), (dict(audio=audio, keys=[]), "watermark keys must be"),
                        (dict(audio=audio, keys=list(range(1, 18))), "watermark keys must be"), (dict(audio=audio, keys=[True]), "integer key"),
                        (dict(audio=audio), "scan_watermark needs keys"),                                            # no key anywhere
                        (dict(audio="@@@", keys=[31]), "base64"), (dict(audio=base64.b64encode(b"RIFFxxxx").decode(), keys=[31]), "Invalid audio")):
        r = c.post("/v1/audio/watermark/scan", json=body)
        assert r.status_code == 400 and words in r.json()["detail"], (body.get("keys"), r.json())
    # over 600 s: the manager's message (a silent mono WAV at 8 kHz keeps the upload small)
    long_wav = serve.wav_bytes(np.zeros(8000 * 600 + 8, dtype=np.int16), 8000).getvalue()
    with pytest.raises(ValueError, match="at most 14400000"):
        mgr.scan_watermark(long_wav, [31])
    r = c.post("/v1/audio/watermark/scan", json=dict(audio=base64.b64encode(long_wav).decode(), keys=[31]))
    assert r.status_code == 400 and "at most 14400000" in r.json()["detail"]
    # a WAV at 44.1 kHz and a FLAC upload
    for upload in (serve.wav_bytes(infer.resample_pcm16(y, 44100), 44100).getvalue(), infer.encode_flac(y, R).tobytes()):
        r = c.post("/v1/audio/watermark/scan", json=dict(audio=base64.b64encode(upload).decode(), keys=[31, 32]))
        assert r.status_code == 200, r.text
        got = r.json()["spans"]
        assert [(d["key"], d["start"], d["offset"], d["id"]) for d in got] == [(31, 0.0, 0, 424242)], got
        assert got[0]["end"] == pytest.approx(3.0, abs=1e-3) and r.json()["seconds"] == pytest.approx(3.0, abs=1e-3)


def test_the_detect_route_answers_as_before(client):
    c, mgr, _ = client
    y = wave_codec.mark_pcm16(ref.host(3 * R, 6), WatermarkTag(31, 424242))
    body = dict(audio=base64.b64encode(_wav24(y)).decode(), keys=[31, 32])
    x = y.astype(np.float32) / np.float32(32768.0)
    plain = [dict(key=s.key, detected=s.detected, score=s.z, offset=s.offset) for s in wave_codec.detect_watermark(x, [31, 32])]
    reads = [dict(key=s.key, detected=s.detected, score=s.z, offset=s.offset, id=s.id, id_score=s.id_z) for s in wave_codec.read_watermark(x, [31, 32])]
    as_bytes = lambda results: json.dumps({"results": results}, ensure_ascii=False, allow_nan=False, separators=(",", ":")).encode()
    assert c.post("/v1/audio/watermark/detect", json=body).content == as_bytes(plain)
    assert c.post("/v1/audio/watermark/detect", json=dict(body, ids=True)).content == as_bytes(reads)
    assert "ScanRequest" in vars(serve.request_models()) and "watermark" in infer.REQUEST_OPTIONS
    assert not any("scan" in name for name in infer.REQUEST_OPTIONS)                    # no new request option
