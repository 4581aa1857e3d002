"""Host side of the waveform back-end (CPU): `audio_prep.remove_silence_pcm` (the reference's `remove_silence_for_generated_wav`,
F/infer/utils_infer.py:530-539) on known answers and against an integer restatement of the silence kernel's rule (csrc/wave_out.h),
`infer.finish_requests` against `request_wave` / `pcm16`, the kernel's closed-form join against `cross_fade_concat`, the `remove_silence`
request option and its refusal on every streaming path, and the routes over `tests/test_serve.py`'s stand-in model.

Every comparison is integer or bit equality: nothing here has a tolerance."""
import io
import wave

import numpy as np
import pytest
import torch

from tts_indic_server_f5_amd import audio_prep, infer, serve

from test_serve import FakeModel, _voice  # noqa: E402

RATE = 24000
F = int(infer.cross_fade_duration * RATE)          # 3600


def _loud(n, seed=0, amp=3000):
    """int16 noise far above the -50 dBFS threshold (rms about `amp`)"""
    return np.clip(np.random.default_rng(seed).standard_normal(n) * amp, -32768, 32767).astype(np.int16)


def _plateau(n, amp, seed=0):
    """constant magnitude `amp` with random signs: every window's sum of squares is exactly amp^2 * n"""
    return (amp * np.sign(np.random.default_rng(seed).standard_normal(n) + 1e-9)).astype(np.int16)


# ------------------------------------------------------------------------------------------------ remove_silence_pcm: known answers
def test_a_pause_shrinks_to_500_ms_on_each_side():
    x = np.concatenate([_loud(2 * RATE, 1), np.zeros(int(2.5 * RATE), dtype=np.int16), _loud(2 * RATE, 2)])
    y = audio_prep.remove_silence_pcm(x)
    # silent windows start at 2000 .. 3500 ms -> the silent range is [2000, 4500]; kept: [0, 2500) and [4000, 6500) ms
    assert y.dtype == np.int16 and np.array_equal(y, np.concatenate([x[:24 * 2500], x[24 * 4000:]]))
    assert len(x) - len(y) == 24 * 1500


@pytest.mark.parametrize("n", [24 * 3000, 24 * 3000 + 5, 24 * 3000 + 20])
def test_no_pause_keeps_the_whole_milliseconds(n):
    x = _loud(n, 3)
    len_ms = len(audio_prep.PcmSegment(x, RATE))
    assert np.array_equal(audio_prep.remove_silence_pcm(x), x[:min(24 * len_ms, n)])


def test_all_quiet_comes_back_empty_and_a_short_wave_whole():
    y = audio_prep.remove_silence_pcm(_plateau(3 * RATE, 50))
    assert y.dtype == np.int16 and y.shape == (0,)
    short = _plateau(RATE // 2, 50)                      # under 1 s: no window fits, nothing is silent
    assert np.array_equal(audio_prep.remove_silence_pcm(short), short)


def test_amplitude_103_is_silent_and_104_is_loud():
    """10^(-50/20) * 32768 = 103.62: a plateau of 103 has rms 103 (silent), one of 104 has S = 10816 n exactly (loud)."""
    for amp, removed in ((103, 24 * 1500), (104, 0)):
        x = np.concatenate([_loud(2 * RATE, 4), _plateau(int(2.5 * RATE), amp), _loud(2 * RATE, 5)])
        y = audio_prep.remove_silence_pcm(x)
        assert len(x) - len(y) == removed, amp
        if removed:
            assert np.array_equal(y, np.concatenate([x[:24 * 2500], x[24 * 4000:]]))
    with pytest.raises(ValueError):
        audio_prep.remove_silence_pcm(np.zeros(10, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ the silence kernel's rule on integers
def kept_ranges(x):
    """csrc/wave_out.h wave_silence_kernel restated: the kept sample ranges [(sa, sb)] of mono int16 samples at 24 kHz, integers only."""
    N = len(x)
    whole, rem = divmod(N, 24)
    len_ms = whole + (1 if rem > 12 or (rem == 12 and whole % 2 == 1) else 0)      # Python's round: half to even
    if len_ms < 1000:
        return [(0, min(24 * len_ms, N))]
    sq = x.astype(np.int64) ** 2
    nc = (N + 239) // 240
    cells = np.array([int(sq[240 * c:240 * c + 240].sum()) for c in range(nc)], dtype=np.int64)     # 10 ms cells, the last one partial
    last = len_ms - 1000
    A = last // 10 + 1                                                             # aligned windows: starts 0, 10, ..., 10 (A - 1)
    flag = np.zeros(A, dtype=np.int64)
    for i in range(A):
        n = min(24 * (10 * i + 1000), N) - 240 * i
        flag[i] = int(cells[i:min(i + 100, nc)].sum()) < 10816 * n
    cnt = np.concatenate([[0], np.cumsum(flag)])
    extra_silent = False
    if last % 10:                                                                  # the unaligned window at `last`, from the samples
        a, b = 24 * last, min(24 * len_ms, N)
        extra_silent = int(sq[a:b].sum()) < 10816 * (b - a)
    comps, cur = [], None                                                          # silent ranges [start_ms, end_ms, last window]
    for b in range((A + 99) // 100):                                               # at most one range start and one range end per bucket
        st = en = -1
        for i in range(100 * b, min(100 * b + 100, A)):
            if flag[i]:
                if cnt[i] == cnt[max(i - 100, 0)]:
                    assert st < 0
                    st = i
                if cnt[min(i + 101, A)] == cnt[i + 1]:
                    assert en < 0
                    en = i
        if st >= 0:
            cur = 10 * st
        if en >= 0:
            comps.append([cur, 10 * en + 1000, en])
    if extra_silent:
        if comps and last <= 10 * comps[-1][2] + 1000:
            comps[-1][1] = len_ms
        else:
            comps.append([last, len_ms, -1])
    out, prev_end, first = [], 0, True
    for s, e, _ in comps + ([] if comps and comps[-1][1] == len_ms else [[len_ms, None, None]]):
        if not (first and prev_end == 0 and s == 0):
            out.append((24 * max(prev_end - 500, 0), min(24 * min(s + 500, len_ms), N)))
        first, prev_end = False, e
    return out


def _with_pauses(n, seed):
    rng = np.random.default_rng(seed)
    x = _loud(n, seed)
    for _ in range(int(rng.integers(1, 5))):
        a, length, amp = int(rng.integers(0, n)), int(rng.integers(12000, 90000)), int(rng.choice([0, 50, 103, 104, 200]))
        x[a:a + length] = _plateau(len(x[a:a + length]), amp, seed) if amp else 0
    if seed % 3 == 0:
        x[:int(rng.integers(20000, 40000))] = 0          # a silent head ...
    if seed % 4 == 0:
        x[-int(rng.integers(20000, 40000)):] = 0         # ... and tail
    return x


@pytest.mark.parametrize("rem", [0, 11, 12, 13, 23])
@pytest.mark.parametrize("whole", [5000, 5001, 5007, 5010, 1000, 1007, 999])      # len_ms even / odd at rem 12; (len_ms - 1000) % 10 in {0, 7, ..}
def test_integer_rule_equals_remove_silence_pcm(whole, rem):
    n = 24 * whole + rem
    for seed in range(4):
        x = _with_pauses(n, seed + 10 * rem)
        want = audio_prep.remove_silence_pcm(x)
        r = kept_ranges(x)
        got = np.concatenate([x[a:b] for a, b in r]) if r else np.zeros(0, dtype=np.int16)
        assert np.array_equal(want, got), (n, seed, r)


def test_the_cases_cover_both_roundings_and_window_layouts():
    lens = {(w, r): len(audio_prep.PcmSegment(np.zeros(24 * w + r, dtype=np.int16), RATE)) for w in (5000, 5001, 5007, 5010) for r in (0, 12, 13)}
    assert lens[5000, 12] == 5000 and lens[5001, 12] == 5002 and lens[5000, 13] == 5001          # half to even, both ways
    assert (lens[5000, 0] - 1000) % 10 == 0 and (lens[5007, 0] - 1000) % 10 == 7


def test_integer_threshold_equals_the_host_threshold_at_the_boundary():
    """S < 10816 n against int(sqrt(float(S) / n)) <= 10^(-50/20) * 32768 around S = 10816 n, for every window length the rule meets."""
    thresh = (10 ** (-50 / 20.0)) * 32768.0
    for n in (24000, 23999, 23989, 12007, 240, 1):
        for d in (-2, -1, 0, 1, 2):
            S = 10816 * n + d
            assert (int(np.sqrt(float(S) / n)) <= thresh) == (S < 10816 * n), (n, d)


# ------------------------------------------------------------------------------------------------ finish_requests, back-end off
def _chunks(lengths, seed):
    rng = np.random.default_rng(seed)
    return [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lengths]


def test_finish_requests_off_equals_request_wave_and_pcm16():
    reqs = [_chunks([9000], 1), _chunks([7200, 7201, 9003], 2), _chunks([5000, 4000], 3), _chunks([30011, 7200], 4)]   # (one with chunks < 2 F)
    texts = ["a", "b", ["head"], "d"]
    floats = infer.finish_requests(reqs, texts, infer.cross_fade_duration)
    pcms = infer.finish_requests(reqs, texts, infer.cross_fade_duration, want="pcm16")
    for waves, text, f, p in zip(reqs, texts, floats, pcms):
        want = infer.request_wave(text, waves, infer.cross_fade_duration)
        if isinstance(text, list):
            assert all(np.array_equal(a, b) for a, b in zip(f, want)) and all(np.array_equal(a, b) for a, b in zip(p, want))
        else:
            assert f.dtype == np.float32 and np.array_equal(f, want)
            assert p.dtype == np.int16 and p.tobytes() == serve.pcm16(want)
    # a flagged request is remove_silence_pcm of its quantised joined wave, whatever `want`
    quiet = [np.concatenate([c, np.zeros(2 * RATE, dtype=np.float32), c]) for c in _chunks([30000, 30000], 5)]
    for want_kind in ("float", "pcm16"):
        got, = infer.finish_requests([quiet], ["x"], infer.cross_fade_duration, [True], want=want_kind)
        ref = audio_prep.remove_silence_pcm(infer.quantise_pcm16(infer.request_wave("x", quiet, infer.cross_fade_duration)))
        assert got.dtype == np.int16 and np.array_equal(got, ref) and len(ref) < len(quiet[0]) * 2 - F
    with pytest.raises(ValueError):
        infer.finish_requests([quiet], [["x"]], infer.cross_fade_duration, [True])
    with pytest.raises(ValueError):
        infer.finish_requests([quiet], ["x"], infer.cross_fade_duration, device_backend=True)          # the device path produces PCM only
    # chunk waves that are not on a HIP device take the host path even with the back-end on, and are counted
    infer.backend_stats.clear()
    got = infer.finish_requests([[torch.from_numpy(c) for c in r] for r in reqs[:2]], texts[:2], infer.cross_fade_duration, device_backend=True, want="pcm16")
    assert all(np.array_equal(g, p) for g, p in zip(got, pcms[:2]))
    assert infer.backend_stats["host_requests"] == 2 and infer.backend_stats["device_requests"] == 0


# ------------------------------------------------------------------------------------------------ the kernel's closed form
def closed_form_join(waves, fade):
    """csrc/wave_out.h wave_join_kernel restated: a gather with two products and one sum per faded sample, in fp64, rounded to fp32."""
    if len(waves) == 1:
        return waves[0].astype(np.float32)
    ramp = np.arange(fade, dtype=np.float64) * (1.0 / (fade - 1))
    ramp[fade - 1] = 1.0
    pos, parts = 0, []
    for c, w in enumerate(waves):
        lo = fade if c > 0 else 0
        hi = len(w) - fade if c + 1 < len(waves) else len(w)
        if c > 0:
            prev = waves[c - 1]
            parts.append(prev[len(prev) - fade:].astype(np.float64) * ramp[::-1] + w[:fade].astype(np.float64) * ramp)
        parts.append(w[lo:hi].astype(np.float64))
    return np.concatenate(parts).astype(np.float32)


def test_ramp_is_linspace_bit_for_bit():
    for fade in (2, 3, 7, 2400, F, 4801):
        ramp = np.arange(fade, dtype=np.float64) * (1.0 / (fade - 1))
        ramp[fade - 1] = 1.0
        assert np.array_equal(ramp, np.linspace(0, 1, fade))


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_closed_form_join_equals_cross_fade_concat(k):
    for lengths in ([2 * F] * k, [2 * F + 1] * k, [3 * F + 17] * k, [2 * F, 3 * F + 17, 2 * F + 1, 2 * F][:k]):
        waves = _chunks(lengths, k + len(lengths) + lengths[0])
        want = np.asarray(infer.cross_fade_concat(waves, infer.cross_fade_duration), dtype=np.float32)
        got = closed_form_join(waves, F)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), lengths


def test_closed_form_does_not_hold_below_two_fades():
    """Why the call refuses such requests: with a chunk of F + 100 samples between two long ones the reference's nested fades overlap."""
    waves = _chunks([3 * F, F + 100, 3 * F], 9)
    want = np.asarray(infer.cross_fade_concat(waves, infer.cross_fade_duration), dtype=np.float32)
    pos = [0, 3 * F - F, 3 * F - F + 100]
    assert len(want) == pos[2] + 3 * F          # (the length still follows the closed form; the samples do not)
    mid = want[pos[1]:pos[1] + F]
    plain = (waves[0][2 * F:].astype(np.float64) * np.linspace(0, 1, F)[::-1] + waves[1][:F].astype(np.float64) * np.linspace(0, 1, F)).astype(np.float32)
    assert not np.array_equal(mid, plain)


# ------------------------------------------------------------------------------------------------ the option
def test_remove_silence_option_is_validated():
    assert "remove_silence" in infer.REQUEST_OPTIONS and "remove_silence" not in serve.EDIT_OPTIONS
    assert serve.check_request_options(dict(remove_silence=True)) == dict(remove_silence=True)
    assert serve.check_request_options(dict(remove_silence=False)) == {} and serve.check_request_options(dict(remove_silence=None)) == {}
    for bad in (1, 0, "true", 1.0, [True]):
        with pytest.raises(ValueError, match="remove_silence"):
            serve.check_request_options(dict(remove_silence=bad))
    with pytest.raises(ValueError, match="unknown option"):
        serve.check_request_options(dict(remove_silence=True), allowed=serve.EDIT_OPTIONS)
    assert serve.DEVICE_BACKEND_DEFAULT is False and serve.TTSManager().device_backend is False
    assert serve.TTSManager(device_backend=True).device_backend is True


class PauseVocoder:
    """Vocos stand-in whose wave holds a 1.5 s pause from 0.5 s on"""
    def decode(self, mel):
        n = mel.shape[-1] * 256
        w = 0.25 * torch.sin(torch.arange(n) * 0.05)
        w[RATE // 2:RATE // 2 + 3 * RATE // 2] = 0.0
        return w[None]


LONG_TEXT = "hello world, this is a test of a sentence that is long enough for three seconds."


@pytest.fixture()
def manager(tmp_path):
    path = _voice(tmp_path)
    mgr = serve.TTSManager(nfe_step=4).load(FakeModel(), PauseVocoder())
    return mgr, path


def test_manager_remove_silence_and_streaming_refusals(manager):
    mgr, path = manager
    plain = mgr.synthesize(LONG_TEXT, ref_audio_path=path, ref_text="reference words")
    cut = mgr.synthesize(LONG_TEXT, ref_audio_path=path, ref_text="reference words", remove_silence=True)
    assert plain.dtype == np.float32 and cut.dtype == np.int16
    assert np.array_equal(cut, audio_prep.remove_silence_pcm(infer.quantise_pcm16(plain))) and len(plain) - len(cut) == 24 * 500
    with pytest.raises(ValueError, match="remove_silence"):
        mgr.synthesize(LONG_TEXT, ref_audio_path=path, ref_text="reference words", remove_silence="yes")
    with pytest.raises(ValueError, match="streaming"):
        mgr.synthesize_stream(LONG_TEXT, ref_audio_path=path, ref_text="reference words", remove_silence=True)
    with open(path, "rb") as f:
        raw = f.read()
    with pytest.raises(ValueError, match="streaming"):
        mgr.synthesize_clip_stream(LONG_TEXT, raw, "reference words", remove_silence=True)
    clip_cut = mgr.synthesize_clip(LONG_TEXT, raw, "reference words", remove_silence=True)
    clip_plain = mgr.synthesize_clip(LONG_TEXT, raw, "reference words")
    assert clip_cut.dtype == np.int16 and len(clip_plain) - len(clip_cut) == 24 * 500
    # list texts are how a stream reaches infer_requests: refused there too, and so is join=False
    voice, ref_text = mgr._voice(path, "reference words")
    with pytest.raises(ValueError, match="whole wave"):
        infer.infer_requests([(voice, ref_text, ["a chunk."], dict(remove_silence=True))], mgr.model_obj, mgr.vocoder, nfe_step=4)
    with pytest.raises(ValueError, match="whole wave"):
        infer.infer_requests([(voice, ref_text, LONG_TEXT, dict(remove_silence=True))], mgr.model_obj, mgr.vocoder, nfe_step=4, join=False)
    (wave, sr, spec), = infer.infer_requests([(voice, ref_text, LONG_TEXT, dict(remove_silence=True))], mgr.model_obj, mgr.vocoder, nfe_step=4)
    assert sr == RATE and np.array_equal(wave, cut) and spec.shape[0] == 100
    # with the back-end on, CPU stand-ins fall back to the host path: same bytes, int16 either way
    on = serve.TTSManager(nfe_step=4, device_backend=True).load(FakeModel(), PauseVocoder())
    got = on.synthesize(LONG_TEXT, ref_audio_path=path, ref_text="reference words")
    assert got.dtype == np.int16 and serve.wav_bytes(got).getvalue() == serve.wav_bytes(plain).getvalue()


def _frames(content):
    with wave.open(io.BytesIO(content), "rb") as f:
        assert f.getframerate() == RATE and f.getnchannels() == 1 and f.getsampwidth() == 2
        return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")


def test_routes_take_remove_silence(tmp_path):
    import base64
    from fastapi.testclient import TestClient
    reg = serve.VoiceRegistry()
    path = _voice(tmp_path)
    reg.add("KAN_F (Happy)", path, "reference words")
    mgr = serve.TTSManager(nfe_step=4).load(FakeModel(), PauseVocoder())
    c = TestClient(serve.create_app(mgr, reg))
    plain = c.post("/v1/audio/speech", json={"text": LONG_TEXT})
    cut = c.post("/v1/audio/speech", json={"text": LONG_TEXT, "remove_silence": True})
    assert plain.status_code == 200 and cut.status_code == 200 and cut.headers["content-type"] == "audio/wav"
    a, b = _frames(plain.content), _frames(cut.content)
    assert len(a) - len(b) == 24 * 500 and np.array_equal(b, audio_prep.remove_silence_pcm(a))
    r = c.post("/v1/audio/speech/voice", json={"text": LONG_TEXT, "ref_audio_name": "KAN_F (Happy)", "remove_silence": True})
    assert r.status_code == 200 and np.array_equal(_frames(r.content), b)
    with open(path, "rb") as f:
        clip = base64.b64encode(f.read()).decode()
    r = c.post("/v1/audio/speech/clone", json={"text": LONG_TEXT, "ref_audio": clip, "ref_text": "reference words", "remove_silence": True})
    assert r.status_code == 200 and len(_frames(r.content)) == len(b)
    for route, body in (("/v1/audio/speech", {"text": LONG_TEXT}), ("/v1/audio/speech/voice", {"text": LONG_TEXT, "ref_audio_name": "KAN_F (Happy)"}),
                        ("/v1/audio/speech/clone", {"text": LONG_TEXT, "ref_audio": clip, "ref_text": "reference words"})):
        r = c.post(route, json=dict(body, stream=True, remove_silence=True))
        assert r.status_code == 400 and "streaming" in r.json()["detail"], route
        assert c.post(route, json=dict(body, stream=True, remove_silence=False)).status_code == 200
