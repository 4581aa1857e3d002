"""Host side of cloning from an uploaded clip (CPU): `infer.resample_taps` against `resample_sinc_hann`, the vectorised silence code of
`audio_prep` against the loop versions it replaced (kept below, verbatim, as the yardstick), `preprocess_ref_segment`, the deferred
`PreparedVoice`, and the `/v1/audio/speech/clone` route over a stand-in sampler: responses, refusals, the LRU cache and its per-key lock."""
import base64
import io
import math
import threading
import wave

import numpy as np
import pytest
import torch

from tts_indic_server_f5_amd import audio_prep, infer, serve
from tts_indic_server_f5_amd.audio_prep import PcmSegment

RATES = [48000, 16000, 44100, 22050, 11025]


# ------------------------------------------------------------------------------------------------ resample_taps
def _resample_before(wave_, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """`resample_sinc_hann` as it was before it was built on `resample_taps`"""
    g = math.gcd(int(orig_freq), int(new_freq))
    of, nf = int(orig_freq) // g, int(new_freq) // g
    base_freq = min(of, nf) * rolloff
    width = math.ceil(lowpass_filter_width * of / base_freq)
    idx = torch.arange(-width, width + of, dtype=torch.float64)[None, None] / of
    t = torch.arange(0, -nf, -1, dtype=torch.float64)[:, None, None] / nf + idx
    t = (t * base_freq).clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base_freq / of)
    kernels = kernels.to(torch.float32)
    shape = wave_.shape
    w = wave_.reshape(-1, shape[-1]).to(torch.float32)
    length = w.shape[-1]
    w = torch.nn.functional.pad(w, (width, width + of))
    out = torch.nn.functional.conv1d(w[:, None], kernels, stride=of)
    out = out.transpose(1, 2).reshape(w.shape[0], -1)
    target = math.ceil(nf * length / of)
    return out[..., :target].reshape(*shape[:-1], target)


@pytest.mark.parametrize("sr", [16000, 44100, 22050, 48000])
def test_resample_sinc_hann_keeps_its_bits(sr):
    x = torch.randn(2, 5003, generator=torch.Generator().manual_seed(sr))
    got, want = infer.resample_sinc_hann(x, sr, 24000), _resample_before(x, sr, 24000)
    assert got.shape == want.shape and torch.equal(got, want)


@pytest.mark.parametrize("sr", [16000, 48000, 44100])
def test_taps_are_what_the_resampler_convolves_with(sr):
    """A one-hot input at position i of xpad's second polyphase block reads column k = i + width - q * of of the table at block q: every
    column of every phase comes back exactly (1.0 * tap + zeros)."""
    of, nf, width, taps = infer.resample_taps(sr, 24000)
    L = taps.shape[1]
    assert taps.shape == (nf, 2 * width + of) and taps.dtype == torch.float32 and L == 2 * width + of
    assert infer.resample_taps(sr, 24000)[3] is taps                       # cached per rate pair
    n = 4 * of + 2 * width
    for i in range(width + of, width + 2 * of):                            # one polyphase block, away from both edges
        x = torch.zeros(1, n)
        x[0, i] = 1.0
        y = infer.resample_sinc_hann(x, sr, 24000)[0]
        for q in range(y.shape[0] // nf):
            k = i + width - q * of
            want = taps[:, k] if 0 <= k < L else torch.zeros(nf)
            assert torch.equal(y[q * nf:(q + 1) * nf], want), (i, q)


def test_tap_table_sizes_and_the_refused_pair():
    sizes = {sr: infer.resample_taps(sr, 24000)[3].numel() * 4 for sr in RATES}
    assert sizes == {48000: 112, 16000: 192, 44100: 80 * 171 * 4, 22050: 160 * 161 * 4, 11025: 320 * 161 * 4}
    with pytest.raises(ValueError, match="tap table"):
        infer.resample_taps(44101, 24000)
    with pytest.raises(ValueError, match="tap table"):
        infer.resample_sinc_hann(torch.zeros(1, 10), 44101, 24000)


@pytest.mark.parametrize("sr", RATES + [24000])
def test_deferred_voice_knows_its_lengths(sr):
    g = math.gcd(sr, 24000)
    of = sr // g
    for n in sorted({1, max(of - 1, 1), of, of + 1, 10 * of + 7}):
        wav = 0.2 * torch.randn(2, n, generator=torch.Generator().manual_seed(n))
        eager, lazy = infer.PreparedVoice((wav, sr), 0.1), infer.PreparedVoice.deferred((wav, sr), 0.1)
        assert lazy.audio is None and lazy.rms is None and lazy.mel is None and lazy.pending is not None
        assert lazy.seconds == eager.seconds and lazy.ref_frames == eager.ref_frames, (sr, n)
        infer.prepare_voices([lazy], device=None)                          # the host front-end: what a model without the device one gets
        assert lazy.pending is None and torch.equal(lazy.audio, eager.audio) and torch.equal(lazy.rms, eager.rms)


# ------------------------------------------------------------------------------------------------ silence code: the loops it replaced
_MAX_AMP = 32768.0


def _loop_rms_ms(seg, start_ms, end_ms):
    a, b = seg._frame(max(0, min(start_ms, len(seg)))), seg._frame(max(0, min(end_ms, len(seg))))
    n = (b - a) * seg.frames.shape[1]
    if n <= 0:
        return 0
    c = seg._cum_squares()
    return int(math.sqrt(float(c[b] - c[a]) / n))


def _loop_dbfs_ms(seg, start_ms, end_ms):
    r = _loop_rms_ms(seg, start_ms, end_ms)
    return -math.inf if r == 0 else 20.0 * math.log10(r / _MAX_AMP)


def _loop_detect_silence(seg, min_silence_len=1000, silence_thresh=-16, seek_step=1):
    seg_len = len(seg)
    if seg_len < min_silence_len:
        return []
    thresh = (10 ** (silence_thresh / 20.0)) * _MAX_AMP
    last = seg_len - min_silence_len
    starts = list(range(0, last + 1, seek_step))
    if last % seek_step:
        starts.append(last)
    silent = [i for i in starts if _loop_rms_ms(seg, i, i + min_silence_len) <= thresh]
    if not silent:
        return []
    ranges = []
    prev = silent[0]
    cur = prev
    for i in silent[1:]:
        if i != prev + seek_step and i > prev + min_silence_len:
            ranges.append([cur, prev + min_silence_len])
            cur = i
        prev = i
    ranges.append([cur, prev + min_silence_len])
    return ranges


def _loop_detect_nonsilent(seg, min_silence_len=1000, silence_thresh=-16, seek_step=1):
    silent = _loop_detect_silence(seg, min_silence_len, silence_thresh, seek_step)
    n = len(seg)
    if not silent:
        return [[0, n]]
    if silent[0][0] == 0 and silent[0][1] == n:
        return []
    out, prev_end, end = [], 0, 0
    for start, end in silent:
        out.append([prev_end, start])
        prev_end = end
    if end != n:
        out.append([prev_end, n])
    if out[0] == [0, 0]:
        out.pop(0)
    return out


def _loop_split_on_silence(seg, min_silence_len=1000, silence_thresh=-16, keep_silence=100, seek_step=1):
    ranges = [[s - keep_silence, e + keep_silence] for s, e in _loop_detect_nonsilent(seg, min_silence_len, silence_thresh, seek_step)]
    for a, b in zip(ranges, ranges[1:]):
        if b[0] < a[1]:
            a[1] = (a[1] + b[0]) // 2
            b[0] = a[1]
    return [seg.slice_ms(max(s, 0), min(e, len(seg))) for s, e in ranges]


def _loop_detect_leading_silence(seg, silence_threshold=-50.0, chunk_size=10):
    trim = 0
    while _loop_dbfs_ms(seg, trim, trim + chunk_size) < silence_threshold and trim < len(seg):
        trim += chunk_size
    return min(trim, len(seg))


def _loop_remove_silence_edges(seg, silence_threshold=-42):
    seg = seg.slice_ms(_loop_detect_leading_silence(seg, silence_threshold), len(seg) + 1)
    end = seg.duration_seconds
    for ms in range(len(seg) - 1, -1, -1):
        if _loop_dbfs_ms(seg, ms, ms + 1) > silence_threshold:
            break
        end -= 0.001
    return seg.slice_ms(0, int(end * 1000))


def _level(db):
    return 32768.0 * 10 ** (db / 20.0)


def _signals(rate, channels, ms):
    """int16 [n, channels] test signals of `ms` milliseconds: tone / pause patterns and noise whose rms straddles the three thresholds"""
    n = int(rate * ms / 1000)
    rng = np.random.default_rng(rate + 7 * channels + ms)
    t = np.arange(n) / rate
    out = {}
    tone = 8000 * np.sin(2 * np.pi * 220 * t)
    gate = np.ones(n)
    for a, b in ((0.0, 0.12), (0.9, 2.1), (4.0, 4.15), (6.5, 8.2), (12.0, 13.3), (16.2, 17.0)):      # pauses, in seconds
        gate[int(a * rate):int(b * rate)] = 0.0
    out["tone_pause"] = tone * gate + rng.normal(0, 2.0, n) * (1 - gate)
    for db in (-50, -42, -40):
        # the level wanders +-1.5 dB around the threshold, slowly, so windows fall on both sides of it
        out[f"noise{db}"] = rng.normal(0, 1.0, n) * _level(db + 1.5 * np.sin(2 * np.pi * 0.7 * t + 1.0))
    out["loud_then_quiet"] = np.where(t < ms / 2000.0, tone, rng.normal(0, _level(-46), n))
    sigs = {}
    for name, x in out.items():
        cols = [x] + [np.roll(x, 17 * c) * (0.9 ** c) for c in range(1, channels)]
        sigs[name] = np.clip(np.rint(np.stack(cols, axis=1)), -32768, 32767).astype(np.int16).reshape(n, channels)
    return sigs


def _same(a, b):
    return a.rate == b.rate and a.frames.shape == b.frames.shape and np.array_equal(a.frames, b.frames)


@pytest.mark.parametrize("ms", [0, 999, 1000, 1001, 17000])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rate", [11025, 22050, 44100])
def test_vectorised_silence_code_equals_the_loops(rate, channels, ms):
    for name, frames in _signals(rate, channels, ms).items():
        seg, tag = PcmSegment(frames, rate), (rate, channels, ms, name)
        for msl, thr, step in ((1000, -50, 10), (100, -40, 10), (1000, -50, 1), (250, -42, 7)):
            if step == 1 and ms > 2000 and name != "tone_pause":
                continue                                                   # (the loop yardstick at seek_step 1 is the slow part)
            want = _loop_detect_silence(seg, msl, thr, step)
            got = audio_prep.detect_silence(seg, msl, thr, step)
            assert got == want and all(type(v) is int for r in got for v in r), tag
            assert audio_prep.detect_nonsilent(seg, msl, thr, step) == _loop_detect_nonsilent(seg, msl, thr, step), tag
            a, b = audio_prep.split_on_silence(seg, msl, thr, 1000, step), _loop_split_on_silence(seg, msl, thr, 1000, step)
            assert len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b)), tag
        for thr in (-50.0, -42, -40):
            assert audio_prep.detect_leading_silence(seg, thr) == _loop_detect_leading_silence(seg, thr), tag
            assert _same(audio_prep.remove_silence_edges(seg, thr), _loop_remove_silence_edges(seg, thr)), tag
        starts = np.arange(0, len(seg) + 3, 13)
        assert audio_prep.PcmSegment.rms_windows(seg, starts, starts + 37).tolist() == [_loop_rms_ms(seg, int(s), int(s) + 37) for s in starts], tag


def _write_wav(path, frames, rate):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(frames.shape[1]); f.setsampwidth(2); f.setframerate(rate)
        f.writeframes(np.ascontiguousarray(frames, dtype="<i2").tobytes())


@pytest.mark.parametrize("clip_short", [True, False])
def test_preprocess_ref_segment_is_what_the_path_version_writes(tmp_path, clip_short):
    frames = _signals(22050, 2, 17000)["tone_pause"]
    src = tmp_path / "long.wav"
    _write_wav(src, frames, 22050)
    path, text = audio_prep.preprocess_ref_audio_text(str(src), "some words", clip_short=clip_short, show_info=lambda *_: None)
    seg = audio_prep.preprocess_ref_segment(PcmSegment(frames, 22050), clip_short, show_info=lambda *_: None)
    assert text == "some words. " == audio_prep.normalize_ref_text("some words")
    assert _same(PcmSegment.from_wav(path), seg)
    assert (len(seg) <= 15050) == clip_short
    with pytest.raises(ValueError, match="11025"):
        audio_prep.preprocess_ref_segment(PcmSegment(frames, 8000), clip_short)


# ------------------------------------------------------------------------------------------------ the clone route
class StandInModel:
    """CFM.sample stand-in whose mel depends on the prompt it was given (its length and mean), so two different prompts cannot pass for
    one another."""

    def __init__(self):
        self.calls = []

    def sample(self, cond, text, duration, steps, cfg_strength, sway_sampling_coef):
        self.calls.append((tuple(cond.shape), text, duration, steps))
        tag = float(cond.abs().mean()) + 1e-6 * cond.shape[-1]
        return torch.full((1, duration, 100), tag), None


class StandInVocoder:
    def decode(self, mel):
        n = mel.shape[-1] * 256
        return float(mel.mean()) * torch.sin(torch.arange(n) * 0.05)[None]


def _tone16(rate=24000, seconds=3.0, amp=9000, freq=200, channels=1):
    x = (amp * np.sin(2 * np.pi * freq * np.arange(int(rate * seconds)) / rate)).astype(np.int16)
    return np.stack([x] * channels, axis=1)


def _wav(frames, rate, sampwidth=2):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as f:
        f.setnchannels(frames.shape[1]); f.setsampwidth(sampwidth); f.setframerate(rate)
        f.writeframes(np.ascontiguousarray(frames, dtype="<i2").tobytes())
    return buf.getvalue()


def _b64(raw):
    return base64.b64encode(raw).decode()


def _pcm(content):
    with wave.open(io.BytesIO(content), "rb") as f:
        assert f.getframerate() == 24000 and f.getnchannels() == 1 and f.getsampwidth() == 2
        return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")


def _stream_pcm(content):
    assert content[:44] == serve.wav_stream_header()
    return np.frombuffer(content[44:], dtype="<i2")


@pytest.fixture()
def served(tmp_path):
    from fastapi.testclient import TestClient
    frames = _tone16()
    assert math.sqrt(float(np.mean((frames / 32768.0) ** 2))) > 0.1
    path = tmp_path / "prompt.wav"
    _write_wav(path, frames, 24000)
    reg = serve.VoiceRegistry()
    reg.add("KAN_F (Happy)", str(path), "reference words")
    mgr = serve.TTSManager(nfe_step=4)
    return TestClient(serve.create_app(mgr, reg)), mgr, StandInModel(), _wav(frames, 24000), str(path)


TEXT = "hello world, this is a test. And a second sentence, so that there is something to join."


def test_clone_route_contract(served):
    c, mgr, model, raw, path = served
    body = {"text": TEXT, "ref_audio": _b64(raw), "ref_text": "reference words"}
    r = c.post("/v1/audio/speech/clone", json=body)
    assert r.status_code == 503 and r.json()["detail"] == "TTS model not loaded"
    mgr.load(model, StandInVocoder())
    r = c.post("/v1/audio/speech/clone", json=body)
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and "synthesized_speech.wav" in r.headers["content-disposition"]
    pcm = _pcm(r.content)
    want = mgr.synthesize(TEXT, ref_audio_path=path, ref_text="reference words")
    assert len(pcm) > 0 and np.array_equal(pcm, np.frombuffer(serve.pcm16(want), dtype="<i2"))
    assert np.array_equal(mgr.synthesize_clip(TEXT, raw, "reference words"), want)
    assert "".join(model.calls[-1][1][0]).startswith("reference words.  hello world")
    r = c.post("/v1/audio/speech/clone", json=dict(body, stream=True))
    assert r.status_code == 200 and np.array_equal(_stream_pcm(r.content), pcm)
    assert np.array_equal(np.concatenate(list(mgr.synthesize_clip_stream(TEXT, raw, "reference words"))), want)
    # a (wave, sr) pair instead of the file's bytes; a different clip gives a different result
    assert np.array_equal(mgr.synthesize_clip(TEXT, infer.load_wav(raw), "reference words"), want)
    other = mgr.synthesize_clip(TEXT, _wav(_tone16(amp=5000, seconds=2.0), 24000), "reference words")
    assert other.shape != want.shape or not np.array_equal(other, want)
    # the three routes that were there still answer
    assert c.post("/v1/audio/speech", json={"text": "again"}).status_code == 200


def test_clone_route_refusals(served):
    c, mgr, model, raw, _ = served
    mgr.load(model, StandInVocoder())

    def post(**kw):
        r = c.post("/v1/audio/speech/clone", json=dict(dict(text="hello there.", ref_audio=_b64(raw), ref_text="reference words"), **kw))
        return r.status_code, r.json().get("detail") if r.status_code != 200 else None

    assert post(text="   ") == (400, "Text to synthesize cannot be empty.")
    assert post(ref_text="  ") == (400, "Reference text cannot be empty.")
    assert post(ref_audio="not base64 !!") == (400, "Audio must be a base64-encoded WAV file.")
    code, detail = post(ref_audio=_b64(b"RIFFxxxxWAVEjunk"))
    assert code == 400 and detail.startswith("Invalid audio: ")
    code, detail = post(ref_audio=_b64(b"fLaC" + bytes(40)))
    assert code == 400 and detail.startswith("Invalid audio: not a WAV file")
    code, detail = post(ref_audio=_b64(_wav(_tone16(rate=8000), 8000)))
    assert code == 400 and "11025" in detail
    code, detail = post(ref_audio=_b64(_wav(np.zeros((24000, 1), dtype=np.int16), 24000)))
    assert code == 400 and "silent" in detail
    code, detail = post(ref_audio=_b64(_wav(_tone16(rate=44101), 44101)))
    assert code == 400 and "tap table" in detail
    assert post(nfe_step=0)[0] == 400 and post(speed=-1.0)[0] == 400 and post(ode_method="heun")[0] == 400
    # non-finite samples: an IEEE-float WAV with a NaN in it
    x = (0.3 * np.sin(np.arange(24000) * 0.05)).astype("<f4")
    x[100] = np.nan
    hdr = b"RIFF" + (36 + 4 * len(x)).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") + \
        (3).to_bytes(2, "little") + (1).to_bytes(2, "little") + (24000).to_bytes(4, "little") + (96000).to_bytes(4, "little") + \
        (4).to_bytes(2, "little") + (32).to_bytes(2, "little") + b"data" + (4 * len(x)).to_bytes(4, "little")
    code, detail = post(ref_audio=_b64(hdr + x.tobytes()))
    assert code == 400 and "non-finite" in detail
    with pytest.raises(ValueError, match="non-finite"):
        mgr.synthesize_clip("hello.", (torch.full((1, 24000), float("inf")), 24000), "reference words")
    assert model.calls == []                                               # nothing reached the sampler
    # a float WAV without the NaN is quantised like clip(round(x * 32768)) and accepted
    x[100] = 0.0
    assert post(ref_audio=_b64(hdr + x.tobytes()))[0] == 200


def test_uploads_are_prepared_once_and_the_cache_is_an_lru(served, monkeypatch):
    c, mgr, model, raw, _ = served
    mgr.load(model, StandInVocoder())
    seen = []
    real = audio_prep.preprocess_ref_segment
    monkeypatch.setattr(audio_prep, "preprocess_ref_segment", lambda seg, *a, **k: (seen.append(seg.frames.shape[0]), real(seg, *a, **k))[1])
    for _ in range(3):
        mgr.synthesize_clip("hello.", raw, "reference words")
    assert len(seen) == 1
    mgr.synthesize_clip("hello.", raw, "other words")                       # another transcript: another voice
    mgr.synthesize_clip("hello.", raw, "reference words", clip_short=False)
    assert len(seen) == 3

    small = serve.TTSManager(nfe_step=4).load(model, StandInVocoder())
    assert small.clip_cache == 64
    clips = [_wav(_tone16(seconds=0.3, freq=100 + 5 * i), 24000) for i in range(65)]
    seen.clear()
    for clip in clips[:64]:
        small._clip_voice(clip, "reference words")
    small._clip_voice(clips[0], "reference words")                          # still there, and now the most recently used
    assert len(seen) == 64
    small._clip_voice(clips[64], "reference words")                         # the 65th distinct upload evicts the least recently used: clip 1
    small._clip_voice(clips[0], "reference words")
    assert len(seen) == 65
    small._clip_voice(clips[1], "reference words")
    assert len(seen) == 66
    small = serve.TTSManager(nfe_step=4, clip_cache=64).load(model, StandInVocoder())
    seen.clear()
    for clip in clips:                                                      # 65 distinct uploads, none touched again: the first one is gone
        small._clip_voice(clip, "reference words")
    small._clip_voice(clips[0], "reference words")
    assert len(seen) == 66


def test_two_uploads_do_not_wait_for_each_other(served, monkeypatch):
    c, mgr, model, raw, _ = served
    mgr.load(model, StandInVocoder())
    slow = _wav(_tone16(seconds=1.0, freq=300), 24000)
    inside, release = threading.Event(), threading.Event()
    real = audio_prep.preprocess_ref_segment

    def pre_step(seg, *a, **k):
        if seg.frames.shape[0] == 24000:                                   # the slow upload: parks inside its pre-step
            inside.set()
            assert release.wait(timeout=30)
        return real(seg, *a, **k)

    monkeypatch.setattr(audio_prep, "preprocess_ref_segment", pre_step)
    result = {}
    t = threading.Thread(target=lambda: result.setdefault("slow", mgr._clip_voice(slow, "reference words")))
    t.start()
    try:
        assert inside.wait(timeout=30)
        voice, _ = mgr._clip_voice(raw, "reference words")                  # completes while the other is still being prepared
        assert voice is not None and not release.is_set() and "slow" not in result
        # the same upload a second time waits for the first preparation instead of repeating it
        t2 = threading.Thread(target=lambda: result.setdefault("again", mgr._clip_voice(slow, "reference words")))
        t2.start()
    finally:
        release.set()
        t.join(timeout=30)
    t2.join(timeout=30)
    assert result["slow"][0] is result["again"][0]


# ------------------------------------------------------------------------------------------------ continuous batching and sharding
class _Ticket:
    def __init__(self, request):
        self.request, self.left, self.result, self.cancelled = request, 3, None, False

    def cancel(self):
        self.cancelled = True


class StandInScheduler:
    """The surface `serve.ContinuousBatcher` drives, with requests that take three spans; `prepare` is `infer.SpanScheduler`'s own."""
    prepare = infer.SpanScheduler.prepare

    def __init__(self, model_obj=None, gate=None):
        self.model_obj, self.gate = model_obj, gate
        self.in_flight, self.span_units, self.spans = [], [], []

    @property
    def busy(self):
        return bool(self.in_flight)

    def admit(self, request):
        if self.gate is not None and request[2] == "gate":
            assert self.gate.wait(timeout=30)
        if isinstance(request[0], infer.PreparedVoice):
            request[0].cond(self.model_obj)                                # what the real admit does first
        ticket = _Ticket(request)
        self.in_flight.append(ticket)
        return ticket

    def step(self):
        self.spans.append([t.request[2] for t in self.in_flight])
        self.span_units.append(len(self.in_flight))
        for t in self.in_flight:
            t.left -= 1
        done = [t for t in self.in_flight if t.left == 0]
        for t in done:
            t.result = t.request[2]
        self.in_flight = [t for t in self.in_flight if t.left > 0]
        return done

    def take_in_flight(self):
        taken, self.in_flight = self.in_flight, []
        return taken


def test_a_streams_tail_still_boards_with_its_head():
    """What `on_start` submits during an admission is admitted at the same boundary: head and tail advance together from the first span."""
    sched = StandInScheduler()
    batcher = serve.ContinuousBatcher(sched)
    try:
        tail = {}
        head = batcher.submit(("voice", "ref", "head"), on_start=lambda: tail.setdefault("f", batcher.submit(("voice", "ref", "tail"))))
        assert head.result(timeout=30) == "head" and tail["f"].result(timeout=30) == "tail"
    finally:
        batcher.close()
    assert sched.spans == [["head", "tail"]] * 3


class CountingModel:
    """A model object with the front-end hook (here: the host arithmetic), counting its calls"""

    def __init__(self):
        self.calls = []

    def prepare_voices(self, voices):
        self.calls.append(len(voices))
        return infer.prepare_voices(voices, device=None)


def test_uploads_that_arrive_together_share_one_front_end_call():
    model, gate = CountingModel(), threading.Event()
    sched = StandInScheduler(model, gate)
    batcher = serve.ContinuousBatcher(sched)
    clips = [(0.2 * torch.randn(1 + i % 2, 3000 + 100 * i, generator=torch.Generator().manual_seed(i)), 44100) for i in range(4)]
    voices = [infer.PreparedVoice.deferred(c) for c in clips]
    try:
        first = batcher.submit(("eager voice", "ref", "gate"))               # parks the worker inside its admission ...
        futures = [batcher.submit((v, "ref", f"upload {i}")) for i, v in enumerate(voices)]   # ... while four uploads queue up
        gate.set()
        assert first.result(timeout=30) == "gate"
        assert [f.result(timeout=30) for f in futures] == [f"upload {i}" for i in range(4)]
    finally:
        gate.set()
        batcher.close()
    assert model.calls == [4]                                                # one call for all four, none at their own admissions
    for c, v in zip(clips, voices):
        want = infer.PreparedVoice(c)
        assert v.pending is None and torch.equal(v.audio, want.audio) and torch.equal(v.rms, want.rms)
    assert sched.spans[0] == ["gate"] + [f"upload {i}" for i in range(4)]    # admitted one by one, in order, at one boundary


def test_sharded_sampler_forwards_the_front_end():
    model = CountingModel()
    voices = [infer.PreparedVoice.deferred((0.2 * torch.randn(1, 2000), 48000)) for _ in range(2)]
    serve.ShardedSampler(model).prepare_voices(voices)
    assert model.calls == [2] and all(v.pending is None for v in voices)
    voice = infer.PreparedVoice.deferred((0.2 * torch.randn(2, 2000), 16000))
    serve.ShardedSampler(StandInModel()).prepare_voices([voice])             # a local model without the hook: the host front-end
    assert voice.pending is None and voice.audio.shape[-1] == 3000


def test_tap_table_caches_are_bounded():
    for sr in range(25000, 25000 + 1000 * (infer.TAP_TABLE_CACHE + 4), 1000):   # a client cycling through sample rates (small tables)
        infer.resample_taps(sr, 24000)
    assert len(infer._tap_tables) <= infer.TAP_TABLE_CACHE
    of, nf, width, taps = infer.resample_taps(44100, 24000)
    assert infer.resample_taps(44100, 24000)[3] is taps
