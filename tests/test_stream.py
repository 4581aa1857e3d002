"""CPU: streamed synthesis on deterministic stand-ins -- `infer.StreamJoiner` against `cross_fade_concat`, `infer.infer_process_stream`
against `infer_process`, the ragged vocoder hook of `infer_requests`, `serve.MicroBatcher` scheduling of a stream's first chunk and its
remaining chunks (never one batch; a cancelled queued item is skipped) and the `"stream": true` form of the speech routes."""
import io
import struct
import threading
import time
import wave

import numpy as np
import pytest
import torch

from tts_indic_server_f5_amd import infer, serve


class UnitModel:
    """Batch interface of F5HipModel: the mel of a unit is a closed form of its own prompt, tokens and frame count; records every
    `sample_units` call (units per call) in `calls`."""
    device = torch.device("cpu")

    def __init__(self, events=None):
        self.calls = []
        self.events = events if events is not None else []

    def cond_mel(self, audio):
        n = audio.shape[-1] // 256 + 1
        return audio[0, : (n - 1) * 256].reshape(n - 1, 256).mean(1, keepdim=True).repeat(1, 100)[None]

    def sample_units(self, audio, units, *, steps, cfg_strength, sway_sampling_coef, seed=None):
        audios = list(audio) if isinstance(audio, (list, tuple)) else [audio] * len(units)
        self.calls.append(len(units))
        self.events.append(("sample_units", len(units)))
        out = []
        for a, (tokens, frames) in zip(audios, units):
            mel = self.cond_mel(a) if a.ndim == 2 else a
            key = float(mel.abs().sum()) * 1e-3 + sum(map(ord, "".join(tokens))) * 1e-4 + steps
            out.append(torch.linspace(-1, 1, frames * 100).reshape(frames, 100) * key)
        return out


class Vocoder:
    def decode(self, mel):
        t = mel.shape[-1]
        return (torch.sin(torch.arange(256 * (t - 1), dtype=torch.float32) * 0.01) * mel.mean() * 3)[None]


class RaggedVocoder(Vocoder):
    """Also offers `decode_ragged` (what F5HipVocos does): one call for a list of mels."""

    def __init__(self):
        self.ragged_calls = []

    def decode_ragged(self, mels):
        self.ragged_calls.append([m.shape[-1] for m in mels])
        return [self.decode(m[None])[0] for m in mels]


def _clip(freq, seconds=2.0, amp=0.3):
    return (amp * torch.sin(2 * torch.pi * freq * torch.arange(int(24000 * seconds)) / 24000))[None], 24000


REF_TEXT = "Hi there."      # 2 s prompt: ~100-byte chunks
LONG = ("The quick brown fox jumps over the lazy dog. " * 7).strip()
QUIET = dict(show_info=lambda *_: None)


# ------------------------------------------------------------------------------------------------------------------ joiner
@pytest.mark.parametrize("fade_seconds", [0.15, 0.0, -1.0, 0.001, 1e-6])
def test_stream_joiner_equals_cross_fade_concat(fade_seconds):
    rng = np.random.default_rng(int(abs(fade_seconds) * 1e6) + 1)
    fade = int(fade_seconds * 24000) if fade_seconds > 0 else 0
    for trial in range(40):
        n = 1 if trial % 5 == 0 else int(rng.integers(2, 6))
        lengths = [int(rng.choice([0, 1, max(fade // 2, 1), fade, fade + 1, rng.integers(1, 3 * fade + 50)])) for _ in range(n)]
        waves = [rng.standard_normal(m).astype(np.float32) for m in lengths]
        ref = infer.cross_fade_concat(waves, fade_seconds)
        j = infer.StreamJoiner(fade_seconds)
        pieces = [j.push(w) for w in waves] + [j.flush()]
        got = np.concatenate(pieces)
        assert got.dtype == ref.dtype and np.array_equal(got, ref), (lengths, fade_seconds)
        # nothing that is emitted is ever rewritten: every piece but the flush is a prefix of the final wave
        assert sum(len(p) for p in pieces[:-1]) + len(pieces[-1]) == len(ref)
        assert len(pieces[-1]) <= max(fade, 0)


def test_stream_joiner_holds_back_exactly_the_fade():
    j = infer.StreamJoiner(0.15)
    first = j.push(np.ones(10000, dtype=np.float32))
    assert len(first) == 10000 - 3600 and first.dtype == np.float32
    second = j.push(np.ones(5000, dtype=np.float32))
    assert second.dtype == np.float64 and len(second) == 1400        # 3600 held + 5000 new - 3600 faded = 5000, of which 3600 are held again
    assert len(j.flush()) == 3600


# ------------------------------------------------------------------------------------------------------------------ inference layer
def test_infer_process_stream_equals_infer_process_and_yields_the_head_first():
    a = _clip(200.0)
    assert len(infer.request_chunks(REF_TEXT, 2.0, LONG)) >= 3
    w, sr, _ = infer.infer_process(a, REF_TEXT, LONG, UnitModel(), Vocoder(), nfe_step=4, **QUIET)
    events = []
    m = UnitModel(events)
    gen = infer.infer_process_stream(a, REF_TEXT, LONG, m, Vocoder(), nfe_step=4, **QUIET)
    first = next(gen)
    events.append(("piece", len(first)))
    assert m.calls == [1]                                 # the first chunk was sampled alone, and its samples came out ...
    rest = list(gen)
    assert m.calls == [1, len(infer.request_chunks(REF_TEXT, 2.0, LONG)) - 1]   # ... before the remaining chunks' ONE sample_units call
    assert [e[0] for e in events[:3]] == ["sample_units", "piece", "sample_units"]
    pieces = [first] + rest
    assert all(p.dtype == np.float32 for p in pieces) and len(first) > 0
    np.testing.assert_array_equal(np.concatenate(pieces), w.astype(np.float32))


def test_infer_process_stream_single_chunk_and_per_unit_model():
    a = _clip(250.0)
    w, _, _ = infer.infer_process(a, REF_TEXT, "Short.", UnitModel(), Vocoder(), nfe_step=4, **QUIET)
    pieces = list(infer.infer_process_stream(a, REF_TEXT, "Short.", UnitModel(), Vocoder(), nfe_step=4, **QUIET))
    np.testing.assert_array_equal(np.concatenate(pieces), w.astype(np.float32))


def test_infer_requests_uses_one_ragged_vocoder_call_and_keeps_results():
    a, b = _clip(200.0), _clip(330.0, 1.5, 0.02)          # the second voice is below the rms floor
    reqs = [(a, REF_TEXT, LONG), (b, "Others say mother.", "Always remember, I endure."), (a, REF_TEXT, ["Explicit chunk one.", "Two."])]
    v = RaggedVocoder()
    got = infer.infer_requests(reqs, UnitModel(), v, nfe_step=4)
    loop = infer.infer_requests(reqs, UnitModel(), Vocoder(), nfe_step=4)
    assert len(v.ragged_calls) == 1 and len(v.ragged_calls[0]) == len(infer.request_chunks(REF_TEXT, 2.0, LONG)) + 1 + 2
    for (w, sr, s), (w1, _, s1) in zip(got, loop):
        assert w.dtype == w1.dtype and sr == 24000
        np.testing.assert_array_equal(w, w1)
        np.testing.assert_array_equal(s, s1)
    # explicit chunk texts are used as given; join=False returns the per-chunk waves that the default joins
    per = infer.infer_requests(reqs, UnitModel(), v, nfe_step=4, join=False)
    assert len(per[2][0]) == 2 and len(per[2][2]) == 2
    for (waves, _, _), (w, _, _) in zip(per, got):
        np.testing.assert_array_equal(infer.cross_fade_concat(waves, infer.cross_fade_duration), w)


def test_bigvgan_keeps_the_per_chunk_loop():
    class BigV:
        def __init__(self):
            self.calls = 0

        def __call__(self, mel):
            self.calls += 1
            return torch.ones(1, 1, 256 * mel.shape[-1]) * mel.mean()

        def decode_ragged(self, mels):   # never used for mel_spec_type="bigvgan"
            raise AssertionError("ragged decode on the BigVGAN path")

    v = BigV()
    infer.infer_requests([(_clip(200.0), REF_TEXT, LONG)], UnitModel(), v, mel_spec_type="bigvgan", nfe_step=4)
    assert v.calls == len(infer.request_chunks(REF_TEXT, 2.0, LONG))


# ------------------------------------------------------------------------------------------------------------------ scheduling
def test_micro_batcher_on_start_hook_puts_the_follow_up_in_a_later_batch():
    batches = []

    def run(batch):
        batches.append(list(batch))
        time.sleep(0.02)
        return [r.upper() for r in batch]

    mb = serve.MicroBatcher(run, max_requests=8, max_wait_ms=100)
    box = {}
    head = mb.submit("head", on_start=lambda: box.setdefault("tail", mb.submit("tail")))
    assert head.result(timeout=10) == "HEAD" and box["tail"].result(timeout=10) == "TAIL"
    assert ["head"] in batches and ["tail"] in batches        # never the same batch, even with a long collection window
    mb.close()


def test_micro_batcher_skips_a_cancelled_queued_request_and_keeps_serving():
    gate, seen = threading.Event(), []

    def run(batch):
        seen.append(list(batch))
        gate.wait(timeout=10)
        return [r * 2 for r in batch]

    mb = serve.MicroBatcher(run, max_requests=1, max_wait_ms=1)
    first = mb.submit(1)
    time.sleep(0.05)                       # the first batch is running (blocked on the gate)
    queued = mb.submit(2)
    assert queued.cancel()                 # still queued: cancellable
    gate.set()
    assert first.result(timeout=10) == 2
    later = mb.submit(3)
    assert later.result(timeout=10) == 6   # the worker thread survived the cancelled item
    assert [1] in seen and [3] in seen and [2] not in seen
    assert mb._thread.is_alive()
    mb.close()
    # a cancelled item still queued at shutdown is not failed (no InvalidStateError), the others are
    mb2 = serve.MicroBatcher(lambda b: b, max_requests=2, max_wait_ms=1)
    mb2.close()
    c, f = serve.Future(), serve.Future()
    c.cancel()
    mb2._q.put(("cancelled", c))
    mb2._q.put(("stranded", f))
    mb2._fail_pending()
    assert c.cancelled()
    with pytest.raises(RuntimeError, match="closed"):
        f.result(timeout=1)


def _wav(tmp_path, name, freq):
    x = (6000 * np.sin(2 * np.pi * freq * np.arange(24000 * 2) / 24000)).astype(np.int16)
    p = tmp_path / name
    with wave.open(str(p), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(24000)
        f.writeframes(x.tobytes())
    return str(p)


@pytest.mark.parametrize("micro_batch", [None, dict(max_requests=8, max_wait_ms=50)])
def test_manager_stream_head_and_tail_never_share_a_batch(tmp_path, micro_batch):
    p = _wav(tmp_path, "a.wav", 200)
    model = UnitModel()
    mgr = serve.TTSManager(nfe_step=4, micro_batch=micro_batch).load(model, RaggedVocoder())
    whole = mgr.synthesize(LONG, ref_audio_path=p, ref_text=REF_TEXT)
    n = model.calls[-1]
    assert n >= 3
    stream = mgr.synthesize_stream(LONG, ref_audio_path=p, ref_text=REF_TEXT)
    first = next(stream)
    assert model.calls[-1] == 1                            # the head's samples are out; the tail runs in a batch of its own
    pieces = [first] + list(stream)
    assert model.calls[-2:] == [1, n - 1]
    if micro_batch:
        assert mgr.batcher.batch_sizes[-2:] == [1, 1]
    np.testing.assert_array_equal(np.concatenate(pieces), whole)
    mgr.close()
    with pytest.raises(ValueError):
        mgr.synthesize_stream("x", ref_audio_path=p, ref_text="y")


# ------------------------------------------------------------------------------------------------------------------ HTTP
@pytest.fixture(params=[None, dict(max_requests=8, max_wait_ms=5)], ids=["direct", "micro_batch"])
def client(tmp_path, request):
    from fastapi.testclient import TestClient
    reg = serve.VoiceRegistry()
    reg.add("KAN_F (Happy)", _wav(tmp_path, "a.wav", 200), REF_TEXT)
    reg.add("other", _wav(tmp_path, "b.wav", 320), "Other words.")
    mgr = serve.TTSManager(nfe_step=4, micro_batch=request.param)
    yield TestClient(serve.create_app(mgr, reg)), mgr, reg
    mgr.close()


def _frames(body):
    with wave.open(io.BytesIO(body), "rb") as f:
        return f.readframes(f.getnframes())


def test_stream_route_contract(client):
    c, mgr, reg = client
    r = c.post("/v1/audio/speech", json={"text": "hello", "stream": True})
    assert r.status_code == 503 and r.json()["detail"] == "TTS model not loaded"
    mgr.load(UnitModel(), RaggedVocoder())
    r = c.post("/v1/audio/speech", json={"text": "   ", "stream": True})
    assert r.status_code == 400 and r.json()["detail"] == "Text to synthesize cannot be empty."
    r = c.post("/v1/audio/speech/voice", json={"text": "hi", "ref_audio_name": "nobody", "stream": True})
    assert r.status_code == 400 and r.json()["detail"] == "Invalid reference audio name."
    for route, body in (("/v1/audio/speech", {"text": LONG}), ("/v1/audio/speech/voice", {"text": LONG, "ref_audio_name": "other"})):
        plain = c.post(route, json=body)
        default = c.post(route, json=dict(body, stream=False))
        streamed = c.post(route, json=dict(body, stream=True))
        assert plain.status_code == default.status_code == streamed.status_code == 200
        # stream=false: the body and headers of today's response
        v = reg.get(body.get("ref_audio_name", reg.default_voice))
        ref = serve.wav_bytes(mgr.synthesize(LONG, ref_audio_path=v.audio_path, ref_text=v.ref_text)).read()
        assert plain.content == default.content == ref
        assert plain.headers["content-type"] == "audio/wav" and streamed.headers["content-type"] == "audio/wav"
        assert streamed.headers["content-disposition"] == plain.headers["content-disposition"]
        # stream=true: a 44-byte RIFF header with unknown (0xFFFFFFFF) sizes, then the same PCM bytes
        h = streamed.content[:44]
        assert h[:4] == b"RIFF" and h[8:16] == b"WAVEfmt " and h[36:40] == b"data"
        assert struct.unpack("<I", h[4:8])[0] == 0xFFFFFFFF and struct.unpack("<I", h[40:44])[0] == 0xFFFFFFFF
        assert struct.unpack("<IHHIIHH", h[16:36]) == (16, 1, 1, 24000, 48000, 2, 16)
        assert streamed.content[44:] == _frames(plain.content)


def test_stream_header_and_pcm_rule():
    x = np.array([0.0, 0.5, -1.0, 1.0, 1.5, -2.0, 1 / 65536], dtype=np.float32)
    assert serve.pcm16(x) == _frames(serve.wav_bytes(x).read())
    assert len(serve.wav_stream_header()) == 44
