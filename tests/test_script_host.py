"""CPU: multi-voice scripts as ONE request (F/infer/infer_cli.py:166-208) on deterministic stand-in models -- `infer.join_segments`, the
cut-aware `infer.StreamJoiner`, `infer.ScriptRequest` through `infer.infer_requests`, `serve.TTSManager.synthesize_script` /
`synthesize_script_stream` and the `/v1/audio/speech/script` route.  Every comparison is `np.array_equal` or byte equality."""
import base64
import io
import itertools
import os
import sys
import wave

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tts_indic_server_f5_amd import infer, serve  # noqa: E402


class NoiseModel:
    """Stand-in with F5HipModel's batch interface: a unit's mel is its own noise (from its generator, else the global one, drawn unit by unit
    in order) plus a closed form of ITS OWN prompt and tokens, so a leak between units, a re-ordering or another draw order changes it."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls, self.mel_calls = [], 0

    def cond_mel(self, audio):
        self.mel_calls += 1
        n = audio.shape[-1] // 256
        return audio[0, : n * 256].reshape(n, 256).abs().mean(1, keepdim=True).repeat(1, 100)[None]

    def sample_units(self, cond, units, *, steps, cfg_strength, sway_sampling_coef, generators=None, ode_method=None):
        conds = list(cond) if isinstance(cond, (list, tuple)) else [cond] * len(units)
        gens = generators if generators is not None else [None] * len(units)
        self.calls.append(len(units))
        out = []
        for c, (tokens, frames), g in zip(conds, units, gens):
            key = float(c.sum()) * 1e-4 + sum(map(ord, "".join(tokens))) * 1e-5
            out.append(torch.randn(frames, 100, generator=g) * 0.05 + key)
        return out


class Vocoder:
    """`decode` [1, mel, T] -> [1, 256 T]; `decode_ragged` every item in one (counted) call, each item its own `decode`."""

    def __init__(self):
        self.ragged_calls = self.decode_calls = 0

    def _wave(self, mel):
        t = mel.shape[-1]
        return torch.repeat_interleave(mel.mean(0), 256) * 0.5 + 0.1 * torch.sin(torch.arange(256 * t, dtype=torch.float32) * 0.01)

    def decode(self, mel):
        self.decode_calls += 1
        return self._wave(mel[0])[None]

    def decode_ragged(self, mels):
        self.ragged_calls += 1
        return [self._wave(m) for m in mels]


def _clip(freq, seconds=3.0, amp=0.3):
    return (amp * torch.sin(2 * torch.pi * freq * torch.arange(int(24000 * seconds)) / 24000))[None], 24000


LONG = ("The quick brown fox jumps over the lazy dog. " * 6).strip()
A, B = _clip(200.0), _clip(330.0, 4.0, 0.05)     # B is below target_rms: gained up, and restored on its own chunks only
RA, RB = "first voice words", "second voice says"
SEGMENTS = [(A, RA, LONG), (B, RB, "Short one."), (A, RA, "Again the first voice. " + LONG), (B, RB, LONG)]


def _rand(n, seed):
    return np.random.default_rng(seed).uniform(-0.3, 0.3, n).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------ the join
def test_join_segments_is_concatenate_of_cross_fade_concat():
    fade_s = 0.15
    segs = [[_rand(8000, 0), _rand(7300, 1), _rand(9001, 2)], [_rand(5, 3)], [_rand(7200, 4), _rand(3000, 5)]]   # (3000 < fade: host only)
    got = infer.join_segments(segs, fade_s)
    ref = np.concatenate([infer.cross_fade_concat(s, fade_s) for s in segs])
    assert got.dtype == np.float32 and ref.dtype == np.float64 and np.array_equal(got, ref.astype(np.float32))
    # gap: float32 zeros between consecutive segments, none in front or behind
    gap = 1234
    z = np.zeros(gap, dtype=np.float32)
    ref = np.concatenate([infer.cross_fade_concat(segs[0], fade_s), z, infer.cross_fade_concat(segs[1], fade_s), z,
                          infer.cross_fade_concat(segs[2], fade_s)]).astype(np.float32)
    assert np.array_equal(infer.join_segments(segs, fade_s, gap), ref)
    # single-chunk segments, gap 0: the reference's np.concatenate exactly
    singles = [[_rand(100, 6)], [_rand(1, 7)], [_rand(50, 8)]]
    assert np.array_equal(infer.join_segments(singles, fade_s), np.concatenate([s[0] for s in singles]))
    # no fade at all
    assert np.array_equal(infer.join_segments(segs, 0.0, 3), np.concatenate([*segs[0], z[:3], *segs[1], z[:3], *segs[2]]))
    # one segment: the plain request's wave
    assert np.array_equal(infer.join_segments(segs[:1], fade_s), infer.request_wave("x", segs[0], fade_s))


@pytest.mark.parametrize("gap", [0, 3])
def test_stream_joiner_with_cut_equals_join_segments_for_every_boundary_set(gap):
    fade_s = 4.5 / 24000                                  # 4 samples
    assert int(fade_s * 24000) == 4
    chunks = [_rand(n, 10 + i) for i, n in enumerate([9, 8, 3, 10, 1, 12])]   # 3 and 1 are shorter than the fade: n = min(...) on the host
    for cuts in itertools.product([False, True], repeat=len(chunks) - 1):      # a segment boundary in front of chunk i + 1, or a fade
        segs = [[chunks[0]]]
        for c, cut in zip(chunks[1:], cuts):
            if cut:
                segs.append([c])
            else:
                segs[-1].append(c)
        joiner, pieces = infer.StreamJoiner(fade_s), []
        for k, seg in enumerate(segs):
            if k:
                pieces += list(joiner.pieces(cut=True))
                if gap:
                    pieces += list(joiner.pieces([np.zeros(gap, dtype=np.float32)], cut=True))
            pieces += list(joiner.pieces(seg))
        pieces += list(joiner.pieces(flush=True))
        assert all(p.dtype == np.float32 and len(p) for p in pieces)
        assert np.array_equal(np.concatenate(pieces), infer.join_segments(segs, fade_s, gap)), cuts
    j = infer.StreamJoiner(fade_s)
    assert len(j.cut()) == 0 and len(j.push(chunks[0])) == 5 and len(j.cut()) == 4 and len(j.cut()) == 0 and j.held is None


# ------------------------------------------------------------------------------------------------------------------------ one request
def _successive(segments, seed, opts=None, **kw):
    """The segments as successive plain requests that carry one continuing generator: [(wave, sr, spec)]."""
    g = infer.request_generator(seed)
    out = []
    for seg in segments:
        o = dict(opts or {}, **({} if g is None else dict(generator=g)), **(dict(speed=seg[3]) if len(seg) > 3 else {}))
        out.append(infer.infer_requests([(seg[0], seg[1], seg[2], o)], NoiseModel(), Vocoder(), nfe_step=4, **kw)[0])
    return out


def test_seeded_script_equals_successive_plain_requests_on_one_generator():
    segs = SEGMENTS[:3] + [(B, RB, LONG, 1.3)]            # a per-segment speed
    m, v = NoiseModel(), Vocoder()
    (w, sr, specs), = infer.infer_requests([infer.ScriptRequest(segs, dict(seed=7))], m, v, nfe_step=4)
    ref = _successive(segs, 7)
    assert sr == 24000 and w.dtype == np.float32 and len(m.calls) == 1 and v.ragged_calls == 1 and v.decode_calls == 0
    assert np.array_equal(w, np.concatenate([r[0] for r in ref]).astype(np.float32))
    assert len(specs) == len(segs) and all(np.array_equal(s, r[2]) for s, r in zip(specs, ref))
    assert m.calls[0] > len(segs)                                             # several chunks per long segment
    # the same script again: the same samples (its own generator), and unseeded it differs
    (w2, _, _), = infer.infer_requests([infer.ScriptRequest(segs, dict(seed=7))], NoiseModel(), Vocoder(), nfe_step=4)
    assert np.array_equal(w, w2)
    # unseeded: the global generator in the same flat order
    torch.manual_seed(3)
    (wu, _, _), = infer.infer_requests([infer.ScriptRequest(segs)], NoiseModel(), Vocoder(), nfe_step=4)
    torch.manual_seed(3)
    refu = [infer.infer_requests([(s[0], s[1], s[2], dict(speed=s[3]) if len(s) > 3 else {})], NoiseModel(), Vocoder(), nfe_step=4)[0][0] for s in segs]
    assert np.array_equal(wu, np.concatenate(refu).astype(np.float32)) and not np.array_equal(wu, w)
    # gap, and join=False: the per-segment chunk waves
    (wg, _, _), = infer.infer_requests([infer.ScriptRequest(segs, dict(seed=7), gap=0.01)], NoiseModel(), Vocoder(), nfe_step=4)
    z = np.zeros(240, dtype=np.float32)
    assert np.array_equal(wg, np.concatenate(sum([[z, r[0].astype(np.float32)] for r in ref], [])[1:]))
    (per_seg, _, _), = infer.infer_requests([infer.ScriptRequest(segs, dict(seed=7))], NoiseModel(), Vocoder(), nfe_step=4, join=False)
    assert len(per_seg) == len(segs) and np.array_equal(infer.join_segments(per_seg), w)


def test_script_mixed_with_plain_requests_is_one_sampler_and_one_vocoder_call():
    plain1, plain2 = (A, RA, "A plain request.", dict(seed=1)), (B, RB, LONG, dict(seed=2))
    script = infer.ScriptRequest(SEGMENTS, dict(seed=3))
    m, v = NoiseModel(), Vocoder()
    got = infer.infer_requests([plain1, script, plain2], m, v, nfe_step=4)
    assert len(m.calls) == 1 and v.ragged_calls == 1 and v.decode_calls == 0
    for req, (w, _, _) in zip([plain1, script, plain2], got):                 # each gets what it gets alone
        (w1, _, _), = infer.infer_requests([req], NoiseModel(), Vocoder(), nfe_step=4)
        assert np.array_equal(w, w1) and w.dtype == w1.dtype
    # the serving form (`finish`): float32 waves, or int16 PCM; the script as one item
    want = [np.asarray(w, dtype=np.float32) for w, _, _ in got]
    res = infer.infer_requests([plain1, script, plain2], NoiseModel(), Vocoder(), nfe_step=4, finish=dict(device_backend=False, want="float"))
    assert all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(res, want))
    res = infer.infer_requests([plain1, script, plain2], NoiseModel(), Vocoder(), nfe_step=4, finish=dict(device_backend=False, want="pcm16"))
    assert all(np.array_equal(a, infer.quantise_pcm16(b)) and a.dtype == np.int16 for a, b in zip(res, want))


def test_whole_wave_options_apply_to_the_joined_script():
    def run(**opts):
        (w, sr, _), = infer.infer_requests([infer.ScriptRequest(SEGMENTS, dict(seed=5, **opts), gap=1.5)], NoiseModel(), Vocoder(), nfe_step=4)
        return w, sr
    plain, _ = run()
    pcm = infer.quantise_pcm16(plain)
    cut = infer.remove_silence_pcm(pcm, 24000)
    assert len(cut) < len(pcm)                                               # the 1.5 s gaps shrink to 2 x 500 ms
    w, sr = run(remove_silence=True)
    assert sr == 24000 and w.dtype == np.int16 and np.array_equal(w, cut)
    w, sr = run(sample_rate=8000, encoding="mulaw")
    assert sr == 8000 and w.dtype == np.uint8 and np.array_equal(w, infer.deliver_pcm16(pcm, 8000, "mulaw"))
    w, sr = run(remove_silence=True, sample_rate=16000)
    assert sr == 16000 and np.array_equal(w, infer.deliver_pcm16(cut, 16000, "pcm16"))
    # a chunked script (a stream's tail) hands out chunk waves: nothing that needs the whole wave
    with pytest.raises(ValueError):
        infer.infer_requests([infer.ScriptRequest([(A, RA, ["One.", "Two."])], dict(remove_silence=True))], NoiseModel(), Vocoder(), nfe_step=4)
    res, = infer.infer_requests([infer.ScriptRequest([(A, RA, ["One.", "Two."]), (B, RB, ["Three."])], dict(seed=1))], NoiseModel(), Vocoder(),
                                nfe_step=4, finish=dict(device_backend=False, want="float"))
    assert [len(seg) for seg in res] == [2, 1] and all(isinstance(w, np.ndarray) for seg in res for w in seg)


def test_infer_multi_voice_is_unchanged():
    voices = {"main": dict(ref_audio=A, ref_text=RA), "town": dict(ref_audio=B, ref_text=RB)}
    text = "A long time ago. [town] I live in town. " + LONG + " [nobody] Who is this? [main]Back to me. [town]"
    torch.manual_seed(11)
    w, sr, specs = infer.infer_multi_voice(text, voices, NoiseModel(), Vocoder(), nfe_step=4)
    torch.manual_seed(11)
    parts = [infer.infer_requests([(voices[t]["ref_audio"], voices[t]["ref_text"], p)], NoiseModel(), Vocoder(), nfe_step=4)[0]
             for t, p in infer.split_voice_tags(text, voices)]
    ref = np.concatenate([p[0] for p in parts])
    assert sr == 24000 and w.dtype == ref.dtype == np.float64 and np.array_equal(w, ref) and len(specs) == 4   # its signature and its bits
    # the script request of the same pieces is that wave as float32
    torch.manual_seed(11)
    (ws, _, _), = infer.infer_requests([infer.ScriptRequest([(voices[t]["ref_audio"], voices[t]["ref_text"], p)
                                                            for t, p in infer.split_voice_tags(text, voices)])], NoiseModel(), Vocoder(), nfe_step=4)
    assert np.array_equal(ws, w.astype(np.float32))


def test_script_request_refusals():
    ok = (A, RA, "Hello.")
    for bad in ([], [ok] * 65, [(A, RA)], [(A, RA, "  ")], [(A, RA, [])], [(A, RA, ["x", " "])], [(A, "", "Hello.")], [ok, (A, RA, ["Hello."])],
                [(A, RA, "Hello.", 0.0)], [(A, RA, "Hello.", float("nan"))]):
        with pytest.raises(ValueError):
            infer.ScriptRequest(bad)
    for gap in (-0.001, 5.001, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError):
            infer.ScriptRequest([ok], gap=gap)
    assert infer.ScriptRequest([ok] * 64, gap=5).gap_samples == 120000 and infer.ScriptRequest([ok], gap=0.0001).gap_samples == 2
    m = NoiseModel()
    with pytest.raises(ValueError):
        infer.infer_requests([infer.ScriptRequest([ok], dict(gap=1.0))], m, Vocoder())      # gap is a script field, not a request option
    with pytest.raises(ValueError):
        infer.infer_requests([infer.ScriptRequest([ok], dict(volume=2))], m, Vocoder())
    assert m.calls == []


# ------------------------------------------------------------------------------------------------------------------------ serving
def _wav(clip):
    x, sr = clip
    buf = io.BytesIO()
    with wave.open(buf, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(sr)
        f.writeframes(infer.quantise_pcm16(x[0].numpy()).tobytes())
    return buf.getvalue()


VOICES = {"main": dict(ref_audio=A, ref_text=RA), "town": dict(ref_audio=_wav(B), ref_text=RB, clip_short=True, speed=1.2)}
SCRIPT = "A long time ago. " + LONG + " [town] I live in town. " + LONG + " [nobody] Who is this? [main]Back to me. [town]"


@pytest.mark.parametrize("micro_batch", [None, dict(max_requests=4, max_wait_ms=1)])
def test_manager_script_and_stream(micro_batch):
    mgr = serve.TTSManager(nfe_step=4, micro_batch=micro_batch).load(NoiseModel(), Vocoder())
    try:
        w = mgr.synthesize_script(SCRIPT, VOICES, seed=9)
        assert w.dtype == np.float32 and len(mgr.model_obj.calls) == 1
        # what the client had to do before: one clip request per piece on one continuing generator, concatenated
        g, parts = infer.request_generator(9), []
        for tag, piece in infer.split_voice_tags(SCRIPT, VOICES):
            v = VOICES[tag]
            voice, ref_text = mgr._clip_voice(v["ref_audio"], v["ref_text"], v.get("clip_short", True))
            o = dict(generator=g, **(dict(speed=v["speed"]) if "speed" in v else {}))
            parts.append(infer.infer_requests([(voice, ref_text, piece, o)], NoiseModel(), Vocoder(), nfe_step=4)[0][0])
        assert np.array_equal(w, np.concatenate(parts).astype(np.float32))
        assert len(mgr._clip_cache) == 2                                       # the two uploads, each prepared once
        for gap in (0.0, 0.02):
            whole = mgr.synthesize_script(SCRIPT, VOICES, gap=gap, seed=9)
            pieces = list(mgr.synthesize_script_stream(SCRIPT, VOICES, gap=gap, seed=9))
            assert len(pieces) > 4 and np.array_equal(np.concatenate(pieces), whole)
            assert (gap == 0.0) == np.array_equal(whole, w)
        # the delivery format: whole, and piece by piece on the stream
        enc = mgr.synthesize_script(SCRIPT, VOICES, gap=0.02, seed=9, sample_rate=8000, encoding="alaw")
        assert enc.dtype == np.uint8 and np.array_equal(enc, infer.deliver_pcm16(infer.quantise_pcm16(whole), 8000, "alaw"))
        assert np.array_equal(np.concatenate(list(mgr.synthesize_script_stream(SCRIPT, VOICES, gap=0.02, seed=9, sample_rate=8000, encoding="alaw"))), enc)
        cut = mgr.synthesize_script(SCRIPT, VOICES, gap=2.0, seed=9, remove_silence=True)
        assert np.array_equal(cut, infer.remove_silence_pcm(infer.quantise_pcm16(mgr.synthesize_script(SCRIPT, VOICES, gap=2.0, seed=9)), 24000))
        # a one-piece, one-chunk script streams too (no tail)
        one = list(mgr.synthesize_script_stream("Hi there.", VOICES, seed=2))
        assert np.array_equal(np.concatenate(one), mgr.synthesize_script("Hi there.", VOICES, seed=2))
    finally:
        mgr.close()


def test_manager_refusals_queue_nothing():
    mgr = serve.TTSManager(nfe_step=4, micro_batch=dict(max_requests=4, max_wait_ms=1))
    with pytest.raises(ValueError, match="not loaded"):
        mgr.synthesize_script(SCRIPT, VOICES)
    mgr.load(NoiseModel(), Vocoder())
    try:
        many = " ".join(f"[town] piece {i}." for i in range(65))
        cases = [
            (dict(text=SCRIPT, voices={"town": VOICES["town"]}), "main"),
            (dict(text="  ", voices=VOICES), "empty"),
            (dict(text="[town] [main]", voices=VOICES), "empty"),
            (dict(text=many, voices=VOICES), "64"),
            (dict(text=SCRIPT, voices=VOICES, gap=5.5), "gap"),
            (dict(text=SCRIPT, voices=VOICES, gap=-1), "gap"),
            (dict(text=SCRIPT, voices=VOICES, volume=3), "volume"),
            (dict(text=SCRIPT, voices=VOICES, nfe_step=0), "nfe_step"),
            (dict(text=SCRIPT, voices=dict(VOICES, town=dict(VOICES["town"], speed=-1.0))), "speed"),
            (dict(text=SCRIPT, voices=dict(VOICES, town=dict(ref_text=RB))), "town"),
            (dict(text=SCRIPT, voices=dict(VOICES, town=dict(VOICES["town"], ref_text=" "))), "Reference text"),
            (dict(text=SCRIPT, voices=dict(VOICES, town=dict(VOICES["town"], ref_audio=b"not a wav"))), "Invalid audio"),
        ]
        for kw, word in cases:
            with pytest.raises(ValueError, match=word):
                mgr.synthesize_script(**kw)
            with pytest.raises(ValueError, match=word):
                mgr.synthesize_script_stream(**kw)
        with pytest.raises(ValueError, match="remove_silence"):
            mgr.synthesize_script_stream(SCRIPT, VOICES, remove_silence=True)
        assert mgr.model_obj.calls == [] and mgr.batcher.batch_sizes == []   # nothing was queued
        assert len(mgr.synthesize_script("[town] " + " ".join(f"[town] piece {i}." for i in range(63)), VOICES, seed=1)) > 0   # 64 pieces pass
    finally:
        mgr.close()


@pytest.fixture()
def client(tmp_path):
    from fastapi.testclient import TestClient
    p = tmp_path / "prompt.wav"
    p.write_bytes(_wav(A))
    reg = serve.VoiceRegistry()
    reg.add("KAN_F (Happy)", str(p), RA)
    mgr = serve.TTSManager(nfe_step=4)
    return TestClient(serve.create_app(mgr, reg)), mgr, str(p)


def test_script_route(client):
    c, mgr, path = client
    town = dict(ref_audio=base64.b64encode(_wav(B)).decode(), ref_text=RB)
    body = dict(text=SCRIPT, voices=dict(main=dict(ref_audio_name="KAN_F (Happy)"), town=town), seed=4)
    url = "/v1/audio/speech/script"
    r = c.post(url, json=body)
    assert r.status_code == 503 and r.json()["detail"] == "TTS model not loaded"
    mgr.load(NoiseModel(), Vocoder())
    r = c.post(url, json=body)
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and "synthesized_script.wav" in r.headers["content-disposition"]
    with wave.open(io.BytesIO(r.content), "rb") as f:
        assert (f.getframerate(), f.getnchannels(), f.getsampwidth()) == (24000, 1, 2)
        pcm = f.readframes(f.getnframes())
    assert len(mgr.model_obj.calls) == 1
    voices = dict(main=dict(ref_audio_path=path, ref_text=RA), town=dict(ref_audio=_wav(B), ref_text=RB))
    assert pcm == infer.quantise_pcm16(mgr.synthesize_script(SCRIPT, voices, seed=4)).tobytes()
    # response_format, the delivery format, the stream: the same samples
    r = c.post(url, json=dict(body, response_format="pcm"))
    assert r.status_code == 200 and r.headers["content-type"] == "audio/pcm" and r.content == pcm
    r = c.post(url, json=dict(body, stream=True, response_format="pcm"))
    assert r.status_code == 200 and r.content == pcm
    r = c.post(url, json=dict(body, stream=True))
    assert r.status_code == 200 and r.content[44:] == pcm
    r = c.post(url, json=dict(body, gap=0.5, sample_rate=8000, encoding="mulaw", response_format="pcm"))
    whole = infer.quantise_pcm16(mgr.synthesize_script(SCRIPT, voices, gap=0.5, seed=4))
    assert r.status_code == 200 and r.content == infer.deliver_pcm16(whole, 8000, "mulaw").tobytes()
    r = c.post(url, json=dict(body, gap=2.0, remove_silence=True, response_format="pcm"))
    assert r.status_code == 200 and r.content == infer.remove_silence_pcm(infer.quantise_pcm16(mgr.synthesize_script(SCRIPT, voices, gap=2.0, seed=4)),
                                                                         24000).tobytes()
    calls = len(mgr.model_obj.calls)
    many = " ".join(f"[town] piece {i}." for i in range(65))
    table = [
        (dict(body, voices=dict(body["voices"], main=dict(ref_audio_name="nobody"))), "Invalid reference audio name."),
        (dict(body, voices=dict(town=town)), 'voices needs a "main" entry'),
        (dict(body, text="   "), "Text to synthesize cannot be empty."),
        (dict(body, text="[town] [main]"), "Text to synthesize cannot be empty."),
        (dict(body, text=many), "a script needs between 1 and 64 pieces (got 65)"),
        (dict(body, gap=5.5), "gap must be"),
        (dict(body, gap=-0.1), "gap must be"),
        (dict(body, voices=dict(body["voices"], town=dict(town, ref_audio="@@@"))), "Audio must be a base64-encoded WAV file."),
        (dict(body, voices=dict(body["voices"], town=dict(town, ref_audio=base64.b64encode(b"junk").decode()))), "Invalid audio"),
        (dict(body, voices=dict(body["voices"], town=dict(town, ref_text=""))), "Reference text cannot be empty."),
        (dict(body, voices=dict(body["voices"], town=dict(ref_text=RB))), "needs either ref_audio_name or ref_audio"),
        (dict(body, voices=dict(body["voices"], town=dict(town, speed=0))), "speed"),
        (dict(body, nfe_step=0), "nfe_step"),
        (dict(body, encoding="mp3"), "encoding"),
        (dict(body, response_format="ogg"), "response_format"),
        (dict(body, stream=True, remove_silence=True), serve.STREAM_REMOVE_SILENCE),
    ]
    for bad, detail in table:
        r = c.post(url, json=bad)
        assert r.status_code == 400 and detail in r.json()["detail"], (detail, r.status_code, r.text)
    assert len(mgr.model_obj.calls) == calls                                  # none of them reached the sampler


def test_script_route_model_has_every_request_option():
    fields = serve.request_models().ScriptRequest.model_fields
    assert set(infer.REQUEST_OPTIONS) <= set(fields)
    assert {"text", "voices", "gap", "stream", "response_format"} <= set(fields)
    assert set(serve.request_models().ScriptVoice.model_fields) == {"ref_audio_name", "ref_audio", "ref_text", "clip_short", "speed"}
