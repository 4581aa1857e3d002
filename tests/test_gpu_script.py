"""Multi-voice scripts served as ONE request on a tiny model: `TTSManager.synthesize_script` / `synthesize_script_stream` and the
`/v1/audio/speech/script` route, with the device back-end (the batch's one `ops.wave_finish_joins` call) on and off, direct and through the
continuous batcher.  The definition is the script's pieces served as plain requests on one continuing generator and joined on the host
(`np.concatenate`, zeros for the gap, then the whole-wave functions).  Every comparison is byte equality: there is no tolerance anywhere."""
import ctypes as C
import io
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, serve, synth  # noqa: E402

from test_gpu_request_knobs import ARCH, REF_TEXT, TEXT, VOCAB, _prompt  # noqa: E402

RATE = 24000
GAP = 1.5                                                 # seconds: long enough for `remove_silence` to cut into it
TOWN_TEXT = "Town speaks."
SCRIPT = f"{TEXT[:150]} [town] I live in town. [nobody] Always remember, I endure. [town] {TEXT[60:230]}"   # 4 pieces, 2 voices, 2 of several chunks
MODES = [None, dict(span_steps=3)]
IDS = ["direct", "span_steps"]
OPTIONS = [dict(), dict(sample_rate=8000, encoding="mulaw"), dict(sample_rate=8000, encoding="mulaw", remove_silence=True)]


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


def _town_clip():
    return synth.ref_audio(16000 * 2, seed=77, amp=0.05), 16000        # an upload at another rate, below target_rms


def _voices(path):
    return {"main": dict(ref_audio_path=path, ref_text=REF_TEXT), "town": dict(ref_audio=_town_clip(), ref_text=TOWN_TEXT, speed=1.1)}


@pytest.fixture(scope="module")
def reference(hip_objects, tmp_path_factory):
    """The definition, computed once and shared: the script's pieces as successive plain requests on one continuing generator (seed 7), each
    alone in its call, joined on the host as float32 with the gap's zeros between them."""
    path = _prompt(tmp_path_factory.mktemp("script"))
    voices = _voices(path)
    mgr = serve.TTSManager(nfe_step=8, device_backend=False).load(*hip_objects)
    try:
        g, parts = infer.request_generator(7), []
        for tag, piece in infer.split_voice_tags(SCRIPT, voices):
            v = voices[tag]
            voice, ref_text = mgr._voice(v["ref_audio_path"], v["ref_text"]) if "ref_audio_path" in v else mgr._clip_voice(v["ref_audio"], v["ref_text"])
            wave_, = mgr._run_batch([(voice, ref_text, piece, dict(generator=g, **({"speed": v["speed"]} if "speed" in v else {})))])
            assert wave_.dtype == np.float32
            if parts:
                parts.append(np.zeros(int(GAP * RATE), dtype=np.float32))
            parts.append(wave_)
    finally:
        mgr.close()
    assert len(parts) == 7
    return path, np.concatenate(parts)


def _want(whole, opts):
    pcm = infer.quantise_pcm16(whole)
    if opts.get("remove_silence"):
        cut = infer.remove_silence_pcm(pcm, RATE)
        assert len(cut) < len(pcm)
        pcm = cut
    return infer.deliver_pcm16(pcm, opts.get("sample_rate"), opts.get("encoding"))


@pytest.mark.parametrize("micro_batch", MODES, ids=IDS)
def test_script_equals_its_pieces_as_plain_requests(hip_objects, reference, micro_batch):
    path, whole = reference
    voices = _voices(path)
    for backend in (False, True):
        mgr = serve.TTSManager(nfe_step=8, micro_batch=micro_batch, device_backend=backend).load(*hip_objects)
        try:
            for opts in OPTIONS:
                cut, fmt = bool(opts.get("remove_silence")), infer.delivery_format(opts.get("sample_rate"), opts.get("encoding"))
                _reset()
                infer.backend_stats.clear()
                got = mgr.synthesize_script(SCRIPT, voices, gap=GAP, seed=7, **opts)
                want = _want(whole, opts)
                if not opts:
                    assert got.dtype == (np.int16 if backend else np.float32)
                    assert got.tobytes() == (want if backend else whole).tobytes(), backend
                assert serve.wav_bytes(got, *fmt).getvalue() == serve.wav_bytes(want, *fmt).getvalue(), (backend, opts)
                # one wave_finish launch per batch, three with silence removal; at most two copies per format group
                assert _counter("wave_finish_launches") == ((3 if cut else 1) if backend else 0), (backend, opts)
                assert _counter("wave_finish_requests") == (1 if backend else 0)
                if backend:
                    assert infer.backend_stats["device_requests"] == 1 and infer.backend_stats.get("host_requests", 0) == 0
                    assert infer.backend_stats["d2h_copies"] <= 2, dict(infer.backend_stats)
            # the stream's pieces concatenate to the same bytes, in the plain format and in the delivery format
            pieces = list(mgr.synthesize_script_stream(SCRIPT, voices, gap=GAP, seed=7))
            assert len(pieces) > 4 and infer.quantise_pcm16(np.concatenate(pieces)).tobytes() == infer.quantise_pcm16(whole).tobytes()
            pieces = list(mgr.synthesize_script_stream(SCRIPT, voices, gap=GAP, seed=7, **OPTIONS[1]))
            assert np.concatenate(pieces).tobytes() == _want(whole, OPTIONS[1]).tobytes()
            with pytest.raises(ValueError, match="remove_silence"):
                mgr.synthesize_script_stream(SCRIPT, voices, gap=GAP, seed=7, remove_silence=True)
        finally:
            mgr.close()


def test_a_script_and_two_plain_requests_in_one_batch_get_what_they_get_alone(hip_objects, reference):
    path, whole = reference
    mgr = serve.TTSManager(nfe_step=8, device_backend=True).load(*hip_objects)
    try:
        voices = _voices(path)
        voice, ref_text = mgr._voice(path, REF_TEXT)
        segments = mgr._script_segments(SCRIPT, voices, GAP)
        script = infer.ScriptRequest(segments, dict(seed=7), GAP)
        plain1, plain2 = (voice, ref_text, TEXT, dict(seed=3)), (voice, ref_text, "Always remember, I endure.", dict(seed=4, remove_silence=True))
        alone = [mgr._run_batch([r])[0] for r in (plain1, script, plain2)]
        _reset()
        infer.backend_stats.clear()
        together = mgr._run_batch([plain1, script, plain2])
        assert _counter("wave_finish_launches") == 3 and _counter("wave_finish_requests") == 3      # one call (plain2 is flagged)
        assert infer.backend_stats["device_calls"] == 1 and infer.backend_stats["d2h_copies"] <= 2
        for a, t in zip(alone, together):
            assert a.dtype == t.dtype == np.int16 and a.tobytes() == t.tobytes()
        assert together[1].tobytes() == infer.quantise_pcm16(whole).tobytes()
    finally:
        mgr.close()


def test_script_route_returns_the_script(hip_objects, reference):
    """Without the feature this route does not exist (404)."""
    import base64
    from fastapi.testclient import TestClient
    path, whole = reference
    reg = serve.VoiceRegistry()
    reg.add("prompt", path, REF_TEXT)
    mgr = serve.TTSManager(nfe_step=8, device_backend=True).load(*hip_objects)
    try:
        clip, sr = _town_clip()
        buf = io.BytesIO()
        with wave.open(buf, "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(sr)
            f.writeframes(infer.quantise_pcm16(clip[0].numpy()).tobytes())
        body = dict(text=SCRIPT, gap=GAP, seed=7, voices=dict(main=dict(ref_audio_name="prompt"),
                                                              town=dict(ref_audio=base64.b64encode(buf.getvalue()).decode(), ref_text=TOWN_TEXT, speed=1.1)))
        c = TestClient(serve.create_app(mgr, reg))
        r = c.post("/v1/audio/speech/script", json=body)
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav"
        with wave.open(io.BytesIO(r.content), "rb") as f:
            assert (f.getframerate(), f.getnchannels(), f.getsampwidth()) == (RATE, 1, 2)
            pcm = f.readframes(f.getnframes())
        # (the upload is 16-bit here and a float clip in `reference`: `_clip_voice` quantises both to the same int16 samples)
        assert pcm == infer.quantise_pcm16(whole).tobytes()
        r = c.post("/v1/audio/speech/script", json=dict(body, stream=True, response_format="pcm"))
        assert r.status_code == 200 and r.content == pcm
        assert c.post("/v1/audio/speech/script", json=dict(body, gap=6.0)).status_code == 400
    finally:
        mgr.close()
