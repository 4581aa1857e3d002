"""Speech editing on the host (CPU): the edit plan of F/infer/speech_edit.py:129-148 (worked example, rounding, truncation, the
`fix_duration` splice, rejections), `load_wav`'s RIFF reader over the formats recordings come in, and `/v1/audio/edit` +
`TTSManager.edit` over stand-in sampler / vocoder objects."""
import base64
import io
import itertools
import struct
import wave

import numpy as np
import pytest
import torch

from tts_indic_server_f5_amd import infer, serve


def _runs(mask):
    return [("T" if k else "F", len(list(g))) for k, g in itertools.groupby(mask.tolist())]


# ------------------------------------------------------------------------------------------------------------------------- plan
# the reference script's own case (speech_edit.py: parts_to_edit = [[1.42, 2.44], [4.04, 4.9]], fix_duration = [1.2, 1]) on 6.0 s
@pytest.mark.parametrize("fix,runs,frames,length", [
    (None, [("T", 133), ("F", 96), ("T", 150), ("F", 81), ("T", 103)], 563, 144_000),
    ([1.2, 1], [("T", 133), ("F", 112), ("T", 150), ("F", 94), ("T", 104)], 593, 151_680),
], ids=["no_fix", "fix_duration"])
def test_worked_example(fix, runs, frames, length):
    p = infer.plan_edit(144_000, [[1.42, 2.44], [4.04, 4.9]], fix)
    assert _runs(p.edit_mask) == runs
    assert p.edit_mask.shape == (frames,) and p.edit_mask.dtype == torch.bool
    assert p.length == length and p.duration == length // 256 == frames - 1
    audio = torch.arange(144_000, dtype=torch.float32)[None]
    cond = p.cond(audio)
    assert cond.shape == (1, length)
    if fix is None:
        assert torch.equal(cond, audio)   # the reference's cond: the recording itself
    else:                                 # the splice: kept slices, zeros of the requested length, the tail
        want = torch.cat([audio[:, :34080], torch.zeros(1, 28800), audio[:, 58560:96960], torch.zeros(1, 24000), audio[:, 117600:]], -1)
        assert torch.equal(cond, want)


def test_bankers_rounding():
    """1.2 s = 28800 samples = 112.5 frames -> 112 (Python's round, like the reference), not 113."""
    p = infer.plan_edit(48_000, [[0.5, 1.0]], [1.2])
    assert _runs(p.edit_mask)[:2] == [("T", round(12000 / 256)), ("F", 112)]
    assert round(112.5) == 112 and p.length == 12000 + 28800 + 24000


def test_mask_longer_than_recording_is_truncated():
    """Six touching 410-sample parts each round up to 2 frames: 12 mask entries for a 2600-sample recording, whose mask has
    2600 // 256 + 1 = 11 entries -- cut there like F.pad with a negative pad."""
    parts = [[k * 410 / 24000, (k + 1) * 410 / 24000] for k in range(6)]
    p = infer.plan_edit(2600, parts)
    assert p.edit_mask.shape == (11,) and not p.edit_mask.any()


def test_fix_duration_is_not_mutated():
    fix = [1.2, 1]
    infer.plan_edit(144_000, [[1.42, 2.44], [4.04, 4.9]], fix)
    assert fix == [1.2, 1]


@pytest.mark.parametrize("parts,fix,msg", [
    ([], None, "empty"),
    ([[1.0, 1.0]], None, "empty"),
    ([[2.0, 1.0]], None, "empty"),
    ([[2.0, 3.0], [0.5, 1.0]], None, "unsorted or overlaps"),
    ([[1.0, 2.0], [1.5, 3.0]], None, "unsorted or overlaps"),
    ([[5.0, 6.5]], None, "outside the recording"),
    ([[-0.1, 1.0]], None, "outside the recording"),
    ([[1.0, 2.0]], [1.0, 2.0], "2 entries for 1 parts"),
    ([[1.0, 2.0], [3.0, 4.0]], [1.0, 0.0], "positive"),
    ([[1.0, 2.0]], [-1.0], "positive"),
], ids=["no_parts", "zero_length", "reversed", "unsorted", "overlap", "past_end", "negative_start", "fix_len", "fix_zero", "fix_neg"])
def test_plan_rejections(parts, fix, msg):
    with pytest.raises(ValueError, match=msg):
        infer.plan_edit(144_000, parts, fix)


def test_plan_rejects_beyond_max_duration():
    infer.plan_edit(4094 * 256, [[1.0, 2.0]])   # duration 4094: the sampler's lens + 1 = 4096 frames still fit
    with pytest.raises(ValueError, match="max_duration"):
        infer.plan_edit(4095 * 256, [[1.0, 2.0]])
    with pytest.raises(ValueError, match="max_duration"):   # the splice can grow a recording past the limit
        infer.plan_edit(4000 * 256, [[1.0, 2.0]], [5.0])


@pytest.mark.parametrize("n", [4094 * 256, 4094 * 256 + 255, 4095 * 256, 4095 * 256 + 255, 4096 * 256])
def test_max_duration_bound_per_front_end(n):
    """The final frame count is the front-end's mel frames + 1 (cfm.py:136): L // 256 + 2 for vocos, L // 256 + 1 for bigvgan."""
    for mel_spec_type, mel_frames in (("vocos", n // 256 + 1), ("bigvgan", n // 256)):
        if mel_frames + 1 <= 4096:
            assert infer.plan_edit(n, [[1.0, 2.0]], mel_spec_type=mel_spec_type).duration == n // 256
        else:
            with pytest.raises(ValueError, match="max_duration"):
                infer.plan_edit(n, [[1.0, 2.0]], mel_spec_type=mel_spec_type)


@pytest.mark.parametrize("fix", [[1e6], [1e12], [1e300], [43.7]])
def test_oversized_fix_duration_is_rejected_before_any_allocation(fix):
    """A huge fix_duration is refused from the arithmetic alone: no mask or wave of the requested size is ever built."""
    import time
    import tracemalloc
    tracemalloc.start()
    t0 = time.perf_counter()
    with pytest.raises(ValueError, match="max_duration"):
        infer.plan_edit(144_000, [[1.0, 2.0]], fix)
    dt, peak = time.perf_counter() - t0, tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    assert dt < 0.5 and peak < 1 << 20


@pytest.mark.parametrize("parts,fix", [
    ([[1.0, float("inf")]], None),
    ([[float("nan"), 2.0]], None),
    ([[float("-inf"), 2.0]], None),
    ([[1.0, 2.0]], [float("inf")]),
    ([[1.0, 2.0]], [float("nan")]),
], ids=["end_inf", "start_nan", "start_neg_inf", "fix_inf", "fix_nan"])
def test_non_finite_inputs_are_value_errors(parts, fix):
    with pytest.raises(ValueError, match="finite"):
        infer.plan_edit(144_000, parts, fix)


# ---------------------------------------------------------------------------------------------------------- stand-in objects
class EditModel:
    """CFM.sample stand-in: records what the glue hands the sampler and returns `duration` zero frames."""
    def __init__(self):
        self.calls = []

    def sample(self, cond, text, duration, edit_mask, steps, cfg_strength, sway_sampling_coef, seed):
        self.calls.append(dict(cond=cond.clone(), text=text, duration=duration, edit_mask=edit_mask.clone(), steps=steps))
        return torch.zeros(1, duration, 100), None


class MelEditModel(EditModel):
    """Stand-in with `cond_mel` (like F5HipModel): the glue then hands over ONE padded mel batch with `lens`."""
    def cond_mel(self, audio):
        return torch.zeros(1, audio.shape[-1] // 256 + 1, 100)

    def sample(self, cond, text, duration, lens, edit_mask, steps, cfg_strength, sway_sampling_coef, seed):
        self.calls.append(dict(cond=cond.clone(), text=text, duration=duration.clone(), lens=lens.clone(), edit_mask=edit_mask.clone()))
        return torch.zeros(cond.shape[0], int(torch.maximum(lens + 1, duration).max()), 100), None


class FakeVocoder:
    def decode(self, mel):
        n = mel.shape[-1] * 256
        return 0.25 * torch.sin(torch.arange(n) * 0.05)[None]


def _recording(seconds=6.0, amp=0.3, seed=0):
    g = torch.Generator().manual_seed(seed)
    return amp * torch.sin(torch.arange(int(24000 * seconds)) * 0.03)[None] + 0.01 * torch.randn(1, int(24000 * seconds), generator=g)


def test_speech_edit_hands_the_plan_to_the_sampler():
    text = "Some call me optimist, and I am happy."
    for fix in (None, [1.2, 1]):
        model = EditModel()
        wave_out, sr, spec = infer.speech_edit((_recording(), 24000), text, [[1.42, 2.44], [4.04, 4.9]], model, FakeVocoder(),
                                               fix_duration=fix, nfe_step=4)
        plan = infer.plan_edit(144_000, [[1.42, 2.44], [4.04, 4.9]], fix)
        (call,) = model.calls
        assert call["cond"].shape == (1, plan.length) and call["duration"] == plan.duration and call["steps"] == 4
        assert torch.equal(call["edit_mask"], plan.edit_mask[None])
        assert call["text"] == infer.text_to_tokens([text])
        assert sr == 24000 and spec.shape == (100, plan.duration) and wave_out.dtype == np.float32
        assert wave_out.shape == (plan.duration * 256,)


def test_speech_edit_restores_rms_of_a_quiet_recording():
    quiet = _recording(amp=0.02)
    rms = float(torch.sqrt(torch.mean(quiet ** 2)))
    assert rms < 0.1
    model = EditModel()
    w, _, _ = infer.speech_edit((quiet, 24000), "quiet words", [[1.0, 2.0]], model, FakeVocoder())
    assert abs(float(model.calls[0]["cond"].pow(2).mean().sqrt()) - 0.1) < 1e-6   # gained to target_rms before sampling
    full = FakeVocoder().decode(torch.zeros(1, 100, len(w) // 256))[0].numpy()
    np.testing.assert_allclose(w, full * rms / 0.1, rtol=1e-6, atol=1e-7)


def test_speech_edit_batch_is_one_padded_sampler_call():
    edits = [((_recording(6.0), 24000), "first edited sentence", [[1.42, 2.44], [4.04, 4.9]], None),
             ((_recording(3.0, seed=1), 24000), "second one", [[0.5, 1.0]], [1.5]),
             ((_recording(4.5, seed=2), 24000), "third", [[2.0, 3.0]], None)]
    model = MelEditModel()
    res = infer.speech_edit_batch(edits, model, FakeVocoder(), nfe_step=4)
    (call,) = model.calls
    plans = [infer.plan_edit(a.shape[-1], parts, fix) for (a, _), _, parts, fix in edits]
    lens = [p.length // 256 + 1 for p in plans]
    assert call["lens"].tolist() == lens and call["duration"].tolist() == [p.duration for p in plans]
    assert call["cond"].shape == (3, max(lens), 100) and call["edit_mask"].shape == (3, max(lens))
    for i, p in enumerate(plans):
        assert torch.equal(call["edit_mask"][i, :lens[i]], p.edit_mask) and not call["edit_mask"][i, lens[i]:].any()
        assert res[i][2].shape == (100, lens[i] + 1)   # every frame of the edit's final duration lens + 1 is vocoded
    assert call["text"] == [infer.text_to_tokens([t])[0] for _, t, _, _ in edits]


def test_speech_edit_rejections():
    model = EditModel()
    rec = (_recording(), 24000)
    with pytest.raises(ValueError, match="target_text is empty"):
        infer.speech_edit(rec, "  ", [[1.0, 2.0]], model, FakeVocoder())
    short = (_recording(2560 / 24000), 24000)   # 11 mel frames
    with pytest.raises(ValueError, match="12 tokens, more than the 11 mel frames"):
        infer.speech_edit(short, "x" * 12, [[0.01, 0.05]], model, FakeVocoder())
    infer.speech_edit(short, "x" * 11, [[0.01, 0.05]], model, FakeVocoder())
    with pytest.raises(ValueError, match="outside the recording"):
        infer.speech_edit(rec, "words", [[5.5, 6.5]], model, FakeVocoder())
    assert len(model.calls) == 1


# ------------------------------------------------------------------------------------------------------------------- load_wav
_KS_TAIL = b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"


def _riff(tag, ch, sr, bits, payload, sub=None):
    block = ch * bits // 8
    if sub is None:
        fmt = struct.pack("<HHIIHH", tag, ch, sr, sr * block, block, bits)
    else:
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, ch, sr, sr * block, block, bits, 22, bits, 0) + struct.pack("<H", sub) + _KS_TAIL
    body = (b"fmt " + struct.pack("<I", len(fmt)) + fmt
            + b"LIST" + struct.pack("<I", 5) + b"INFOx\x00"        # an odd-sized chunk (word-aligned with a pad byte) before the data
            + b"data" + struct.pack("<I", len(payload)) + payload)
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WAVE" + body


def _ints(n, ch, lo, hi, seed=3):
    return np.random.default_rng(seed).integers(lo, hi, size=(n, ch), endpoint=True)


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("kind", ["pcm8", "pcm16", "pcm24", "pcm32", "float32", "float64", "ext_pcm24", "ext_float32"])
def test_load_wav_formats(kind, ch):
    n = 777
    if kind == "pcm8":
        x = _ints(n, ch, 0, 255).astype(np.uint8)
        payload, want, tag, bits = x.tobytes(), (x.astype(np.float64) - 128) / 128, 1, 8
    elif kind == "pcm16":
        x = _ints(n, ch, -32768, 32767).astype("<i2")
        payload, want, tag, bits = x.tobytes(), x / 2.0 ** 15, 1, 16
    elif kind in ("pcm24", "ext_pcm24"):
        x = _ints(n, ch, -(1 << 23), (1 << 23) - 1)
        payload = b"".join(int(v).to_bytes(3, "little", signed=True) for v in x.reshape(-1))
        want, tag, bits = x / 2.0 ** 23, 1, 24
    elif kind == "pcm32":
        x = _ints(n, ch, -(1 << 31), (1 << 31) - 1).astype("<i4")
        payload, want, tag, bits = x.tobytes(), x / 2.0 ** 31, 1, 32
    else:
        x = np.random.default_rng(5).uniform(-1.2, 1.2, size=(n, ch))
        dt = "<f4" if kind.endswith("32") else "<f8"
        payload, want, tag, bits = x.astype(dt).tobytes(), x.astype(dt), 3, 32 if dt == "<f4" else 64
    data = _riff(tag, ch, 22050, bits, payload, sub=tag if kind.startswith("ext_") else None)
    a, sr = infer.load_wav(data)
    assert sr == 22050 and a.dtype == torch.float32 and a.shape == (ch, n)
    np.testing.assert_array_equal(a.numpy(), want.T.astype(np.float32))


def test_load_wav_16bit_matches_previous_decoder(tmp_path):
    """16-bit PCM comes out bit-identical to the stdlib-wave decoder it replaces, from a path, bytes or a file object."""
    x = _ints(5000, 2, -32768, 32767, seed=11).astype("<i2")
    p = tmp_path / "s.wav"
    with wave.open(str(p), "wb") as f:
        f.setnchannels(2); f.setsampwidth(2); f.setframerate(16000); f.writeframes(x.tobytes())
    with wave.open(str(p), "rb") as f:
        raw = f.readframes(f.getnframes())
    old = np.frombuffer(raw, dtype="<i2").reshape(-1, 2).T.astype(np.float32) / 32768.0
    for src in (str(p), p, p.read_bytes(), io.BytesIO(p.read_bytes())):
        a, sr = infer.load_wav(src)
        assert sr == 16000 and a.numpy().view(np.uint32).tobytes() == np.ascontiguousarray(old).view(np.uint32).tobytes()


def test_load_wav_rejections():
    with pytest.raises(ValueError, match="FLAC"):
        infer.load_wav(b"fLaC\x00\x00\x00\x22" + bytes(64))
    with pytest.raises(ValueError, match="MS ADPCM"):
        infer.load_wav(_riff(2, 1, 24000, 4, bytes(64)))
    with pytest.raises(ValueError, match="MP3"):
        infer.load_wav(b"ID3\x04\x00" + bytes(64))
    with pytest.raises(ValueError, match="IEEE float at 16 bits"):
        infer.load_wav(_riff(3, 1, 24000, 16, bytes(64)))
    with pytest.raises(ValueError, match="sub-format format code 0x0002"):
        infer.load_wav(_riff(1, 1, 24000, 16, bytes(64), sub=2))
    good = _riff(1, 1, 24000, 16, bytes(200))
    with pytest.raises(ValueError, match="truncated WAV: 'data' chunk declares 200 bytes, 100 present"):
        infer.load_wav(good[:-100])
    with pytest.raises(ValueError, match="not a RIFF/WAVE"):
        infer.load_wav(b"OggS" + bytes(64))


# ---------------------------------------------------------------------------------------------------------- manager and route
def _wav_b64(x, sr=24000):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(sr)
        f.writeframes(np.clip(np.rint(x * 32768), -32768, 32767).astype("<i2").tobytes())
    return base64.b64encode(buf.getvalue()).decode()


def test_manager_edit():
    mgr = serve.TTSManager(nfe_step=4)
    with pytest.raises(ValueError, match="TTS model not loaded"):
        mgr.edit((_recording(), 24000), "words", [[1.0, 2.0]])
    model = EditModel()
    mgr.load(model, FakeVocoder())
    w = mgr.edit((_recording(), 24000), "new words", [[1.42, 2.44], [4.04, 4.9]], fix_duration=[1.2, 1])
    plan = infer.plan_edit(144_000, [[1.42, 2.44], [4.04, 4.9]], [1.2, 1])
    (call,) = model.calls
    assert call["cond"].shape == (1, plan.length) and call["duration"] == plan.duration and call["steps"] == 4
    assert torch.equal(call["edit_mask"][0], plan.edit_mask)
    assert w.dtype == np.float32 and w.shape == (plan.duration * 256,)

    class Sharded:            # a ShardedSampler-like wrapper: the edit runs on rank 0's own model
        def __init__(self, local):
            self.local = local
    inner = EditModel()
    mgr2 = serve.TTSManager(nfe_step=4).load(Sharded(inner), FakeVocoder())
    mgr2.edit((_recording(), 24000), "new words", [[1.0, 2.0]])
    assert len(inner.calls) == 1


def test_manager_edit_prepares_and_rejects_outside_the_device_lock():
    """Reading, planning and every rejection happen before the device lock is taken: with the lock held elsewhere (a synthesis batch
    running), a bad edit is refused at once instead of queueing behind it, and a good one waits only for the sampler."""
    import threading
    model = EditModel()
    mgr = serve.TTSManager(nfe_step=4).load(model, FakeVocoder())
    out = {}

    def run(key, parts, fix):
        try:
            out[key] = mgr.edit((_recording(), 24000), "new words", parts, fix)
        except ValueError as e:
            out[key] = e
    with mgr._device_lock:
        for key, parts, fix in (("huge", [[1.0, 2.0]], [1e12]), ("inf", [[1.0, float("inf")]], None)):
            t = threading.Thread(target=run, args=(key, parts, fix))
            t.start()
            t.join(timeout=10)
            assert not t.is_alive() and isinstance(out[key], ValueError)
        good = threading.Thread(target=run, args=("good", [[1.0, 2.0]], None))
        good.start()
        good.join(timeout=0.5)
        assert good.is_alive() and not model.calls   # prepared, now waiting for the device
    good.join(timeout=10)
    assert not good.is_alive() and isinstance(out["good"], np.ndarray) and len(model.calls) == 1


def test_prepared_edit_settings_must_match_the_call():
    prep = infer.prepare_edit((_recording(), 24000), "new words", [[1.0, 2.0]], mel_spec_type="bigvgan")
    assert prep.edit_mask.shape == (144_000 // 256,)   # cut to the bigvgan front-end's frames
    with pytest.raises(ValueError, match="PreparedEdit made for mel_spec_type='bigvgan'"):
        infer.speech_edit_batch([prep], EditModel(), FakeVocoder(), mel_spec_type="vocos")
    w, _, _ = infer.speech_edit_batch([infer.prepare_edit((_recording(), 24000), "new words", [[1.0, 2.0]])], EditModel(), FakeVocoder())[0]
    assert w.dtype == np.float32


def test_edit_route_contract():
    from fastapi.testclient import TestClient
    mgr = serve.TTSManager(nfe_step=4)
    c = TestClient(serve.create_app(mgr, serve.VoiceRegistry()))
    rec = _recording()[0].numpy()
    body = dict(audio=_wav_b64(rec), text="Some call me optimist.", parts_to_edit=[[1.42, 2.44], [4.04, 4.9]], fix_duration=None)
    r = c.post("/v1/audio/edit", json=body)
    assert r.status_code == 503 and r.json()["detail"] == "TTS model not loaded"
    model = EditModel()
    mgr.load(model, FakeVocoder())
    for bad, status, detail in [
        (dict(audio="not base64!"), 400, "Audio must be a base64-encoded WAV file."),
        (dict(audio=base64.b64encode(b"fLaC" + bytes(40)).decode()), 400, "Invalid audio: not a WAV file: FLAC stream ('fLaC' magic)"),
        (dict(text="  "), 400, "Text to synthesize cannot be empty."),
        (dict(parts_to_edit=[[2.0, 3.0], [1.0, 1.5]]), 400, None),
        (dict(parts_to_edit=[[1.0, 7.0]]), 400, None),
        (dict(fix_duration=[1.0]), 400, "fix_duration has 1 entries for 2 parts_to_edit"),
    ]:
        r = c.post("/v1/audio/edit", json={**body, **bad})
        assert r.status_code == status, (bad, r.text)
        if detail is not None:
            assert r.json()["detail"] == detail
    for raw in ('"parts_to_edit": [[1.0, Infinity]]', '"parts_to_edit": [[NaN, 2.0]]', '"fix_duration": [1e300, 1.0]',
                '"fix_duration": [Infinity, 1.0]'):
        js = '{"audio": "%s", "text": "Some call me optimist.", "parts_to_edit": [[1.42, 2.44], [4.04, 4.9]], %s}' % (body["audio"], raw)
        if raw.startswith('"parts_to_edit"'):
            js = js.replace('"parts_to_edit": [[1.42, 2.44], [4.04, 4.9]], ', "")
        r = c.post("/v1/audio/edit", content=js, headers={"content-type": "application/json"})
        assert r.status_code == 400, (raw, r.text)
    assert "unsorted or overlaps" in c.post("/v1/audio/edit", json={**body, "parts_to_edit": [[2.0, 3.0], [1.0, 1.5]]}).json()["detail"]
    assert not model.calls
    for fix in (None, [1.2, 1]):
        r = c.post("/v1/audio/edit", json={**body, "fix_duration": fix})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav"
        assert "edited_speech.wav" in r.headers["content-disposition"]
        plan = infer.plan_edit(144_000, body["parts_to_edit"], fix)
        call = model.calls[-1]
        assert call["cond"].shape == (1, plan.length) and call["duration"] == plan.duration
        assert torch.equal(call["edit_mask"][0], plan.edit_mask)
        with wave.open(io.BytesIO(r.content), "rb") as f:
            assert f.getframerate() == 24000 and f.getnchannels() == 1 and f.getsampwidth() == 2
            assert f.getnframes() == plan.duration * 256
