"""GPU: speech editing (`infer.speech_edit`, F/infer/speech_edit.py:119-192) on the HIP objects -- the masked sampler
(`F5HipModel.sample(edit_mask=...)`), the mel front-ends and the vocoders -- against the same host glue driving the CPU oracle
(oracle mel -> `cfm_sample(edit_mask=...)` with the same noise -> oracle vocoder -> rms restore).  Bounds are the ones
tests/test_gpu_e2e.py applies to `infer_process`: mel RMS < 1e-3, wave max < 1e-4."""
import base64
import io
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import bigvgan_oracle as B  # noqa: E402
from oracle import dit_oracle as O  # noqa: E402
from oracle import vocos_oracle as V  # noqa: E402
from tts_indic_server_f5_amd import infer, synth  # noqa: E402
from tts_indic_server_f5_amd.tokenizer import list_str_to_idx  # noqa: E402

VOCAB = {chr(32 + i): i for i in range(96)}   # printable ASCII, " " -> 0
ARCH = dict(dim=256, depth=4, heads=4, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=96)
UARCH = dict(dim=128, depth=4, heads=2, ff_mult=4, text_num_embeds=96)
KW = dict(nfe_step=8, cfg_strength=2.0, sway_sampling_coef=-1.0)
TEXT = "Some call me nature, others call me mother nature."
PARTS = [[0.6, 1.1], [1.9, 2.4]]
FIX = [0.8, 0.3]


class OracleEditModel:
    """CFM.sample with `edit_mask` on the CPU oracle: raw-wave cond -> the oracle mel of `mel_spec_type`; list[str] text -> vocab."""

    def __init__(self, sd, cfg, forward_fn=None, mel_spec_type="vocos"):
        self.sd, self.cfg, self.fwd = sd, cfg, forward_fn
        self.front = V.vocos_mel_spectrogram if mel_spec_type == "vocos" else B.bigvgan_mel_spectrogram

    def sample(self, cond, text, duration, edit_mask, steps, cfg_strength, sway_sampling_coef, seed):
        mel = self.front(cond.cpu()).permute(0, 2, 1)
        out, _ = O.cfm_sample(self.sd, self.cfg, mel, list_str_to_idx(text, VOCAB), duration, steps=steps, cfg_strength=cfg_strength,
                              sway_sampling_coef=sway_sampling_coef, seed=seed, edit_mask=edit_mask.cpu(), forward_fn=self.fwd,
                              keep_trajectory=False)
        return out, None


class OracleVocos:
    def __init__(self, sd):
        self.sd = sd

    def decode(self, mel):
        return V.vocos_decode(self.sd, mel.cpu())


class OracleBigVGAN:
    def __init__(self, sd, cfg):
        self.sd, self.cfg = sd, cfg

    def __call__(self, mel):
        return B.bigvgan_forward(self.sd, self.cfg, mel.cpu())


def _recording(seconds=3.0, amp=0.05, seed=5):
    return synth.ref_audio(int(24000 * seconds), seed=seed, amp=amp)   # amp 0.05: below target_rms, so the gain / restore path runs


def _compare(tag, hip, ref):
    (w, sr, s), (w0, sr0, s0) = hip, ref
    assert sr == sr0 == 24000 and w.shape == w0.shape and s.shape == s0.shape and w.dtype == np.float32
    mel_rms = float(np.sqrt(np.mean((s - s0) ** 2)))
    wav_max = float(np.max(np.abs(w - w0)))
    print(f"[parity] {tag}: mel rms err {mel_rms:.3e}  wave max err {wav_max:.3e}  frames {s.shape[1]}  n={len(w)}")
    assert mel_rms < 1e-3
    assert wav_max < 1e-4


def _check_kept_rows(model, audio, parts, fix, spec, mel_spec_type="vocos"):
    """Rows the mask keeps are the conditioning mel bit for bit; rows it regenerates are not."""
    wav, _ = infer._prepare_reference(audio, 24000, infer.target_rms, None)
    plan = infer.plan_edit(wav.shape[-1], parts, fix)
    cond = model.cond_mel(plan.cond(wav))[0].cpu().numpy()
    n = cond.shape[0]
    keep = plan.edit_mask[:n].numpy()
    rows = spec.T[:n]
    assert keep.sum() > 0 and (~keep).sum() > 0
    assert np.array_equal(rows[keep], cond[keep])
    assert (rows[~keep] != cond[~keep]).any(axis=1).all()


_ORACLE_CACHE = {}


def _oracle(backbone, fix):
    """The CPU pipeline's result for (backbone, fix): shared by both GEMM modes."""
    key = (backbone, None if fix is None else tuple(fix))
    if key not in _ORACLE_CACHE:
        if backbone == "dit":
            sd, cfg = synth.dit_state_dict(**ARCH), O.DiTConfig(**ARCH)
            model = OracleEditModel(sd, cfg)
        else:
            sd, cfg = synth.unett_state_dict(**UARCH), O.UNetTConfig(**UARCH)
            model = OracleEditModel(sd, cfg, forward_fn=lambda **kw: O.unett_forward(sd, cfg, **kw))
        torch.manual_seed(321)
        _ORACLE_CACHE[key] = infer.speech_edit((_recording(), 24000), TEXT, PARTS, model, OracleVocos(synth.vocos_state_dict()),
                                               fix_duration=fix, **KW)
    return _ORACLE_CACHE[key]


@pytest.mark.parametrize("fix", [None, FIX], ids=["no_fix", "fix_duration"])
@pytest.mark.parametrize("planes", [2, 3], ids=["bf16x3", "mixed_f16"])
@pytest.mark.parametrize("backbone", ["dit", "unett"])
def test_speech_edit_matches_oracle_pipeline(backbone, planes, fix):
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel, UNetTArch
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    if backbone == "dit":
        model = F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB, gemm_planes=planes)
    else:
        model = F5HipModel(UNetTArch(**UARCH), synth.unett_state_dict(**UARCH), vocab_char_map=VOCAB, gemm_planes=planes)
    torch.manual_seed(321)
    hip = infer.speech_edit((_recording(), 24000), TEXT, PARTS, model, F5HipVocos(synth.vocos_state_dict()), fix_duration=fix,
                            device="cuda", **KW)
    _compare(f"speech_edit {backbone} planes={planes} fix={fix}", hip, _oracle(backbone, fix))
    _check_kept_rows(model, _recording(), PARTS, fix, hip[2])


def test_speech_edit_bigvgan_matches_oracle_pipeline():
    """mel_spec_type="bigvgan": BigVGAN's front-end (L // 256 frames, the mask cut to them) and a reduced-width BigVGAN generator."""
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipBigVGAN
    sd = synth.dit_state_dict(**ARCH)
    vsd = synth.bigvgan_state_dict(upsample_initial_channel=256)
    audio, parts, text = _recording(1.5), [[0.3, 0.6], [0.9, 1.1]], "Some call me nature."
    model = F5HipModel(DiTArch(**ARCH), sd, vocab_char_map=VOCAB, mel_spec_type="bigvgan")
    torch.manual_seed(99)
    hip = infer.speech_edit((audio, 24000), text, parts, model, F5HipBigVGAN(vsd, upsample_initial_channel=256),
                            mel_spec_type="bigvgan", device="cuda", **KW)
    torch.manual_seed(99)
    ref = infer.speech_edit((audio, 24000), text, parts, OracleEditModel(sd, O.DiTConfig(**ARCH), mel_spec_type="bigvgan"),
                            OracleBigVGAN(vsd, B.BigVGANConfig(upsample_initial_channel=256)), mel_spec_type="bigvgan", **KW)
    assert hip[2].shape[1] == 1.5 * 24000 // 256 + 1   # lens (= L // 256 mel frames) + 1
    _compare("speech_edit bigvgan", hip, ref)
    _check_kept_rows(model, audio, parts, None, hip[2], "bigvgan")


def _three_edits():
    return [((_recording(3.0), 24000), TEXT, PARTS, None),
            ((_recording(2.2, seed=8, amp=0.2), 24000), "Always remember, I endure.", [[0.4, 0.9]], [1.1]),
            ((_recording(4.1, seed=9), 24000), "I have been a silent spectator, watching species evolve.", [[0.2, 0.5], [1.0, 1.6], [3.0, 3.9]], None)]


def test_speech_edit_batch_is_one_call_and_bit_identical_to_alone():
    """Three edits of different lengths and parts in one sampler call (a ragged batch with interior regenerated runs), shape-invariant
    attention: each result is bit-identical to that edit run alone."""
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    model = F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB, attn_shape_invariant=True)
    voc = F5HipVocos(synth.vocos_state_dict())
    calls, inner = [], model.sample

    def counting_sample(*a, **k):
        calls.append(k["cond"].shape[0])
        return inner(*a, **k)
    model.sample = counting_sample
    edits = _three_edits()
    torch.manual_seed(55)
    batch = infer.speech_edit_batch(edits, model, voc, device="cuda", **KW)
    assert calls == [3]
    torch.manual_seed(55)
    alone = [infer.speech_edit(a, t, p, model, voc, fix_duration=f, device="cuda", **KW) for a, t, p, f in edits]
    assert calls == [3, 1, 1, 1]
    for i, ((w, _, s), (w1, _, s1)) in enumerate(zip(batch, alone)):
        print(f"[parity] speech_edit_batch item {i}: frames {s.shape[1]}, vs alone wave max {np.abs(w - w1).max():.3e}")
        assert np.array_equal(w, w1) and np.array_equal(s, s1)
    assert len({s.shape[1] for _, _, s in batch}) == 3


def test_edit_route_on_hip_path():
    """POST /v1/audio/edit through TTSManager.edit on the HIP objects: the WAV in the response is the 16-bit quantisation of the direct
    `speech_edit` output for the same (16-bit) recording, knobs and noise."""
    from fastapi.testclient import TestClient
    from tts_indic_server_f5_amd import serve
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    model = F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB)
    voc = F5HipVocos(synth.vocos_state_dict())
    mgr = serve.TTSManager(nfe_step=8).load(model, voc)
    buf = io.BytesIO()
    with wave.open(buf, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(24000)
        f.writeframes(np.clip(np.rint(_recording()[0].numpy() * 32768), -32768, 32767).astype("<i2").tobytes())
    client = TestClient(serve.create_app(mgr, serve.VoiceRegistry()))
    torch.manual_seed(7)
    r = client.post("/v1/audio/edit", json=dict(audio=base64.b64encode(buf.getvalue()).decode(), text=TEXT, parts_to_edit=PARTS,
                                                fix_duration=FIX))
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav"
    with wave.open(io.BytesIO(r.content), "rb") as f:
        assert f.getframerate() == 24000
        pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    torch.manual_seed(7)
    w, _, _ = infer.speech_edit(buf.getvalue(), TEXT, PARTS, model, voc, fix_duration=FIX, device="cuda", **KW)
    want = np.clip(np.rint(w.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    print(f"[parity] /v1/audio/edit vs direct speech_edit: n={len(pcm)}, max |diff| {np.abs(pcm.astype(int) - want).max()} LSB")
    assert np.array_equal(pcm, want)


def test_speech_edit_f5_base_width_matches_oracle_pipeline():
    """F5-Base geometry (synthetic weights), a 10 s recording, 4 steps, CFG 2, the fix_duration splice."""
    from tts_indic_server_f5_amd.model import F5TTS_BASE, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    sd, vsd = synth.dit_state_dict(), synth.vocos_state_dict()
    audio, parts, fix = (synth.ref_audio(240_000, amp=0.15), 24000), [[2.0, 3.5], [6.0, 7.2]], [1.2, 1.0]
    text = "I do not care what you call me. I have been a silent spectator, watching species evolve, empires rise and fall."
    kw = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0)
    torch.manual_seed(31)
    hip = infer.speech_edit(audio, text, parts, F5HipModel(F5TTS_BASE, sd, vocab_char_map=VOCAB), F5HipVocos(vsd), fix_duration=fix,
                            device="cuda", **kw)
    torch.manual_seed(31)
    ref = infer.speech_edit(audio, text, parts, OracleEditModel(sd, O.DiTConfig()), OracleVocos(vsd), fix_duration=fix, **kw)
    s, s0 = hip[2], ref[2]
    mel_rms = float(np.sqrt(np.mean((s - s0) ** 2)))
    print(f"[parity] speech_edit F5-Base 10 s: mel rms err {mel_rms:.3e}  wave max err {np.abs(hip[0] - ref[0]).max():.3e}  frames {s.shape[1]}")
    assert s.shape == s0.shape and mel_rms < 1e-3
