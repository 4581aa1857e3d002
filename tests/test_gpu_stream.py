"""GPU: the ragged Vocos decode (`F5HipVocos.decode_ragged`, f5hip_vocos_decode_ragged) against per-item `decode` and the CPU oracle, and
streamed synthesis (`infer.infer_process_stream`, `serve.TTSManager.synthesize_stream`) against the unstreamed result, to the last bit."""
import ctypes as C
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vocos_ref as R  # noqa: E402
from oracle import vocos_oracle as V  # noqa: E402
from tts_indic_server_f5_amd import _lib, infer, serve, synth  # noqa: E402

ARCH = dict(dim=256, depth=4, heads=4, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=96)
VOCAB = {chr(32 + i): i for i in range(96)}   # printable ASCII, " " -> 0
FRAMES = [2, 3, 127, 128, 129, 700, 1404]
KW = dict(nfe_step=8, cfg_strength=2.0, sway_sampling_coef=-1.0)
# 2 s prompt with a 9-byte transcript: 103-byte chunks, so this text is three chunks of ~1 000 frames
REF_TEXT = "Hi there."
TEXT = ("I do not care what you call me, I have been a silent spectator. Watching species evolve, empires rise and fall. "
        "Always remember, I am mighty and enduring. Respect me and I will nurture you; ignore me and you shall face the consequences.")


@pytest.fixture(scope="module")
def vocos():
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipVocos(synth.vocos_state_dict())


def _mels(frames, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(100, t, generator=g) * 1.5 - 1.0 for t in frames]


def test_decode_ragged_equals_per_item_decode(vocos):
    mels = _mels(FRAMES)
    alone = [vocos.decode(m[None])[0] for m in mels]
    got = vocos.decode_ragged(mels)
    assert [w.shape[0] for w in got] == [256 * (t - 1) for t in FRAMES]
    for t, a, w in zip(FRAMES, alone, got):
        assert torch.equal(a, w), f"T={t}: max diff {(a - w).abs().max().item():.3e}"
    order = np.random.default_rng(3).permutation(len(FRAMES))
    shuffled = vocos.decode_ragged([mels[i] for i in order])
    for i, w in zip(order, shuffled):
        assert torch.equal(alone[i], w), f"shuffled T={FRAMES[i]}"
    # the C entry point through ctypes (packed output, item i at hop * sum_{j<i} (T_j - 1)) gives the same bytes
    mel = torch.zeros(len(mels), 100, max(FRAMES))
    for i, m in enumerate(mels):
        mel[i, :, :FRAMES[i]] = m
    mel = mel.cuda()
    f = torch.tensor(FRAMES, dtype=torch.int32)
    packed = torch.empty(256 * sum(t - 1 for t in FRAMES), device="cuda")
    _lib.check(_lib.lib().f5hip_vocos_decode_ragged(vocos._h, len(FRAMES), C.c_void_p(f.data_ptr()), C.c_void_p(mel.data_ptr()),
                                                    C.c_void_p(packed.data_ptr()), _lib.current_stream_ptr()), "decode_ragged")
    assert torch.equal(packed, torch.cat(alone))


def test_decode_ragged_vs_oracle(vocos):
    mels = _mels(FRAMES, seed=12)
    got = vocos.decode_ragged(mels)
    sd = synth.vocos_state_dict()
    for t, m, w in zip(FRAMES, mels, got):
        ref = V.vocos_decode(sd, m[None])[0]
        mx = (w.cpu() - ref).abs().max().item()
        print(f"[parity] decode_ragged T={t}: max_err {mx:.3e}")
        assert mx < 1e-4
    # and by the rule of tests/test_gpu_vocos_stages.py: within 3 x the split-bf16 operand model's own distance from float64
    (g_max, g_rms), (m_max, m_rms) = R.decode_errors(R.Weights(sd), mels, got, 2)
    print(f"[parity] decode_ragged: gpu_err max {g_max:.3e} rms {g_rms:.3e}   model_err max {m_max:.3e} rms {m_rms:.3e}")
    assert g_max <= 3.0 * m_max and g_rms <= 3.0 * m_rms


def test_decode_ragged_rejects_bad_frames(vocos):
    with pytest.raises(_lib.F5HipError):
        vocos.decode_ragged([torch.zeros(100, 5), torch.zeros(100, 1)])
    with pytest.raises(_lib.F5HipError):
        vocos.decode_ragged([torch.zeros(100, 5), torch.zeros(80, 5)])


class PerChunkVocos:
    """The same vocoder without `decode_ragged`: infer falls back to one `decode` per chunk."""

    def __init__(self, v):
        self.v = v

    def decode(self, mel):
        return self.v.decode(mel)


def _model():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB, attn_shape_invariant=True)


def test_infer_requests_ragged_vocode_equals_per_chunk_loop(vocos):
    va = (synth.ref_audio(24000 * 2, amp=0.15), 24000)
    vb = (synth.ref_audio(int(24000 * 1.4), seed=9, amp=0.03), 24000)     # below the rms floor: gain restored per chunk
    reqs = [(va, REF_TEXT, TEXT), (vb, "Others say mother.", "Always remember, I endure."), (va, REF_TEXT, TEXT[:150])]
    model = _model()
    torch.manual_seed(21)
    ragged = infer.infer_requests(reqs, model, vocos, device="cuda", **KW)
    torch.manual_seed(21)
    loop = infer.infer_requests(reqs, model, PerChunkVocos(vocos), device="cuda", **KW)
    n_chunks = [len(infer.request_chunks(rt, a[0].shape[-1] / a[1], gt)) for a, rt, gt in reqs]
    assert n_chunks == [3, 1, 2]
    for (w, sr, s), (w1, sr1, s1) in zip(ragged, loop):
        assert sr == sr1 == 24000 and w.dtype == w1.dtype
        np.testing.assert_array_equal(w, w1)
        np.testing.assert_array_equal(s, s1)


def test_infer_process_stream_equals_infer_process(vocos):
    va = (synth.ref_audio(24000 * 2, amp=0.15), 24000)
    model = _model()
    torch.manual_seed(5)
    w, sr, _ = infer.infer_process(va, REF_TEXT, TEXT, model, vocos, device="cuda", show_info=lambda *_: None, **KW)
    torch.manual_seed(5)
    pieces = list(infer.infer_process_stream(va, REF_TEXT, TEXT, model, vocos, device="cuda", show_info=lambda *_: None, **KW))
    assert len(pieces) >= 2 and all(p.dtype == np.float32 for p in pieces)
    np.testing.assert_array_equal(np.concatenate(pieces), w.astype(np.float32))


def _pcm(x):
    return np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def test_manager_stream_equals_unstreamed_through_micro_batcher(vocos, tmp_path):
    x = (synth.ref_audio(24000 * 2, amp=0.15).numpy()[0] * 32767).astype(np.int16)
    p = tmp_path / "prompt.wav"
    with wave.open(str(p), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(24000)
        f.writeframes(x.tobytes())
    mgr = serve.TTSManager(nfe_step=8, micro_batch=dict(max_requests=8, max_wait_ms=5)).load(_model(), vocos)
    try:
        torch.manual_seed(8)
        whole = mgr.synthesize(TEXT, ref_audio_path=str(p), ref_text=REF_TEXT)
        torch.manual_seed(8)
        pieces = list(mgr.synthesize_stream(TEXT, ref_audio_path=str(p), ref_text=REF_TEXT))
        assert len(pieces) >= 2 and mgr.batcher.batch_sizes[-2:] == [1, 1]     # head and tail in batches of their own
        np.testing.assert_array_equal(_pcm(np.concatenate(pieces)), _pcm(whole))
    finally:
        mgr.close()
