"""GPU: per-unit CFG strength (f5hip_cfm_sample_units, torch.ops.f5hip.cfm_sample_units) and per-request sampler settings through the
serving manager.  A unit sampled inside a mixed-strength call equals the same unit sampled alone with its strength as the scalar, bit for
bit (shape-invariant attention), for DiT, UNetT and MMDiT under Euler, midpoint and RK4, and stays within north_star's 1e-3 RMS of the CPU
oracle's sampler at that strength."""
import threading
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dit_oracle as O  # noqa: E402
from rk4_oracle import cfm_sample_rk4  # noqa: E402
from tts_indic_server_f5_amd import serve, synth, torch_ops  # noqa: E402

TINY = dict(dim=128, depth=2, heads=2, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=40)
UTINY = dict(dim=128, depth=4, heads=2, ff_mult=4, text_num_embeds=40)
MMTINY = dict(dim=128, depth=3, heads=2, ff_mult=2, text_num_embeds=40)
CFGS = [2.0, 0.0, 3.5, 2.0]
PROMPTS, TEXTS, FRAMES = [24, 30, 18, 24], [12, 20, 8, 12], [60, 90, 45, 140]


def _rms(a, b):
    return (a.float().cpu() - b.float().cpu()).pow(2).mean().sqrt().item()


def _units(seed=5, n_tok=40):
    """Four units with their own prompt mel, text, planned frames and noise (at the final duration, cfm.py:136)."""
    from tts_indic_server_f5_amd.model import unit_duration
    g = torch.Generator().manual_seed(seed)
    out = []
    for p, t, f in zip(PROMPTS, TEXTS, FRAMES):
        cond = torch.randn(1, p, 100, generator=g)
        text = torch.randint(0, n_tok, (1, t), generator=g)
        y0 = torch.randn(unit_duration(p, t, f), 100, generator=g)
        out.append((cond, text, f, y0))
    return out


def _batched(model, units, cfg, steps=6):
    conds = torch.nn.utils.rnn.pad_sequence([c[0] for c, _, _, _ in units], batch_first=True)
    texts = torch.nn.utils.rnn.pad_sequence([t[0] for _, t, _, _ in units], batch_first=True, padding_value=-1)
    lens = torch.tensor([c.shape[1] for c, _, _, _ in units])
    frames = torch.tensor([f for _, _, f, _ in units])
    out, _ = model.sample(conds, texts, frames, lens=lens, y0=[y for _, _, _, y in units], steps=steps, cfg_strength=cfg,
                          sway_sampling_coef=-1.0)
    return [out[i, :y.shape[0]] for i, (_, _, _, y) in enumerate(units)]


def _backbone(kind):
    from tts_indic_server_f5_amd.model import DiTArch, MMDiTArch, UNetTArch
    if kind == "dit":
        sd, cfg = synth.dit_state_dict(**TINY), O.DiTConfig(**TINY)
        return DiTArch(**TINY), sd, (lambda **kw: O.dit_forward(sd, cfg, **kw)), cfg
    if kind == "unett":
        sd, cfg = synth.unett_state_dict(**UTINY), O.UNetTConfig(**UTINY)
        return UNetTArch(**UTINY), sd, (lambda **kw: O.unett_forward(sd, cfg, **kw)), cfg
    sd, cfg = synth.mmdit_state_dict(**MMTINY), O.MMDiTConfig(**MMTINY)
    return MMDiTArch(**MMTINY), sd, (lambda **kw: O.mmdit_forward(sd, cfg, **kw)), cfg


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("kind", ["dit", "unett", "mmdit"])
def test_mixed_cfg_units_equal_alone_and_oracle(kind, method, attn_shape_invariant):
    from tts_indic_server_f5_amd.model import F5HipModel
    arch, sd, fwd, cfg = _backbone(kind)
    model = F5HipModel(arch, sd, odeint_kwargs=dict(method=method))
    units = _units()
    mixed = _batched(model, units, CFGS)
    for i, (u, c) in enumerate(zip(units, CFGS)):
        alone = _batched(model, [u], c)[0]
        assert torch.equal(mixed[i], alone), f"{kind} {method} unit {i} (cfg {c}): max diff {(mixed[i] - alone).abs().max().item():.3e}"
        cond, text, f, y0 = u
        kw = dict(steps=6, cfg_strength=c, sway_sampling_coef=-1.0, y0=y0[None], forward_fn=fwd)
        if method == "rk4":
            ref = cfm_sample_rk4(sd, cfg, cond, text, f, **kw)
        else:
            ref, _ = O.cfm_sample(sd, cfg, cond, text, f, method=method, keep_trajectory=False, **kw)
        p = cond.shape[1]
        rms = _rms(mixed[i][p:], ref[0, p:])
        print(f"[parity] {kind} {method} unit {i} cfg {c}: rms vs oracle {rms:.3e}")
        assert rms < 1e-3
    # the per-unit path with one strength everywhere is the scalar path
    same = _batched(model, units, [2.0] * 4)
    for a, b in zip(same, _batched(model, units, 2.0)):
        assert torch.equal(a, b)


def test_cfm_sample_units_torch_op_equals_ctypes(monkeypatch, attn_shape_invariant):
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    assert torch_ops.load()
    model = F5HipModel(DiTArch(**TINY), synth.dit_state_dict(**TINY))
    units = _units(seed=6)
    via_op = _batched(model, units, CFGS)
    monkeypatch.setattr(torch_ops, "load", lambda: False)
    via_ctypes = _batched(model, units, CFGS)
    for a, b in zip(via_op, via_ctypes):
        assert torch.equal(a, b)


def test_cfm_sample_units_op_checks_its_arguments():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    model = F5HipModel(DiTArch(**TINY), synth.dit_state_dict(**TINY))
    dur = torch.tensor([30, 40], dtype=torch.int32)
    cond = torch.zeros(70, 100, device="cuda")
    args = (int(model._h), dur, None, cond, torch.ones(70, dtype=torch.uint8), torch.zeros(2, 5, dtype=torch.int32), cond.clone(),
            torch.linspace(0, 1, 3))
    with pytest.raises(RuntimeError, match="one value per unit"):
        torch_ops.ops().cfm_sample_units(*args, torch.tensor([2.0]))
    with pytest.raises(RuntimeError, match="sum\\(dur\\)"):
        torch_ops.ops().cfm_sample_units(*args[:3], cond[:60], torch.ones(60, dtype=torch.uint8), args[5], cond[:60].clone(), args[7],
                                         torch.tensor([2.0, 0.0]))


def test_f5_base_width_mixed_cfg_batch_vs_oracle():
    """F5-Base geometry (real-width block GEMMs), default mixed mode: three units at CFG 2, 0 and 3 in one call, 4 Euler steps."""
    from tts_indic_server_f5_amd.model import F5TTS_BASE, F5HipModel, unit_duration
    sd, cfg = synth.dit_state_dict(), O.DiTConfig()
    model = F5HipModel(F5TTS_BASE, sd)
    g = torch.Generator().manual_seed(31)
    units = []
    for p, n_gen, f, c in [(80, 60, 256, 2.0), (64, 40, 200, 0.0), (96, 50, 300, 3.0)]:
        cond = torch.randn(1, p, 100, generator=g)
        text = synth.text_ids(n_ref=20, n_gen=n_gen)
        units.append((cond, text, f, torch.randn(unit_duration(p, text.shape[1], f), 100, generator=g), c))
    conds = torch.nn.utils.rnn.pad_sequence([u[0][0] for u in units], batch_first=True)
    texts = torch.nn.utils.rnn.pad_sequence([u[1][0] for u in units], batch_first=True, padding_value=-1)
    out, _ = model.sample(conds, texts, torch.tensor([u[2] for u in units]), lens=torch.tensor([u[0].shape[1] for u in units]),
                          y0=[u[3] for u in units], steps=4, cfg_strength=[u[4] for u in units], sway_sampling_coef=-1.0)
    for i, (cond, text, f, y0, c) in enumerate(units):
        ref, _ = O.cfm_sample(sd, cfg, cond, text, f, steps=4, cfg_strength=c, sway_sampling_coef=-1.0, y0=y0[None], keep_trajectory=False)
        p, n = cond.shape[1], y0.shape[0]
        rms = _rms(out[i, p:n], ref[0, p:])
        print(f"[parity] F5-Base mixed-CFG unit {i} (cfg {c}, {n} frames): rms vs oracle {rms:.3e}")
        assert rms < 1e-3


# ---------------------------------------------------------------------------------------------------------------- serving
ARCH = dict(dim=256, depth=4, heads=4, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=96)
VOCAB = {chr(32 + i): i for i in range(96)}
REF_TEXT = "Hi there."
TEXT = ("I do not care what you call me, I have been a silent spectator. Watching species evolve, empires rise and fall. "
        "Always remember, I am mighty and enduring. Respect me and I will nurture you; ignore me and you shall face the consequences.")
REQS = [dict(text=TEXT, speed=1.3, nfe_step=8, cfg_strength=2.0, seed=11),
        dict(text="Always remember, I endure.", speed=0.8, nfe_step=6, cfg_strength=0.0, seed=12),
        dict(text=TEXT[:150], speed=1.0, nfe_step=8, cfg_strength=3.5, sway_sampling_coef=0.0, seed=13)]


def _prompt(tmp_path):
    x = (synth.ref_audio(24000 * 2, amp=0.15).numpy()[0] * 32767).astype(np.int16)
    p = tmp_path / "prompt.wav"
    with wave.open(str(p), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(24000)
        f.writeframes(x.tobytes())
    return str(p)


def test_manager_mixed_requests_equal_alone_and_seeded_repeat(tmp_path):
    """Three concurrent requests with different speed, nfe_step, cfg_strength and seed ride in one micro-batch (two time grids: two
    sampler calls); each equals the same request served alone.  A seeded request served twice is identical, and streamed it equals the
    unstreamed wave."""
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    path = _prompt(tmp_path)
    model = F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB)
    mgr = serve.TTSManager(nfe_step=8, micro_batch=dict(max_requests=8, max_wait_ms=300)).load(model, F5HipVocos(synth.vocos_state_dict()))
    try:
        mgr.synthesize("Warm up.", ref_audio_path=path, ref_text=REF_TEXT, seed=1)    # the voice is prepared before the concurrent burst
        res, barrier = [None] * 3, threading.Barrier(3)

        def run(i):
            kw = dict(REQS[i])
            text = kw.pop("text")
            barrier.wait()
            res[i] = mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, **kw)

        threads = [threading.Thread(target=run, args=(i,)) for i in range(3)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=600)
        assert mgr.batcher.batch_sizes[-1] == 3, mgr.batcher.batch_sizes
        for i, r in enumerate(REQS):
            kw = dict(r)
            text = kw.pop("text")
            alone = mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, **kw)
            assert mgr.batcher.batch_sizes[-1] == 1
            np.testing.assert_array_equal(res[i], alone)
            again = mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, **kw)
            np.testing.assert_array_equal(alone, again)
        assert res[0].shape != res[2].shape and not np.array_equal(res[0][:1000], res[2][:1000])
        kw = dict(REQS[0])
        text = kw.pop("text")
        whole = mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, **kw)
        pieces = list(mgr.synthesize_stream(text, ref_audio_path=path, ref_text=REF_TEXT, **kw))
        assert len(pieces) >= 2
        np.testing.assert_array_equal(np.concatenate(pieces), whole)
    finally:
        mgr.close()
