"""GPU: the fixed-grid RK4 solver (CFM(odeint_kwargs=dict(method="rk4")), f5hip_dit_set_ode_method(h, 2): cfg_step_kernel's RK4 ops, four
backbone evaluations per step) against the CPU RK4 sampler of tests/rk4_oracle.py, for all three backbones and every entry point.  The
rule itself is pinned by tests/test_rk4_rule.py (torchdiffeq is absent: unpinned leaf).  Tolerances: north_star's 1e-3 RMS on mel frames."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dit_oracle as O  # noqa: E402
from oracle import vocos_oracle as V  # noqa: E402
from rk4_oracle import cfm_sample_rk4  # noqa: E402
from tts_indic_server_f5_amd import infer, synth  # noqa: E402
from tts_indic_server_f5_amd.tokenizer import list_str_to_idx  # noqa: E402

TINY = dict(dim=128, depth=2, heads=2, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=40)
UTINY = dict(dim=128, depth=4, heads=2, ff_mult=4, text_num_embeds=40)
MMTINY = dict(dim=128, depth=3, heads=2, ff_mult=2, text_num_embeds=40)


def _rms(a, b):
    return (a.float().cpu() - b.float().cpu()).pow(2).mean().sqrt().item()


def _report(tag, got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    d = got - ref
    rms = d.pow(2).mean().sqrt().item()
    print(f"[parity] {tag}: rms_err {rms:.3e} max_err {d.abs().max():.3e} ref_rms {ref.pow(2).mean().sqrt():.3e}")
    return rms


def _tiny_inputs(seed=63):
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(1, 24, 100, generator=g)
    text = torch.randint(0, 40, (1, 12), generator=g)
    y0 = torch.randn(1, 60, 100, generator=g)
    return cond, text, y0


def _solver_comparison(tag, arch, sd, cfg, forward_fn, planes):
    """RK4 on the device vs the CPU RK4 sampler (8 steps, CFG 2, sway -1), and clearly apart from the Euler and midpoint samples of the
    same backbone (not a relabelled solver).  Returns the RK4 model."""
    from tts_indic_server_f5_amd.model import F5HipModel
    cond, text, y0 = _tiny_inputs()
    kw = dict(steps=8, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0)
    rk4 = F5HipModel(arch, sd, gemm_planes=planes, odeint_kwargs=dict(method="rk4"))
    got, _ = rk4.sample(cond, text, 60, **kw)
    ref = cfm_sample_rk4(sd, cfg, cond, text, 60, forward_fn=forward_fn, **kw)
    assert _report(f"{tag} rk4 sample", got[:, 24:], ref[:, 24:]) < 1e-3
    assert torch.equal(got[:, :24].cpu(), cond)
    for other in ("euler", "midpoint"):
        o, _ = F5HipModel(arch, sd, gemm_planes=planes, odeint_kwargs=dict(method=other)).sample(cond, text, 60, **kw)
        d = _rms(got[:, 24:], o[:, 24:])
        print(f"[parity] {tag} rk4 vs {other}: rms {d:.3e}")
        assert d > 1e-2
    return rk4


@pytest.mark.parametrize("planes", [2, 3], ids=["bf16x3", "mixed_f16"])
def test_rk4_tiny_dit_vs_cpu_rk4(planes):
    from tts_indic_server_f5_amd._lib import F5HipError
    from tts_indic_server_f5_amd.model import DiTArch
    sd, cfg = synth.dit_state_dict(**TINY), O.DiTConfig(**TINY)
    model = _solver_comparison("dit tiny", DiTArch(**TINY), sd, cfg, lambda **kw: O.dit_forward(sd, cfg, **kw), planes)
    cond, text, y0 = _tiny_inputs()
    # 3 * steps + 1 time points of the 128 the time table holds: 42 steps is the limit, 43 is refused before any launch
    out, _ = model.sample(cond, text, 60, steps=42, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0)
    assert torch.isfinite(out).all()
    with pytest.raises(F5HipError, match="rk4.*42"):
        model.sample(cond, text, 60, steps=43, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0)
    again, _ = model.sample(cond, text, 60, steps=42, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0)
    assert torch.equal(out, again)                                   # the handle is still usable after the refusal


@pytest.mark.parametrize("planes", [2, 3], ids=["bf16x3", "mixed_f16"])
def test_rk4_tiny_unett_vs_cpu_rk4(planes):
    """UNetT: the time-token row of every sequence takes each stage's own time embedding."""
    from tts_indic_server_f5_amd.model import UNetTArch
    sd, cfg = synth.unett_state_dict(**UTINY), O.UNetTConfig(**UTINY)
    _solver_comparison("unett tiny", UNetTArch(**UTINY), sd, cfg, lambda **kw: O.unett_forward(sd, cfg, **kw), planes)


@pytest.mark.parametrize("planes", [2, 3], ids=["bf16x3", "mixed_f16"])
def test_rk4_tiny_mmdit_vs_cpu_rk4(planes):
    """MMDiT: the text stream restarts from its step-invariant embedding at every stage, modulated with that stage's time."""
    from tts_indic_server_f5_amd.model import MMDiTArch
    sd, cfg = synth.mmdit_state_dict(**MMTINY), O.MMDiTConfig(**MMTINY)
    _solver_comparison("mmdit tiny", MMDiTArch(**MMTINY), sd, cfg, lambda **kw: O.mmdit_forward(sd, cfg, **kw), planes)


def test_rk4_f5_base_short_utterance_vs_cpu_rk4():
    """F5-Base geometry (the real-width block GEMMs), one short utterance: 256 frames, 4 steps = 16 NFE, CFG 2, default (mixed) mode."""
    from tts_indic_server_f5_amd.model import F5TTS_BASE, F5HipModel
    sd, cfg = synth.dit_state_dict(), O.DiTConfig()
    g = torch.Generator().manual_seed(21)
    cond = torch.randn(1, 80, 100, generator=g)
    text = synth.text_ids(n_ref=20, n_gen=60)
    y0 = synth.noise(256, 0)[None]
    kw = dict(steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0)
    got, _ = F5HipModel(F5TTS_BASE, sd, odeint_kwargs=dict(method="rk4")).sample(cond, text, 256, **kw)
    ref = cfm_sample_rk4(sd, cfg, cond, text, 256, **kw)
    assert _report("F5-Base rk4, 256 frames, 4 steps (generated frames)", got[:, 80:], ref[:, 80:]) < 1e-3


def test_rk4_batch_of_copies_and_ragged_pair_equal_single(attn_shape_invariant):
    """With the shape-invariant attention a unit's RK4 sample does not depend on what it is batched with: 3 copies in one call, and a
    ragged pair (different lengths, texts and noise), each equal bit for bit to the unit sampled alone."""
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    model = F5HipModel(DiTArch(**TINY), synth.dit_state_dict(**TINY), odeint_kwargs=dict(method="rk4"))
    kw = dict(steps=6, cfg_strength=2.0, sway_sampling_coef=-1.0)
    cond, text, y0 = _tiny_inputs()
    one, _ = model.sample(cond, text, 60, y0=y0, **kw)
    three, _ = model.sample(cond.expand(3, -1, -1), text.expand(3, -1), 60, y0=y0.expand(3, -1, -1), **kw)
    for i in range(3):
        print(f"[parity] rk4 copy {i} of 3 vs alone: max {(three[i] - one[0]).abs().max().item():.3e}")
        assert torch.equal(three[i], one[0])
    g = torch.Generator().manual_seed(41)
    cond2 = torch.randn(2, 20, 100, generator=g)
    text2 = torch.randint(0, 40, (2, 26), generator=g)
    text2[1, 15:] = -1
    durs = [70, 131]
    y0s = [torch.randn(n, 100, generator=g) for n in durs]
    pair, _ = model.sample(cond2, text2, torch.tensor(durs), y0=y0s, **kw)
    for i, n in enumerate(durs):
        alone, _ = model.sample(cond2[i:i + 1], text2[i:i + 1], n, y0=[y0s[i]], **kw)
        print(f"[parity] rk4 ragged item {i} (n={n}) vs alone: max {(pair[i, :n] - alone[0]).abs().max().item():.3e}")
        assert torch.equal(pair[i, :n], alone[0])
        assert (pair[i, n:] == 0).all()


def test_rk4_torch_custom_op_equals_the_ctypes_path():
    """torch.ops.f5hip.cfm_sample on an RK4 handle (the method lives on the handle) is bit-identical to the ctypes binding."""
    from tts_indic_server_f5_amd import torch_ops
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    assert torch_ops.load()
    model = F5HipModel(DiTArch(**TINY), synth.dit_state_dict(**TINY), odeint_kwargs=dict(method="rk4"))
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(2, 12, 100, generator=g)
    text = torch.randint(0, 40, (2, 14), generator=g)
    y0 = [torch.randn(40, 100, generator=g), torch.randn(33, 100, generator=g)]
    kw = dict(steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0)
    via_ops, _ = model.sample(cond, text, torch.tensor([40, 33]), **kw)
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        via_ctypes, _ = model.sample(cond, text, torch.tensor([40, 33]), **kw)
    finally:
        torch_ops._loaded = True
    assert torch.equal(via_ops, via_ctypes)


# ---------------------------------------------------------------- end to end: load_model(ode_method="rk4") -> infer_process
ARCH = dict(dim=256, depth=4, heads=4, ff_mult=2, text_dim=64, conv_layers=2)
VOCAB = {chr(32 + i): i for i in range(96)}   # printable ASCII, " " -> 0


class OracleRK4Model:
    """CFM.sample with the RK4 solver on the CPU oracle (raw-wave cond -> oracle mel; list[str] text -> vocab lookup)."""

    def __init__(self, sd):
        self.sd, self.cfg = sd, O.DiTConfig(text_num_embeds=96, **ARCH)

    def sample(self, cond, text, duration, steps, cfg_strength, sway_sampling_coef):
        mel = V.vocos_mel_spectrogram(cond.cpu()).permute(0, 2, 1)
        out = cfm_sample_rk4(self.sd, self.cfg, mel, list_str_to_idx(text, VOCAB), duration, steps=steps, cfg_strength=cfg_strength,
                             sway_sampling_coef=sway_sampling_coef)
        return out, None


class OracleVocoder:
    def __init__(self, sd):
        self.sd = sd

    def decode(self, mel):
        return V.vocos_decode(self.sd, mel.cpu())


def test_rk4_load_model_infer_process_matches_oracle_pipeline(tmp_path):
    """A checkpoint file -> infer.load_model(..., ode_method="rk4", ckpt_path=...) -> infer_process with the synthetic Vocos, against the
    same host glue driving the CPU RK4 sampler and the Vocos oracle (the e2e bounds of tests/test_gpu_e2e.py)."""
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    sd, vsd = synth.dit_state_dict(text_num_embeds=96, **ARCH), synth.vocos_state_dict()
    path = str(tmp_path / "model_rk4.pt")
    torch.save({"ema_model_state_dict": {"ema_model." + k: v for k, v in sd.items()}}, path)
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("".join(c + "\n" for c in VOCAB), encoding="utf-8")
    model = infer.load_model(infer.DiT, ARCH, vocab_file=str(vocab), ode_method="rk4", ckpt_path=path, device="cuda")
    assert model.odeint_kwargs == dict(method="rk4") and model.vocab_char_map == VOCAB
    ref_audio = (synth.ref_audio(24000 * 2, amp=0.15), 24000)
    ref_text = "Some call me nature."
    gen_text = "I do not care what you call me. I have been a silent spectator, watching species evolve. Always remember, I endure."
    kw = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0)
    torch.manual_seed(123)
    w_hip, sr, spec_hip = infer.infer_process(ref_audio, ref_text, gen_text, model, F5HipVocos(vsd), device="cuda", **kw)
    torch.manual_seed(123)
    w_ref, _, spec_ref = infer.infer_process(ref_audio, ref_text, gen_text, OracleRK4Model(sd), OracleVocoder(vsd), **kw)
    assert sr == 24000 and w_hip.shape == w_ref.shape and spec_hip.shape == spec_ref.shape
    mel_rms = float(np.sqrt(np.mean((spec_hip - spec_ref) ** 2)))
    wav_max = float(np.max(np.abs(w_hip - w_ref)))
    print(f"[parity] e2e rk4: mel rms err {mel_rms:.3e}  wave max err {wav_max:.3e}  n={len(w_ref)}")
    assert mel_rms < 1e-3
    assert wav_max < 1e-4
