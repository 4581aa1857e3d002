"""CPU: pins the per-block float64 references of tests/block_ref.py and the sensitivity of the per-block GPU test (tests/test_gpu_blocks.py).

Chain check: the unrounded references chained over all blocks reproduce the oracle's whole forwards in float64 (1e-10: float64 rounding).
Sensitivity table: what each deliberate slip of the block composition moves, against the tolerance the GPU test derives (3 x the rms
distance between the reference with a mode's operand formats and the exact reference)."""
import pytest
import torch

import block_ref as B
from oracle import dit_oracle as O
from tts_indic_server_f5_amd import synth

TINY = dict(dim=128, depth=2, heads=2, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=40)   # the tiny configs of tests/test_gpu_dit.py
UTINY = dict(dim=128, depth=4, heads=2, ff_mult=4, text_num_embeds=40)
MMTINY = dict(dim=128, depth=3, heads=2, ff_mult=2, text_num_embeds=40)

FACTOR = 3.0    # gpu_err <= FACTOR x model_err (tests/test_gpu_blocks.py)
MARGIN = 2.0    # a caught mutation moves the block output by at least MARGIN x that tolerance

# (mutation, where it is measured, the modes whose tolerance must catch it).  Where: "A" block 0 of case A's first sequence, "A final" the
# final norm + proj_out behind it (mode-2 tolerance in both modes), "C" layer 3 of case C's first sequence (UNetT: RMSNorm, skips),
# "D" block 0 of case D's second sequence (MMDiT, padded text).
MUTATIONS = [
    ("gelu_exact", "A", (2,)),
    ("unbiased_variance", "A", (2,)),
    ("unbiased_variance", "C", (2,)),
    ("gates_exchanged", "A", (2, 3)),
    ("scale_shift_exchanged", "A", (2, 3)),
    ("no_out_bias", "A", (2, 3)),
    ("rotary_every_head", "A", (2, 3)),
    ("final_scale_shift_exchanged", "A final", (2, 3)),
    ("skip_wrong_layer", "C", (2, 3)),
    ("text_keys_masked", "D", (2, 3)),
    ("eps_1e-5", "A", ()),          # undetectable: below every mode's own rounding (rms 2.5e-6 at case A's inputs; mode 2's tolerance there is 2.0e-5)
]
# below mode 3's floor today; asserted so that this table is revisited if the mixed mode's precision ever improves
BELOW_MODE3 = [("gelu_exact", "A"), ("unbiased_variance", "A"), ("unbiased_variance", "C")]


def _rms(a, b):
    return (a - b).pow(2).mean().sqrt().item()


# ---------------------------------------------------------------------------------------------------------------- chain check
def _tiny_inputs(vocab, seed, nt=30):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 40, 100, generator=g, dtype=torch.float64)
    cond = torch.randn(2, 40, 100, generator=g, dtype=torch.float64)
    text = torch.randint(0, vocab, (2, nt), generator=g)
    text[1, 20:] = -1
    return x, cond, text, torch.tensor(0.37, dtype=torch.float64), O.lens_to_mask(torch.tensor([40, 29]), 40), (40, 29)


def test_chain_reproduces_dit_forward():
    cfg, sd = O.DiTConfig(**TINY), synth.dit_state_dict(**TINY)
    W = B.Weights(sd)
    x, cond, text, t, mask, kv = _tiny_inputs(40, 1)
    ref = O.dit_forward(W.sd, cfg, x, cond, text, t, False, False, mask=mask)
    temb = O.time_embed(W.sd, t.repeat(2))
    h0 = O.input_embed(W.sd, x, cond, O.text_embed(W.sd, cfg, text, 40, False), False)
    for i in range(2):
        h = h0[i]
        for l in range(cfg.depth):
            h = B.dit_block(W, l, h, temb[i], kv[i], B.UNROUNDED)
        assert (B.final_dit(W, h, temb[i], B.UNROUNDED) - ref[i]).abs().max().item() < 1e-10


def test_chain_reproduces_unett_forward():
    cfg, sd = O.UNetTConfig(**UTINY), synth.unett_state_dict(**UTINY)
    W = B.Weights(sd)
    x, cond, text, t, mask, kv = _tiny_inputs(40, 2)
    ref = O.unett_forward(W.sd, cfg, x, cond, text, t, False, False, mask=mask)
    temb = O.time_embed(W.sd, t.repeat(2))
    h0 = O.input_embed(W.sd, x, cond, O.text_embed(W.sd, cfg, text, 40, False), False)
    for i in range(2):
        h, skips = torch.cat((temb[i][None], h0[i])), []
        for l in range(cfg.depth):
            if l < cfg.depth // 2:
                skips.append(h)
            h = B.unett_layer(W, l, cfg.depth, h, None if l < cfg.depth // 2 else skips[cfg.depth - 1 - l], kv[i], B.UNROUNDED)
        assert (B.final_unett(W, h, B.UNROUNDED) - ref[i]).abs().max().item() < 1e-10


def test_chain_reproduces_mmdit_forward():
    cfg, sd = O.MMDiTConfig(**MMTINY), synth.mmdit_state_dict(**MMTINY)
    W = B.Weights(sd)
    x, cond, text, t, mask, kv = _tiny_inputs(40, 3)
    ref = O.mmdit_forward(W.sd, cfg, x, cond, text, t, False, False, mask=mask)
    temb = O.time_embed(W.sd, t.repeat(2))
    c0, h0 = O.mmdit_text_embed(W.sd, cfg, text, False), O.mmdit_audio_embed(W.sd, x, cond, False)
    for i in range(2):
        h, c = h0[i], c0[i]
        for l in range(cfg.depth):
            h, c = B.mmdit_block(W, l, cfg.depth, h, c, temb[i], kv[i], B.UNROUNDED)
        assert c is None
        assert (B.final_mmdit(W, h, temb[i], B.UNROUNDED) - ref[i]).abs().max().item() < 1e-10


# ---------------------------------------------------------------------------------------------------------------- sensitivity table
def _seq(case, x, cond, i):
    f0 = sum(case["seq_len"][:i])
    n = case["seq_len"][i]
    return x[None, f0:f0 + n].double(), cond[None, f0:f0 + n].double(), n


def _site_a():
    """fn(R, mut) of block 0 and of the final layer at case A's first sequence, from the oracle's float64 input embedding"""
    case, cfg = B.CASE_A, O.DiTConfig(**B.ARCH_A)
    W = B.Weights(synth.dit_state_dict(**B.ARCH_A))
    x, cond, text = B.case_inputs(case["seq_len"], case["nt"], case["vocab"], case["seed"])
    xs, cs, n = _seq(case, x, cond, 0)
    h0 = O.input_embed(W.sd, xs, cs, O.text_embed(W.sd, cfg, text[:1], n, False), False)[0]
    kv, t = case["kv_len"][0], case["time"]
    h1 = B.dit_block(W, 0, h0, B.time_embedding(W, t), kv)
    return (lambda R, mut=(): B.dit_block(W, 0, h0, B.time_embedding(W, t, R), kv, R, mut),
            lambda R, mut=(): B.final_dit(W, h1, B.time_embedding(W, t, R), R, mut))


def _site_c():
    """fn(R, mut) of layer 3 (of 4) at case C's first sequence: its skip is the stream in front of layer 0, the slip takes layer 1's"""
    case, cfg = B.CASE_C, O.UNetTConfig(**B.ARCH_C)
    W = B.Weights(synth.unett_state_dict(**B.ARCH_C))
    x, cond, text = B.case_inputs(case["seq_len"], case["nt"], case["vocab"], case["seed"])
    xs, cs, n = _seq(case, x, cond, 0)
    h0 = O.input_embed(W.sd, xs, cs, O.text_embed(W.sd, cfg, text[:1], n, False), False)[0]
    kv = case["kv_len"][0]
    hs = [torch.cat((B.time_embedding(W, case["time"])[None], h0))]
    hs.append(B.unett_layer(W, 0, 4, hs[0], None, kv))
    hs.append(B.unett_layer(W, 1, 4, hs[1], None, kv))
    hs.append(B.unett_layer(W, 2, 4, hs[2], hs[1], kv))
    return lambda R, mut=(): B.unett_layer(W, 3, 4, hs[3], hs[1] if "skip_wrong_layer" in mut else hs[0], kv, R, mut)


def _site_d():
    """fn(R, mut) -> audio and text stream behind block 0 at case D's second sequence (masked tail, text padded behind 40 tokens)"""
    case, cfg = B.CASE_D, O.MMDiTConfig(**B.ARCH_D)
    W = B.Weights(synth.mmdit_state_dict(**B.ARCH_D))
    x, cond, text = B.case_inputs(case["seq_len"], case["nt"], case["vocab"], case["seed"])
    text[1, case["text_valid"][1]:] = -1
    xs, cs, n = _seq(case, x, cond, 1)
    h0, c0 = O.mmdit_audio_embed(W.sd, xs, cs, False)[0], O.mmdit_text_embed(W.sd, cfg, text[1:2], False)[0]
    kv, t = case["kv_len"][1], case["time"]
    return lambda R, mut=(): torch.cat(B.mmdit_block(W, 0, 3, h0, c0, B.time_embedding(W, t, R), kv, R, mut, c_valid=case["text_valid"][1]))


@pytest.fixture(scope="module")
def sites():
    """per place of MUTATIONS: (fn, exact output, {mode: tolerance = FACTOR x rms(model - exact)})"""
    a_block, a_final = _site_a()
    out = {}
    for where, fn in (("A", a_block), ("A final", a_final), ("C", _site_c()), ("D", _site_d())):
        exact = fn(B.EXACT)
        # the final norm and proj_out stay split bf16 in mixed mode: the mode-2 model in both modes
        tol = {mode: FACTOR * _rms(fn(B.MODE2 if where == "A final" else B.MODES[mode]), exact) for mode in (2, 3)}
        out[where] = (fn, exact, tol)
    return out


def sensitivity(fn, exact, tol, entries):
    """[(mutation, distance, {mode: distance / tolerance})] of the entries' mutations applied to fn"""
    rows = []
    for name in entries:
        d = _rms(fn(B.EXACT, (name,)), exact)
        rows.append((name, d, {mode: d / t for mode, t in tol.items()}))
    return rows


def test_sensitivity_table(sites):
    """Every mutation a mode claims moves the block output by at least MARGIN x that mode's tolerance; gelu_exact and unbiased_variance stay
    below MARGIN x mode 3's; eps 1e-5 is below every tolerance itself."""
    bad = []
    for name, where, modes in MUTATIONS:
        fn, exact, tol = sites[where]
        (_, d, ratio), = sensitivity(fn, exact, tol, [name])
        print(f"[sensitivity] {name:30s} at {where:8s}: rms {d:.3e}   / tolerance: mode 2 {ratio[2]:8.2f} (tol {tol[2]:.2e})   "
              f"mode 3 {ratio[3]:8.2f} (tol {tol[3]:.2e})")
        for mode in (2, 3):
            if mode in modes and ratio[mode] < MARGIN:
                bad.append((name, where, mode, ratio[mode]))
            if mode == 3 and (name, where) in BELOW_MODE3 and ratio[3] >= MARGIN:
                bad.append((name, where, "no longer below mode 3's floor", ratio[3]))
        if not modes and max(ratio.values()) >= 1.0:
            bad.append((name, where, "listed as undetectable", ratio))
    assert not bad, bad
