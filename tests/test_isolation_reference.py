"""CPU: the comparison of tests/test_gpu_isolation.py has teeth, and the finite-value "equals alone" checks do not.

The oracle's DiT blocks (float64) over a sequence B with ONE neighbour row behind it, the neighbour kept out of B's attention by the key mask.
The deliberate slip lets the neighbour row through the mask by MULTIPLICATION: softmax over all keys, probabilities times the 0 / 1 mask,
renormalised -- the same function of finite inputs as masking the scores, up to rounding.  With a finite neighbour the slip passes an
"equals alone" check at 1e-3 (the suite's mel bound) by many orders of magnitude; with a NaN neighbour it destroys every row of B."""
import pytest
import torch
import torch.nn.functional as F

from oracle import dit_oracle as O
from tts_indic_server_f5_amd import synth

TINY = dict(dim=128, depth=2, heads=2, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=40)   # the tiny config of tests/test_gpu_dit.py
N = 41


def _sdpa_mask_by_multiplication(q, k, v, attn_mask=None, dropout_p=0.0, is_causal=False):
    """scaled_dot_product_attention with the mask applied to the probabilities instead of the scores"""
    p = torch.softmax(q @ k.transpose(-1, -2) / q.shape[-1] ** 0.5, dim=-1)
    if attn_mask is not None:
        p = p * attn_mask.to(p.dtype)
        p = p / p.sum(dim=-1, keepdim=True)
    return p @ v


def _blocks(sd, cfg, h, t, mask):
    """DiT.forward behind the input embedding (dit_oracle.dit_forward): the blocks, the final modulation, proj_out"""
    rope = O.rotary_freqs(h.shape[1], cfg.dim_head)
    for i in range(cfg.depth):
        h = O.dit_block(sd, f"transformer.transformer_blocks.{i}.", cfg, h, t, mask, rope)
    s = F.linear(F.silu(t), sd["transformer.norm_out.linear.weight"], sd["transformer.norm_out.linear.bias"])
    scale, shift = s.chunk(2, dim=1)
    h = F.layer_norm(h, (cfg.dim,), eps=1e-6) * (1 + scale)[:, None, :] + shift[:, None, :]
    return F.linear(h, sd["transformer.proj_out.weight"], sd["transformer.proj_out.bias"])


@pytest.fixture(scope="module")
def site():
    """(sd, cfg, B's embedded rows [1, N, D], time embedding, B alone through the blocks)"""
    cfg = O.DiTConfig(**TINY)
    sd = {k: v.double() for k, v in synth.dit_state_dict(**TINY).items()}
    g = torch.Generator().manual_seed(17)
    x, cond = torch.randn(1, N, 100, generator=g, dtype=torch.float64), torch.randn(1, N, 100, generator=g, dtype=torch.float64)
    text = torch.randint(0, 40, (1, 12), generator=g)
    h = O.input_embed(sd, x, cond, O.text_embed(sd, cfg, text, N, False), False)
    t = O.time_embed(sd, torch.tensor([0.37], dtype=torch.float64))
    return sd, cfg, h, t, _blocks(sd, cfg, h, t, None)


def _with_neighbour(site, fill, monkeypatch, slip):
    """B's rows of the blocks' output with one neighbour row (a finite random row, or NaN) behind B, masked as a key"""
    sd, cfg, h, t, _ = site
    g = torch.Generator().manual_seed(18)
    row = torch.randn(1, 1, cfg.dim, generator=g, dtype=torch.float64) if fill is None else torch.full((1, 1, cfg.dim), fill, dtype=torch.float64)
    mask = torch.arange(N + 1)[None] < N
    if slip:
        monkeypatch.setattr(O.F, "scaled_dot_product_attention", _sdpa_mask_by_multiplication)
    return _blocks(sd, cfg, torch.cat([h, row], dim=1), t, mask)[:, :N]


def test_masked_finite_neighbour_equals_alone(site, monkeypatch):
    """The oracle's own masking with a finite neighbour: B equals B alone up to float64 rounding (another key count: the softmax sums
    associate differently).  No NaN case here: torch's scaled_dot_product_attention masks the SCORES by selection but still multiplies the
    masked key's value row by its probability of exactly 0, so a NaN value row gets through it too -- the reference of the GPU test is
    therefore never "the oracle with a poisoned neighbour" but the same call with a finite one."""
    got = _with_neighbour(site, None, monkeypatch, slip=False)
    assert torch.isfinite(got).all()
    assert (got - site[4]).abs().max().item() < 1e-12


def test_masking_by_multiplication_passes_finite_equals_alone_and_fails_the_nan_neighbour(site, monkeypatch):
    alone = site[4]
    finite = _with_neighbour(site, None, monkeypatch, slip=True)
    rms = (finite - alone).pow(2).mean().sqrt().item()
    print(f"[teeth] mask by multiplication, finite neighbour: rms vs alone {rms:.3e} (the finite-value check's bound: 1e-3)")
    assert rms < 1e-3                                    # the finite-value check lets the slip through ...
    poisoned = _with_neighbour(site, float("nan"), monkeypatch, slip=True)
    assert not torch.equal(poisoned, finite)             # ... the NaN-neighbour check does not:
    assert torch.isnan(poisoned).any(dim=-1).all()       # every row of B is gone
