"""float64 references of ONE transformer block (or the final norm + proj_out) of each backbone, one sequence at a time, shared by
tests/test_block_reference.py (CPU, which pins them against the oracle's whole forwards) and tests/test_gpu_blocks.py (GPU).

Every function takes a `Rounding`: one callable per place where the library rounds an operand (csrc/f5hip.hip: run_adaln, block_qkv,
launch_attention, block_out, block_ff, forward_unett_layers, run_proj_out).  EXACT is THE reference the GPU is compared with; MODE2 and MODE3
put the library's operand formats into the same arithmetic and exist only to derive tolerances (`model_err`), never to be compared with.
`mut` names deliberate slips (MUTATIONS in tests/test_block_reference.py) for the sensitivity table."""
import math

import torch
import torch.nn.functional as F

from oracle import dit_oracle as O
from row_ops_ref import fmt_f16, fmt_split

Q_SCALE = 0.125 * math.log2(math.e)   # csrc/common.h F5_Q_SCALE: the QKV epilogue folds the softmax scale 1/8 and log2(e) into q


def ident(y):
    return y


def split(y):
    """hi + lo split bf16 of the fp32 value of y"""
    return fmt_split(y).double()


def f16(y):
    """saturated fp16 of the fp32 value of y"""
    return fmt_f16(y).double()


class Rounding:
    """ln: block norm output (operand of QKV and FF1);  qkv: q (after its log2(e) / 8 scale), k and v;  p: the softmax numerators
    exp(s - offset), which also make the row sum;  ao: attention output;  ff1: FF1 output;  w: the four block weights;
    state / w_state: operands / weights of the GEMMs outside the blocks' four -- the time MLP and AdaLN linears, UNetT's skip projection
    (forward_unett_layers: split_rows_kernel writes [x || skip] as split bf16 planes, wskip is packed without the fp16 flag, in every mode),
    the final norm's output and proj_out."""
    SITES = ("ln", "qkv", "p", "ao", "ff1", "w", "state", "w_state")

    def __init__(self, name, **sites):
        self.name = name
        for s in self.SITES:
            setattr(self, s, sites.pop(s, ident))
        assert not sites, sites


UNROUNDED = Rounding("unrounded")                 # the oracle's arithmetic (chain check)
EXACT = Rounding("exact", qkv=f16)                # the library's operand contract in every mode: fp16 q / k / v
MODE2 = Rounding("mode2", ln=split, qkv=f16, p=f16, ao=split, ff1=split, w=split, state=split, w_state=split)
MODE3 = Rounding("mode3", ln=f16, qkv=f16, p=f16, ao=f16, ff1=f16, w=f16, state=split, w_state=split)
MODES = {2: MODE2, 3: MODE3}


class Weights:
    """A state_dict in float64, with its tensors in a Rounding site's format on demand (cached)."""

    def __init__(self, sd):
        self.sd = {k: v.double() for k, v in sd.items()}
        self._cache = {}

    def get(self, key, fmt=ident):
        if fmt is ident:
            return self.sd[key]
        if (key, fmt) not in self._cache:
            self._cache[key, fmt] = fmt(self.sd[key])
        return self._cache[key, fmt]


def _lin(W, key, a, w_fmt, bias=True):
    return F.linear(a, W.get(key + "weight", w_fmt), W.sd[key + "bias"] if bias else None)


# ------------------------------------------------------------------------------------------------------------ time path
def time_embedding(W, t, R=EXACT):
    """TimestepEmbedding of the scalar time t, [dim].  The sinusoid's angle 1000 t f_k is formed in fp32, as the reference model does with its
    fp32 time and as the library's host code does; the MLP runs in float64 on the `state` formats."""
    s = O.sinus_time_embed(torch.tensor([t], dtype=torch.float32)).double()
    p = "transformer.time_embed.time_mlp."
    h = F.silu(_lin(W, p + "0.", R.state(s), R.w_state))
    return _lin(W, p + "2.", R.state(h), R.w_state)[0]


def adaln(W, key, temb, R):
    """One AdaLN linear on silu(temb): the modulation vectors of a block (6 dim) or of a (scale, shift) norm (2 dim)."""
    return _lin(W, key, R.state(F.silu(temb))[None], R.w_state)[0]


# ------------------------------------------------------------------------------------------------------------ pieces
def _norm(x, mut, rms=False):
    """LayerNorm without affine (eps 1e-6), or x-transformers' RMSNorm without its gain: x / max(|x|, 1e-12) sqrt(dim)"""
    d = x.shape[-1]
    if rms:
        return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12) * math.sqrt(d - 1 if "unbiased_variance" in mut else d)
    var = x.var(dim=-1, unbiased="unbiased_variance" in mut, keepdim=True)
    return (x - x.mean(dim=-1, keepdim=True)) / torch.sqrt(var + (1e-5 if "eps_1e-5" in mut else 1e-6))


def _rotary(t, pos, mut):
    """Rotary embedding at the rows' positions on the leading 64 features (head 0 only: SURVEY Appendix B1)"""
    fr = O.rotary_freqs(int(pos.max()) + 1)[0][pos]
    if "rotary_every_head" in mut:
        n, d = t.shape
        return O.apply_rotary(t.view(n, d // 64, 64), fr[:, None, :]).reshape(n, d)
    return O.apply_rotary(t, fr)


def attend(q, k, v, key_ok, R):
    """softmax(q k^T / 8) v per head of 64 over the keys with key_ok, on the Rounding's q / k / v / p formats"""
    heads = q.shape[1] // 64
    hd = lambda t: t.view(t.shape[0], heads, 64).transpose(0, 1)
    qs, ks, vs = hd(R.qkv(q * Q_SCALE) * math.log(2.0)), hd(R.qkv(k)), hd(R.qkv(v))
    s = (qs @ ks.transpose(1, 2)).masked_fill(~key_ok[None, None, :], float("-inf"))
    e = R.p(torch.exp(s - s.amax(dim=-1, keepdim=True)))
    o = (e @ vs) / e.sum(dim=-1, keepdim=True)
    return o.transpose(0, 1).reshape(q.shape[0], heads * 64)


def _qkv(W, p, sfx, h, pos, R, mut):
    q, k, v = (_lin(W, f"{p}{nm}{sfx}.", h, R.w) for nm in ("to_q", "to_k", "to_v"))
    return _rotary(q, pos, mut), _rotary(k, pos, mut), v


def _self_attention(W, p, h, kv_len, R, mut):
    """AttnProcessor on the normed rows h [n, dim] at positions 0 .. n - 1: keys >= kv_len masked, output rows >= kv_len zeroed"""
    n = h.shape[0]
    keep = torch.arange(n) < kv_len
    q, k, v = _qkv(W, p, "", h, torch.arange(n), R, mut)
    o = _lin(W, p + "to_out.0.", R.ao(attend(q, k, v, keep, R)), R.w, bias="no_out_bias" not in mut)
    return o * keep[:, None]


def _ff(W, p, h, R, mut):
    f = _lin(W, p + "0.0.", h, R.w)
    f = F.gelu(f) if "gelu_exact" in mut else F.gelu(f, approximate="tanh")
    return _lin(W, p + "2.", R.ff1(f), R.w)


def _chunks6(m, mut):
    sh_a, sc_a, g_a, sh_m, sc_m, g_m = m.chunk(6)
    if "gates_exchanged" in mut:
        g_a, g_m = g_m, g_a
    if "scale_shift_exchanged" in mut:
        sh_a, sc_a, sh_m, sc_m = sc_a, sh_a, sc_m, sh_m
    return sh_a, sc_a, g_a, sh_m, sc_m, g_m


# ------------------------------------------------------------------------------------------------------------ blocks
def dit_block(W, l, x, temb, kv_len, R=EXACT, mut=()):
    """DiTBlock l on one sequence x [n, dim] -> [n, dim]"""
    p = f"transformer.transformer_blocks.{l}."
    sh_a, sc_a, g_a, sh_m, sc_m, g_m = _chunks6(adaln(W, p + "attn_norm.linear.", temb, R), mut)
    x = x + g_a * _self_attention(W, p + "attn.", R.ln(_norm(x, mut) * (1 + sc_a) + sh_a), kv_len, R, mut)
    return x + g_m * _ff(W, p + "ff.ff.", R.ln(_norm(x, mut) * (1 + sc_m) + sh_m), R, mut)


def unett_layer(W, l, depth, x, skip, kv_len, R=EXACT, mut=()):
    """UNetT layer l on one sequence x [1 + n, dim] with the time token at row 0 (rotary position 0, never masked; kv_len counts frames);
    skip: the stream saved in front of layer depth - 1 - l for l >= depth / 2, else None."""
    p = f"transformer.layers.{l}."
    assert (skip is not None) == (l >= depth // 2)
    if skip is not None:
        x = F.linear(R.state(torch.cat((x, skip), dim=-1)), W.get(p + "0.weight", R.w_state))
    x = x + _self_attention(W, p + "2.", R.ln(_norm(x, mut, rms=True) * W.sd[p + "1.g"]), kv_len + 1, R, mut)
    return x + _ff(W, p + "4.ff.", R.ln(_norm(x, mut, rms=True) * W.sd[p + "3.g"]), R, mut)


def mmdit_block(W, l, depth, x, c, temb, kv_len, R=EXACT, mut=(), c_valid=None):
    """MMDiTBlock l on one sequence: audio rows x [n, dim], text rows c [nt, dim] -> (x', c'); c' is None behind the last
    (context-pre-only) block.  Joint attention over [audio keys ; text keys]: audio keys >= kv_len masked, text keys never
    (mutation text_keys_masked: text keys >= c_valid masked too)."""
    p = f"transformer.transformer_blocks.{l}."
    last = l == depth - 1
    n, nt = x.shape[0], c.shape[0]
    mc = adaln(W, p + "attn_norm_c.linear.", temb, R)
    if last:
        c_sc_a, c_sh_a = mc.chunk(2)          # AdaLayerNormZero_Final: (scale, shift)
    else:
        c_sh_a, c_sc_a, c_g_a, c_sh_m, c_sc_m, c_g_m = _chunks6(mc, mut)
    x_sh_a, x_sc_a, x_g_a, x_sh_m, x_sc_m, x_g_m = _chunks6(adaln(W, p + "attn_norm_x.linear.", temb, R), mut)
    hx = R.ln(_norm(x, mut) * (1 + x_sc_a) + x_sh_a)
    hc = R.ln(_norm(c, mut) * (1 + c_sc_a) + c_sh_a)
    pa = p + "attn."
    q, k, v = (torch.cat(t) for t in zip(_qkv(W, pa, "", hx, torch.arange(n), R, mut), _qkv(W, pa, "_c", hc, torch.arange(nt), R, mut)))
    keep = torch.arange(n) < kv_len
    c_ok = torch.arange(nt) < (c_valid if "text_keys_masked" in mut else nt)
    o = R.ao(attend(q, k, v, torch.cat((keep, c_ok)), R))
    x = x + x_g_a * (_lin(W, pa + "to_out.0.", o[:n], R.w, bias="no_out_bias" not in mut) * keep[:, None])
    if last:
        c = None
    else:
        c = c + c_g_a * _lin(W, pa + "to_out_c.", o[n:], R.w, bias="no_out_bias" not in mut)
        c = c + c_g_m * _ff(W, p + "ff_c.ff.", R.ln(_norm(c, mut) * (1 + c_sc_m) + c_sh_m), R, mut)
    x = x + x_g_m * _ff(W, p + "ff_x.ff.", R.ln(_norm(x, mut) * (1 + x_sc_m) + x_sh_m), R, mut)
    return x, c


# ------------------------------------------------------------------------------------------------------------ final norm + proj_out
def final_dit(W, x, temb, R=EXACT, mut=()):
    """AdaLayerNormZero_Final (scale, shift) + proj_out on one sequence x [n, dim] -> [n, mel]"""
    scale, shift = adaln(W, "transformer.norm_out.linear.", temb, R).chunk(2)
    if "final_scale_shift_exchanged" in mut:
        scale, shift = shift, scale
    return _lin(W, "transformer.proj_out.", R.state(_norm(x, mut) * (1 + scale) + shift), R.w_state)


final_mmdit = final_dit   # the same two modules under the same names (mmdit.py:112-113)


def final_unett(W, x, R=EXACT, mut=()):
    """RMSNorm + proj_out on one sequence x [1 + n, dim]; the time token's row is dropped -> [n, mel]"""
    h = R.state(_norm(x[1:], mut, rms=True) * W.sd["transformer.norm_out.g"])
    return _lin(W, "transformer.proj_out.", h, R.w_state)


# ------------------------------------------------------------------------------------------------------------ statistics
def row_stats(err):
    """(overall rms, worst row's rms) of an error [rows, width]"""
    r = err.double().pow(2).mean(dim=-1)
    return r.mean().sqrt().item(), r.max().sqrt().item()


# ------------------------------------------------------------------------------------------------------------ the GPU cases' inputs
ARCH_A = dict(dim=1024, depth=3, heads=16, ff_mult=2)                        # DiT, ragged one-utterance shapes
ARCH_B = dict(dim=1024, depth=2, heads=16, ff_mult=2)                        # DiT, batch-mode shapes
ARCH_C = dict(dim=1024, depth=4, heads=16, ff_mult=4)                        # UNetT
ARCH_D = dict(dim=512, depth=3, heads=8, ff_mult=2, text_num_embeds=100)     # MMDiT


def case_inputs(seq_len, nt, vocab, seed):
    """Packed frames x, cond [sum(seq_len), 100] and text ids [len(seq_len), nt] of one ragged call"""
    g = torch.Generator().manual_seed(seed)
    frames = sum(seq_len)
    x = torch.randn(frames, 100, generator=g)
    cond = torch.randn(frames, 100, generator=g)
    text = torch.randint(0, vocab, (len(seq_len), nt), generator=g)
    return x, cond, text


CASE_A = dict(seq_len=(385, 129, 1, 255), kv_len=(385, 129, 1, 200), time=0.3, drop_audio=(0, 1, 0, 0), drop_text=(0, 0, 1, 0), nt=300,
              vocab=2545, seed=81)
CASE_B = dict(seq_len=tuple(300 + (i * 37) % 151 for i in range(26)), time=0.55, nt=120, vocab=2545, seed=82)
CASE_C = dict(seq_len=(200, 77), kv_len=(200, 60), time=0.7, nt=90, vocab=2545, seed=83)
CASE_D = dict(seq_len=(300, 300), kv_len=(300, 233), time=0.6, nt=61, vocab=100, seed=84, text_valid=(61, 40))
