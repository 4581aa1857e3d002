"""float64 references of every stage of the Vocos decoder (csrc/vocos.h: vocos_decode_items), one item at a time, shared by
tests/test_vocos_reference.py (CPU, which pins them against oracle/vocos_oracle.py and shows what the per-stage rule catches),
tests/test_gpu_vocos_stages.py and the whole-decode tests of tests/test_gpu_vocos.py / tests/test_gpu_stream.py (GPU).

Rows are frames: the residual stream is x [T, dim], the head output y [T, n_fft + 2] (log-magnitude | phase), the windowed frames
fw [T, n_fft].  Every backbone stage takes a `Formats`: one callable per place where the library rounds.  EXACT is THE reference the GPU is
compared with; MODES[gemm_planes] put the library's operand formats into the same arithmetic and exist only to derive tolerances, never to
be compared with.  `mut` names deliberate slips (MUTATIONS in tests/test_vocos_reference.py) for the sensitivity table."""
import math

import torch
import torch.nn.functional as F

from block_ref import Weights, ident, row_stats, split  # noqa: F401  (re-exported: the tests take them from here)

N_FFT, HOP, CLIP = 1024, 256, 100.0


def bf16(y):
    """one bf16 plane of the fp32 value of y (gemm_planes = 1: the GEMMs read the hi plane only)"""
    return y.float().bfloat16().double()


def f32(y):
    """an fp32 store"""
    return y.float().double()


class Formats:
    """a: the A operands of the five GEMM sites (mel rows, the block norm's output, the hidden activations, the final norm's output);
    w: their weights;  store: what the library keeps in fp32 between kernels (embed conv output, every LayerNorm written in place, the
    block output, the head output, the windowed frames and the wave)."""
    SITES = ("a", "w", "store")

    def __init__(self, name, **sites):
        self.name = name
        for s in self.SITES:
            setattr(self, s, sites.pop(s, ident))
        assert not sites, sites


EXACT = Formats("exact")                                  # the oracle's arithmetic; Vocos has no operand contract below fp32
MODES = {2: Formats("split_bf16", a=split, w=split, store=f32), 1: Formats("bf16", a=bf16, w=bf16, store=f32)}


def _site(R, mut, name):
    """(a, w) formats of GEMM `name` ("pw1" / "pw2"): the mutation <name>_a_lo_lost / <name>_w_lo_lost leaves that operand its hi plane only"""
    return (bf16 if f"{name}_a_lo_lost" in mut else R.a), (bf16 if f"{name}_w_lo_lost" in mut else R.w)


def _ln(x, w, b, mut=()):
    return F.layer_norm(x, (x.shape[-1],), w, b, eps=1e-5 if "eps_1e-5" in mut else 1e-6)


def _conv7(x, mut=(), before=None, after=None):
    """The 7 shifted copies [7, T, C] of the rows x [T, C] that a k = 7, pad = 3 convolution over the frame axis multiplies: tap k holds
    row t + k - 3, zero outside the item.  Slips: replicate_padding repeats the item's first / last row; reads_neighbours takes the rows
    `before` / `after` [3, C] (the neighbouring items' in the packed order) instead of zeros."""
    T = x.shape[0]
    if "replicate_padding" in mut:
        lo, hi = x[:1].expand(3, -1), x[-1:].expand(3, -1)
    elif "reads_neighbours" in mut:
        lo, hi = before, after
    else:
        lo = hi = x.new_zeros(3, x.shape[1])
    p = torch.cat((lo, x, hi))
    return torch.stack([p[k:k + T] for k in range(7)])


# ------------------------------------------------------------------------------------------------------------ backbone stages
def embed(W, mel, R=EXACT, mut=()):
    """mel [C, T] of one item -> x [T, dim]: Conv1d(C -> dim, k 7, zero padding at the item's bounds) as a GEMM over 7 taps x C with the
    operand formats, fp32 bias, stored; then backbone.norm (eps 1e-6), stored in place."""
    taps = _conv7(R.a(mel.double().t()), mut)                          # [7, T, C]
    w = W.get("backbone.embed.weight", R.w)                            # [dim, C, 7]
    x = torch.einsum("ktc,dck->td", taps, w) + W.sd["backbone.embed.bias"]
    return R.store(_ln(R.store(x), W.sd["backbone.norm.weight"], W.sd["backbone.norm.bias"], mut))


def block(W, l, x, R=EXACT, mut=(), before=None, after=None):
    """ConvNeXt block l on one item's stream x [T, dim] -> [T, dim]: depthwise k = 7 (zero padding) + bias and LayerNorm on the fp32
    stream, written as operand planes; pwconv1 + bias, erf GELU, written as operand planes; pwconv2 + bias, x gamma, + x, stored."""
    p = f"backbone.convnext.{l}."
    x = x.double()
    y = torch.einsum("ktc,ck->tc", _conv7(x, mut, before, after), W.sd[p + "dwconv.weight"][:, 0, :])
    if "no_dwconv_bias" not in mut:
        y = y + W.sd[p + "dwconv.bias"]
    a1, w1 = _site(R, mut, "pw1")
    a2, w2 = _site(R, mut, "pw2")
    h = F.linear(a1(_ln(y, W.sd[p + "norm.weight"], W.sd[p + "norm.bias"], mut)), W.get(p + "pwconv1.weight", w1), W.sd[p + "pwconv1.bias"])
    h = F.gelu(h, approximate="tanh") if "tanh_gelu" in mut else F.gelu(h)
    o = F.linear(a2(h), W.get(p + "pwconv2.weight", w2), None if "no_pwconv2_bias" in mut else W.sd[p + "pwconv2.bias"])
    if "no_gamma" not in mut:
        o = o * W.sd[p + "gamma"]
    return R.store(x + o)


def head(W, x, R=EXACT, mut=()):
    """backbone.final_layer_norm as operand planes, then head.out: x [T, dim] -> y [T, n_fft + 2], stored"""
    h = R.a(_ln(x.double(), W.sd["backbone.final_layer_norm.weight"], W.sd["backbone.final_layer_norm.bias"], mut))
    return R.store(F.linear(h, W.get("head.out.weight", R.w), W.sd["head.out.bias"]))


# ------------------------------------------------------------------------------------------------------------ iSTFT head
def hann(periodic=True, dtype=torch.float64):
    return torch.hann_window(N_FFT, periodic=periodic, dtype=dtype)


def _irfft_packed(spec):
    """irfft(n_fft) by one complex inverse FFT of half the length on z[m] = x[2 m] + i x[2 m + 1] -- a transform that relies on the
    spectrum being Hermitian, so it is right only if the imaginary parts of DC and Nyquist are dropped first (the slip nyquist_imag_kept:
    every sample then moves by -Im X[n_fft / 2] / n_fft)."""
    h = N_FFT // 2
    xk, xm = spec[:, :h], spec[:, 1:].flip(-1).conj()                  # X[k], conj(X[h - k]) = X[k + h] of a Hermitian spectrum, k < h
    rot = torch.exp(2j * math.pi * torch.arange(h, dtype=torch.float64) / N_FFT)
    z = torch.fft.ifft((xk + xm) / 2 + 1j * rot * (xk - xm) / 2, dim=-1)
    return torch.stack((z.real, z.imag), dim=-1).reshape(spec.shape[0], N_FFT)


def frames(y, mut=(), dtype=torch.float64):
    """ISTFTHead per frame: y [T, n_fft + 2] -> fw [T, n_fft] = irfft(min(exp(mag), 100) e^{i phase}) x periodic Hann; the imaginary
    parts of DC and Nyquist are ignored.  dtype float32 is the reference implementation's own arithmetic (torch's fp32 exp / cos / sin and
    its fp32 FFT), the yardstick of the frame test -- not the kernel's."""
    y = y.to(dtype)
    mag, ph = torch.exp(y[:, :N_FFT // 2 + 1]), y[:, N_FFT // 2 + 1:]
    if "no_clip" not in mut:
        mag = mag.clamp(max=CLIP)
    spec = torch.complex(mag * torch.cos(ph), mag * torch.sin(ph))
    if "nyquist_imag_kept" in mut:
        spec[:, 0] = spec[:, 0].real + 0j                              # DC alone dropped
        x = _irfft_packed(spec)
    else:
        x = torch.fft.irfft(spec, n=N_FFT, dim=-1)                     # c2r: ignores both
    return x * hann("symmetric_hann" not in mut, dtype)


def ola_terms(fw, mut=()):
    """Overlap-add of one item's windowed frames fw [T, n_fft] at hop 256, centre-trimmed to hop (T - 1) samples:
    (sum of the frames' terms, sum of their magnitudes, window envelope), each [hop (T - 1)]."""
    T = fw.shape[0]
    fw = fw.double()
    w = hann() if "envelope_without_squares" in mut else hann() ** 2
    fold = lambda cols: F.fold(cols.t()[None], (1, HOP * (T - 1) + N_FFT), (1, N_FFT), stride=(1, HOP))[0, 0, 0]
    trim = slice(N_FFT // 2, N_FFT // 2 + HOP * (T - 1))
    return fold(fw)[trim], fold(fw.abs())[trim], fold(w.expand(T, -1))[trim]


def ola(fw, mut=()):
    """torch.istft's tail (center = True): overlap-add / window envelope -> wave [hop (T - 1)]"""
    val, _, env = ola_terms(fw, mut)
    return val / env


# ------------------------------------------------------------------------------------------------------------ chained
def backbone(W, mel, R=EXACT, num_layers=8, mut=()):
    """[x behind embed + norm, behind block 0, ..., behind block num_layers - 1] of one item mel [C, T]"""
    xs = [embed(W, mel, R, mut)]
    for l in range(num_layers):
        xs.append(block(W, l, xs[-1], R, mut))
    return xs


def decode(W, mel, R=EXACT, num_layers=8, mut=()):
    """The whole decode of one item mel [C, T] -> wave [hop (T - 1)] with the formats R in every stage (the wave `model` of the
    whole-decode tests; with EXACT the float64 oracle)."""
    return R.store(ola(R.store(frames(head(W, backbone(W, mel, R, num_layers, mut)[-1], R, mut), mut)), mut))


def decode_errors(W, mels, got, planes):
    """Whole decode of the items mels [C, T_i] against the GPU waves `got`: (max, rms) of GPU - exact and of model - exact over all
    items, model = decode in the formats of gemm_planes = `planes`."""
    exact = torch.cat([decode(W, m) for m in mels])
    model = torch.cat([decode(W, m, MODES[planes]) for m in mels])
    g, m = torch.cat([w.reshape(-1) for w in got]).double().cpu() - exact, model - exact
    return (g.abs().max().item(), g.pow(2).mean().sqrt().item()), (m.abs().max().item(), m.pow(2).mean().sqrt().item())
