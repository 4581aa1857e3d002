"""Shared by tests/test_gpu_mel_levels.py (GPU), tests/test_mel_bound_reference.py (CPU, which fixes the constants below) and the two older
mel tests: test signals for the mel front-ends (mel_frame_kernel, csrc/vocos.h), their float64 references -- the oracles of oracle/ run
unchanged in float64 -- and a bound on the clamped mel energies in the linear domain, which stays meaningful where bins sit at or near
log(clamp(., 1e-5)) and the log magnifies fp32 FFT rounding without limit.  No device code is imported here."""
import math

import torch
import torch.nn.functional as F

from oracle import bigvgan_oracle as B
from oracle import vocos_oracle as V

CLAMP = 1e-5
LOG_CLAMP = math.log(CLAMP)
NW = 24_000          # the longest signal: 94 frames at hop 256
FRONTS = ("vocos", "bigvgan")
PAD_HOP = {"vocos": lambda n_fft, hop: n_fft // 2, "bigvgan": lambda n_fft, hop: (n_fft - hop) // 2}


# ------------------------------------------------------------------------------------------------ float64 references
def float64(fn, *args, **kw):
    """Run an oracle function unchanged in float64: its windows and filterbanks take torch's default dtype."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return fn(*args, **kw)
    finally:
        torch.set_default_dtype(old)


def bigvgan_mel_float64(wave, **kw):
    """The BigVGAN oracle's mel front-end in float64: its window takes torch's default dtype, and its Slaney filterbank (returned as fp32,
    the values the device tables hold too) is widened to float64 before the product."""
    slaney = B.librosa_slaney_mel
    B.librosa_slaney_mel = lambda *a, **k: slaney(*a, **k).double()
    try:
        return float64(B.bigvgan_mel_spectrogram, wave.double(), **kw)
    finally:
        B.librosa_slaney_mel = slaney


def vocos_mel_float64(wave, **kw):
    return float64(V.vocos_mel_spectrogram, wave.double(), **kw)


# geometries other than the default 100 channels / 24 kHz / hop 256, as keyword arguments of ref64 / oracle32
GEOMETRIES = {
    "mels80": dict(n_mels=80), "mels128": dict(n_mels=128), "mels256": dict(n_mels=256),      # 256: every thread of the block owns a channel
    "sr16000": dict(sr=16000), "sr22050": dict(sr=22050), "sr44100": dict(sr=44100),
    "hop128": dict(hop=128), "hop512": dict(hop=512),
}


def _geom(n_fft=1024, hop=256, n_mels=100, sr=24000):
    return dict(n_fft=n_fft, hop=hop, n_mels=n_mels, sr=sr)


def ref64(front, wave, **geom):
    """float64 log-mel of `front` ("vocos" / "bigvgan") for wave [b, nw]; geom: n_fft, hop, n_mels, sr."""
    return (vocos_mel_float64 if front == "vocos" else bigvgan_mel_float64)(wave, **_geom(**geom))


def oracle32(front, wave, **geom):
    """The fp32 oracle itself, as committed."""
    return (V.vocos_mel_spectrogram if front == "vocos" else B.bigvgan_mel_spectrogram)(wave.float(), **_geom(**geom))


def zero_frames(front, wave, n_fft=1024, hop=256):
    """[b, T] bool: the frames of `front` whose n_fft reflect-padded input samples are all exactly zero."""
    pad = PAD_HOP[front](n_fft, hop)
    w = F.pad(wave.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    return (w.unfold(-1, n_fft, hop) == 0).all(-1)


# ------------------------------------------------------------------------------------------------ signals
def _tones(g, n, amp):
    """synth.ref_audio's eight tones (80 Hz .. 4 kHz at 24 kHz, random phases) without its noise, fp64."""
    f = 80.0 + (4000.0 - 80.0) * torch.rand(8, generator=g)
    ph = 2 * math.pi * torch.rand(8, generator=g)
    t = torch.arange(n, dtype=torch.float64)
    return amp * torch.sin(2 * math.pi * f.double()[:, None] * t[None, :] / 24000.0 + ph.double()[:, None]).sum(0) / math.sqrt(8)


def signals(seed=4242):
    """name -> fp32 wave [1, n], n <= 24 000, deterministic.  `control` keeps every bin far above the clamp; the others reach it, or the
    fp32 rounding floor under a loud component, or the reflect padding, in the ways real reference clips do."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = NW
    tones = _tones(g, n, 0.15)
    noise = 0.01 * torch.randn(n, generator=g, dtype=torch.float64)
    t = torch.arange(n, dtype=torch.float64)
    out = {}
    out["control"] = tones + noise                                   # 1: tones + 0.01 noise, as synth.ref_audio
    out["tones"] = tones                                             # 2: nothing above 4 kHz but leakage
    out["tones_1e-3"] = tones * (1e-3 / 0.15)                        # 3: the same at amplitude 1e-3
    half = tones.clone()
    half[n // 2 + 100:] = 0.0                                        # 4: exact zeros from sample 12 100 (inside a frame, not on a hop)
    out["tones_then_zeros"] = half
    out["loud_low_tone"] = 0.9 * torch.sin(2 * math.pi * 217.0 * t / 24000.0 + 0.3)   # 5: worst dynamic range
    out["zeros"] = torch.zeros(n, dtype=torch.float64)               # 6
    imp = torch.zeros(n, dtype=torch.float64)
    imp[12_345] = 1.0                                                # 7: in four or five frames of 94; flat spectrum
    out["impulse"] = imp
    out["dc_plus_tones"] = 0.5 + tones * (0.02 / 0.15)               # 8: DC offset 0.5 and small tones
    out["clipped"] = (tones * (2.5 / 0.15)).clamp(-1.0, 1.0)         # 9: hard-clipped to +-1.0
    edge = tones * (0.05 / 0.15)                                     # 10: a step at sample 1 and at sample n - 2: padding that repeats
    edge[0] = 0.8                                                    #     or drops an end sample changes the edge frames
    edge[n - 1] = -0.8
    out["edge_steps"] = edge
    out["faint_noise"] = 1e-5 * torch.randn(n, generator=g, dtype=torch.float64)      # 11: magnitudes ~2e-4, near BigVGAN's sqrt(1e-9)
    out["dc_tones_noise"] = 0.5 + tones * (0.02 / 0.15) + 30.0 * noise      # 12: signal 8 under 0.3 noise: every bin 1e3 above the clamp
    out["tones_513"] = tones[:513]                                   # the Vocos front-end's shortest wave
    out["tones_1024"] = tones[:1024]                                 # the BigVGAN front-end's shortest wave
    return {k: v.float()[None, :].contiguous() for k, v in out.items()}


CONTROL = "control"


def signals_for(front):
    s = signals()
    if front == "bigvgan":
        del s["tones_513"]           # below its minimum of n_fft samples
    return s


# ------------------------------------------------------------------------------------------------ the bound
# |E_got - E_ref| <= r E_ref + a P_t, E = exp(log-mel) the clamped energies and P_t the largest E_ref of frame t.  Both constants come from
# the fp32 oracle against the float64 oracle on signals() at the default geometry (tests/test_mel_bound_reference.py measures and asserts
# them), never from the kernel; the factor 4 covers the kernel's other summation orders (radix-2 LDS FFT, sequential 513-term filterbank
# sum), whose errors are of the same order eps log N as torch's FFT and matmul.
#   r = 4 max |E32 - E64| / E64 on `control`, where the floor plays no part
#   a = 4 max (|E32 - E64| - r E64) / P_t over all the other signals
# measured (fp32 oracle, before the factor):          r              a
#   vocos   (HTK, fp32-built filterbank)              2.841e-5       1.180e-7 (loud_low_tone)    -> r 1.14e-4, a 4.8e-7
#   bigvgan (Slaney, float64-built filterbank)        7.989e-6       4.409e-8 (edge_steps)       -> r 3.2e-5,  a 1.8e-7
# measured on an MI355X (mel_frame_kernel vs float64, worst over the level cases of tests/test_gpu_mel_levels.py; the filterbank tables are
# built in double, so the relative part is far below the fp32 oracle's):
#   vocos   r-part 5.7e-7  a-part 1.06e-7  worst |dE| / bound 0.22 (dc_plus_tones)
#   bigvgan r-part 1.9e-6  a-part 3.3e-8   worst |dE| / bound 0.22 (tones); 0.31 over the geometry cases (sr 44 100)
# all-zero frames: 3.2e-7 off log(1e-5), the rounding of that number to fp32 (1.59e-6 while the kernel took logf of the clamped energy)
BOUND = {"vocos": (1.14e-4, 4.8e-7), "bigvgan": (3.2e-5, 1.8e-7)}


def linear_parts(got_log, ref_log64, r, a):
    """The excess of |E_got - E_ref| over each half of the bound, as that half's constant: r-part = max (|dE| - a P_t) / E_ref,
    a-part = max (|dE| - r E_ref) / P_t (neither below 0), and the worst |dE| / (r E_ref + a P_t) with its index."""
    e_ref = ref_log64.double().exp()
    d = (got_log.detach().cpu().double().exp() - e_ref).abs()
    p = e_ref.amax(dim=-2, keepdim=True)
    r_part = ((d - a * p) / e_ref).clamp(min=0.0).max().item()
    a_part = ((d - r * e_ref) / p).clamp(min=0.0).max().item()
    use = d / (r * e_ref + a * p) if (r > 0 or a > 0) else d * float("inf")
    return r_part, a_part, use


def check_linear(got_log, ref_log64, r, a, tag="mel"):
    """Asserts |E_got - E_ref| <= r E_ref + a P_t for every bin of log-mels [b, n_mels, T]; prints and returns the measured r- and a-parts."""
    assert got_log.shape == ref_log64.shape, (got_log.shape, ref_log64.shape)
    assert torch.isfinite(got_log).all(), f"{tag}: non-finite log-mel"
    r_part, a_part, use = linear_parts(got_log, ref_log64, r, a)
    worst = use.max().item()
    print(f"[parity] {tag}: linear r-part {r_part:.3e} (r {r:.1e}) a-part {a_part:.3e} (a {a:.1e}) worst |dE| / bound {worst:.3f}")
    if not worst <= 1.0:
        i = [int(v) for v in torch.unravel_index(use.argmax(), use.shape)]
        n_bad = int((use > 1.0).sum())
        raise AssertionError(f"{tag}: {n_bad} of {use.numel()} bins outside r E + a P_t, worst {worst:.3f}x at [b, mel, frame] = {i}: "
                             f"got {got_log.detach().cpu()[tuple(i)].item():.6f} ref {ref_log64[tuple(i)].item():.6f}")
    return r_part, a_part


def check_exact_frames(got_log, zero, tag="mel"):
    """All-zero frames (zero [b, T] bool) give log(1e-5) to within 1e-6 in every channel.  Returns the number of such frames."""
    g = got_log.detach().cpu().double().transpose(-1, -2)[zero]        # [frames, n_mels]
    if g.numel():
        err = (g - LOG_CLAMP).abs().max().item()
        print(f"[parity] {tag}: {g.shape[0]} all-zero frames, max |log-mel - log(1e-5)| {err:.3e}")
        assert err <= 1e-6, f"{tag}: an all-zero frame is {err:.3e} off log(1e-5)"
    return g.shape[0]


def far_above_floor(ref_log64, factor=1e3):
    """Every bin of the float64 reference is `factor` above the clamp: the log-domain bounds of the older tests apply."""
    return bool((ref_log64.double().exp() >= factor * CLAMP).all())
