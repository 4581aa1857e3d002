"""CPU oracle of the BigVGAN v2 generator (fp32, or float64 on float64 inputs) (TEST INFRASTRUCTURE ONLY).

BigVGAN is third-party to the reference: an un-vendored git submodule (`third_party/BigVGAN`, call sites
F/infer/utils_infer.py:7,116-129,474; mel front-end copied into F/model/modules.py:30-72).  This file restates the
published NVIDIA/BigVGAN v2 architecture (`bigvgan_v2_24khz_100band_256x`: upsample_rates [4,4,2,2,2,2],
kernels [8,8,4,4,4,4], initial channel 1536, AMPBlock1 with kernels [3,7,11] x dilations [1,3,5], SnakeBeta with
log-scale parameters, anti-aliased activations with 12-tap Kaiser-sinc filters, no tanh, no final bias) from the
survey's Appendix A.8 -- PARITY UNPINNED by the reference (its least-verified third-party leaf); known-answer tests in
tests/test_oracle_bigvgan.py pin the FIR design (DC gain, symmetry) and the length bookkeeping (256 x T).
State-dict keys are the generator's after `remove_weight_norm()` (utils_infer.py:128).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F


@dataclass(frozen=True)
class BigVGANConfig:
    num_mels: int = 100
    upsample_rates: tuple = (4, 4, 2, 2, 2, 2)
    upsample_kernel_sizes: tuple = (8, 8, 4, 4, 4, 4)
    upsample_initial_channel: int = 1536
    resblock_kernel_sizes: tuple = (3, 7, 11)
    resblock_dilation_sizes: tuple = ((1, 3, 5), (1, 3, 5), (1, 3, 5))


BIGVGAN_V2_24K_100B_256X = BigVGANConfig()


def kaiser_sinc_filter1d(cutoff: float, half_width: float, kernel_size: int, dtype=torch.float32) -> torch.Tensor:
    """alias_free_torch/filter.py of BigVGAN: Kaiser-windowed sinc low-pass, normalised to unit DC gain, evaluated in `dtype`."""
    even = kernel_size % 2 == 0
    half_size = kernel_size // 2
    delta_f = 4 * half_width
    A = 2.285 * (half_size - 1) * math.pi * delta_f + 7.95
    if A > 50.0:
        beta = 0.1102 * (A - 8.7)
    elif A >= 21.0:
        beta = 0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21.0)
    else:
        beta = 0.0
    window = torch.kaiser_window(kernel_size, beta=beta, periodic=False, dtype=dtype)
    time = (torch.arange(-half_size, half_size, dtype=dtype) + 0.5) if even else (torch.arange(kernel_size, dtype=dtype) - half_size)
    filt = 2 * cutoff * window * torch.sinc(2 * cutoff * time)
    return filt / filt.sum()


AA_FILTER = {}


def aa_filter(dtype=torch.float32) -> torch.Tensor:
    """The one 12-tap filter both UpSample1d(2) and DownSample1d(2) use: cutoff 0.25, half_width 0.3, in `dtype` (cached per dtype)."""
    if dtype not in AA_FILTER:
        AA_FILTER[dtype] = kaiser_sinc_filter1d(0.25, 0.3, 12, dtype)
    return AA_FILTER[dtype]


def upsample2(x: torch.Tensor) -> torch.Tensor:
    """UpSample1d(ratio=2, kernel_size=12): replicate-pad 5, grouped conv_transpose (stride 2) * 2, crop 15 / 15.  Follows x's dtype."""
    c = x.shape[1]
    x = F.pad(x, (5, 5), mode="replicate")
    x = 2 * F.conv_transpose1d(x, aa_filter(x.dtype).view(1, 1, 12).expand(c, -1, -1), stride=2, groups=c)
    return x[..., 15:-15]


def downsample2(x: torch.Tensor) -> torch.Tensor:
    """DownSample1d(ratio=2, kernel_size=12): replicate-pad (5, 6), grouped conv stride 2.  Follows x's dtype."""
    c = x.shape[1]
    x = F.pad(x, (5, 6), mode="replicate")
    return F.conv1d(x, aa_filter(x.dtype).view(1, 1, 12).expand(c, -1, -1), stride=2, groups=c)


def snake_beta(x: torch.Tensor, alpha_log: torch.Tensor, beta_log: torch.Tensor) -> torch.Tensor:
    """SnakeBeta(alpha_logscale=True): x + sin^2(x e^alpha) / (e^beta + 1e-9), per channel."""
    a = torch.exp(alpha_log)[None, :, None]
    b = torch.exp(beta_log)[None, :, None]
    return x + (1.0 / (b + 1e-9)) * torch.sin(x * a).pow(2)


def activation1d(x, alpha_log, beta_log):
    return downsample2(snake_beta(upsample2(x), alpha_log, beta_log))


def amp_block1(sd, p: str, x: torch.Tensor, k: int, dilations) -> torch.Tensor:
    for j, d in enumerate(dilations):
        xt = activation1d(x, sd[f"{p}activations.{2 * j}.act.alpha"], sd[f"{p}activations.{2 * j}.act.beta"])
        xt = F.conv1d(xt, sd[f"{p}convs1.{j}.weight"], sd[f"{p}convs1.{j}.bias"], dilation=d, padding=d * (k - 1) // 2)
        xt = activation1d(xt, sd[f"{p}activations.{2 * j + 1}.act.alpha"], sd[f"{p}activations.{2 * j + 1}.act.beta"])
        xt = F.conv1d(xt, sd[f"{p}convs2.{j}.weight"], sd[f"{p}convs2.{j}.bias"], dilation=1, padding=(k - 1) // 2)
        x = xt + x
    return x


@torch.no_grad()
def bigvgan_forward(sd: dict, cfg: BigVGANConfig, mel: torch.Tensor) -> torch.Tensor:
    """BigVGAN.forward: mel [b, num_mels, T] -> wave [b, 1, T * prod(upsample_rates)], clamped to [-1, 1].  Runs in mel's dtype (the
    state dict must match it): a float64 state dict and mel make it a float64 reference."""
    x = F.conv1d(mel, sd["conv_pre.weight"], sd["conv_pre.bias"], padding=3)
    nk = len(cfg.resblock_kernel_sizes)
    for i, (r, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        x = F.conv_transpose1d(x, sd[f"ups.{i}.0.weight"], sd[f"ups.{i}.0.bias"], stride=r, padding=(k - r) // 2)
        xs = None
        for j in range(nk):
            y = amp_block1(sd, f"resblocks.{i * nk + j}.", x, cfg.resblock_kernel_sizes[j], cfg.resblock_dilation_sizes[j])
            xs = y if xs is None else xs + y
        x = xs / nk
    x = activation1d(x, sd["activation_post.act.alpha"], sd["activation_post.act.beta"])
    x = F.conv1d(x, sd["conv_post.weight"], None, padding=3)
    return torch.clamp(x, min=-1.0, max=1.0)


def librosa_slaney_mel(sr: int, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: float | None = None) -> torch.Tensor:
    """librosa.filters.mel(htk=False, norm="slaney") -> [n_mels, 1 + n_fft // 2]  (call site F/model/modules.py:45)."""
    if fmax is None:
        fmax = sr / 2.0

    def hz_to_mel(f):
        f = torch.as_tensor(f, dtype=torch.float64)
        f_sp = 200.0 / 3
        mels = f / f_sp
        min_log_hz, logstep = 1000.0, math.log(6.4) / 27.0
        min_log_mel = min_log_hz / f_sp
        return torch.where(f >= min_log_hz, min_log_mel + torch.log(torch.clamp(f, min=1e-10) / min_log_hz) / logstep, mels)

    def mel_to_hz(m):
        f_sp = 200.0 / 3
        freqs = f_sp * m
        min_log_hz, logstep = 1000.0, math.log(6.4) / 27.0
        min_log_mel = min_log_hz / f_sp
        return torch.where(m >= min_log_mel, min_log_hz * torch.exp(logstep * (m - min_log_mel)), freqs)

    fftfreqs = torch.linspace(0, sr / 2.0, 1 + n_fft // 2, dtype=torch.float64)
    mel_f = mel_to_hz(torch.linspace(float(hz_to_mel(fmin)), float(hz_to_mel(fmax)), n_mels + 2, dtype=torch.float64))
    fdiff = mel_f[1:] - mel_f[:-1]
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = torch.clamp(torch.min(lower, upper), min=0.0)
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    return (w * enorm[:, None]).float()


def bigvgan_mel_spectrogram(wave: torch.Tensor, n_fft=1024, n_mels=100, sr=24000, hop=256, win=1024) -> torch.Tensor:
    """get_bigvgan_mel_spectrogram, F/model/modules.py:30-72: reflect-pad (n_fft - hop)/2, STFT center=False,
    sqrt(re^2 + im^2 + 1e-9), Slaney mel (fmax = sr/2), log(clamp(., 1e-5)).  wave [b, nw] -> [b, n_mels, nw // hop]."""
    pad = (n_fft - hop) // 2
    w = F.pad(wave.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    spec = torch.stft(w, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win), center=False,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    spec = torch.sqrt(torch.view_as_real(spec).pow(2).sum(-1) + 1e-9)
    mel = torch.matmul(librosa_slaney_mel(sr, n_fft, n_mels), spec)
    return torch.log(torch.clamp(mel, min=1e-5))
