"""Vocos vocoder object: stands where the reference passes `vocoder` (F/infer/utils_infer.py:92-115,472).

`decode(mel[b, 100, T]) -> wave[b, 256 (T - 1)]` and `decode_ragged([mel_i [100, T_i]]) -> [wave_i]` run in libf5hip; state_dict keys are vocos 0.1.0's
(`backbone.embed.weight`, `backbone.convnext.{i}.*`, `backbone.final_layer_norm.*`, `head.out.*`)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, torch_ops
from .ops import call_op


def _ragged_mel(mels, frames, channels, device):
    """What the ragged decodes hand the library: (mel [n, channels, max(frames)] fp32 on the device, item i in its first frames[i] columns and
    zeros behind them; frames as the int32 host tensor)."""
    mel = torch.zeros(len(mels), channels, max(frames), device=device, dtype=torch.float32)
    for i, m in enumerate(mels):
        mel[i, :, :frames[i]] = m
    return mel, torch.tensor(frames, dtype=torch.int32)


class F5HipVocos:
    def __init__(self, state_dict: dict, in_channels=100, dim=512, intermediate_dim=1536, num_layers=8, n_fft=1024,
                 hop_length=256, gemm_planes: int = 2, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.F5HipError("F5HipVocos needs a HIP device (no CPU fallback)")
        torch.cuda.set_device(self.device)
        self.hop_length, self.dim, self.n_fft = hop_length, dim, n_fft
        self._lib = _lib.lib()
        cfg = _lib.VocosConfig(in_channels, dim, intermediate_dim, num_layers, n_fft, hop_length, gemm_planes)
        self._h = self._lib.f5hip_vocos_create(C.byref(cfg))
        if not self._h:
            raise _lib.F5HipError("f5hip_vocos_create: " + self._lib.f5hip_last_error().decode())
        for k, v in state_dict.items():
            if k.startswith("feature_extractor."):
                continue   # mel front-end buffers of the checkpoint; decode() does not use them
            a = np.ascontiguousarray(v.detach().to(torch.float32).cpu().numpy())
            _lib.check(self._lib.f5hip_vocos_load_param(self._h, k.encode(), C.c_void_p(a.ctypes.data), a.size),
                       "vocos load_param " + k)
        _lib.check(self._lib.f5hip_vocos_finalize(self._h), "f5hip_vocos_finalize")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.f5hip_vocos_destroy(h)

    def eval(self):
        return self

    def to(self, device):
        return self

    @torch.no_grad()
    def decode(self, mel: torch.Tensor) -> torch.Tensor:
        b, c, t = mel.shape
        mel = mel.to(self.device, torch.float32).contiguous()
        if torch_ops.load():   # TORCH_LIBRARY operator over the same C entry point
            return torch_ops.ops().vocos_decode(int(self._h), mel, self.hop_length)
        wave = torch.empty(b, self.hop_length * (t - 1), device=self.device, dtype=torch.float32)
        _lib.check(self._lib.f5hip_vocos_decode(self._h, b, t, C.c_void_p(mel.data_ptr()), C.c_void_p(wave.data_ptr()),
                                                _lib.current_stream_ptr()), "f5hip_vocos_decode")
        return wave

    @torch.no_grad()
    def decode_ragged(self, mels) -> list:
        """`decode` of several mels of their own lengths in ONE library call (f5hip_vocos_decode_ragged): mels = [mel_i [C, T_i]] ->
        [wave_i [hop (T_i - 1)]], each equal to `decode(mel_i[None])[0]` bit for bit (one padded row slab per item, row-wise kernels)."""
        frames = [int(m.shape[-1]) for m in mels]
        if not frames:
            return []
        c = int(mels[0].shape[0])
        if any(m.dim() != 2 or m.shape[0] != c for m in mels):
            raise _lib.F5HipError("decode_ragged: every mel must be [C, T] with the same C")
        mel, f = _ragged_mel(mels, frames, c, self.device)
        if torch_ops.load():
            wave = call_op("vocos_decode_ragged", int(self._h), mel, f, c, self.hop_length)
        else:
            wave = torch.empty(self.hop_length * sum(t - 1 for t in frames), device=self.device, dtype=torch.float32)
            _lib.check(self._lib.f5hip_vocos_decode_ragged(self._h, len(frames), C.c_void_p(f.data_ptr()), C.c_void_p(mel.data_ptr()),
                                                           C.c_void_p(wave.data_ptr()), _lib.current_stream_ptr()), "f5hip_vocos_decode_ragged")
        return list(wave.split([self.hop_length * (t - 1) for t in frames]))

    @torch.no_grad()
    def decode_taps(self, mel: torch.Tensor, frames, n_blocks: int = -1) -> dict:
        """Parity taps (f5hip_vocos_decode_taps): the ragged decode of mel [n, C, T_max], item i valid for t < frames[i], stopped behind
        `n_blocks` ConvNeXt blocks (0: embed conv + norm; -1: the whole decode).  Returns the valid rows packed item after item:
        {"x": [sum frames, dim]}, and for -1 also "y" [sum frames, n_fft + 2], "fw" [sum frames, n_fft] and "wave" [hop sum (frames - 1)].
        What mel holds behind an item's last frame is the caller's (`decode_ragged` puts zeros there); the library does not read it."""
        frames = [int(t) for t in frames]
        if mel.dim() != 3 or mel.shape[0] != len(frames) or not frames or mel.shape[2] != max(frames):
            raise _lib.F5HipError("decode_taps: mel must be [n, C, max(frames)] with one entry of frames per item")
        mel = mel.to(self.device, torch.float32).contiguous()
        f = torch.tensor(frames, dtype=torch.int32)
        rows = sum(frames)
        new = lambda *shape: torch.empty(*shape, device=self.device, dtype=torch.float32)
        out = {"x": new(rows, self.dim)}
        if n_blocks == -1:
            out.update(y=new(rows, self.n_fft + 2), fw=new(rows, self.n_fft), wave=new(self.hop_length * (rows - len(frames))))
        ptr = lambda k: C.c_void_p(out[k].data_ptr()) if k in out else None
        _lib.check(self._lib.f5hip_vocos_decode_taps(self._h, len(frames), C.c_void_p(f.data_ptr()), C.c_void_p(mel.data_ptr()), n_blocks,
                                                     ptr("x"), ptr("y"), ptr("fw"), ptr("wave"), _lib.current_stream_ptr()), "f5hip_vocos_decode_taps")
        return out


class F5HipBigVGAN:
    """BigVGAN v2 generator object: stands where the reference passes `vocoder` for mel_spec_type="bigvgan"
    (F/infer/utils_infer.py:116-129,474): `vocoder(mel[b, 100, T]) -> wave[b, 1, 256 T]`, and `decode_ragged([mel_i [100, T_i]]) -> [wave_i]`
    for chunks of different lengths in one library call.  state_dict keys are the generator's
    after `remove_weight_norm()`; weight-norm'ed checkpoints (`weight_g` / `weight_v`) are folded here the same way."""

    ragged_mel_spec_type = "bigvgan"   # what `infer._chunk_waves` asks before it hands every chunk of a batch to `decode_ragged`

    def __init__(self, state_dict: dict, num_mels=100, upsample_rates=(4, 4, 2, 2, 2, 2), upsample_kernel_sizes=(8, 8, 4, 4, 4, 4),
                 upsample_initial_channel=1536, resblock_kernel_sizes=(3, 7, 11),
                 resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5)), gemm_planes: int = 2, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.F5HipError("F5HipBigVGAN needs a HIP device (no CPU fallback)")
        torch.cuda.set_device(self.device)
        self.total_up = int(np.prod(upsample_rates))
        self.num_mels = num_mels
        self._lib = _lib.lib()
        cfg = _lib.BigVGANConfig()
        cfg.num_mels, cfg.num_upsamples, cfg.upsample_initial_channel, cfg.gemm_planes = num_mels, len(upsample_rates), upsample_initial_channel, gemm_planes
        for i, (r, k) in enumerate(zip(upsample_rates, upsample_kernel_sizes)):
            cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i] = r, k
        for j, k in enumerate(resblock_kernel_sizes):
            cfg.resblock_kernel_sizes[j] = k
            for d, dil in enumerate(resblock_dilation_sizes[j]):
                cfg.resblock_dilations[j * 3 + d] = dil
        self._h = self._lib.f5hip_bigvgan_create(C.byref(cfg))
        if not self._h:
            raise _lib.F5HipError("f5hip_bigvgan_create: " + self._lib.f5hip_last_error().decode())
        sd = dict(state_dict)
        for k in [k for k in sd if k.endswith(".weight_g")]:   # fold weight norm: w = g * v / ||v|| over all dims but 0
            base = k[: -len("_g")]
            g, v = sd.pop(k), sd.pop(base + "_v")
            sd[base] = v * (g / v.flatten(1).norm(dim=1).view(-1, *([1] * (v.ndim - 1))))
        for k, v in sd.items():
            if k.endswith(".filter"):
                continue   # anti-aliasing FIR buffers: recomputed in the library
            a = np.ascontiguousarray(v.detach().to(torch.float32).cpu().numpy())
            _lib.check(self._lib.f5hip_bigvgan_load_param(self._h, k.encode(), C.c_void_p(a.ctypes.data), a.size), "bigvgan load_param " + k)
        _lib.check(self._lib.f5hip_bigvgan_finalize(self._h), "f5hip_bigvgan_finalize")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.f5hip_bigvgan_destroy(h)

    def eval(self):
        return self

    def to(self, device):
        return self

    def remove_weight_norm(self):
        return None

    @torch.no_grad()
    def __call__(self, mel: torch.Tensor) -> torch.Tensor:
        b, c, t = mel.shape
        mel = mel.to(self.device, torch.float32).contiguous()
        if torch_ops.load():
            return torch_ops.ops().bigvgan_forward(int(self._h), mel, self.total_up)
        wave = torch.empty(b, 1, self.total_up * t, device=self.device, dtype=torch.float32)
        _lib.check(self._lib.f5hip_bigvgan_forward(self._h, b, t, C.c_void_p(mel.data_ptr()), C.c_void_p(wave.data_ptr()),
                                                   _lib.current_stream_ptr()), "f5hip_bigvgan_forward")
        return wave

    @torch.no_grad()
    def decode_ragged(self, mels) -> list:
        """`vocoder(mel)` of several mels of their own lengths in ONE library call (f5hip_bigvgan_forward_ragged): mels = [mel_i [C, T_i]] ->
        [wave_i [total_up T_i]], each equal to `vocoder(mel_i[None]).reshape(-1)` bit for bit (every item has its own rows and bounds)."""
        frames = [int(m.shape[-1]) for m in mels]
        if not frames:
            return []
        if any(m.dim() != 2 or m.shape[0] != self.num_mels for m in mels) or min(frames) < 1:
            raise _lib.F5HipError(f"decode_ragged: every mel must be [{self.num_mels}, T] with T >= 1")
        mel, f = _ragged_mel(mels, frames, self.num_mels, self.device)
        if torch_ops.load():
            wave = call_op("bigvgan_forward_ragged", int(self._h), mel, f, self.num_mels, self.total_up)
        else:
            wave = torch.empty(self.total_up * sum(frames), device=self.device, dtype=torch.float32)
            _lib.check(self._lib.f5hip_bigvgan_forward_ragged(self._h, len(frames), C.c_void_p(f.data_ptr()), C.c_void_p(mel.data_ptr()),
                                                              C.c_void_p(wave.data_ptr()), _lib.current_stream_ptr()), "f5hip_bigvgan_forward_ragged")
        return list(wave.split([self.total_up * t for t in frames]))
