"""Mel front-end (MelSpec with mel_spec_type="vocos", F/model/modules.py:75-101,104-143) on the device."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, torch_ops
from .ops import call_op, pointer_table


def _out(b, n_mels, frames, device):
    """The output buffer.  A geometry that has no frame count (hop_length <= 0, n_mels < 0) gets an empty one: refusing it is the library's
    job, and it does so before it touches the buffer."""
    return torch.empty(b, max(n_mels, 0), max(frames, 0), device=device, dtype=torch.float32)


@torch.no_grad()
def mel_spectrogram(wave: torch.Tensor, n_fft=1024, hop_length=256, n_mel_channels=100, target_sample_rate=24000):
    """wave [b, nw] (device fp32) -> log-mel [b, n_mels, 1 + nw // hop]."""
    if wave.ndim == 3:
        wave = wave.squeeze(1)
    assert wave.ndim == 2
    if wave.device.type != "cuda":
        raise _lib.F5HipError("mel_spectrogram needs a HIP device tensor (no CPU fallback)")
    wave = wave.to(torch.float32).contiguous()
    b, nw = wave.shape
    mel = _out(b, n_mel_channels, 1 + nw // hop_length if hop_length > 0 else 0, wave.device)
    _lib.check(_lib.lib().f5hip_mel_spectrogram(b, nw, C.c_void_p(wave.data_ptr()), C.c_void_p(mel.data_ptr()), n_fft,
                                                hop_length, n_mel_channels, target_sample_rate,
                                                _lib.current_stream_ptr()), "f5hip_mel_spectrogram")
    return mel


@torch.no_grad()
def mel_spectrogram_bigvgan(wave: torch.Tensor, n_fft=1024, hop_length=256, n_mel_channels=100, target_sample_rate=24000):
    """get_bigvgan_mel_spectrogram (F/model/modules.py:30-72): wave [b, nw] (device fp32) -> log-mel [b, n_mels, nw // hop]."""
    if wave.ndim == 3:
        wave = wave.squeeze(1)
    assert wave.ndim == 2
    if wave.device.type != "cuda":
        raise _lib.F5HipError("mel_spectrogram_bigvgan needs a HIP device tensor (no CPU fallback)")
    wave = wave.to(torch.float32).contiguous()
    b, nw = wave.shape
    pad = (n_fft - hop_length) // 2
    frames = (nw + 2 * pad - n_fft) // hop_length + 1 if hop_length > 0 else 0
    mel = _out(b, n_mel_channels, frames, wave.device)
    _lib.check(_lib.lib().f5hip_mel_spectrogram_bigvgan(b, nw, C.c_void_p(wave.data_ptr()), C.c_void_p(mel.data_ptr()), n_fft,
                                                        hop_length, n_mel_channels, target_sample_rate,
                                                        _lib.current_stream_ptr()), "f5hip_mel_spectrogram_bigvgan")
    return mel


MEL_VARIANTS = ("vocos", "bigvgan")   # the library's variant codes 0, 1


def mel_frames(n_samples, variant, n_fft=1024, hop_length=256):
    """Frames of a clip of `n_samples`: the single-clip rule of `mel_spectrogram` ("vocos") or `mel_spectrogram_bigvgan` ("bigvgan")."""
    return 1 + n_samples // hop_length if variant == "vocos" else (n_samples + 2 * ((n_fft - hop_length) // 2) - n_fft) // hop_length + 1


@torch.no_grad()
def mel_spectrogram_ragged(waves, variant="vocos", n_fft=1024, hop_length=256, n_mel_channels=100, target_sample_rate=24000):
    """Both front-ends for several clips of their own lengths in ONE library call and one launch (include/f5hip.h
    f5hip_mel_spectrogram_ragged): `waves` = one 1-D contiguous fp32 device tensor per clip (views of a packed buffer are read in place).
    Returns (mel [sum T, n_mels] fp32 device, frame-major and packed in clip order, [T_i]); clip i's rows equal
    `mel_spectrogram(clip_i[None])[0].T` (resp. `mel_spectrogram_bigvgan`) bit for bit."""
    if variant not in MEL_VARIANTS:
        raise _lib.F5HipError(f"mel_spectrogram_ragged: unknown variant {variant!r} (one of {list(MEL_VARIANTS)})")
    waves = list(waves)
    if not waves:
        raise _lib.F5HipError("mel_spectrogram_ragged: no clips")
    ptrs, lens = pointer_table("mel_spectrogram_ragged", waves, "clip")
    code = MEL_VARIANTS.index(variant)
    short = n_fft if code else n_fft // 2 + 1
    for i, n in enumerate(lens.tolist()):
        if n < short:
            raise _lib.F5HipError(f"mel_spectrogram_ragged: clip {i} has {n} samples (the {variant} front-end needs at least {short})")
    frames = [mel_frames(n, variant, n_fft, hop_length) if hop_length > 0 else 0 for n in lens.tolist()]
    if torch_ops.load():
        mel = call_op("mel_spectrogram_ragged", waves, n_fft, hop_length, n_mel_channels, target_sample_rate, code)
    else:
        with torch.cuda.device(waves[0].device):
            mel = torch.empty(max(sum(frames), 0), max(n_mel_channels, 0), device=waves[0].device, dtype=torch.float32)
            _lib.check(_lib.lib().f5hip_mel_spectrogram_ragged(len(waves), C.c_void_p(lens.ctypes.data), C.c_void_p(ptrs.ctypes.data), C.c_void_p(mel.data_ptr()),
                                                               n_fft, hop_length, n_mel_channels, target_sample_rate, code, _lib.current_stream_ptr()),
                       "f5hip_mel_spectrogram_ragged")
    return mel, frames
