"""torch.ops.f5hip.*: the hot path as PyTorch custom operators (TORCH_LIBRARY registration in csrc/torch_ops.cpp over the C ABI of libf5hip;
north_star: "host Python calling HIP through PyTorch-ROCm custom ops").  `load()` registers them (once); every caller goes through them when
the extension is present and through ctypes otherwise -- the same C entry points either way.  Three groups:
  - the samplers: cfm_sample, cfm_sample_units, cfm_sample_grids, cfm_sample_span and cfm_sample_methods (one ODE method per unit);
    `F5HipModel._call_sampler` is their one caller.
  - the vocoders: vocos_decode, vocos_decode_ragged, bigvgan_forward, bigvgan_forward_ragged (`vocoder.F5HipVocos`, `vocoder.F5HipBigVGAN`).
  - the device audio path: ref_prestep, ref_frontend, ref_assess, watermark_detect, watermark_read_ids, watermark_scan, ref_denoise, flac_decode, mel_spectrogram_ragged in front of the
    model; wave_finish, wave_finish_joins, wave_prosody, wave_prosody_formants, wave_mark, wave_mark_ids, wave_loudness, wave_encode, wave_flac and wave_flac_levels behind the
    vocoder (`ops`, `mel`);
    `ops.call_op` calls them, and the ragged vocoder operators, and turns an operator's c10::Error into F5HipError."""
from __future__ import annotations

import os

from . import _lib

TORCH_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libf5hip_torch.so")
_loaded = None


def load() -> bool:
    """True when torch.ops.f5hip is usable.  Loads libf5hip.so first (the operators are linked against it)."""
    global _loaded
    if _loaded is None:
        _loaded = False
        if os.path.exists(TORCH_LIB_PATH) and os.environ.get("F5HIP_TORCH_OPS", "1") != "0":
            import torch
            _lib.lib()
            torch.ops.load_library(TORCH_LIB_PATH)
            _loaded = True
    return _loaded


def ops():
    import torch
    if not load():
        raise _lib.F5HipError(f"{TORCH_LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    return torch.ops.f5hip
