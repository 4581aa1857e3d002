"""Host-side mirror of the reference's model objects for the inference path.

`F5HipModel` stands where the reference passes `model_obj` (a `CFM` wrapping a `DiT`):
`sample()` has the signature and semantics of `CFM.sample` (F/model/cfm.py:82-210) and
`transformer_forward()` those of `DiT.forward` (F/model/backbones/dit.py:130-163).  All arithmetic runs in
libf5hip (HIP kernels); torch is used only to own device buffers and the stream.
"""
from __future__ import annotations

import ctypes as C
import types
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, torch_ops
from .tokenizer import list_str_to_idx


@dataclass(frozen=True)
class DiTArch:
    """model.arch of F/configs/F5TTS_*_train.yaml:24-30."""
    dim: int = 1024
    depth: int = 22
    heads: int = 16
    ff_mult: int = 2
    text_dim: int = 512
    conv_layers: int = 4
    mel_dim: int = 100
    text_num_embeds: int = 2545


F5TTS_BASE = DiTArch()
F5TTS_SMALL = DiTArch(dim=768, depth=18, heads=12)


@dataclass(frozen=True)
class UNetTArch:
    """model.arch of F/configs/E2TTS_*_train.yaml:24-28: flat-UNet transformer, text_dim = mel_dim, no text conv."""
    dim: int = 1024
    depth: int = 24
    heads: int = 16
    ff_mult: int = 4
    mel_dim: int = 100
    text_num_embeds: int = 2545

    @property
    def text_dim(self):
        return self.mel_dim

    @property
    def conv_layers(self):
        return 0


E2TTS_BASE = UNetTArch()
E2TTS_SMALL = UNetTArch(dim=768, depth=20, heads=12)


@dataclass(frozen=True)
class MMDiTArch:
    """MMDiT.__init__ arguments (F/model/backbones/mmdit.py:84-95): dual-stream blocks over the audio frames and the text tokens, joint
    attention, the last block context-pre-only; the text is embedded at `dim` (no ConvNeXt).  No YAML of the reference uses it."""
    dim: int = 512
    depth: int = 16
    heads: int = 16
    ff_mult: int = 2
    mel_dim: int = 100
    text_num_embeds: int = 256

    @property
    def text_dim(self):
        return self.dim

    @property
    def conv_layers(self):
        return 0


# torchdiffeq method name -> f5hip_dit_set_ode_method code (include/f5hip.h)
_ODE_METHODS = {"euler": 0, "midpoint": 1, "rk4": 2}
# backbone forwards per step of every method
ODE_FORWARDS = {"euler": 1, "midpoint": 2, "rk4": 4}


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _ptr(t):
    if isinstance(t, np.ndarray):
        return C.c_void_p(t.ctypes.data)
    return C.c_void_p(t.data_ptr())


def unit_duration(cond_frames: int, n_tokens: int, frames: int, max_duration: int = 4096) -> int:
    """The rows `sample()` lays out for a batch-1 unit: the planned `frames`, raised to lens + 1 where lens = max(prompt mel frames, text
    tokens) (F/model/cfm.py:123-125,136-137), capped at `max_duration`.  A seeded unit's noise has this many rows."""
    return min(max(max(int(n_tokens), int(cond_frames)) + 1, int(frames)), int(max_duration))


def per_unit_cfg(cfg_strength, n: int):
    """None for one scalar strength (f5hip_cfm_sample_masked), else the n per-unit strengths as fp32 (f5hip_cfm_sample_units)."""
    if isinstance(cfg_strength, (int, float, np.floating, np.integer)) or (isinstance(cfg_strength, torch.Tensor) and cfg_strength.ndim == 0):
        return None
    cfg = np.ascontiguousarray(np.asarray([float(c) for c in cfg_strength], dtype=np.float32))
    if cfg.shape != (n,):
        raise ValueError(f"cfg_strength: one value per unit ({n}) or one float, got {cfg.shape[0]} values")
    return cfg


def per_unit_values(value, n: int, name: str):
    """`value` itself for one value shared by the n units, else the list of the n per-unit values (a list, tuple or 1-d array / tensor)."""
    if value is None or isinstance(value, (int, float, np.floating, np.integer)) or (isinstance(value, torch.Tensor) and value.ndim == 0):
        return value
    vals = [v.item() if isinstance(v, (torch.Tensor, np.ndarray, np.generic)) else v for v in value]
    if len(vals) != n:
        raise ValueError(f"{name}: one value per unit ({n}) or one value, got {len(vals)} values")
    return vals


def per_unit_methods(ode_method, n: int):
    """None when no unit names a solver (`ode_method` None), else the n per-unit names, None where a unit follows the handle: `ode_method` is
    one name for all units or one name (or None) per unit."""
    if ode_method is None:
        return None
    names = [ode_method] * n if isinstance(ode_method, str) else list(ode_method)
    if len(names) != n:
        raise ValueError(f"ode_method: one name per unit ({n}) or one name, got {len(names)} values")
    for name in names:
        if name is not None and name not in _ODE_METHODS:
            raise ValueError(f"ode_method must be one of 'euler', 'midpoint', 'rk4' (got {name!r})")
    return names if any(name is not None for name in names) else None


def time_grid(n_steps: int, sway, t_start: float = 0.0):
    """The fp32 time grid of CFM.sample (F/model/cfm.py:196-198): n_steps + 1 points from t_start to 1, sway-sampled unless `sway` is None."""
    t = torch.linspace(t_start, 1, n_steps + 1, dtype=torch.float32)
    if sway is not None:
        t = t + sway * (torch.cos(torch.pi / 2 * t) - 1 + t)
    return t


def span_slices(units, max_steps: int, method: str = "euler"):
    """What one span asks of every unit: (take, last, t_grids) -- unit i takes take[i] = min(max_steps, remaining) steps, last[i] = 1 when that
    brings it to its end, and t_grids holds the units' take[i] + 1 grid points from their cursors on, one slice after the other (slices
    of the units' own fp32 arrays: the values of the whole grid, bit for bit).
    A unit with a solver of its own (`unit.method`; `method` is the handle's) is budgeted in backbone forwards: it takes
    min(remaining, max(1, max_steps * forwards(method) // forwards(unit.method))) steps, so a span costs every unit about the same number of
    forwards, and a unit whose solver is the handle's takes max_steps like a unit without one."""
    units = list(units)
    if not units or int(max_steps) < 1 or any(u.done for u in units):
        raise ValueError("a span needs at least one unit, none of them done, and max_steps >= 1")
    take = []
    for u in units:
        own = getattr(u, "method", None)
        budget = int(max_steps) if own is None else max(1, int(max_steps) * ODE_FORWARDS[method] // ODE_FORWARDS[own])
        take.append(min(budget, u.remaining))
    last = np.ascontiguousarray(np.asarray([k == u.remaining for k, u in zip(take, units)], dtype=np.uint8))
    return take, last, np.ascontiguousarray(np.concatenate([u.grid[u.cursor:u.cursor + k + 1] for k, u in zip(take, units)]))


class SpanUnit:
    """One sampling unit that is advanced span by span (`F5HipModel.plan_unit` / `advance`): what `sample()` would hand the library for it
    -- conditioning rows, their mask, the text row, the whole fp32 time grid, the CFG strength, the ODE method (None: the handle's) -- plus
    the ODE state on the device and the step cursor.  `noise` is the state before the first step (kept so that the unit can start over: `reset()`); `mel` is the final
    [dur, mel] result once the last step has run, else None."""

    def __init__(self, cond, cond_mask, text, grid, cfg_strength, noise, method=None):
        self.cond, self.cond_mask, self.text, self.grid, self.cfg_strength = cond, cond_mask, text, grid, float(cfg_strength)
        self.method = method
        self.noise, self.state = noise, noise.clone()
        self.cursor, self.mel = 0, None

    @property
    def dur(self) -> int:
        return int(self.state.shape[0])

    @property
    def steps(self) -> int:
        return len(self.grid) - 1

    @property
    def remaining(self) -> int:
        return self.steps - self.cursor

    @property
    def done(self) -> bool:
        return self.mel is not None

    def stepped(self, k: int, end) -> bool:
        """After a span that wrote `state`: k steps on; at the end of the grid the state is the unit's mel.  True when it ended."""
        self.cursor += k
        if end:
            self.mel = self.state
        return bool(end)

    def reset(self):
        """Back to the first step with the noise the unit already drew."""
        self.state.copy_(self.noise)
        self.cursor, self.mel = 0, None


class F5HipModel:
    # plan_unit() / advance(): units are sampled in resumable spans (f5hip_cfm_sample_span), so new units can join between the spans of
    # others; infer.SpanScheduler and serve.TTSManager(micro_batch=dict(span_steps=...)) look for this flag
    resumable_spans = True
    # sample() / sample_units() take `steps` and `sway_sampling_coef` per unit too and sample units of different time grids in ONE call
    # (f5hip_cfm_sample_grids); infer.infer_requests and serve.ShardedSampler look for this flag before they merge time grids
    per_unit_time_grids = True

    def __init__(self, arch: DiTArch | UNetTArch | MMDiTArch, state_dict: dict, vocab_char_map: dict | None = None, gemm_planes: int = 3,
                 device: str | torch.device = "cuda:0", mel_spec_type: str = "vocos", odeint_kwargs: dict | None = None,
                 attn_shape_invariant: bool | None = None):
        # odeint_kwargs: CFM's constructor argument (F/model/cfm.py:37-41), dict(method="euler") by default; "midpoint" (the other solver
        # the reference names) and "rk4" are torchdiffeq's other fixed-grid solvers.  Adaptive torchdiffeq solvers are not offered.
        self.odeint_kwargs = dict(odeint_kwargs) if odeint_kwargs is not None else dict(method="euler")
        method = self.odeint_kwargs.get("method", "euler")
        if method not in _ODE_METHODS or set(self.odeint_kwargs) - {"method"}:
            raise ValueError(f"odeint_kwargs={self.odeint_kwargs!r}: only method='euler', 'midpoint' or 'rk4' on the fixed grid is supported")
        self.arch = arch
        self.device = torch.device(device)
        self.vocab_char_map = vocab_char_map
        self.mel_spec_type = mel_spec_type
        self.num_channels = arch.mel_dim
        self.gemm_planes = gemm_planes   # 3 = mixed parity mode (default), 2 = bf16x3 everywhere, 1 = plain bf16 (include/f5hip.h)
        self._lib = _lib.lib()
        if self.device.type != "cuda":
            raise _lib.F5HipError("F5HipModel needs a HIP device (no CPU fallback)")
        torch.cuda.set_device(self.device)
        cfg = _lib.DitConfig(arch.dim, arch.depth, arch.heads, arch.ff_mult, arch.text_dim, arch.conv_layers,
                             arch.mel_dim, arch.text_num_embeds, gemm_planes, 1 if isinstance(arch, UNetTArch) else (2 if isinstance(arch, MMDiTArch) else 0))
        self._h = self._lib.f5hip_dit_create(C.byref(cfg))
        if not self._h:
            raise _lib.F5HipError("f5hip_dit_create: " + self._lib.f5hip_last_error().decode())
        # reference checkpoint keys: strip the EMA prefix like load_checkpoint does (F/infer/utils_infer.py:198-202)
        for k, v in state_dict.items():
            k = k.replace("ema_model.", "")
            if not k.startswith("transformer."):
                continue
            a = np.ascontiguousarray(v.detach().to(torch.float32).cpu().numpy())
            _lib.check(self._lib.f5hip_dit_load_param(self._h, k.encode(), _ptr(a), a.size), "load_param " + k)
        _lib.check(self._lib.f5hip_dit_finalize(self._h), "f5hip_dit_finalize")
        _lib.check(self._lib.f5hip_dit_set_ode_method(self._h, _ODE_METHODS[method]), "f5hip_dit_set_ode_method")
        self.set_attention_shape_invariant(attn_shape_invariant)

    @property
    def ode_method(self) -> str:
        """The handle's solver (odeint_kwargs): what a unit without an `ode_method` of its own is stepped by."""
        return self.odeint_kwargs.get("method", "euler")

    def set_attention_shape_invariant(self, on: bool | None):
        """This handle's attention arithmetic (include/f5hip.h): True = a sequence's output does not depend on what it is batched with,
        False = the fastest kernel per launch shape, None = follow the process default (f5hip_set_attention_shape_invariant)."""
        self.attn_shape_invariant = on
        _lib.check(self._lib.f5hip_dit_set_attention_shape_invariant(self._h, -1 if on is None else int(bool(on))), "f5hip_dit_set_attention_shape_invariant")

    def set_profiling(self, enabled: bool):
        """HIP-event timing of this handle's launches, per kernel class (its own spans and totals: other handles are not counted)."""
        _lib.check(self._lib.f5hip_dit_set_profiling(self._h, int(bool(enabled))), "f5hip_dit_set_profiling")

    def get_profile(self) -> dict:
        out = {}
        for cls in ("gemm", "attn", "ln", "other"):
            ms, n = C.c_double(0), C.c_int64(0)
            _lib.check(self._lib.f5hip_dit_get_profile(self._h, cls.encode(), C.byref(ms), C.byref(n)), "f5hip_dit_get_profile")
            out[cls] = {"total_ms": ms.value, "launches": n.value}
        return out

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.f5hip_dit_destroy(h)

    def eval(self):
        return self

    # ------------------------------------------------------------------ DiT.forward
    def transformer_forward(self, x, cond, text, time, drop_audio_cond, drop_text, mask=None, n_blocks=-1):
        """DiT.forward for x/cond [b, n, mel] (device fp32), text int [b, nt], scalar time.  With `mask`
        ([b, n] bool) the reference's padded-batch semantics are reproduced (key-padding + zeroed rows)."""
        b, n, mel = x.shape
        x = x.to(self.device, torch.float32).contiguous()
        cond = cond.to(self.device, torch.float32).contiguous()
        text = _i32(text.cpu().numpy() if isinstance(text, torch.Tensor) else text).reshape(b, -1)
        seq_len = _i32([n] * b)
        kv_len = _i32(mask.sum(-1).cpu().numpy()) if mask is not None else seq_len
        da = np.full(b, 1 if drop_audio_cond else 0, dtype=np.uint8)
        dt = np.full(b, 1 if drop_text else 0, dtype=np.uint8)
        width = mel if n_blocks < 0 else self.arch.dim
        out = torch.empty(b, n, width, device=self.device, dtype=torch.float32)
        _lib.check(self._lib.f5hip_dit_forward(
            self._h, b, _ptr(seq_len), _ptr(kv_len), _ptr(x), _ptr(cond), _ptr(text), text.shape[1], float(time),
            _ptr(da), _ptr(dt), n_blocks, _ptr(out) if n_blocks < 0 else None, _ptr(out) if n_blocks >= 0 else None,
            _lib.current_stream_ptr()), "f5hip_dit_forward")
        return out

    def read_tap(self, name: str, rows: int, width: int):
        out = torch.empty(rows, width, device=self.device, dtype=torch.float32)
        _lib.check(self._lib.f5hip_dit_read_tap(self._h, name.encode(), _ptr(out), out.numel(), _lib.current_stream_ptr()),
                   "f5hip_dit_read_tap")
        return out

    # ------------------------------------------------------------------ CFM.sample
    def cond_mel(self, audio):
        """The mel front-end CFM.sample applies to a raw-wave `cond` (F/model/cfm.py:103-106, modules.py:123-143): [b, nw] -> [b, n, mel].
        infer_batch_process computes it once per request and hands the mel to every chunk (the reference recomputes it per chunk)."""
        from .mel import mel_spectrogram, mel_spectrogram_bigvgan
        fe = mel_spectrogram_bigvgan if self.mel_spec_type == "bigvgan" else mel_spectrogram
        cond = fe(audio.to(self.device, torch.float32)).permute(0, 2, 1)
        assert cond.shape[-1] == self.num_channels
        return cond

    def cond_mel_ragged(self, audios):
        """`cond_mel` for several reference waves of their own lengths ([1, nw] or [nw] each, on this model's device) in ONE launch
        (f5hip_mel_spectrogram_ragged): [mel_i [1, n_i, mel]], views of one packed buffer, each `cond_mel(audio_i)` bit for bit."""
        from .mel import mel_spectrogram_ragged
        waves = [a.to(self.device, torch.float32).reshape(-1) for a in audios]   # (views: a prepared voice's wave is read where it lies)
        mel, frames = mel_spectrogram_ragged(waves, "bigvgan" if self.mel_spec_type == "bigvgan" else "vocos", n_mel_channels=self.num_channels)
        return [m[None] for m in mel.split(frames)]

    def prepare_voices(self, voices):
        """The reference-audio front-end of deferred `infer.PreparedVoice`s on this model's device: `infer.prepare_voices`, one ragged
        f5hip_ref_frontend call per distinct sample rate -- and then the reference mel of every voice it just prepared in ONE
        `cond_mel_ragged` call, read straight from the front-end's packed output (a script that brings four uploads launches one mel kernel,
        not four back to back)."""
        from .infer import PreparedVoice, prepare_voices
        ready = {id(v) for v in voices if isinstance(v, PreparedVoice) and v.pending is None}
        out = prepare_voices(voices, device=self.device)
        fresh = list({id(v): v for v in out if id(v) not in ready and v.mel is None}.values())
        if fresh:
            for v, mel in zip(fresh, self.cond_mel_ragged([v.audio for v in fresh])):
                v.mel = mel
        return out

    @torch.no_grad()
    def sample_units(self, audio, units, *, steps=32, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=None, generators=None, y0=None,
                     ode_method=None):
        """Independent sampling units in ONE sampler call: the text chunks of one request (independent `sample()` calls in the
        reference, F/infer/utils_infer.py:441-466), or the chunks of several requests with different voices (`infer.infer_requests`).
        `audio`: the reference wave [1, nw] (or its mel [1, n, mel]) shared by all units, or a list with one such tensor per unit;
        `units` = [(tokens, frames)].  Returns one [frames_i, mel] tensor per unit.  Every unit keeps batch-1 semantics with its own
        prompt length (`lens`), and noise is drawn unit by unit in order, i.e. the same draws the reference's sequential calls make
        from the global generator.

        Per-unit settings: `cfg_strength` is one float or one value per unit (a unit below 1e-5 runs no unconditional branch); `generators`
        ([torch.Generator | None] per unit) draws a unit's noise from its own CPU generator instead of the global one, with the unit's final
        duration (`unit_duration`), and `y0` ([tensor [dur_i, mel] | None] per unit) hands a unit its noise outright.  Units without either
        keep drawing from the global generator, unit by unit in order.  `steps` and `sway_sampling_coef` are one value or one value per unit
        (None allowed per unit for the sway): units of different time grids are sampled in the same call.  `ode_method`: None (the handle's
        solver), one name, or one name (or None) per unit: units of different solvers are sampled in the same call too (`sample`)."""
        b = len(units)
        frames = torch.tensor([int(f) for _, f in units], dtype=torch.long)
        lens = None
        if isinstance(audio, (list, tuple)):
            assert len(audio) == b, "one reference per unit"
            mels, cache = [], {}
            for a in audio:   # the mel of a voice is computed once however many units share it
                if id(a) not in cache:
                    cache[id(a)] = (self.cond_mel(a) if a.ndim == 2 else a.to(self.device, torch.float32))[0]
                mels.append(cache[id(a)])
            lens = torch.tensor([m.shape[0] for m in mels], dtype=torch.long)
            cond = torch.nn.utils.rnn.pad_sequence(mels, batch_first=True)
        else:
            cond = (self.cond_mel(audio) if audio.ndim == 2 else audio.to(self.device, torch.float32)).expand(b, -1, -1)
        p = self._plan_batch(cond, [t for t, _ in units], frames, lens=lens, steps=steps, cfg_strength=cfg_strength,
                             sway_sampling_coef=sway_sampling_coef, seed=seed, generators=generators, y0=y0, ode_method=ode_method)
        out = self._sample_planned(p)
        # (a duration is raised to lens + 1 like the reference does, cfm.py:136: the rows of unit i are its FINAL duration)
        return [out[i, :p.durs[i]] for i in range(b)]

    @torch.no_grad()
    def sample(self, cond, text, duration, *, lens=None, steps=32, cfg_strength=1.0, sway_sampling_coef=None,
               seed=None, max_duration=4096, vocoder=None, no_ref_audio=False, duplicate_test=False, t_inter=0.1,
               edit_mask=None, y0=None, padded_batch=False, generators=None, ode_method=None):
        """CFM.sample (F/model/cfm.py:82-210).  Returns (out [b, n, mel] on the device, None): the trajectory is
        not materialised (its only in-tree consumer drops it, F/infer/utils_infer.py:459).

        Batch semantics.  Default: every item is sampled with the reference's batch-1 semantics (mask=None, no padding) -- what
        `infer_batch_process` uses, and independent of the batch composition.  `padded_batch=True` reproduces what the reference
        computes when it is handed b > 1 items itself (cfm.py:151-154: every item padded to the longest, key-padding mask, zeroed
        attention rows, unmasked convolutions over the padding), padded rows included.
        `y0` ([b, n, mel] or list of [dur_i, mel]; host or device) overrides the noise, which is otherwise drawn exactly like the
        reference's CPU path (per item `torch.manual_seed(seed)`; `torch.randn(dur, mel)` from the global CPU generator).  Per item, a
        list `y0` may hold None and `generators` ([torch.Generator | None]) draws the item's `randn(dur, mel)` from its own generator.
        `cfg_strength`: one float (f5hip_cfm_sample_masked) or one value per item (f5hip_cfm_sample_units).
        `steps` / `sway_sampling_coef`: one value, or one value per item (sway None allowed per item).  Every item's grid is built as the
        scalar call builds it; when they all come out equal the call is the one-grid call, otherwise f5hip_cfm_sample_grids samples every
        item on its own grid in the same call (an item whose steps are done leaves the batch).
        `ode_method`: None = the handle's solver (odeint_kwargs); else "euler" / "midpoint" / "rk4" for all items, or one name (or None) per
        item.  When some item's solver differs from the handle's, f5hip_cfm_sample_methods steps every item by its own rule in the same
        call; an item's result is what it gets alone on a handle built with its method."""
        p = self._plan_batch(cond, text, duration, lens=lens, steps=steps, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef,
                             seed=seed, max_duration=max_duration, duplicate_test=duplicate_test, t_inter=t_inter, edit_mask=edit_mask, y0=y0,
                             padded_batch=padded_batch, generators=generators, ode_method=ode_method)
        out = self._sample_planned(p)
        if no_ref_audio:   # cfm.py:157-158: the final overwrite then copies zeros
            out = torch.where(p.cond_mask[..., None].to(self.device), torch.zeros_like(out), out)
        if vocoder is not None:
            out = vocoder(out.permute(0, 2, 1))
        return out, None

    def _sample_planned(self, p):
        """The one whole-grid library call for a planned batch (`_plan_batch`): packs the items' rows back to back, picks the entry point
        -- one grid and one strength: f5hip_cfm_sample_masked; one grid, a strength per item: f5hip_cfm_sample_units; a grid per item:
        f5hip_cfm_sample_grids; some item's ODE method is not the handle's: f5hip_cfm_sample_methods -- and returns the result as
        [b, nmax, mel], zero behind an item's laid-out rows."""
        batch, nmax, lay = p.batch, p.nmax, p.lay
        t = p.grids[0]
        cond_packed = torch.cat([p.cond[i, :lay[i]] for i in range(batch)], dim=0).contiguous()
        mask_packed = np.ascontiguousarray(
            torch.cat([p.cond_mask[i, :lay[i]] for i in range(batch)]).numpy().astype(np.uint8))
        y0_packed = torch.cat(p.ys, dim=0).contiguous()
        tg = np.ascontiguousarray(t.numpy().astype(np.float32))
        if any(name != self.ode_method for name in p.methods):
            cfg_all = p.cfg_units if p.cfg_units is not None else np.full(batch, float(p.cfg_strength), dtype=np.float32)
            entry, tail = "cfm_sample_methods", [_i32(p.steps_u), np.ascontiguousarray(torch.cat(p.grids).numpy().astype(np.float32)), cfg_all,
                                                 _i32([_ODE_METHODS[name] for name in p.methods]), None]
        elif not all(g.shape == t.shape and torch.equal(g, t) for g in p.grids[1:]):
            cfg_all = p.cfg_units if p.cfg_units is not None else np.full(batch, float(p.cfg_strength), dtype=np.float32)
            entry, tail = "cfm_sample_grids", [_i32(p.steps_u), np.ascontiguousarray(torch.cat(p.grids).numpy().astype(np.float32)), cfg_all]
        elif p.cfg_units is not None:
            entry, tail = "cfm_sample_units", [tg, p.cfg_units]
        else:
            entry, tail = "cfm_sample", [tg, float(p.cfg_strength)]
        out_packed = self._call_sampler(entry, [_i32(lay), _i32(p.durs) if p.padded else None, mask_packed, _i32(p.text.numpy())],
                                        cond_packed, y0_packed, tail)
        if all(n == nmax for n in lay):
            return out_packed.view(batch, nmax, self.num_channels)
        out = torch.zeros(batch, nmax, self.num_channels, device=self.device, dtype=torch.float32)
        o = 0
        for i in range(batch):
            out[i, :lay[i]] = out_packed[o:o + lay[i]]
            o += lay[i]
        return out

    def _call_sampler(self, entry, host_arrays, cond, y0, tail):
        """ONE sampler call, `entry` one of cfm_sample / cfm_sample_units / cfm_sample_grids / cfm_sample_span / cfm_sample_methods: the TORCH_LIBRARY operator
        (csrc/torch_ops.cpp) when it is loaded, else the same C entry point through ctypes.  `host_arrays` = (dur, kv_len | None, cond_mask,
        text [b, nt]) and the arrays in `tail` (what the entry takes behind y0; a scalar strength travels as it is, None as a null) are numpy arrays on the
        host; `cond` and `y0` are the packed device rows.  Returns the packed result, shaped like `y0`."""
        use_op = torch_ops.load()
        wrap = torch.from_numpy if use_op else _ptr
        dur, kv, mask, text = [wrap(a) if isinstance(a, np.ndarray) else a for a in host_arrays]
        rest = [wrap(a) if isinstance(a, np.ndarray) else a for a in tail]
        if use_op:
            try:
                return getattr(torch_ops.ops(), entry)(int(self._h), dur, kv, cond, mask, text, y0, *rest)
            except RuntimeError as e:
                raise _lib.F5HipError(str(e).split("\n")[0]) from None
        if entry in ("cfm_sample", "cfm_sample_units"):   # the one-grid C entries take `steps` behind the grid (the operator reads it off the grid)
            rest.insert(1, tail[0].size - 1)
        out = torch.empty_like(y0)
        fn = getattr(self._lib, "f5hip_cfm_sample_masked" if entry == "cfm_sample" else "f5hip_" + entry)
        _lib.check(fn(self._h, len(host_arrays[0]), dur, kv, _ptr(cond), mask, text, host_arrays[3].shape[1], _ptr(y0), *rest, _ptr(out),
                      _lib.current_stream_ptr()), "f5hip_" + entry)
        return out

    @torch.no_grad()
    def plan_unit(self, cond, tokens, frames, *, steps=32, cfg_strength=2.0, sway_sampling_coef=-1.0, generator=None, y0=None,
                  ode_method=None) -> SpanUnit:
        """Plans one unit as `sample_units` would sample it -- `cond` the prompt mel [1, n, mel] (or wave [1, nw]), `tokens` its text (a token list, or ids [nt]), `frames`
        its planned rows -- without running a step: conditioning, mask, text row and time grid come from the code `sample()` uses, and the
        noise is drawn here as `sample()` draws it (`y0` [dur, mel], else `generator`, else the global generator).  `ode_method`: the unit's own
        solver (None: the handle's); `advance` steps units of different solvers in one call."""
        if ode_method is not None and ode_method not in _ODE_METHODS:
            raise ValueError(f"ode_method must be one of 'euler', 'midpoint', 'rk4' (got {ode_method!r})")
        text = tokens.reshape(1, -1) if isinstance(tokens, torch.Tensor) else [tokens]
        p = self._plan_batch(cond, text, torch.tensor([int(frames)], dtype=torch.long), steps=int(steps), cfg_strength=float(cfg_strength),
                             sway_sampling_coef=sway_sampling_coef, y0=None if y0 is None else [y0],
                             generators=None if generator is None else [generator])
        dur = p.durs[0]
        return SpanUnit(p.cond[0, :dur].contiguous(), np.ascontiguousarray(p.cond_mask[0, :dur].numpy().astype(np.uint8)), _i32(p.text.numpy()[0]),
                        np.ascontiguousarray(p.grids[0].numpy().astype(np.float32)), cfg_strength, p.ys[0].contiguous(), method=ode_method)

    @torch.no_grad()
    def advance(self, units, max_steps: int):
        """ONE f5hip_cfm_sample_span call over `units` (planned, not done): each takes min(max_steps, remaining) steps of its own grid from its
        cursor on.  States and cursors are updated in place; a unit that reaches its end gets `mel` (the prompt rows overwritten with
        the conditioning, cfm.py:204).  Returns the units that ended.  Units planned with a solver of their own are budgeted in backbone
        forwards (`span_slices`); when one of them differs from the handle's, the call is f5hip_cfm_sample_methods."""
        units = list(units)
        take, last, tgs = span_slices(units, max_steps, self.ode_method)
        methods = [getattr(u, "method", None) or self.ode_method for u in units]
        entry, extra = "cfm_sample_span", [last]
        if any(name != self.ode_method for name in methods):
            entry, extra = "cfm_sample_methods", [_i32([_ODE_METHODS[name] for name in methods]), last]
        nt = max(len(u.text) for u in units)
        text_np = np.full((len(units), nt), -1, dtype=np.int32)
        for i, u in enumerate(units):
            text_np[i, :len(u.text)] = u.text
        cfg = np.ascontiguousarray(np.asarray([u.cfg_strength for u in units], dtype=np.float32))
        mask = np.ascontiguousarray(np.concatenate([u.cond_mask for u in units]))
        out = self._call_sampler(entry, [_i32([u.dur for u in units]), None, mask, text_np], torch.cat([u.cond for u in units], dim=0),
                                 torch.cat([u.state for u in units], dim=0), [_i32(take), tgs, cfg, *extra])
        ended, o = [], 0
        for u, k, end in zip(units, take, last):
            u.state.copy_(out[o:o + u.dur])
            o += u.dur
            if u.stepped(k, end):
                ended.append(u)
        return ended

    def _plan_batch(self, cond, text, duration, *, steps, cfg_strength, sway_sampling_coef, lens=None, seed=None, max_duration=4096,
                    duplicate_test=False, t_inter=0.1, edit_mask=None, y0=None, padded_batch=False, generators=None, ode_method=None):
        """Everything `sample()` decides before its library call (cfm.py:103-146,181-198), per item: the padded conditioning and its mask, the
        text rows, the final durations and laid-out rows, the noise (drawn here, in item order), the fp32 time grid and the ODE method
        (`methods`: a name per item, the handle's where the item names none).  The one place that
        builds them: `sample()` hands them to one whole call, `plan_unit()` keeps them for a unit that is advanced span by span."""
        if cond.ndim == 2:   # raw wave -> mel (cfm.py:103-106) with the extractor of mel_spec_type (modules.py:123-126)
            cond = self.cond_mel(cond)
        cond = cond.to(self.device, torch.float32)
        batch, cond_seq_len = cond.shape[:2]
        if lens is None:
            lens = torch.full((batch,), cond_seq_len, dtype=torch.long)
        lens = lens.cpu()
        if isinstance(text, list):
            assert self.vocab_char_map is not None, "string text needs a vocab_char_map"
            text = list_str_to_idx(text, self.vocab_char_map)
            assert text.shape[0] == batch
        text = text.cpu()
        text_lens = (text != -1).sum(dim=-1)
        lens = torch.maximum(text_lens, lens)                                     # cfm.py:123-125
        cond_mask = torch.arange(int(lens.amax()))[None, :] < lens[:, None]       # lens_to_mask
        if edit_mask is not None:
            cond_mask = cond_mask & edit_mask.cpu()
        if isinstance(duration, int):
            duration = torch.full((batch,), duration, dtype=torch.long)
        duration = torch.maximum(lens + 1, duration.cpu()).clamp(max=max_duration)  # cfm.py:136-137
        nmax = int(duration.amax())
        test_cond = None
        if duplicate_test:   # cfm.py:139-141: the prompt mel repeated once right behind itself
            test_cond = torch.nn.functional.pad(cond, (0, 0, cond_seq_len, nmax - 2 * cond_seq_len), value=0.0)
        cond = torch.nn.functional.pad(cond, (0, 0, 0, nmax - cond_seq_len), value=0.0)
        cond_mask = torch.nn.functional.pad(cond_mask, (0, nmax - cond_mask.shape[-1]), value=False)

        durs = [int(d) for d in duration]
        padded = bool(padded_batch) and batch > 1
        lay = [nmax] * batch if padded else durs          # rows laid out per item

        # noise (cfm.py:181-186): per item randn(dur_i), zero padded to the laid-out length
        if generators is not None and len(generators) != batch:
            raise ValueError(f"generators: one per item ({batch}), got {len(generators)}")
        cfg_units = per_unit_cfg(cfg_strength, batch)
        ys = []
        for i, dur in enumerate(durs):
            given = y0[i] if y0 is not None else None
            if given is not None:
                if given.shape[0] < dur:
                    raise ValueError(f"y0 of item {i}: {given.shape[0]} rows for a duration of {dur}")
                yi = given[:dur].to(self.device, torch.float32)
            elif generators is not None and generators[i] is not None:
                yi = torch.randn(dur, self.num_channels, generator=generators[i]).to(self.device)
            else:
                if seed is not None:
                    torch.manual_seed(seed)
                yi = torch.randn(dur, self.num_channels).to(self.device)
            if lay[i] > dur:
                yi = torch.nn.functional.pad(yi, (0, 0, 0, lay[i] - dur))
            ys.append(yi)

        t_start = 0.0
        steps_u = per_unit_values(steps, batch, "steps")
        sway_u = per_unit_values(sway_sampling_coef, batch, "sway_sampling_coef")
        steps_u = [int(x) for x in steps_u] if isinstance(steps_u, list) else [int(steps_u)] * batch
        sway_u = sway_u if isinstance(sway_u, list) else [sway_u] * batch
        if duplicate_test:   # cfm.py:190-194
            t_start = float(t_inter)
            ys = [(1 - t_start) * ys[i] + t_start * test_cond[i, :lay[i]] for i in range(batch)]
            steps_u = [int(x * (1 - t_start)) for x in steps_u]

        grids, cache = [], {}
        for n_steps, sway in zip(steps_u, sway_u):
            key = (n_steps, None if sway is None else float(sway))
            if key not in cache:
                cache[key] = time_grid(n_steps, sway, t_start)
            grids.append(cache[key])
        return types.SimpleNamespace(batch=batch, nmax=nmax, cond=cond, cond_mask=cond_mask, text=text, durs=durs, lay=lay, padded=padded,
                                     cfg_strength=cfg_strength, cfg_units=cfg_units, ys=ys, steps_u=steps_u, grids=grids,
                                     methods=[name or self.ode_method for name in per_unit_methods(ode_method, batch) or [None] * batch])
