"""GPU: every transformer block of the three backbones, and the final norm + proj_out, against the float64 references of tests/block_ref.py.

f5hip_dit_forward(n_blocks = k) returns the residual stream behind k blocks.  Block l's reference starts from the GPU's OWN h_l (upcast), so
nothing accumulates across blocks and a failure names the block and the stream.  The GPU is compared with block_ref.EXACT only.  Tolerance,
per block, sequence and stream: with model_err = reference(the mode's operand formats) - reference(exact) on the same input,
    rms(GPU - exact) <= 3 rms(model_err)   and   worst row rms(GPU - exact) <= 3 worst row rms(model_err);
the 3 covers what the operand model leaves out (fp32 accumulation over K <= 4096, the device's exp2 / tanh, rounding ties that fall
differently).  tests/test_block_reference.py shows on the CPU what this catches.  The final layer is held to the mode-2 model in both
modes: the final norm and proj_out stay split bf16 in mixed mode.  Every case also checks with the launch counters that the GEMM kernels
it is about ran, and that two identical calls return equal bits.

UNetT's time-token row is no frame and is not returned: the reference carries its own token row from layer to layer (one key of n + 1
and one row of the skip projection; its error does not reach the frames at this precision).

Largest gpu_err / model_err measured on an MI355X, per backbone and mode, is in each test's docstring: 1.26 .. 1.40 everywhere.  The blocks sit
at 1.0 .. 1.2 of the model; the largest rms ratios (1.28 .. 1.34) are the final layer's, in both modes alike (a split-bf16 GEMM sums hi x hi + hi x lo + lo x hi, the
operand model multiplies hi + lo by hi + lo; not separated further)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import block_ref as B  # noqa: E402
import test_block_reference as T  # noqa: E402
from tts_indic_server_f5_amd import synth  # noqa: E402

GEMM_COUNTERS = ("gemm5_rb11", "gemm5_rb8", "gemm6", "gemm3", "gemm_reg_bn64", "gemm_reg_bn128")
_MODES = pytest.mark.parametrize("mode", [2, 3], ids=["bf16x3", "mixed_f16"])


def _counters():
    from tts_indic_server_f5_amd import _lib
    out = {}
    for name in GEMM_COUNTERS:
        v = C.c_int64(0)
        _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
        out[name] = v.value
    return {"gemm5": out["gemm5_rb11"] + out["gemm5_rb8"], "gemm6": out["gemm6"], "gemm3": out["gemm3"],
            "gemm_reg_bn64": out["gemm_reg_bn64"], "gemm_reg_bn128": out["gemm_reg_bn128"]}


def _reset_counters():
    from tts_indic_server_f5_amd import _lib
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


class _Run:
    """One case on one handle: forward(k) -> the packed frames' stream behind k blocks (k = -1: the output) on the CPU, and the GEMM
    launches that call made."""

    def __init__(self, model, case, text=None):
        self.model, self.case = model, case
        self.seq_len = list(case["seq_len"])
        self.kv_len = list(case.get("kv_len", case["seq_len"]))
        x, cond, tx = B.case_inputs(self.seq_len, case["nt"], case["vocab"], case["seed"])
        self.text = tx if text is None else text(tx)
        self.x, self.cond = x.to(model.device).contiguous(), cond.to(model.device).contiguous()
        self.launches = {}

    def forward(self, k):
        from tts_indic_server_f5_amd import _lib
        m, n = self.model, len(self.seq_len)
        i32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int32))
        u8 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.uint8))
        sl, kv, tx = i32(self.seq_len), i32(self.kv_len), i32(self.text.numpy())
        da, dt = u8(self.case.get("drop_audio", [0] * n)), u8(self.case.get("drop_text", [0] * n))
        out = torch.empty(sum(self.seq_len), m.arch.mel_dim if k < 0 else m.arch.dim, device=m.device, dtype=torch.float32)
        p = lambda a: C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else C.c_void_p(a.data_ptr())
        _reset_counters()
        _lib.check(m._lib.f5hip_dit_forward(m._h, n, p(sl), p(kv), p(self.x), p(self.cond), p(tx), tx.shape[1], float(self.case["time"]), p(da),
                                            p(dt), k, p(out) if k < 0 else None, p(out) if k >= 0 else None, _lib.current_stream_ptr()),
                   "f5hip_dit_forward")
        self.launches[k] = _counters()
        return out.cpu()

    def added(self, k, k0):
        """GEMM launches of forward(k) that forward(k0) did not make"""
        return {name: v - self.launches[k0][name] for name, v in self.launches[k].items() if v != self.launches[k0][name]}

    def rows(self, i):
        f0 = sum(self.seq_len[:i])
        return slice(f0, f0 + self.seq_len[i])


class _Report:
    """Prints one [parity] line per comparison and collects the ones above the factor; the test asserts on them at its end, so one run shows
    every figure."""

    def __init__(self, label):
        self.label, self.bad, self.worst = label, [], (0.0, 0.0)

    def check(self, tag, got, exact, model):
        g, m = B.row_stats(got.double() - exact), B.row_stats(model - exact)
        ratio = (g[0] / m[0], g[1] / m[1])
        print(f"[parity] {self.label} {tag}: gpu_err rms {g[0]:.3e} worst row {g[1]:.3e}   model_err rms {m[0]:.3e} worst row {m[1]:.3e}   "
              f"gpu_err / model_err {ratio[0]:.2f} / {ratio[1]:.2f}   (ref rms {exact.pow(2).mean().sqrt():.3f})")
        self.worst = (max(self.worst[0], ratio[0]), max(self.worst[1], ratio[1]))
        if not (ratio[0] <= T.FACTOR and ratio[1] <= T.FACTOR):
            self.bad.append((tag, ratio))

    def finish(self):
        print(f"[parity] {self.label}: largest gpu_err / model_err {self.worst[0]:.2f} (rms) {self.worst[1]:.2f} (worst row)")
        assert not self.bad, self.bad


def _model(arch, sd, mode):
    from tts_indic_server_f5_amd.model import F5HipModel
    return F5HipModel(arch, sd, gemm_planes=mode)


def _block_gemms(mode, n_gemm, n_qkv, wide):
    """What block_qkv / block_out / block_ff must have launched for n_gemm GEMMs, n_qkv of them QKV.  Mode 3: gemm5, or gemm6 at the
    batch-mode shapes.  Mode 2: QKV always on gemm.h (128-wide tiles); the others on gemm3 up to 256 tiles, else on gemm.h (out / FF2
    64-wide, FF1 128-wide)."""
    if mode == 3:
        return {"gemm6" if wide else "gemm5": n_gemm}
    if not wide:
        return {"gemm3": n_gemm - n_qkv, "gemm_reg_bn128": n_qkv}
    rest = n_gemm - n_qkv          # out, FF1, FF2 per stream
    return {"gemm_reg_bn64": rest * 2 // 3, "gemm_reg_bn128": n_qkv + rest // 3}


def _recheck(label, mode, where, fn, exact, model):
    """The margins of test_block_reference.MUTATIONS at `where`, recomputed at the GPU's own input: fn(R, mut) is the reference there, and
    every mutation this mode claims must move it by MARGIN x the tolerance this test applies."""
    tol = {mode: T.FACTOR * B.row_stats(model - exact)[0]}
    names = [n for n, w, modes in T.MUTATIONS if w == where and mode in modes]
    for name, d, ratio in T.sensitivity(fn, exact, tol, names):
        print(f"[sensitivity] {label} mode {mode} {name} at {where}: rms {d:.3e}, {ratio[mode]:.2f} x the tolerance")
        assert ratio[mode] >= T.MARGIN, (name, where, ratio)


def _dit_case(mode, arch_kw, case, check_seqs, wide, label, recheck_sensitivity=False):
    from tts_indic_server_f5_amd.model import DiTArch
    sd = synth.dit_state_dict(**arch_kw)
    run = _Run(_model(DiTArch(**arch_kw), sd, mode), case)
    depth = arch_kw["depth"]
    hs = [run.forward(k) for k in range(depth + 1)]
    out = run.forward(-1)
    assert torch.equal(run.forward(1), hs[1]), "two identical calls differ"
    assert all(torch.isfinite(h).all() for h in hs + [out])
    for l in range(depth):
        assert run.added(l + 1, l) == _block_gemms(mode, 4, 1, wide), (l, run.added(l + 1, l))
    assert run.added(-1, depth) == {"gemm3": 1}, run.added(-1, depth)   # proj_out: split bf16 in both modes (128 columns: few tiles)
    W, R, rep = B.Weights(sd), B.MODES[mode], _Report(f"{label} mode {mode}")
    temb, temb_r, temb_2 = (B.time_embedding(W, case["time"], r) for r in (B.EXACT, R, B.MODE2))
    for i in check_seqs:
        rows, kv = run.rows(i), run.kv_len[i]
        for l in range(depth):
            hin = hs[l][rows].double()
            exact = B.dit_block(W, l, hin, temb, kv)
            model = B.dit_block(W, l, hin, temb_r, kv, R)
            rep.check(f"seq {i} (n {run.seq_len[i]}, kv {kv}) block {l}", hs[l + 1][rows], exact, model)
            if recheck_sensitivity and i == 0 and l == 0:
                _recheck(label, mode, "A", lambda r, mut=(): B.dit_block(W, 0, hin, temb, kv, r, mut), exact, model)
        hin = hs[depth][rows].double()
        exact, model = B.final_dit(W, hin, temb), B.final_dit(W, hin, temb_2, B.MODE2)
        rep.check(f"seq {i} final norm + proj_out", out[rows], exact, model)
        if recheck_sensitivity and i == 0:
            _recheck(label, mode, "A final", lambda r, mut=(): B.final_dit(W, hin, temb, r, mut), exact, model)
    rep.finish()
    return run


@_MODES
def test_dit_blocks_ragged(mode):
    """Case A: DiT 1024 / 16 heads / ff_mult 2, 3 blocks, one ragged call of (385, 129, 1, 255 with 200 keys): row_keep epilogue of block_out,
    zeroed rows, a one-row sequence, non-zero time, audio conditioning and text dropped once each.  Mode 3 on gemm5; mode 2 on gemm3 with
    gemm.h for QKV.
    Measured on an MI355X, largest gpu_err / model_err (rms / worst row): mode 2 1.29 / 1.37, mode 3 1.28 / 1.31.  Blocks in mode 2: gpu_err rms
    8e-6 .. 2.4e-5 on a stream of rms 1.8; in mode 3 1.5e-4, at 1.00 of the model.  Exact GELU sits at 2.6 x the mode-2 tolerance there."""
    _dit_case(mode, B.ARCH_A, B.CASE_A, range(4), False, "DiT ragged", recheck_sensitivity=True)


@_MODES
def test_dit_blocks_batch_mode(mode):
    """Case B: DiT 1024 / 16, 2 blocks, 26 sequences of 300 .. 450 frames (not all multiples of 16), >= 9 681 padded rows: in mode 3 all four
    block GEMMs take gemm6, in mode 2 out / FF1 / FF2 exceed 256 tiles and take gemm.h.  The reference is computed for the first sequence,
    the last one, and the first whose rows straddle a 176-row tile boundary that is no multiple of 128; all others must be finite.
    Measured on an MI355X, largest gpu_err / model_err (rms / worst row): mode 2 1.33 / 1.38, mode 3 1.34 / 1.38."""
    seq_len = B.CASE_B["seq_len"]
    row0 = np.concatenate(([0], np.cumsum([(n + 127) // 128 * 128 for n in seq_len])))
    assert row0[-1] >= 9681 and any(n % 16 for n in seq_len)
    mid = next(i for i in range(1, len(seq_len) - 1)
               if any(row0[i] < b < row0[i] + seq_len[i] and b % 128 for b in range(0, int(row0[-1]), 176)))
    _dit_case(mode, B.ARCH_B, B.CASE_B, (0, mid, len(seq_len) - 1), True, "DiT batch mode")


@_MODES
def test_unett_layers(mode):
    """Case C: UNetT 1024 / 16 / ff_mult 4, 4 layers, (200, 77 with 60 keys) frames behind the time token.  Layers 2 and 3 consume the skips
    saved in front of layers 1 and 0 (taken from the GPU's h_1 and h_0); the skip projection and the final RMSNorm + proj_out are split
    bf16 in both modes (one more gemm3 launch in layers 2 and 3).
    Measured on an MI355X, largest gpu_err / model_err (rms / worst row): mode 2 1.28 / 1.29, mode 3 1.29 / 1.26."""
    from tts_indic_server_f5_amd.model import UNetTArch
    case, depth = B.CASE_C, B.ARCH_C["depth"]
    sd = synth.unett_state_dict(**B.ARCH_C)
    run = _Run(_model(UNetTArch(**B.ARCH_C), sd, mode), case)
    hs = [run.forward(k) for k in range(depth + 1)]
    out = run.forward(-1)
    assert torch.equal(run.forward(1), hs[1]), "two identical calls differ"
    assert all(torch.isfinite(h).all() for h in hs + [out])
    for l in range(depth):
        want = _block_gemms(mode, 4, 1, False)
        if l >= depth // 2:
            want["gemm3"] = want.get("gemm3", 0) + 1          # the skip projection: split bf16 on gemm3 in every mode
        assert run.added(l + 1, l) == want, (l, run.added(l + 1, l))
    assert run.added(-1, depth) == {"gemm3": 1}, run.added(-1, depth)
    W, R, rep = B.Weights(sd), B.MODES[mode], _Report(f"UNetT mode {mode}")
    for i in range(len(run.seq_len)):
        rows, kv = run.rows(i), run.kv_len[i]
        tok = [B.time_embedding(W, case["time"])]             # the reference's own time-token row behind 0 .. depth layers
        full = lambda j: torch.cat((tok[j][None], hs[j][rows].double()))
        for l in range(depth):
            skip = full(depth - 1 - l) if l >= depth // 2 else None
            exact = B.unett_layer(W, l, depth, full(l), skip, kv)
            model = B.unett_layer(W, l, depth, full(l), skip, kv, R)
            tok.append(exact[0])
            rep.check(f"seq {i} (n {run.seq_len[i]}, kv {kv}) layer {l}", hs[l + 1][rows], exact[1:], model[1:])
            if i == 0 and l == depth - 1:   # its skip is the stream in front of layer 0; the slip takes layer 1's
                _recheck("UNetT", mode, "C", lambda r, mut=(): B.unett_layer(W, l, depth, full(l), full(1 if "skip_wrong_layer" in mut else 0),
                                                                            kv, r, mut), exact, model)
        rep.check(f"seq {i} final norm + proj_out", out[rows], B.final_unett(W, full(depth)), B.final_unett(W, full(depth), B.MODE2))
    rep.finish()


def _pad_text(text):
    text = text.clone()
    text[1, B.CASE_D["text_valid"][1]:] = -1
    return text


@_MODES
def test_mmdit_blocks(mode):
    """Case D: MMDiT 512 / 8 heads, 3 blocks, two sequences of 300 frames (233 keys in the second) with 61 text positions, -1 padding behind
    40 tokens in the second.  Both streams behind blocks 0 and 1 (the text stream through the "text_stream" tap), the audio stream behind
    the context-pre-only block 2, whose text stream is dropped.  (The library takes dim == 64 x heads only:
    test_mmdit_inner_width_other_than_dim_is_refused.)
    Measured on an MI355X, largest gpu_err / model_err (rms / worst row): mode 2 1.28 / 1.40, mode 3 1.28 / 1.30."""
    from tts_indic_server_f5_amd.model import MMDiTArch
    case, depth, D = B.CASE_D, B.ARCH_D["depth"], B.ARCH_D["dim"]
    sd = synth.mmdit_state_dict(**B.ARCH_D)
    run = _Run(_model(MMDiTArch(**B.ARCH_D), sd, mode), case, text=_pad_text)
    nt, S = case["nt"], len(run.seq_len)
    pitch = (nt + 127) // 128 * 128
    hs, cs = [], []
    for k in range(depth + 1):
        hs.append(run.forward(k))
        cs.append(run.model.read_tap("text_stream", S * pitch, D).cpu())
    out = run.forward(-1)
    again = run.forward(1)
    assert torch.equal(again, hs[1]) and torch.equal(run.model.read_tap("text_stream", S * pitch, D).cpu(), cs[1]), "two identical calls differ"
    assert all(torch.isfinite(h).all() for h in hs + cs + [out])
    for l in range(depth):
        want = _block_gemms(mode, 5, 2, False) if l == depth - 1 else _block_gemms(mode, 8, 2, False)
        assert run.added(l + 1, l) == want, (l, run.added(l + 1, l))
    assert run.added(-1, depth) == {"gemm3": 1}, run.added(-1, depth)
    W, R, rep = B.Weights(sd), B.MODES[mode], _Report(f"MMDiT mode {mode}")
    temb, temb_r, temb_2 = (B.time_embedding(W, case["time"], r) for r in (B.EXACT, R, B.MODE2))
    for i in range(S):
        rows, crow, kv = run.rows(i), slice(i * pitch, i * pitch + nt), run.kv_len[i]
        for l in range(depth):
            hin, cin = hs[l][rows].double(), cs[l][crow].double()
            ex_x, ex_c = B.mmdit_block(W, l, depth, hin, cin, temb, kv)
            mo_x, mo_c = B.mmdit_block(W, l, depth, hin, cin, temb_r, kv, R)
            rep.check(f"seq {i} (kv {kv}) block {l} audio stream", hs[l + 1][rows], ex_x, mo_x)
            if l < depth - 1:
                rep.check(f"seq {i} (kv {kv}) block {l} text stream", cs[l + 1][crow], ex_c, mo_c)
            else:
                assert ex_c is None
            if i == 1 and l == 0:
                fn = lambda r, mut=(): torch.cat(B.mmdit_block(W, 0, depth, hin, cin, temb, kv, r, mut, c_valid=case["text_valid"][1]))
                _recheck("MMDiT", mode, "D", fn, torch.cat((ex_x, ex_c)), torch.cat((mo_x, mo_c)))
        hin = hs[depth][rows].double()
        rep.check(f"seq {i} final norm + proj_out", out[rows], B.final_mmdit(W, hin, temb), B.final_mmdit(W, hin, temb_2, B.MODE2))
    rep.finish()


def test_mmdit_inner_width_other_than_dim_is_refused():
    """16 heads of 64 at dim 512 (inner width 1024): f5hip_dit_create supports dim == 64 x heads only and says so, it does not run."""
    from tts_indic_server_f5_amd._lib import F5HipError
    from tts_indic_server_f5_amd.model import F5HipModel, MMDiTArch
    with pytest.raises(F5HipError, match="unsupported backbone geometry"):
        F5HipModel(MMDiTArch(dim=512, depth=3, heads=16, text_num_embeds=100), {})


def test_text_stream_tap_arguments():
    """The "text_stream" tap is refused on a DiT handle and with a wrong element count."""
    from tts_indic_server_f5_amd._lib import F5HipError
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel, MMDiTArch
    tiny = dict(dim=128, depth=2, heads=2, ff_mult=2, text_num_embeds=40)
    g = torch.Generator().manual_seed(5)
    x, text = torch.randn(1, 20, 100, generator=g), torch.randint(0, 40, (1, 9), generator=g)
    mm = F5HipModel(MMDiTArch(**tiny), synth.mmdit_state_dict(**tiny))
    mm.transformer_forward(x, x, text, 0.5, False, False, n_blocks=1)
    assert mm.read_tap("text_stream", 128, 128).shape == (128, 128)
    with pytest.raises(F5HipError, match="text_stream"):
        mm.read_tap("text_stream", 127, 128)
    dit = dict(tiny, text_dim=64, conv_layers=2)
    d = F5HipModel(DiTArch(**dit), synth.dit_state_dict(**dit))
    d.transformer_forward(x, x, text, 0.5, False, False, n_blocks=1)
    with pytest.raises(F5HipError, match="text_stream"):
        d.read_tap("text_stream", 128, 128)
