"""Python face of the operations of the C ABI (include/f5hip.h) on torch tensors on the HIP device.  Two families:
  - the per-kernel unit ops (`gemm` .. `time_table`): one production HIP kernel each, fp32 in and out, called through ctypes.  Used by the
    per-kernel parity tests and the timing tools; not on the hot path.
  - the device audio path that every request takes (`ref_frontend`, `ref_prestep`, `ref_denoise`, `ref_assess`, `wave_finish` .. `wave_loudness`, `flac_decode`): one
    library call per batch.  Each is bound twice over the same C entry point: as a TORCH_LIBRARY operator (csrc/torch_ops.cpp), taken when
    `torch_ops.load()`, and through ctypes otherwise; both return the same bits.  The steps the wrappers share -- the operator call, the
    per-request host arrays, the PCM request table, its sources, the pointer table and the packing of the outputs -- are the helpers in
    front of them, and csrc/torch_ops.cpp holds the same helpers in C++."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, torch_ops
from .wave_codec import rate_pair

ACT = {"none": 0, "gelu_tanh": 1, "gelu_erf": 2, "mish": 3, "silu": 4}


def _p(t):
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return C.c_void_p(t.ctypes.data)
    return C.c_void_p(t.data_ptr())


def _f32(t, dev):
    return None if t is None else t.to(dev, torch.float32).contiguous()


def gemm(a, w, bias=None, *, prec=3, act="none", mul=None, res=None, row_keep=None, out16=False, w_copies=1, iters=0, bn=128):
    """out = (act(a @ w.T + bias), masked rows zeroed) * mul + res.  Returns (out, avg_us); out is fp32 [M, N], or the fp16 plane.
    bn: the column-tile width a call site passes to the dispatcher (128, or 64 as the residual and UNetT skip GEMMs do); only the
    register-staged gemm.h kernel reads it."""
    dev = a.device
    M, K = a.shape
    N = w.shape[0]
    a, w, bias, mul, res = (_f32(t, dev) for t in (a, w, bias, mul, res))
    out = torch.empty(M, N, device=dev, dtype=torch.float16 if out16 else torch.float32)
    keep = None if row_keep is None else np.ascontiguousarray(row_keep.cpu().numpy().astype(np.uint8))
    us = C.c_double(0.0)
    _lib.check(_lib.lib().f5hip_op_gemm(M, N, K, _p(a), _p(w), _p(bias), prec, ACT[act], _p(mul), _p(res), _p(keep),
                                        None if out16 else _p(out), _p(out) if out16 else None, w_copies, iters, C.byref(us),
                                        _lib.current_stream_ptr(), bn), "f5hip_op_gemm")
    return out, us.value


def qkv(a, w, bias, row_pos, *, prec=3, iters=0):
    """Fused QKV projection + epilogue.  Returns (q [M, D] (already scaled by log2(e) / 8), k [M, D], v [M, D]) as fp32 views of the fp16 outputs, avg_us."""
    dev = a.device
    M, D = a.shape
    M_pad = (M + 127) // 128 * 128
    a, w, bias = (_f32(t, dev) for t in (a, w, bias))
    qk = torch.zeros(M_pad, 2 * D, device=dev, dtype=torch.float16)
    vt = torch.zeros(D, M_pad, device=dev, dtype=torch.float16)
    pos = np.ascontiguousarray(np.asarray(row_pos, dtype=np.int32))
    us = C.c_double(0.0)
    _lib.check(_lib.lib().f5hip_op_qkv(M, D, _p(a), _p(w), _p(bias), _p(pos), prec, _p(qk), _p(vt), iters, C.byref(us),
                                       _lib.current_stream_ptr()), "f5hip_op_qkv")
    # V^T keeps the tokens of every aligned group of 16 in the order 0-3, 8-11, 4-7, 12-15 (csrc/common.h vt_col): undo it for the caller
    t = torch.arange(M_pad, device=dev)
    col = (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)
    return qk[:M, :D].float(), qk[:M, D:].float(), vt[:, col[:M]].t().float(), us.value


def layernorm(x, scale, shift, *, gain_off=1.0, eps=1e-6, rms=False):
    dev = x.device
    M, D = x.shape
    x, scale, shift = (_f32(t, dev) for t in (x, scale, shift))
    out = torch.empty_like(x)
    _lib.check(_lib.lib().f5hip_op_layernorm(M, D, _p(x), _p(scale), _p(shift), float(gain_off), float(eps), int(rms), _p(out),
                                             _lib.current_stream_ptr()), "f5hip_op_layernorm")
    return out


# output formats of the attention unit ops (what the kernel writes; the op returns it as fp32): split-bf16 planes, one fp16 plane (the
# blocks' fp16 GEMM mode), the bf16 hi plane alone (bf16 GEMM mode)
ATTN_OUT_SPLIT, ATTN_OUT_F16, ATTN_OUT_BF16 = 0, 1, 2


def attention(q, k, v, seq_len, kv_len=None, *, heads, impl=3, iters=0, shape_invariant=-1, out_format=ATTN_OUT_SPLIT):
    """softmax(q k^T / 8 + key mask) v per (sequence, head); q / k / v fp32 [sum(seq_len), 64 * heads] packed.  Returns (out, avg_us).
    impl must be 3 (attn3, the production kernel); shape_invariant 1 / 0 / -1 (the process default, f5hip_set_attention_shape_invariant)."""
    dev = q.device
    q, k, v = (_f32(t, dev) for t in (q, k, v))
    out = torch.empty_like(q)
    sl = np.ascontiguousarray(np.asarray(seq_len, dtype=np.int32))
    kl = None if kv_len is None else np.ascontiguousarray(np.asarray(kv_len, dtype=np.int32))
    us = C.c_double(0.0)
    _lib.check(_lib.lib().f5hip_op_attention(len(sl), _p(sl), _p(kl), heads, _p(q), _p(k), _p(v), _p(out), impl, iters, C.byref(us),
                                             _lib.current_stream_ptr(), int(shape_invariant), int(out_format)), "f5hip_op_attention")
    return out, us.value


def conv1d(x, weight, bias=None, res=None, *, batch, valid, dilation=1, prec=2, impl=5, iters=0, stamps=False):
    """One BigVGAN-style Conv1d over channel-last rows.  x fp32 [batch * P, c_in] (P = rows per sequence, a multiple of 128; `valid`
    rows of each are real, the rest is padding), weight [c_out, c_in, k] (nn.Conv1d layout), `same` zero padding at the sequence bounds.
    Returns (out [batch * P, c_out], avg_us, stamps | None); impl 0 = implicit GEMM, 5 = sliding-window kernel."""
    dev = x.device
    x = _f32(x, dev)
    c_out, c_in, k = weight.shape
    M = x.shape[0]
    P = M // batch
    w = np.ascontiguousarray(weight.detach().to(torch.float32).cpu().numpy())
    b = None if bias is None else np.ascontiguousarray(bias.detach().to(torch.float32).cpu().numpy())
    r = None if res is None else _f32(res, dev)
    out = torch.empty(M, c_out, dtype=torch.float32, device=dev)
    us = C.c_double(0.0)
    nblk = (M // 256) * ((c_out + 127) // 128)
    st = np.zeros((nblk, 16), dtype=np.uint64) if stamps else None
    _lib.check(_lib.lib().f5hip_op_conv1d(batch, P, valid, c_in, c_out, k, dilation, _p(x), _p(w), _p(b), _p(r), _p(out), prec, impl, iters,
                                          C.byref(us), _p(st), nblk, _lib.current_stream_ptr()), "f5hip_op_conv1d")
    return out, us.value, st


# output formats of the BigVGAN snake op: fp32 rows, split-bf16 planes, one fp16 plane
SNAKE_OUT_F32, SNAKE_OUT_SPLIT, SNAKE_OUT_F16 = 0, 1, 2


def bigvgan_snake(x, alpha_log, beta_log, *, batch, valid, out_format=SNAKE_OUT_F32, out=None):
    """The generator's Activation1d(SnakeBeta) over channel-last rows x fp32 [batch * P, C] (`valid` rows of each sequence are real).
    out: optional fp32 [rows >= batch * P, C] the op writes into (rows it does not compute keep their contents, up to the format's
    rounding); returns it."""
    dev = x.device
    x, alpha_log, beta_log = (_f32(t, dev) for t in (x, alpha_log, beta_log))
    M, Cc = x.shape
    if out is None:
        out = torch.zeros(M, Cc, dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[1] == Cc and out.shape[0] >= M
    _lib.check(_lib.lib().f5hip_op_bigvgan_snake(batch, M // batch, valid, Cc, _p(x), _p(alpha_log), _p(beta_log), out_format, _p(out),
                                                 out.shape[0], _lib.current_stream_ptr()), "f5hip_op_bigvgan_snake")
    return out


def bigvgan_upsample(x, weight, bias=None, *, batch, valid, rate, prec=2):
    """One generator up-sampler, ConvTranspose1d(c_in, c_out, 2 rate, stride rate, padding rate / 2) + bias, over channel-last rows
    x fp32 [batch * P, c_in] (P % 128 == 0); weight [c_in, c_out, 2 rate] (nn.ConvTranspose1d layout).  Returns [batch * P * rate, c_out]."""
    dev = x.device
    x = _f32(x, dev)
    c_in, c_out, k = weight.shape
    assert k == 2 * rate
    M = x.shape[0]
    w = np.ascontiguousarray(weight.detach().to(torch.float32).cpu().numpy())
    b = None if bias is None else np.ascontiguousarray(bias.detach().to(torch.float32).cpu().numpy())
    out = torch.empty(M * rate, c_out, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().f5hip_op_bigvgan_upsample(batch, M // batch, valid, c_in, c_out, rate, _p(x), _p(w), _p(b), _p(out), prec,
                                                    _lib.current_stream_ptr()), "f5hip_op_bigvgan_upsample")
    return out


def bigvgan_conv_post(a, weight, *, batch, valid, variant=0):
    """The generator's conv_post (Conv1d(C, 1, 7, padding 3), no bias) + clamp(-1, 1) over channel-last rows a fp32 [batch * P, C];
    weight [1, C, 7] or [C, 7].  variant 0 = the generator's choice, 1 = LDS-tiled kernel, 2 = the kernel without the tile.
    Returns wave [batch, valid]."""
    dev = a.device
    a = _f32(a, dev)
    M, Cc = a.shape
    w = _f32(weight.reshape(Cc, 7), dev)
    wave = torch.empty(batch, valid, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().f5hip_op_bigvgan_conv_post(batch, M // batch, valid, Cc, _p(a), _p(w), variant, _p(wave), _lib.current_stream_ptr()),
               "f5hip_op_bigvgan_conv_post")
    return wave


def conv1d_ragged(x, weight, bias=None, res=None, *, row0, valid, rows=None, blk, dilation=1, prec=2, impl=5, ups_rate=0):
    """conv1d() over ragged items, the layout of the ragged BigVGAN forward: x fp32 [M, c_in]; item i owns rows [row0[i], + rows[i]) (rows
    None: valid rounded up to the alignment), the first valid[i] of them real; the kernels read one [start, end) per block of blk rows.
    ups_rate > 0: the 3-tap form of an up-sampler, weight [c_in, c_out, 2 ups_rate] as in bigvgan_upsample(), out [M ups_rate, c_out].
    Layouts the kernels exclude are refused (include/f5hip.h).  Returns out."""
    dev = x.device
    x = _f32(x, dev)
    M = x.shape[0]
    if ups_rate:
        c_in, c_out, k = weight.shape
        assert k == 2 * ups_rate
    else:
        c_out, c_in, k = weight.shape
    w = np.ascontiguousarray(weight.detach().to(torch.float32).cpu().numpy())
    b = None if bias is None else np.ascontiguousarray(bias.detach().to(torch.float32).cpu().numpy())
    r = None if res is None else _f32(res, dev)
    r0, rw, vl = _i32(row0), _i32(rows), _i32(valid)
    assert len(vl) == len(r0) and (rw is None or len(rw) == len(r0))
    out = torch.empty(M * max(ups_rate, 1), c_out, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().f5hip_op_conv1d_ragged(len(r0), _p(r0), _p(rw), _p(vl), M, blk, c_in, c_out, k, dilation, ups_rate, _p(x), _p(w), _p(b),
                                                 _p(r), _p(out), prec, impl, _lib.current_stream_ptr()), "f5hip_op_conv1d_ragged")
    return out


def bigvgan_snake_ragged(x, alpha_log, beta_log, *, row0, valid, scale, out_format=SNAKE_OUT_F32, out=None):
    """bigvgan_snake() over ragged items: item i = rows [row0[i], + valid[i]) of x fp32 [M, C], multiples of `scale` (the kernel's item
    table is in first-stage rows).  out as in bigvgan_snake(); returns it."""
    dev = x.device
    x, alpha_log, beta_log = (_f32(t, dev) for t in (x, alpha_log, beta_log))
    M, Cc = x.shape
    if out is None:
        out = torch.zeros(M, Cc, dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[1] == Cc and out.shape[0] >= M
    r0, vl = _i32(row0), _i32(valid)
    assert len(vl) == len(r0)
    _lib.check(_lib.lib().f5hip_op_bigvgan_snake_ragged(len(r0), _p(r0), _p(vl), scale, M, Cc, _p(x), _p(alpha_log), _p(beta_log), out_format,
                                                        _p(out), out.shape[0], _lib.current_stream_ptr()), "f5hip_op_bigvgan_snake_ragged")
    return out


def bigvgan_conv_post_ragged(a, weight, wave, *, row0, valid, wave_off, scale, variant=0):
    """bigvgan_conv_post() over ragged items: item i = rows [row0[i], + valid[i]) of a fp32 [M, C] -> samples [wave_off[i], + valid[i]) of
    `wave` (fp32, 1-D, on the device; written in place, nothing else of it is touched).  Returns wave."""
    dev = a.device
    a = _f32(a, dev)
    M, Cc = a.shape
    w = _f32(weight.reshape(Cc, 7), dev)
    assert wave.dtype == torch.float32 and wave.is_contiguous() and wave.dim() == 1 and wave.device == dev
    r0, vl, wo = _i32(row0), _i32(valid), _i32(wave_off)
    assert len(vl) == len(r0) == len(wo)
    _lib.check(_lib.lib().f5hip_op_bigvgan_conv_post_ragged(len(r0), _p(r0), _p(vl), _p(wo), scale, M, Cc, _p(a), _p(w), variant, _p(wave),
                                                            wave.numel(), _lib.current_stream_ptr()), "f5hip_op_bigvgan_conv_post_ragged")
    return wave


# plane modes of bigvgan_mean3: none, split bf16, one fp16 plane, the bf16 hi plane alone
MEAN3_NONE, MEAN3_SPLIT, MEAN3_F16, MEAN3_BF16 = 0, 1, 2, 3


def bigvgan_mean3(ys, *, mode=MEAN3_NONE, planes=None, want_f32=True):
    """The generator's mean of a stage's three AMP blocks: ys = 3 fp32 [rows, C] tensors ((y0 + y1 + y2) / 3) or 1 (its conversion).
    mode > 0: `planes` fp32 [rows, ldo >= C] is loaded into operand planes of that mode, the kernel writes channels < C, and the planes
    come back in it as fp32.  Returns (fp32 rows [rows, C] | None, planes | None)."""
    dev = ys[0].device
    ys = [_f32(y, dev) for y in ys]
    rows, Cc = ys[0].shape
    out = torch.empty(rows, Cc, dtype=torch.float32, device=dev) if want_f32 or mode == 0 else None
    ldo = 0
    if mode:
        assert planes.dtype == torch.float32 and planes.is_contiguous() and planes.shape[0] == rows and planes.device == dev
        ldo = planes.shape[1]
    y = ys + [None, None]
    _lib.check(_lib.lib().f5hip_op_bigvgan_mean3(rows, Cc, len(ys), _p(y[0]), _p(y[1]), _p(y[2]), mode, ldo, _p(out), _p(planes) if mode else None,
                                                 _lib.current_stream_ptr()), "f5hip_op_bigvgan_mean3")
    return out, planes if mode else None


def bigvgan_mel_rows(mel, *, rows, row0=None, frames=None, f16=False):
    """The generator's first operand planes as fp32 [rows, 128]: mel fp32 [n, C, T] -> one row of 128 channels per frame.  row0 None: n
    uniform sequences of T frames at pitch rows / n.  Else the ragged kernel: item i has frames[i] <= T frames from row row0[i] (a
    multiple of 128) and T is the column stride."""
    dev = mel.device
    mel = _f32(mel, dev)
    n, Cc, T = mel.shape
    out = torch.empty(rows, 128, dtype=torch.float32, device=dev)
    r0, fr = _i32(row0), _i32(frames)
    assert r0 is None or (fr is not None and len(r0) == len(fr) == n)
    _lib.check(_lib.lib().f5hip_op_bigvgan_mel_rows(n, _p(r0), _p(fr), T, rows, Cc, _p(mel), int(f16), _p(out), _lib.current_stream_ptr()),
               "f5hip_op_bigvgan_mel_rows")
    return out


def joint_attention(q, k, v, x_len, c_len, x_kvlen=None, *, heads, shape_invariant=-1, out_format=ATTN_OUT_SPLIT):
    """MMDiT joint attention: per sequence softmax(q [x ; c] k^T / 8 + mask on the padded audio keys) v over the concatenation of its audio
    rows and its text rows.  q / k / v fp32 [sum(x_len) + sum(c_len), 64 * heads]: all audio frames first, then all text tokens.
    shape_invariant and out_format as in attention()."""
    dev = q.device
    q, k, v = (_f32(t, dev) for t in (q, k, v))
    out = torch.empty_like(q)
    xl = np.ascontiguousarray(np.asarray(x_len, dtype=np.int32))
    cl = np.ascontiguousarray(np.asarray(c_len, dtype=np.int32))
    kl = None if x_kvlen is None else np.ascontiguousarray(np.asarray(x_kvlen, dtype=np.int32))
    _lib.check(_lib.lib().f5hip_op_joint_attention(len(xl), _p(xl), _p(kl), _p(cl), heads, _p(q), _p(k), _p(v), _p(out), _lib.current_stream_ptr(),
                                                   int(shape_invariant), int(out_format)), "f5hip_op_joint_attention")
    return out


def _host_f32(t):
    return np.ascontiguousarray(t.detach().to(torch.float32).cpu().numpy())


def conv_pos_embed(x, w1, b1, w2, b2, *, seq_len, lead=0, impl=5, prec=2, taps=False, pad_nan=False):
    """The backbone's ConvPositionEmbedding plus its residual, x + Mish(conv2(Mish(conv1(x)))), over packed sequences x fp32 [sum(seq_len), D];
    weights [D, D / 16, 31] (nn.Conv1d, groups 16), biases [D].  lead=1: the UNetT layout (a time-token row heads every sequence).
    impl 5 = conv5.h, 0 = gemm.h; prec 2 = split bf16, 1 = bf16.  pad_nan: NaN instead of 0 in the padding rows, the time-token rows and
    the slack behind the internal buffers.  Returns out, or (out, stage 1 as the second convolution reads it) with taps."""
    dev = x.device
    x = _f32(x, dev)
    frames, D = x.shape
    sl = np.ascontiguousarray(np.asarray(seq_len, dtype=np.int32))
    assert int(sl.sum()) == frames
    hw = [_host_f32(t) for t in (w1, b1, w2, b2)]
    out = torch.empty(frames, D, dtype=torch.float32, device=dev)
    c1 = torch.empty(frames, D, dtype=torch.float32, device=dev) if taps else None
    _lib.check(_lib.lib().f5hip_op_conv_pos_embed(len(sl), _p(sl), int(lead), D, _p(x), *(_p(a) for a in hw), int(impl), int(prec), int(pad_nan),
                                                  _p(out), _p(c1), _lib.current_stream_ptr()), "f5hip_op_conv_pos_embed")
    return (out, c1) if taps else out


CONVNEXT_PARAMS = ("dwconv.weight", "dwconv.bias", "norm.weight", "norm.bias", "pwconv1.weight", "pwconv1.bias", "grn.gamma", "grn.beta",
                   "pwconv2.weight", "pwconv2.bias")


def convnext_block(x, params, *, seq_len, taps=False, pad_nan=False):
    """One ConvNeXtV2 text block of the backbone over packed sequences x fp32 [sum(seq_len), Td]; params: the block's tensors by their
    state-dict suffix (CONVNEXT_PARAMS).  Returns out, or (out, {"ln", "ty", "grn", "gx"}) with taps: each stage as the next kernel reads it,
    and gx [len(seq_len), 2 Td], the GRN column norms of every sequence."""
    dev = x.device
    x = _f32(x, dev)
    n, Td = x.shape
    sl = np.ascontiguousarray(np.asarray(seq_len, dtype=np.int32))
    assert int(sl.sum()) == n
    hp = [_host_f32(params[k]).reshape(-1) for k in CONVNEXT_PARAMS]
    arr = (C.c_void_p * 10)(*(a.ctypes.data for a in hp))
    out = torch.empty(n, Td, dtype=torch.float32, device=dev)
    tp = {"ln": torch.empty(n, Td, dtype=torch.float32, device=dev), "ty": torch.empty(n, 2 * Td, dtype=torch.float32, device=dev),
          "grn": torch.empty(n, 2 * Td, dtype=torch.float32, device=dev),
          "gx": torch.empty(len(sl), 2 * Td, dtype=torch.float32, device=dev)} if taps else {}
    _lib.check(_lib.lib().f5hip_op_convnext_block_gx(len(sl), _p(sl), Td, _p(x), arr, int(pad_nan), _p(out), _p(tp.get("ln")), _p(tp.get("ty")),
                                                     _p(tp.get("grn")), _p(tp.get("gx")), _lib.current_stream_ptr()), "f5hip_op_convnext_block_gx")
    return (out, tp) if taps else out


def _i32(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _col_ptr(table, col):
    """Pointer to column `col` of row 0 of a contiguous fp32 device table."""
    assert table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 2
    return C.c_void_p(table.data_ptr() + 4 * int(col))


def gemm_rowmul(a, w, bias, table, col, row_mod, res, *, prec=3, row_keep=None, bn=64):
    """f5hip_op_gemm_rowmul: out = ((a @ w.T + bias), masked rows zeroed) * table[row_mod[r], col : col + N] + res, the per-row-multiplier
    epilogue of the gated residual projections.  table fp32 [T, mod_ld] on the device, row_mod int [M]; bn as in gemm() (the model's
    residual call sites pass 64).  Returns out fp32 [M, N]."""
    dev = a.device
    M, K = a.shape
    N = w.shape[0]
    a, w, bias, res = (_f32(t, dev) for t in (a, w, bias, res))
    assert table.device == a.device and col + N <= table.shape[1]
    out = torch.empty(M, N, device=dev, dtype=torch.float32)
    keep = None if row_keep is None else np.ascontiguousarray(row_keep.cpu().numpy().astype(np.uint8))
    rm = _i32(row_mod)
    assert rm.shape == (M,)
    _lib.check(_lib.lib().f5hip_op_gemm_rowmul(M, N, K, _p(a), _p(w), _p(bias), prec, _col_ptr(table, col), _p(rm), table.shape[1], table.shape[0],
                                               _p(res), _p(keep), _p(out), _lib.current_stream_ptr(), bn), "f5hip_op_gemm_rowmul")
    return out


# output formats of layernorm_planes (what the kernel writes; the op returns it as fp32): split-bf16 planes, one fp16 plane
LN_OUT_SPLIT, LN_OUT_F16 = 0, 1


def layernorm_planes(x, scale, shift, *, out_format=LN_OUT_SPLIT, gain_off=1.0, eps=1e-6, table=None, row_mod=None):
    """LayerNorm + modulation through the 16-bit plane outputs the GEMMs read, returned as fp32.  Plain: scale / shift fp32 [D].  Per row
    (table fp32 [T, mod_ld] on the device, row_mod int [M]): scale / shift are COLUMN OFFSETS into the table and row r takes
    table[row_mod[r], scale : scale + D] and table[row_mod[r], shift : shift + D]."""
    dev = x.device
    M, D = x.shape
    x = _f32(x, dev)
    out = torch.empty_like(x)
    if table is None:
        scale, shift = _f32(scale, dev), _f32(shift, dev)
        ps, ph, rm, ld, nrow = _p(scale), _p(shift), None, 0, 0
    else:
        assert table.device == x.device and max(scale, shift) + D <= table.shape[1]
        rm = _i32(row_mod)
        assert rm.shape == (M,)
        ps, ph, ld, nrow = _col_ptr(table, scale), _col_ptr(table, shift), table.shape[1], table.shape[0]
    _lib.check(_lib.lib().f5hip_op_layernorm_planes(M, D, _p(x), ps, ph, _p(rm), ld, nrow, float(gain_off), float(eps), int(out_format), _p(out),
                                                    _lib.current_stream_ptr()), "f5hip_op_layernorm_planes")
    return out


CFG_EULER, CFG_RK4, CFG_NO_STEP = 0, 2, -1


def cfg_step(method, stage, xout, xbase, pred, urow_c, urow_u, xs, *, cfg=0.0, cfg_frame=None, dt=0.0, frame_unit=None, unit_dt=None, n_act=0,
             k=(None, None, None), final_flags=None, cond=None):
    """One launch of the sampler's CFG combine + ODE update IN PLACE on the caller's fp32 device tensors (include/f5hip.h f5hip_op_cfg_step):
    xout / xbase / k [U, mel], pred / xs [rows, 128].  final_flags (uint8 [U]) + cond: also the final select, whose result is returned."""
    U, mel = xbase.shape
    for t in (xout, xbase, pred, xs, cfg_frame, cond) + tuple(k):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda)
    uc, uu = (None if a is None else _i32(a) for a in (urow_c, urow_u))
    fu = None if frame_unit is None else _i32(frame_unit)
    ud = None if unit_dt is None else np.ascontiguousarray(np.asarray(unit_dt, dtype=np.float32))
    ff = None if final_flags is None else np.ascontiguousarray(np.asarray(final_flags, dtype=np.uint8))
    out = torch.empty_like(xbase) if ff is not None else None
    _lib.check(_lib.lib().f5hip_op_cfg_step(int(method), int(stage), U, mel, 0 if pred is None else pred.shape[0], _p(xout), _p(xbase), _p(pred), _p(uc),
                                            _p(uu), float(cfg), _p(cfg_frame), float(dt), _p(fu), _p(ud), 0 if ud is None else len(ud), int(n_act),
                                            _p(k[0]), _p(k[1]), _p(k[2]), _p(xs), _p(ff), _p(cond), _p(out), _lib.current_stream_ptr()),
               "f5hip_op_cfg_step")
    return out


# op codes of cfg_mixed (csrc/elementwise.h CfgOp): RK4 stage s is CFG_OP_RK4_1 + s - 1
CFG_OP_NONE, CFG_OP_EULER, CFG_OP_MID_HALF, CFG_OP_MID_FULL, CFG_OP_RK4_1 = 0, 1, 2, 3, 4


def cfg_mixed(xstate, pred, urow_c, urow_u, xs, cfg_frame, frame_unit, unit_op, unit_dt, n_act, k):
    """One launch of the CFG combine + ODE update of a mixed-method sampler call IN PLACE on the caller's fp32 device tensors (include/f5hip.h
    f5hip_op_cfg_mixed): xstate / k[0..2] [U, mel], pred / xs [rows, 128], cfg_frame [U]; frame_unit [U], unit_op / unit_dt [n_units] on the
    host: every frame is stepped by its unit's op code and step size."""
    U, mel = xstate.shape
    for t in (xstate, pred, xs, cfg_frame) + tuple(k):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda
    uc, uu, fu, uo = (_i32(a) for a in (urow_c, urow_u, frame_unit, unit_op))
    ud = np.ascontiguousarray(np.asarray(unit_dt, dtype=np.float32))
    assert uo.shape == ud.shape and fu.shape == (U,)
    _lib.check(_lib.lib().f5hip_op_cfg_mixed(U, mel, pred.shape[0], _p(xstate), _p(pred), _p(uc), _p(uu), _p(cfg_frame), _p(fu), _p(uo), _p(ud), len(uo),
                                             int(n_act), _p(k[0]), _p(k[1]), _p(k[2]), _p(xs), _lib.current_stream_ptr()), "f5hip_op_cfg_mixed")


def row_tp(row_unit, unit_tp):
    """row_tp[r] = unit_tp[row_unit[r]] by the sampler's kernel; int arrays in, numpy int32 out."""
    ru, ut = _i32(row_unit), _i32(unit_tp)
    out = np.full(ru.shape, -1, dtype=np.int32)
    _lib.check(_lib.lib().f5hip_op_row_tp(len(ru), _p(ru), len(ut), _p(ut), _p(out), _lib.current_stream_ptr()), "f5hip_op_row_tp")
    return out


def time_table(model, t):
    """The time precompute of a model.F5HipModel over the time points t (at most 256): (sinus [n_t, 256] as the time MLP reads it, mod
    [n_t, n_adaln] the AdaLN modulation rows or None (UNetT), temb [n_t, dim] the time embeddings (UNetT) or None)."""
    from .model import MMDiTArch, UNetTArch
    arch, dev = model.arch, model.device
    th = np.ascontiguousarray(np.asarray(t, dtype=np.float32))
    n_t, D = len(th), arch.dim
    unett = isinstance(arch, UNetTArch)
    cols = 0 if unett else (6 * arch.depth + 2) * D + ((6 * (arch.depth - 1) + 2) * D if isinstance(arch, MMDiTArch) else 0)
    sinus = torch.empty(n_t, 256, device=dev, dtype=torch.float32)
    mod = None if unett else torch.empty(n_t, cols, device=dev, dtype=torch.float32)
    temb = torch.empty(n_t, D, device=dev, dtype=torch.float32) if unett else None
    _lib.check(_lib.lib().f5hip_op_time_table(model._h, _p(th), n_t, _p(sinus), _p(mod), cols, _p(temb), _lib.current_stream_ptr()),
               "f5hip_op_time_table")
    return sinus, mod, temb


# ------------------------------------------------------------------------------------------------ the steps the audio operations share
def call_op(name, *args):
    """The TORCH_LIBRARY operator `name` over the same C entry point as the ctypes call next to it; a c10::Error from the operator's checks
    or the library is an F5HipError, as the ctypes path raises."""
    try:
        return getattr(torch_ops.ops(), name)(*args)
    except RuntimeError as e:
        raise _lib.F5HipError(str(e)) from e


def _per_request(op, what, values, dtype, n=None, per="request"):
    """Contiguous host array of `dtype` with one value per request: `n` of them, or (None: the array that sets the count) at least one."""
    a = np.ascontiguousarray(np.asarray(values, dtype=dtype))
    if a.ndim < 1 or len(a) < 1 or (n is not None and len(a) != n):
        raise _lib.F5HipError(f"{op}: {what} needs one value per {per} ({'at least one' if n is None else n}), got {a.shape}")
    return a


def _check_dev_f32(op, t, name):
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda):
        raise _lib.F5HipError(f"{op}: {name} must be a contiguous fp32 tensor on the HIP device")


def pointer_table(op, tensors, what):
    """A `Tensor[]` argument the library reads through a pointer table: every one a contiguous 1-D fp32 tensor on the first one's device.
    Returns (pointers uint64, lengths int32) as the ctypes path passes them; the length rules are the caller's."""
    for i, t in enumerate(tensors):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.is_cuda and t.dim() == 1 and t.is_contiguous() and t.device == tensors[0].device):
            raise _lib.F5HipError(f"{op}: {what} {i} must be a contiguous 1-D fp32 tensor on one HIP device (no CPU fallback)")
    return np.array([t.data_ptr() for t in tensors], dtype=np.uint64), np.array([t.numel() for t in tensors], dtype=np.int32)


def _pcm_requests(op, pcm, in_off, max_len, len_dev, several=False):
    """The request table (pcm, in_off, max_len, len_dev) of the wave operations: one offset and one length bound per request; `pcm` one
    contiguous 1-D int16 device tensor or, where the operation allows `several`, one per request on one device; `len_dev` None or int32 on
    that device with one value per request.  Returns (tensors, in_off int64, max_len int32, n, len_dev contiguous)."""
    tensors = list(pcm) if several and not torch.is_tensor(pcm) else [pcm]
    ml = _per_request(op, "max_len", max_len, np.int32)
    n = len(ml)
    io = _per_request(op, "in_off", in_off, np.int64, n)
    if len(tensors) not in (1, n):
        raise _lib.F5HipError(f"{op}: pcm is one tensor or one per request (got {len(tensors)} for {n})")
    for t in tensors:
        if not (torch.is_tensor(t) and t.dtype == torch.int16 and t.is_cuda and t.dim() == 1 and t.is_contiguous() and t.device == tensors[0].device):
            raise _lib.F5HipError(f"{op}: pcm must be contiguous 1-D int16 tensors on one HIP device")
    if len_dev is not None:
        if not (torch.is_tensor(len_dev) and len_dev.dtype == torch.int32 and len_dev.is_cuda and len_dev.numel() == n and len_dev.device == tensors[0].device):
            raise _lib.F5HipError(f"{op}: len_dev must be an int32 tensor with one value per request on the pcm's device")
        len_dev = len_dev.contiguous()
    return tensors, io, ml, n, len_dev


def _pcm_sources(op, tensors, io, ml):
    """Where the ctypes path reads a request table from: request i reads samples [in_off[i], in_off[i] + max_len[i]) of its tensor (the one
    tensor, or tensor i), which must hold them.  Returns (anchor, rel): the first tensor that has an address -- the library's `pcm` -- and
    every request's first sample relative to it."""
    anchor = next((t for t in tensors if t.numel()), None)
    if anchor is None:
        anchor = torch.zeros(8, device=tensors[0].device, dtype=torch.int16)
    base, rel = anchor.data_ptr(), np.zeros(len(ml), dtype=np.int64)
    for i in range(len(ml)):
        t = tensors[0 if len(tensors) == 1 else i]
        if ml[i] < 0 or io[i] < 0 or int(io[i]) + int(ml[i]) > t.numel():
            raise _lib.F5HipError(f"{op}: request {i} reads samples [{io[i]}, {int(io[i]) + int(ml[i])}) of a tensor of {t.numel()}")
        rel[i] = (t.data_ptr() - base) // 2 + int(io[i]) if ml[i] else 0   # (an empty tensor has no address to speak of)
    return anchor, rel


def _pack(sizes, align):
    """Outputs packed in request order, each at a multiple of `align`: (offsets, total)."""
    offsets, total = [], 0
    for s in sizes:
        offsets.append(total)
        total += (int(s) + align - 1) & -align
    return offsets, total


# ------------------------------------------------------------------------------------------------ the audio operations
def ref_frontend(wave, n_in, channels, orig_freq, new_freq, taps=None, rms_floor=0.1):
    """The reference-audio front-end of several clips of one sample-rate pair in ONE library call (include/f5hip.h f5hip_ref_frontend): mono
    mix, rms, gain up to `rms_floor`, polyphase sinc resampling.  wave: fp32 device tensor, the clips packed back to back, clip i as
    channels[i] planes of n_in[i] samples; taps: fp32 device [nf, 2 width + of] (`infer.resample_taps`), not needed when the rates are
    equal.  Returns (out packed fp32 device, rms [n] fp32 device -- measured before the gain --, [n_out_i]); clip i's part of `out` and its
    rms equal its own call's, bit for bit."""
    ni = _per_request("ref_frontend", "n_in", n_in, np.int32, per="clip")
    ch = _per_request("ref_frontend", "channels", channels, np.int32, len(ni), per="clip")
    _check_dev_f32("ref_frontend", wave, "wave")
    if taps is not None:
        _check_dev_f32("ref_frontend", taps, "taps")
    of, nf, _, L = rate_pair(orig_freq, new_freq)
    n_out = [(nf * int(v) + of - 1) // of for v in ni]
    if of != nf:   # the library derives the row length itself (csrc/rate_pair.h): refuse a table of another shape
        if taps is None or tuple(taps.shape) != (nf, L):
            raise _lib.F5HipError(f"ref_frontend: taps must be [{nf}, {L}] for {orig_freq} -> {new_freq} Hz "
                                  f"(got {None if taps is None else tuple(taps.shape)})")
    if torch_ops.load():
        out, rms = call_op("ref_frontend", wave, torch.from_numpy(ni), torch.from_numpy(ch), int(orig_freq), int(new_freq), taps, float(rms_floor))
    else:
        if int((ni.astype(np.int64) * ch).sum()) != wave.numel():
            raise _lib.F5HipError("ref_frontend: wave needs sum(n_in * channels) samples")
        with torch.cuda.device(wave.device):
            out = torch.empty(max(sum(n_out), 0), device=wave.device, dtype=torch.float32)
            rms = torch.empty(len(ni), device=wave.device, dtype=torch.float32)
            _lib.check(_lib.lib().f5hip_ref_frontend(len(ni), _p(ni), _p(ch), _p(wave), int(orig_freq), int(new_freq), _p(taps), float(rms_floor),
                                                     _p(out), _p(rms), _lib.current_stream_ptr()), "f5hip_ref_frontend")
    return out, rms, n_out


def ref_prestep(frames, n_in, channels, rate, clip_short=True, device=None):
    """The reference-clip pre-step of several clips of ONE sample rate in one library call and three launches (include/f5hip.h
    f5hip_ref_prestep): `audio_prep.preprocess_ref_segment` of each clip -- clip at a pause, strip the silent edges, append 50 ms of silence --
    bit for bit.  frames: the clips' int16 frames, interleaved as `PcmSegment` holds them and packed back to back: a host array (uploaded
    once, to `device`) or a 1-D int16 device tensor; n_in, channels: one value per clip (a clip of 0 frames is valid); clip_short: one bool, or
    one per clip.  Returns (packed fp32 device tensor: clip i as channels[i] planes of lengths[i] samples, x / 32768, packed by those lengths
    -- `ref_frontend`'s `wave` as it stands --, lengths [n], flags [n]: whether any output sample of the clip is non-zero).  One download:
    the [n, 2] lengths and flags; the samples stay on the device."""
    ni = _per_request("ref_prestep", "n_in", np.asarray(n_in).reshape(-1), np.int32, per="clip")
    ch = _per_request("ref_prestep", "channels", np.asarray(channels).reshape(-1), np.int32, len(ni), per="clip")
    cs = np.ascontiguousarray(np.broadcast_to(np.asarray(clip_short, dtype=bool), ni.shape).astype(np.uint8))
    if int(rate) < 11025:
        raise _lib.F5HipError(f"ref_prestep: reference audio below 11025 Hz is not supported on this path (got {rate})")
    if (ni < 0).any() or (ch < 1).any():
        raise _lib.F5HipError("ref_prestep: a clip needs a frame count of 0 or more and at least one channel")
    total = int((ni.astype(np.int64) * ch).sum())
    if total > 2 ** 31 - 1:
        raise _lib.F5HipError("ref_prestep: the clips of the call exceed 2^31 - 1 samples")
    if not torch.is_tensor(frames):
        host = np.ascontiguousarray(np.asarray(frames)).reshape(-1)
        if host.dtype != np.int16:
            raise _lib.F5HipError(f"ref_prestep: int16 frames expected (got {host.dtype})")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        frames = torch.from_numpy(host).to(dev)                   # the one upload
    if frames.dtype != torch.int16 or not frames.is_cuda or not frames.is_contiguous() or frames.dim() != 1:
        raise _lib.F5HipError("ref_prestep: frames must be a contiguous 1-D int16 tensor on the device")
    if frames.numel() != total:
        raise _lib.F5HipError(f"ref_prestep: the frames need sum(n_in * channels) = {total} samples (got {frames.numel()})")
    if torch_ops.load():
        out, info = call_op("ref_prestep", frames, torch.from_numpy(ni), torch.from_numpy(ch), torch.from_numpy(cs), int(rate))
    else:
        bound = int(_lib.lib().f5hip_ref_prestep_bound(len(ni), _p(ni), _p(ch), int(rate)))
        if bound < 0 or bound > 2 ** 31 - 1:
            raise _lib.F5HipError("ref_prestep: the clips of the call exceed 2^31 - 1 samples")
        with torch.cuda.device(frames.device):
            out = torch.empty(bound, device=frames.device, dtype=torch.float32)
            info = torch.empty(len(ni), 2, device=frames.device, dtype=torch.int32)
            _lib.check(_lib.lib().f5hip_ref_prestep(len(ni), _p(ni), _p(ch), _p(cs), _p(frames) if total else None, total, int(rate), _p(out), _p(info),
                                                    _lib.current_stream_ptr()), "f5hip_ref_prestep")
    got = info.cpu().numpy()                                      # the one download: lengths and flags
    if (got[:, 0] < 0).any():
        raise _lib.F5HipError("ref_prestep: a clip kept more ranges than the device holds")
    lengths = [int(v) for v in got[:, 0]]
    return out[:int((got[:, 0].astype(np.int64) * ch).sum())], lengths, [bool(v) for v in got[:, 1]]


def ref_prestep_planes(packed, lengths, channels):
    """Clip i's [channels[i], lengths[i]] view of `ref_prestep`'s packed output."""
    out, at = [], 0
    for n, c in zip(lengths, channels):
        out.append(packed[at:at + int(n) * int(c)].view(int(c), int(n)))
        at += int(n) * int(c)
    return out


def ref_denoise(wave, offsets, lengths):
    """The per-voice denoiser of uploaded reference clips for several clips in ONE library call and four launches (include/f5hip.h
    f5hip_ref_denoise): `audio_prep.denoise_reference` of each clip in fp32, IN PLACE.  wave: the contiguous 1-D fp32 device tensor that holds
    the clips -- `ref_frontend`'s packed output as it stands --; clip i is wave[offsets[i] : offsets[i] + lengths[i]], mono at 24 kHz, 1 to
    `audio_prep.DENOISE_MAX_SAMPLES` samples.  The ranges are disjoint and need not be adjacent: samples between them, and clips left out of
    the table, keep their bits.  A clip's result equals its own single-clip call's bit for bit.  Returns `wave`."""
    from .audio_prep import DENOISE_MAX_SAMPLES
    ln = _per_request("ref_denoise", "lengths", lengths, np.int32, per="clip")
    off = _per_request("ref_denoise", "offsets", offsets, np.int64, len(ln), per="clip")
    if not (torch.is_tensor(wave) and wave.dtype == torch.float32 and wave.is_contiguous() and wave.is_cuda and wave.dim() == 1):
        raise _lib.F5HipError("ref_denoise: wave must be a contiguous 1-D fp32 tensor on the HIP device")
    if torch_ops.load():
        call_op("ref_denoise", wave, torch.from_numpy(off), torch.from_numpy(ln))
        return wave
    for i in range(len(ln)):
        if ln[i] < 1 or ln[i] > DENOISE_MAX_SAMPLES:
            raise _lib.F5HipError(f"ref_denoise: clip {i} has {ln[i]} samples (1 .. {DENOISE_MAX_SAMPLES})")
        if off[i] < 0 or int(off[i]) + int(ln[i]) > wave.numel():
            raise _lib.F5HipError(f"ref_denoise: clip {i} is samples [{off[i]}, {int(off[i]) + int(ln[i])}) of a tensor of {wave.numel()}")
    with torch.cuda.device(wave.device):
        _lib.check(_lib.lib().f5hip_ref_denoise(len(ln), _p(off), _p(ln), _p(wave), _lib.current_stream_ptr()), "f5hip_ref_denoise")
    return wave


def ref_assess(raw, raw_offsets, channels, raw_lengths, wave, offsets, lengths):
    """The reference-clip report of several clips in ONE library call and six launches (include/f5hip.h f5hip_ref_assess):
    `audio_prep.assess_reference` of each clip on the two buffers of a front-end call.  raw: the contiguous 1-D fp32 device tensor that holds
    the raw clips as `ref_frontend` is handed them -- clip i is channels[i] channels of raw_lengths[i] samples, channel after channel, at
    raw[raw_offsets[i]] --; wave, offsets, lengths as `ref_denoise` takes them (`ref_frontend`'s packed output; pass
    min(length, `audio_prep.ASSESS_MAX_SAMPLES`)).  Both are read only.  Returns the rows, int64 [n, len(`audio_prep.ASSESS_ROW`)] on the
    device (`audio_prep.report_from_row` reads one): counts and peak exactly the host's, and a clip's row equals its own single-clip call's
    bit for bit."""
    from .audio_prep import ASSESS_MAX_CHANNELS, ASSESS_MAX_SAMPLES, ASSESS_ROW
    ln = _per_request("ref_assess", "lengths", lengths, np.int32, per="clip")
    off = _per_request("ref_assess", "offsets", offsets, np.int64, len(ln), per="clip")
    ro = _per_request("ref_assess", "raw_offsets", raw_offsets, np.int64, len(ln), per="clip")
    ch = _per_request("ref_assess", "channels", channels, np.int32, len(ln), per="clip")
    rl = _per_request("ref_assess", "raw_lengths", raw_lengths, np.int32, len(ln), per="clip")
    for t, name in ((raw, "raw"), (wave, "wave")):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda and t.dim() == 1):
            raise _lib.F5HipError(f"ref_assess: {name} must be a contiguous 1-D fp32 tensor on the HIP device")
    if raw.device != wave.device:
        raise _lib.F5HipError("ref_assess: raw and wave must be on one HIP device")
    if torch_ops.load():
        return call_op("ref_assess", raw, torch.from_numpy(ro), torch.from_numpy(ch), torch.from_numpy(rl), wave, torch.from_numpy(off), torch.from_numpy(ln))
    for i in range(len(ln)):
        if ch[i] < 1 or ch[i] > ASSESS_MAX_CHANNELS:
            raise _lib.F5HipError(f"ref_assess: clip {i} has {ch[i]} channels (1 .. {ASSESS_MAX_CHANNELS})")
        if rl[i] < 1 or ro[i] < 0 or int(ro[i]) + int(rl[i]) * int(ch[i]) > raw.numel():
            raise _lib.F5HipError(f"ref_assess: raw clip {i} is {ch[i]} x {rl[i]} samples at {ro[i]} of a tensor of {raw.numel()}")
        if ln[i] < 1 or ln[i] > ASSESS_MAX_SAMPLES:
            raise _lib.F5HipError(f"ref_assess: clip {i} has {ln[i]} samples (1 .. {ASSESS_MAX_SAMPLES})")
        if off[i] < 0 or int(off[i]) + int(ln[i]) > wave.numel():
            raise _lib.F5HipError(f"ref_assess: clip {i} is samples [{off[i]}, {int(off[i]) + int(ln[i])}) of a tensor of {wave.numel()}")
    with torch.cuda.device(wave.device):
        rows = torch.empty(len(ln), len(ASSESS_ROW), device=wave.device, dtype=torch.int64)
        _lib.check(_lib.lib().f5hip_ref_assess(len(ln), _p(raw), _p(ro), _p(ch), _p(rl), _p(wave), _p(off), _p(ln), _p(rows), _lib.current_stream_ptr()),
                   "f5hip_ref_assess")
    return rows


def wave_finish(chunks, chunks_per_request, fade, remove_silence=None, sample_rate=24000):
    """The waveform back-end for several requests in ONE library call (include/f5hip.h f5hip_wave_finish): `chunks` = the chunk waves of all
    requests in request and chunk order, each a 1-D contiguous fp32 device tensor with the rms gain applied (views of a vocoder's packed
    output are read in place); `chunks_per_request` [n]; `fade` in samples; `remove_silence` one bool per request (None: none).  Joins each
    request's chunks with the reference's linear cross-fade, quantises to int16 by `serve.pcm16`'s rule and, for a flagged request, applies
    `audio_prep.remove_silence_pcm`'s rule.  Returns (pcm int16 device, lengths [n] int32 device, offsets): request i's samples are
    pcm[offsets[i] : offsets[i] + lengths[i]].  Refused (F5HipError): a chunk shorter than 2 * fade in a request of several chunks, a negative
    fade, a rate other than 24 000, more than 2^31 - 1 samples."""
    return _wave_finish(chunks, chunks_per_request, fade, None, remove_silence, sample_rate)


def wave_finish_joins(chunks, chunks_per_request, fade, chunk_fade, remove_silence=None, sample_rate=24000):
    """`wave_finish` with a choice per join (include/f5hip.h f5hip_wave_finish_joins): `chunk_fade` one bool per chunk of the call -- True: the
    chunk cross-fades into the one before it in its request over `fade` samples, False: it butts against it (a request's first chunk is
    ignored) -- so a multi-voice script's request is joined as `infer.join_segments` joins it, a gap being a chunk of zeros.  None is
    `wave_finish`.  Refused instead of the 2 * fade rule: a chunk shorter than the fades it takes part in (`fade` if it fades in, plus `fade`
    if its successor does)."""
    chunks = list(chunks)
    if chunk_fade is not None:
        chunk_fade = _per_request("wave_finish_joins", "chunk_fade", np.asarray(chunk_fade, dtype=bool), np.uint8, len(chunks), per="chunk")
    return _wave_finish(chunks, chunks_per_request, fade, chunk_fade, remove_silence, sample_rate)


def _wave_finish(chunks, chunks_per_request, fade, chunk_fade, remove_silence, sample_rate):
    k = _per_request("wave_finish", "chunks_per_request", chunks_per_request, np.int32)
    flags = np.zeros(len(k), dtype=np.uint8) if remove_silence is None else _per_request("wave_finish", "remove_silence",
                                                                                         np.asarray(remove_silence, dtype=bool), np.uint8, len(k))
    chunks = list(chunks)
    if (k < 1).any() or int(k.sum()) != len(chunks):
        raise _lib.F5HipError("wave_finish: a chunk count of 1 or more per request, sum(chunks_per_request) chunk waves")
    ptrs, lens = pointer_table("wave_finish", chunks, "chunk")
    samples = lens.tolist()
    if min(samples) < 1:
        raise _lib.F5HipError("wave_finish: every chunk must be a non-empty tensor")
    fade = int(fade)
    joined, c = [], 0
    for kk in k.tolist():
        fading = kk - 1 if chunk_fade is None else int(np.count_nonzero(chunk_fade[c + 1:c + kk]))
        joined.append(sum(samples[c:c + kk]) - fading * max(fade, 0))
        c += kk
    offsets, off = _pack(joined, 8)
    if torch_ops.load():
        if chunk_fade is None:
            pcm, lengths = call_op("wave_finish", chunks, torch.from_numpy(k), fade, torch.from_numpy(flags), int(sample_rate))
        else:
            pcm, lengths = call_op("wave_finish_joins", chunks, torch.from_numpy(k), fade, torch.from_numpy(chunk_fade), torch.from_numpy(flags),
                                   int(sample_rate))
    else:
        dev = chunks[0].device
        with torch.cuda.device(dev):
            pcm = torch.empty(max(off, 0), device=dev, dtype=torch.int16)
            lengths = torch.empty(len(k), device=dev, dtype=torch.int32)
            _lib.check(_lib.lib().f5hip_wave_finish_joins(len(k), _p(k), _p(ptrs), _p(lens), fade, _p(chunk_fade), _p(flags), int(sample_rate), _p(pcm),
                                                          _p(lengths), _lib.current_stream_ptr()), "f5hip_wave_finish")
    return pcm, lengths, offsets


WAVE_ENCODINGS = ("pcm16", "mulaw", "alaw")   # the library's encoding codes 0, 1, 2 (infer.OUTPUT_ENCODINGS)


def wave_encode_tile(sample_rate):
    """24 kHz input samples one block of `wave_encode` owns at `sample_rate` (0: a rate the library refuses)."""
    return int(_lib.lib().f5hip_wave_encode_tile(int(sample_rate)))


def wave_encode(pcm, in_off, max_len, len_dev, sample_rate, encoding, taps=None):
    """The delivery format of several finished requests in ONE library call and one launch (include/f5hip.h f5hip_wave_encode): their 24 kHz
    int16 PCM on the device -> `sample_rate`, then "pcm16", "mulaw" or "alaw" (or the code 0, 1, 2).  `pcm`: one int16 device tensor that holds
    every request (`wave_finish`'s packed PCM; request i starts at sample in_off[i]) or one tensor per request (in_off[i] within its own);
    `max_len` [n]: an upper bound of each length, which sizes the output; `len_dev`: int32 device [n], the actual lengths (`wave_finish`'s
    `lengths`, never needed on the host), or None: `max_len`; `taps`: fp32 device table of `infer.resample_taps(24000, sample_rate)`, not
    needed at 24 000.  Returns (data uint8 device, out_len int32 device [n], offsets): request i's result is
    data[offsets[i] : offsets[i] + out_len[i] * bytes_per_sample] -- little-endian int16 samples, or one code byte per sample --, bit for bit
    `infer.deliver_pcm16` of its PCM."""
    tensors, io, ml, n, len_dev = _pcm_requests("wave_encode", pcm, in_off, max_len, len_dev, several=True)
    code = WAVE_ENCODINGS.index(encoding) if encoding in WAVE_ENCODINGS else encoding
    if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or not 0 <= int(code) <= 2:
        raise _lib.F5HipError(f"wave_encode: unknown encoding {encoding!r} (one of {list(WAVE_ENCODINGS)} or its code)")
    code, rate = int(code), int(sample_rate)
    if rate < 1:
        raise _lib.F5HipError(f"wave_encode: the sample rate must be positive (got {sample_rate})")
    of, nf, _, L = rate_pair(24000, rate)
    if rate != 24000:
        if taps is None or not (taps.dtype == torch.float32 and taps.is_contiguous() and taps.is_cuda) or tuple(taps.shape) != (nf, L):
            raise _lib.F5HipError(f"wave_encode: taps must be a contiguous fp32 device tensor [{nf}, {L}] for 24000 -> {rate} Hz "
                                  f"(got {None if taps is None else tuple(taps.shape)})")
    if torch_ops.load():
        data, out_len, out_off = call_op("wave_encode", tensors, torch.from_numpy(io), torch.from_numpy(ml), len_dev, rate, code, taps)
        return data, out_len, out_off.tolist()
    anchor, rel = _pcm_sources("wave_encode", tensors, io, ml)
    out_off, nbytes = _pack([((nf * int(m) + of - 1) // of) * (2 if code == 0 else 1) for m in ml], 16)
    oo = np.asarray(out_off, dtype=np.int64)
    dev = tensors[0].device
    with torch.cuda.device(dev):
        data = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)[:nbytes]   # (a call of empty requests still has an address to give)
        out_len = torch.empty(n, device=dev, dtype=torch.int32)
        _lib.check(_lib.lib().f5hip_wave_encode(n, _p(anchor), _p(rel), _p(ml), _p(len_dev), rate, code, _p(taps) if rate != 24000 else None, _p(data),
                                                _p(oo), _p(out_len), _lib.current_stream_ptr()), "f5hip_wave_encode")
    return data, out_len, out_off


def wave_flac(pcm, in_off, max_len, len_dev, sample_rate, level=None):
    """The FLAC streams of several finished requests in ONE library call and at most three launches (include/f5hip.h f5hip_wave_flac): their
    int16 PCM at `sample_rate`, on the device -> each request's complete native FLAC stream.  `pcm`, `in_off`, `max_len`, `len_dev` as in
    `wave_encode`: `wave_finish`'s packed PCM and device lengths at 24 kHz, or `wave_encode(..., "pcm16")`'s data viewed as int16 (offsets in
    samples) and its `out_len` at another rate.  Returns (data uint8 device, out_len int32 device [n], offsets): request i's stream is
    data[offsets[i] : offsets[i] + out_len[i]], byte for byte `infer.encode_flac` of its samples.  `level`: None (level 0, the entry point
    f5hip_wave_flac), or the FLAC level (`wave_codec.check_flac_level`) of every request as one int or one int per request
    (f5hip_wave_flac_levels: LPC subframes for the requests at level 1, the same three launches)."""
    tensors, io, ml, n, len_dev = _pcm_requests("wave_flac", pcm, in_off, max_len, len_dev, several=True)
    rate, lv = int(sample_rate), None
    if level is not None:
        given = [level] * n if isinstance(level, (int, np.integer)) else list(level)
        if len(given) != n or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) not in (0, 1) for v in given):
            raise _lib.F5HipError(f"wave_flac: level is 0 or 1, one int or one per request (got {level!r} for {n} requests)")
        lv = _per_request("wave_flac", "level", given, np.int32, n)
    if torch_ops.load():
        if lv is None:
            data, out_len, out_off = call_op("wave_flac", tensors, torch.from_numpy(io), torch.from_numpy(ml), len_dev, rate)
        else:
            data, out_len, out_off = call_op("wave_flac_levels", tensors, torch.from_numpy(io), torch.from_numpy(ml), len_dev, rate, torch.from_numpy(lv))
        return data, out_len, out_off.tolist()
    anchor, rel = _pcm_sources("wave_flac", tensors, io, ml)
    out_off, nbytes = _pack([_lib.lib().f5hip_wave_flac_bound(int(m)) for m in ml], 16)
    oo = np.asarray(out_off, dtype=np.int64)
    dev = tensors[0].device
    with torch.cuda.device(dev):
        data = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        out_len = torch.empty(n, device=dev, dtype=torch.int32)
        if lv is None:
            _lib.check(_lib.lib().f5hip_wave_flac(n, _p(anchor), _p(rel), _p(ml), _p(len_dev), rate, _p(data), _p(oo), _p(out_len),
                                                  _lib.current_stream_ptr()), "f5hip_wave_flac")
        else:
            _lib.check(_lib.lib().f5hip_wave_flac_levels(n, _p(anchor), _p(rel), _p(ml), _p(len_dev), rate, _p(lv), _p(data), _p(oo),
                                                         _p(out_len), _lib.current_stream_ptr()), "f5hip_wave_flac_levels")
    return data, out_len, out_off


_prosody_taps: dict = {}   # device -> the twelve pitch tables there, uploaded once


def wave_prosody_taps(device):
    """The tap tables of the twelve pitch steps as ONE fp32 tensor on `device` (include/f5hip.h f5hip_wave_prosody: table s =
    `wave_codec.resample_taps(p, q)` of `wave_codec.PITCH_RATIOS[s]` at float f5hip_wave_prosody_tap_offset(s)); uploaded once per device."""
    from . import wave_codec
    key = str(torch.device(device))
    hit = _prosody_taps.get(key)
    if hit is None:
        lib = _lib.lib()
        host = torch.zeros(int(lib.f5hip_wave_prosody_tap_offset(0)), dtype=torch.float32)
        for s, (p, q) in wave_codec.PITCH_RATIOS.items():
            taps = wave_codec.resample_taps(p, q)[3].reshape(-1)
            at = int(lib.f5hip_wave_prosody_tap_offset(s))
            host[at:at + taps.numel()] = taps
        hit = _prosody_taps[key] = host.to(device)
    return hit


def wave_prosody_formants_launches():
    """Launches `wave_prosody` adds for a call in which a request keeps its formants (3)."""
    return int(_lib.lib().f5hip_wave_prosody_formants_launches())


def wave_prosody(pcm, in_off, max_len, len_dev, stretches, pitches, keep_formants=None):
    """The tempo and pitch of several finished requests in ONE library call and two launches, one when no request has a pitch
    (include/f5hip.h f5hip_wave_prosody): their 24 kHz int16 PCM on the device -> each request's `wave_codec.shift_pcm16`, bit for bit.
    `pcm`: the int16 device tensor that holds every request (`wave_finish`'s packed PCM; request i starts at sample in_off[i]); `max_len`,
    `len_dev` as in `wave_encode`; `stretches` [n]: (P, Q) of each request (`WaveSpec.stretch`; (1, 1) leaves the duration alone);
    `pitches` [n]: semitones, 0 for none.  A neutral request is copied through.  Returns (pcm2 int16 device, lengths2 int32 device [n],
    offsets2, bounds2): request i's samples are pcm2[offsets2[i] : offsets2[i] + lengths2[i]], and bounds2[i] is the length that max_len[i]
    gives -- what `wave_loudness`, `wave_encode` and `wave_flac` take in the place of `wave_finish`'s buffer, offsets, bounds and lengths.
    `keep_formants` [n] of bools (None: the call above, unchanged): a flagged request needs a pitch, takes the stretch of its tempo alone
    (`wave_codec.formant_stretch`) and keeps its spectral envelope -- `wave_codec.shift_pcm16(..., keep_formants=True)` bit for bit, three
    more launches whatever n (include/f5hip.h f5hip_wave_prosody_formants), the resampler's only when another request has a plain pitch."""
    (pcm,), io, ml, n, len_dev = _pcm_requests("wave_prosody", pcm, in_off, max_len, len_dev)
    kf = None
    if keep_formants is not None:
        if any(not isinstance(v, (bool, np.bool_)) for v in keep_formants):
            raise _lib.F5HipError(f"wave_prosody: keep_formants is one bool per request (got {list(keep_formants)!r})")
        kf = np.ascontiguousarray(_per_request("wave_prosody", "keep_formants", [bool(v) for v in keep_formants], np.int64, n).astype(np.uint8))
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in pitches):
        raise _lib.F5HipError(f"wave_prosody: a pitch is a whole number of semitones (got {list(pitches)!r})")
    pt = _per_request("wave_prosody", "pitches", pitches, np.int64, n)
    st = _per_request("wave_prosody", "stretches", [tuple(s) for s in stretches], np.int64, n)
    if st.shape != (n, 2) or (np.abs(st) > 1 << 20).any() or (st < 1).any() or (st[:, 0] > 2 * st[:, 1]).any() or (st[:, 1] > 2 * st[:, 0]).any():
        raise _lib.F5HipError(f"wave_prosody: a stretch is a pair of positive terms up to 2^20 with a ratio from 1/2 to 2 (got {st.tolist()})")
    if (np.abs(pt) > 6).any():
        raise _lib.F5HipError(f"wave_prosody: a pitch is -6 to 6 semitones (got {pt.tolist()})")
    sp, sq, pt = (np.ascontiguousarray(a.astype(np.int32)) for a in (st[:, 0], st[:, 1], pt))
    if kf is not None and (kf.astype(bool) & (pt == 0)).any():
        raise _lib.F5HipError(f"wave_prosody: a request keeps its formants without a pitch (pitches {pt.tolist()}, keep_formants {kf.tolist()})")
    plain = pt if kf is None else np.where(kf.astype(bool), 0, pt)     # the steps that go through the resampler
    taps = wave_prosody_taps(pcm.device) if plain.any() else None
    if torch_ops.load() and kf is not None:
        pcm2, lengths2, offsets2, bounds2 = call_op("wave_prosody_formants", pcm, torch.from_numpy(io), torch.from_numpy(ml), len_dev, torch.from_numpy(sp),
                                                    torch.from_numpy(sq), torch.from_numpy(pt), torch.from_numpy(kf), taps)
        return pcm2, lengths2, offsets2.tolist(), bounds2.tolist()
    if torch_ops.load():
        pcm2, lengths2, offsets2, bounds2 = call_op("wave_prosody", pcm, torch.from_numpy(io), torch.from_numpy(ml), len_dev, torch.from_numpy(sp),
                                                    torch.from_numpy(sq), torch.from_numpy(pt), taps)
        return pcm2, lengths2, offsets2.tolist(), bounds2.tolist()
    from . import wave_codec
    anchor, rel = _pcm_sources("wave_prosody", [pcm], io, ml)
    bounds2 = [wave_codec.shifted_length(int(m), (int(p), int(q)), int(s)) for m, p, q, s in zip(ml, sp, sq, plain)]
    offsets2, total = _pack(bounds2, 8)
    oo = np.asarray(offsets2, dtype=np.int64)
    with torch.cuda.device(pcm.device):
        pcm2 = torch.empty(max(total, 8), device=pcm.device, dtype=torch.int16)[:total]   # (a call of empty requests still has an address to give)
        lengths2 = torch.empty(n, device=pcm.device, dtype=torch.int32)
        if kf is not None:
            _lib.check(_lib.lib().f5hip_wave_prosody_formants(n, _p(anchor), _p(rel), _p(ml), _p(len_dev), _p(sp), _p(sq), _p(pt), _p(kf), _p(taps), _p(pcm2),
                                                              _p(oo), _p(lengths2), _lib.current_stream_ptr()), "f5hip_wave_prosody_formants")
        else:
            _lib.check(_lib.lib().f5hip_wave_prosody(n, _p(anchor), _p(rel), _p(ml), _p(len_dev), _p(sp), _p(sq), _p(pt), _p(taps), _p(pcm2), _p(oo), _p(lengths2),
                                                     _lib.current_stream_ptr()), "f5hip_wave_prosody")
    return pcm2, lengths2, offsets2, bounds2


def wave_loudness_tile():
    """Samples one block of `wave_loudness`'s first launch owns (two 100 ms sub-blocks)."""
    return int(_lib.lib().f5hip_wave_loudness_tile())


def wave_loudness(pcm, in_off, max_len, len_dev, gain_k):
    """The loudness target of several finished requests in ONE library call and three launches (include/f5hip.h f5hip_wave_loudness): their
    24 kHz int16 PCM on the device, normalised IN PLACE.  `pcm`: the int16 device tensor that holds every request (`wave_finish`'s packed
    PCM; request i starts at sample in_off[i]); `max_len`, `len_dev` as in `wave_encode`; `gain_k` [n]: `wave_codec.loudness_gain_constant`
    of each request's target, 0 (or None) for a request that is left alone.  A call without a flagged request launches nothing.  Returns
    stats, int64 device [n, 4]: n2, S2, peak and the bits of the gain g of each flagged request (zeros for the others) --
    `wave_codec.measure_loudness` and `loudness_gain` of its samples, and afterwards its samples are `normalise_loudness_pcm16`'s, bit for
    bit."""
    (pcm,), io, ml, n, len_dev = _pcm_requests("wave_loudness", pcm, in_off, max_len, len_dev)
    gk = _per_request("wave_loudness", "gain_k", [0.0 if k is None else k for k in gain_k], np.float64, n)
    if not np.isfinite(gk).all():
        raise _lib.F5HipError("wave_loudness: a gain constant is not finite")
    if torch_ops.load():
        return call_op("wave_loudness", pcm, torch.from_numpy(io), torch.from_numpy(ml), len_dev, torch.from_numpy(gk))
    anchor, rel = _pcm_sources("wave_loudness", [pcm], io, ml)
    with torch.cuda.device(pcm.device):
        stats = torch.zeros(n, 4, device=pcm.device, dtype=torch.int64)
        if (gk > 0).any() and pcm.numel():
            _lib.check(_lib.lib().f5hip_wave_loudness(n, _p(anchor), _p(rel), _p(ml), _p(len_dev), _p(gk), _p(stats), _lib.current_stream_ptr()),
                       "f5hip_wave_loudness")
    return stats


def wave_mark_tile():
    """Samples one block of `wave_mark`'s second launch owns (32 blocks of 240)."""
    return int(_lib.lib().f5hip_wave_mark_tile())


def watermark_carriers(keys, device):
    """The carriers of `keys` as ONE int16 tensor [len(keys), 16384] on `device`, what `wave_mark` and `watermark_detect` hand to the
    library.  Each distinct key's carrier (`wave_codec.watermark_carrier`) is uploaded once per device and kept (the last
    `wave_codec.TAP_TABLE_CACHE`, like `_device_taps`); several keys are stacked on the device."""
    from . import wave_codec
    rows = [wave_codec._device_carrier(k, device) for k in keys]
    return rows[0].reshape(1, -1) if len(rows) == 1 else torch.stack(rows)


def watermark_tag_carriers(keys, device):
    """The carriers of `keys` for calls with trace ids as ONE int16 tensor [len(keys), 4, 16384] on `device`, what `wave_mark` (for tags)
    and `watermark_read_ids` hand to the library: per key its own carrier, then those of its sub-keys 0 .. 2
    (`wave_codec.watermark_subkey`).  Each distinct key's four rows are uploaded once per device and kept (the last
    `wave_codec.TAP_TABLE_CACHE`); several keys are stacked on the device."""
    from . import wave_codec
    rows = [wave_codec._device_tag_carriers(k, device) for k in keys]
    return rows[0][None] if len(rows) == 1 else torch.stack(rows)


def _check_carriers(op, carriers, device, tagged=False):
    from . import wave_codec
    most = wave_codec.WATERMARK_ID_KEYS_MAX if op == "watermark_read_ids" or (op == "watermark_scan" and tagged) else wave_codec.WATERMARK_KEYS_MAX
    shape = (4, wave_codec.WATERMARK_PERIOD) if tagged else (wave_codec.WATERMARK_PERIOD,)
    if not (torch.is_tensor(carriers) and carriers.dtype == torch.int16 and carriers.is_cuda and carriers.is_contiguous() and tuple(carriers.shape[1:]) == shape
            and 1 <= carriers.shape[0] <= most and carriers.device == device):
        raise _lib.F5HipError(f"{op}: carriers must be a contiguous int16 tensor [1 .. {most}, {', '.join(map(str, shape))}] on the samples' device")


def wave_mark(pcm, in_off, max_len, len_dev, keys):
    """The provenance watermark of several finished requests in ONE library call and two launches (include/f5hip.h f5hip_wave_mark): their
    24 kHz int16 PCM on the device, marked IN PLACE.  `pcm`: the int16 device tensor that holds every request (`wave_finish`'s or
    `wave_prosody`'s buffer; request i starts at sample in_off[i]); `max_len`, `len_dev` as in `wave_encode`; `keys` [n]: each request's key
    (`wave_codec.check_watermark`), None for a request that is left alone.  A call without a flagged request launches nothing.  Afterwards a
    flagged request's samples are `wave_codec.mark_pcm16`'s, bit for bit; the others and the samples between requests keep their bits.
    A value of `keys` may be a `wave_codec.WatermarkTag(key, id)` (or its dict): that request's mark carries the trace id too, and the call
    is f5hip_wave_mark_ids', still two launches; with no tag among them nothing changes.  Returns `pcm`."""
    from . import wave_codec
    (pcm,), io, ml, n, len_dev = _pcm_requests("wave_mark", pcm, in_off, max_len, len_dev)
    keys = list(keys)
    if len(keys) != n:
        raise _lib.F5HipError(f"wave_mark: keys needs one value per request ({n}), got {len(keys)}")
    try:
        keys = [wave_codec.check_watermark(k) for k in keys]
    except ValueError as e:
        raise _lib.F5HipError(f"wave_mark: {e}") from e
    tagged = any(isinstance(k, wave_codec.WatermarkTag) for k in keys)
    ids = np.ascontiguousarray(np.asarray([k.id if isinstance(k, wave_codec.WatermarkTag) else -1 for k in keys], dtype=np.int32))
    keys = [wave_codec.watermark_key(k) for k in keys]
    distinct = sorted({k for k in keys if k is not None})
    if len(distinct) > wave_codec.WATERMARK_KEYS_MAX:
        raise _lib.F5HipError(f"wave_mark: at most {wave_codec.WATERMARK_KEYS_MAX} distinct keys in a call (got {len(distinct)})")
    ki = np.ascontiguousarray(np.asarray([-1 if k is None else distinct.index(k) for k in keys], dtype=np.int32))
    carriers = None if not distinct else watermark_tag_carriers(distinct, pcm.device) if tagged else watermark_carriers(distinct, pcm.device)
    if torch_ops.load():
        if tagged:
            call_op("wave_mark_ids", pcm, torch.from_numpy(io), torch.from_numpy(ml), len_dev, torch.from_numpy(ki), torch.from_numpy(ids), carriers)
        else:
            call_op("wave_mark", pcm, torch.from_numpy(io), torch.from_numpy(ml), len_dev, torch.from_numpy(ki), carriers)
        return pcm
    anchor, rel = _pcm_sources("wave_mark", [pcm], io, ml)
    if int(ml.astype(np.int64).sum()) > 2 ** 31 - 1:
        raise _lib.F5HipError("wave_mark: the call exceeds 2^31 - 1 samples")
    if distinct and pcm.numel():
        with torch.cuda.device(pcm.device):
            if tagged:
                _lib.check(_lib.lib().f5hip_wave_mark_ids(n, _p(anchor), _p(rel), _p(ml), _p(len_dev), _p(ki), _p(ids), _p(carriers), len(distinct),
                                                          _lib.current_stream_ptr()), "f5hip_wave_mark_ids")
            else:
                _lib.check(_lib.lib().f5hip_wave_mark(n, _p(anchor), _p(rel), _p(ml), _p(len_dev), _p(ki), _p(carriers), len(distinct), _lib.current_stream_ptr()),
                           "f5hip_wave_mark")
    return pcm


def _watermark_rows(op, wave, offsets, lengths, carriers, ids):
    """`watermark_detect` (ids False) and `watermark_read_ids` under their names: the clip checks, then either binding."""
    from . import wave_codec
    ln = _per_request(op, "lengths", lengths, np.int32, per="clip")
    off = _per_request(op, "offsets", offsets, np.int64, len(ln), per="clip")
    if not (torch.is_tensor(wave) and wave.dtype == torch.float32 and wave.is_contiguous() and wave.is_cuda and wave.dim() == 1):
        raise _lib.F5HipError(f"{op}: wave must be a contiguous 1-D fp32 tensor on the HIP device")
    _check_carriers(op, carriers, wave.device, ids)
    if torch_ops.load():
        return call_op(op, wave, torch.from_numpy(off), torch.from_numpy(ln), carriers)
    for i in range(len(ln)):
        if ln[i] < 1 or ln[i] > wave_codec.WATERMARK_MAX_SAMPLES:
            raise _lib.F5HipError(f"{op}: clip {i} has {ln[i]} samples (1 .. {wave_codec.WATERMARK_MAX_SAMPLES})")
        if off[i] < 0 or int(off[i]) + int(ln[i]) > wave.numel():
            raise _lib.F5HipError(f"{op}: clip {i} is samples [{off[i]}, {int(off[i]) + int(ln[i])}) of a tensor of {wave.numel()}")
    call = _lib.lib().f5hip_watermark_read_ids if ids else _lib.lib().f5hip_watermark_detect
    with torch.cuda.device(wave.device):
        rows = torch.empty(len(ln), carriers.shape[0], 10 if ids else 4, device=wave.device, dtype=torch.float32)
        _lib.check(call(len(ln), _p(wave), _p(off), _p(ln), carriers.shape[0], _p(carriers), _p(rows), _lib.current_stream_ptr()), f"f5hip_{op}")
    return rows


def watermark_detect(wave, offsets, lengths, carriers):
    """Several clips scored against several keys in ONE library call and four launches (include/f5hip.h f5hip_watermark_detect):
    `wave_codec.detect_watermark` of each clip in fp32.  wave: the contiguous 1-D fp32 device tensor that holds the clips (mono, 24 kHz) --
    `ref_frontend`'s packed output as it stands --, read only; clip i is wave[offsets[i] : offsets[i] + lengths[i]], 1 to
    `wave_codec.WATERMARK_MAX_SAMPLES` samples, disjoint ranges; `carriers`: `watermark_carriers(keys, device)`.  Returns scores, fp32 device
    [n, n_keys, 4]: z, the offset, r at the offset and the deviation of r; a clip below `wave_codec.WATERMARK_MIN_SAMPLES` scores zeros.  A
    clip's rows equal its own single-clip call's bit for bit."""
    return _watermark_rows("watermark_detect", wave, offsets, lengths, carriers, False)


def watermark_scores(rows, keys) -> list:
    """`wave_codec.WatermarkScore`s of one clip's downloaded score rows [n_keys, 4]."""
    from . import wave_codec
    return [wave_codec.WatermarkScore(k, float(z), int(o), bool(z >= wave_codec.WATERMARK_THRESHOLD)) for k, (z, o, _, _) in zip(keys, rows.tolist())]


def watermark_read_ids_launches():
    """Launches of one `watermark_read_ids` call (4)."""
    return int(_lib.lib().f5hip_watermark_read_ids_launches())


def watermark_read_ids(wave, offsets, lengths, carriers):
    """Several clips scored against 1 to 4 keys and read for the trace ids their marks carry in ONE library call and four launches
    (include/f5hip.h f5hip_watermark_read_ids): `wave_codec.read_watermark` of each clip in fp32.  `wave`, `offsets`, `lengths` as
    `watermark_detect`'s; `carriers`: `watermark_tag_carriers(keys, device)`.  Returns rows, fp32 device [n, n_keys, 10]: `watermark_detect`'s
    four words of that clip and key, bit for bit, then (s_d, z_d) of the three symbols; `watermark_reads` turns a clip's rows into
    `WatermarkRead`s.  A clip's rows equal its own single-clip call's bit for bit."""
    return _watermark_rows("watermark_read_ids", wave, offsets, lengths, carriers, True)


def watermark_reads(rows, keys) -> list:
    """`wave_codec.WatermarkRead`s of one clip's downloaded rows [n_keys, 10], by `wave_codec.watermark_read`'s rule: the id only when the
    key is detected and every symbol scores `WATERMARK_ID_THRESHOLD`."""
    from . import wave_codec
    out = []
    for k, row in zip(keys, rows.tolist()):
        score = wave_codec.WatermarkScore(k, float(row[0]), int(row[1]), bool(row[0] >= wave_codec.WATERMARK_THRESHOLD))
        out.append(wave_codec.watermark_read(score, [(int(row[4 + 2 * d]), float(row[5 + 2 * d])) for d in range(wave_codec.WATERMARK_ID_SYMBOLS)]))
    return out


WATERMARK_SCAN_RANGES_MAX = 4096                  # ranges of one `watermark_scan_rows` call (csrc/wave_mark_core.h kWsRangesMax)


def watermark_scan_launches(n_ranges=1, n_keys=1, ids=False):
    """Launches of one `watermark_scan_rows` call: 2 + 2 slabs (include/f5hip.h f5hip_watermark_scan), four for a call of one slab."""
    slabs = int(_lib.lib().f5hip_watermark_scan_slabs(int(n_ranges), int(n_keys), int(bool(ids))))
    if slabs < 1:
        raise _lib.F5HipError(f"watermark_scan_launches: {_lib.lib().f5hip_last_error().decode(errors='replace')}")
    return int(_lib.lib().f5hip_watermark_scan_launches()) + 2 * (slabs - 1)


def watermark_scan_rows(wave, ranges, carriers, ids=False):
    """Segment ranges of ONE recording scored against several keys in one library call (include/f5hip.h f5hip_watermark_scan), the raw
    call under `watermark_scan`.  wave: a contiguous 1-D fp32 device tensor, mono 24 kHz, 1 to `wave_codec.WATERMARK_SCAN_MAX_SAMPLES`
    samples, read only; `ranges`: (first segment, segments) pairs, 1 to 4096 of them, each inside the recording's ceil(n / 16384) segments;
    `carriers`: `watermark_carriers(keys, device)` (1 to 16 keys) -> rows fp32 device [n_ranges, n_keys, 4], `watermark_detect`'s row of the
    range's fold; with `ids`, `watermark_tag_carriers(keys, device)` (1 to 4 keys) -> [n_ranges, n_keys, 10], `watermark_read_ids`' row.  A
    range's rows equal its own single-range call's bit for bit."""
    from . import wave_codec
    op = "watermark_scan"
    rg = np.asarray(ranges, dtype=np.int64)
    if rg.ndim != 2 or rg.shape[1] != 2 or not 1 <= len(rg) <= WATERMARK_SCAN_RANGES_MAX:
        raise _lib.F5HipError(f"{op}: ranges are 1 .. {WATERMARK_SCAN_RANGES_MAX} (first segment, segments) pairs (got shape {rg.shape})")
    if not (torch.is_tensor(wave) and wave.dtype == torch.float32 and wave.is_contiguous() and wave.is_cuda and wave.dim() == 1
            and 1 <= wave.numel() <= wave_codec.WATERMARK_SCAN_MAX_SAMPLES):
        raise _lib.F5HipError(f"{op}: wave must be a contiguous 1-D fp32 tensor of 1 .. {wave_codec.WATERMARK_SCAN_MAX_SAMPLES} samples on the HIP device")
    _check_carriers(op, carriers, wave.device, bool(ids))
    S = -(-wave.numel() // wave_codec.WATERMARK_PERIOD)
    for i, (first, count) in enumerate(rg.tolist()):
        if first < 0 or count < 1 or first + count > S:
            raise _lib.F5HipError(f"{op}: range {i} is {count} segments from segment {first} of a recording of {S}")
    first = np.ascontiguousarray(rg[:, 0], dtype=np.int32)
    count = np.ascontiguousarray(rg[:, 1], dtype=np.int32)
    if torch_ops.load():
        return call_op(op, wave, torch.from_numpy(first), torch.from_numpy(count), carriers)
    with torch.cuda.device(wave.device):
        rows = torch.empty(len(rg), carriers.shape[0], 10 if ids else 4, device=wave.device, dtype=torch.float32)
        _lib.check(_lib.lib().f5hip_watermark_scan(_p(wave), wave.numel(), len(rg), _p(first), _p(count), carriers.shape[0], int(bool(ids)), _p(carriers),
                                                   _p(rows), _lib.current_stream_ptr()), "f5hip_watermark_scan")
    return rows


def watermark_scan(wave, keys) -> list:
    """`wave_codec.scan_watermark` of one recording on the device, fp32: the `wave_codec.WatermarkSpan`s of `keys` (1 to 16) in `wave`, a
    contiguous 1-D fp32 device tensor (mono 24 kHz, finite, at most `wave_codec.WATERMARK_SCAN_MAX_SAMPLES` samples).  ONE
    `watermark_scan_rows` call scores every window against every key; the rows come down and `wave_codec.watermark_spans` runs on the host;
    then at most one more call per four keys reads the spans with their ids, decided by `watermark_reads`.  Below
    `wave_codec.WATERMARK_MIN_SAMPLES` the answer is [] and no device call is made."""
    from . import wave_codec
    keys = wave_codec.check_watermark_keys(keys)
    if not (torch.is_tensor(wave) and wave.dim() == 1):
        raise _lib.F5HipError("watermark_scan: wave must be a contiguous 1-D fp32 tensor on the HIP device")
    n = wave.numel()
    if n > wave_codec.WATERMARK_SCAN_MAX_SAMPLES:
        raise _lib.F5HipError(f"watermark_scan: the recording has {n} samples; at most {wave_codec.WATERMARK_SCAN_MAX_SAMPLES} (600 s at 24 kHz) are scanned")
    if n < wave_codec.WATERMARK_MIN_SAMPLES:
        return []
    W, most = wave_codec.WATERMARK_SCAN_WINDOW, wave_codec.WATERMARK_ID_KEYS_MAX
    S = -(-n // wave_codec.WATERMARK_PERIOD)
    windows = [(w, min(w + W, S) - w) for w in range(wave_codec.watermark_windows(n))]
    rows = watermark_scan_rows(wave, windows, watermark_carriers(keys, wave.device)).cpu().numpy()
    found = wave_codec.watermark_spans([watermark_scores(rows[w], keys) for w in range(len(windows))], n)
    reads = {}
    for at in range(0, len(keys), most):                            # the spans of four keys at a time: one call with ids
        group = keys[at:at + most]
        mine = [i for i, g in enumerate(found) if g.key in group]
        if not mine:
            continue
        got = watermark_scan_rows(wave, [(found[i].first, found[i].count) for i in mine], watermark_tag_carriers(group, wave.device), ids=True).cpu().numpy()
        for j, i in enumerate(mine):
            reads[i] = watermark_reads(got[j], group)[group.index(found[i].key)]
    out = []
    for i, g in enumerate(found):
        read = reads[i]
        if read.detected:                                           # (a span whose own fold stays below the threshold is dropped)
            out.append(wave_codec.WatermarkSpan(g.key, g.start, g.end, read.z, read.offset, read.id, read.id_z))
    return out


def flac_decode_packed(buffer, spans, device=None):
    """`flac_decode` of streams that already lie in one byte buffer: `spans[i] = (first, last + 1)` byte of stream i ("fLaC" included), in
    ascending order and not overlapping; whatever lies between them is not looked at."""
    from . import wave_codec
    buf = np.frombuffer(bytes(buffer), dtype=np.uint8) if not isinstance(buffer, np.ndarray) else np.ascontiguousarray(buffer, dtype=np.uint8)
    n = len(spans)
    if n < 1:
        raise _lib.F5HipError("flac_decode: at least one stream")
    streams, infos = [], []
    for a, b in spans:                                        # everything that needs no samples is refused here, before the device is touched
        if not 0 <= a <= b <= len(buf):
            raise _lib.F5HipError(f"flac_decode: stream bytes [{a}, {b}) of a buffer of {len(buf)}")
        streams.append(buf[a:b].tobytes())
        infos.append(wave_codec.flac_stream_info(streams[-1]))
    host = [wave_codec.flac_needs_host(f) for f in infos]
    results = [None] * n
    if not all(host):
        begin = np.array([a + f["first"] for (a, _), f in zip(spans, infos)], dtype=np.int64)
        end = np.array([b for _, b in spans], dtype=np.int64)
        total = np.array([f["total"] for f in infos], dtype=np.int64)
        most = np.array([wave_codec.FLAC_MAX_SECONDS * f["rate"] for f in infos], dtype=np.int64)
        bound = _lib.lib().f5hip_flac_decode_bound
        info = np.zeros((n, 8), dtype=np.int32)
        for i, f in enumerate(infos):
            cap = int(bound(int(total[i]), int(end[i] - begin[i]), int(most[i])))
            info[i] = (f["channels"], f["bits"], f["rate"], f["min_block"], f["max_block"], cap, int(host[i]), 0)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        with torch.cuda.device(dev):
            data = torch.from_numpy(buf.copy()).to(dev)
            if torch_ops.load():
                out, out_off = call_op("flac_decode", data, torch.from_numpy(begin), torch.from_numpy(end), torch.from_numpy(info), torch.from_numpy(total),
                                       torch.from_numpy(most))
                out_off = out_off.numpy()
            else:
                out_off, words = np.zeros(n, dtype=np.int64), 2 * n
                for i in range(n):
                    out_off[i] = words
                    words += 0 if host[i] else int(info[i, 0]) * int(info[i, 5])
                out = torch.empty(words, device=dev, dtype=torch.int32)
                _lib.check(_lib.lib().f5hip_flac_decode(n, _p(data), data.numel(), _p(begin), _p(end), _p(info), _p(total), _p(most), _p(out), _p(out_off),
                                                        _p(out), _lib.current_stream_ptr()), "f5hip_flac_decode")
            got = out.cpu().numpy()                           # the one download: statuses and samples
        for i, f in enumerate(infos):
            if got[2 * i] == 0:
                cap, count = int(info[i, 5]), int(got[2 * i + 1])
                planes = got[out_off[i]:out_off[i] + f["channels"] * cap].reshape(f["channels"], cap)[:, :count].copy()
                wave_codec.flac_check_md5(planes, f)
                results[i] = (planes, int(f["rate"]), int(f["bits"]))
    for i in range(n):                                        # outside the limits, or refused: the definition decodes it or raises
        if results[i] is None:
            results[i] = wave_codec.read_flac(streams[i])
    return results


def flac_decode(streams, device=None):
    """Native FLAC streams (bytes each) -> [(samples int32 [channels, n], sample_rate, bits)], `wave_codec.read_flac` of each, decoded on the
    device in ONE library call and five launches (include/f5hip.h f5hip_flac_decode) with one upload and one download.  A stream outside the
    device's limits (more than 2 channels, a depth outside 8 .. 24 bits, a block over 16 384) and every stream the device does not accept are
    decoded by `read_flac` on the host, so the samples -- or the ValueError -- are the definition's either way."""
    streams = [bytes(s.tobytes() if isinstance(s, np.ndarray) else s) for s in streams]
    spans, at = [], 0
    for s in streams:
        spans.append((at, at + len(s)))
        at += len(s)
    return flac_decode_packed(b"".join(streams), spans, device)
