"""MXFP8 (OCP Microscaling v1.0) in plain numpy, the definition csrc/gemm8.h states: blocks of 32 consecutive elements along the last axis,
E4M3 ("fn", max 448) codes, one E8M0 scale 2^e per block with e = clamp(floor(log2(amax)) - 8, -127, 127) (a block of zeros: e = -127),
elements v * 2^-e rounded to nearest-even and saturated at +-448; a NaN or an infinity makes its whole block NaN (code 0x7f, e = 0)."""
import numpy as np

BLOCK = 32


def e4m3_encode(x):
    """float64 values -> E4M3 codes (uint8), round to nearest-even, saturating at +-448"""
    x = np.asarray(x, dtype=np.float64)
    a = np.minimum(np.abs(x), 448.0)
    ex = np.floor(np.log2(np.maximum(a, 2.0 ** -6)))          # binade; everything below 2^-6 shares the subnormal step 2^-9
    q = np.minimum(np.rint(a / 2.0 ** (ex - 3)) * 2.0 ** (ex - 3), 448.0)   # np.rint: ties to even
    ex = np.floor(np.log2(np.maximum(q, 2.0 ** -6)))          # the rounding may have reached the next binade
    normal = q >= 2.0 ** -6
    mant = np.where(normal, q / 2.0 ** ex * 8 - 8, q * 2.0 ** 9)
    code = np.where(normal, (ex + 7) * 8, 0) + mant
    return (code.astype(np.uint8) | np.where(np.signbit(x), 0x80, 0).astype(np.uint8))


def e4m3_decode(code):
    code = np.asarray(code, dtype=np.uint8)
    e, m = ((code >> 3) & 15).astype(np.float64), (code & 7).astype(np.float64)
    v = np.where(e > 0, (1 + m / 8) * 2.0 ** (e - 7), m * 2.0 ** -9)
    v = np.where((code & 0x7f) == 0x7f, np.nan, v)
    return np.where(code & 0x80, -v, v)


def quant(x):
    """x [..., K] (K % 32 == 0) -> (codes uint8 [..., K], exponents int32 [..., K / 32])"""
    x = np.asarray(x, dtype=np.float64)
    b = x.reshape(*x.shape[:-1], -1, BLOCK)
    amax = np.abs(b).max(-1)
    bad = ~np.isfinite(amax)
    safe = np.where(bad | (amax == 0), 1.0, amax)
    e = np.clip(np.frexp(safe)[1] - 1 - 8, -127, 127).astype(np.int32)    # frexp: safe = m 2^p with m in [0.5, 1) -> floor(log2) = p - 1
    e = np.where(amax == 0, -127, np.where(bad, 0, e)).astype(np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        codes = e4m3_encode(np.where(bad[..., None], 0.0, np.ldexp(np.where(bad[..., None], 0.0, b), -e[..., None])))
    codes = np.where(bad[..., None], np.uint8(0x7f), codes)
    return codes.reshape(x.shape), e


def dequant(codes, e):
    c = e4m3_decode(codes).reshape(*codes.shape[:-1], -1, BLOCK)
    return np.ldexp(c, e[..., None]).reshape(codes.shape)
