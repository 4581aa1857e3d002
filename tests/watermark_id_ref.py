"""The watermark's trace ids restated from their written definition, independently of `wave_codec.mark_pcm16` / `read_watermark`: the
sub-keys from SplitMix64 in Python integers, the combined carrier entry by entry, the mark sample by sample, the read with every correlation
as direct sums (tests/watermark_ref.py `correlate`) and the candidates of a symbol one by one."""
import math

import numpy as np

import watermark_ref as ref

ID_BITS, SYMBOLS, STEP, ID_SHIFT = 30, 3, 16, 24
ID_MAX, ID_THRESHOLD = 2 ** 30 - 1, 6.0
KEY_MAX = 2 ** 48 - 1


def subkey(key, d):
    return 1 + ref.splitmix_outputs(key, 257 + d)[256 + d] % KEY_MAX


def symbols(tag):
    return [(tag >> (10 * d)) & 1023 for d in range(SYMBOLS)]


def combined(key, tag=None):
    """C [P] as Python integers: 2 c_K[m], and with an id + sum_d c_d[(m - 16 s_d) mod P]."""
    c = [int(v) for v in ref.carrier(key)]
    C = [2 * v for v in c]
    if tag is not None:
        for d, s in enumerate(symbols(tag)):
            cd = [int(v) for v in ref.carrier(subkey(key, d))]
            for m in range(ref.P):
                C[m] += cd[(m - STEP * s) % ref.P]
    return C


def mark(x, key, tag=None):
    """int16 [n] -> int16 [n], sample by sample in Python integers."""
    x = [int(v) for v in x]
    n = len(x)
    nb = -(-n // ref.BLOCK)
    A = [sum(abs(v) for v in x[b * ref.BLOCK:(b + 1) * ref.BLOCK]) for b in range(nb)]
    C = combined(key, tag)
    y = []
    for j, v in enumerate(x):
        b = j // ref.BLOCK
        E = max(A[b - 1] if b > 0 else 0, A[b], A[b + 1] if b + 1 < nb else 0)
        y.append(min(max(v + ((E * C[j % ref.P]) >> ID_SHIFT), -32768), 32767))
    return np.asarray(y, dtype=np.int16)


def _z(r, at):
    sigma = math.sqrt(float(np.mean((r - r.mean()) ** 2)))
    return (r[at] - r.mean()) / sigma if sigma > 0 else 0.0


def read(wave, keys):
    """[(key, z, offset, detected, id, id_z)] of the definition."""
    wave = np.asarray(wave)
    x = (wave.astype(np.float64) / 32768.0 if wave.dtype == np.int16 else wave.astype(np.float64)).reshape(-1)[:ref.MAX_SAMPLES]
    if len(x) < ref.MIN_SAMPLES:
        return [(k, 0.0, 0, False, None, 0.0) for k in keys]
    Z = ref.fold(x)
    out = []
    for k in keys:
        r = ref.correlate(Z, k)
        o = int(np.argmax(r))
        z = _z(r, o)
        found, zs = [], []
        for d in range(SYMBOLS):
            rd = ref.correlate(Z, subkey(k, d))
            best = 0
            for s in range(1, 1024):                                    # the smallest argmax
                if rd[(o - STEP * s) % ref.P] > rd[(o - STEP * best) % ref.P]:
                    best = s
            found.append(best)
            zs.append(_z(rd, (o - STEP * best) % ref.P))
        ok = z >= ref.THRESHOLD and all(v >= ID_THRESHOLD for v in zs)
        out.append((k, float(z), o, bool(z >= ref.THRESHOLD), sum(s << (10 * d) for d, s in enumerate(found)) if ok else None, float(min(zs))))
    return out
