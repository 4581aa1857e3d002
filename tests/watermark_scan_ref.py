"""The watermark scan restated from its written definition (above `wave_codec.scan_watermark`), independently of it: the whitened band
frame by frame, every window's and span's fold as sums over explicit sample indices (no padding, no reshape), the span rule as a state
machine over one window at a time, the symbols candidate by candidate.  It shares with `wave_codec` only the carriers and the idea of
forming the correlation over the offsets with fp64 FFTs."""
import math

import numpy as np

from tts_indic_server_f5_amd import wave_codec

P, W, SLACK = 16384, 2, 2
THRESHOLD, ID_THRESHOLD, MIN_SAMPLES, MAX_SAMPLES = 7.0, 6.0, 12000, 14_400_000
N_FFT, HOP, PAD = 1024, 256, 768
BAND = (22, 136)


def whitened(x):
    """u [n] of fp64 samples x [n], one frame at a time, overlap-added in ascending frame order."""
    n = len(x)
    F = (n + PAD + HOP - 1) // HOP
    w = np.sin(np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT)
    u = np.zeros(HOP * (F - 1) + N_FFT)
    for m in range(F):
        first = HOP * m - PAD
        frame = np.zeros(N_FFT)
        a, b = max(first, 0), min(first + N_FFT, n)
        if a < b:
            frame[a - first:b - first] = x[a:b]
        X = np.fft.rfft(frame * w)
        U = np.zeros_like(X)
        k = slice(BAND[0], BAND[1] + 1)
        U[k] = X[k] / np.sqrt(X[k].real ** 2 + X[k].imag ** 2 + 1e-10)
        u[HOP * m:HOP * m + N_FFT] += np.fft.irfft(U, n=N_FFT) * w
    return u[PAD:PAD + n]


def fold_segments(u, first, last):
    """Z [P] of segments first .. last - 1 of u [n]: Z[m] = sum_s u[s P + m], s ascending, a sample at or past n counting zero."""
    n, Z = len(u), np.zeros(P)
    for s in range(first, last):
        count = max(0, min(n - s * P, P))
        Z[:count] += u[s * P:s * P + count]
    return Z


def correlation(Z, key):
    """r [P], r[o] = sum_m Z[m] c[(m + o) mod P]."""
    c = wave_codec.watermark_carrier(key).astype(np.float64)
    return np.fft.irfft(np.conj(np.fft.rfft(Z)) * np.fft.rfft(c), n=P)


def score(r):
    """(z, offset) of a correlation: the smallest argmax against the population deviation."""
    o, best = 0, r[0]
    for i in range(1, P):
        if r[i] > best:
            o, best = i, r[i]
    mean = float(np.sum(r)) / P
    sigma = math.sqrt(float(np.sum((r - mean) ** 2)) / P)
    return ((float(best) - mean) / sigma if sigma > 0 else 0.0), o


def symbol(r, offset):
    """(s, z_s) of a sub-key's correlation: the best of the 1024 candidates r[(offset - 16 s) mod P], ties to the smaller s."""
    s_best, best = 0, r[offset % P]
    for s in range(1, 1024):
        v = r[(offset - 16 * s) % P]
        if v > best:
            s_best, best = s, v
    mean = float(np.sum(r)) / P
    sigma = math.sqrt(float(np.sum((r - mean) ** 2)) / P)
    return s_best, ((float(best) - mean) / sigma if sigma > 0 else 0.0)


def spans_of(detected, offsets, n):
    """[(first window a, last window b)] of one key from its windows' decisions and offsets: the state machine of the span rule."""
    runs, state, a, prev = [], "out", 0, 0
    for w in range(len(detected)):
        if state == "in":
            gap = (offsets[w] - prev) % P
            if not detected[w] or min(gap, P - gap) > SLACK:
                runs.append((a, w - 1))
                state = "out"
        if detected[w]:
            if state == "out":
                state, a = "in", w
            prev = offsets[w]
    if state == "in":
        runs.append((a, len(detected) - 1))
    return runs


def scan(wave, keys):
    """[(key, start, end, z, offset, id, id_z)] of the definition, sorted by (start, position of the key)."""
    wave = np.asarray(wave)
    x = (wave.astype(np.float64) / 32768.0 if wave.dtype == np.int16 else wave.astype(np.float64)).reshape(-1)
    n = len(x)
    assert n <= MAX_SAMPLES
    if n < MIN_SAMPLES:
        return []
    u = whitened(x)
    S = (n + P - 1) // P
    windows = max(1, S - W + 1)
    out = []
    for pos, key in enumerate(keys):
        decided, offsets = [], []
        for w in range(windows):
            z, o = score(correlation(fold_segments(u, w, min(w + W, S)), key))
            decided.append(z >= THRESHOLD)
            offsets.append(o)
        for a, b in spans_of(decided, offsets, n):
            last = min(b + W, S)
            Z = fold_segments(u, a, last)
            z, o = score(correlation(Z, key))
            if z < THRESHOLD:
                continue
            symbols = [symbol(correlation(Z, wave_codec.watermark_subkey(key, d)), o) for d in range(3)]
            id_z = min(zs for _, zs in symbols)
            value = sum(s << (10 * d) for d, (s, _) in enumerate(symbols)) if all(zs >= ID_THRESHOLD for _, zs in symbols) else None
            out.append((a * P, pos, (key, a * P, min(n, last * P), z, o, value, id_z)))
    return [t for _, _, t in sorted(out, key=lambda t: t[:2])]
