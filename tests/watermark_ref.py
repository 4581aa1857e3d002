"""The provenance watermark restated from its written definition, independently of `wave_codec.mark_pcm16` / `detect_watermark`: the chips
bit by bit from Python integers, the carrier as 129 rolled copies of the chips, the mark sample by sample, the detector frame by frame with
the correlation over the offsets as direct sums (no FFT across the period).  Also the seeded hosts the watermark tests share."""
import functools
import math

import numpy as np

import denoise_ref

P, BLOCK, TAPS, SHIFT = 16384, 240, 129, 23
BAND = (22, 136)
THRESHOLD, MIN_SAMPLES, MAX_SAMPLES = 7.0, 12000, 1_440_000
N_FFT, HOP, PAD = 1024, 256, 768
MASK = (1 << 64) - 1


def splitmix_outputs(key, count):
    state, out = key, []
    for _ in range(count):
        state = (state + 0x9E3779B97F4A7C15) & MASK
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        out.append(z ^ (z >> 31))
    return out


def chips(key):
    return [1 if (z >> i) & 1 else -1 for z in splitmix_outputs(key, P // 64) for i in range(64)]


def taps():
    g = []
    for k in range(TAPS):
        hann = 0.5 - 0.5 * math.cos(2.0 * math.pi * (k + 1) / 130.0)
        hi, lo = 2.0 * 3200.0 / 24000.0, 2.0 * 500.0 / 24000.0
        g.append(int(np.rint(2.0 ** 14 * hann * (hi * np.sinc(hi * (k - 64)) - lo * np.sinc(lo * (k - 64))))))
    return g


@functools.lru_cache(maxsize=8)
def carrier(key):
    ch = np.asarray(chips(key), dtype=np.int64)
    acc = np.zeros(P, dtype=np.int64)
    for k, g in enumerate(taps()):
        acc += g * np.roll(ch, k - 64)              # roll(ch, s)[m] = ch[(m - s) mod P]
    c = acc >> 3
    c.setflags(write=False)
    return c


def mark(x, key):
    """int16 [n] -> int16 [n], sample by sample in Python integers."""
    x = [int(v) for v in x]
    n = len(x)
    nb = -(-n // BLOCK)
    A = [sum(abs(v) for v in x[b * BLOCK:(b + 1) * BLOCK]) for b in range(nb)]
    c = carrier(key)
    y = []
    for j, v in enumerate(x):
        b = j // BLOCK
        E = max(A[b - 1] if b > 0 else 0, A[b], A[b + 1] if b + 1 < nb else 0)
        y.append(min(max(v + ((E * int(c[j % P])) >> SHIFT), -32768), 32767))
    return np.asarray(y, dtype=np.int16)


def fold(x):
    """Z [P] of a clip x (fp64 [n]): frame by frame, explicit overlap-add, then the fold residue by residue."""
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
        for k in range(BAND[0], BAND[1] + 1):
            U[k] = X[k] / math.sqrt(X[k].real ** 2 + X[k].imag ** 2 + 1e-10)
        u[HOP * m:HOP * m + N_FFT] += np.fft.irfft(U, n=N_FFT) * w
    u = u[PAD:PAD + n]
    Z = np.zeros(P)
    for j0 in range(0, n, P):
        seg = u[j0:j0 + P]
        Z[:len(seg)] += seg
    return Z


def correlate(Z, key):
    """r [P]: r[o] = sum_m Z[m] c[(m + o) mod P], as direct sums (a block of offsets at a time)."""
    cc = np.concatenate([carrier(key), carrier(key)]).astype(np.float64)
    r = np.empty(P)
    for o0 in range(0, P, 512):
        r[o0:o0 + 512] = np.lib.stride_tricks.sliding_window_view(cc[o0:o0 + 511 + P], P) @ Z
    return r


def detect(wave, keys):
    """[(key, z, offset, detected)] of the definition."""
    wave = np.asarray(wave)
    x = (wave.astype(np.float64) / 32768.0 if wave.dtype == np.int16 else wave.astype(np.float64)).reshape(-1)[:MAX_SAMPLES]
    if len(x) < MIN_SAMPLES:
        return [(k, 0.0, 0, False) for k in keys]
    Z = fold(x)
    out = []
    for k in keys:
        r = correlate(Z, k)
        o = int(np.argmax(r))
        sigma = math.sqrt(float(np.mean((r - r.mean()) ** 2)))
        z = (r[o] - r.mean()) / sigma if sigma > 0 else 0.0
        out.append((k, float(z), o, z >= THRESHOLD))
    return out


# ------------------------------------------------------------------------------------------------ hosts
@functools.lru_cache(maxsize=64)
def host(n, seed, noisy=False, peak=12000):
    """int16 [n] (read-only): `denoise_ref.speechlike(n, seed)`, or with `noisy` the same in white noise at 25 dB, its peak scaled to `peak`."""
    s = denoise_ref.noisy_speech(n, seed, 25.0)[1] if noisy else denoise_ref.speechlike(n, seed)
    x = np.rint(s * (peak / np.abs(s).max())).astype(np.int16)
    x.setflags(write=False)
    return x
