"""The reference-clip dereverberator restated from its written definition (single-channel WPE: a delayed linear prediction per frequency
bin, `audio_prep.dereverb_reference`), independently of it: frames filled one by one, the delay line by its index rule, R and p added frame by
frame in ascending order, the filter tap by tap.  With `dtype=np.float32` every array, transform and solve stays in fp32 / complex64 -- what
the device's arithmetic can be expected to reach -- and with `np.float64` it is the definition.  Also the seeded hosts the dereverberator's
tests share: a speech-like dry signal with pauses and noise bursts, and an exponentially decaying noise impulse response."""
import numpy as np

import denoise_ref as R0

N_FFT, HOP, PAD, RATE = R0.N_FFT, R0.HOP, R0.PAD, R0.RATE
DELAY, TAPS, ITERATIONS = 4, 16, 3
FLOOR, LOAD, TINY = 1e-3, 1e-3, 1e-20
n_frames = R0.n_frames


def dereverb(x, dtype=np.float64):
    dt = np.dtype(dtype).type
    ct = np.complex64 if dtype == np.float32 else np.complex128
    x = np.asarray(x, dtype=dtype).reshape(-1)
    n, F = len(x), n_frames(len(x))
    w = np.sin(np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT).astype(dtype)
    frames = np.zeros((F, N_FFT), dtype=dtype)
    for m in range(F):
        first = HOP * m - PAD
        a, b = max(first, 0), min(first + N_FFT, n)
        if a < b:
            frames[m, a - first:b - first] = x[a:b]
    X = np.fft.rfft(frames * w, axis=1)
    assert X.dtype == ct
    bins = X.shape[1]

    def taps(f):                                                  # [bins, TAPS]: x~[f, k, j] = X[f - DELAY - j, k], zero before the clip
        xt = np.zeros((bins, TAPS), dtype=ct)
        for j in range(TAPS):
            if f - DELAY - j >= 0:
                xt[:, j] = X[f - DELAY - j]
        return xt

    PX = X.real * X.real + X.imag * X.imag
    floor = dt(FLOOR) * (PX.sum(axis=0) / dt(F)) + dt(TINY)
    Y = X.copy()
    for _ in range(ITERATIONS):
        PY = Y.real * Y.real + Y.imag * Y.imag
        Rm, p = np.zeros((bins, TAPS, TAPS), dtype=ct), np.zeros((bins, TAPS), dtype=ct)
        for f in range(F):
            lam = np.maximum((PY[max(f - 1, 0)] + PY[f] + PY[min(f + 1, F - 1)]) / dt(3.0), floor)
            xt = taps(f)
            Rm += xt[:, :, None] * xt.conj()[:, None, :] / lam[:, None, None]
            p += xt * X[f].conj()[:, None] / lam[:, None]
        load = dt(LOAD) * np.trace(Rm, axis1=1, axis2=2).real / dt(TAPS) + dt(TINY)
        Rm = Rm + load[:, None, None].astype(dtype) * np.eye(TAPS, dtype=dtype)
        g = np.linalg.solve(Rm, p[:, :, None])[:, :, 0]
        assert g.dtype == ct
        for f in range(F):
            Y[f] = X[f] - (g.conj() * taps(f)).sum(axis=1)
    y = np.fft.irfft(Y, n=N_FFT, axis=1).astype(dtype) * w
    out = np.zeros(HOP * (F - 1) + N_FFT, dtype=dtype)
    for m in range(F):
        out[HOP * m:HOP * m + N_FFT] += y[m]
    return out[PAD:PAD + n] / dt(2.0)


# ------------------------------------------------------------------------------------------------ hosts
EARLY = int(0.050 * RATE)                                          # the first 50 ms of a response: what a listener hears as the voice itself


def dry_speech(n, seed):
    """A speech-like dry signal, float64 [n] of rms 0.1: syllables of 0.12 to 0.3 s, each a harmonic voice with its own gliding pitch (90 to
    220 Hz) and three formants of its own under a raised-cosine envelope, every third one led by a 30 ms noise burst (a consonant), 40 to 120 ms
    of silence between syllables and a pause of 0.4 s after every fifth."""
    rng = np.random.default_rng(seed)
    x, at, count = np.zeros(n), int(0.05 * RATE), 0
    while at < n:
        m = int(rng.uniform(0.12, 0.3) * RATE)
        t = np.arange(m) / RATE
        f0 = rng.uniform(90.0, 220.0) * (1.0 + rng.uniform(-0.2, 0.2) * t / t[-1])
        phase = 2 * np.pi * np.cumsum(f0) / RATE
        formants = np.array([500.0, 1500.0, 2500.0]) * (1.0 + 0.3 * rng.uniform(-1, 1, 3))
        syl = np.zeros(m)
        for h in range(1, 18):
            amp = sum(np.exp(-0.5 * ((h * f0.mean() - fc) / 180.0) ** 2) for fc in formants) + 0.02
            syl += amp * np.sin(h * phase + rng.uniform(0, 2 * np.pi))
        syl *= 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(m) / m)
        if count % 3 == 0:
            b = int(0.03 * RATE)
            syl[:b] += 0.5 * np.abs(syl).max() * rng.standard_normal(b) * np.hanning(b)
        k = min(m, n - at)
        x[at:at + k] = syl[:k]
        count += 1
        at += m + int(rng.uniform(0.04, 0.12) * RATE) + (int(0.4 * RATE) if count % 5 == 0 else 0)
    return x * (0.1 / np.sqrt(np.mean(x * x)))


def room(t60, seed):
    """An exponentially decaying noise impulse response of 1.2 T60 seconds behind a unit direct path: -60 dB at `t60` seconds."""
    m = int(1.2 * t60 * RATE)
    h = np.random.default_rng(seed).standard_normal(m) * 10.0 ** (-3.0 * np.arange(m) / (t60 * RATE)) * 0.1
    h[0] = 1.0
    return h


def host(seconds, t60, seed):
    """(reverberant, early): the dry signal through `room`, and through the room's first 50 ms alone; both float64 [n]."""
    n = int(seconds * RATE)
    dry, h = dry_speech(n, seed), room(t60, seed + 1)
    return np.convolve(dry, h)[:n], np.convolve(dry, h[:EARLY])[:n]


def late_to_early_db(y, early):
    """The power of everything in y that is not the early part, against the early part's, in dB."""
    return 10.0 * np.log10(np.sum((y - early) ** 2) / np.sum(early ** 2))


def device_clips(chunk):
    """name -> float32 clip of peak at most 0.5, the lengths at which the device path can go wrong (`chunk`: the frames its Gram pass stages at
    a time): one sample; F = DELAY (no tap yet) and DELAY + 1 (one tap live); F = DELAY + TAPS - 1 and DELAY + TAPS (the delay line just full);
    one frame past a chunk; 1.5 s; an all-zero clip and a DC clip.  The short clips are white noise, the two long ones reverberant hosts."""
    def noise(n, seed):
        return R0.white_noise(n, seed, 0.01)

    def last_of(F):                                                # the greatest length with F frames
        return HOP * F - PAD

    clips = dict(one_sample=np.array([0.3]), no_tap=noise(last_of(DELAY) - 56, 1), short_one_tap=noise(last_of(DELAY + 1) - 212, 2),
                 line_short_by_one=noise(last_of(DELAY + TAPS - 1), 3), line_full=noise(last_of(DELAY + TAPS) - 152, 4),
                 chunk_plus_one=host(2.0, 0.3, 11)[0][:last_of(chunk + 1) - 100], seconds_1p5=host(1.5, 0.6, 12)[0],
                 zeros=np.zeros(3000), dc=np.full(3000, 0.25))
    return {name: (x * min(1.0, 0.5 / max(np.abs(x).max(), 1e-30))).astype(np.float32) for name, x in clips.items()}
