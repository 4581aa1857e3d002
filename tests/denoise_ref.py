"""The reference-clip denoiser restated from its written definition (quantile noise floor, power spectral subtraction), independently of
`audio_prep.denoise_reference`: frame by frame, `np.sort` for the order statistic, the nine smoothing cells by clamped index tables.  With
`dtype=np.float32` every array and every transform stays in fp32 -- what the device's arithmetic can be expected to reach -- and with
`np.float64` it is the definition.  Also the two seeded signals the denoiser tests share: a speech-like voiced signal with pauses, and white
noise."""
import numpy as np

N_FFT, HOP, PAD = 1024, 256, 768
RANK_DIV, SUBTRACT, MIN_GAIN = 5, 6.75, 0.125
RATE = 24000


def n_frames(n):
    return (n + PAD + HOP - 1) // HOP


def rank(F):
    return (F - 1) // RANK_DIV


def stages(x, dtype=np.float64):
    """Every stage of the definition for a clip x [n]: dict(X, P, floor, S, G, y, out), all in `dtype` (X complex of that width)."""
    dt = np.dtype(dtype).type
    x = np.asarray(x, dtype=dtype).reshape(-1)
    n = len(x)
    F = n_frames(n)
    w = np.sin(np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT).astype(dtype)
    frames = np.zeros((F, N_FFT), dtype=dtype)
    for m in range(F):
        first = HOP * m - PAD
        a, b = max(first, 0), min(first + N_FFT, n)
        if a < b:
            frames[m, a - first:b - first] = x[a:b]
    X = np.fft.rfft(frames * w, axis=1)
    assert X.dtype == (np.complex64 if dtype == np.float32 else np.complex128)
    P = X.real * X.real + X.imag * X.imag
    floor = np.sort(P, axis=0)[rank(F)]
    mi = np.clip(np.arange(F)[:, None] + np.array([-1, 0, 1])[None], 0, F - 1)          # [F, 3] frames of a cell's window
    ki = np.clip(np.arange(513)[:, None] + np.array([-1, 0, 1])[None], 0, 512)          # [513, 3] bins
    S = np.zeros_like(P)
    for a in range(3):
        for b in range(3):
            S = S + P[mi[:, a]][:, ki[:, b]]
    S = S / dt(9.0)
    G = np.full_like(S, dt(MIN_GAIN))
    pos = S > 0
    G[pos] = np.maximum(dt(MIN_GAIN), ((S - dt(SUBTRACT) * floor[None]) / np.where(pos, S, dt(1.0)))[pos])
    y = np.fft.irfft(G * X, n=N_FFT, axis=1).astype(dtype) * w
    out = np.zeros(HOP * (F - 1) + N_FFT, dtype=dtype)
    for m in range(F):
        out[HOP * m:HOP * m + N_FFT] += y[m]
    return dict(X=X, P=P, floor=floor, S=S, G=G, y=y, out=(out[PAD:PAD + n] / dt(2.0)))


def denoise(x, dtype=np.float64):
    return stages(x, dtype)["out"]


# ------------------------------------------------------------------------------------------------ signals
def gate(n, period=1.5, on=0.9, ramp=0.02):
    """A slow gate over n samples at 24 kHz: `on` seconds open of every `period`, raised-cosine ramps of `ramp` seconds inside the open
    part, EXACTLY zero in the pauses."""
    t = (np.arange(n) / RATE) % period
    g = np.where(t < on, 1.0, 0.0)
    g = np.where(t < ramp, 0.5 - 0.5 * np.cos(np.pi * t / ramp), g)
    g = np.where((t >= on - ramp) & (t < on), 0.5 + 0.5 * np.cos(np.pi * (t - (on - ramp)) / ramp), g)
    return g


def speechlike(n, seed, rms=0.1):
    """A 120 Hz harmonic voice with three formant bumps (near 500, 1500 and 2500 Hz) and 3 Hz syllables under `gate`; float64 [n] of the given
    rms.  `seed` fixes the harmonics' phases and the formants' places."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    formants = np.array([500.0, 1500.0, 2500.0]) * (1.0 + 0.05 * rng.uniform(-1, 1, 3))
    x = np.zeros(n)
    for h in range(1, 34):                                  # harmonics up to 3960 Hz
        f = 120.0 * h
        amp = sum(np.exp(-0.5 * ((f - fc) / 180.0) ** 2) for fc in formants) + 0.02
        x += amp * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    x *= (0.55 - 0.45 * np.cos(2 * np.pi * 3.0 * t)) * gate(n)
    return x * (rms / np.sqrt(np.mean(x * x)))


def white_noise(n, seed, power=1.0):
    """Seed-fixed white Gaussian noise, float64 [n], scaled to EXACTLY the mean power `power`."""
    v = np.random.default_rng(seed).standard_normal(n)
    return v * np.sqrt(power / np.mean(v * v))


def noisy_speech(n, seed, snr_db=15.0):
    """(clean, noisy): `speechlike(n, seed)` and the same plus `white_noise(n, seed + 1)` at exactly `snr_db`."""
    s = speechlike(n, seed)
    return s, s + white_noise(n, seed + 1, np.mean(s * s) / 10.0 ** (snr_db / 10.0))


def pause_mask(n, margin=N_FFT):
    """The samples deep inside the pauses of `gate(n)`: at least `margin` samples from any open sample."""
    closed = gate(n) == 0.0
    k = np.ones(2 * margin + 1)
    return np.convolve((~closed).astype(np.float64), k, mode="same") < 0.5


LENGTHS = (1, 255, 256, 257, 769, 1024, 4097, 12000, 60000)      # F = 4, 4, 4, 5, 7, 7, 20, 50, 238; r = 0, 0, 0, 0, 1, 1, 3, 9, 47
SPEECH_FROM = 12000                                                # a clip at least this long holds noisy speech-like content


def clip(n, seed=None):
    """The test clip of n samples, float32: noisy speech-like content (white noise at 15 dB) where the clip is long enough, otherwise random
    samples at an rms of 0.1.  The seed defaults to the length."""
    seed = n if seed is None else seed
    if n >= SPEECH_FROM:
        return noisy_speech(n, seed)[1].astype(np.float32)
    return white_noise(n, seed, 0.01).astype(np.float32)
