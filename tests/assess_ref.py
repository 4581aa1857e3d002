"""The reference-clip report restated from its written definition (audio_prep.assess_reference), independently of it: the clipping count by
a plain loop over every channel's runs, the spectrum frame by frame (tests/denoise_ref.py's framing), every sum by a loop in ascending order.
With `dtype=np.float32` every array, transform and sum stays in fp32 -- what the device's arithmetic can be expected to reach -- and with
`np.float64` it is the definition.  Also the signals the report's tests share."""
import math

import numpy as np

import denoise_ref as R

HOT = 1.0 - 2.0 ** -10
MIN_PEAK, MIN_RUN = 0.25, 3
BAND = range(3, 342)
FLOOR_TO_MEAN = -1.0 / math.log(0.8)
SPEECH_FACTOR, MEAN_BINS, BANDWIDTH_REL = 4.0, 8, 1e-5
FLOAT_MEASURES = ("N", "S", "noise_db", "snr_db", "speech_ratio", "bandwidth_hz")


def clipping(raw):
    """(peak float32, clipped) of raw [ch, n] float32: the runs of every channel walked one sample at a time."""
    raw = np.asarray(raw, dtype=np.float32)
    raw = raw.reshape(1, -1) if raw.ndim == 1 else raw
    peak = np.float32(0.0)
    for row in raw:
        for v in row:
            peak = max(peak, np.float32(abs(v)))
    thr = np.float32(peak * np.float32(HOT))
    if peak < np.float32(MIN_PEAK):
        return peak, 0
    clipped, hot_total = 0, 0
    for row in raw:
        run = 0
        for v in list(row) + [None]:                    # (the sentinel ends the channel's last run: no run continues into the next channel)
            if v is not None and np.float32(abs(v)) >= thr:
                run += 1
                continue
            hot_total += run
            if run >= MIN_RUN:
                clipped += run
            run = 0
    return peak, (0 if hot_total == raw.size else clipped)


def powers(x, dtype):
    """P [F, 513] of the clip x in `dtype`: the denoiser's framing and window, frame by frame."""
    x = np.asarray(x, dtype=dtype).reshape(-1)
    n, F = len(x), R.n_frames(len(x))
    w = np.sin(np.pi * np.arange(R.N_FFT, dtype=np.float64) / R.N_FFT).astype(dtype)
    frames = np.zeros((F, R.N_FFT), dtype=dtype)
    for m in range(F):
        first = R.HOP * m - R.PAD
        a, b = max(first, 0), min(first + R.N_FFT, n)
        if a < b:
            frames[m, a - first:b - first] = x[a:b]
    X = np.fft.rfft(frames * w, axis=1)
    assert X.dtype == (np.complex64 if dtype == np.float32 else np.complex128)
    return X.real * X.real + X.imag * X.imag


def spectrum(prepared, dtype=np.float64):
    """The spectral measures of a prepared clip in `dtype`, with the values the threshold decisions are made on:
    dict(F, E [F], m [506], N, S, noise_db, snr_db, speech_frames, speech_ratio, k_star, bandwidth_hz)."""
    dt = np.dtype(dtype).type
    P = powers(np.asarray(prepared).reshape(-1)[:1_440_000], dtype)
    F = P.shape[0]
    floor = np.sort(P, axis=0)[R.rank(F)]
    E = np.zeros(F, dtype=dtype)
    for k in BAND:
        E = E + P[:, k]
    floor_sum, total = dt(0.0), dt(0.0)
    for k in BAND:
        floor_sum = floor_sum + floor[k]
    for f in range(F):
        total = total + E[f]
    N, S = dt(FLOOR_TO_MEAN) * floor_sum, total / dt(F)
    speech = int(sum(1 for f in range(F) if E[f] >= dt(SPEECH_FACTOR) * N and E[f] > 0))
    w = np.zeros((F, 513 - MEAN_BINS + 1), dtype=dtype)
    for d in range(MEAN_BINS):
        w = w + P[:, d:d + w.shape[1]]
    w = w / dt(MEAN_BINS)
    m = np.zeros(w.shape[1], dtype=dtype)
    for f in range(F):
        m = m + w[f]
    m = m / dt(F)
    top = m.max()
    k_star = max(k for k in range(len(m)) if m[k] >= dt(BANDWIDTH_REL) * top) if top > 0 else -1
    N, S = float(N), float(S)
    return dict(F=F, E=E, m=m, N=N, S=S, speech_frames=speech, k_star=k_star,
                noise_db=10.0 * math.log10(N) if N > 0 else -math.inf,
                snr_db=math.inf if not N > 0 else (10.0 * math.log10((S - N) / N) if S > N else -math.inf),
                speech_ratio=speech / F, bandwidth_hz=(k_star + MEAN_BINS) * 24000.0 / 1024 if k_star >= 0 else 0.0)


def near_thresholds(s, rel=1e-3):
    """From a float64 `spectrum`: (bins of m within a relative `rel` of the bandwidth threshold, frames of E within `rel` of the speech
    threshold) -- the decisions another arithmetic may make the other way."""
    thr_m, thr_e = BANDWIDTH_REL * float(s["m"].max()), SPEECH_FACTOR * s["N"]
    bins = [k for k, v in enumerate(s["m"]) if thr_m > 0 and abs(float(v) - thr_m) <= rel * thr_m]
    frames = [f for f, v in enumerate(s["E"]) if thr_e > 0 and abs(float(v) - thr_e) <= rel * thr_e]
    return bins, frames


# ------------------------------------------------------------------------------------------------ signals
def calibration_host(snr_db, seconds=6.0, seed=11):
    """(clean, noise): `denoise_ref.speechlike` (40 % pauses) and white noise at exactly `snr_db` below it, float64 at 24 kHz."""
    n = int(seconds * R.RATE)
    s = R.speechlike(n, seed)
    return s, R.white_noise(n, seed + 1, np.mean(s * s) / 10.0 ** (snr_db / 10.0))


def true_snr_db(clean, noise):
    """The SNR of a calibration host from its known parts, inside the report's band: the ratio of the two parts' own S."""
    return 10.0 * math.log10(spectrum(clean)["S"] / spectrum(noise)["S"])


def lowpass(x, cutoff_hz, taps=511):
    """x through a Kaiser-windowed (beta 10) sinc low-pass with its -6 dB point at `cutoff_hz` (24 kHz samples), same length."""
    t = np.arange(taps) - (taps - 1) / 2
    h = 2 * cutoff_hz / R.RATE * np.sinc(2 * cutoff_hz / R.RATE * t) * np.kaiser(taps, 10.0)
    return np.convolve(x, h / h.sum(), mode="same")


def run_cases():
    """name -> float32 [ch, n]: the clipping rule's cases, each with the count the definition gives."""
    top, a = np.float32(32767 / 32768), np.float32(0.3)

    def ch(*v):
        return np.array(v, dtype=np.float32)

    return {
        "run2": (ch(a, 1, 1, a, -a, a, a, a)[None], 0),
        "run3": (ch(a, 1, -1, 1, a, a, a, a)[None], 3),
        "channel_edge": (np.stack([ch(a, a, a, a, a, a, 1, 1), ch(1, a, a, a, a, a, a, a)]), 0),       # 2 at the end + 1 at the start: not joined
        "channel_edge_runs": (np.stack([ch(a, a, a, a, a, 1, 1, 1), ch(1, 1, a, a, a, a, a, a)]), 3),  # 3 at the end count, the 2 behind do not
        "run_at_0": (ch(1, 1, 1, 1, a, a, a, a)[None], 4),
        "run_at_end": (ch(a, a, a, a, a, -1, -1, -1)[None], 3),
        "quiet": (ch(0.2, 0.2, 0.2, 0.2, 0.1, 0.1, 0.1, 0.1)[None], 0),                              # peak < 0.25
        "int16_tops": (ch(a, top, top, -1, top, a, a, top)[None], 4),                                  # 32767 / 32768 against -1.0: all hot
        "zeros": (np.zeros((1, 9), dtype=np.float32), 0),
        "dc": (np.full((2, 9), 0.5, dtype=np.float32), 0),
        "one_sample": (ch(0.7)[None], 0),
        "two_separate_runs": (ch(1, 1, 1, a, 1, 1, a, 1, 1, 1, 1)[None], 7),
    }
