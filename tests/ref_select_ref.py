"""The reference-stretch selection restated from its written definition (audio_prep.select_reference), independently of it: the windows
by a loop, each window's floor by a sort per bin, every sum by a loop in ascending order, the clipped samples from every channel's runs.
With `dtype=np.float32` every array, transform and sum stays in fp32 -- what the device's arithmetic can be expected to reach -- and with
`np.float64` it is the definition.  Also the signal the selection's tests share."""
import math

import numpy as np

import assess_ref as A
import denoise_ref as R

HOP = 48


def windows(F, W, hop=HOP):
    return [(0, F)] if F < W else [(f0, W) for f0 in range(0, F - W + 1, hop)]


def clipped_flags(raw):
    """int [n]: per sample index, the channels in which it is one of the report's clipped samples (none where the report counts 0)."""
    raw = np.asarray(raw, dtype=np.float32)
    raw = raw.reshape(1, -1) if raw.ndim == 1 else raw
    peak = np.float32(np.abs(raw).max())
    flags = np.zeros(raw.shape[1], dtype=np.int64)
    hot = np.abs(raw) >= np.float32(peak * np.float32(A.HOT))
    if peak < np.float32(A.MIN_PEAK) or hot.all():
        return flags
    for row in hot:                                       # the channel's runs from their edges: [start, end) pairs
        edges = np.flatnonzero(np.diff(np.concatenate([[0], row.astype(np.int8), [0]])))
        for a, b in zip(edges[0::2], edges[1::2]):
            if b - a >= A.MIN_RUN:
                flags[a:b] += 1
    return flags


def table(raw, sr, prepared, W, hop=HOP, dtype=np.float64):
    """(rows float64 [windows, 5]: clipped, speech, N, S, snr_db; E [F]) in `dtype`."""
    dt = np.dtype(dtype).type
    prepared = np.asarray(prepared).reshape(-1)
    P = A.powers(prepared, dtype)
    E = np.zeros(P.shape[0], dtype=dtype)
    for k in A.BAND:
        E = E + P[:, k]
    flags = clipped_flags(raw)
    rows = []
    for f0, Ww in windows(P.shape[0], W, hop):
        floor = np.sort(P[f0:f0 + Ww], axis=0)[R.rank(Ww)]
        floor_sum, total = dt(0.0), dt(0.0)
        for k in A.BAND:
            floor_sum = floor_sum + floor[k]
        for f in range(f0, f0 + Ww):
            total = total + E[f]
        N, S = float(dt(A.FLOOR_TO_MEAN) * floor_sum), float(total / dt(Ww))
        speech = sum(1 for f in range(f0, f0 + Ww) if E[f] >= dt(A.SPEECH_FACTOR) * dt(N) and E[f] > 0)
        j0, j1 = max(0, 256 * f0 - 768) * sr // 24000, min(len(prepared), 256 * (f0 + Ww)) * sr // 24000
        snr = math.inf if not N > 0 else (10.0 * math.log10((S - N) / N) if S > N else -math.inf)
        rows.append([float(flags[j0:j1].sum()), float(speech), N, S, snr])
    return np.array(rows, dtype=np.float64), E


def ranked(rows):
    """The windows from the best key to the worst."""
    return sorted(range(len(rows)), key=lambda w: (rows[w][0], -rows[w][4], w))


def key_margin(rows):
    """How far the best key is from the runner-up: (the runner-up's clipped minus the best's, the best's snr_db minus the runner-up's)."""
    a, b = (rows[w] for w in ranked(rows)[:2])
    if b[0] > a[0] or (math.isinf(a[4]) and a[4] == b[4]):       # (equal infinities: the window index decides, exactly, on either side)
        return b[0] - a[0], math.inf
    return 0.0, a[4] - b[4]


def staged(frames, seed, quiet_from=None):
    """A recording of exactly `frames` frames (its length is no multiple of the hop), float32: speech-like content over white noise whose
    level falls by 24 dB along the recording, so that the windows' snr_db differ by far more than rounding.  `quiet_from` (a fraction): the
    rest is exact digital silence."""
    n = 256 * (frames - 3) - 17 if frames > 4 else 200
    s = R.speechlike(n, seed)
    level = np.mean(s * s) / 10.0 ** (np.linspace(4.0, 28.0, n) / 10.0)
    x = s + np.random.default_rng(seed + 1).standard_normal(n) * np.sqrt(level)
    if quiet_from is not None:
        x[int(quiet_from * n):] = 0.0
    return x.astype(np.float32)
