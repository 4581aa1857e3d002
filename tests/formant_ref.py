"""The formant-preserving pitch shift (TD-PSOLA) restated mark by mark and sample by sample in plain Python integers, for
tests/test_formant_host.py: it shares nothing with `wave_codec` -- not the window, not the lag rule, not the chains, not the blend -- so an
agreement of the two is an agreement of two readings of the written definition.  Loops over frames, lags, marks and samples; the one array
expression is the literal sum of one lag's absolute differences (353 x 480 terms a frame are too many for an interpreter)."""
import math
from fractions import Fraction

import numpy as np

HOP, WIN, LAG_MIN, LAG_MAX, MIN_ADVANCE, TABLE = 120, 480, 48, 400, 24, 1024
RATIOS = {1: Fraction(18, 17), 2: Fraction(46, 41), 3: Fraction(44, 37), 4: Fraction(29, 23), 5: Fraction(4, 3), 6: Fraction(41, 29)}


def window():
    """M[0 .. 1024]: the falling half of a Hann window at 2^15, rounded half to even from fp64."""
    return [round(32768.0 * (1.0 + math.cos(math.pi * j / TABLE)) / 2.0) for j in range(TABLE + 1)]


def ratio(semitones):
    return RATIOS[semitones] if semitones > 0 else 1 / RATIOS[-semitones]


def track(x):
    """[(lag, voiced)] per frame of the list of ints x."""
    n = len(x)
    F = -(-n // HOP)
    xt = np.zeros(F * HOP + WIN + LAG_MAX, dtype=np.int64)
    xt[:n] = x
    out = []
    for f in range(F):
        t = f * HOP
        frame = xt[t:t + WIN]
        E = int(np.abs(frame).sum())
        d = {l: int(np.abs(frame - xt[t + l:t + l + WIN]).sum()) for l in range(LAG_MIN, LAG_MAX + 1)}
        dmin = min(d.values())
        lag = next(l for l in range(LAG_MIN, LAG_MAX + 1) if 8 * d[l] <= 8 * dmin + E)
        while lag < LAG_MAX and d[lag + 1] < d[lag]:
            lag += 1
        out.append((lag, E >= 64 * WIN and 2 * d[lag] <= E))
    return out


def analysis_marks(x, frames):
    """[(a, T, voiced)]: one chain from t = 0."""
    n = len(x)
    marks = []
    t = 0
    while t < n:
        lag, voiced = frames[t // HOP]
        if not voiced:
            marks.append((t, HOP, False))
        else:
            if marks and marks[-1][2]:
                lo, hi = max(t - lag // 8, marks[-1][0] + MIN_ADVANCE), t + lag // 8
            else:
                lo, hi = t, t + lag - 1
            best = None
            for j in range(lo, min(hi, n - 1) + 1):
                if best is None or x[j] > x[best]:                      # a strict improvement only: ties stay with the earlier position
                    best = j
            marks.append((best, lag, True))
        t = marks[-1][0] + marks[-1][1]
    return marks


def synthesis_marks(marks, n, semitones):
    """[(u, i)]: i the nearest analysis mark of u, ties to the earlier one, searched over all of them."""
    f = ratio(semitones)
    p, q = f.numerator, f.denominator
    out = []
    if not marks:
        return out
    u, rem = marks[0][0], 0
    while u < n:
        i = min(range(len(marks)), key=lambda k: (abs(marks[k][0] - u), k))
        out.append((u, i))
        _, T, voiced = marks[i]
        if voiced:
            u, rem = u + (T * q + rem) // p, (T * q + rem) % p
        else:
            u += T
    return out


def psola(x, semitones):
    """The n output samples of a list of ints x."""
    n = len(x)
    marks = analysis_marks(x, track(x))
    M = window()
    num, den = [0] * n, [0] * n
    for u, i in synthesis_marks(marks, n, semitones):
        a, T, _ = marks[i]
        for k in range(-T, T + 1):
            j = u + k
            if 0 <= j < n:
                w = M[(abs(k) * TABLE) // T]
                num[j] += w * (x[a + k] if 0 <= a + k < n else 0)
                den[j] += w
    y = []
    for j in range(n):
        v = x[j] if den[j] == 0 else (2 * num[j] + den[j]) // (2 * den[j])
        y.append(min(max(v, -32768), 32767))
    return y
