"""The tempo / pitch definition restated sample by sample in plain Python integers, for tests/test_prosody_host.py: it shares nothing with
`wave_codec` -- not the window, not the geometry, not the tie rule, not the stretch -- so an agreement of the two is an agreement of two
readings of the written definition.  The resampler's tap table is data and is handed in."""
import math
from fractions import Fraction
from operator import sub

L, H, D = 960, 480, 240
RATIOS = {1: Fraction(18, 17), 2: Fraction(46, 41), 3: Fraction(44, 37), 4: Fraction(29, 23), 5: Fraction(4, 3), 6: Fraction(41, 29)}


def window():
    """W[0 .. 960): the rising half rounded half to even from fp64, the falling half its complement to 2^15."""
    rise = [round(32768.0 * math.sin(math.pi * (2 * i + 1) / (2 * L)) ** 2) for i in range(H)]
    return rise + [32768 - w for w in rise]


def ratio(semitones):
    return Fraction(1) if semitones == 0 else RATIOS[semitones] if semitones > 0 else 1 / RATIOS[-semitones]


def stretch(hundredths, semitones):
    """(P, Q) in lowest terms of a tempo in whole hundredths and a pitch in semitones."""
    f = ratio(semitones) * Fraction(100, hundredths)
    return f.numerator, f.denominator


def wsola(x, P, Q):
    """(y, s) of a list of ints x: the m = ceil(n P / Q) output samples and the frame starts, with no shortcut for P == Q."""
    n = len(x)
    m = -((-n * P) // Q)
    if m == 0:
        return [], [-H]

    def xt(a, b):   # xt[a .. b) as a list
        return [x[j] if 0 <= j < n else 0 for j in range(a, b)]

    K = -(-m // H) + 1
    s = [-H]
    for k in range(1, K):
        p = (k * H * Q) // P - H
        target = xt(s[-1] + H, s[-1] + H + L)
        source = xt(p - D, p + D + L)
        best = None
        for d in sorted(range(-D, D + 1), key=lambda d: (abs(d), d)):   # 0, -1, 1, -2, 2, ...: the first strict minimum in this order
            cost = sum(map(abs, map(sub, source[d + D:d + D + L], target)))
            if best is None or cost < best[0]:
                best = (cost, d)
        s.append(p + best[1])
    W = window()
    y = []
    for j in range(m):
        k, i = divmod(j, H)
        a = s[k] + H + i
        b = s[k + 1] + i
        va = x[a] if 0 <= a < n else 0
        vb = x[b] if 0 <= b < n else 0
        y.append((W[H + i] * va + W[i] * vb + 16384) >> 15)
    return y, s


def polyphase(y, p, q, width, taps):
    """ceil(q m / p) samples of the m samples y: output j = b q + r is the sum over k, ascending, of taps[r][k] * ypad[b p + k] in fp64, ypad
    = y with `width` zeros in front and zeros behind; rounded half to even, clipped to int16.  taps: q rows of 2 width + p floats."""
    m = len(y)
    out = []
    for j in range(-((-q * m) // p)):
        b, r = divmod(j, q)
        acc = 0.0
        for k, t in enumerate(taps[r]):
            at = b * p + k - width
            acc = acc + t * float(y[at] if 0 <= at < m else 0)
        out.append(min(max(round(acc), -32768), 32767))
    return out


def shift(x, hundredths, semitones, taps=None, width=None):
    """`tempo` (whole hundredths) and `pitch` on a list of ints: WSOLA by the combined stretch, then the resampler p : q for a pitch."""
    P, Q = stretch(hundredths, semitones)
    y = list(x) if (hundredths, semitones) == (100, 0) else wsola(x, P, Q)[0]
    if semitones:
        f = ratio(semitones)
        y = polyphase(y, f.numerator, f.denominator, width, taps)
    return y
