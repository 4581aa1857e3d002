"""The true-peak limiter of `wave_codec.limit_pcm16` once more in Python integers and direct loops, for tests/test_limit_host.py: no numpy, no
doubling, no convolution.  `limit(x, G, c)` takes the gain in Q16 (`wave_codec.limit_gain`: the meter has a restatement of its own,
tests/loudness_ref.py)."""
import math
from operator import mul

M, UNITY = 240, 1 << 16


def _i0(x):
    total, term = 1.0, 1.0
    for k in range(1, 40):
        term *= (x / 2.0) / k
        total += term * term
    return total


def taps():
    rows = []
    for p in (1, 2, 3):
        c = []
        for k in range(12):
            d = k - 5 - p / 4
            c.append(math.sin(math.pi * d) / (math.pi * d) * _i0(5.0 * math.sqrt(1.0 - (d / 6.0) ** 2)) / _i0(5.0))
        rows.append([round(16384.0 * v / sum(c)) for v in c])
    return rows


def window():
    w = [round(65536.0 * (1.0 + math.cos(math.pi * k / (M + 1))) / (2.0 * (M + 1))) for k in range(-M, M + 1)]
    w[M] += UNITY - sum(w)
    return w


def true_peak(x):
    n, t = len(x), taps()
    at = lambda j: x[j] if 0 <= j < n else 0
    return [max([abs(x[i]) << 14] + [abs(sum(row[k] * at(i - 5 + k) for k in range(12))) for row in t]) for i in range(n)]


def limit(x, G, c):
    """(y, m, a): the output, the readings and the gain reduction of the samples x (Python ints)."""
    n, w = len(x), window()
    m = true_peak(x)
    r = [UNITY if m[i] * G <= c << 30 else (c << 46) // (m[i] * G) for i in range(n)]
    rp = [UNITY] * (2 * M) + r + [UNITY] * (2 * M)                       # r over [-2 M, n + 2 M)
    s = [min(rp[u:u + 2 * M + 1]) for u in range(n + 2 * M)]            # s over [-M, n + M)
    a = [sum(map(mul, w, s[i:i + 2 * M + 1])) >> 16 for i in range(n)]
    y = []
    for i in range(n):
        p = x[i] * G * a[i]
        q, rem = divmod(p, 1 << 32)
        q += rem > 1 << 31 or (rem == 1 << 31 and q & 1)
        y.append(min(max(q, -32768), 32767))
    return y, m, a
