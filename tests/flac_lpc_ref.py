"""Test-only: the level-1 FLAC rule (the comment above `wave_codec.encode_flac`) once more, in Python ints and floats and written from
that rule, not from `wave_codec` -- the brute-force minimum of a block's subframe, the LPC orders' coefficients -- and the signal matrix the
level-1 tests share.  Nothing here is fast: a block costs about a quarter of a second, so `best` remembers the blocks it has seen."""
from __future__ import annotations

import math

import numpy as np

BLOCK = 4096
ORDERS = (6, 8, 10, 12)
GUARD = 1 << 21
FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))


def zigzag(r):
    return 2 * r if r >= 0 else -2 * r - 1


def rice_bits(u, parts, o):
    """sum over partitions of 4 + min_k (sum(u >> k) + n (1 + k)), u the residuals behind the o warm-up samples of a block of len(u) + o."""
    b = len(u) + o
    plen, total, at = b // parts, 0, 0
    for p in range(parts):
        n = plen - (o if p == 0 else 0)
        part = u[at:at + n]
        at += n
        total += 4 + min(sum(v >> k for v in part) + n * (1 + k) for k in range(15))
    return total


def lpc_orders(x):
    """{order: (valid, shift, q, inside)} of one full block x (ints): steps 1 to 5 of the rule.  `valid`: Levinson and the quantisation gave
    coefficients; `inside`: no zigzag residual reaches the guard (None when not valid)."""
    x = [int(v) for v in x]
    assert len(x) == BLOCK
    d = (BLOCK - 1) ** 2
    xw = [(x[i] * ((32768 * (d - (2 * i - (BLOCK - 1)) ** 2)) // d)) >> 15 for i in range(BLOCK)]
    R = [sum(xw[i] * xw[i - j] for i in range(j, BLOCK)) for j in range(13)]
    out = {o: (False, 0, [0] * o, None) for o in ORDERS}
    if R[0] == 0:
        return out
    err, a = float(R[0]), []
    for m in range(1, 13):
        acc = float(R[m])
        for j in range(m - 1):
            prod = a[j] * float(R[m - 1 - j])
            acc = acc - prod
        k = acc / err
        new = []
        for j in range(m - 1):
            prod = k * a[m - 2 - j]
            new.append(a[j] - prod)
        a = new + [k]
        kk = k * k
        err = err * (1.0 - kk)
        if not err > 0.0:
            break
        if m not in ORDERS:
            continue
        cmax = max(abs(v) for v in a)
        if cmax != cmax or cmax in (math.inf, -math.inf):
            continue
        e = math.frexp(cmax)[1]
        shift = min(11 - e, 15)
        if shift < 0:
            continue
        q = [min(max(round(v * 2.0 ** shift), -2048), 2047) for v in a]
        out[m] = (True, shift, q, residual_inside(x, q, shift))
    return out


def lpc_u(x, q, shift):
    o = len(q)
    return [zigzag(x[i] - (sum(q[j] * x[i - 1 - j] for j in range(o)) >> shift)) for i in range(o, len(x))]


def residual_inside(x, q, shift):
    return max(lpc_u([int(v) for v in x], q, shift)) < GUARD


_seen = {}


def best(x, level):
    """(bits, name) of the block's subframe under the rule at `level`: the brute-force minimum, ties to the earlier candidate."""
    x = [int(v) for v in x]
    key = (tuple(x), level)
    if key in _seen:
        return _seen[key]
    b = len(x)
    if all(v == x[0] for v in x):
        _seen[key] = (8 + 16, "constant")
        return _seen[key]
    parts = 16 if b == BLOCK else 1
    cands = []
    for o in range(min(5, b)):
        c = FIXED[o]
        u = [zigzag(x[i] - sum(c[j] * x[i - 1 - j] for j in range(o))) for i in range(o, b)]
        cands.append((8 + 16 * o + 2 + 4 + rice_bits(u, parts, o), f"fixed{o}"))
    if level == 1 and b == BLOCK:
        for o, (valid, shift, q, inside) in lpc_orders(x).items():
            if valid and inside:
                cands.append((8 + 16 * o + 4 + 5 + 12 * o + 2 + 4 + rice_bits(lpc_u(x, q, shift), parts, o), f"lpc{o}"))
    bits, name = min(cands, key=lambda c: c[0])          # (min keeps the first of equals)
    if 8 + 16 * b < bits:
        bits, name = 8 + 16 * b, "verbatim"
    _seen[key] = (bits, name)
    return _seen[key]


def frame_bytes(x, number, level):
    """The size of the frame of block x as frame `number`: header (sync 2, codes 2, the number, 16-bit block size for a short block, CRC-8),
    the subframe up to a byte, CRC-16."""
    nb = 1 if number < 0x80 else 2 if number < 0x800 else 3
    return 4 + nb + (0 if len(x) == BLOCK else 2) + 1 + (best(x, level)[0] + 7) // 8 + 2


def _crc16_step(c, byte):
    c ^= byte << 8
    for _ in range(8):
        c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


def frames_of(stream):
    """[(name, size)] of the frames of a mono 16-bit stream of 4096-sample blocks, read from the stream alone: the subframe's type from its
    header byte ("constant", "verbatim", "fixedN", "lpcN"), the frame's end from its CRC-16 (the first sync code, or the stream's end, in
    front of which the two bytes are the CRC of everything before them)."""
    data = bytes(stream)
    assert data[:4] == b"fLaC" and data[4] == 0x80
    total = int.from_bytes(data[18:26], "big") & ((1 << 36) - 1)
    out, pos, f = [], 42, 0
    while pos < len(data):
        b = min(BLOCK, total - BLOCK * f)
        nb = 1 if f < 0x80 else 2 if f < 0x800 else 3
        assert data[pos:pos + 2] == b"\xff\xf8" and b > 0
        body = pos + 4 + nb + (0 if b == BLOCK else 2) + 1
        code = data[body] >> 1
        name = "constant" if code == 0 else "verbatim" if code == 1 else f"fixed{code - 8}" if 8 <= code <= 12 else f"lpc{code - 31}"
        assert code in (0, 1) or 8 <= code <= 12 or 32 <= code <= 63, code
        crcs, end = [0], None                                # crcs[k]: CRC-16 of data[pos : pos + k]
        for j in range(pos, len(data)):
            crcs.append(_crc16_step(crcs[-1], data[j]))
            k = j + 1 - pos                                  # a frame of k bytes would end behind byte j
            if k >= body - pos + 3 and (j + 1 == len(data) or data[j + 1:j + 3] == b"\xff\xf8") and crcs[k - 2] == (data[j - 1] << 8 | data[j]):
                end = j + 1
                break
        assert end is not None, f"frame {f} has no end"
        out.append((name, end - pos))
        pos, f = end, f + 1
    return out


# ----------------------------------------------------------------------------------------------------------------------- the signal matrix
LENGTHS = (0, 1, 12, 13, 4095, 4096, 4097, 8192 + 5)
LONGEST = 8192 + 5


def _clip(v):
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def resonance(n, seed=7, radius=0.97, angle=0.6, gain=900.0):
    """A second-order resonance driven by noise."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n) * gain
    y = np.zeros(n)
    a1, a2 = 2 * radius * math.cos(angle), -radius * radius
    for i in range(n):
        y[i] = e[i] + (a1 * y[i - 1] if i >= 1 else 0.0) + (a2 * y[i - 2] if i >= 2 else 0.0)
    return _clip(y)


def signals(n=LONGEST):
    """{name: int16 [n]}: every signal is a prefix of its longer self, so the lengths of the matrix share their first blocks."""
    rng = np.random.default_rng(2024)
    t = np.arange(n)
    smooth = 20000.0 * np.sin(2 * np.pi * t / 2000.0)
    smooth[:16] = np.where(t % 2 == 0, 32767, -32768)[:16]
    edges = np.zeros(n)
    for f in range(0, n, BLOCK):                         # non-zero only in the first two and last two samples of each block
        e = min(f + BLOCK, n)
        edges[f:f + 2] = (30000, -30000)[:max(0, min(2, e - f))]
        if e - f >= 4:
            edges[e - 2:e] = (-30000, 30000)
    return {
        "zeros": np.zeros(n, dtype=np.int16),
        "constant": np.full(n, -1234, dtype=np.int16),
        "noise": rng.integers(-32768, 32768, n).astype(np.int16),
        "walk": _clip(np.cumsum(rng.integers(-40, 41, n))),
        "quiet_sine": _clip(200.0 * np.sin(2 * np.pi * t / 300.0)),
        "sine041": _clip(12000.0 * np.sin(2 * np.pi * 0.41 * t) + rng.integers(-3, 4, n)),
        "square": np.where(t % 2 == 0, 32767, -32768).astype(np.int16),
        "resonance": resonance(n),
        "smooth_loud_head": _clip(smooth),
        "edges": _clip(edges),
    }


def filtered_noise_blocks(count, seed=99):
    """int16 [count, 4096]: noise through random stable all-pole filters of order 2 to 12 (poles inside radius 0.99) at random gains."""
    rng = np.random.default_rng(seed)
    out = np.empty((count, BLOCK), dtype=np.int16)
    for c in range(count):
        order = int(rng.integers(2, 13))
        poles = []
        while len(poles) < order:
            if order - len(poles) >= 2 and rng.random() < 0.8:
                p = rng.uniform(0.3, 0.99) * np.exp(1j * rng.uniform(0.05, 3.09))
                poles += [p, np.conj(p)]
            else:
                poles.append(complex(rng.uniform(-0.95, 0.95)))
        a = np.real(np.poly(poles))                      # y[i] = e[i] - sum a[j] y[i-j]
        e = rng.standard_normal(BLOCK + 256)
        y = np.zeros(BLOCK + 256)
        for i in range(len(y)):
            y[i] = e[i] - sum(a[j] * y[i - j] for j in range(1, min(order, i) + 1))
        y = y[256:]
        out[c] = _clip(y / max(np.abs(y).max(), 1e-9) * 10.0 ** rng.uniform(1.0, 4.5))
    return out
