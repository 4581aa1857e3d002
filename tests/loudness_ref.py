"""A float64 mono programme-loudness meter written from ITU-R BS.1770-4, for the tests of the integer meter: the two K-weighting biquads run
as recursions, 400 ms blocks every 100 ms, the -70 LUFS absolute gate and the -10 LU relative gate.  It imports nothing from the package.

The biquads come from the analytic design libebur128 and pyloudnorm use, which at 48 kHz reproduces the standard's table; that is asserted
when the module is loaded (the table's high-pass a2 is itself rounded in the standard, hence its own figure)."""
import math

import numpy as np

SHELF = dict(f0=1681.974450955533, G=3.999843853973347, Q=0.7071752369554196, vb_exp=0.4996667741545416)
HIGH_PASS = dict(f0=38.13547087602444, Q=0.5003270373238773)


def biquads(fs):
    """[(b, a)] of the shelf and the high-pass at the rate fs, a[0] = 1."""
    K = math.tan(math.pi * SHELF["f0"] / fs)
    Vh = 10.0 ** (SHELF["G"] / 20.0)
    Vb = Vh ** SHELF["vb_exp"]
    Q = SHELF["Q"]
    a0 = 1.0 + K / Q + K * K
    shelf = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0), (1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    K = math.tan(math.pi * HIGH_PASS["f0"] / fs)
    Q = HIGH_PASS["Q"]
    a0 = 1.0 + K / Q + K * K
    high = (1.0, -2.0, 1.0), (1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    return [shelf, high]


# BS.1770-4, tables 1 and 2 (48 kHz)
_TABLE = [((1.53512485958697, -2.69169618940638, 1.19839281085285), (1.0, -1.69065929318241, 0.73248077421585)),
          ((1.0, -2.0, 1.0), (1.0, -1.99004745483398, 0.99007225036621))]
for (_b, _a), (_tb, _ta) in zip(biquads(48000.0), _TABLE):
    assert all(abs(x - y) <= 1e-9 for x, y in zip(_b + _a, _tb + _ta)), (_b, _a, _tb, _ta)


def k_weight(x, fs):
    """The K-weighted signal: both biquads as direct-form-I recursions in float64, from rest."""
    y = [float(v) for v in x]
    for b, a in biquads(fs):
        b0, b1, b2 = b
        _, a1, a2 = a
        x1 = x2 = y1 = y2 = 0.0
        out = []
        for v in y:
            w = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
            x2, x1, y2, y1 = x1, v, y1, w
            out.append(w)
        y = out
    return np.asarray(y, dtype=np.float64)


def block_loudness(x, fs):
    """The loudness of every 400 ms block (75 % overlap) of samples at full scale 1: -0.691 + 10 log10(mean square), -inf for a silent one."""
    step, z = int(round(0.1 * fs)), k_weight(x, fs)
    nb = len(z) // step - 3
    if nb < 1:
        return np.zeros(0)
    sq = np.concatenate([[0.0], np.cumsum(z * z)])
    ms = np.array([(sq[(b + 4) * step] - sq[b * step]) / (4 * step) for b in range(nb)])
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(ms)


def integrated_loudness(x, fs=24000):
    """The gated programme loudness in LUFS of mono samples at full scale 1 (int16 PCM: divide by 32768 first); None when no block passes
    the gates."""
    L = block_loudness(x, fs)
    ms = 10.0 ** ((L + 0.691) / 10.0)
    keep = L > -70.0
    if not keep.any():
        return None
    rel = -0.691 + 10.0 * math.log10(ms[keep].mean()) - 10.0
    keep &= L > rel
    if not keep.any():
        return None
    return -0.691 + 10.0 * math.log10(ms[keep].mean())
