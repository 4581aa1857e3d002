// wave_codec.truepeak_taps(): phase p = 1, 2, 3 of the 4x true-peak interpolator, t[p][k] = rint(2^14 c_k / sum c) with c_k = sinc(d)
// I0(5 sqrt(1 - (d / 6)^2)) / I0(5) at d = k - 5 - p / 4: the point i + p / 4 from x[i - 5 .. i + 6].  The largest sum |t[p]| is
// 31400.  Written by tools/gen_limit_tables.py; tests/test_limit_host.py compares it with the function.
-80, 241, -562, 1186, -2678, 14709, 4753, -1738, 820, -376, 146, -37,
-79, 268, -653, 1395, -3022, 10283, 10283, -3022, 1395, -653, 268, -79,
-37, 146, -376, 820, -1738, 4753, 14709, -2678, 1186, -562, 241, -80,
