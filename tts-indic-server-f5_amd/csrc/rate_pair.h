// The resampler's rate-pair rule, stated once for C++ (Python: wave_codec.rate_pair): the reduced pair of : nf of a resampling and the shape of
// its tap table (wave_codec.resample_taps), rows of L = 2 width + of taps.  Equal rates: 1 : 1 and no table.  Needs <algorithm> and <cmath>
// only: the library (resample.h, wave_out.h) and the torch operators (torch_ops.cpp), which check a table's shape before the library reads it
// with that stride, both include it.
#pragma once
#include <algorithm>
#include <cmath>

static inline int rate_gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

struct RatePair { int of, nf, width, L; };
static inline RatePair rate_pair(int orig_freq, int new_freq) {
    if (orig_freq == new_freq) return RatePair{1, 1, 0, 0};
    const int g = rate_gcd(orig_freq, new_freq), of = orig_freq / g, nf = new_freq / g;
    const int width = (int)std::ceil(6.0 * of / (std::min(of, nf) * 0.99));   // torchaudio: lowpass_filter_width 6, rolloff 0.99
    return RatePair{of, nf, width, 2 * width + of};
}
