// Time-scale modification of finished PCM, the part with no HIP in it: the index geometry, the tie rule and the blend of the WSOLA launch
// (wave_out.h wave_wsola_kernel, f5hip_wave_prosody) as inline functions that a plain host compiler takes too.  tools/wave_prosody_check.cpp
// runs them serially under AddressSanitizer and UBSan over tables of exactly their size; that CPU run is the evidence for the bounds below.
// The definition is wave_codec.wsola_pcm16 (written down above wave_codec.wsola_window):
//   m = ceil(n P / Q) outputs, K = ceil(m / H) + 1 frames of L = 960 samples at hop H = 480, nominal starts p_k = floor(k H Q / P) - H,
//   s_0 = -H; for k >= 1 the start s_k = p_k + d_k, d_k in -D .. D (D = 240) minimising sum_{i < L} |xt[p_k + d + i] - xt[s_{k-1} + H + i]|,
//   ties to the smaller |d|, then to the negative one; y[k H + i] = (W[H + i] xt[s_k + H + i] + W[i] xt[s_{k+1} + i] + 16384) >> 15.
//
// Bounds, in one place:
//   x       pr_source reads x[j] only for 0 <= j < n: every other index is the zero of xt, an index predicate and never a read
//   window  frame k's candidates lie in win[0 .. kPrWindow) = xt[p_k - D .. p_k + D + L): candidate c = d + D reads win[c .. c + L), c <= 2 D
//   target  tgt[0 .. L) = xt[s_{k-1} + H ..): the search reads all of it, the blend its first H samples (the falling half of frame k - 1)
//   blend   frame k's rising half is win[c_k .. c_k + H): inside the window, no second read of x
//   sums    a cost is below 960 * 65535 < 2^26, a key cost * 2^9 + rank below 2^35; k H Q and n P stay below 2^63 for P, Q <= kPrMaxTerm and
//           fewer than 2^31 samples; the blend's numerator stays within 2^30 + 2^14
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PR_HD __host__ __device__ inline
#else
#define PR_HD inline
#endif

constexpr int kPrFrame = 960, kPrHop = 480, kPrSearch = 240;        // wave_codec.PROSODY_FRAME, PROSODY_HOP, PROSODY_SEARCH
constexpr int kPrCands = 2 * kPrSearch + 1;                         // 481 search offsets
constexpr int kPrWindow = 2 * kPrSearch + kPrFrame;                 // 1440 source samples hold every candidate of a frame
constexpr int kPrMaxTerm = 1 << 20;                                 // P and Q at most this: 64-bit products
constexpr int kPrPitchMax = 6;                                      // semitones either way
// p / q per semitone (wave_codec.PITCH_RATIOS): +1 .. +6; a negative step takes the reciprocal
constexpr int kPrPitchP[kPrPitchMax] = {18, 46, 44, 29, 4, 41}, kPrPitchQ[kPrPitchMax] = {17, 41, 37, 23, 3, 29};

struct PrGeom {
    long long n;        // input samples
    long long m;        // output samples, ceil(n P / Q)
    long long K;        // frames, ceil(m / H) + 1 (0 for an empty output)
    int P, Q;
};

PR_HD PrGeom pr_geom(long long n, int P, int Q) {
    PrGeom g;
    g.n = n; g.P = P; g.Q = Q;
    g.m = (n * P + Q - 1) / Q;
    g.K = g.m ? (g.m + kPrHop - 1) / kPrHop + 1 : 0;
    return g;
}

// whether P / Q is a stretch the search can follow: both terms in 1 .. kPrMaxTerm and 1/2 <= P / Q <= 2
PR_HD bool pr_stretch_ok(long long P, long long Q) { return P >= 1 && Q >= 1 && P <= kPrMaxTerm && Q <= kPrMaxTerm && P <= 2 * Q && Q <= 2 * P; }

// frame k's nominal start p_k (k >= 0; p_0 = -H = s_0)
PR_HD long long pr_nominal(const PrGeom& g, long long k) { return (k * kPrHop * g.Q) / g.P - kPrHop; }

// (of, nf) = (p, q) of a pitch step s in -6 .. 6, s != 0: the resampler's rate pair (host: the kernels get it per request)
inline void pr_pitch_ratio(int s, int* p, int* q) {
    const int a = s < 0 ? -s : s;
    *p = s < 0 ? kPrPitchQ[a - 1] : kPrPitchP[a - 1];
    *q = s < 0 ? kPrPitchP[a - 1] : kPrPitchQ[a - 1];
}

// the tie rule: offsets 0, -1, 1, -2, 2, ... rank 0, 1, 2, 3, 4, ...; a key orders by cost, then by rank, and does not depend on who found it
PR_HD int pr_rank(int d) { return d < 0 ? -2 * d - 1 : 2 * d; }
PR_HD int pr_offset_of_rank(int r) { return (r & 1) ? -((r + 1) >> 1) : (r >> 1); }
PR_HD unsigned long long pr_key(unsigned cost, int d) { return ((unsigned long long)cost << 9) | (unsigned)pr_rank(d); }
PR_HD int pr_key_offset(unsigned long long key) { return pr_offset_of_rank((int)(key & 511)); }

// xt[j] biased by 32768 (order and absolute differences are those of the samples; the zero outside the wave is 0x8000)
PR_HD unsigned pr_source(const short* x, long long n, long long j) { return (j >= 0 && j < n ? (unsigned)(unsigned short)x[j] : 0u) ^ 0x8000u; }
PR_HD int pr_unbias(unsigned v) { return (int)v - 32768; }

// one output: `rise` = W[i], a = the falling frame's sample, b = the rising frame's (a floor shift: >> on a negative int is arithmetic)
PR_HD int pr_blend(int rise, int a, int b) { return ((32768 - rise) * a + rise * b + 16384) >> 15; }
