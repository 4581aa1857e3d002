// FLAC level 1, the part with no HIP in it: steps 1 to 5 of the level-1 rule (the comment above wave_codec.encode_flac is the definition)
// for one block of 4096 samples, as inline functions that a plain host compiler takes too.  wave_flac_frame_kernel<true> (wave_out.h)
// compiles this text; tools/flac_lpc_check.cpp runs it serially under AddressSanitizer and UBSan, and tests/test_flac_lpc_core.py holds
// that run to the Python definition line for line.
//
// Exactness, in one place:
//   window    w < 2^15 and |x| <= 2^15, so x w < 2^30 (int); |xw| <= 32767 (a short holds it)
//   autocorr  4096 products below 2^30: below 2^42 (long long), any order of summation
//   Levinson  fp64, contraction off in this file: every operation below is one IEEE operation, in the written order
//   quantise  a valid order has cmax < 2^e and shift <= 11 - e, so |a 2^shift| < 2^11: the conversion to int is defined
//   residual  |sum q x| <= 12 * 2048 * 32768 < 2^31 (int); |r| < 2^15 + 2^31 / 2^shift needs long long for the zigzag at shift 0
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FL1_HD __host__ __device__ inline
#else
#define FL1_HD inline
#endif

constexpr int kFl1Block = 4096;
constexpr int kFl1Orders = 4;                      // LPC orders 6, 8, 10, 12
constexpr int kFl1MaxOrder = 12;
constexpr int kFl1Lags = kFl1MaxOrder + 1;
constexpr int kFl1Precision = 12;
constexpr unsigned kFl1Guard = 1u << 21;           // a zigzag residual at or above it drops the order

FL1_HD int fl1_order(int i) { return 6 + 2 * i; }

struct Fl1Order {            // one LPC order of one block after Levinson and the quantisation
    int valid;
    int shift;
    int q[kFl1MaxOrder];     // q[0] multiplies the most recent sample; zero behind the order
};

// w[i] = (32768 (4095^2 - (2 i - 4095)^2)) // 4095^2, with 4095^2 - (2 i - 4095)^2 = 4 i (4095 - i)
FL1_HD int fl1_window(int i) {
    return (int)((131072LL * i * (kFl1Block - 1 - i)) / ((long long)(kFl1Block - 1) * (kFl1Block - 1)));
}
FL1_HD int fl1_windowed(int x, int i) { return (x * fl1_window(i)) >> 15; }

// Steps 3 and 4: the four orders of a block from its autocorrelation R[0 .. 12]
FL1_HD void fl1_levinson(const long long* R, Fl1Order* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int i = 0; i < kFl1Orders; i++) {
        out[i].valid = 0; out[i].shift = 0;
        for (int j = 0; j < kFl1MaxOrder; j++) out[i].q[j] = 0;
    }
    if (R[0] == 0) return;
    double Rf[kFl1Lags], a[kFl1MaxOrder], next[kFl1MaxOrder];
    for (int j = 0; j < kFl1Lags; j++) Rf[j] = (double)R[j];
    double err = Rf[0];
    for (int m = 1; m <= kFl1MaxOrder; m++) {
        double acc = Rf[m];
        for (int j = 0; j < m - 1; j++) {
            const double prod = a[j] * Rf[m - 1 - j];
            acc = acc - prod;
        }
        const double k = acc / err;
        for (int j = 0; j < m - 1; j++) {
            const double prod = k * a[m - 2 - j];
            next[j] = a[j] - prod;
        }
        next[m - 1] = k;
        for (int j = 0; j < m; j++) a[j] = next[j];
        const double kk = k * k;
        const double rest = 1.0 - kk;
        err = err * rest;
        if (!(err > 0.0)) return;                              // order m and every higher order are no candidates
        if (m < 6 || (m & 1)) continue;
        double cmax = 0.0;
        bool finite = true;
        for (int j = 0; j < m; j++) {
            const double v = fabs(a[j]);
            if (!(v <= 1.7976931348623157e308)) finite = false;
            else if (v > cmax) cmax = v;
        }
        if (!finite) continue;                                 // (a coefficient that is not finite: no exponent, no candidate)
        int e = 0;
        if (cmax != 0.0) (void)frexp(cmax, &e);
        int shift = kFl1Precision - 1 - e;
        if (shift > 15) shift = 15;
        if (shift < 0) continue;
        Fl1Order& o = out[(m - 6) >> 1];
        const double scale = (double)(1 << shift);
        for (int j = 0; j < m; j++) {
            const double scaled = a[j] * scale;                // (exact: a power of two, no underflow going up)
            int q = (int)rint(scaled);                         // (round half to even: the default rounding mode)
            q = q < -(1 << (kFl1Precision - 1)) ? -(1 << (kFl1Precision - 1)) : q > (1 << (kFl1Precision - 1)) - 1 ? (1 << (kFl1Precision - 1)) - 1 : q;
            o.q[j] = q;
        }
        o.shift = shift; o.valid = 1;
    }
}

// Step 5 for one sample: x points at sample i >= order of the block; the zigzag of x[i] - ((sum_j q[j] x[i-1-j]) >> shift), saturated at
// 2^32 - 1 (far above the guard, which is all that such a value decides)
template <typename Sample>
FL1_HD unsigned fl1_residual(const Sample* x, const int* q, int order, int shift) {
    int sum = 0;
    for (int j = 0; j < order; j++) sum += q[j] * (int)x[-1 - j];
    const long long r = (long long)x[0] - (long long)(sum >> shift);
    const long long u = r >= 0 ? 2 * r : -2 * r - 1;
    return u > 0xffffffffLL ? 0xffffffffu : (unsigned)u;
}

// Steps 1 to 5 of one block, serially: the orders, and per order whether every residual stays below the guard
FL1_HD void fl1_block(const int16_t* x, Fl1Order* out, int* inside) {
    long long R[kFl1Lags];
    for (int j = 0; j < kFl1Lags; j++) {
        long long s = 0;
        for (int i = j; i < kFl1Block; i++) s += (long long)fl1_windowed(x[i], i) * fl1_windowed(x[i - j], i - j);
        R[j] = s;
    }
    fl1_levinson(R, out);
    for (int c = 0; c < kFl1Orders; c++) {
        inside[c] = 0;
        if (!out[c].valid) continue;
        unsigned top = 0;
        for (int i = fl1_order(c); i < kFl1Block; i++) {
            const unsigned u = fl1_residual(x + i, out[c].q, fl1_order(c), out[c].shift);
            if (u > top) top = u;
        }
        inside[c] = top < kFl1Guard;
    }
}
