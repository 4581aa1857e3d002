// The reference-clip denoiser, the part with no HIP in it: the constants, the row geometry and the checked clip table of the device call
// (ref_denoise.h, f5hip_ref_denoise) as inline functions that a plain host compiler takes too.  tools/ref_denoise_check.cpp walks them
// serially under AddressSanitizer and UBSan over tables of exactly their size; that CPU run is the evidence for the bounds below.  The
// definition is audio_prep.denoise_reference (written down above it):
//   F = ceil((n + 768) / 256) frames of 1024 samples at hop 256, frame m = clip samples 256 m - 768 .. 256 m + 255 (zeros outside the
//   clip) times w[i] = sin(pi i / 1024); P = |rfft|^2; floor[k] = the r-th smallest of P[0 .. F)[k], r = (F - 1) / 5; S = the mean of P over
//   the 3 x 3 cells around (m, k), indices clamped; G = max(1/8, (S - 6.75 floor) / S); y_m = irfft(G X) w; out = overlap_add(y) / 2.
//
// Bounds, in one place:
//   clip    rd_frame_sample(m, i) is an index predicate: the kernels read x[j] only for 0 <= j < n; every other index is a zero
//   rows    clip c owns rows [row0, row0 + F) of X [rows][513], P [rows][kRdPStride] and fw [rows][1024]; a frame index is in [0, F)
//   smooth  rd_clamp keeps the nine cells of (m, k) in rows [0, F) and bins [0, 513): always nine reads, none outside the clip's rows
//   ola     sample j lies in frames rd_sample_frame0(j) .. + 3, all below F, at offsets rd_sample_offset(j, m) in [0, 1024)
//   table   rd_layout refuses what the call refuses, so a table it accepts has rows and samples below 2^31 and disjoint ranges
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define RD_HD __host__ __device__ inline
#else
#define RD_HD inline
#endif

constexpr int kRdNfft = 1024, kRdHop = 256, kRdPad = 768;           // audio_prep.DENOISE_N_FFT, DENOISE_HOP, DENOISE_PAD
constexpr int kRdBins = kRdNfft / 2 + 1;                            // 513
constexpr int kRdPStride = 516;                                     // floats per row of P: 513 bins, padded to 16 bytes
constexpr int kRdRankDiv = 5;                                       // DENOISE_RANK_DIV
constexpr float kRdSubtract = 6.75f, kRdMinGain = 0.125f;           // DENOISE_SUBTRACT, DENOISE_MIN_GAIN
constexpr int kRdMaxSamples = 1440000;                              // DENOISE_MAX_SAMPLES: 60 s at 24 kHz
constexpr int kRdFramesPerSample = kRdNfft / kRdHop;                // every clip sample lies in exactly four frames

struct RdClip {
    long long off;      // its first sample in the wave
    long long out0;     // the samples of the clips before it in the table (the overlap-add launch's thread space)
    int n;              // samples
    int F;              // frames
    int row0;           // its first row of X, P and fw
    int pad_;
};

RD_HD int rd_frames(long long n) { return (int)((n + kRdPad + kRdHop - 1) / kRdHop); }
RD_HD int rd_rank(int F) { return (F - 1) / kRdRankDiv; }
// the clip sample under position i of frame m (outside [0, n): a zero)
RD_HD long long rd_frame_sample(int m, int i) { return (long long)m * kRdHop - kRdPad + i; }
// the first of the four frames that hold sample j, and j's position in frame m
RD_HD int rd_sample_frame0(long long j) { return (int)(j / kRdHop); }
RD_HD int rd_sample_offset(long long j, int m) { return (int)(j + kRdPad - (long long)m * kRdHop); }
// the smoothing window's clamp: index i of [0, hi)
RD_HD int rd_clamp(int i, int hi) { return i < 0 ? 0 : (i >= hi ? hi - 1 : i); }

// ---- host only
enum { RD_OK = 0, RD_NO_CLIPS, RD_NULL, RD_LENGTH, RD_OFFSET, RD_OVERLAP, RD_ROWS };

// The clip table of a call, checked: RD_OK and h[0 .. n), *rows and *samples filled, or the reason for the refusal and the clip it is about
inline int rd_layout(int32_t n, const int64_t* offset, const int32_t* n_samples, std::vector<RdClip>& h, long long* rows, long long* samples, int* bad) {
    *bad = 0;
    if (n < 1) return RD_NO_CLIPS;
    if (!offset || !n_samples) return RD_NULL;
    h.assign((size_t)n, RdClip());
    long long r = 0, s = 0;
    for (int i = 0; i < n; i++) {
        *bad = i;
        if (n_samples[i] < 1 || n_samples[i] > kRdMaxSamples) return RD_LENGTH;
        if (offset[i] < 0 || offset[i] > INT64_MAX - kRdMaxSamples) return RD_OFFSET;
        RdClip& c = h[(size_t)i];
        c.off = offset[i]; c.out0 = s; c.n = n_samples[i]; c.F = rd_frames(c.n); c.row0 = (int)r; c.pad_ = 0;
        r += c.F; s += c.n;
        if (r > 2147483647LL) return RD_ROWS;
    }
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; i++) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return offset[a] < offset[b] || (offset[a] == offset[b] && a < b); });
    for (int i = 1; i < n; i++) {
        const int a = order[(size_t)i - 1], b = order[(size_t)i];
        if (offset[a] + n_samples[a] > offset[b]) { *bad = b; return RD_OVERLAP; }
    }
    *rows = r; *samples = s; *bad = -1;
    return RD_OK;
}
