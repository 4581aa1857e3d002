// The reference-clip dereverberator, the part with no HIP in it: the constants, the delay-line geometry of a frame chunk and the checked clip
// table of the device call (ref_dereverb.h, f5hip_ref_dereverb) as inline functions that a plain host compiler takes too.
// tools/ref_dereverb_check.cpp walks them serially under AddressSanitizer and UBSan over tables of exactly their size; that CPU run is the
// evidence for the bounds below.  The definition is audio_prep.dereverb_reference (written down above it); the framing is the denoiser's
// (ref_denoise_core.h).
//
// Bounds, in one place:
//   stage   a chunk of kRvChunk frames starting at frame `base` stages X of frames base - kRvHalo .. base + kRvChunk - 1 of ONE bin in
//           xs[kRvStage]; rv_stage_frame gives slot s its frame, and a frame outside [0, F) is a zero, never a read
//   taps    frame base + t reads tap j (X of frame base + t - D - j) at slot rv_tap_slot(t, j) in [0, kRvStage) and its own X at
//           rv_own_slot(t): 0 <= t < kRvChunk, 0 <= j < K
//   power   slot s of ps[kRvPow] holds |Y|^2 of frame clamp(base - 1 + s): lam of frame base + t reads slots t, t + 1, t + 2
//   grid    one workgroup per (clip, group of kRvGroupBins bins): n * kRvGroups of them, which rv_layout keeps below 2^31
#pragma once
#include "ref_denoise_core.h"

constexpr int kRvDelay = 4, kRvTaps = 16, kRvIters = 3;              // audio_prep.DEREVERB_DELAY, DEREVERB_TAPS, DEREVERB_ITERATIONS
constexpr float kRvFloorRel = 1e-3f, kRvLoadRel = 1e-3f, kRvTiny = 1e-20f;   // DEREVERB_FLOOR, DEREVERB_LOAD, DEREVERB_TINY
constexpr int kRvChunk = 128;                                        // frames a workgroup stages at a time (f5hip_ref_dereverb_chunk)
constexpr int kRvHalo = kRvDelay + kRvTaps - 1;                      // frames in front of a chunk that its taps reach: 19
constexpr int kRvStage = kRvChunk + kRvHalo;                         // slots of xs
constexpr int kRvPow = kRvChunk + 2;                                 // slots of ps
constexpr int kRvGroupBins = 8;                                      // bins per workgroup: one wave each
constexpr int kRvGroups = (kRdBins + kRvGroupBins - 1) / kRvGroupBins;   // 65
constexpr int kRvCols = 2 * kRvTaps;                                 // the real embedding [Re x~ | Im x~]: 32 columns, one MFMA tile

RD_HD int rv_chunks(int F) { return (F + kRvChunk - 1) / kRvChunk; }
RD_HD int rv_stage_frame(int base, int s) { return base - kRvHalo + s; }
RD_HD int rv_tap_slot(int t, int j) { return t + kRvTaps - 1 - j; }
RD_HD int rv_own_slot(int t) { return t + kRvHalo; }
RD_HD int rv_pow_frame(int base, int s, int F) { return rd_clamp(base - 1 + s, F); }

// ---- host only
// rd_layout's table and refusals, and one more: a call whose (clip, bin group) grid would pass 2^31 - 1 workgroups is RD_ROWS too
inline int rv_layout(int32_t n, const int64_t* offset, const int32_t* n_samples, std::vector<RdClip>& h, long long* rows, long long* samples, int* bad) {
    if (n > 2147483647 / kRvGroups) { *bad = 0; return RD_ROWS; }
    return rd_layout(n, offset, n_samples, h, rows, samples, bad);
}
