// The reference-clip report, the part with no HIP in it: the constants, the run rule of the clipping count, the index geometry of the raw
// side and the checked clip tables of the device call (ref_assess.h, f5hip_ref_assess) as inline functions that a plain host compiler takes
// too.  tools/ref_assess_check.cpp runs them serially under AddressSanitizer and UBSan over tables of exactly their size; that CPU run is the
// evidence for the bounds below.  The definition is audio_prep.assess_reference (written down above it); the spectrum side's geometry is the
// denoiser's (ref_denoise_core.h).
//
// Bounds, in one place:
//   raw     clip c owns raw[off, off + ch * n): channel q is raw[off + q n, off + (q + 1) n).  Flat index i of the clip is channel i / n,
//           sample i % n (ra_channel, ra_sample); ch * n <= 2^31 - 1
//   run     ra_in_run reads x[j - 2 .. j + 2] of ONE channel through ra_hot_at, an index predicate: a position outside [0, n) is not read
//           and is not hot, so a run never continues from a channel's end into the next channel's start, nor across clips
//   means   the 8-bin window k .. k + 7 of k = 0 .. kRaMeans - 1 ends at bin 512: inside a row of P
//   tiles   clip c owns tiles [tile0, tile0 + ra_tiles(F)) of kRaTile frame rows each; tile t of the clip holds its frames kRaTile t ..
//           min(F, kRaTile (t + 1)) - 1 (ra_tile_rows): every frame in exactly one tile, none past the clip's rows
//   table   ra_layout refuses what the call refuses, so a table it accepts has 1 .. kRaMaxClips clips of 1 .. 8 channels with disjoint ranges
#pragma once
#include <math.h>

#include "ref_denoise_core.h"

#define RA_HD RD_HD

constexpr float kRaHot = 0.9990234375f;                              // audio_prep.ASSESS_HOT: 1 - 2^-10, exact in fp32
constexpr float kRaMinPeak = 0.25f;                                  // ASSESS_MIN_PEAK
constexpr int kRaMinRun = 3;                                         // ASSESS_MIN_RUN (ra_in_run is written for 3)
constexpr int kRaBand0 = 3, kRaBand1 = 341;                          // ASSESS_BAND, both ends included
constexpr double kRaFloorToMean = 4.481420117724551;                 // ASSESS_FLOOR_TO_MEAN: -1 / ln(0.8)
constexpr double kRaSpeechFactor = 4.0, kRaBandwidthRel = 1e-5;      // ASSESS_SPEECH_FACTOR, ASSESS_BANDWIDTH_REL
constexpr int kRaMeanBins = 8;                                       // ASSESS_MEAN_BINS
constexpr int kRaMeans = kRdBins - kRaMeanBins + 1;                  // 506 windows per frame
constexpr int kRaWStride = 508;                                      // values per row of the tiles' window sums: 506, padded to 16 bytes
constexpr int kRaTile = 16;                                          // frame rows per block of the frame launch
constexpr int kRaMaxChannels = 8, kRaMaxClips = 4096;                // ASSESS_MAX_CHANNELS; clips in a call
constexpr int kRaRowWords = 10;                                      // ASSESS_ROW: 64-bit words per clip of the output
enum { RA_CLIPPED = 0, RA_PEAK_BITS, RA_SPEECH_FRAMES, RA_K_STAR, RA_N, RA_S, RA_NOISE_DB, RA_SNR_DB, RA_SPEECH_RATIO, RA_BANDWIDTH_HZ };

struct RaClip {
    long long off;      // its first sample in the raw buffer
    long long n;        // samples per channel
    int ch;             // channels
    int tile0;          // the clip's first tile of frame rows (the prepared side; ascending over the table)
};

RA_HD long long ra_total(const RaClip& c) { return c.n * c.ch; }
RA_HD int ra_channel(const RaClip& c, long long i) { return (int)(i / c.n); }
RA_HD long long ra_sample(const RaClip& c, long long i) { return i % c.n; }
RA_HD float ra_threshold(float peak) { return peak * kRaHot; }
// position j of the channel x[0 .. n) is hot: inside the channel and |x[j]| >= thr
RA_HD bool ra_hot_at(const float* x, long long n, long long j, float thr) { return j >= 0 && j < n && fabsf(x[j]) >= thr; }
// sample j of the channel is hot and lies in a run of at least three hot samples of that channel
RA_HD bool ra_in_run(const float* x, long long n, long long j, float thr) {
    static_assert(kRaMinRun == 3, "ra_in_run: the three placements of a run of three around j");
    if (!ra_hot_at(x, n, j, thr)) return false;
    const bool l1 = ra_hot_at(x, n, j - 1, thr), r1 = ra_hot_at(x, n, j + 1, thr);
    return (l1 && r1) || (l1 && ra_hot_at(x, n, j - 2, thr)) || (r1 && ra_hot_at(x, n, j + 2, thr));
}
// `clipped` of a clip from the count of its samples in runs: 0 for a quiet clip and for one whose every sample is hot (zeros, DC)
RA_HD long long ra_clipped(long long in_runs, float peak, long long total) { return peak < kRaMinPeak || in_runs == total ? 0 : in_runs; }
RA_HD int ra_tiles(int F) { return (F + kRaTile - 1) / kRaTile; }
// the frame rows of tile t of a clip of F frames
RA_HD int ra_tile_rows(int F, int t) { return F - t * kRaTile < kRaTile ? F - t * kRaTile : kRaTile; }
RA_HD double ra_bandwidth_hz(int k_star) { return k_star < 0 ? 0.0 : (double)(k_star + kRaMeanBins) * 24000.0 / (double)kRdNfft; }

// ---- host only
enum { RA_OK = 0, RA_CLIPS, RA_NULL, RA_CHANNELS, RA_LENGTH, RA_OFFSET, RA_OVERLAP };

// The raw side's clip table of a call, checked: RA_OK and h[0 .. n) filled, or the reason for the refusal and the clip it is about
inline int ra_layout(int32_t n, const int64_t* raw_offset, const int32_t* channels, const int32_t* raw_len, std::vector<RaClip>& h, int* bad) {
    *bad = 0;
    if (n < 1 || n > kRaMaxClips) return RA_CLIPS;
    if (!raw_offset || !channels || !raw_len) return RA_NULL;
    h.assign((size_t)n, RaClip());
    for (int i = 0; i < n; i++) {
        *bad = i;
        if (channels[i] < 1 || channels[i] > kRaMaxChannels) return RA_CHANNELS;
        if (raw_len[i] < 1 || (long long)raw_len[i] * channels[i] > 2147483647LL) return RA_LENGTH;
        if (raw_offset[i] < 0 || raw_offset[i] > INT64_MAX - 2147483647LL) return RA_OFFSET;
        RaClip& c = h[(size_t)i];
        c.off = raw_offset[i]; c.n = raw_len[i]; c.ch = channels[i]; c.tile0 = 0;
    }
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; i++) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return h[(size_t)a].off < h[(size_t)b].off || (h[(size_t)a].off == h[(size_t)b].off && a < b); });
    for (int i = 1; i < n; i++) {
        const RaClip &a = h[(size_t)order[(size_t)i - 1]], &b = h[(size_t)order[(size_t)i]];
        if (a.off + ra_total(a) > b.off) { *bad = order[(size_t)i]; return RA_OVERLAP; }
    }
    *bad = -1;
    return RA_OK;
}

// The tiles of the prepared side into a checked raw table, from the denoiser's checked table of the same clips: returns their number
inline long long ra_tile_layout(const std::vector<RdClip>& clips, std::vector<RaClip>& h) {
    long long t = 0;
    for (size_t i = 0; i < clips.size(); i++) { h[i].tile0 = (int)t; t += ra_tiles(clips[i].F); }
    return t;
}
