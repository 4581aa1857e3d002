// The provenance watermark, the part with no HIP in it: the constants, the carrier, the block geometry and the sample arithmetic of the mark
// (wave_mark.h wave_mark_sum_kernel / wave_mark_add_kernel, f5hip_wave_mark) and the geometry and the tie rule of the detector
// (f5hip_watermark_detect) as inline functions that a plain host compiler takes too.  tools/wave_mark_check.cpp runs them serially under
// AddressSanitizer and UBSan over tables of exactly their size; that CPU run is the evidence for the bounds below.  The definition is
// wave_codec.mark_pcm16 / detect_watermark (written down above wave_codec.check_watermark):
//   chips    SplitMix64 with state `key`; bit i of output k is chip 64 k + i, +1 set and -1 clear; P = 16384 chips
//   carrier  c[m] = (sum_k g[k] chip[(m - k + 64) mod P]) >> 3, g = watermark_taps.inc (129 taps, sum |g| = 34684): |c| <= 4336
//   mark     A[b] = sum |x[j]| over block b of 240 samples; E[b] = max(A[b-1], A[b], A[b+1]), a missing neighbour counting 0;
//            y[j] = clip(x[j] + ((E[j / 240] c[j mod P]) >> 23)), a 64-bit product and a floor shift
//
// Bounds, in one place:
//   x        wm_block_sum reads x[j] only for j < len: a block past the length sums to 0, which is what a missing neighbour counts
//   A        launch 1 writes all kWmTileBlocks sums of every tile, so A holds tiles * kWmTileBlocks values; wm_envelope reads A[b - 1 .. b + 1]
//            only inside [0, nA)
//   carrier  a sample j reads c[j & (P - 1)]; a group of 8 samples starts at a multiple of 8 and P is one, so it reads 8 values of one row
//   sums     A <= 240 * 32768 < 2^23; |E c| < 2^23 * 2^13 = 2^36; |E c >> 23| <= 4336 * 0.9375 < 4066
//
// Trace ids (wave_mark_id_add_kernel / f5hip_wave_mark_ids, watermark_id_score_kernel / f5hip_watermark_read_ids; the definition is written
// down in wave_codec.py beside the mark's): a key has kWmTagRows = 4 carrier rows, its own and its three sub-keys';
//   symbols  s_d = (id >> 10 d) & 1023; C[m] = 2 c_K[m] + sum_d c_d[(m - 16 s_d) mod P]; y[j] = clip(x[j] + ((E C[j mod P]) >> 24))
//   read     candidate s of sub-key d is r_d[(o* - 16 s) mod P]; ties to the smaller s
// Bounds:
//   rows     a group of 8 samples starts at j = 0 mod 8 and 16 s_d = 0 mod 8, so wm_id_index is a multiple of 8 at most P - 8: 8 values of
//            one row, 16-byte aligned when the rows are; a request of key k reads rows 4 k .. 4 k + 3 of n_keys * 4
//   sums     |C| <= 5 * 4336 = 21680; |E C| < 2^23 * 2^15 = 2^38; |E C >> 24| <= 21680 * 0.9375 / 2 = 10162.5, so |y - x| <= 10163
//   grid     wd_id_offset is in [0, P) for o* in [0, P) and s in [0, 1024)
//
// The scan of one long recording (ws_range_fold_kernel / f5hip_watermark_scan; the definition is wave_codec.scan_watermark, written down
// above it): the recording of n samples is S = ws_segments(n) segments of P samples, the last one zero-filled; a range is `count`
// consecutive segments from segment `first`; its row is Z[m] = sum over its segments s ascending of u[s P + m], u the whitened band of the
// whole recording, u[j] = its four frames added in ascending frame order (the detector's framing: 768 zeros in front, 1024 at hop 256).
// Bounds:
//   range    ws_range_ok admits 0 <= first, 1 <= count, first + count <= S, so ws_range_first < n and 1 <= ws_range_samples <= count P
//   samples  residue m of a range reads u[j] for j = first P + m + k P < first P + ws_range_samples = min(n, (first + count) P): only j < n;
//            a sample at or past n is the zero fill and is not read
//   frames   sample j < n lies in frames ws_sample_frame0(j) .. + 3 at offsets ws_sample_offset in [0, 1024); the last of them is
//            (n - 1) / 256 + 3 <= ws_frames(n) - 1, so every read stays inside fw [ws_frames(n)][1024]
//   slabs    the correlate and score launches take ws_slab_ranges(n_rows) ranges at a time, a function of the carrier rows alone: r never
//            holds more than kWsSlabRows rows of P floats (256 MiB)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WM_HD __host__ __device__ inline
#else
#define WM_HD inline
#endif

constexpr int kWmPeriod = 16384;                      // wave_codec.WATERMARK_PERIOD
constexpr int kWmBlock = 240;                         // WATERMARK_BLOCK
constexpr int kWmTaps = 129;                          // WATERMARK_TAPS
constexpr int kWmShift = 23;                          // WATERMARK_SHIFT
constexpr int kWmCarrierShift = 3;
constexpr int kWmKeysMax = 16;                        // WATERMARK_KEYS_MAX
constexpr unsigned long long kWmKeyMax = (1ULL << 48) - 1;
constexpr int kWmTileBlocks = 32;                     // 240-sample blocks per tile of either launch
constexpr int kWmTile = kWmBlock * kWmTileBlocks;     // 7680 samples: a multiple of 8, so a group of 8 samples lies in one block
static_assert(kWmBlock % 8 == 0 && kWmPeriod % 8 == 0, "wave_mark: a group of 8 samples shares its block and its carrier row");

constexpr int kWmIdSymbols = 3;                       // WATERMARK_ID_SYMBOLS
constexpr int kWmIdStep = 16;                         // WATERMARK_ID_STEP
constexpr int kWmIdSymbolBits = 10;                   // WATERMARK_ID_BITS / WATERMARK_ID_SYMBOLS
constexpr int kWmIdSymbolCount = 1 << kWmIdSymbolBits;
constexpr int kWmIdMax = (1 << (kWmIdSymbols * kWmIdSymbolBits)) - 1;   // WATERMARK_ID_MAX
constexpr int kWmIdShift = kWmShift + 1;              // WATERMARK_ID_SHIFT: the key's carrier counts twice in C
constexpr int kWmTagRows = 1 + kWmIdSymbols;          // carrier rows of a key: its own, then its sub-keys 0 .. 2
constexpr int kWdIdKeysMax = kWmKeysMax / kWmTagRows; // WATERMARK_ID_KEYS_MAX: keys of one f5hip_watermark_read_ids call
constexpr int kWdIdRowWords = 4 + 2 * kWmIdSymbols;   // z, o*, r[o*], sigma, then (s_d, z_d) per symbol
static_assert(kWmIdStep % 8 == 0 && kWmIdStep * kWmIdSymbolCount == kWmPeriod, "wave_mark: a rotation keeps a group of 8 samples in one row, and the symbols cover the period");

constexpr int kWdBandLo = 22, kWdBandHi = 136;        // WATERMARK_BAND: bins of the 1024-point STFT
constexpr int kWdMinSamples = 12000;                  // WATERMARK_MIN_SAMPLES
constexpr float kWdThreshold = 7.0f;                  // WATERMARK_THRESHOLD
constexpr float kWdEps = 1e-10f;                      // under the square root of the unit-modulus step
constexpr int kWdOffTile = 512;                       // offsets one block of the correlation launch owns
constexpr int kWdGroup = 4;                           // clips that share one staged carrier window there
constexpr int kWdChunk = 512;                         // residues staged at a time there

// ---- the mark
WM_HD long long wm_tiles(long long cap) { return cap > 0 ? (cap + kWmTile - 1) / kWmTile : 1; }   // (an empty request keeps one block)

// A[b] of a request of `len` samples: the masked sum of block b's magnitudes
WM_HD int wm_block_sum(const short* x, long long len, long long b) {
    int s = 0;
    for (long long j = b * kWmBlock; j < (b + 1) * kWmBlock && j < len; j++) s += x[j] < 0 ? -(int)x[j] : (int)x[j];
    return s;
}

// E[b] from the nA block sums of a request
WM_HD int wm_envelope(const int* A, long long nA, long long b) {
    int e = A[b];
    if (b > 0 && A[b - 1] > e) e = A[b - 1];
    if (b + 1 < nA && A[b + 1] > e) e = A[b + 1];
    return e;
}

// one marked sample (>> on a negative long long is arithmetic: floor)
WM_HD int wm_mark(int x, int E, int c) {
    const long long y = (long long)x + (((long long)E * (long long)c) >> kWmShift);
    return (int)(y < -32768 ? -32768 : (y > 32767 ? 32767 : y));
}

// symbol d of a trace id, and where sample j of a request reads sub-key row d rotated by symbol s
WM_HD int wm_id_symbol(int id, int d) { return (id >> (kWmIdSymbolBits * d)) & (kWmIdSymbolCount - 1); }
WM_HD int wm_id_index(long long j, int s) { return (int)((j - (long long)kWmIdStep * s) & (kWmPeriod - 1)); }

// one marked sample from the combined carrier C = 2 c_K (+ the rotated sub-key carriers): wm_mark(x, E, c) when C = 2 c
WM_HD int wm_mark_id(int x, int E, int C) {
    const long long y = (long long)x + (((long long)E * (long long)C) >> kWmIdShift);
    return (int)(y < -32768 ? -32768 : (y > 32767 ? 32767 : y));
}

// ---- the detector
// the offset of sub-key d's correlation that candidate symbol s reads, o the key's offset
WM_HD int wd_id_offset(int o, int s) { return (o - kWmIdStep * s) & (kWmPeriod - 1); }

// whether (v, i) takes the place of (bv, bi) as the maximum of r: the larger value, at equal values the smaller offset
WM_HD bool wd_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// ---- the scan of one recording: ranges of whole segments
constexpr int kWsWindow = 2;                          // WATERMARK_SCAN_WINDOW: segments per window
constexpr int kWsSlack = 2;                           // WATERMARK_SCAN_SLACK
constexpr int kWsMaxSamples = 14400000;               // WATERMARK_SCAN_MAX_SAMPLES: 600 s at 24 kHz
constexpr int kWsRangesMax = 4096;                    // ranges of one call: Z [ranges][P] stays within 256 MiB
constexpr int kWsSlabRows = 4096;                     // rows of r [P] one correlate launch writes: 256 MiB
constexpr int kWsNfft = 1024, kWsHop = 256, kWsPad = 768;   // the detector's framing (ref_denoise_core.h kRdNfft, kRdHop, kRdPad)
constexpr int kWsFramesPerSample = kWsNfft / kWsHop;

WM_HD int ws_segments(long long n) { return (int)((n + kWmPeriod - 1) / kWmPeriod); }
WM_HD int ws_frames(long long n) { return (int)((n + kWsPad + kWsHop - 1) / kWsHop); }
WM_HD bool ws_range_ok(long long n, long long first, long long count) { return first >= 0 && count >= 1 && first + count <= ws_segments(n); }
// the first sample of a range, and how many of the recording's n samples it holds (the rest of its last segment is the zero fill)
WM_HD long long ws_range_first(int first) { return (long long)first * kWmPeriod; }
WM_HD int ws_range_samples(long long n, int first, int count) {
    const long long end = (long long)(first + count) * kWmPeriod;
    return (int)((end < n ? end : n) - ws_range_first(first));
}
// the sample that segment k of a range starting at sample j0 adds to residue m (at or past j0 + the range's samples: the zero fill)
WM_HD long long ws_fold_sample(long long j0, int m, int k) { return j0 + m + (long long)k * kWmPeriod; }
// the first of the four frames that hold sample j, and j's position in frame f
WM_HD int ws_sample_frame0(long long j) { return (int)(j / kWsHop); }
WM_HD int ws_sample_offset(long long j, int f) { return (int)(j + kWsPad - (long long)f * kWsHop); }
// ranges per correlate / score launch of a call with n_rows carrier rows (1 .. 16), and the slabs of a call
WM_HD int ws_slab_ranges(int n_rows) { return kWsSlabRows / n_rows; }
WM_HD int ws_slabs(int n_ranges, int n_rows) { return (n_ranges + ws_slab_ranges(n_rows) - 1) / ws_slab_ranges(n_rows); }

// ---- host only: the carrier of a key
inline unsigned long long wm_splitmix64(unsigned long long* state) {
    unsigned long long z = (*state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

inline bool wm_key_ok(unsigned long long key) { return key >= 1 && key <= kWmKeyMax; }

// sub-key d of a key (wave_codec.watermark_subkey): output number P / 64 + 1 + d of the generator whose first P / 64 outputs are the chips
inline unsigned long long wm_subkey(unsigned long long key, int d) {
    unsigned long long state = key, z = 0;
    for (int k = 0; k < kWmPeriod / 64 + 1 + d; k++) z = wm_splitmix64(&state);
    return 1 + z % kWmKeyMax;
}

// chips [kWmPeriod] (+1 / -1 as signed bytes) and carrier [kWmPeriod] of `key` from the taps g [kWmTaps]
inline void wm_carrier(unsigned long long key, const int* g, signed char* chips, short* carrier) {
    unsigned long long state = key;
    for (int k = 0; k < kWmPeriod / 64; k++) {
        const unsigned long long z = wm_splitmix64(&state);
        for (int i = 0; i < 64; i++) chips[64 * k + i] = ((z >> i) & 1) ? 1 : -1;
    }
    for (int m = 0; m < kWmPeriod; m++) {
        int acc = 0;
        for (int k = 0; k < kWmTaps; k++) acc += g[k] * chips[(m - k + kWmTaps / 2 + kWmPeriod) & (kWmPeriod - 1)];
        carrier[m] = (short)(acc >> kWmCarrierShift);   // (arithmetic: floor)
    }
}
