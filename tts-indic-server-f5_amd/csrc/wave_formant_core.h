// The formant-preserving pitch shift (TD-PSOLA) of finished PCM, the part with no HIP in it: the geometry, the lag rule, the tie rules, the
// mark chain's steps and the blend of the three launches of wave_formant.h (f5hip_wave_prosody_formants) as inline functions that a plain
// host compiler takes too.  tools/wave_formant_check.cpp runs them serially under AddressSanitizer and UBSan over tables of exactly their
// size; that CPU run is the evidence for the bounds below.  The definition is wave_codec.psola_pcm16 (written down above
// wave_codec.psola_window):
//   track      frame f at t = 120 f, F = ceil(n / 120): d[l] = sum_{i < 480} |xt[t + i] - xt[t + l + i]|, l = 48 .. 400, E = sum |xt[t + i]|;
//              the lag = the smallest l with 8 d[l] <= 8 dmin + E, then upwards while d decreases; voiced iff E >= 64 * 480 and 2 d[lag] <= E
//   marks      from t = 0 while t < n, frame t / 120: unvoiced (a = t, T = 120); voiced, T = the lag: a = the largest sample's position in
//              [t, t + T) at the start of a voiced run, else in [max(t - T / 8, a_prev + 24), t + T / 8], inside the wave, ties to the
//              earlier one; t = a + T
//   synthesis  u_0 = a_0; u takes the nearest mark i (ties to the earlier); voiced: u += (T_i q + rem) / p with the remainder carried,
//              unvoiced: u += 120; while u < n
//   output     y[j] = clip(round-half-up(num / den)) over the grains with |j - u| <= T_i, weight M[(|j - u| 1024) / T_i], source
//              xt[a_i + j - u]; y[j] = x[j] where den == 0
//
// Bounds, in one place:
//   x        fp_source / fp_sample_at read x[j] only for 0 <= j < n: every other index is the zero of xt, an index predicate and never a read
//   tile     a tile of kFpTileFrames frames from frame f0 reads xt[120 f0 .. 120 f0 + kFpSpan): its last frame's last lag ends at
//            120 (kFpTileFrames - 1) + 400 + 480 = kFpSpan
//   sums     d, E <= 480 * 65535 < 2^25; 8 d + E < 2^29: unsigned 32-bit
//   marks    every analysis mark lies in [0, n) and at least kFpMinAdvance after the one before: at most fp_max_marks(n) = ceil(n / 24);
//            every synthesis step is at least kFpMinStep = 48 * 29 / 41 = 33: at most fp_max_synth(n) = ceil(n / 33) synthesis marks
//   grains   a sample j is touched only by marks with |u - j| <= 400: the marks of a tile of kFpOutTile outputs lie in a closed range of
//            kFpOutTile + 800 positions, at most kFpTileGrains of them
//   blend    |num| <= grains * 2^15 * 2^15, den <= grains * 2^15: 64-bit; M[1021] >= 1 and (|k| 1024) / T <= 1021 for |k| < T <= 400
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FP_HD __host__ __device__ inline
#else
#define FP_HD inline
#endif

constexpr int kFpHop = 120, kFpWin = 480, kFpLagMin = 48, kFpLagMax = 400;   // wave_codec.PSOLA_HOP, PSOLA_WINDOW, PSOLA_LAG_MIN, PSOLA_LAG_MAX
constexpr int kFpLags = kFpLagMax - kFpLagMin + 1;                          // 353
constexpr int kFpMinAdvance = 24;                                           // wave_codec.PSOLA_MIN_ADVANCE
constexpr int kFpTable = 1024;                                              // wave_codec.PSOLA_TABLE: the master window has kFpTable + 1 entries
constexpr int kFpMinStep = 33;                                              // floor(48 * 29 / 41): the shortest synthesis step
constexpr int kFpPeakMax = kFpLagMax;                                       // samples of the longest peak search (the start of a voiced run)
constexpr int kFpTileFrames = 5;                                            // frames of one period tile: 5 * 354 sums = 6.9 rounds of 256 threads
constexpr int kFpSpan = kFpHop * (kFpTileFrames - 1) + kFpLagMax + kFpWin;  // 1360 samples hold every sum of a tile
constexpr int kFpOutTile = 2048;                                            // outputs of one overlap-add tile
constexpr int kFpTileGrains = (kFpOutTile + 2 * kFpLagMax - 1) / kFpMinStep + 1;   // 87
static_assert(kFpLagMin * 29 / 41 == kFpMinStep && kFpMinAdvance * 2 <= kFpLagMin && kFpSpan % 2 == 0 && kFpHop % 8 == 0 && kFpWin % 8 == 0, "wave_formant geometry");
static_assert(480LL * 65535 * 9 < (1LL << 32), "wave_formant: 8 d + E in 32 bits");

struct FpMark  { int a; int T; };      // an analysis mark: its position; its period, bit 16 set when voiced
struct FpSynth { int u; int i; };      // a synthesis mark: its position; the analysis mark it takes
struct FpGrain { int u; int a; int T; };

FP_HD long long fp_frames(long long n) { return (n + kFpHop - 1) / kFpHop; }
FP_HD long long fp_period_tiles(long long n) { return (fp_frames(n) + kFpTileFrames - 1) / kFpTileFrames; }
FP_HD long long fp_max_marks(long long n) { return (n + kFpMinAdvance - 1) / kFpMinAdvance; }
FP_HD long long fp_max_synth(long long n) { return (n + kFpMinStep - 1) / kFpMinStep; }
FP_HD long long fp_out_tiles(long long n) { return (n + kFpOutTile - 1) / kFpOutTile; }

// xt[j] biased by 32768 (absolute differences are those of the samples; the zero outside the wave is 0x8000), and unbiased
FP_HD unsigned fp_source(const short* x, long long n, long long j) { return (j >= 0 && j < n ? (unsigned)(unsigned short)x[j] : 0u) ^ 0x8000u; }
FP_HD int fp_sample_at(const short* x, long long n, long long j) { return j >= 0 && j < n ? (int)x[j] : 0; }

// the lag rule: whether a lag's d is within E / 8 of the best; the walk to the bottom of its dip (li = lag - 48 over d[0 .. 353))
FP_HD bool fp_lag_ok(unsigned d, unsigned dmin, unsigned E) { return 8u * d <= 8u * dmin + E; }
FP_HD int fp_lag_walk(const unsigned* d, int li) {
    while (li + 1 < kFpLags && d[li + 1] < d[li]) li++;
    return li;
}
FP_HD bool fp_voiced(unsigned d, unsigned E) { return E >= 64u * kFpWin && 2u * d <= E; }
FP_HD int fp_track_entry(int lag, bool voiced) { return lag | (voiced ? 1 << 16 : 0); }
FP_HD int fp_entry_lag(int e) { return e & 0xffff; }
FP_HD bool fp_entry_voiced(int e) { return (e >> 16) & 1; }

// a frame's lag and flag from its 353 sums and E, serially (the kernel finds dmin and the first lag by two reductions and walks the same way)
FP_HD int fp_frame_entry(const unsigned* d, unsigned E) {
    unsigned dmin = d[0];
    for (int li = 1; li < kFpLags; li++) dmin = d[li] < dmin ? d[li] : dmin;
    int li = 0;
    while (!fp_lag_ok(d[li], dmin, E)) li++;                            // (the best lag itself passes: li stops inside the table)
    li = fp_lag_walk(d, li);
    return fp_track_entry(li + kFpLagMin, fp_voiced(d[li], E));
}

// the samples [b, e) a voiced mark is searched in, predicted at t with period T; chained: the mark before was voiced, at a_prev.  Inside
// the wave and never empty for t < n: b <= t < e
FP_HD void fp_peak_range(long long t, int T, bool chained, long long a_prev, long long n, long long* b, long long* e) {
    long long lo = t, hi = t + T;
    if (chained) {
        lo = t - T / 8;
        if (lo < a_prev + kFpMinAdvance) lo = a_prev + kFpMinAdvance;
        hi = t + T / 8 + 1;
    }
    *b = lo;
    *e = hi < n ? hi : n;
}
// the keyed maximum of the peak search: the larger sample, then the earlier position (positions below 2^31)
FP_HD unsigned long long fp_peak_key(int sample, long long pos) { return ((unsigned long long)(unsigned)(sample + 32768) << 32) | (0xffffffffu - (unsigned)pos); }
FP_HD long long fp_peak_pos(unsigned long long key) { return (long long)(0xffffffffu - (unsigned)(key & 0xffffffffu)); }

// whether mark a_next is strictly nearer to u than a_cur (ties stay with the earlier one)
FP_HD bool fp_nearer(long long a_next, long long a_cur, long long u) {
    const long long dn = a_next > u ? a_next - u : u - a_next, dc = a_cur > u ? a_cur - u : u - a_cur;
    return dn < dc;
}
// the step after a synthesis mark that took (T, voiced): the remainder is carried over voiced marks and stays over unvoiced ones
FP_HD int fp_synth_step(int T, bool voiced, int p, int q, int* rem) {
    if (!voiced) return T;
    const int v = T * q + *rem;
    *rem = v % p;
    return v / p;
}

// the chain's state while analysis marks arrive: synthesis marks are final as soon as the mark after their candidate is known
struct FpChain {
    long long u; int rem; int cur; int cur_a; int cur_T; int ns;
};
// hands out the synthesis marks that stay with the candidate now that mark k = (a, T) has arrived (or, with last = true, all that remain),
// then makes k the candidate.  emit(u, i) is called in order.
template <typename Emit>
FP_HD void fp_chain_advance(FpChain& c, int k, int a, int T, bool last, long long n, int p, int q, Emit emit) {
    if (c.cur < 0) {                                                    // the first mark: u_0 = a_0
        if (last) return;
        c.u = a; c.rem = 0; c.cur = k; c.cur_a = a; c.cur_T = T; c.ns = 0;
        return;
    }
    while (c.u < n && (last || !fp_nearer(a, c.cur_a, c.u))) {
        emit(c.u, c.cur);
        c.ns++;
        c.u += fp_synth_step(c.cur_T & 0xffff, (c.cur_T >> 16) & 1, p, q, &c.rem);
    }
    if (!last) { c.cur = k; c.cur_a = a; c.cur_T = T; }
}

// the first of the ns synthesis marks (ascending) at or after position v; ns when there is none
FP_HD int fp_first_at_or_after(const FpSynth* s, int ns, long long v) {
    int lo = 0, hi = ns;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[mid].u < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the marks [*m0, *m0 + count) that may touch the outputs [j0, j1): those with j0 - 400 <= u <= j1 - 1 + 400
FP_HD int fp_tile_marks(const FpSynth* s, int ns, long long j0, long long j1, int* m0) {
    *m0 = fp_first_at_or_after(s, ns, j0 - kFpLagMax);
    const int count = fp_first_at_or_after(s, ns, j1 + kFpLagMax) - *m0;
    return count < kFpTileGrains ? count : kFpTileGrains;               // (the bound above: never more)
}

// one output sample from the grains g[0 .. ng) that may touch it (any order: integer sums), M the master window
FP_HD int fp_output(const short* x, long long n, long long j, const FpGrain* g, int ng, const unsigned short* M) {
    long long num = 0, den = 0;
    for (int m = 0; m < ng; m++) {
        const int T = g[m].T;
        const long long k = j - g[m].u;
        const long long ak = k < 0 ? -k : k;
        if (ak > T) continue;
        const long long w = M[(ak * kFpTable) / T];
        num += w * fp_sample_at(x, n, g[m].a + k);
        den += w;
    }
    if (den == 0) return fp_sample_at(x, n, j);
    const long long a = 2 * num + den, b = 2 * den;
    long long v = a / b;
    if (a % b < 0) v--;                                                 // a floor division
    return (int)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
}
