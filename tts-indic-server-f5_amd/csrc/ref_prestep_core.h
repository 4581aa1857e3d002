// The reference-clip pre-step, the part with no HIP in it: the geometry, the integer comparisons and the sequential rule of the device call
// (ref_prestep.h, f5hip_ref_prestep) as inline functions that a plain host compiler takes too.  tools/ref_prestep_check.cpp runs them
// serially under AddressSanitizer and UBSan over tables of exactly their size; that CPU run is the evidence for the bounds below.  The
// definition of every rule here is audio_prep.preprocess_ref_segment, restated as index arithmetic by audio_prep.preprocess_ref_ranges:
// this file is that function line for line.
//
//   clip at a pause   silent windows (S < (T + 1)^2 n on exact integer sums) -> silent ranges -> non-silent ranges -> chunks padded by
//                     1000 ms, overlaps split at the midpoint -> the "more than 6 s so far and more than 15 s with this chunk" stop;
//                     (1000 ms, -50 dBFS) first, (100 ms, -40 dBFS) if that leaves more than 15 s, then a hard cut at 15 000 ms
//   edges             on the clipped CONCATENATION, whose millisecond grid starts at its own frame 0: leading silence in 10 ms windows
//                     (rms < 261), then on the trimmed rest, whose grid restarts once more, the last millisecond with rms >= 261 and the
//                     reference's running `end -= 0.001`
// fp64 appears in three places, each a single IEEE operation as on the host: the frame of a millisecond (ms * (rate / 1000.0), truncated),
// a length in milliseconds (1000.0 * frames / rate: one exact product, one division, round half to even) and the running subtraction.
//
// Bounds, in one place:
//   P       rp_window_silent and rp_src_sum read P[0 .. L]: L + 1 entries (L = rp_len_ms(N)); every index is clamped to [0, L] first
//   flags   rp_clip_pass reads flags[0 .. rp_nwin(L, msl))
//   frames  Part::operator()(a, b) is called with 0 <= a <= b <= N only (rp_frame clamps to N, ranges are built from rp_frame values)
//   ranges  RpRanges holds kRpMaxRanges; a range is added only where the chunk before it ended more than 2000 ms of source earlier (else the
//           two merge), and none is added once the kept length is over 15 000 ms: fewer than 16.  rp_add refuses to write past the array
//           (overflow is reported, never written).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RP_HD __host__ __device__ inline
#else
#define RP_HD inline
#endif

constexpr int kRpSeekMs = 10, kRpKeepMs = 1000, kRpMinMs = 6000, kRpMaxMs = 15000, kRpTailMs = 50, kRpMinRate = 11025;
constexpr int kRpPass1Ms = 1000, kRpPass2Ms = 100;                                  // min_silence_len of the two parameter sets
constexpr long long kRpPass1Square = 104LL * 104, kRpPass2Square = 328LL * 328;     // -50 dBFS: rms <= 103.6; -40 dBFS: rms <= 327.68 (audio_prep.silence_square)
constexpr long long kRpEdgeSquare = 261LL * 261;                    // -42 dBFS: 20 log10(260 / 32768) < -42 < 20 log10(261 / 32768) (audio_prep.edge_rms_thresholds)
constexpr int kRpMaxRanges = 16;
constexpr long long kRpMaxWindowSamples = 1LL << 23;                // rate x channels below this: the window sums stay below 2^53

struct RpGeom {
    long long N;        // frames
    long long L;        // len(seg) in milliseconds
    double k;           // rate / 1000.0, formed once
    int rate, C;
};

struct RpRanges {
    long long a[kRpMaxRanges], b[kRpMaxRanges];   // source frames [a, b), in output order
    long long frames;                             // their sum
    int nr, overflow;
};

RP_HD int rp_pass_ms(int p) { return p == 0 ? kRpPass1Ms : kRpPass2Ms; }
RP_HD long long rp_pass_square(int p) { return p == 0 ? kRpPass1Square : kRpPass2Square; }

RP_HD long long rp_len_ms(long long frames, int rate) { return (long long)rint(1000.0 * (double)frames / (double)rate); }

RP_HD RpGeom rp_geom(long long frames, int channels, int rate) {
    RpGeom g;
    g.N = frames; g.C = channels; g.rate = rate; g.k = (double)rate / 1000.0; g.L = rp_len_ms(frames, rate);
    return g;
}

// PcmSegment._frame of a segment of n frames and n_ms milliseconds
RP_HD long long rp_frame_of(double k, long long n, long long n_ms, long long ms) {
    ms = ms < 0 ? 0 : (ms > n_ms ? n_ms : ms);
    const long long f = (long long)((double)ms * k);
    return f < 0 ? 0 : (f > n ? n : f);
}
RP_HD long long rp_frame(const RpGeom& g, long long ms) { return rp_frame_of(g.k, g.N, g.L, ms); }

RP_HD long long rp_tail_frames(int rate) { return (long long)((double)(rate * kRpTailMs) / 1000.0); }

// ---------------------------------------------------------------- windows of detect_silence(seek_step 10)
RP_HD long long rp_nwin(long long L, int msl) {
    if (L < msl) return 0;
    const long long last = L - msl;
    return last / kRpSeekMs + 1 + (last % kRpSeekMs ? 1 : 0);
}
RP_HD long long rp_window_start(long long L, int msl, long long w) {
    const long long last = L - msl;
    return w <= last / kRpSeekMs ? kRpSeekMs * w : last;
}
// P[m] = the sum of squares of all samples of frames [0, rp_frame(m)), m = 0 .. L
RP_HD bool rp_window_silent(const RpGeom& g, const long long* P, long long s, int msl, long long square) {
    const long long n = (rp_frame(g, s + msl) - rp_frame(g, s)) * g.C;
    return n <= 0 || P[s + msl] - P[s] < square * n;
}

// ---------------------------------------------------------------- one _clip_at_pause pass, O(1) state
RP_HD void rp_add(RpRanges& r, long long fa, long long fb) {
    if (fb <= fa) return;
    if (r.nr > 0 && r.b[r.nr - 1] == fa) {
        r.b[r.nr - 1] = fb;
    } else if (r.nr < kRpMaxRanges) {
        r.a[r.nr] = fa; r.b[r.nr] = fb; r.nr++;
    } else {
        r.overflow = 1;
        return;
    }
    r.frames += fb - fa;
}

struct RpWalk {
    RpGeom g;
    int msl;
    bool have_prev, any_silent, first, pend, stopped;
    long long prev, cur, prev_end, last_end, ps, pe;
    RpRanges out;
};

RP_HD void rp_walk_init(RpWalk& w, const RpGeom& g, int msl) {
    w.g = g; w.msl = msl;
    w.have_prev = w.any_silent = w.pend = w.stopped = false;
    w.first = true;
    w.prev = w.cur = w.prev_end = w.last_end = w.ps = w.pe = 0;
    w.out.nr = 0; w.out.overflow = 0; w.out.frames = 0;
}

RP_HD void rp_chunk(RpWalk& w, long long a_ms, long long b_ms) {     // `out + chunk` unless the stop has fired
    if (w.stopped) return;
    const long long fa = rp_frame(w.g, a_ms), fb = rp_frame(w.g, b_ms);
    const long long n = fb > fa ? fb - fa : 0;
    if (rp_len_ms(w.out.frames, w.g.rate) > kRpMinMs && rp_len_ms(w.out.frames + n, w.g.rate) > kRpMaxMs) {
        w.stopped = true;
        return;
    }
    rp_add(w.out, fa, fb);
}

RP_HD void rp_nonsilent(RpWalk& w, long long p, long long s, bool droppable) {   // split_on_silence: pad, split overlaps at the midpoint
    const bool head = w.first && droppable && p == 0 && s == 0;    // detect_nonsilent drops a leading [0, 0]
    w.first = false;
    if (head) return;
    long long ns = p - kRpKeepMs;
    const long long ne = s + kRpKeepMs;
    if (w.pend) {
        if (ns < w.pe) {
            w.pe = (w.pe + ns) >> 1;                               // (pe + ns = an end plus a later start: never negative)
            ns = w.pe;
        }
        rp_chunk(w, w.ps > 0 ? w.ps : 0, w.pe < w.g.L ? w.pe : w.g.L);
    }
    w.ps = ns; w.pe = ne; w.pend = true;
}

RP_HD void rp_silent_range(RpWalk& w, long long s, long long e) {
    w.any_silent = true;
    rp_nonsilent(w, w.prev_end, s, true);
    w.prev_end = w.last_end = e;
}

RP_HD void rp_silent_start(RpWalk& w, long long s) {                // detect_silence: a start neither 10 ms nor at most msl behind the last opens a range
    if (!w.have_prev) {
        w.cur = s;
    } else if (s != w.prev + kRpSeekMs && s > w.prev + w.msl) {
        rp_silent_range(w, w.cur, w.prev + w.msl);
        w.cur = s;
    }
    w.prev = s; w.have_prev = true;
}

RP_HD void rp_walk_finish(RpWalk& w) {
    if (w.have_prev) rp_silent_range(w, w.cur, w.prev + w.msl);
    if (!w.any_silent) rp_nonsilent(w, 0, w.g.L, false);
    else if (w.last_end != w.g.L) rp_nonsilent(w, w.prev_end, w.g.L, true);
    if (w.pend) rp_chunk(w, w.ps > 0 ? w.ps : 0, w.pe < w.g.L ? w.pe : w.g.L);
}

// flags[w] != 0: window w of the pass is silent
RP_HD void rp_clip_pass(const RpGeom& g, const uint8_t* flags, int msl, RpRanges& out) {
    RpWalk w;
    rp_walk_init(w, g, msl);
    const long long nwin = rp_nwin(g.L, msl);
    for (long long i = 0; i < nwin && !w.stopped; i++)
        if (flags[i]) rp_silent_start(w, rp_window_start(g.L, msl, i));
    if (!w.stopped) rp_walk_finish(w);
    out = w.out;
}

RP_HD void rp_truncate(RpRanges& r, long long frames) {             // the first `frames` frames of the concatenation
    long long left = frames;
    int nr = 0;
    for (int i = 0; i < r.nr && left > 0; i++) {
        if (r.b[i] - r.a[i] > left) r.b[i] = r.a[i] + left;
        left -= r.b[i] - r.a[i];
        nr = i + 1;
    }
    r.nr = nr;
    r.frames = frames - left;
}

// the clipped concatenation: both passes in turn, then the hard cut (flags of pass p at flags[p])
RP_HD void rp_clip(const RpGeom& g, const uint8_t* const flags[2], bool clip_short, RpRanges& out) {
    out.nr = 0; out.overflow = 0; out.frames = 0;
    if (!clip_short) {
        rp_add(out, 0, g.N);
        return;
    }
    for (int p = 0; p < 2; p++) {
        rp_clip_pass(g, flags[p], rp_pass_ms(p), out);
        if (rp_len_ms(out.frames, g.rate) <= kRpMaxMs) break;
    }
    if (rp_len_ms(out.frames, g.rate) > kRpMaxMs) {                 // slice_ms(0, 15000) of the concatenation
        const long long cut = (long long)((double)kRpMaxMs * g.k);
        if (cut < out.frames) rp_truncate(out, cut);
    }
}

// ---------------------------------------------------------------- sums over source frames and over the concatenation
// Sum of squares of the samples of source frames [a, b): whole millisecond cells from P, the partial cells at either end from the samples
// (part(a, b): the exact sum over frames [a, b), 0 <= a <= b <= N).
template <typename Part>
RP_HD long long rp_src_sum(const RpGeom& g, const long long* P, const Part& part, long long a, long long b) {
    if (b <= a) return 0;
    long long ma = a * 1000 / g.rate, mb = b * 1000 / g.rate;      // guesses; the loops settle them on the exact grid
    ma = ma > g.L ? g.L : ma; mb = mb > g.L ? g.L : mb;
    while (ma < g.L && rp_frame(g, ma) < a) ma++;                  // the first millisecond at or after a
    while (ma > 0 && rp_frame(g, ma - 1) >= a) ma--;
    while (mb > 0 && rp_frame(g, mb) > b) mb--;                    // the last millisecond at or before b
    while (mb < g.L && rp_frame(g, mb + 1) <= b) mb++;
    const long long fa = rp_frame(g, ma), fb = rp_frame(g, mb);
    if (ma > mb || fa < a || fb > b || fa > fb) return part(a, b);
    return part(a, fa) + (P[mb] - P[ma]) + part(fb, b);
}

// frames [x, y) of the concatenation of r
template <typename Part>
RP_HD long long rp_concat_sum(const RpGeom& g, const long long* P, const Part& part, const RpRanges& r, long long x, long long y) {
    long long s = 0, at = 0;
    for (int i = 0; i < r.nr; i++) {
        const long long len = r.b[i] - r.a[i];
        const long long lo = x > at ? x : at, hi = y < at + len ? y : at + len;
        if (lo < hi) s += rp_src_sum(g, P, part, r.a[i] + (lo - at), r.a[i] + (hi - at));
        at += len;
    }
    return s;
}

// ---------------------------------------------------------------- remove_silence_edges
struct RpEdges {
    long long total, L1;      // the concatenation: frames, milliseconds
    long long x0, n2, L2;     // after the leading trim: its first frame in the concatenation, frames, milliseconds
};

RP_HD long long rp_lead_windows(const RpRanges& r, int rate) { return (rp_len_ms(r.frames, rate) + kRpSeekMs - 1) / kRpSeekMs; }

// detect_leading_silence's window i (10 i ms of the concatenation): not below -42 dBFS
template <typename Part>
RP_HD bool rp_lead_loud(const RpGeom& g, const long long* P, const Part& part, const RpRanges& r, long long i) {
    const long long L1 = rp_len_ms(r.frames, g.rate);
    const long long x = rp_frame_of(g.k, r.frames, L1, kRpSeekMs * i), y = rp_frame_of(g.k, r.frames, L1, kRpSeekMs * i + kRpSeekMs);
    const long long n = (y - x) * g.C;
    return n > 0 && rp_concat_sum(g, P, part, r, x, y) >= kRpEdgeSquare * n;
}

// lead_window: the first loud window, or -1
RP_HD RpEdges rp_edges(const RpGeom& g, const RpRanges& r, long long lead_window) {
    RpEdges e;
    e.total = r.frames; e.L1 = rp_len_ms(r.frames, g.rate);
    const long long lead = lead_window >= 0 ? kRpSeekMs * lead_window : e.L1;
    e.x0 = rp_frame_of(g.k, e.total, e.L1, lead);
    e.n2 = rp_frame_of(g.k, e.total, e.L1, e.L1) - e.x0;           // slice_ms(lead, L1 + 1)
    e.L2 = rp_len_ms(e.n2, g.rate);
    return e;
}

// millisecond m of the trimmed rest: above -42 dBFS
template <typename Part>
RP_HD bool rp_trail_loud(const RpGeom& g, const long long* P, const Part& part, const RpRanges& r, const RpEdges& e, long long m) {
    const long long x = e.x0 + rp_frame_of(g.k, e.n2, e.L2, m), y = e.x0 + rp_frame_of(g.k, e.n2, e.L2, m + 1);
    const long long n = (y - x) * g.C;
    return n > 0 && rp_concat_sum(g, P, part, r, x, y) >= kRpEdgeSquare * n;
}

// last_loud: the last loud millisecond, or -1.  Leaves in r the source ranges of the result and returns its frames (without the tail).
RP_HD long long rp_finish(const RpGeom& g, RpRanges& r, const RpEdges& e, long long last_loud) {
    double end = (double)e.n2 / (double)g.rate;                    // duration_seconds
    const long long quiet_tail = last_loud >= 0 ? e.L2 - 1 - last_loud : e.L2;
    for (long long i = 0; i < quiet_tail; i++) end -= 0.001;       // the reference's running subtraction, rounding included
    const long long x1 = e.x0 + rp_frame_of(g.k, e.n2, e.L2, (long long)(end * 1000.0));
    long long at = 0, frames = 0;
    int nr = 0;
    for (int i = 0; i < r.nr; i++) {                               // concatenation frames [x0, x1) back to source frames
        const long long len = r.b[i] - r.a[i];
        const long long lo = e.x0 > at ? e.x0 : at, hi = x1 < at + len ? x1 : at + len;
        const long long a = r.a[i];
        if (lo < hi) { r.a[nr] = a + (lo - at); r.b[nr] = a + (hi - at); frames += hi - lo; nr++; }
        at += len;
    }
    r.nr = nr; r.frames = frames;
    return frames;
}
