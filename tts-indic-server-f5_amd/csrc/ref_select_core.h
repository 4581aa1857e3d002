// The reference-stretch selection, the part with no HIP in it: the constants, the window geometry, the radix digits and the digit pick of the
// sliding order statistic, the source buckets of the clipping count, the row arithmetic, the key order and the checked recording table of the
// device call (ref_select.h, f5hip_ref_select) as inline functions that a plain host compiler takes too.  tools/ref_select_check.cpp runs them
// serially under AddressSanitizer and UBSan over tables of exactly their size; that CPU run is the evidence for the bounds below.  The
// definition is audio_prep.select_reference (written down above it); the framing is the denoiser's (ref_denoise_core.h), the band, the floor's
// rank and the clipping run rule are the report's (ref_assess_core.h).
//
// Bounds, in one place:
//   frames   recording c has F = rd_frames(len) frames; its band power is bin-major: bin b (k = 3 + b) owns Pb[col0 + b Fs, + Fs), Fs = F
//            rounded up to 4 (the pad cells hold zeros and lie in no window), col0 a multiple of 4: every column starts on 16 bytes
//   windows  F >= W: nwin = (F - W) / hop + 1 windows of Wc = W frames, window w = frames [hop w, hop w + W), the last one ending at or
//            before F.  F < W: ONE window of Wc = F frames.  rank (Wc - 1) / 5 < Wc
//   runs     a workgroup owns windows [run r, min(nwin, run (r + 1))) of one bin and stages frames [fa, fb) = rs_stage_range, at most
//            hop (run - 1) + W <= kRsStageCap values (rs_run), read as 16-byte cells from fa & ~3 up to fb rounded up to 4 <= Fs: at most
//            kRsStageCap + 6 values of the kRsStageCap + 8 the kernel holds
//   buckets  prepared samples [256 m, 256 (m + 1)) & [0, len) <-> raw samples [g(m), g(m + 1)), g(m) = floor(min(256 m, len) sr / 24000);
//            nb = ceil(len / 256) buckets and nb + 1 prefix cells; raw sample j lies in bucket rs_bucket(j) < nb, or past g(nb) in none.
//            Window w counts cells rs_cell(f0 - 3) .. rs_cell(f0 + Wc), both clamped to [0, nb]
//   table    rs_layout refuses what the call refuses, so a table it accepts has 1 .. kRsMaxRecs recordings of 1 .. kRsMaxSamples samples,
//            at most kRsMaxCallSamples in all, 1 <= W <= kRsMaxWindow, 1 <= hop <= kRsMaxHop, sample rates 1 .. kRsMaxRate and every count
//            below 2^31
#pragma once
#include "ref_assess_core.h"

#define RS_HD RD_HD

constexpr int kRsMaxSamples = 14400000;                             // audio_prep.SELECT_MAX_SAMPLES: 600 s at 24 kHz
constexpr long long kRsMaxCallSamples = 4LL * kRsMaxSamples;        // prepared samples of ONE call: the workspace is about 29 bytes a sample (1.7 GB at the cap)
constexpr int kRsHop = 48;                                          // SELECT_HOP, the default of the call
constexpr int kRsMaxWindow = 1407;                                  // floor(15.01 * 93.75): frames of the longest window
constexpr int kRsMaxHop = 1 << 20, kRsMaxRate = 768000, kRsMaxRecs = 64;
constexpr int kRsBand = kRaBand1 - kRaBand0 + 1;                    // 339 bins
constexpr int kRsFloorStride = 340;                                 // floats per window of the floor table: 339, padded to 16 bytes
constexpr int kRsStageCap = 4096;                                   // frames of one bin a workgroup of the floor launch holds in LDS
constexpr int kRsRun = 16;                                          // windows per workgroup where they fit (rs_run)
constexpr int kRsRowWords = 5;                                      // 64-bit words per window of the output
enum { RS_CLIPPED = 0, RS_SPEECH, RS_N, RS_S, RS_SNR_DB };
constexpr int kRsTile = 32;                                         // frame rows per block of the band launch

struct RsRec {
    long long col0;     // its first float of the bin-major band power
    int len;            // prepared samples
    int sr;             // the raw side's sample rate
    int F, Fs;          // frames; floats per bin column
    int Wc, nwin;       // frames per window; windows
    int win0;           // its first row of the window tables (ascending over the table)
    int run0, nruns;    // its first workgroup column of the floor launch (ascending), and how many
    int tile0;          // its first tile of the band launch (ascending)
    int nb, cell0;      // source buckets; its first of nb + 1 prefix cells
    int row0;           // its first frame row of P and E
    int pad_;
};

RS_HD int rs_padded(int F) { return (F + 3) & ~3; }
RS_HD int rs_window_frames(int F, int W) { return F < W ? F : W; }
RS_HD int rs_windows(int F, int W, int hop) { return F < W ? 1 : (F - W) / hop + 1; }
RS_HD int rs_rank(int Wc) { return rd_rank(Wc); }
// windows per workgroup of the floor launch: kRsRun, or as many as keep hop (run - 1) + W values inside the stage
RS_HD int rs_run(int W, int hop) {
    const int fit = (kRsStageCap - W) / hop + 1;
    return fit < kRsRun ? fit : kRsRun;
}
// the frames [*fa, *fb) a workgroup stages for windows [w0, w1) of a recording
RS_HD void rs_stage_range(const RsRec& c, int hop, int w0, int w1, int* fa, int* fb) {
    *fa = hop * w0;
    *fb = hop * (w1 - 1) + c.Wc;
}
// digit `pass` (0: the top) of the bit pattern of a non-negative float: four 8-bit digits, whose order is the values' order
RS_HD int rs_digit(unsigned bits, int pass) { return (int)((bits >> (24 - 8 * pass)) & 255u); }
// the bits above digit `pass`
RS_HD unsigned rs_above(unsigned bits, int pass) { return pass == 0 ? 0u : bits >> (32 - 8 * pass); }
// the digit that holds rank r of a histogram of 256 counts (r below their sum), and r's rank inside it
RS_HD int rs_pick(const int* hist, int r, int* rest) {
    int d = 0;
    while (d < 255 && r >= hist[d]) r -= hist[d++];
    *rest = r;
    return d;
}
// the frames that leave and enter between one window and the next: `r` frames from the old start, `r` up to the new end
RS_HD int rs_slide(int Wc, int hop) { return hop < Wc ? hop : Wc; }

RS_HD int rs_buckets(int len) { return (len + kRdHop - 1) / kRdHop; }
// g(m): the first raw sample of bucket m (m = nb: the end of the last)
RS_HD long long rs_bucket_start(const RsRec& c, int m) {
    const long long s = (long long)m * kRdHop < c.len ? (long long)m * kRdHop : c.len;
    return s * c.sr / 24000;
}
// the bucket of raw sample j, or -1 past the last one's end
RS_HD int rs_bucket(const RsRec& c, long long j) {
    if (j >= rs_bucket_start(c, c.nb)) return -1;
    return (int)(((j + 1) * 24000 - 1) / ((long long)kRdHop * c.sr));
}
// the prefix cell of boundary m, which is g(clamp(m, 0, nb))
RS_HD int rs_cell(const RsRec& c, int m) { return m < 0 ? 0 : (m > c.nb ? c.nb : m); }
// the window's source range in raw samples
RS_HD void rs_source_range(const RsRec& c, int f0, long long* start, long long* end) {
    *start = rs_bucket_start(c, rs_cell(c, f0 - kRdPad / kRdHop));
    *end = rs_bucket_start(c, rs_cell(c, f0 + c.Wc));
}

RS_HD double rs_inf() { return HUGE_VAL; }
RS_HD double rs_snr_db(double N, double S) { return !(N > 0.0) ? rs_inf() : (S > N ? 10.0 * log10((S - N) / N) : -rs_inf()); }
// the key (clipped, -snr_db, w) of window a sorts before window b's
RS_HD bool rs_key_less(long long ca, double sa, int wa, long long cb, double sb, int wb) {
    if (ca != cb) return ca < cb;
    if (sa != sb) return sa > sb;
    return wa < wb;
}

// ---- host only
enum { RS_OK = 0, RS_RECS, RS_NULL, RS_WINDOW, RS_HOP, RS_RATE, RS_LENGTH, RS_OFFSET, RS_OVERLAP, RS_TOTAL };

struct RsPlan {
    long long rows = 0, cols = 0;      // frame rows; floats of the bin-major band power
    int windows = 0, runs = 0, tiles = 0, cells = 0, run = 1;
};

// The recording table of a call, checked: RS_OK and h, clips (the STFT's table of the same recordings) and plan filled, or the reason for the
// refusal and the recording it is about.  The raw side is ra_layout's.
inline int rs_layout(int32_t n, const int32_t* sample_rate, const int64_t* offset, const int32_t* n_samples, int W, int hop, std::vector<RsRec>& h,
                     std::vector<RdClip>& clips, RsPlan* plan, int* bad) {
    *bad = 0;
    if (n < 1 || n > kRsMaxRecs) return RS_RECS;
    if (!sample_rate || !offset || !n_samples) return RS_NULL;
    if (W < 1 || W > kRsMaxWindow) return RS_WINDOW;
    if (hop < 1 || hop > kRsMaxHop) return RS_HOP;
    h.assign((size_t)n, RsRec());
    clips.assign((size_t)n, RdClip());
    RsPlan p;
    p.run = rs_run(W, hop);
    long long samples = 0;
    for (int i = 0; i < n; i++) {
        *bad = i;
        if (sample_rate[i] < 1 || sample_rate[i] > kRsMaxRate) return RS_RATE;
        if (n_samples[i] < 1 || n_samples[i] > kRsMaxSamples) return RS_LENGTH;
        if (offset[i] < 0 || offset[i] > INT64_MAX - kRsMaxSamples) return RS_OFFSET;
        RsRec& c = h[(size_t)i];
        RdClip& d = clips[(size_t)i];
        d.off = offset[i]; d.out0 = samples; d.n = n_samples[i]; d.F = rd_frames(d.n); d.row0 = (int)p.rows; d.pad_ = 0;
        c.col0 = p.cols; c.len = d.n; c.sr = sample_rate[i]; c.F = d.F; c.Fs = rs_padded(c.F);
        c.Wc = rs_window_frames(c.F, W); c.nwin = rs_windows(c.F, W, hop);
        c.win0 = p.windows; c.run0 = p.runs; c.nruns = (c.nwin + p.run - 1) / p.run; c.tile0 = p.tiles;
        c.nb = rs_buckets(c.len); c.cell0 = p.cells; c.row0 = d.row0; c.pad_ = 0;
        p.rows += c.F; p.cols += (long long)kRsBand * c.Fs; p.windows += c.nwin; p.runs += c.nruns;
        p.tiles += (c.F + kRsTile - 1) / kRsTile; p.cells += c.nb + 1;
        samples += d.n;
        if (samples > kRsMaxCallSamples) return RS_TOTAL;
    }
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; i++) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return offset[a] < offset[b] || (offset[a] == offset[b] && a < b); });
    for (int i = 1; i < n; i++) {
        const int a = order[(size_t)i - 1], b = order[(size_t)i];
        if (offset[a] + n_samples[a] > offset[b]) { *bad = b; return RS_OVERLAP; }
    }
    *plan = p; *bad = -1;
    return RS_OK;
}

// The order statistic as the floor launch finds it, serially: rank r of the bit patterns v[0 .. count), digit by digit from the top
inline unsigned rs_select_serial(const unsigned* v, int count, int r) {
    unsigned prefix = 0;
    for (int pass = 0; pass < 4; pass++) {
        int hist[256] = {0};
        for (int i = 0; i < count; i++)
            if (rs_above(v[i], pass) == prefix) hist[rs_digit(v[i], pass)]++;
        prefix = (prefix << 8) | (unsigned)rs_pick(hist, r, &r);
    }
    return prefix;
}
