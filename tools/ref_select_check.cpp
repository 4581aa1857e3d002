// The reference-stretch selection's order statistic, geometry and row arithmetic (csrc/ref_select.h) run serially on the CPU over
// csrc/ref_select_core.h, the same text the kernels compile.  Built with -fsanitize=address,undefined, this is the evidence for the core's
// bounds: the stage, the candidate list, the bin column and the prefix cells live in heap blocks of exactly the size the kernels hold, and a
// workgroup's walk is replayed read for read, so an index past any of them is a sanitizer report.  tests/test_ref_select_core.py builds and
// runs it.
//
//   ref_select_check --constants              "max_samples hop max_window band floor_stride stage_cap run row_words tile"
//   ref_select_check --select W HOP F SEED    a bin column of F values (SEED 0: all equal; 1: half exact zeros; else random, clustered like
//                                             a power spectrum) through every workgroup of the floor launch: per window one line
//                                             "w bits", the radix select's pick, found with the top digit's histogram kept from window to
//                                             window; exits 3 where it differs from the sorted window's element
//   ref_select_check --buckets LEN SR N       every raw sample 0 .. N - 1 through rs_bucket, against the boundaries rs_bucket_start: "nb in out"
//   ref_select_check --rows                   the snr rule and the key order on hand-written rows
//   ref_select_check --table                  a ragged call's table, then every refusal by its code
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../tts-indic-server-f5_amd/csrc/ref_select_core.h"

static unsigned bits_of(float v) { unsigned b; memcpy(&b, &v, 4); return b; }

// one workgroup of rs_window_floor_kernel, serially: windows [w0, w1) of the column col[0 .. Fs)
static int workgroup(const RsRec& c, int hop, int w0, int w1, const unsigned* col, unsigned* out) {
    unsigned* stage = (unsigned*)malloc(sizeof(unsigned) * (kRsStageCap + 8));
    unsigned* cand = (unsigned*)malloc(sizeof(unsigned) * (kRsMaxWindow + 1));
    if (!stage || !cand) return 2;
    int fa, fb;
    rs_stage_range(c, hop, w0, w1, &fa, &fb);
    const int a4 = fa & ~3, b4 = std::min(c.Fs, (fb + 3) & ~3);
    if (b4 - a4 > kRsStageCap + 8) { fprintf(stderr, "windows %d .. %d: %d values staged\n", w0, w1, b4 - a4); return 3; }
    for (int i = 0; i < b4 - a4; i++) stage[i] = col[a4 + i];
    const int base = fa - a4, Wc = c.Wc, slide = rs_slide(Wc, hop);
    int top[256] = {0};
    for (int i = 0; i < Wc; i++) top[rs_digit(stage[base + i], 0)]++;
    for (int w = w0; w < w1; w++) {
        const int o = base + hop * (w - w0);
        if (w > w0)
            for (int i = 0; i < slide; i++) {
                top[rs_digit(stage[o - hop + i], 0)]--;
                top[rs_digit(stage[o + Wc - slide + i], 0)]++;
            }
        int rank = rs_rank(Wc), nc = 0;
        unsigned prefix = (unsigned)rs_pick(top, rank, &rank);
        int hist[256] = {0};
        for (int i = 0; i < Wc; i++) {
            const unsigned v = stage[o + i];
            if (rs_above(v, 1) == prefix) { hist[rs_digit(v, 1)]++; cand[nc++] = v; }
        }
        prefix = (prefix << 8) | (unsigned)rs_pick(hist, rank, &rank);
        for (int pass = 2; pass < 4; pass++) {
            memset(hist, 0, sizeof(hist));
            for (int i = 0; i < nc; i++)
                if (rs_above(cand[i], pass) == prefix) hist[rs_digit(cand[i], pass)]++;
            prefix = (prefix << 8) | (unsigned)rs_pick(hist, rank, &rank);
        }
        out[w] = prefix;
    }
    free(stage); free(cand);
    return 0;
}

static int select(int W, int hop, int F, unsigned seed) {
    const int32_t sr = 24000, len = (F - 3) * kRdHop;
    const int64_t off = 0;
    std::vector<RsRec> h;
    std::vector<RdClip> clips;
    RsPlan plan;
    int bad = 0;
    if (len < 1 || rs_layout(1, &sr, &off, &len, W, hop, h, clips, &plan, &bad) != RS_OK || h[0].F != F) return 2;
    const RsRec c = h[0];
    unsigned* col = (unsigned*)malloc(sizeof(unsigned) * (size_t)c.Fs);
    unsigned* out = (unsigned*)malloc(sizeof(unsigned) * (size_t)c.nwin);
    unsigned* sorted = (unsigned*)malloc(sizeof(unsigned) * (size_t)c.Wc);
    if (!col || !out || !sorted) return 2;
    unsigned s = seed * 2654435761u + 12345u;
    for (int f = 0; f < c.Fs; f++) {
        s = s * 1664525u + 1013904223u;
        const float v = seed == 0 ? 0.375f : (seed == 1 && (s >> 16 & 1)) ? 0.0f : 1e-4f * (float)(1 + (s >> 8) % 4096) * (float)(1 + (s >> 24) % 7);
        col[f] = f < c.F ? bits_of(v) : 0u;
    }
    for (int r = 0; r < c.nruns; r++) {
        const int w0 = r * plan.run, w1 = c.nwin < w0 + plan.run ? c.nwin : w0 + plan.run;
        const int rc = workgroup(c, hop, w0, w1, col, out);
        if (rc) return rc;
    }
    for (int w = 0; w < c.nwin; w++) {
        const int f0 = c.F < W ? 0 : hop * w;
        memcpy(sorted, col + f0, sizeof(unsigned) * (size_t)c.Wc);
        std::sort(sorted, sorted + c.Wc);
        if (out[w] != sorted[rs_rank(c.Wc)] || out[w] != rs_select_serial(col + f0, c.Wc, rs_rank(c.Wc))) {
            fprintf(stderr, "window %d: picked %08x, the sorted window holds %08x\n", w, out[w], sorted[rs_rank(c.Wc)]);
            return 3;
        }
        printf("%d %u\n", w, out[w]);
    }
    free(col); free(out); free(sorted);
    return 0;
}

static int buckets(int len, int sr, long long n) {
    RsRec c = RsRec();
    c.len = len; c.sr = sr; c.nb = rs_buckets(len);
    int* cell = (int*)calloc((size_t)c.nb + 1, sizeof(int));
    if (!cell) return 2;
    long long in = 0, out = 0;
    for (long long j = 0; j < n; j++) {
        const int m = rs_bucket(c, j);
        if (m < 0) { if (j < rs_bucket_start(c, c.nb)) return 3; out++; continue; }
        if (m >= c.nb || j < rs_bucket_start(c, m) || j >= rs_bucket_start(c, m + 1)) { fprintf(stderr, "sample %lld -> bucket %d\n", j, m); return 3; }
        cell[m]++; in++;
    }
    if (rs_cell(c, -3) != 0 || rs_cell(c, c.nb + 3) != c.nb) return 3;
    printf("%d %lld %lld\n", c.nb, in, out);
    free(cell);
    return 0;
}

static int rows() {
    const double inf = rs_inf();
    printf("%.17g %.17g %.17g %.17g\n", rs_snr_db(0.0, 1.0), rs_snr_db(1.0, 1.0), rs_snr_db(1.0, 11.0), rs_snr_db(0.0, 0.0));
    // clipped beats snr; +inf first; -inf last; the earliest on ties
    printf("%d %d %d %d %d %d\n", rs_key_less(0, 1.0, 5, 1, 50.0, 0), rs_key_less(2, inf, 3, 2, 90.0, 0), rs_key_less(2, -inf, 0, 2, -5.0, 9),
           rs_key_less(0, 7.0, 1, 0, 7.0, 2), rs_key_less(0, 7.0, 2, 0, 7.0, 1), rs_key_less(0, inf, 4, 0, inf, 2));
    return 0;
}

static int table() {
    const int32_t sr[3] = {48000, 24000, 8000}, len[3] = {256 * 100, 1, 256 * 30 + 5};
    const int64_t off[3] = {100000, 0, 50};
    std::vector<RsRec> h;
    std::vector<RdClip> clips;
    RsPlan plan;
    int bad = 0;
    if (rs_layout(3, sr, off, len, 20, 4, h, clips, &plan, &bad) != RS_OK) return 3;
    printf("ok %lld %lld %d %d %d %d %d", plan.rows, plan.cols, plan.windows, plan.runs, plan.tiles, plan.cells, plan.run);
    for (const RsRec& c : h) printf(" %d:%d:%d:%d:%d:%d:%d:%d:%d", c.F, c.Fs, c.Wc, c.nwin, c.win0, c.run0, c.nruns, c.nb, c.cell0);
    printf("\n");
    struct { int32_t n; int32_t sr; int64_t off[2]; int32_t len[2]; int W, hop; bool null; } bad_calls[] = {
        {0, 24000, {0, 0}, {1, 1}, 20, 4, false},                        // no recordings
        {kRsMaxRecs + 1, 24000, {0, 0}, {1, 1}, 20, 4, false},           // too many
        {1, 24000, {0, 0}, {1, 1}, 20, 4, true},                         // null tables
        {1, 24000, {0, 0}, {1, 1}, 0, 4, false},                         // no window
        {1, 24000, {0, 0}, {1, 1}, kRsMaxWindow + 1, 4, false},          // a window the stage cannot hold
        {1, 24000, {0, 0}, {1, 1}, 20, 0, false},                        // no hop
        {1, 0, {0, 0}, {1, 1}, 20, 4, false},                            // no rate
        {1, 24000, {0, 0}, {0, 1}, 20, 4, false},                        // an empty recording
        {1, 24000, {0, 0}, {kRsMaxSamples + 1, 1}, 20, 4, false},        // over 600 s
        {1, 24000, {-1, 0}, {1, 1}, 20, 4, false},                       // a negative offset
        {2, 24000, {0, 4}, {5, 5}, 20, 4, false},                        // an overlap
        {2, 24000, {0, 5}, {5, kRsMaxSamples}, 1407, 1, false},          // adjacent, the longest window, the shortest hop: passes
    };
    for (const auto& b : bad_calls) {
        const int32_t rates[2] = {b.sr, b.sr};
        printf("%d ", rs_layout(b.n, b.null ? nullptr : rates, b.off, b.len, b.W, b.hop, h, clips, &plan, &bad));
    }
    int32_t sr5[5], len5[5];
    int64_t off5[5];
    for (int i = 0; i < 5; i++) { sr5[i] = 24000; len5[i] = i < 4 ? kRsMaxSamples : 1; off5[i] = (int64_t)i * kRsMaxSamples; }
    printf("%d ", rs_layout(5, sr5, off5, len5, 20, 4, h, clips, &plan, &bad));       // four of 600 s and one sample more: past the call's cap
    printf("%d ", rs_layout(4, sr5, off5, len5, 20, 4, h, clips, &plan, &bad));       // four of 600 s: passes
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%d %d %d %d %d %d %d %d %d\n", kRsMaxSamples, kRsHop, kRsMaxWindow, kRsBand, kRsFloorStride, kRsStageCap, kRsRun, kRsRowWords, kRsTile);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "--rows")) return rows();
    if (argc == 2 && !strcmp(argv[1], "--table")) return table();
    if (argc == 6 && !strcmp(argv[1], "--select")) {
        const int W = atoi(argv[2]), hop = atoi(argv[3]), F = atoi(argv[4]);
        if (W < 1 || W > kRsMaxWindow || hop < 1 || hop > kRsMaxHop || F < 4 || F > 100000) { fprintf(stderr, "--select: refused\n"); return 2; }
        return select(W, hop, F, (unsigned)atoi(argv[5]));
    }
    if (argc == 5 && !strcmp(argv[1], "--buckets")) {
        const int len = atoi(argv[2]), sr = atoi(argv[3]);
        const long long n = atoll(argv[4]);
        if (len < 1 || len > kRsMaxSamples || sr < 1 || sr > kRsMaxRate || n < 1 || n > 100000000) { fprintf(stderr, "--buckets: refused\n"); return 2; }
        return buckets(len, sr, n);
    }
    fprintf(stderr, "usage: ref_select_check --constants | --rows | --table | --select W HOP F SEED | --buckets LEN SR N\n");
    return 2;
}
