// The reference-clip pre-step's rule (csrc/ref_prestep.h: prefix sums, window flags, clip at a pause, edges) run serially on the CPU over
// csrc/ref_prestep_core.h, the same text the kernels compile.  Built with -fsanitize=address,undefined, this is the evidence for the core's
// bounds: every table lives in a heap block of exactly its size -- the L millisecond sums, the L + 1 prefix sums, each pass's window flags and
// the per-frame sums that stand in for the samples of a partial cell -- so a read past a table's end is a sanitizer report.
// tests/test_ref_prestep_core.py builds and runs it.
//
//   ref_prestep_check --constants   "T1 T2 lead": the integer rms thresholds the core compares against
//   ref_prestep_check FILE...       FILE = int64 little-endian: frames N, channels, rate, clip_short, then the sum of squares of every
//                                   millisecond cell [frame(m), frame(m + 1)), m = 0 .. L - 1, then the sum of squares of every frame
//                                   (N values).  One line per FILE: "nr a0 b0 a1 b1 ... tail_frames", the ranges of
//                                   audio_prep.preprocess_ref_ranges
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../tts-indic-server-f5_amd/csrc/ref_prestep_core.h"

struct FramePart {                 // the exact sum over source frames [a, b), as the kernels take it from the samples
    const long long* sq;
    long long operator()(long long a, long long b) const {
        long long s = 0;
        for (long long f = a; f < b; f++) s += sq[f];
        return s;
    }
};

static long long isqrt_floor(long long v) {
    long long r = 0;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%lld %lld %lld\n", isqrt_floor(kRpPass1Square) - 1, isqrt_floor(kRpPass2Square) - 1, isqrt_floor(kRpEdgeSquare));
        return 0;
    }
    if (argc < 2) { fprintf(stderr, "usage: ref_prestep_check --constants | FILE...\n"); return 2; }
    for (int arg = 1; arg < argc; arg++) {
        FILE* f = fopen(argv[arg], "rb");
        if (!f) { perror(argv[arg]); return 2; }
        long long head[4];
        if (fread(head, sizeof(long long), 4, f) != 4) { fprintf(stderr, "%s: short header\n", argv[arg]); return 2; }
        const long long N = head[0];
        const int C = (int)head[1], rate = (int)head[2];
        const bool clip_short = head[3] != 0;
        if (N < 0 || C < 1 || rate < kRpMinRate || (long long)rate * C >= kRpMaxWindowSamples) { fprintf(stderr, "%s: refused\n", argv[arg]); return 2; }
        const RpGeom g = rp_geom(N, C, rate);
        long long* cells = (long long*)malloc(sizeof(long long) * (g.L ? g.L : 1));      // exactly the tables: the sanitizer guards their ends
        long long* sq = (long long*)malloc(sizeof(long long) * (N ? N : 1));
        if ((g.L && fread(cells, sizeof(long long), g.L, f) != (size_t)g.L) || (N && fread(sq, sizeof(long long), N, f) != (size_t)N) || fgetc(f) != EOF) {
            fprintf(stderr, "%s: needs %lld cell sums and %lld frame sums\n", argv[arg], g.L, N);
            return 2;
        }
        fclose(f);
        long long* P = (long long*)malloc(sizeof(long long) * (g.L + 1));
        P[0] = 0;
        for (long long m = 0; m < g.L; m++) P[m + 1] = P[m] + cells[m];
        free(cells);
        uint8_t* flags[2];
        for (int p = 0; p < 2; p++) {
            const long long nwin = rp_nwin(g.L, rp_pass_ms(p));
            flags[p] = (uint8_t*)malloc(nwin ? nwin : 1);
            for (long long w = 0; w < nwin; w++)
                flags[p][w] = rp_window_silent(g, P, rp_window_start(g.L, rp_pass_ms(p), w), rp_pass_ms(p), rp_pass_square(p)) ? 1 : 0;
        }
        RpRanges r;
        rp_clip(g, flags, clip_short, r);
        if (r.overflow) { fprintf(stderr, "%s: more than %d ranges\n", argv[arg], kRpMaxRanges); return 3; }
        const FramePart part{sq};
        long long lead = -1, last_loud = -1;
        const long long nlead = rp_lead_windows(r, rate);
        for (long long i = 0; i < nlead && lead < 0; i++)
            if (rp_lead_loud(g, P, part, r, i)) lead = i;
        const RpEdges e = rp_edges(g, r, lead);
        for (long long m = e.L2 - 1; m >= 0 && last_loud < 0; m--)
            if (rp_trail_loud(g, P, part, r, e, m)) last_loud = m;
        rp_finish(g, r, e, last_loud);
        printf("%d", r.nr);
        for (int i = 0; i < r.nr; i++) printf(" %lld %lld", r.a[i], r.b[i]);
        printf(" %lld\n", rp_tail_frames(rate));
        free(flags[0]); free(flags[1]); free(P); free(sq);
    }
    return 0;
}
