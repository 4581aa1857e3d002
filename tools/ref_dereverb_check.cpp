// The reference-clip dereverberator's geometry (csrc/ref_dereverb.h: the staged chunk of a bin's delay line, the power window of lam, the
// chunking of a clip's frames, the clip table) walked serially on the CPU over csrc/ref_dereverb_core.h, the same text the kernel compiles.
// Built with -fsanitize=address,undefined, this is the evidence for the core's bounds: one bin's X and Y columns [F] and the two staging
// arrays xs [kRvStage] and ps [kRvPow] live in heap blocks of exactly their size, every index the kernel forms is formed here and used, so one
// past a table's end is a sanitizer report.  tests/test_ref_dereverb_core.py builds and runs it.
//
//   ref_dereverb_check --constants   "delay taps iterations chunk halo stage pow group_bins groups cols floor load tiny"
//   ref_dereverb_check N...          per N one line "N F chunks taps": the frames, the chunks and the taps that fall inside the clip
//   ref_dereverb_check --table       the clip table: a ragged call's rows and sample starts, then refusals by their code
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../tts-indic-server-f5_amd/csrc/ref_dereverb_core.h"

static int walk(long long n) {
    const int F = rd_frames(n), chunks = rv_chunks(F);
    int* X = (int*)malloc(sizeof(int) * (size_t)F);           // a column holds its own frame index, so a slot can be checked against its rule
    int* Y = (int*)malloc(sizeof(int) * (size_t)F);
    int* xs = (int*)malloc(sizeof(int) * kRvStage);
    int* ps = (int*)malloc(sizeof(int) * kRvPow);
    if (!X || !Y || !xs || !ps) { fprintf(stderr, "out of memory at n = %lld\n", n); return 2; }
    for (int f = 0; f < F; f++) X[f] = Y[f] = f;
    long long taps = 0, covered = 0;
    for (int ch = 0; ch < chunks; ch++) {
        const int base = ch * kRvChunk, frames = std::min(kRvChunk, F - base);
        if (frames < 1) return 3;
        for (int s = 0; s < kRvStage; s++) {                  // rv_stage: a frame outside the clip is a zero (-1 here), never a read
            const int f = rv_stage_frame(base, s);
            xs[s] = f >= 0 && f < F ? X[f] : -1;
        }
        for (int s = 0; s < kRvPow; s++) ps[s] = Y[rv_pow_frame(base, s, F)];
        for (int t = 0; t < frames + (frames & 1); t++) {     // the Gram pass: two frames a step, so an odd chunk reads one slot past its frames
            const int f = base + t;
            for (int j = 0; j < kRvTaps; j++) {
                const int got = xs[rv_tap_slot(t, j)], want = f - kRvDelay - j;
                if (got != (want >= 0 && want < F ? want : -1)) { fprintf(stderr, "n = %lld: frame %d tap %d reads frame %d\n", n, f, j, got); return 3; }
                if (t < frames && got >= 0) taps++;
            }
            if (xs[rv_own_slot(t)] != (f < F ? f : -1)) { fprintf(stderr, "n = %lld: frame %d reads frame %d as its own\n", n, f, xs[rv_own_slot(t)]); return 3; }
            if (t >= frames) continue;
            if (ps[t] != rd_clamp(f - 1, F) || ps[t + 1] != f || ps[t + 2] != rd_clamp(f + 1, F)) { fprintf(stderr, "n = %lld: lam of frame %d\n", n, f); return 3; }
            Y[f] = f;                                         // the filter pass writes the frames it read
            covered++;
        }
    }
    if (covered != F) return 3;
    printf("%lld %d %d %lld\n", n, F, chunks, taps);
    free(X); free(Y); free(xs); free(ps);
    return 0;
}

static int table() {
    const int32_t len[3] = {1, kRdMaxSamples, 32257};
    const int64_t off[3] = {5000000, 10, 2000000};
    std::vector<RdClip> h;
    long long rows = 0, samples = 0;
    int bad = 0;
    if (rv_layout(3, off, len, h, &rows, &samples, &bad) != RD_OK) return 3;
    printf("ok %lld %lld", rows, samples);
    for (const RdClip& c : h) printf(" %d:%d:%lld:%lld", c.row0, c.F, c.out0, c.off);
    printf("\n");
    const int32_t zero_len[2] = {10, 0}, long_len[2] = {10, kRdMaxSamples + 1}, ok_len[2] = {10, 5};
    const int64_t apart[2] = {0, 10}, negative[2] = {0, -1}, over[2] = {0, 9};
    printf("%d ", rv_layout(0, apart, ok_len, h, &rows, &samples, &bad));
    printf("%d ", rv_layout(2, apart, zero_len, h, &rows, &samples, &bad));
    printf("%d ", rv_layout(2, apart, long_len, h, &rows, &samples, &bad));
    printf("%d ", rv_layout(2, negative, ok_len, h, &rows, &samples, &bad));
    printf("%d ", rv_layout(2, over, ok_len, h, &rows, &samples, &bad));
    printf("%d ", rv_layout(2, nullptr, ok_len, h, &rows, &samples, &bad));
    // one (clip, bin group) workgroup too many for a grid: refused before the tables are looked at
    printf("%d ", rv_layout(2147483647 / kRvGroups + 1, nullptr, nullptr, h, &rows, &samples, &bad));
    printf("%d\n", rv_layout(2, apart, ok_len, h, &rows, &samples, &bad));
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%d %d %d %d %d %d %d %d %d %d %g %g %g\n", kRvDelay, kRvTaps, kRvIters, kRvChunk, kRvHalo, kRvStage, kRvPow, kRvGroupBins, kRvGroups, kRvCols,
               (double)kRvFloorRel, (double)kRvLoadRel, (double)kRvTiny);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "--table")) return table();
    if (argc < 2) { fprintf(stderr, "usage: ref_dereverb_check --constants | --table | N...\n"); return 2; }
    for (int a = 1; a < argc; a++) {
        const long long n = atoll(argv[a]);
        if (n < 1 || n > kRdMaxSamples) { fprintf(stderr, "%s: refused\n", argv[a]); return 2; }
        const int rc = walk(n);
        if (rc) return rc;
    }
    return 0;
}
