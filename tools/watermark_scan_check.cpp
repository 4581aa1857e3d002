// The watermark scan's range arithmetic (csrc/wave_mark.h ws_range_fold_kernel / f5hip_watermark_scan: the segments of a recording, a
// range's first sample and sample count, the samples a residue adds, the four frames that hold a sample) run serially on the CPU over
// csrc/wave_mark_core.h, the same text the kernel compiles.  Built with -fsanitize=address,undefined, this is the evidence for the core's
// bounds: the frames live in a heap block of exactly ws_frames(n) * 1024 floats and the fold row in one of exactly 16384, so a read or write
// past an end is a sanitizer report.  tests/test_watermark_scan_core.py builds and runs it and equates its output with the Python definition.
//
//   watermark_scan_check --constants          "window slack max_samples ranges_max slab_rows nfft hop pad": the constants the core compiles
//   watermark_scan_check --slabs RANGES ROWS  ranges per slab and slabs of a call of RANGES ranges and ROWS carrier rows (1 .. 16)
//   watermark_scan_check N FIRST COUNT [M...] one range of a recording of N samples.  Line 1: "S F samples": segments, frames, the range's
//                                             sample count.  Line 2: "pairs sum fold": over ALL 16384 residues, the (sample, frame) pairs read,
//                                             the sum of (m + 1) (1024 f + o) over them mod 2^64, and the sum of (m % 13 + 1) Z[m] of the fold
//                                             of frames filled with fw[f][o] = (7 f + 3 o) % 11.  Then per residue M: "M: j f:o f:o f:o f:o; ..."
//                                             -- each sample it adds, ascending, with its four frames and positions, ascending
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../tts-indic-server-f5_amd/csrc/wave_mark_core.h"

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%d %d %d %d %d %d %d %d\n", kWsWindow, kWsSlack, kWsMaxSamples, kWsRangesMax, kWsSlabRows, kWsNfft, kWsHop, kWsPad);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "--slabs")) {
        const int ranges = atoi(argv[2]), rows = atoi(argv[3]);
        if (ranges < 1 || ranges > kWsRangesMax || rows < 1 || rows > kWmKeysMax) { fprintf(stderr, "%s %s: refused\n", argv[2], argv[3]); return 2; }
        printf("%d %d\n", ws_slab_ranges(rows), ws_slabs(ranges, rows));
        return 0;
    }
    if (argc < 4) { fprintf(stderr, "usage: watermark_scan_check --constants | --slabs RANGES ROWS | N FIRST COUNT [M...]\n"); return 2; }
    const long long n = atoll(argv[1]), first = atoll(argv[2]), count = atoll(argv[3]);
    if (n < 1 || n > kWsMaxSamples || !ws_range_ok(n, first, count)) { fprintf(stderr, "%s %s %s: refused\n", argv[1], argv[2], argv[3]); return 2; }
    const int S = ws_segments(n), F = ws_frames(n);
    const long long j0 = ws_range_first((int)first);
    const int samples = ws_range_samples(n, (int)first, (int)count);
    printf("%d %d %d\n", S, F, samples);
    float* fw = (float*)malloc(sizeof(float) * (size_t)F * kWsNfft);     // exactly the frames: the sanitizer guards their ends
    float* Z = (float*)malloc(sizeof(float) * kWmPeriod);
    for (int f = 0; f < F; f++)
        for (int o = 0; o < kWsNfft; o++) fw[(size_t)f * kWsNfft + o] = (float)((7LL * f + 3LL * o) % 11);
    unsigned long long pairs = 0, sum = 0;
    for (int m = 0; m < kWmPeriod; m++) {                                // ws_range_fold_kernel's thread (range, m)
        float acc = 0.0f;
        for (int k = 0;; k++) {
            const long long j = ws_fold_sample(j0, m, k);
            if (j >= j0 + samples) break;
            const int f0 = ws_sample_frame0(j);
            float u = 0.0f;
            for (int d = 0; d < kWsFramesPerSample; d++) {
                const int o = ws_sample_offset(j, f0 + d);
                u += fw[(size_t)(f0 + d) * kWsNfft + o];
                pairs++;
                sum += (unsigned long long)(m + 1) * (unsigned long long)(1024LL * (f0 + d) + o);
            }
            acc += u;
        }
        Z[m] = acc;
    }
    double fold = 0.0;
    for (int m = 0; m < kWmPeriod; m++) fold += (double)(m % 13 + 1) * (double)Z[m];
    printf("%llu %llu %.0f\n", pairs, sum, fold);
    for (int arg = 4; arg < argc; arg++) {
        const int m = atoi(argv[arg]);
        if (m < 0 || m >= kWmPeriod) { fprintf(stderr, "%s: refused\n", argv[arg]); return 2; }
        printf("%d:", m);
        for (int k = 0;; k++) {
            const long long j = ws_fold_sample(j0, m, k);
            if (j >= j0 + samples) break;
            const int f0 = ws_sample_frame0(j);
            printf(" %lld", j);
            for (int d = 0; d < kWsFramesPerSample; d++) printf(" %d:%d", f0 + d, ws_sample_offset(j, f0 + d));
            printf(";");
        }
        printf("\n");
    }
    free(fw); free(Z);
    return 0;
}
