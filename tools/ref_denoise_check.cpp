// The reference-clip denoiser's geometry (csrc/ref_denoise.h: the frames of a clip, the smoothing window, the overlap-add, the clip table)
// walked serially on the CPU over csrc/ref_denoise_core.h, the same text the kernels compile.  Built with -fsanitize=address,undefined, this
// is the evidence for the core's bounds: the clip, its powers P [F][516], its frames fw [F][1024] and the cover counts live in heap blocks of
// exactly their size, every index the kernels form is formed here and used, so one past a table's end is a sanitizer report.
// tests/test_ref_denoise_core.py builds and runs it.
//
//   ref_denoise_check --constants        "n_fft hop pad bins p_stride rank_div subtract min_gain max_samples"
//   ref_denoise_check N...               per N one line "N F r reads": the frames, the rank and the clip samples read by all frames (4 N)
//   ref_denoise_check --table            the clip table: a ragged call's rows and sample starts, then every refusal by its code
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../tts-indic-server-f5_amd/csrc/ref_denoise_core.h"

static int walk(long long n) {
    const int F = rd_frames(n);
    float* x = (float*)malloc(sizeof(float) * (size_t)n);
    float* P = (float*)malloc(sizeof(float) * (size_t)F * kRdPStride);
    float* fw = (float*)malloc(sizeof(float) * (size_t)F * kRdNfft);
    unsigned char* cover = (unsigned char*)calloc((size_t)n, 1);
    if (!x || !P || !fw || !cover) { fprintf(stderr, "out of memory at n = %lld\n", n); return 2; }
    for (long long j = 0; j < n; j++) x[j] = (float)(j % 7);
    long long reads = 0;
    float sink = 0.0f;
    for (int m = 0; m < F; m++) {                                     // the STFT launch: one block per row, 1024 positions
        for (int i = 0; i < kRdNfft; i++) {
            const long long j = rd_frame_sample(m, i);
            if (j >= 0 && j < n) { sink += x[j]; cover[j]++; reads++; }
        }
        for (int k = 0; k < kRdBins; k++) P[(size_t)m * kRdPStride + k] = (float)(m + k);
    }
    for (long long j = 0; j < n; j++)
        if (cover[j] != kRdFramesPerSample) { fprintf(stderr, "n = %lld: sample %lld lies in %d frames\n", n, j, cover[j]); return 3; }
    for (int m = 0; m < F; m++)                                       // the gain launch: nine cells per (row, bin)
        for (int k = 0; k < kRdBins; k++) {
            int cells = 0;
            for (int dm = -1; dm <= 1; dm++)
                for (int dk = -1; dk <= 1; dk++) { sink += P[(size_t)rd_clamp(m + dm, F) * kRdPStride + rd_clamp(k + dk, kRdBins)]; cells++; }
            if (cells != 9) return 3;
            for (int half = 0; half < 2; half++) fw[(size_t)m * kRdNfft + (half ? (kRdNfft - k) % kRdNfft : k)] = 1.0f;
        }
    for (long long j = 0; j < n; j++) {                               // the overlap-add launch: one thread per sample
        const int m0 = rd_sample_frame0(j);
        for (int d = 0; d < kRdFramesPerSample; d++) {
            const int m = m0 + d, i = rd_sample_offset(j, m);
            if (m < 0 || m >= F || i < 0 || i >= kRdNfft || rd_frame_sample(m, i) != j) { fprintf(stderr, "n = %lld: sample %lld, frame %d, offset %d\n", n, j, m, i); return 3; }
            sink += fw[(size_t)m * kRdNfft + i];
        }
        x[j] = sink;
    }
    const int r = rd_rank(F);
    if (r < 0 || r >= F) return 3;
    printf("%lld %d %d %lld\n", n, F, r, reads);
    free(x); free(P); free(fw); free(cover);
    return 0;
}

static int table() {
    const int32_t len[4] = {1, 2100, kRdMaxSamples, 257};
    const int64_t off[4] = {5000000, 10, 2000000, 2200};
    std::vector<RdClip> h;
    long long rows = 0, samples = 0;
    int bad = 0;
    if (rd_layout(4, off, len, h, &rows, &samples, &bad) != RD_OK) return 3;
    printf("ok %lld %lld", rows, samples);
    for (const RdClip& c : h) printf(" %d:%d:%lld:%lld", c.row0, c.F, c.out0, c.off);
    printf("\n");
    struct { int32_t n; int64_t off[3]; int32_t len[3]; bool null; } bad_calls[] = {
        {0, {0, 0, 0}, {1, 1, 1}, false}, {2, {0, 10, 0}, {10, 0, 1}, false}, {2, {0, 10, 0}, {10, kRdMaxSamples + 1, 1}, false},
        {2, {0, -1, 0}, {10, 5, 1}, false}, {3, {0, 20, 9}, {10, 5, 2}, false}, {3, {100, 20, 20}, {10, 5, 1}, false}, {1, {0, 0, 0}, {1, 1, 1}, true},
    };
    for (const auto& b : bad_calls) printf("%d ", rd_layout(b.n, b.null ? nullptr : b.off, b.len, h, &rows, &samples, &bad));
    // more than 2^31 - 1 rows: clips of the greatest length, far apart
    const int many = (int)(2147483647LL / rd_frames(kRdMaxSamples)) + 1;
    std::vector<int64_t> o((size_t)many);
    std::vector<int32_t> l((size_t)many, kRdMaxSamples);
    for (int i = 0; i < many; i++) o[(size_t)i] = (int64_t)i * kRdMaxSamples;
    printf("%d ", rd_layout(many, o.data(), l.data(), h, &rows, &samples, &bad));
    printf("%d\n", rd_layout(many - 1, o.data(), l.data(), h, &rows, &samples, &bad));
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%d %d %d %d %d %d %g %g %d\n", kRdNfft, kRdHop, kRdPad, kRdBins, kRdPStride, kRdRankDiv, (double)kRdSubtract, (double)kRdMinGain, kRdMaxSamples);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "--table")) return table();
    if (argc < 2) { fprintf(stderr, "usage: ref_denoise_check --constants | --table | N...\n"); return 2; }
    for (int a = 1; a < argc; a++) {
        const long long n = atoll(argv[a]);
        if (n < 1 || n > kRdMaxSamples) { fprintf(stderr, "%s: refused\n", argv[a]); return 2; }
        const int rc = walk(n);
        if (rc) return rc;
    }
    return 0;
}
