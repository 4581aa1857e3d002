// The grain launch of the formant shift (csrc/wave_formant.h wave_shape_kernel) run serially on the CPU over csrc/wave_formant_core.h, the
// same text the kernel compiles: per output tile the marks that may touch it (fs_tile_marks), their grains (fs_grain), the staged source
// window, and per run of 8 outputs the gather (fs_gather) and the rounded divide (fs_finish).  Built with -fsanitize=address,undefined,
// this is the evidence for the bounds the core derives: the samples, both mark lists, a tile's grains (kFsTileGrains), its staged window
// (kFsStage) and the output each live in a heap block of exactly their size, so a read or write past an end is a sanitizer report.
// tests/test_shape_core.py builds and runs it, and passes the marks in.
//
//   wave_shape_check --constants   "half_max tile_grains drift reach stage run"
//   wave_shape_check FILE...       FILE = little-endian int32 P, Q (the formant ratio), n, na, ns, then na analysis marks (a, T, voiced),
//                                  ns synthesis marks (u, i), then n int16 samples.  One line per FILE: n and the n samples of
//                                  wave_codec.psola_shape_pcm16
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../tts-indic-server-f5_amd/csrc/wave_formant_core.h"

static const unsigned short kWindow[kFpTable + 1] = {
#include "../tts-indic-server-f5_amd/csrc/psola_window.inc"
};

template <typename T>
static T* block(long long count) { return (T*)malloc(sizeof(T) * (size_t)count); }   // exactly `count`: the sanitizer guards both ends

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%d %d %d %d %d %d\n", kFsHalfMax, kFsTileGrains, kFsDrift, kFsReach, kFsStage, kFsRun);
        return 0;
    }
    if (argc < 2) { fprintf(stderr, "usage: wave_shape_check --constants | FILE...\n"); return 2; }
    for (int arg = 1; arg < argc; arg++) {
        FILE* f = fopen(argv[arg], "rb");
        if (!f) { perror(argv[arg]); return 2; }
        int32_t head[5];
        if (fread(head, sizeof(int32_t), 5, f) != 5) { fprintf(stderr, "%s: refused (header)\n", argv[arg]); return 2; }
        const int P = head[0], Q = head[1], na = head[3], ns = head[4];
        const long long n = head[2];
        if (!fs_ratio_ok(P, Q) || n < 0 || na < 0 || ns < 0 || na > fp_max_marks(n) || ns > fp_max_synth(n)) {
            fprintf(stderr, "%s: refused\n", argv[arg]);
            return 2;
        }
        FpMark* marks = block<FpMark>(na);
        FpSynth* synth = block<FpSynth>(ns);
        short* x = block<short>(n);
        bool ok = true;
        for (int i = 0; i < na && ok; i++) {
            int32_t m[3];
            ok = fread(m, sizeof(int32_t), 3, f) == 3 && m[0] >= 0 && m[0] < n && m[1] >= kFpLagMin && m[1] <= kFpLagMax;
            if (ok) { marks[i].a = m[0]; marks[i].T = m[1] | (m[2] ? 1 << 16 : 0); }
        }
        for (int i = 0; i < ns && ok; i++) {
            int32_t m[2];
            ok = fread(m, sizeof(int32_t), 2, f) == 2 && m[0] >= 0 && m[0] < n && m[1] >= 0 && m[1] < na && (i == 0 || m[0] - synth[i - 1].u >= kFpMinStep);
            if (ok) { synth[i].u = m[0]; synth[i].i = m[1]; }
        }
        if (!ok || (n && fread(x, sizeof(short), n, f) != (size_t)n) || fgetc(f) != EOF) { fprintf(stderr, "%s: refused (marks or samples)\n", argv[arg]); return 2; }
        fclose(f);

        short* y = block<short>(n);
        FsGrain* grains = block<FsGrain>(kFsTileGrains);
        short* stage = block<short>(kFsStage);
        for (long long tile = 0; tile < fp_out_tiles(n); tile++) {
            const long long j0 = tile * kFpOutTile, j1 = j0 + kFpOutTile < n ? j0 + kFpOutTile : n, base = fs_stage_base(j0);
            int m0;
            const int ng = fs_tile_marks(synth, ns, j0, j1, &m0);
            for (int m = 0; m < ng; m++) {
                const FpMark mk = marks[synth[m0 + m].i];
                grains[m] = fs_grain(synth[m0 + m].u, mk.a, mk.T & 0xffff, (mk.T >> 16) & 1, P, Q);
                if (grains[m].H < 0) { fprintf(stderr, "%s: mark %d lies %d samples from the mark it reads\n", argv[arg], m0 + m, grains[m].u - mk.a); return 3; }
            }
            for (int i = 0; i < kFsStage; i++) stage[i] = fs_stage_sample(x, n, base + i);
            for (long long j = j0; j < j1; j += kFsRun) {                        // (a run may end behind the wave, as a thread's does)
                long long num[kFsRun], den[kFsRun];
                for (int e = 0; e < kFsRun; e++) num[e] = den[e] = 0;
                for (int m = ng - 1; m >= 0; m--) fs_gather(grains[m], Q, j, stage, base, kWindow, num, den);   // (any order: integer sums)
                for (int e = 0; e < kFsRun && j + e < j1; e++) y[j + e] = (short)fs_finish(num[e], den[e], stage[j + e - base]);
            }
        }
        printf("%lld", n); for (long long j = 0; j < n; j++) printf(" %d", (int)y[j]); printf("\n");
        free(marks); free(synth); free(x); free(y); free(grains); free(stage);
    }
    return 0;
}
