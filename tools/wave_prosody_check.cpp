// The WSOLA launch's frame loop (csrc/wave_out.h wave_wsola_kernel: window and target staging, the search, the packed key, the blend) run
// serially on the CPU over csrc/wave_prosody_core.h, the same text the kernel compiles.  Built with -fsanitize=address,undefined, this is the
// evidence for the core's bounds: the samples, the candidate window, the target and the output each live in a heap block of exactly their
// size, so a read or write past an end is a sanitizer report.  tests/test_wave_prosody_core.py builds and runs it.
//
//   wave_prosody_check --constants   "L H D cands window": the constants the core compiles
//   wave_prosody_check FILE...       FILE = little-endian int32 P, Q, n, then n int16 samples.  Two lines per FILE: "K s_0 .. s_{K-1}" and
//                                    "m y_0 .. y_{m-1}", the frame starts and the samples of wave_codec._wsola_frames
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../tts-indic-server-f5_amd/csrc/wave_prosody_core.h"

static const int kRise[kPrHop] = {
#include "../tts-indic-server-f5_amd/csrc/wsola_window.inc"
};

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%d %d %d %d %d\n", kPrFrame, kPrHop, kPrSearch, kPrCands, kPrWindow);
        return 0;
    }
    if (argc < 2) { fprintf(stderr, "usage: wave_prosody_check --constants | FILE...\n"); return 2; }
    for (int arg = 1; arg < argc; arg++) {
        FILE* f = fopen(argv[arg], "rb");
        if (!f) { perror(argv[arg]); return 2; }
        int32_t head[3];
        if (fread(head, sizeof(int32_t), 3, f) != 3) { fprintf(stderr, "%s: short header\n", argv[arg]); return 2; }
        const int P = head[0], Q = head[1];
        const long long n = head[2];
        if (!pr_stretch_ok(P, Q) || n < 0) { fprintf(stderr, "%s: refused\n", argv[arg]); return 2; }
        short* x = (short*)malloc(sizeof(short) * (n ? n : 1));                 // exactly the samples: the sanitizer guards their ends
        if ((n && fread(x, sizeof(short), n, f) != (size_t)n) || fgetc(f) != EOF) { fprintf(stderr, "%s: needs %lld samples\n", argv[arg], n); return 2; }
        fclose(f);
        if (n == 0) { free(x); x = (short*)malloc(0); }
        const PrGeom g = pr_geom(n, P, Q);
        short* y = (short*)malloc(sizeof(short) * g.m);
        unsigned short* win = (unsigned short*)malloc(sizeof(unsigned short) * kPrWindow);
        unsigned short* tgt = (unsigned short*)malloc(sizeof(unsigned short) * kPrFrame);
        printf("%lld", g.K ? g.K : 1);
        long long s = -kPrHop;
        printf(" %lld", s);
        for (long long k = 1; k < g.K; k++) {
            const long long pk = pr_nominal(g, k), t = s + kPrHop;
            for (int i = 0; i < kPrWindow; i++) win[i] = (unsigned short)pr_source(x, n, pk - kPrSearch + i);
            for (int i = 0; i < kPrFrame; i++) tgt[i] = (unsigned short)pr_source(x, n, t + i);
            unsigned long long best = ~0ULL;
            for (int c = kPrCands - 1; c >= 0; c--) {                              // (any order: the key decides)
                unsigned cost = 0;
                for (int i = 0; i < kPrFrame; i++) cost += win[c + i] > tgt[i] ? win[c + i] - tgt[i] : tgt[i] - win[c + i];
                const unsigned long long key = pr_key(cost, c - kPrSearch);
                if (key < best) best = key;
            }
            const int c = pr_key_offset(best) + kPrSearch;
            s = pk + c - kPrSearch;
            printf(" %lld", s);
            for (int i = 0; i < kPrHop; i++) {                                      // frame k - 1's outputs: its falling half over frame k's rising half
                const long long j = (k - 1) * kPrHop + i;
                if (j < g.m) y[j] = (short)pr_blend(kRise[i], pr_unbias(tgt[i]), pr_unbias(win[c + i]));
            }
        }
        printf("\n%lld", g.m);
        for (long long j = 0; j < g.m; j++) printf(" %d", (int)y[j]);
        printf("\n");
        free(x); free(y); free(win); free(tgt);
    }
    return 0;
}
