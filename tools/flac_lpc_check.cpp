// The level-1 FLAC encoder's per-block arithmetic (csrc/flac_lpc_core.h: window, autocorrelation, Levinson-Durbin in fp64, quantisation,
// residual guard) run serially on the CPU, the same text wave_flac_frame_kernel<true> compiles.  Built with -ffp-contract=off
// -fsanitize=address,undefined, this is the evidence for the core's fp64 exactness and its int32 bounds: tests/test_flac_lpc_core.py builds
// it, runs it and compares every line with the Python definition (wave_codec.flac_lpc_coefficients / flac_lpc_residual).
//
//   flac_lpc_check blocks FILE     FILE holds int16 blocks of 4096, little-endian; per block and order one line
//                                  "order valid shift inside q0 q1 ..." (inside: every residual below the guard; 0 when not valid)
//   flac_lpc_check guard FILE      FILE holds blocks as above, each followed by 12 int32 coefficients and one int32 shift: per block one line
//                                  "inside" for order 12 with those hand-made coefficients
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tts-indic-server-f5_amd/csrc/flac_lpc_core.h"

int main(int argc, char** argv) {
    if (argc != 3 || (strcmp(argv[1], "blocks") && strcmp(argv[1], "guard"))) { fprintf(stderr, "usage: flac_lpc_check blocks|guard FILE\n"); return 2; }
    const bool guard = !strcmp(argv[1], "guard");
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    fseek(f, 0, SEEK_END);
    const long long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    const long long record = 2LL * kFl1Block + (guard ? 4LL * (kFl1MaxOrder + 1) : 0);
    if (n % record) { fprintf(stderr, "%s: not a whole number of records\n", argv[2]); return 2; }
    for (long long at = 0; at < n; at += record) {
        int16_t* x = (int16_t*)malloc(2 * kFl1Block);               // exactly one block: the sanitizer guards both ends
        if (fread(x, 2, kFl1Block, f) != (size_t)kFl1Block) { perror(argv[2]); return 2; }
        if (guard) {
            int32_t tail[kFl1MaxOrder + 1];
            if (fread(tail, 4, kFl1MaxOrder + 1, f) != (size_t)(kFl1MaxOrder + 1)) { perror(argv[2]); return 2; }
            unsigned top = 0;
            for (int i = kFl1MaxOrder; i < kFl1Block; i++) {
                const unsigned u = fl1_residual(x + i, tail, kFl1MaxOrder, tail[kFl1MaxOrder]);
                if (u > top) top = u;
            }
            printf("%d\n", top < kFl1Guard ? 1 : 0);
        } else {
            Fl1Order orders[kFl1Orders];
            int inside[kFl1Orders];
            fl1_block(x, orders, inside);
            for (int c = 0; c < kFl1Orders; c++) {
                printf("%d %d %d %d", fl1_order(c), orders[c].valid, orders[c].shift, inside[c]);
                for (int j = 0; j < fl1_order(c); j++) printf(" %d", orders[c].q[j]);
                printf("\n");
            }
        }
        free(x);
    }
    fclose(f);
    return 0;
}
