// The watermark's trace ids (csrc/wave_mark.h wave_mark_sum_kernel / wave_mark_id_add_kernel: the tiles, the masked block sums, the envelope,
// the groups of 8 samples, the key's row and the three rotated sub-key rows; watermark_id_score_kernel's candidate offsets) run serially on the
// CPU over csrc/wave_mark_core.h, the same text the kernels compile.  Built with -fsanitize=address,undefined, this is the evidence for the
// core's bounds: the samples, the block sums and each of the four carrier rows live in a heap block of exactly their size, so a read or
// write past an end is a sanitizer report.  tests/test_wave_mark_id_core.py builds and runs it.
//
//   wave_mark_id_check --constants    "symbols step symbol_bits id_max id_shift tag_rows read_keys_max row_words": the constants the core compiles
//   wave_mark_id_check --subkeys KEY  the key's three sub-keys
//   wave_mark_id_check --grid O S     the offset of a sub-key's correlation that candidate symbol S reads when the key's offset is O
//   wave_mark_id_check FILE...        FILE = little-endian uint64 key, int32 id (-1: none), int32 n, int32 len (the device length, <= n), then n
//                                     int16 samples.  One line per FILE: "n fnv1a changed y_0 .. y_{min(n, 64) - 1}": the digest of all n
//                                     samples afterwards (the first len of them marked), how many changed, and the first samples
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../tts-indic-server-f5_amd/csrc/wave_mark_core.h"

static const int kTaps[kWmTaps] = {
#include "../tts-indic-server-f5_amd/csrc/watermark_taps.inc"
};

static unsigned long long fnv1a(const short* v, long long n) {   // over the little-endian bytes of the samples
    unsigned long long h = 0xcbf29ce484222325ULL;
    for (long long i = 0; i < n; i++) {
        const unsigned u = (unsigned short)v[i];
        h = (h ^ (u & 0xff)) * 0x100000001b3ULL;
        h = (h ^ (u >> 8)) * 0x100000001b3ULL;
    }
    return h;
}

static short* carrier_of(unsigned long long key) {
    signed char* chips = (signed char*)malloc(kWmPeriod);
    short* c = (short*)malloc(sizeof(short) * kWmPeriod);
    wm_carrier(key, kTaps, chips, c);
    free(chips);
    return c;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%d %d %d %d %d %d %d %d\n", kWmIdSymbols, kWmIdStep, kWmIdSymbolBits, kWmIdMax, kWmIdShift, kWmTagRows, kWdIdKeysMax, kWdIdRowWords);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "--subkeys")) {
        const unsigned long long key = strtoull(argv[2], nullptr, 0);
        if (!wm_key_ok(key)) { fprintf(stderr, "%s: refused\n", argv[2]); return 2; }
        for (int d = 0; d < kWmIdSymbols; d++) printf("%llu%c", wm_subkey(key, d), d + 1 < kWmIdSymbols ? ' ' : '\n');
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "--grid")) {
        const int o = atoi(argv[2]), s = atoi(argv[3]);
        if (o < 0 || o >= kWmPeriod || s < 0 || s >= kWmIdSymbolCount) { fprintf(stderr, "%s %s: refused\n", argv[2], argv[3]); return 2; }
        printf("%d\n", wd_id_offset(o, s));
        return 0;
    }
    if (argc < 2) { fprintf(stderr, "usage: wave_mark_id_check --constants | --subkeys KEY | --grid O S | FILE...\n"); return 2; }
    for (int arg = 1; arg < argc; arg++) {
        FILE* f = fopen(argv[arg], "rb");
        if (!f) { perror(argv[arg]); return 2; }
        unsigned long long key;
        int32_t head[3];
        if (fread(&key, sizeof key, 1, f) != 1 || fread(head, sizeof(int32_t), 3, f) != 3) { fprintf(stderr, "%s: short header\n", argv[arg]); return 2; }
        const int id = head[0];
        const long long n = head[1], len = head[2];
        if (!wm_key_ok(key) || id < -1 || id > kWmIdMax || n < 0 || len < 0 || len > n) { fprintf(stderr, "%s: refused\n", argv[arg]); return 2; }
        short* x = (short*)malloc(sizeof(short) * (size_t)n);               // exactly the samples: the sanitizer guards their ends
        if ((n && fread(x, sizeof(short), (size_t)n, f) != (size_t)n) || fgetc(f) != EOF) { fprintf(stderr, "%s: needs %lld samples\n", argv[arg], n); return 2; }
        fclose(f);
        short* before = (short*)malloc(sizeof(short) * (size_t)n);
        if (n) memcpy(before, x, sizeof(short) * (size_t)n);
        short* rows[kWmTagRows];                                             // each row a heap block of its own: an index past a row is a report
        rows[0] = carrier_of(key);
        for (int d = 0; d < kWmIdSymbols; d++) rows[1 + d] = carrier_of(wm_subkey(key, d));
        const long long tiles = wm_tiles(n), nA = tiles * kWmTileBlocks;
        int* A = (int*)malloc(sizeof(int) * (size_t)nA);
        for (long long t = 0; t < tiles; t++)                                // launch 1: every block sum of every tile, masked by the length
            for (int b = 0; b < kWmTileBlocks; b++) A[t * kWmTileBlocks + b] = wm_block_sum(x, len, t * kWmTileBlocks + b);
        for (long long t = 0; t < tiles; t++)                                // launch 2: groups of 8 samples
            for (int grp = 0; grp < kWmTile / 8; grp++) {
                const long long j = t * kWmTile + 8LL * grp;
                if (j >= len) break;
                const int E = wm_envelope(A, nA, j / kWmBlock);
                if (E == 0) continue;
                int C[8];
                const short* k8 = rows[0] + (j & (kWmPeriod - 1));           // the kernel's 16-byte loads: 8 values of each row
                for (int e = 0; e < 8; e++) C[e] = 2 * k8[e];
                if (id >= 0)
                    for (int d = 0; d < kWmIdSymbols; d++) {
                        const short* d8 = rows[1 + d] + wm_id_index(j, wm_id_symbol(id, d));
                        for (int e = 0; e < 8; e++) C[e] += d8[e];
                    }
                for (int e = 0; e < 8 && j + e < len; e++) x[j + e] = (short)wm_mark_id(x[j + e], E, C[e]);
            }
        long long changed = 0;
        for (long long j = 0; j < n; j++) changed += x[j] != before[j];
        printf("%lld %llu %lld", n, fnv1a(x, n), changed);
        for (long long j = 0; j < n && j < 64; j++) printf(" %d", (int)x[j]);
        printf("\n");
        free(x); free(before); free(A);
        for (int t = 0; t < kWmTagRows; t++) free(rows[t]);
    }
    return 0;
}
