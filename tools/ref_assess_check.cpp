// The reference-clip report's run rule and index geometry (csrc/ref_assess.h: the raw side's flat index, the run of three, the 8-bin windows,
// the raw clip table) run serially on the CPU over csrc/ref_assess_core.h, the same text the kernels compile.  Built with
// -fsanitize=address,undefined, this is the evidence for the core's bounds: every clip lives in a heap block of exactly its size, the rule is
// applied to every flat index as the runs launch applies it, so a read past a channel that leaves the block is a sanitizer report.
// tests/test_ref_assess_core.py builds and runs it.
//
//   ref_assess_check --constants        "hot min_peak min_run band0 band1 floor_to_mean speech_factor bandwidth_rel mean_bins means w_stride
//                                        max_channels max_clips row_words tile"
//   ref_assess_check --runs CH N V...   a clip of CH channels of N samples (CH * N values, channel after channel): "peak_bits in_runs clipped"
//   ref_assess_check --walk CH N        every flat index of a CH x N clip through ra_channel / ra_sample, every window through its bins:
//                                       "CH N reads last_bin"
//   ref_assess_check --tiles F...       per F one line "F tiles rows_of_last": every frame row of a clip of F frames in exactly one tile, through
//                                       a cover table of exactly F cells; then the tiles of a ragged table
//   ref_assess_check --table            the raw clip table: a ragged call's entries, then every refusal by its code
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../tts-indic-server-f5_amd/csrc/ref_assess_core.h"

static int runs(int ch, long long n, char** v) {
    const long long total = (long long)ch * n;
    float* x = (float*)malloc(sizeof(float) * (size_t)total);
    if (!x) return 2;
    for (long long i = 0; i < total; i++) x[i] = strtof(v[i], nullptr);
    unsigned peak_bits = 0;                                           // the peak launch: the greatest bit pattern of |x|
    for (long long i = 0; i < total; i++) {
        unsigned b;
        memcpy(&b, &x[i], 4);
        b &= 0x7fffffffu;
        if (b > peak_bits) peak_bits = b;
    }
    float peak;
    memcpy(&peak, &peak_bits, 4);
    const RaClip c = {0, n, ch, 0};
    const float thr = ra_threshold(peak);
    long long in_runs = 0;
    if (!(peak < kRaMinPeak))                                         // the runs launch: one decision per flat index
        for (long long i = 0; i < total; i++) in_runs += ra_in_run(x + (long long)ra_channel(c, i) * c.n, c.n, ra_sample(c, i), thr) ? 1 : 0;
    printf("%u %lld %lld\n", peak_bits, in_runs, ra_clipped(in_runs, peak, total));
    free(x);
    return 0;
}

static int walk(int ch, long long n) {
    const RaClip c = {0, n, ch, 0};
    const long long total = ra_total(c);
    float* x = (float*)malloc(sizeof(float) * (size_t)total);
    float* p = (float*)malloc(sizeof(float) * (size_t)kRdPStride);
    float* w = (float*)malloc(sizeof(float) * (size_t)kRaWStride);
    if (!x || !p || !w) return 2;
    for (long long i = 0; i < total; i++) x[i] = 1.0f;                // every sample hot: every neighbour inside the channel is read
    long long reads = 0, at = 0;
    for (long long i = 0; i < total; i++) {
        const int q = ra_channel(c, i);
        const long long j = ra_sample(c, i);
        if (q < 0 || q >= ch || j < 0 || j >= n || (long long)q * n + j != i || i != at++) { fprintf(stderr, "index %lld -> channel %d sample %lld\n", i, q, j); return 3; }
        const float* base = x + (long long)q * n;
        const bool want = n >= kRaMinRun;
        if (ra_in_run(base, n, j, 1.0f) != want) { fprintf(stderr, "%d x %lld: sample %lld of channel %d\n", ch, n, j, q); return 3; }
        for (long long d = -2; d <= 2; d++) reads += ra_hot_at(base, n, j + d, 1.0f) ? 1 : 0;
    }
    for (int k = 0; k < kRdBins; k++) p[k] = (float)k;
    int last = -1;
    for (int k = 0; k < kRaMeans; k++) {                              // the frame launch: the windows of a row
        float s = 0.0f;
        for (int d = 0; d < kRaMeanBins; d++) { s += p[k + d]; last = k + d; }
        w[k] = s;
    }
    if (kRaBand0 < 0 || kRaBand1 >= kRdBins || kRaMeans > kRaWStride) return 3;
    printf("%d %lld %lld %d\n", ch, n, reads, last);
    free(x); free(p); free(w);
    return 0;
}

static int tiles(long long F) {
    unsigned char* cover = (unsigned char*)calloc((size_t)F, 1);
    if (!cover) return 2;
    const int nt = ra_tiles((int)F);
    for (int t = 0; t < nt; t++) {
        const int rows = ra_tile_rows((int)F, t);
        if (rows < 1 || rows > kRaTile) { fprintf(stderr, "F = %lld: tile %d has %d rows\n", F, t, rows); return 3; }
        for (int r = 0; r < rows; r++) cover[(size_t)t * kRaTile + r]++;  // the frame launch: row f0 + r of the clip
    }
    for (long long f = 0; f < F; f++)
        if (cover[f] != 1) { fprintf(stderr, "F = %lld: frame %lld lies in %d tiles\n", F, f, cover[f]); return 3; }
    printf("%lld %d %d\n", F, nt, ra_tile_rows((int)F, nt - 1));
    free(cover);
    return 0;
}

static int table() {
    const int32_t ch[3] = {2, 1, 8}, len[3] = {1000, 1, 5};
    const int64_t off[3] = {5000, 0, 100};
    std::vector<RaClip> h;
    int bad = 0;
    if (ra_layout(3, off, ch, len, h, &bad) != RA_OK) return 3;
    std::vector<RdClip> hd(3);
    hd[0].F = 1; hd[1].F = 16; hd[2].F = 17;
    const long long nt = ra_tile_layout(hd, h);
    printf("ok %lld", nt);
    for (const RaClip& c : h) printf(" %lld:%lld:%d:%lld:%d", c.off, c.n, c.ch, ra_total(c), c.tile0);
    printf("\n");
    struct { int32_t n; int64_t off[3]; int32_t ch[3]; int32_t len[3]; bool null; } bad_calls[] = {
        {0, {0, 0, 0}, {1, 1, 1}, {1, 1, 1}, false},            // no clips
        {kRaMaxClips + 1, {0, 0, 0}, {1, 1, 1}, {1, 1, 1}, false},   // too many (refused before the tables are read)
        {1, {0, 0, 0}, {1, 1, 1}, {1, 1, 1}, true},             // null tables
        {2, {0, 10, 0}, {1, 0, 1}, {5, 5, 1}, false},           // no channel
        {2, {0, 10, 0}, {1, 9, 1}, {5, 5, 1}, false},           // nine channels
        {2, {0, 10, 0}, {1, 1, 1}, {5, 0, 1}, false},           // an empty clip
        {1, {0, 0, 0}, {8, 1, 1}, {2147483647 / 8 + 1, 1, 1}, false},   // more than 2^31 - 1 samples in a clip
        {2, {0, -1, 0}, {1, 1, 1}, {5, 5, 1}, false},           // a negative offset
        {2, {0, 9, 0}, {2, 1, 1}, {5, 5, 1}, false},            // the second channel of clip 0 reaches into clip 1
        {3, {100, 20, 20}, {1, 1, 1}, {10, 5, 1}, false},       // a shared start
        {2, {0, 10, 0}, {2, 1, 1}, {5, 5, 1}, false},           // adjacent: passes
    };
    for (const auto& b : bad_calls) printf("%d ", ra_layout(b.n, b.null ? nullptr : b.off, b.ch, b.len, h, &bad));
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%.17g %.17g %d %d %d %.17g %.17g %.17g %d %d %d %d %d %d %d\n", (double)kRaHot, (double)kRaMinPeak, kRaMinRun, kRaBand0, kRaBand1, kRaFloorToMean,
               kRaSpeechFactor, kRaBandwidthRel, kRaMeanBins, kRaMeans, kRaWStride, kRaMaxChannels, kRaMaxClips, kRaRowWords, kRaTile);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "--table")) return table();
    if (argc >= 3 && !strcmp(argv[1], "--tiles")) {
        for (int a = 2; a < argc; a++) {
            const long long F = atoll(argv[a]);
            if (F < 1 || F > rd_frames(kRdMaxSamples)) { fprintf(stderr, "--tiles: refused\n"); return 2; }
            const int rc = tiles(F);
            if (rc) return rc;
        }
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "--runs")) {
        const int ch = atoi(argv[2]);
        const long long n = atoll(argv[3]);
        if (ch < 1 || ch > kRaMaxChannels || n < 1 || n > 1000000 || argc != 4 + ch * n) { fprintf(stderr, "--runs: CH N and CH * N values\n"); return 2; }
        return runs(ch, n, argv + 4);
    }
    if (argc == 4 && !strcmp(argv[1], "--walk")) {
        const int ch = atoi(argv[2]);
        const long long n = atoll(argv[3]);
        if (ch < 1 || ch > kRaMaxChannels || n < 1 || n > 10000000) { fprintf(stderr, "--walk: refused\n"); return 2; }
        return walk(ch, n);
    }
    fprintf(stderr, "usage: ref_assess_check --constants | --table | --runs CH N V... | --walk CH N | --tiles F...\n");
    return 2;
}
