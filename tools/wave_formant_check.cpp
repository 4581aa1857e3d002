// The three launches of csrc/wave_formant.h (wave_period_kernel, wave_marks_kernel, wave_psola_kernel) run serially on the CPU over
// csrc/wave_formant_core.h, the same text the kernels compile: tile staging and the frame sums, the lag rule, the mark chain with its peak
// search and the synthesis marks it hands out, the grain gather of an output tile and the 64-bit divide.  Built with
// -fsanitize=address,undefined, this is the evidence for the core's bounds: the samples, a tile's staged samples, the track, both mark lists
// (at the sizes the call reserves: fp_max_marks, fp_max_synth), a tile's grains and the output each live in a heap block of exactly their
// size, so a read or write past an end is a sanitizer report.  tests/test_formant_core.py builds and runs it.
//
//   wave_formant_check --constants   "hop window lag_min lag_max min_advance table min_step tile_frames span out_tile tile_grains"
//   wave_formant_check FILE...       FILE = little-endian int32 s, then s pitch steps, n, then n int16 samples.  Lines of a count and then
//                                    that many values: per FILE the frames' lags and their voiced flags; then per step the analysis
//                                    marks' positions, periods and voiced flags, the synthesis marks' positions and the marks they take,
//                                    and the samples of wave_codec.psola_pcm16
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../tts-indic-server-f5_amd/csrc/wave_prosody_core.h"
#include "../tts-indic-server-f5_amd/csrc/wave_formant_core.h"

static const unsigned short kWindow[kFpTable + 1] = {
#include "../tts-indic-server-f5_amd/csrc/psola_window.inc"
};

template <typename T>
static T* block(long long count) { return (T*)malloc(sizeof(T) * (size_t)count); }   // exactly `count`: the sanitizer guards both ends

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%d %d %d %d %d %d %d %d %d %d %d\n", kFpHop, kFpWin, kFpLagMin, kFpLagMax, kFpMinAdvance, kFpTable, kFpMinStep, kFpTileFrames, kFpSpan,
               kFpOutTile, kFpTileGrains);
        return 0;
    }
    if (argc < 2) { fprintf(stderr, "usage: wave_formant_check --constants | FILE...\n"); return 2; }
    for (int arg = 1; arg < argc; arg++) {
        FILE* f = fopen(argv[arg], "rb");
        if (!f) { perror(argv[arg]); return 2; }
        int32_t steps = 0, pitches[2 * kPrPitchMax], len = 0;
        if (fread(&steps, sizeof(int32_t), 1, f) != 1 || steps < 1 || steps > 2 * kPrPitchMax || fread(pitches, sizeof(int32_t), steps, f) != (size_t)steps ||
            fread(&len, sizeof(int32_t), 1, f) != 1) { fprintf(stderr, "%s: refused (header)\n", argv[arg]); return 2; }
        const long long n = len;
        bool ok = n >= 0;
        for (int s = 0; s < steps; s++) ok = ok && pitches[s] != 0 && pitches[s] >= -kPrPitchMax && pitches[s] <= kPrPitchMax;
        if (!ok) { fprintf(stderr, "%s: refused\n", argv[arg]); return 2; }
        short* x = block<short>(n);
        if ((n && fread(x, sizeof(short), n, f) != (size_t)n) || fgetc(f) != EOF) { fprintf(stderr, "%s: needs %lld samples\n", argv[arg], n); return 2; }
        fclose(f);
        // ---- wave_period_kernel: per tile the staged samples, per (frame, lag) a sum over the staged block, per frame the rule
        const long long F = fp_frames(n);
        int* track = block<int>(F);
        unsigned short* win = block<unsigned short>(kFpSpan);
        unsigned* d = block<unsigned>(kFpLags);
        for (long long tile = 0; tile < fp_period_tiles(n); tile++) {
            const long long f0 = tile * kFpTileFrames;
            for (int i = 0; i < kFpSpan; i++) win[i] = (unsigned short)fp_source(x, n, f0 * kFpHop + i);
            for (int fr = 0; fr < kFpTileFrames && f0 + fr < F; fr++) {
                const unsigned short* t = win + fr * kFpHop;
                unsigned E = 0;
                for (int i = 0; i < kFpWin; i++) E += t[i] > 0x8000 ? t[i] - 0x8000 : 0x8000 - t[i];
                for (int li = kFpLags - 1; li >= 0; li--) {                      // (any order: each sum stands alone)
                    const unsigned short* c = t + kFpLagMin + li;
                    unsigned s = 0;
                    for (int i = 0; i < kFpWin; i++) s += c[i] > t[i] ? c[i] - t[i] : t[i] - c[i];
                    d[li] = s;
                }
                track[f0 + fr] = fp_frame_entry(d, E);
            }
        }

        printf("%lld", F); for (long long i = 0; i < F; i++) printf(" %d", fp_entry_lag(track[i])); printf("\n");
        printf("%lld", F); for (long long i = 0; i < F; i++) printf(" %d", (int)fp_entry_voiced(track[i])); printf("\n");

        for (int step = 0; step < steps; step++) {
        int p, q;
        pr_pitch_ratio(pitches[step], &p, &q);
        // ---- wave_marks_kernel: the chain of analysis marks; the synthesis marks are handed out as the analysis marks arrive
        FpMark* marks = block<FpMark>(fp_max_marks(n));
        FpSynth* synth = block<FpSynth>(fp_max_synth(n));
        FpChain chain;
        memset(&chain, 0, sizeof(chain));
        chain.cur = -1;
        auto emit = [&](long long u, int i) { synth[chain.ns].u = (int)u; synth[chain.ns].i = i; };
        int na = 0;
        long long t = 0, a_prev = 0;
        bool chained = false;
        while (t < n) {
            const int e = track[t / kFpHop];
            long long a = t;
            int T = kFpHop;
            if (fp_entry_voiced(e)) {
                T = fp_entry_lag(e);
                long long b, end;
                fp_peak_range(t, T, chained, a_prev, n, &b, &end);
                unsigned long long best = 0;
                for (long long j = end - 1; j >= b; j--) {                         // (any order: the key decides)
                    const unsigned long long key = fp_peak_key(x[j], j);
                    if (key > best) best = key;
                }
                a = fp_peak_pos(best);
                chained = true;
            } else {
                chained = false;
            }
            const int packed = T | (chained ? 1 << 16 : 0);
            marks[na].a = (int)a; marks[na].T = packed;
            fp_chain_advance(chain, na, (int)a, packed, false, n, p, q, emit);
            na++;
            a_prev = a;
            t = a + T;
        }
        fp_chain_advance(chain, -1, 0, 0, true, n, p, q, emit);
        const int ns = chain.cur < 0 ? 0 : chain.ns;

        // ---- wave_psola_kernel: per output tile the marks that may touch it, as grains; per sample the gather and the divide
        short* y = block<short>(n);
        FpGrain* grains = block<FpGrain>(kFpTileGrains);
        for (long long tile = 0; tile < fp_out_tiles(n); tile++) {
            const long long j0 = tile * kFpOutTile, j1 = j0 + kFpOutTile < n ? j0 + kFpOutTile : n;
            int m0;
            const int ng = fp_tile_marks(synth, ns, j0, j1, &m0);
            for (int m = 0; m < ng; m++) {
                const FpMark mk = marks[synth[m0 + m].i];
                grains[m].u = synth[m0 + m].u; grains[m].a = mk.a; grains[m].T = mk.T & 0xffff;
            }
            for (long long j = j0; j < j1; j++) y[j] = (short)fp_output(x, n, j, grains, ng, kWindow);
        }

        printf("%d", na); for (int i = 0; i < na; i++) printf(" %d", marks[i].a); printf("\n");
        printf("%d", na); for (int i = 0; i < na; i++) printf(" %d", marks[i].T & 0xffff); printf("\n");
        printf("%d", na); for (int i = 0; i < na; i++) printf(" %d", (marks[i].T >> 16) & 1); printf("\n");
        printf("%d", ns); for (int i = 0; i < ns; i++) printf(" %d", synth[i].u); printf("\n");
        printf("%d", ns); for (int i = 0; i < ns; i++) printf(" %d", synth[i].i); printf("\n");
        printf("%lld", n); for (long long j = 0; j < n; j++) printf(" %d", (int)y[j]); printf("\n");
        free(marks); free(synth); free(y); free(grains);
        }
        free(x); free(track); free(win); free(d);
    }
    return 0;
}
