// The formant-preserving pitch shift on the device: f5hip_wave_prosody_formants = f5hip_wave_prosody plus a per-request flag; a flagged
// request is stretched by its tempo alone (wave_out.h wave_wsola_kernel, into the workspace) and then pitch-shifted by time-domain
// pitch-synchronous overlap-add, bit for bit wave_codec.psola_pcm16.  Included at the end of f5hip.hip (same translation unit).  The
// definition is written down in wave_codec.py and include/f5hip.h; the geometry, the lag rule, the tie rules, the chain's steps and the blend
// are wave_formant_core.h, which a host program compiles too (tools/wave_formant_check.cpp, under sanitizers).
//
//   wave_period_kernel  one block per tile of 5 analysis frames of a flagged request.  The tile's 1360 samples go to LDS once, biased by 32768
//                       (the same absolute differences) and twice, the second copy one sample on, so that a lag that starts at an odd sample
//                       reads aligned 32-bit words too (wave_wsola_kernel's packed form).  The 5 x 354 sums -- 353 lags and E, which is the
//                       difference from the zero 0x8000 -- go across the 256 threads, 240 v_sad_u16 each, the frame's own samples as 16-byte
//                       reads.  Then a wavefront per frame: dmin and the first lag within E / 8 of it by two min-reductions (values, not
//                       lanes, decide), and one lane walks to the bottom of the dip.  Lag and flag per frame -> the workspace.
//   wave_marks_kernel   one wavefront per flagged request, the only serial part: the chain of analysis marks.  The track and the samples
//                       come through LDS in chunks (1024 frames, 4096 samples: the chain only moves forward), so a step is LDS reads and
//                       shuffles: the peak search (at most 400 samples at the start of a voiced run, at most 101 afterwards) across the
//                       lanes by a keyed maximum (sample, then the earlier position).  Synthesis marks are final as soon as the analysis
//                       mark after their candidate is known (fp_chain_advance), so the same loop hands them out from registers.  Both
//                       lists and their counts stay on the device.
//   wave_psola_kernel   one block per 2048 outputs.  Two binary searches give the synthesis marks within 400 samples of the tile (at most 87:
//                       steps are at least 33 samples); they go to LDS as grains (u, a, T) beside the master window.  A thread gathers 8
//                       consecutive outputs over the grains that cover each, does the 64-bit divide and stores 16 bytes.  No accumulator
//                       buffer and no atomics: nothing depends on an order.
// THREE launches whatever n, behind the WSOLA launch; no host sync; a request's bytes depend on that request alone.
#pragma once
#include "ragged_util.h"
#include "wave_formant_core.h"

constexpr int kFpWords = kFpSpan / 2;           // 680 words hold a tile's samples
constexpr int kFpOddBase = 736;                 // the odd copy's first word: 32 banks on from the even copy's (736 = 11 * 64 + 32)
constexpr int kFpSums = kFpLags + 1;            // a frame's 353 lags, then E
constexpr int kFpTrackChunk = 1024, kFpSampleChunk = 4096;
static_assert(kFpOddBase >= kFpWords && kFpOddBase % 64 == 32 && (kFpHop / 2) % 4 == 0 && kFpPeakMax <= kFpSampleChunk && kFpOutTile == 8 * 256 &&
              kFpTileGrains <= 256, "wave_formant tiling");
__device__ const unsigned short kFpWindowTable[kFpTable + 1] = {
#include "psola_window.inc"
};

struct FpReq {
    long long mid_off;   // its stretched samples in the prosody workspace (where wave_wsola_kernel left them)
    long long out_off;   // its first output sample (a multiple of 8: 16-byte stores)
    int cap, req;        // the bound of its input length; its index in the call: len_dev
    int P, Q;            // its WSOLA stretch: the samples here are pr_geom(len, P, Q).m
    int p, q;            // its pitch ratio
    int ptile0;          // its first block of the period launch
    int frame0;          // its first entry of the track
    int mark0, synth0;   // its first analysis / synthesis mark
    int otile0;          // its first block of the overlap-add launch
    int pad_;
};

F5_DEVICE int fp_len(const int* len_dev, const FpReq& r) {
    const int len = len_dev ? min(max(len_dev[r.req], 0), r.cap) : r.cap;
    return (int)pr_geom(len, r.P, r.Q).m;
}

__global__ __launch_bounds__(256) void wave_period_kernel(const FpReq* __restrict__ reqs, int nf, const short* __restrict__ mid,
                                                          const int* __restrict__ len_dev, int* __restrict__ track) {
    __shared__ __attribute__((aligned(16))) unsigned wn[kFpOddBase + kFpWords];    // the tile's samples: even copy, then the odd copy
    __shared__ unsigned d[kFpTileFrames][kFpSums];
    const int tid = threadIdx.x;
    const FpReq r = reqs[last_at_or_before<&FpReq::ptile0>(reqs, nf, (int)blockIdx.x)];
    const int n = fp_len(len_dev, r);
    const long long F = fp_frames(n), f0 = (long long)((int)blockIdx.x - r.ptile0) * kFpTileFrames;
    if (f0 >= F) return;                                                // a tile past the request's actual length (the same for the whole block)
    const short* x = mid + r.mid_off;
    unsigned short* const ev16 = reinterpret_cast<unsigned short*>(wn);
    unsigned short* const od16 = reinterpret_cast<unsigned short*>(wn + kFpOddBase);
    for (int i = tid; i < kFpSpan; i += 256) {
        const unsigned short v = (unsigned short)fp_source(x, n, f0 * kFpHop + i);
        ev16[i] = v;
        if (i > 0) od16[i - 1] = v;
    }
    if (tid == 0) od16[kFpSpan - 1] = 0x8000;                           // (the sample behind the tile: never part of a sum)
    __syncthreads();

    for (int it = tid; it < kFpTileFrames * kFpSums; it += 256) {
        const int fr = it / kFpSums, li = it - fr * kFpSums;
        if (f0 + fr >= F) break;
        const uint4* t4 = reinterpret_cast<const uint4*>(wn + fr * (kFpHop / 2));   // the frame's own samples: 240 bytes a frame, 16-byte aligned
        unsigned acc = 0;
        if (li == kFpLags) {                                            // E: the differences from zero
#pragma unroll 4
            for (int w = 0; w < kFpWin / 8; w++) {
                const uint4 tv = t4[w];
                acc = __builtin_amdgcn_sad_u16(tv.x, 0x80008000u, acc); acc = __builtin_amdgcn_sad_u16(tv.y, 0x80008000u, acc);
                acc = __builtin_amdgcn_sad_u16(tv.z, 0x80008000u, acc); acc = __builtin_amdgcn_sad_u16(tv.w, 0x80008000u, acc);
            }
        } else {
            const int s = fr * kFpHop + kFpLagMin + li;                 // the lagged frame's first sample in the tile: at most 880
            const unsigned* const b = wn + ((s & 1) ? kFpOddBase : 0) + (s >> 1);
#pragma unroll 4
            for (int w = 0; w < kFpWin / 8; w++) {
                const uint4 tv = t4[w];
                acc = __builtin_amdgcn_sad_u16(b[4 * w], tv.x, acc); acc = __builtin_amdgcn_sad_u16(b[4 * w + 1], tv.y, acc);
                acc = __builtin_amdgcn_sad_u16(b[4 * w + 2], tv.z, acc); acc = __builtin_amdgcn_sad_u16(b[4 * w + 3], tv.w, acc);
            }
        }
        d[fr][li] = acc;
    }
    __syncthreads();

    const int lane = tid & 63;
    for (int fr = tid >> 6; fr < kFpTileFrames && f0 + fr < F; fr += 4) {   // a wavefront per frame
        const unsigned* const df = d[fr];
        const unsigned E = df[kFpLags];
        unsigned dmin = 0xffffffffu;
        for (int li = lane; li < kFpLags; li += 64) dmin = min(dmin, df[li]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dmin = min(dmin, (unsigned)__shfl_xor((int)dmin, o));
        int first = kFpLags - 1;
        for (int li = lane; li < kFpLags; li += 64)
            if (fp_lag_ok(df[li], dmin, E)) { first = min(first, li); break; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
        if (lane == 0) {
            const int li = fp_lag_walk(df, first);
            track[r.frame0 + f0 + fr] = fp_track_entry(li + kFpLagMin, fp_voiced(df[li], E));
        }
    }
}

__global__ __launch_bounds__(64) void wave_marks_kernel(const FpReq* __restrict__ reqs, const short* __restrict__ mid, const int* __restrict__ len_dev,
                                                        const int* __restrict__ track, FpMark* __restrict__ marks, FpSynth* __restrict__ synth,
                                                        int* __restrict__ counts) {
    __shared__ int tr[kFpTrackChunk];
    __shared__ short sm[kFpSampleChunk];
    const int lane = threadIdx.x;
    const FpReq r = reqs[blockIdx.x];
    const long long n = fp_len(len_dev, r), F = fp_frames(n);
    const short* x = mid + r.mid_off;
    const int* trk = track + r.frame0;
    FpMark* mk = marks + r.mark0;
    FpSynth* sy = synth + r.synth0;
    long long tbase = -kFpTrackChunk, sbase = -kFpSampleChunk;          // nothing staged yet
    FpChain chain;
    chain.u = 0; chain.rem = 0; chain.cur = -1; chain.cur_a = 0; chain.cur_T = 0; chain.ns = 0;
    auto emit = [&](long long u, int i) {
        if (lane == 0) { sy[chain.ns].u = (int)u; sy[chain.ns].i = i; }
    };
    int na = 0;
    long long t = 0, a_prev = 0;
    bool chained = false;
    // every value that steers the loop is the same in all lanes: the block is one wavefront and each reduction ends in all of them
    while (t < n) {
        const long long f = t / kFpHop;
        if (f >= tbase + kFpTrackChunk) {
            __syncthreads();
            tbase = f;
            for (int i = lane; i < kFpTrackChunk; i += 64) tr[i] = tbase + i < F ? trk[tbase + i] : 0;
            __syncthreads();
        }
        const int e = tr[f - tbase];
        long long a = t;
        int T = kFpHop;
        if (fp_entry_voiced(e)) {
            T = fp_entry_lag(e);
            long long b, end;
            fp_peak_range(t, T, chained, a_prev, n, &b, &end);
            if (b < sbase || end > sbase + kFpSampleChunk) {
                __syncthreads();
                sbase = b;
                for (int i = lane; i < kFpSampleChunk; i += 64) sm[i] = sbase + i < n ? x[sbase + i] : (short)0;
                __syncthreads();
            }
            unsigned long long best = 0;
            for (long long j = b + lane; j < end; j += 64) best = max(best, fp_peak_key(sm[j - sbase], j));
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, o));
            a = fp_peak_pos(best);
            chained = true;
        } else {
            chained = false;
        }
        const int packed = T | (chained ? 1 << 16 : 0);
        if (lane == 0) { mk[na].a = (int)a; mk[na].T = packed; }
        fp_chain_advance(chain, na, (int)a, packed, false, n, r.p, r.q, emit);
        na++;
        a_prev = a;
        t = a + T;
    }
    fp_chain_advance(chain, -1, 0, 0, true, n, r.p, r.q, emit);
    if (lane == 0) {
        counts[2 * blockIdx.x] = na;
        counts[2 * blockIdx.x + 1] = chain.cur < 0 ? 0 : chain.ns;
    }
}

__global__ __launch_bounds__(256) void wave_psola_kernel(const FpReq* __restrict__ reqs, int nf, const short* __restrict__ mid,
                                                         const int* __restrict__ len_dev, const FpMark* __restrict__ marks,
                                                         const FpSynth* __restrict__ synth, const int* __restrict__ counts, short* __restrict__ out) {
    __shared__ FpGrain g[kFpTileGrains];
    __shared__ unsigned short M[kFpTable + 1];
    const int tid = threadIdx.x;
    const int f = last_at_or_before<&FpReq::otile0>(reqs, nf, (int)blockIdx.x);
    const FpReq r = reqs[f];
    const long long n = fp_len(len_dev, r);
    const long long j0 = (long long)((int)blockIdx.x - r.otile0) * kFpOutTile;
    if (j0 >= n) return;                                                // a tile past the request's actual length (the same for the whole block)
    const long long j1 = min(j0 + kFpOutTile, n);
    const FpSynth* sy = synth + r.synth0;
    const FpMark* mk = marks + r.mark0;
    int m0;
    const int ng = fp_tile_marks(sy, counts[2 * f + 1], j0, j1, &m0);
    for (int i = tid; i < kFpTable + 1; i += 256) M[i] = kFpWindowTable[i];
    if (tid < ng) {
        const FpSynth s = sy[m0 + tid];
        const FpMark k = mk[s.i];
        g[tid].u = s.u; g[tid].a = k.a; g[tid].T = k.T & 0xffff;
    }
    __syncthreads();
    const short* x = mid + r.mid_off;
    short* y = out + r.out_off;
    const long long j = j0 + 8 * tid;
    if (j >= j1) return;
    int v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = j + e < j1 ? fp_output(x, n, j + e, g, ng, M) : 0;
    if (j + 8 <= j1) {                                                  // (y + j is 16-byte aligned: the request's first sample and j are multiples of 8)
        *reinterpret_cast<int4*>(y + j) = make_int4((v[0] & 0xffff) | (v[1] << 16), (v[2] & 0xffff) | (v[3] << 16), (v[4] & 0xffff) | (v[5] << 16),
                                                    (v[6] & 0xffff) | (v[7] << 16));
    } else {
        for (int e = 0; e < 8 && j + e < j1; e++) y[j + e] = (short)v[e];
    }
}

struct FpWorkspace {
    FpReq* reqs = nullptr; size_t cap_reqs = 0;
    int* track = nullptr; size_t cap_track = 0;
    FpMark* marks = nullptr; size_t cap_marks = 0;
    FpSynth* synth = nullptr; size_t cap_synth = 0;
    int* counts = nullptr; size_t cap_counts = 0;
    WorkspaceUse use;
};

int f5hip_wave_prosody_formants_launches(void) { return 3; }

static int wave_formant_launches(const std::vector<PrKept>& kept, const short* mid, const int32_t* len_dev, int16_t* out_dev, void* stream);

int f5hip_wave_prosody_formants(int32_t n, const int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev,
                                const int32_t* stretch_p, const int32_t* stretch_q, const int32_t* pitch, const uint8_t* keep_formants,
                                const float* taps_dev, int16_t* out_dev, const int64_t* out_off, int32_t* out_len_dev, void* stream) {
    if (!keep_formants) return fail(-1, "wave_prosody: bad argument");
    std::vector<PrKept> kept;
    // (the three launches below read the stretched PCM of wave_prosody's workspace: they run inside its turn, and inside their own)
    return wave_prosody_run(n, pcm_dev, in_off, max_len, len_dev, stretch_p, stretch_q, pitch, keep_formants, taps_dev, out_dev, out_off, out_len_dev, &kept,
                            stream, [&](const short* mid) { return wave_formant_launches(kept, mid, len_dev, out_dev, stream); });
}

static int wave_formant_launches(const std::vector<PrKept>& kept, const short* mid, const int32_t* len_dev, int16_t* out_dev, void* stream) {
    if (kept.empty()) return 0;
    std::vector<FpReq> h;
    long long ptiles = 0, frames = 0, nmarks = 0, nsynth = 0, otiles = 0;
    for (const PrKept& k : kept) {
        const long long m = pr_geom(k.cap, k.P, k.Q).m;                 // the bound of its stretched length: every table below is sized by it
        FpReq r;
        memset(&r, 0, sizeof(r));
        r.mid_off = k.mid_off; r.out_off = k.out_off; r.cap = k.cap; r.req = k.req; r.P = k.P; r.Q = k.Q;
        pr_pitch_ratio(k.pitch, &r.p, &r.q);
        r.ptile0 = (int)ptiles; r.frame0 = (int)frames; r.mark0 = (int)nmarks; r.synth0 = (int)nsynth; r.otile0 = (int)otiles;
        h.push_back(r);
        ptiles += fp_period_tiles(m); frames += fp_frames(m); nmarks += fp_max_marks(m); nsynth += fp_max_synth(m); otiles += fp_out_tiles(m);
    }
    FpWorkspace* const wsp = device_workspace<FpWorkspace>("wave_prosody_formants");
    if (!wsp) return -6;
    FpWorkspace& ws = *wsp;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(dev_reserve(&ws.reqs, &ws.cap_reqs, h.size(), "wave_prosody_formants requests"));
    CK(dev_reserve(&ws.track, &ws.cap_track, (size_t)std::max<long long>(frames, 1), "wave_prosody_formants track"));
    CK(dev_reserve(&ws.marks, &ws.cap_marks, (size_t)std::max<long long>(nmarks, 1), "wave_prosody_formants analysis marks"));
    CK(dev_reserve(&ws.synth, &ws.cap_synth, (size_t)std::max<long long>(nsynth, 1), "wave_prosody_formants synthesis marks"));
    CK(dev_reserve(&ws.counts, &ws.cap_counts, 2 * h.size(), "wave_prosody_formants counts"));
    if (upload_sync(st, ws.reqs, h) != hipSuccess) return fail(-6, "wave_prosody_formants metadata upload");
    const int nf = (int)h.size();
    // (a call whose flagged requests are all empty keeps one block a launch: it finds its tile past the length and leaves)
    hipLaunchKernelGGL(wave_period_kernel, dim3((unsigned)std::max<long long>(ptiles, 1)), dim3(256), 0, st, ws.reqs, nf, mid, (const int*)len_dev, ws.track);
    CKL("wave_period");
    hipLaunchKernelGGL(wave_marks_kernel, dim3((unsigned)nf), dim3(64), 0, st, ws.reqs, mid, (const int*)len_dev, (const int*)ws.track, ws.marks, ws.synth,
                       ws.counts);
    CKL("wave_marks");
    hipLaunchKernelGGL(wave_psola_kernel, dim3((unsigned)std::max<long long>(otiles, 1)), dim3(256), 0, st, ws.reqs, nf, mid, (const int*)len_dev,
                       (const FpMark*)ws.marks, (const FpSynth*)ws.synth, (const int*)ws.counts, (short*)out_dev);
    CKL("wave_psola");
    g_counters[CNT_WAVE_FORMANT_LAUNCHES] += 3;
    g_counters[CNT_WAVE_FORMANT_REQUESTS] += nf;
    return 0;
}
