// Reference-audio front-end on the device: the prologue of infer_batch_process (F/infer/utils_infer.py:423-433) for n clips of one
// sample-rate pair in ONE call -- mono mix, rms, gain up to rms_floor, torchaudio-style polyphase sinc resampling -- as two launches with
// no host sync between them.  Included at the end of f5hip.hip (same translation unit).  Memory- and launch-bound: no MFMA here.
//
//   ref_reduce_kernel     one block per 4096-sample chunk of a clip: mono mean, sum of squares in fp64 -> one partial per block in a fixed
//                         slot; a few more blocks find each phase's non-zero tap range [first, last) from the table itself
//   ref_resample_kernel   one block per tile of `tq` polyphase blocks (q) of a clip: sums the clip's partials in a fixed order (the order
//                         depends on the clip's length alone), takes the rms < rms_floor branch, stages the gained mono window and -- when
//                         it fits -- the tap table in LDS, then one thread per output sums taps[p][k] * xpad[q * of + k], k ascending, fp32 FMA
//                         (table: 16-byte loads; samples: coalesced 4-byte loads, a channel plane starts at any sample of the packed buffer)
// A clip's bits depend on nothing but the clip: no atomics, every reduction tree is a function of the clip's length, and the zero padding
// is an index predicate against the clip's own [0, n_in) (never a read of the neighbour in the packed buffer).
#pragma once
#include "ragged_util.h"

struct RefClip {
    long long in_off;   // first float of the clip in wave_dev (channel c at in_off + c * n_in)
    int n_in, ch;
    int out_off, n_out;
    int part0, nparts;  // its slots of the partial array
    int tile0, ntiles;  // its blocks of the resample launch
};

constexpr int kRefChunk = 4096;               // samples per partial (16 per thread)
constexpr int kRefTileOutputs = 2048;         // outputs a resample block aims for ...
constexpr int kRefTileOutputsMax = 8192;      // ... or, with the table in LDS, half as many as the table has taps, up to this: every block copies the
                                              // whole table (zeros included), so a block that stages 26 K taps for 2 K outputs moves mostly table
constexpr int kRefRedBytes = 256 * 8;         // the fp64 reduction scratch in front of the dynamic LDS

// mono sample i of a clip: the mean over its channel planes, summed in fp64 in channel order and rounded to fp32 once (one channel: the
// sample itself, bit for bit).  An fp32 sum would lose to cancellation between the channels what no bound in |mono| covers.
F5_DEVICE float ref_mono(const float* __restrict__ x, int n_in, int ch, int i) {
    if (ch == 1) return x[i];
    double s = (double)x[i];
    for (int c = 1; c < ch; c++) s += (double)x[(size_t)c * n_in + i];
    return (float)(s / (double)ch);
}

__global__ __launch_bounds__(256) void ref_reduce_kernel(const RefClip* __restrict__ clips, int n, int total_parts, const float* __restrict__ wave,
                                                         double* __restrict__ partials, const float* __restrict__ taps, int nf, int L,
                                                         int2* __restrict__ range) {
    __shared__ double red[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (b >= total_parts) {   // tap ranges: phase p's first non-zero tap and one past its last (an all-zero phase: [0, 0))
        const int p = (b - total_parts) * 256 + tid;
        if (p >= nf) return;
        const float* t = taps + (size_t)p * L;
        int first = L, last = 0;
        for (int k = 0; k < L; k++)
            if (t[k] != 0.0f) { if (first == L) first = k; last = k + 1; }
        range[p] = last ? make_int2(first, last) : make_int2(0, 0);
        return;
    }
    const RefClip c = clips[last_at_or_before<&RefClip::part0>(clips, n, b)];
    const float* x = wave + c.in_off;
    const long long i0 = (long long)(b - c.part0) * kRefChunk;   // (64-bit: the last chunk of a clip near 2^31 samples ends past INT_MAX)
    double acc = 0.0;
#pragma unroll 4
    for (int j = 0; j < kRefChunk / 256; j++) {
        const long long i = i0 + j * 256 + tid;
        if (i < c.n_in) {
            const double m = (double)ref_mono(x, c.n_in, c.ch, (int)i);
            acc += m * m;
        }
    }
    const double total = block_sum(red, tid, acc);
    if (tid == 0) partials[b] = total;
}

// MODE 0: tap table staged in LDS; 1: tap table read through L2; 2: orig_freq == new_freq (no taps: out = the gained mono clip)
template <int MODE>
__global__ __launch_bounds__(256) void ref_resample_kernel(const RefClip* __restrict__ clips, int n, const float* __restrict__ wave,
                                                           const double* __restrict__ partials, const float* __restrict__ taps,
                                                           const int2* __restrict__ range, int of, int nf, int width, int L, int tq,
                                                           float rms_floor, float* __restrict__ out, float* __restrict__ rms_out) {
    extern __shared__ __attribute__((aligned(16))) char ref_sm[];
    double* red = reinterpret_cast<double*>(ref_sm);
    float* xs = reinterpret_cast<float*>(ref_sm + kRefRedBytes);
    const int tid = threadIdx.x;
    const int ci = last_at_or_before<&RefClip::tile0>(clips, n, (int)blockIdx.x);
    const RefClip c = clips[ci];
    const int tile = blockIdx.x - c.tile0;
    const int nx = tq * of + 2 * width;            // the window of xpad this tile reads: xpad[q0 * of .. q0 * of + nx)
    float* tp = xs + ((nx + 3) & ~3);              // (16-byte aligned: the table is staged with 16-byte stores)

    // the clip's rms: its partials in slot order, thread t taking slots t, t + 256, ..., then the fixed tree
    double acc = 0.0;
    for (int i = tid; i < c.nparts; i += 256) acc += partials[c.part0 + i];
    const double sumsq = block_sum(red, tid, acc);
    const float rms = (float)sqrt(sumsq / (double)c.n_in);
    if (tile == 0 && tid == 0) rms_out[ci] = rms;
    const bool gain = rms < rms_floor;

    const float* x = wave + c.in_off;
    const int q0 = tile * tq;
    const long long src0 = (long long)q0 * of - width;
    for (int i = tid; i < nx; i += 256) {
        const long long src = src0 + i;
        float v = 0.0f;
        if (src >= 0 && src < c.n_in) {
            v = ref_mono(x, c.n_in, c.ch, (int)src);
            if (gain) v = (v * rms_floor) / rms;
        }
        xs[i] = v;
    }
    if (MODE == 0) stage_taps(tp, taps, nf * L, tid);
    __syncthreads();

    const int n_local = tq * nf;
    for (int jl = tid; jl < n_local; jl += 256) {
        const int ql = jl / nf, p = jl - ql * nf;
        const long long j = (long long)(q0 + ql) * nf + p;
        if (j >= c.n_out) break;                   // (j grows with jl)
        float y;
        if (MODE == 2) {
            y = xs[ql];
        } else {
            const int2 r = range[p];
            const float* t = (MODE == 0 ? tp : taps) + (size_t)p * L;
            const float* xq = xs + ql * of;
            y = 0.0f;
            for (int k = r.x; k < r.y; k++) y = fmaf(t[k], xq[k], y);
        }
        out[(size_t)c.out_off + j] = y;
    }
}

struct RefWorkspace {
    RefClip* clips = nullptr; size_t cap_clips = 0;
    double* partials = nullptr; size_t cap_parts = 0;
    int2* range = nullptr; size_t cap_range = 0;
    WorkspaceUse use;
};
int f5hip_ref_frontend(int32_t n, const int32_t* n_in, const int32_t* channels, const float* wave_dev, int32_t orig_freq, int32_t new_freq,
                       const float* taps_dev, float rms_floor, float* out_dev, float* rms_dev, void* stream) {
    if (n < 1 || !n_in || !channels || !wave_dev || !out_dev || !rms_dev) return fail(-1, "ref_frontend: bad argument");
    if (orig_freq < 1 || new_freq < 1) return fail(-1, "ref_frontend: sample rates must be positive (%d -> %d)", orig_freq, new_freq);
    const bool identity = orig_freq == new_freq;
    if (!identity && !taps_dev) return fail(-1, "ref_frontend: %d -> %d Hz needs the tap table", orig_freq, new_freq);
    const RatePair rp = rate_pair(orig_freq, new_freq);
    const int of = rp.of, nf = rp.nf, width = rp.width, L = rp.L;
    // Tile: a block owns tq polyphase blocks.  With the table in LDS the tile grows with the table (2 staged taps per output at most), while
    // window + table fit the CU's LDS; else the small tile, with the table in LDS if that fits, else read through L2.  An output's bits do
    // not depend on the tile: one thread adds its terms in k order whatever block it runs in.
    const long long table = (long long)nf * L;
    auto window = [&](int q) { return (((long long)q * of + 2 * width) + 3) & ~3LL; };
    auto fits = [&](int q, bool with_table) { return kRefRedBytes + 4 * (window(q) + (with_table ? table : 0)) <= kLdsMax; };
    int tq = std::max(1, kRefTileOutputs / nf);
    if (table > (1LL << 28) || !fits(tq, false)) return fail(-1, "ref_frontend: %d -> %d Hz is not supported (%d : %d)", orig_freq, new_freq, of, nf);
    bool taps_lds = !identity && fits(tq, true);
    if (taps_lds) {
        const int big = (int)(std::min<long long>(std::max<long long>(table / 2, kRefTileOutputs), kRefTileOutputsMax) / nf);
        if (big > tq && fits(big, true)) tq = big;
    }
    const int lds = kRefRedBytes + 4 * (int)(window(tq) + (taps_lds ? table : 0));
    std::vector<RefClip> h(n);
    long long in_off = 0, out_off = 0, parts = 0, tiles = 0;
    for (int i = 0; i < n; i++) {
        if (n_in[i] < 1 || channels[i] < 1) return fail(-1, "ref_frontend: clip %d has %d samples in %d channels", i, n_in[i], channels[i]);
        const long long n_out = ((long long)nf * n_in[i] + of - 1) / of;
        const long long nq = (n_out + nf - 1) / nf;
        RefClip& c = h[i];
        c.in_off = in_off; c.n_in = n_in[i]; c.ch = channels[i];
        c.out_off = (int)out_off; c.n_out = (int)n_out;
        c.part0 = (int)parts; c.nparts = (n_in[i] + kRefChunk - 1) / kRefChunk;
        c.tile0 = (int)tiles; c.ntiles = (int)((nq + tq - 1) / tq);
        in_off += (long long)n_in[i] * channels[i];
        out_off += n_out; parts += c.nparts; tiles += c.ntiles;
        if (out_off > 2147483647LL) return fail(-1, "ref_frontend: the outputs of the call exceed 2^31 - 1 samples");
    }
    const int range_blocks = identity ? 0 : (nf + 255) / 256;
    if (parts + range_blocks > 2147483647LL || tiles > 2147483647LL) return fail(-1, "ref_frontend: call too large");
    RefWorkspace* const wsp = device_workspace<RefWorkspace>("ref_frontend");
    if (!wsp) return -6;
    RefWorkspace& ws = *wsp;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(dev_reserve(&ws.clips, &ws.cap_clips, (size_t)n, "ref_frontend clips"));
    CK(dev_reserve(&ws.partials, &ws.cap_parts, (size_t)parts, "ref_frontend partials"));
    CK(dev_reserve(&ws.range, &ws.cap_range, (size_t)nf, "ref_frontend tap ranges"));
    static unsigned lds_attr_done = 0;
    if (taps_lds && lds > 64 * 1024 && f5_set_lds_attr((const void*)ref_resample_kernel<0>, kLdsMax, lds_attr_done) != hipSuccess)
        return fail(-7, "ref_frontend: LDS opt-in");
    if (upload_sync(st, ws.clips, h) != hipSuccess) return fail(-6, "ref_frontend metadata upload");

    hipLaunchKernelGGL(ref_reduce_kernel, dim3((unsigned)(parts + range_blocks)), dim3(256), 0, st, ws.clips, n, (int)parts, wave_dev, ws.partials,
                       taps_dev, nf, L, ws.range);
    CKL("ref_reduce");
    g_counters[CNT_REF_LAUNCHES]++;
#define F5_REF_LAUNCH(MODE)                                                                                                                  \
    hipLaunchKernelGGL(ref_resample_kernel<MODE>, dim3((unsigned)tiles), dim3(256), lds, st, ws.clips, n, wave_dev, ws.partials, taps_dev, ws.range, \
                       of, nf, width, L, tq, rms_floor, out_dev, rms_dev)
    if (identity) F5_REF_LAUNCH(2);
    else if (taps_lds) F5_REF_LAUNCH(0);
    else F5_REF_LAUNCH(1);
#undef F5_REF_LAUNCH
    CKL("ref_resample");
    g_counters[CNT_REF_LAUNCHES]++;
    g_counters[taps_lds ? CNT_REF_TAPS_LDS : CNT_REF_TAPS_L2] += identity ? 0 : 1;
    return 0;
}
