// The reference-clip pre-step on the device (F/infer/utils_infer.py:282-350 between reading the clip and writing the temporary WAV: clip
// at a pause, strip the silent edges, append 50 ms of silence) for n uploaded clips of one sample rate in ONE call: interleaved int16
// frames in, each clip's planar fp32 samples out, as f5hip_ref_frontend reads them.  Included at the end of f5hip.hip (same translation
// unit).  The definition is audio_prep.preprocess_ref_segment; the rule itself is ref_prestep_core.h, which a host program compiles too.
//
//   rp_cells_kernel    one thread per millisecond cell [frame(m), frame(m + 1)) of a clip: the exact int64 sum of squares of all its
//                      interleaved samples
//   rp_rule_kernel     one block per clip: the prefix sums over its cells; the silent flag of every window of BOTH parameter sets
//                      (S < (T + 1)^2 n); thread 0 walks them (rp_clip: ranges, the 6 s / 15 s stop, the choice of the set, the hard cut);
//                      the block looks for the first loud 10 ms window of the concatenation and the last loud millisecond of the trimmed
//                      rest, 256 windows at a time -- each a difference of prefix sums plus the partial cells at its ends, summed from the
//                      samples --; thread 0 runs the trailing subtraction and leaves the final ranges and the output length
//   rp_gather_kernel   one block per 1024 output frames: the kept ranges to planar fp32 (x / 32768, exact), the 50 ms tail of zeros, and
//                      the "any sample non-zero" flag.  A clip's planes start where the lengths of the clips before it end, so the output
//                      is packed as f5hip_ref_frontend takes it.
// THREE launches whatever n and whatever the clips hold.  A clip's result depends on that clip alone; no atomics on global memory (the two
// block-wide searches use an LDS min / max, whose result does not depend on the order).
#pragma once
#include "ragged_util.h"
#include "ref_prestep_core.h"

struct RpClip {
    long long in_off;      // its first interleaved sample in the input
    long long N;           // frames
    long long p_off;       // its L + 1 prefix sums
    long long f_off[2];    // its window flags, one table per parameter set
    int C, clip_short;
    int cell_block0;       // its first block of the cells launch (256 cells per block)
    int out_block0;        // its first block of the gather launch (kRpGatherTile output frames per block, over N + tail)
};

constexpr int kRpGatherTile = 1024;

struct RpSamples {         // the exact sum of squares over source frames [a, b) of one clip
    const short* x;
    int C;
    __host__ __device__ long long operator()(long long a, long long b) const {
        long long s = 0;
        for (long long i = a * C; i < b * C; i++) s += (long long)((int)x[i] * (int)x[i]);
        return s;
    }
};

__global__ __launch_bounds__(256) void rp_cells_kernel(const RpClip* __restrict__ clips, int n, int rate, const short* __restrict__ frames,
                                                       long long* __restrict__ P) {
    const int ci = last_at_or_before<&RpClip::cell_block0>(clips, n, (int)blockIdx.x);
    const RpClip c = clips[ci];
    const RpGeom g = rp_geom(c.N, c.C, rate);
    const long long m = (long long)(blockIdx.x - c.cell_block0) * 256 + threadIdx.x;
    if (m >= g.L) return;
    const RpSamples part{frames + c.in_off, c.C};
    P[c.p_off + 1 + m] = part(rp_frame(g, m), rp_frame(g, m + 1));
}

__global__ __launch_bounds__(256) void rp_rule_kernel(const RpClip* __restrict__ clips, int rate, const short* __restrict__ frames,
                                                      long long* __restrict__ Pall, uint8_t* __restrict__ flags_all, RpRanges* __restrict__ ranges,
                                                      int* __restrict__ info) {
    __shared__ long long runsum[256];
    __shared__ RpRanges rg;
    __shared__ RpEdges ed;
    __shared__ int found;
    const int tid = threadIdx.x, ci = blockIdx.x;
    const RpClip c = clips[ci];
    const RpGeom g = rp_geom(c.N, c.C, rate);
    long long* P = Pall + c.p_off;
    const RpSamples part{frames + c.in_off, c.C};

    // the cells P[1 .. L] become their inclusive prefix sums; a thread owns a run of them
    const long long run = (g.L + 255) / 256, i0 = min(tid * run, g.L), i1 = min(i0 + run, g.L);
    long long local = 0;
    for (long long i = i0; i < i1; i++) local += P[1 + i];
    runsum[tid] = local;
    __syncthreads();
    if (tid == 0) {
        long long acc = 0;
        for (int t = 0; t < 256; t++) { const long long v = runsum[t]; runsum[t] = acc; acc += v; }
        P[0] = 0;
    }
    __syncthreads();
    local = runsum[tid];
    for (long long i = i0; i < i1; i++) { local += P[1 + i]; P[1 + i] = local; }
    __syncthreads();

    // both parameter sets: the silent flag of every window
    uint8_t* fl[2] = {flags_all + c.f_off[0], flags_all + c.f_off[1]};
    if (c.clip_short) {
        for (int p = 0; p < 2; p++) {
            const int msl = rp_pass_ms(p);
            const long long nwin = rp_nwin(g.L, msl);
            for (long long w = tid; w < nwin; w += 256) fl[p][w] = rp_window_silent(g, P, rp_window_start(g.L, msl, w), msl, rp_pass_square(p)) ? 1 : 0;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const uint8_t* const cf[2] = {fl[0], fl[1]};
        rp_clip(g, cf, c.clip_short != 0, rg);
        found = 0x7fffffff;
    }
    __syncthreads();

    // the first loud 10 ms window of the concatenation
    const long long nlead = rp_lead_windows(rg, rate);
    for (long long base = 0; base < nlead; base += 256) {
        const long long i = base + tid;
        if (i < nlead && rp_lead_loud(g, P, part, rg, i)) atomicMin(&found, (int)i);
        __syncthreads();
        const int v = found;
        __syncthreads();
        if (v != 0x7fffffff) break;
    }
    if (tid == 0) {
        ed = rp_edges(g, rg, found != 0x7fffffff ? found : -1);
        found = -1;
    }
    __syncthreads();

    // the last loud millisecond of the trimmed rest
    for (long long top = ed.L2; top > 0; top -= 256) {
        const long long m = top - 1 - tid;
        if (m >= 0 && rp_trail_loud(g, P, part, rg, ed, m)) atomicMax(&found, (int)m);
        __syncthreads();
        const int v = found;
        __syncthreads();
        if (v >= 0) break;
    }
    if (tid == 0) {
        const long long body = rp_finish(g, rg, ed, found);
        ranges[ci] = rg;
        info[2 * ci] = rg.overflow ? -1 : (int)(body + rp_tail_frames(rate));
        info[2 * ci + 1] = 0;
    }
}

__global__ __launch_bounds__(256) void rp_gather_kernel(const RpClip* __restrict__ clips, int n, const short* __restrict__ frames,
                                                        const RpRanges* __restrict__ ranges, float* __restrict__ out, int* __restrict__ info) {
    __shared__ long long off_s;
    const int tid = threadIdx.x;
    const int ci = last_at_or_before<&RpClip::out_block0>(clips, n, (int)blockIdx.x);
    const RpClip c = clips[ci];
    const long long len = info[2 * ci];
    if (len <= 0) return;                                          // (uniform over the block)
    const long long j0 = (long long)(blockIdx.x - c.out_block0) * kRpGatherTile;
    if (j0 >= len) return;
    if (tid == 0) {
        long long off = 0;
        for (int j = 0; j < ci; j++) off += (long long)max(info[2 * j], 0) * clips[j].C;
        off_s = off;
    }
    __syncthreads();
    const RpRanges* rg = ranges + ci;
    const int nr = rg->nr;
    const long long body = rg->frames;
    const short* x = frames + c.in_off;
    float* o = out + off_s;
    int nz = 0;
    for (long long j = j0 + tid; j < min(j0 + kRpGatherTile, len); j += 256) {
        long long src = -1, at = 0;
        if (j < body)
            for (int i = 0; i < nr; i++) {
                const long long l = rg->b[i] - rg->a[i];
                if (j < at + l) { src = rg->a[i] + (j - at); break; }
                at += l;
            }
        for (int ch = 0; ch < c.C; ch++) {
            const int v = src >= 0 ? (int)x[src * c.C + ch] : 0;
            nz |= v;
            o[(long long)ch * len + j] = (float)v * (1.0f / 32768.0f);
        }
    }
    if (__syncthreads_or(nz) && tid == 0) info[2 * ci + 1] = 1;
}

struct RpWorkspace {
    RpClip* clips = nullptr; size_t cap_clips = 0;
    long long* P = nullptr; size_t cap_P = 0;
    uint8_t* flags = nullptr; size_t cap_flags = 0;
    RpRanges* ranges = nullptr; size_t cap_ranges = 0;
    HostStage stage;
    WorkspaceUse use;
};

int64_t f5hip_ref_prestep_bound(int32_t n, const int32_t* n_in, const int32_t* channels, int32_t rate) {
    if (n < 1 || !n_in || !channels || rate < kRpMinRate) return -1;
    long long total = 0;
    for (int i = 0; i < n; i++) {
        if (n_in[i] < 0 || channels[i] < 1) return -1;
        total += ((long long)n_in[i] + rp_tail_frames(rate)) * channels[i];
    }
    return total;
}

int f5hip_ref_prestep(int32_t n, const int32_t* n_in, const int32_t* channels, const uint8_t* clip_short, const int16_t* frames_dev, int64_t n_samples,
                      int32_t rate, float* out_dev, int32_t* info_dev, void* stream) {
    if (n < 1) return fail(-1, "ref_prestep: at least one clip (got %d)", n);
    if (!n_in || !channels || !clip_short || !out_dev || !info_dev) return fail(-1, "ref_prestep: bad argument");
    if (rate < kRpMinRate) return fail(-1, "ref_prestep: reference audio below %d Hz is not supported on this path (got %d)", kRpMinRate, rate);
    std::vector<RpClip> h(n);
    long long in_off = 0, p_off = 0, f_off = 0, cell_blocks = 0, out_blocks = 0, out_total = 0;
    const long long tail = rp_tail_frames(rate);
    for (int i = 0; i < n; i++) {
        if (n_in[i] < 0 || channels[i] < 1) return fail(-1, "ref_prestep: clip %d has %d frames in %d channels", i, n_in[i], channels[i]);
        if ((long long)rate * channels[i] >= kRpMaxWindowSamples)
            return fail(-1, "ref_prestep: clip %d: %d Hz x %d channels is more than the exact window sums allow", i, rate, channels[i]);
        RpClip& c = h[i];
        memset(&c, 0, sizeof(c));
        c.in_off = in_off; c.N = n_in[i]; c.C = channels[i]; c.clip_short = clip_short[i] ? 1 : 0;
        const long long L = rp_len_ms(c.N, rate);
        c.p_off = p_off; p_off += L + 1;
        for (int p = 0; p < 2; p++) { c.f_off[p] = f_off; f_off += rp_nwin(L, rp_pass_ms(p)); }
        c.cell_block0 = (int)cell_blocks; cell_blocks += (L + 255) / 256;
        c.out_block0 = (int)out_blocks; out_blocks += (c.N + tail + kRpGatherTile - 1) / kRpGatherTile;
        in_off += c.N * c.C;
        out_total += (c.N + tail) * c.C;
        if (in_off > 2147483647LL || out_total > 2147483647LL) return fail(-1, "ref_prestep: the clips of the call exceed 2^31 - 1 samples");
    }
    if (in_off != n_samples)
        return fail(-1, "ref_prestep: the frames need sum(n_in * channels) = %lld samples (got %lld)", in_off, (long long)n_samples);
    if (in_off > 0 && !frames_dev) return fail(-1, "ref_prestep: bad argument");
    RpWorkspace* const wsp = device_workspace<RpWorkspace>("ref_prestep");
    if (!wsp) return -6;
    RpWorkspace& ws = *wsp;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(dev_reserve(&ws.clips, &ws.cap_clips, (size_t)n, "ref_prestep clips"));
    CK(dev_reserve(&ws.P, &ws.cap_P, (size_t)p_off, "ref_prestep prefix sums"));
    CK(dev_reserve(&ws.flags, &ws.cap_flags, (size_t)std::max(f_off, 1LL), "ref_prestep window flags"));
    CK(dev_reserve(&ws.ranges, &ws.cap_ranges, (size_t)n, "ref_prestep ranges"));
    CK(ws.stage.upload(ws.clips, h.data(), sizeof(RpClip) * (size_t)n, st));   // pinned staging, queued on `stream`: no wait

    const short* x = (const short*)frames_dev;
    hipLaunchKernelGGL(rp_cells_kernel, dim3((unsigned)std::max(cell_blocks, 1LL)), dim3(256), 0, st, ws.clips, n, rate, x, ws.P);
    CKL("rp_cells");
    hipLaunchKernelGGL(rp_rule_kernel, dim3((unsigned)n), dim3(256), 0, st, ws.clips, rate, x, ws.P, ws.flags, ws.ranges, (int*)info_dev);
    CKL("rp_rule");
    hipLaunchKernelGGL(rp_gather_kernel, dim3((unsigned)out_blocks), dim3(256), 0, st, ws.clips, n, x, ws.ranges, out_dev, (int*)info_dev);
    CKL("rp_gather");
    g_counters[CNT_REF_PRESTEP_LAUNCHES] += 3;
    g_counters[CNT_REF_PRESTEP_CLIPS] += n;
    return 0;
}
