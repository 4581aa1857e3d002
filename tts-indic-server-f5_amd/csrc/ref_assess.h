// The reference-clip report on the device: is an uploaded clip fit to clone from?  The measures of n clips of their own lengths in ONE call,
// on the two buffers a front-end call already holds: its packed raw upload (clip i: ch_i channels of n_i samples, channel after channel) and
// f5hip_ref_frontend's packed 24 kHz output.  Included at the end of f5hip.hip (same translation unit).  The definition is
// audio_prep.assess_reference; the geometry and the run rule are ref_assess_core.h, which a host program compiles too.
//
//   ra_peak_kernel     grid (64, n): the clip's samples strided over 64 blocks; the maximum of the bit patterns of |x| (non-negative floats
//                      order like integers) per block in LDS, then ONE integer atomicMax per block on the clip's cell: exact, order-free
//   ra_runs_kernel     grid (64, n): one thread per sample and turn decides from its own sample and the two on each side, inside its
//                      channel's bounds (ra_in_run); the block's count is an integer sum in LDS and ONE 64-bit atomic add on the clip's cell.
//                      A clip whose peak is below 0.25 is skipped: its count stays 0
//   rd_stft_kernel     ref_denoise.h's, as it stands: P [rows][516] of the prepared clips' frames
//   rd_floor_kernel    ref_denoise.h's, as it stands: floor[k] = the r-th smallest of the clip's P[.][k], exactly
//   ra_frame_kernel    one block per tile of 16 frame rows of one clip, staged in LDS: E[row] = sum_{k in B} P in fp64 per row (a wave per row, a
//                      fixed tree over the row alone), and per window k the rows' 8-bin means added in ascending row order in fp64 ->
//                      T [tiles][508].  (One block per row and one per-clip block that adds 506 columns over every row was measured first: the
//                      per-clip block then reads the clip's whole spectrum through one CU, 0.46 ms for a 15 s clip; through the tiles 1/16 of it)
//   ra_clip_kernel     one block per clip: m[k] = the clip's tiles added in ascending tile order in fp64, / F; N from the floor (ascending k) and
//                      S from E (ascending f), each by one thread in fp64; the speech frames and k* as integer reductions; the row
// SIX launches whatever n (f5hip_ref_assess_launches), behind one memset of the n accumulator cells.  A clip's row depends on that clip alone:
// the two atomics are integer, no float is added across clips or in an order that depends on the batch, so a clip's row is bit-identical
// alone and in any batch.  Nothing is written but the rows and the workspace.
#pragma once
#include "ragged_util.h"
#include "ref_assess_core.h"
#include "ref_denoise.h"

constexpr int kRaRawBlocks = 64;               // blocks per clip of the two raw-side launches
constexpr int kRaBatch = 8;                    // tiles (or frames) whose values the per-clip launch loads before it adds them

struct RaAcc {
    unsigned long long in_runs;                // samples in runs of at least three hot samples
    unsigned peak_bits;                        // the bit pattern of max |x|
    unsigned pad_;
};

__global__ __launch_bounds__(256) void ra_peak_kernel(const RaClip* __restrict__ clips, const float* __restrict__ raw, RaAcc* __restrict__ acc) {
    __shared__ unsigned red[256];
    const int tid = threadIdx.x;
    const RaClip c = clips[blockIdx.y];
    const long long total = ra_total(c);
    if ((long long)blockIdx.x * 256 >= total) return;                    // (the same for the whole block)
    const unsigned* x = reinterpret_cast<const unsigned*>(raw + c.off);
    unsigned best = 0;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < total; i += (long long)kRaRawBlocks * 256) best = max(best, x[i] & 0x7fffffffu);
    red[tid] = best;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = max(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0 && red[0]) atomicMax(&acc[blockIdx.y].peak_bits, red[0]);
}

__global__ __launch_bounds__(256) void ra_runs_kernel(const RaClip* __restrict__ clips, const float* __restrict__ raw, RaAcc* __restrict__ acc) {
    __shared__ int red[256];
    const int tid = threadIdx.x;
    const RaClip c = clips[blockIdx.y];
    const long long total = ra_total(c);
    const float peak = __uint_as_float(acc[blockIdx.y].peak_bits);
    if ((long long)blockIdx.x * 256 >= total || peak < kRaMinPeak) return;   // (the same for the whole block)
    const float thr = ra_threshold(peak);
    const float* x = raw + c.off;
    int count = 0;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < total; i += (long long)kRaRawBlocks * 256)
        count += ra_in_run(x + (long long)ra_channel(c, i) * c.n, c.n, ra_sample(c, i), thr) ? 1 : 0;
    const int sum = block_sum(red, tid, count);
    if (tid == 0 && sum) atomicAdd(&acc[blockIdx.y].in_runs, (unsigned long long)sum);
}

__global__ __launch_bounds__(256) void ra_frame_kernel(const RdClip* __restrict__ clips, const RaClip* __restrict__ raws, int n, const float* __restrict__ P,
                                                       double* __restrict__ E, double* __restrict__ T) {
    __shared__ float p[kRaTile][kRdPStride];
    const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ci = last_at_or_before<&RaClip::tile0>(raws, n, tile);
    const RdClip c = clips[ci];
    const int f0 = (tile - raws[ci].tile0) * kRaTile, rows = ra_tile_rows(c.F, tile - raws[ci].tile0);
    const float* Pt = P + (size_t)(c.row0 + f0) * kRdPStride;
    for (int r = 0; r < rows; r++)
        for (int k = tid; k < kRdBins; k += 256) p[r][k] = Pt[(size_t)r * kRdPStride + k];
    __syncthreads();
    for (int r = wv; r < rows; r += 4) {                                 // a wave per row: the band sum by a fixed tree over the row alone
        double v = 0.0;
        for (int k = kRaBand0 + lane; k <= kRaBand1; k += 64) v += (double)p[r][k];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
        if (lane == 0) E[c.row0 + f0 + r] = v;
    }
    for (int k = tid; k < kRaMeans; k += 256) {                          // a thread per window: each row's 8-bin mean, the rows in ascending order
        double a = 0.0;
        for (int r = 0; r < rows; r++) {
            float s = 0.0f;
#pragma unroll
            for (int d = 0; d < kRaMeanBins; d++) s += p[r][k + d];
            a += (double)(s * (1.0f / kRaMeanBins));
        }
        T[(size_t)tile * kRaWStride + k] = a;
    }
}

__global__ __launch_bounds__(256) void ra_clip_kernel(const RdClip* __restrict__ clips, const RaClip* __restrict__ raws, const RaAcc* __restrict__ acc,
                                                      const float* __restrict__ floor_, const double* __restrict__ E, const double* __restrict__ T,
                                                      long long* __restrict__ rows) {
    __shared__ double m[kRaMeans];
    __shared__ double red[256];
    __shared__ int redi[256];
    __shared__ double ns[2];
    const int ci = blockIdx.x, tid = threadIdx.x;
    const RdClip c = clips[ci];
    const double* Ec = E + c.row0;
    {   // the thread's two windows, kRaBatch tiles at a time: the batch's loads are in flight together, then added in ascending tile order
        const double* col = T + (size_t)raws[ci].tile0 * kRaWStride + tid;
        const int nt = ra_tiles(c.F);
        const bool two = tid + 256 < kRaMeans;
        double a0 = 0.0, a1 = 0.0;
        for (int t0 = 0; t0 < nt; t0 += kRaBatch) {
            double v0[kRaBatch], v1[kRaBatch];
#pragma unroll
            for (int j = 0; j < kRaBatch; j++) {                         // (a tile past the clip's last adds +0.0: the sums are of non-negative values)
                const bool in = t0 + j < nt;
                v0[j] = in ? col[(size_t)(t0 + j) * kRaWStride] : 0.0;
                v1[j] = in && two ? col[(size_t)(t0 + j) * kRaWStride + 256] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < kRaBatch; j++) { a0 += v0[j]; a1 += v1[j]; }
        }
        m[tid] = a0 / (double)c.F;
        if (two) m[tid + 256] = a1 / (double)c.F;
    }
    if (tid == 255) {                                                    // (one of the threads with a single window)
        double a = 0.0;
        for (int k = kRaBand0; k <= kRaBand1; k++) a += (double)floor_[(size_t)ci * kRdPStride + k];
        ns[0] = kRaFloorToMean * a;
        a = 0.0;
        for (int f0 = 0; f0 < c.F; f0 += kRaBatch) {
            double v[kRaBatch];
#pragma unroll
            for (int j = 0; j < kRaBatch; j++) v[j] = f0 + j < c.F ? Ec[f0 + j] : 0.0;
#pragma unroll
            for (int j = 0; j < kRaBatch; j++) a += v[j];
        }
        ns[1] = a / (double)c.F;
    }
    __syncthreads();
    const double N = ns[0], S = ns[1];
    int speech = 0;
    for (int f = tid; f < c.F; f += 256) speech += (Ec[f] >= kRaSpeechFactor * N && Ec[f] > 0.0) ? 1 : 0;
    speech = block_sum(redi, tid, speech);
    double top = 0.0;
    for (int k = tid; k < kRaMeans; k += 256) top = fmax(top, m[k]);
    red[tid] = top;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    top = red[0];
    int k_star = -1;
    if (top > 0.0)
        for (int k = tid; k < kRaMeans; k += 256)
            if (m[k] >= kRaBandwidthRel * top) k_star = k;                // (ascending k: the thread's largest)
    redi[tid] = k_star;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) redi[tid] = max(redi[tid], redi[tid + s]);
        __syncthreads();
    }
    if (tid == 0) {
        k_star = redi[0];
        const float peak = __uint_as_float(acc[ci].peak_bits);
        const double inf = __longlong_as_double(0x7ff0000000000000LL);
        long long* row = rows + (size_t)ci * kRaRowWords;
        row[RA_CLIPPED] = ra_clipped((long long)acc[ci].in_runs, peak, ra_total(raws[ci]));
        row[RA_PEAK_BITS] = (long long)acc[ci].peak_bits;
        row[RA_SPEECH_FRAMES] = speech;
        row[RA_K_STAR] = k_star;
        row[RA_N] = __double_as_longlong(N);
        row[RA_S] = __double_as_longlong(S);
        row[RA_NOISE_DB] = __double_as_longlong(N > 0.0 ? 10.0 * log10(N) : -inf);
        row[RA_SNR_DB] = __double_as_longlong(!(N > 0.0) ? inf : (S > N ? 10.0 * log10((S - N) / N) : -inf));
        row[RA_SPEECH_RATIO] = __double_as_longlong((double)speech / (double)c.F);
        row[RA_BANDWIDTH_HZ] = __double_as_longlong(ra_bandwidth_hz(k_star));
    }
}

struct RaWorkspace {
    RdClip* clips = nullptr; size_t cap_clips = 0;
    RaClip* raws = nullptr; size_t cap_raws = 0;
    RaAcc* acc = nullptr; size_t cap_acc = 0;
    float2* X = nullptr; size_t cap_X = 0;
    float* P = nullptr; size_t cap_P = 0;
    float* floor_ = nullptr; size_t cap_floor = 0;
    double* E = nullptr; size_t cap_E = 0;
    double* T = nullptr; size_t cap_T = 0;
    HostStage stage, stage_raw;
    WorkspaceUse use;
};

int f5hip_ref_assess(int32_t n, const float* raw_dev, const int64_t* raw_offset, const int32_t* channels, const int32_t* raw_len, const float* wave_dev,
                     const int64_t* offset, const int32_t* n_samples, int64_t* rows_dev, void* stream) {
    std::vector<RaClip> hr;
    std::vector<RdClip> h;
    long long rows = 0, total = 0;
    int bad = 0;
    switch (ra_layout(n, raw_offset, channels, raw_len, hr, &bad)) {
        case RA_OK: break;
        case RA_CLIPS: return fail(-1, "ref_assess: 1 .. %d clips in a call (got %d)", kRaMaxClips, n);
        case RA_NULL: return fail(-1, "ref_assess: bad argument");
        case RA_CHANNELS: return fail(-1, "ref_assess: clip %d has %d channels (1 .. %d)", bad, channels[bad], kRaMaxChannels);
        case RA_LENGTH: return fail(-1, "ref_assess: raw clip %d has %d samples in each of %d channels (at least 1, 2^31 - 1 in all)", bad, raw_len[bad], channels[bad]);
        case RA_OFFSET: return fail(-1, "ref_assess: raw clip %d starts at %lld", bad, (long long)raw_offset[bad]);
        default: return fail(-1, "ref_assess: raw clip %d overlaps another clip of the call", bad);
    }
    switch (rd_layout(n, offset, n_samples, h, &rows, &total, &bad)) {
        case RD_OK: break;
        case RD_NO_CLIPS: return fail(-1, "ref_assess: at least one clip (got %d)", n);
        case RD_NULL: return fail(-1, "ref_assess: bad argument");
        case RD_LENGTH: return fail(-1, "ref_assess: clip %d has %d samples (1 .. %d)", bad, n_samples[bad], kRdMaxSamples);
        case RD_OFFSET: return fail(-1, "ref_assess: clip %d starts at %lld", bad, (long long)offset[bad]);
        case RD_OVERLAP: return fail(-1, "ref_assess: clip %d overlaps another clip of the call", bad);
        default: return fail(-1, "ref_assess: the clips of the call exceed 2^31 - 1 frames");
    }
    if (!raw_dev || !wave_dev || !rows_dev) return fail(-1, "ref_assess: bad argument");
    if ((reinterpret_cast<uintptr_t>(raw_dev) & 3) || (reinterpret_cast<uintptr_t>(wave_dev) & 3) || (reinterpret_cast<uintptr_t>(rows_dev) & 7))
        return fail(-1, "ref_assess: the samples must be 4-byte aligned, the rows 8-byte");
    RdWorkspace* const tables = device_workspace<RdWorkspace>("ref_assess");     // the window and the twiddles of the denoiser's FFT
    RaWorkspace* const wsp = device_workspace<RaWorkspace>("ref_assess");
    if (!tables || !wsp) return -6;
    RaWorkspace& ws = *wsp;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(rd_tables(*tables));
    CK(dev_reserve(&ws.clips, &ws.cap_clips, (size_t)n, "ref_assess clips"));
    CK(dev_reserve(&ws.raws, &ws.cap_raws, (size_t)n, "ref_assess raw clips"));
    CK(dev_reserve(&ws.acc, &ws.cap_acc, (size_t)n, "ref_assess accumulators"));
    CK(dev_reserve(&ws.X, &ws.cap_X, (size_t)rows * kRdBins, "ref_assess spectra"));
    CK(dev_reserve(&ws.P, &ws.cap_P, (size_t)rows * kRdPStride, "ref_assess powers"));
    CK(dev_reserve(&ws.floor_, &ws.cap_floor, (size_t)n * kRdPStride, "ref_assess noise floors"));
    CK(dev_reserve(&ws.E, &ws.cap_E, (size_t)rows, "ref_assess band sums"));
    const long long tiles = ra_tile_layout(h, hr);
    CK(dev_reserve(&ws.T, &ws.cap_T, (size_t)tiles * kRaWStride, "ref_assess window sums"));
    CK(ws.stage.upload(ws.clips, h.data(), sizeof(RdClip) * (size_t)n, st));       // pinned staging, queued on `stream`: no wait
    CK(ws.stage_raw.upload(ws.raws, hr.data(), sizeof(RaClip) * (size_t)n, st));
    if (hipMemsetAsync(ws.acc, 0, sizeof(RaAcc) * (size_t)n, st) != hipSuccess) return fail(-6, "ref_assess: memset");

    hipLaunchKernelGGL(ra_peak_kernel, dim3(kRaRawBlocks, (unsigned)n), dim3(256), 0, st, (const RaClip*)ws.raws, raw_dev, ws.acc);
    CKL("ra_peak");
    hipLaunchKernelGGL(ra_runs_kernel, dim3(kRaRawBlocks, (unsigned)n), dim3(256), 0, st, (const RaClip*)ws.raws, raw_dev, ws.acc);
    CKL("ra_runs");
    hipLaunchKernelGGL(rd_stft_kernel, dim3((unsigned)rows), dim3(256), 0, st, ws.clips, n, wave_dev, tables->window, tables->twiddle, ws.X, ws.P);
    CKL("rd_stft");
    hipLaunchKernelGGL(rd_floor_kernel, dim3((unsigned)n * kRdFloorChunks), dim3(kRdFloorWaves * 64), 0, st, ws.clips, ws.P, ws.floor_);
    CKL("rd_floor");
    hipLaunchKernelGGL(ra_frame_kernel, dim3((unsigned)tiles), dim3(256), 0, st, (const RdClip*)ws.clips, (const RaClip*)ws.raws, n, (const float*)ws.P, ws.E, ws.T);
    CKL("ra_frame");
    hipLaunchKernelGGL(ra_clip_kernel, dim3((unsigned)n), dim3(256), 0, st, (const RdClip*)ws.clips, (const RaClip*)ws.raws, (const RaAcc*)ws.acc,
                       (const float*)ws.floor_, (const double*)ws.E, (const double*)ws.T, (long long*)rows_dev);
    CKL("ra_clip");
    g_counters[CNT_REF_ASSESS_LAUNCHES] += 6;
    g_counters[CNT_REF_ASSESS_CLIPS] += n;
    return 0;
}

int f5hip_ref_assess_launches(void) { return 6; }
