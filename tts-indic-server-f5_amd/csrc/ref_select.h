// The cleanest stretch of a long reference recording, on the device: the report's measures (ref_assess.h) over EVERY window of n recordings
// of their own lengths in ONE call, and the window the key picks, on the two buffers a front-end call already holds (its packed raw upload
// and f5hip_ref_frontend's packed 24 kHz output).  Included at the end of f5hip.hip (same translation unit).  The definition is
// audio_prep.select_reference; the geometry, the digits and the row arithmetic are ref_select_core.h, which a host program compiles too.
//
//   rs_clear_kernel         the accumulator cells and the bucket cells to zero (a kernel, so the call can be captured into a graph)
//   ra_peak_kernel          ref_assess.h's, as it stands: the recording's peak, one integer atomicMax per block
//   ra_runs_kernel          ref_assess.h's, as it stands: the recording's samples in runs of three hot samples (for the "every sample is hot" rule)
//   rs_bucket_kernel        grid (64, n): the same run rule per raw sample; a sample in a run adds 1 to the cell of the 256-sample stretch of
//                           the prepared wave it falls under (rs_bucket): integer atomics, rare, order-free
//   rs_scan_kernel          one block per recording: the cells to their exclusive prefix sums, in place (zeros where the report's rule says
//                           clipped = 0); a window's count is then the difference of two cells
//   rd_stft_kernel          ref_denoise.h's, as it stands: P [rows][516] of the prepared recordings' frames
//   rs_band_kernel          one block per tile of 32 frame rows, staged in LDS: the band 3 .. 341 written bin-major, Pb[b][f], so that a window
//                           of one bin is contiguous, and E[f] = sum_b P in fp64 by one thread per row in ascending k
//   rs_window_floor_kernel  THE HOT ONE.  grid (runs, 339): a workgroup owns one bin of one recording and a run of consecutive windows.  The
//                           bin's frames of the whole run go into LDS once, by 16-byte loads.  Each window's rank is found by radix select
//                           on the bit patterns (non-negative floats order like unsigned integers): four 8-bit digits from the top, per-wave
//                           LDS histograms (integer atomics) added in wave order, the digit by a scan of the 256 counts in one wave.
//                           Consecutive windows share Wc - hop frames, so the TOP digit's histograms are kept from window to window: hop
//                           frames leave, hop enter (rs_slide).  The pass over the second digit reads the window once and compacts the
//                           values under the picked top digit into a candidate list; the last two passes read only that list.  The
//                           result is an element of the window, whatever order the atomics land in: every count is an integer
//   rs_window_rows_kernel   one wave per window: N over ascending k and S over ascending f in fp64, each value handed from its lane to the sum
//                           in index order (the wave loads 64 at a time; the additions are the serial ones of the definition), the speech
//                           frames by an integer wave sum, the clipped count from two prefix cells, snr_db; the row
//   rs_choose_kernel        one block per recording: the smallest key (clipped, -snr_db, w) by a fixed tree over a total order
// TEN launches whatever n.  A recording's rows depend on that recording alone: the atomics are integer, the order statistic does not depend
// on any order, and every fp64 sum runs in the definition's order, so its rows are bit-identical alone, in any batch and in any order.
#pragma once
#include "ragged_util.h"
#include "ref_assess.h"
#include "ref_select_core.h"

constexpr int kRsWaves = 4;                    // waves per workgroup of the floor launch

__global__ __launch_bounds__(256) void rs_clear_kernel(RaAcc* __restrict__ acc, int n, int* __restrict__ cells, int ncells) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) { acc[i].in_runs = 0; acc[i].peak_bits = 0; acc[i].pad_ = 0; }
    if (i < ncells) cells[i] = 0;
}

__global__ __launch_bounds__(256) void rs_bucket_kernel(const RaClip* __restrict__ clips, const RsRec* __restrict__ recs, const float* __restrict__ raw,
                                                        const RaAcc* __restrict__ acc, int* __restrict__ cells) {
    const int tid = threadIdx.x;
    const RaClip c = clips[blockIdx.y];
    const RsRec rec = recs[blockIdx.y];
    const long long total = ra_total(c);
    const float peak = __uint_as_float(acc[blockIdx.y].peak_bits);
    if ((long long)blockIdx.x * 256 >= total || peak < kRaMinPeak) return;   // (the same for the whole block)
    const float thr = ra_threshold(peak);
    const float* x = raw + c.off;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < total; i += (long long)kRaRawBlocks * 256) {
        const long long j = ra_sample(c, i);
        if (!ra_in_run(x + (long long)ra_channel(c, i) * c.n, c.n, j, thr)) continue;
        const int m = rs_bucket(rec, j);
        if (m >= 0) atomicAdd(&cells[rec.cell0 + m], 1);
    }
}

__global__ __launch_bounds__(256) void rs_scan_kernel(const RaClip* __restrict__ clips, const RsRec* __restrict__ recs, const RaAcc* __restrict__ acc,
                                                      int* __restrict__ cells) {
    __shared__ int part[256];
    const int ci = blockIdx.x, tid = threadIdx.x;
    const RsRec rec = recs[ci];
    int* cell = cells + rec.cell0;
    const int count = rec.nb + 1, chunk = (count + 255) / 256;
    const int lo = min(count, tid * chunk), hi = min(count, lo + chunk);
    const bool none = ra_clipped((long long)acc[ci].in_runs, __uint_as_float(acc[ci].peak_bits), ra_total(clips[ci])) == 0;
    int sum = 0;
    for (int m = lo; m < hi; m++) sum += cell[m];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int at = 0;
        for (int t = 0; t < 256; t++) { const int v = part[t]; part[t] = at; at += v; }
    }
    __syncthreads();
    int at = part[tid];
    for (int m = lo; m < hi; m++) {
        const int v = cell[m];
        cell[m] = none ? 0 : at;
        at += v;
    }
}

__global__ __launch_bounds__(256) void rs_band_kernel(const RsRec* __restrict__ recs, int n, const float* __restrict__ P, float* __restrict__ Pb,
                                                      double* __restrict__ E) {
    __shared__ float t[kRsTile][kRsBand + 2];                            // 341 floats per row: rows a lane apart fall into different banks
    const int tile = blockIdx.x, tid = threadIdx.x;
    const RsRec c = recs[last_at_or_before<&RsRec::tile0>(recs, n, tile)];
    const int f0 = (tile - c.tile0) * kRsTile, rows = min(kRsTile, c.F - f0);
    const float* Pt = P + (size_t)(c.row0 + f0) * kRdPStride + kRaBand0;
    for (int r = 0; r < rows; r++)
        for (int b = tid; b < kRsBand; b += 256) t[r][b] = Pt[(size_t)r * kRdPStride + b];
    __syncthreads();
    float* out = Pb + c.col0 + f0;
    const int cols = min(kRsTile, c.Fs - f0);                            // the pad cells behind the last frame are this tile's: zeros
    for (int i = tid; i < kRsBand * kRsTile; i += 256) {
        const int b = i / kRsTile, r = i % kRsTile;
        if (r < cols) out[(size_t)b * c.Fs + r] = r < rows ? t[r][b] : 0.0f;
    }
    if (tid < rows) {
        double a = 0.0;
        for (int b = 0; b < kRsBand; b++) a += (double)t[tid][b];
        E[c.row0 + f0 + tid] = a;
    }
}

// the digit of `rank` in the four per-wave histograms h, and the rank inside it -> sel[0], sel[1]; every thread of the block calls it
__device__ __forceinline__ void rs_pick_block(const int (*h)[256], int* tot, int* sel, int tid, int rank) {
    tot[tid] = h[0][tid] + h[1][tid] + h[2][tid] + h[3][tid];            // wave order
    __syncthreads();
    if (tid < 64) {
        const int4 c = reinterpret_cast<const int4*>(tot)[tid];
        const int s = c.x + c.y + c.z + c.w;
        int incl = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (tid >= d) incl += up;
        }
        int r = rank - (incl - s);
        if (r >= 0 && r < s) {                                           // exactly one lane: the counts' sum exceeds the rank
            int d = 4 * tid;
            if (r >= c.x) { r -= c.x; d++; if (r >= c.y) { r -= c.y; d++; if (r >= c.z) { r -= c.z; d++; } } }
            sel[0] = d; sel[1] = r;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kRsWaves * 64) void rs_window_floor_kernel(const RsRec* __restrict__ recs, int n, int hop, int run,
                                                                        const float* __restrict__ Pb, float* __restrict__ floor_) {
    __shared__ __align__(16) unsigned stage[kRsStageCap + 8];
    __shared__ unsigned cand[kRsMaxWindow + 1];
    __shared__ int top[kRsWaves][256];                                   // the top digit's counts of the current window, per wave
    __shared__ int hist[kRsWaves][256];
    __shared__ __align__(16) int tot[256];
    __shared__ int sel[3];                                               // the picked digit, the rank inside it, the candidates
    const int tid = threadIdx.x, wv = tid >> 6;
    const RsRec c = recs[last_at_or_before<&RsRec::run0>(recs, n, (int)blockIdx.x)];
    const int b = blockIdx.y;
    const int w0 = ((int)blockIdx.x - c.run0) * run, w1 = min(c.nwin, w0 + run);
    int fa, fb;
    rs_stage_range(c, hop, w0, w1, &fa, &fb);
    const int a4 = fa & ~3, b4 = min(c.Fs, (fb + 3) & ~3);
    const uint4* col = reinterpret_cast<const uint4*>(Pb + c.col0 + (size_t)b * c.Fs + a4);
    for (int i = tid; i < (b4 - a4) / 4; i += kRsWaves * 64) reinterpret_cast<uint4*>(stage)[i] = col[i];
    for (int i = tid; i < kRsWaves * 256; i += kRsWaves * 64) (&top[0][0])[i] = 0;
    __syncthreads();
    const int base = fa - a4, Wc = c.Wc, slide = rs_slide(Wc, hop);
    for (int i = tid; i < Wc; i += kRsWaves * 64) atomicAdd(&top[wv][rs_digit(stage[base + i], 0)], 1);
    for (int w = w0; w < w1; w++) {
        const int o = base + hop * (w - w0);
        if (w > w0)
            for (int i = tid; i < slide; i += kRsWaves * 64) {
                atomicSub(&top[wv][rs_digit(stage[o - hop + i], 0)], 1);
                atomicAdd(&top[wv][rs_digit(stage[o + Wc - slide + i], 0)], 1);
            }
        if (tid == 0) sel[2] = 0;
        for (int i = tid; i < kRsWaves * 256; i += kRsWaves * 64) (&hist[0][0])[i] = 0;
        __syncthreads();
        rs_pick_block(top, tot, sel, tid, rs_rank(Wc));
        unsigned prefix = (unsigned)sel[0];
        int rank = sel[1];
        for (int i = tid; i < Wc; i += kRsWaves * 64) {                  // the second digit, and the candidates of the last two
            const unsigned v = stage[o + i];
            if (rs_above(v, 1) == prefix) {
                atomicAdd(&hist[wv][rs_digit(v, 1)], 1);
                cand[atomicAdd(&sel[2], 1)] = v;
            }
        }
        __syncthreads();
        const int nc = sel[2];
        rs_pick_block(hist, tot, sel, tid, rank);
        prefix = (prefix << 8) | (unsigned)sel[0];
        rank = sel[1];
#pragma unroll
        for (int pass = 2; pass < 4; pass++) {
            for (int i = tid; i < kRsWaves * 256; i += kRsWaves * 64) (&hist[0][0])[i] = 0;
            __syncthreads();
            for (int i = tid; i < nc; i += kRsWaves * 64) {
                const unsigned v = cand[i];
                if (rs_above(v, pass) == prefix) atomicAdd(&hist[wv][rs_digit(v, pass)], 1);
            }
            __syncthreads();
            rs_pick_block(hist, tot, sel, tid, rank);
            prefix = (prefix << 8) | (unsigned)sel[0];
            rank = sel[1];
        }
        if (tid == 0) floor_[(size_t)(c.win0 + w) * kRsFloorStride + b] = __uint_as_float(prefix);
    }
}

// sum of v[0 .. count) in ascending index order in fp64, by one wave: 64 loads at a time, each value handed from its lane in index order
template <typename T>
__device__ __forceinline__ double rs_ordered_sum(const T* __restrict__ v, int count, int lane) {
    double a = 0.0;
    for (int i0 = 0; i0 < count; i0 += 64) {
        const double mine = i0 + lane < count ? (double)v[i0 + lane] : 0.0;
        const int live = min(64, count - i0);
        for (int j = 0; j < live; j++) a += __shfl(mine, j, 64);
    }
    return a;
}

__global__ __launch_bounds__(256) void rs_window_rows_kernel(const RsRec* __restrict__ recs, int n, int windows, int hop, const float* __restrict__ floor_,
                                                             const double* __restrict__ E, const int* __restrict__ cells, long long* __restrict__ rows) {
    const int lane = threadIdx.x & 63, gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= windows) return;                                           // (the same for the whole wave)
    const RsRec c = recs[last_at_or_before<&RsRec::win0>(recs, n, gw)];
    const int f0 = hop * (gw - c.win0);
    const double* Ew = E + c.row0 + f0;
    const double N = kRaFloorToMean * rs_ordered_sum(floor_ + (size_t)gw * kRsFloorStride, kRsBand, lane);
    const double S = rs_ordered_sum(Ew, c.Wc, lane) / (double)c.Wc;
    int speech = 0;
    for (int f = lane; f < c.Wc; f += 64) speech += (Ew[f] >= kRaSpeechFactor * N && Ew[f] > 0.0) ? 1 : 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) speech += __shfl_down(speech, s, 64);
    if (lane == 0) {
        long long* row = rows + (size_t)gw * kRsRowWords;
        row[RS_CLIPPED] = (long long)(cells[c.cell0 + rs_cell(c, f0 + c.Wc)] - cells[c.cell0 + rs_cell(c, f0 - kRdPad / kRdHop)]);
        row[RS_SPEECH] = speech;
        row[RS_N] = __double_as_longlong(N);
        row[RS_S] = __double_as_longlong(S);
        row[RS_SNR_DB] = __double_as_longlong(rs_snr_db(N, S));
    }
}

__global__ __launch_bounds__(256) void rs_choose_kernel(const RsRec* __restrict__ recs, const long long* __restrict__ rows, long long* __restrict__ choice) {
    __shared__ long long bc[256];
    __shared__ double bs[256];
    __shared__ int bw[256];
    const int tid = threadIdx.x;
    const RsRec c = recs[blockIdx.x];
    const long long* row = rows + (size_t)c.win0 * kRsRowWords;
    long long best_c = 0;
    double best_s = 0.0;
    int best_w = -1;
    for (int w = tid; w < c.nwin; w += 256) {
        const long long cw = row[(size_t)w * kRsRowWords + RS_CLIPPED];
        const double sw = __longlong_as_double(row[(size_t)w * kRsRowWords + RS_SNR_DB]);
        if (best_w < 0 || rs_key_less(cw, sw, w, best_c, best_s, best_w)) { best_c = cw; best_s = sw; best_w = w; }
    }
    bc[tid] = best_c; bs[tid] = best_s; bw[tid] = best_w;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s && bw[tid + s] >= 0 && (bw[tid] < 0 || rs_key_less(bc[tid + s], bs[tid + s], bw[tid + s], bc[tid], bs[tid], bw[tid]))) {
            bc[tid] = bc[tid + s]; bs[tid] = bs[tid + s]; bw[tid] = bw[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) choice[blockIdx.x] = bw[0];
}

struct RsWorkspace {
    RdClip* clips = nullptr; size_t cap_clips = 0;
    RaClip* raws = nullptr; size_t cap_raws = 0;
    RsRec* recs = nullptr; size_t cap_recs = 0;
    RaAcc* acc = nullptr; size_t cap_acc = 0;
    int* cells = nullptr; size_t cap_cells = 0;
    float2* X = nullptr; size_t cap_X = 0;
    float* P = nullptr; size_t cap_P = 0;
    float* Pb = nullptr; size_t cap_Pb = 0;
    float* floor_ = nullptr; size_t cap_floor = 0;
    double* E = nullptr; size_t cap_E = 0;
    HostStage stage, stage_raw, stage_rec;
    WorkspaceUse use;
};

int f5hip_ref_select_run(int32_t window_frames, int32_t hop_frames) {
    if (window_frames < 1 || window_frames > kRsMaxWindow || hop_frames < 1 || hop_frames > kRsMaxHop)
        return fail(-1, "ref_select_run: window_frames 1 .. %d, hop_frames 1 .. %d (got %d, %d)", kRsMaxWindow, kRsMaxHop, window_frames, hop_frames);
    return rs_run(window_frames, hop_frames);
}

int f5hip_ref_select(int32_t n, const float* raw_dev, const int64_t* raw_offset, const int32_t* channels, const int32_t* raw_len, const int32_t* sample_rate,
                     const float* wave_dev, const int64_t* offset, const int32_t* n_samples, int32_t window_frames, int32_t hop_frames, int64_t* rows_dev,
                     int64_t* choice_dev, float* floor_dev, float* power_dev, void* stream) {
    std::vector<RaClip> hr;
    std::vector<RdClip> h;
    std::vector<RsRec> hs;
    RsPlan plan;
    int bad = 0;
    if (n < 1 || n > kRsMaxRecs) return fail(-1, "ref_select: 1 .. %d recordings in a call (got %d)", kRsMaxRecs, n);
    switch (ra_layout(n, raw_offset, channels, raw_len, hr, &bad)) {
        case RA_OK: break;
        case RA_CLIPS: return fail(-1, "ref_select: 1 .. %d recordings in a call (got %d)", kRsMaxRecs, n);
        case RA_NULL: return fail(-1, "ref_select: bad argument");
        case RA_CHANNELS: return fail(-1, "ref_select: recording %d has %d channels (1 .. %d)", bad, channels[bad], kRaMaxChannels);
        case RA_LENGTH: return fail(-1, "ref_select: raw recording %d has %d samples in each of %d channels (at least 1, 2^31 - 1 in all)", bad, raw_len[bad], channels[bad]);
        case RA_OFFSET: return fail(-1, "ref_select: raw recording %d starts at %lld", bad, (long long)raw_offset[bad]);
        default: return fail(-1, "ref_select: raw recording %d overlaps another recording of the call", bad);
    }
    switch (rs_layout(n, sample_rate, offset, n_samples, window_frames, hop_frames, hs, h, &plan, &bad)) {
        case RS_OK: break;
        case RS_RECS: return fail(-1, "ref_select: 1 .. %d recordings in a call (got %d)", kRsMaxRecs, n);
        case RS_NULL: return fail(-1, "ref_select: bad argument");
        case RS_WINDOW: return fail(-1, "ref_select: window_frames must be 1 .. %d (got %d)", kRsMaxWindow, window_frames);
        case RS_HOP: return fail(-1, "ref_select: hop_frames must be 1 .. %d (got %d)", kRsMaxHop, hop_frames);
        case RS_RATE: return fail(-1, "ref_select: recording %d has the sample rate %d (1 .. %d)", bad, sample_rate[bad], kRsMaxRate);
        case RS_LENGTH: return fail(-1, "ref_select: recording %d has %d samples (1 .. %d)", bad, n_samples[bad], kRsMaxSamples);
        case RS_OFFSET: return fail(-1, "ref_select: recording %d starts at %lld", bad, (long long)offset[bad]);
        case RS_OVERLAP: return fail(-1, "ref_select: recording %d overlaps another recording of the call", bad);
        default: return fail(-1, "ref_select: the recordings of a call hold at most %lld samples in all (four of 600 s); recording %d passes that", kRsMaxCallSamples, bad);
    }
    if (!raw_dev || !wave_dev || !rows_dev || !choice_dev) return fail(-1, "ref_select: bad argument");
    if ((reinterpret_cast<uintptr_t>(raw_dev) & 3) || (reinterpret_cast<uintptr_t>(wave_dev) & 3) || (reinterpret_cast<uintptr_t>(rows_dev) & 7) ||
        (reinterpret_cast<uintptr_t>(choice_dev) & 7) || (reinterpret_cast<uintptr_t>(floor_dev) & 3) || (reinterpret_cast<uintptr_t>(power_dev) & 15))
        return fail(-1, "ref_select: the samples and floors must be 4-byte aligned, the rows and choices 8-byte, the powers 16-byte");
    RdWorkspace* const tables = device_workspace<RdWorkspace>("ref_select");     // the window and the twiddles of the denoiser's FFT
    RsWorkspace* const wsp = device_workspace<RsWorkspace>("ref_select");
    if (!tables || !wsp) return -6;
    RsWorkspace& ws = *wsp;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(rd_tables(*tables));
    CK(dev_reserve(&ws.clips, &ws.cap_clips, (size_t)n, "ref_select clips"));
    CK(dev_reserve(&ws.raws, &ws.cap_raws, (size_t)n, "ref_select raw recordings"));
    CK(dev_reserve(&ws.recs, &ws.cap_recs, (size_t)n, "ref_select recordings"));
    CK(dev_reserve(&ws.acc, &ws.cap_acc, (size_t)n, "ref_select accumulators"));
    CK(dev_reserve(&ws.cells, &ws.cap_cells, (size_t)plan.cells, "ref_select clipping cells"));
    CK(dev_reserve(&ws.X, &ws.cap_X, (size_t)plan.rows * kRdBins, "ref_select spectra"));
    CK(dev_reserve(&ws.P, &ws.cap_P, (size_t)plan.rows * kRdPStride, "ref_select powers"));
    CK(dev_reserve(&ws.E, &ws.cap_E, (size_t)plan.rows, "ref_select band sums"));
    float* Pb = power_dev;
    float* floor_ = floor_dev;
    if (!Pb) { CK(dev_reserve(&ws.Pb, &ws.cap_Pb, (size_t)plan.cols, "ref_select band powers")); Pb = ws.Pb; }
    if (!floor_) { CK(dev_reserve(&ws.floor_, &ws.cap_floor, (size_t)plan.windows * kRsFloorStride, "ref_select window floors")); floor_ = ws.floor_; }
    CK(ws.stage.upload(ws.clips, h.data(), sizeof(RdClip) * (size_t)n, st));       // pinned staging, queued on `stream`: no wait
    CK(ws.stage_raw.upload(ws.raws, hr.data(), sizeof(RaClip) * (size_t)n, st));
    CK(ws.stage_rec.upload(ws.recs, hs.data(), sizeof(RsRec) * (size_t)n, st));

    const int clear = plan.cells > n ? plan.cells : n;
    hipLaunchKernelGGL(rs_clear_kernel, dim3((unsigned)((clear + 255) / 256)), dim3(256), 0, st, ws.acc, n, ws.cells, plan.cells);
    CKL("rs_clear");
    hipLaunchKernelGGL(ra_peak_kernel, dim3(kRaRawBlocks, (unsigned)n), dim3(256), 0, st, (const RaClip*)ws.raws, raw_dev, ws.acc);
    CKL("ra_peak");
    hipLaunchKernelGGL(ra_runs_kernel, dim3(kRaRawBlocks, (unsigned)n), dim3(256), 0, st, (const RaClip*)ws.raws, raw_dev, ws.acc);
    CKL("ra_runs");
    hipLaunchKernelGGL(rs_bucket_kernel, dim3(kRaRawBlocks, (unsigned)n), dim3(256), 0, st, (const RaClip*)ws.raws, (const RsRec*)ws.recs, raw_dev,
                       (const RaAcc*)ws.acc, ws.cells);
    CKL("rs_bucket");
    hipLaunchKernelGGL(rs_scan_kernel, dim3((unsigned)n), dim3(256), 0, st, (const RaClip*)ws.raws, (const RsRec*)ws.recs, (const RaAcc*)ws.acc, ws.cells);
    CKL("rs_scan");
    hipLaunchKernelGGL(rd_stft_kernel, dim3((unsigned)plan.rows), dim3(256), 0, st, ws.clips, n, wave_dev, tables->window, tables->twiddle, ws.X, ws.P);
    CKL("rd_stft");
    hipLaunchKernelGGL(rs_band_kernel, dim3((unsigned)plan.tiles), dim3(256), 0, st, (const RsRec*)ws.recs, n, (const float*)ws.P, Pb, ws.E);
    CKL("rs_band");
    hipLaunchKernelGGL(rs_window_floor_kernel, dim3((unsigned)plan.runs, kRsBand), dim3(kRsWaves * 64), 0, st, (const RsRec*)ws.recs, n, (int)hop_frames, plan.run,
                       (const float*)Pb, floor_);
    CKL("rs_window_floor");
    hipLaunchKernelGGL(rs_window_rows_kernel, dim3((unsigned)((plan.windows + 3) / 4)), dim3(256), 0, st, (const RsRec*)ws.recs, n, plan.windows, (int)hop_frames,
                       (const float*)floor_, (const double*)ws.E, (const int*)ws.cells, (long long*)rows_dev);
    CKL("rs_window_rows");
    hipLaunchKernelGGL(rs_choose_kernel, dim3((unsigned)n), dim3(256), 0, st, (const RsRec*)ws.recs, (const long long*)rows_dev, (long long*)choice_dev);
    CKL("rs_choose");
    return 0;
}
