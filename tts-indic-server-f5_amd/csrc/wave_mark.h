// The provenance watermark on the device: f5hip_wave_mark adds a key's mark to the finished 24 kHz PCM of the flagged requests in place, bit
// for bit wave_codec.mark_pcm16; f5hip_watermark_detect scores a ragged batch of clips against every key (wave_codec.detect_watermark).
// Included at the end of f5hip.hip (same translation unit).  The definitions are written down in wave_codec.py; the constants, the block
// geometry, the sample arithmetic and the tie rule are wave_mark_core.h, which a host program compiles too.
//
//   wave_mark_sum_kernel  one block per tile of 32 blocks of 240 samples of a flagged request: the tile's samples, masked by the device
//                         length, as magnitudes into LDS (coalesced), eight threads per block sum, A [tiles * 32] int to the workspace
//   wave_mark_add_kernel  one block per tile: groups of 8 samples (one 16-byte load and store where the address allows), E from the three
//                         block sums around the group, the carrier's 8 values as one 16-byte load, wm_mark per sample
//   wave_mark_id_add_kernel  wave_mark_add_kernel for a call in which a request carries a trace id (f5hip_wave_mark_ids): the key's 8 carrier
//                         values doubled, and for a request with an id three more 16-byte loads, its sub-key rows rotated by 16 s_d, added:
//                         wm_mark_id per sample.  A request without an id skips the three loads and gets wave_mark_add_kernel's bytes
// TWO launches whatever n, none when nobody is flagged.  Integers only: no sum depends on an order.
//
//   wd_frame_kernel       one block per frame row of the packed batch: the frame times w through fft1024_lds, X[k] / sqrt(|X[k]|^2 + 1e-10)
//                         inside the band and 0 outside, the Hermitian fill, fft1024_lds with sign +1, times w / 1024 -> fw [rows][1024]
//   wd_fold_kernel        one thread per (clip, residue m): for j = m, m + P, ... ascending, u[j] = its four frames added in ascending frame
//                         order, Z[m] = their sum in that order
//   wd_corr_kernel        one block per (group of 4 clips, key, tile of 512 offsets): 512 residues of the group's Z and the carrier window
//                         that the tile's offsets need over them staged in LDS, so a carrier tile is read once per clip group; each thread
//                         owns 2 offsets x 4 clips and adds Z[m] c[(m + o) mod P] for m ascending from 0: r [n][n_keys][P]
//   wd_score_kernel       one block per (clip, key): the maximum of r (ties to the smaller offset), mean and population deviation in fp64
//                         by fixed trees -> (z, offset, r[o*], sigma); a clip below WATERMARK_MIN_SAMPLES gets zeros
//   watermark_id_score_kernel  f5hip_watermark_read_ids' fourth launch, one block per (clip, key) over the key's four rows of r: the key's row
//                         as wd_score_kernel scores it (wd_moments, wd_grid_max: the same trees), then per sub-key row its moments and the
//                         maximum over the 1024 offsets o* - 16 s (ties to the smaller s) -> (z, offset, r[o*], sigma, s_0, z_0, .., s_2, z_2)
// FOUR launches whatever n.  Every sum runs in an order fixed by the clip alone, so a clip's row is bit-identical alone and in a batch.
//
//   ws_range_fold_kernel  f5hip_watermark_scan's second launch (wave_codec.scan_watermark: ONE recording of up to 600 s, any number of ranges of
//                         whole segments of P samples): wd_fold_kernel over a range -- one thread per (range, residue m), the range's segments
//                         ascending, each sample's four frames ascending -- on the frames wd_frame_kernel wrote for the whole recording, so
//                         Z[m] folds the samples by their absolute index
// wd_frame_kernel and ws_range_fold_kernel once, then wd_corr_kernel and wd_score_kernel / watermark_id_score_kernel as they stand once per slab
// of ws_slab_ranges(carrier rows) ranges: 2 + 2 slabs launches, FOUR for a call of one slab.  A range's row is bit-identical alone, with any
// other ranges, in any order and in any slab.
#pragma once
#include "ragged_util.h"
#include "ref_denoise_core.h"
#include "wave_mark_core.h"

struct WmReq {
    long long in_off;    // its first sample, relative to pcm_dev
    int cap;             // upper bound of its length (the length itself without len_dev)
    int req;             // its index in the call: len_dev
    int key;             // its row of carriers_dev
    int tile0;           // its first block of either launch; its block sums start at kWmTileBlocks * tile0
    int tiles;
    int id;              // its trace id, -1 without one (f5hip_wave_mark: always -1)
};

F5_DEVICE int wm_len(const int* len_dev, const WmReq& q) { return len_dev ? min(max(len_dev[q.req], 0), q.cap) : q.cap; }

__global__ __launch_bounds__(256) void wave_mark_sum_kernel(const WmReq* __restrict__ reqs, int nf, const short* __restrict__ pcm,
                                                            const int* __restrict__ len_dev, int* __restrict__ A) {
    __shared__ unsigned short mag[kWmTile];
    __shared__ int part[256];
    const int tid = threadIdx.x;
    const WmReq q = reqs[last_at_or_before<&WmReq::tile0>(reqs, nf, (int)blockIdx.x)];
    const int len = wm_len(len_dev, q);
    const long long j0 = (long long)(blockIdx.x - q.tile0) * kWmTile;
    const short* x = pcm + q.in_off;
    for (int i = tid; i < kWmTile; i += 256) {
        const long long j = j0 + i;
        const int v = j < len ? (int)x[j] : 0;
        mag[i] = (unsigned short)(v < 0 ? -v : v);
    }
    __syncthreads();
    constexpr int kPer = kWmBlock / 8;                                   // 30 samples per thread, eight threads per block of 240
    int s = 0;
#pragma unroll
    for (int i = 0; i < kPer; i++) s += mag[tid * kPer + i];
    part[tid] = s;
    __syncthreads();
    if (tid < kWmTileBlocks) {
        int a = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) a += part[8 * tid + t];
        A[(long long)blockIdx.x * kWmTileBlocks + tid] = a;
    }
}

__global__ __launch_bounds__(256) void wave_mark_add_kernel(const WmReq* __restrict__ reqs, int nf, short* __restrict__ pcm,
                                                            const int* __restrict__ len_dev, const int* __restrict__ A,
                                                            const short* __restrict__ carriers) {
    const WmReq q = reqs[last_at_or_before<&WmReq::tile0>(reqs, nf, (int)blockIdx.x)];
    const int len = wm_len(len_dev, q);
    const int tile = blockIdx.x - q.tile0;
    const long long j0 = (long long)tile * kWmTile;
    short* x = pcm + q.in_off;
    const int* Aq = A + (long long)q.tile0 * kWmTileBlocks;
    const long long nA = (long long)q.tiles * kWmTileBlocks;
    const short* c = carriers + (long long)q.key * kWmPeriod;
    for (int grp = threadIdx.x; grp < kWmTile / 8; grp += 256) {
        const long long j = j0 + 8 * grp;
        if (j >= len) break;
        const int E = wm_envelope(Aq, nA, j / kWmBlock);
        if (E == 0) continue;                                           // silence around it: the samples stay
        const int4 cv = *reinterpret_cast<const int4*>(c + (j & (kWmPeriod - 1)));
        const int c8[4] = {cv.x, cv.y, cv.z, cv.w};
        if (j + 8 <= len && (reinterpret_cast<uintptr_t>(x + j) & 15) == 0) {
            const int4 in = *reinterpret_cast<const int4*>(x + j);
            const int w8[4] = {in.x, in.y, in.z, in.w};
            int o[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int lo = wm_mark((int)(short)(w8[e] & 0xffff), E, (int)(short)(c8[e] & 0xffff));
                const int hi = wm_mark(w8[e] >> 16, E, c8[e] >> 16);
                o[e] = (lo & 0xffff) | (hi << 16);
            }
            *reinterpret_cast<int4*>(x + j) = make_int4(o[0], o[1], o[2], o[3]);
        } else {
            for (int e = 0; e < 8 && j + e < len; e++) {
                const int ce = (e & 1) ? c8[e >> 1] >> 16 : (int)(short)(c8[e >> 1] & 0xffff);
                x[j + e] = (short)wm_mark((int)x[j + e], E, ce);
            }
        }
    }
}

__global__ __launch_bounds__(256) void wave_mark_id_add_kernel(const WmReq* __restrict__ reqs, int nf, short* __restrict__ pcm,
                                                               const int* __restrict__ len_dev, const int* __restrict__ A,
                                                               const short* __restrict__ carriers) {
    const WmReq q = reqs[last_at_or_before<&WmReq::tile0>(reqs, nf, (int)blockIdx.x)];
    const int len = wm_len(len_dev, q);
    const int tile = blockIdx.x - q.tile0;
    const long long j0 = (long long)tile * kWmTile;
    short* x = pcm + q.in_off;
    const int* Aq = A + (long long)q.tile0 * kWmTileBlocks;
    const long long nA = (long long)q.tiles * kWmTileBlocks;
    const short* c = carriers + (long long)q.key * kWmPeriod;           // the key's row; its sub-keys' rows follow it
    for (int grp = threadIdx.x; grp < kWmTile / 8; grp += 256) {
        const long long j = j0 + 8 * grp;
        if (j >= len) break;
        const int E = wm_envelope(Aq, nA, j / kWmBlock);
        if (E == 0) continue;                                           // silence around it: the samples stay
        const int4 kv = *reinterpret_cast<const int4*>(c + (j & (kWmPeriod - 1)));
        const int k8[4] = {kv.x, kv.y, kv.z, kv.w};
        int C[8];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            C[2 * e] = 2 * (int)(short)(k8[e] & 0xffff);
            C[2 * e + 1] = 2 * (k8[e] >> 16);
        }
        if (q.id >= 0) {                                                // (the same for the whole block)
#pragma unroll
            for (int d = 0; d < kWmIdSymbols; d++) {
                const int4 dv = *reinterpret_cast<const int4*>(c + (long long)(1 + d) * kWmPeriod + wm_id_index(j, wm_id_symbol(q.id, d)));
                const int d8[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    C[2 * e] += (int)(short)(d8[e] & 0xffff);
                    C[2 * e + 1] += d8[e] >> 16;
                }
            }
        }
        if (j + 8 <= len && (reinterpret_cast<uintptr_t>(x + j) & 15) == 0) {
            const int4 in = *reinterpret_cast<const int4*>(x + j);
            const int w8[4] = {in.x, in.y, in.z, in.w};
            int o[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int lo = wm_mark_id((int)(short)(w8[e] & 0xffff), E, C[2 * e]);
                const int hi = wm_mark_id(w8[e] >> 16, E, C[2 * e + 1]);
                o[e] = (lo & 0xffff) | (hi << 16);
            }
            *reinterpret_cast<int4*>(x + j) = make_int4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++)
                if (j + e < len) x[j + e] = (short)wm_mark_id((int)x[j + e], E, C[e]);
        }
    }
}

struct WmWorkspace {
    WorkspaceUse use;
    WmReq* reqs = nullptr; size_t cap_reqs = 0;
    int* A = nullptr; size_t cap_A = 0;
    HostStage stage;
};

int f5hip_wave_mark_tile(void) { return kWmTile; }

int f5hip_watermark_carrier(uint64_t key, int16_t* carrier) {
    static const int g[kWmTaps] = {
#include "watermark_taps.inc"
    };
    if (!carrier) return fail(-1, "watermark_carrier: bad argument");
    if (!wm_key_ok(key)) return fail(-1, "watermark_carrier: a key is 1 .. 2^48 - 1 (got %llu)", (unsigned long long)key);
    std::vector<signed char> chips((size_t)kWmPeriod);
    wm_carrier(key, g, chips.data(), carrier);
    return 0;
}

// f5hip_wave_mark (id null, one carrier row per key) and f5hip_wave_mark_ids (kWmTagRows rows per key) under their names
static int wave_mark_call(const char* op, int32_t n, int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev,
                          const int32_t* key_index, const int32_t* id, const int16_t* carriers_dev, int32_t n_keys, int key_rows, void* stream) {
    if (n < 1 || !pcm_dev || !in_off || !max_len || !key_index) return fail(-1, "%s: bad argument", op);
    if ((reinterpret_cast<uintptr_t>(pcm_dev) & 1) || (reinterpret_cast<uintptr_t>(len_dev) & 3))
        return fail(-1, "%s: the samples must be 2-byte aligned and the lengths 4-byte", op);
    if (n_keys < 0 || n_keys > kWmKeysMax) return fail(-1, "%s: 1 .. %d keys in a call (got %d)", op, kWmKeysMax, n_keys);
    std::vector<WmReq> h;
    long long total = 0, tiles = 0;
    int tagged = 0;
    for (int i = 0; i < n; i++) {
        if (max_len[i] < 0) return fail(-1, "%s: request %d has a negative length bound (%d)", op, i, max_len[i]);
        if (in_off[i] < 0) return fail(-1, "%s: request %d has a negative offset", op, i);
        if (key_index[i] < -1 || key_index[i] >= n_keys) return fail(-1, "%s: request %d names key %d of %d", op, i, key_index[i], n_keys);
        const int tag = id ? id[i] : -1;
        if (tag < -1 || tag > kWmIdMax) return fail(-1, "%s: request %d has id %d (-1, or 0 .. %d)", op, i, tag, kWmIdMax);
        if (tag >= 0 && key_index[i] < 0) return fail(-1, "%s: request %d has an id and no key", op, i);
        total += max_len[i];
        if (total > 2147483647LL) return fail(-1, "%s: the call exceeds 2^31 - 1 samples", op);
        if (key_index[i] < 0) continue;                                 // -1: the request is left alone
        const long long t = wm_tiles(max_len[i]);
        h.push_back(WmReq{in_off[i], max_len[i], i, key_index[i] * key_rows, (int)tiles, (int)t, tag});
        tiles += t;
        tagged += tag >= 0;
    }
    if (h.empty()) return 0;
    if (!carriers_dev || (reinterpret_cast<uintptr_t>(carriers_dev) & 15)) return fail(-1, "%s: the carriers must be 16-byte aligned", op);
    WmWorkspace* const wsp = device_workspace<WmWorkspace>("wave_mark");
    if (!wsp) return -6;
    WmWorkspace& ws = *wsp;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(dev_reserve(&ws.reqs, &ws.cap_reqs, h.size(), "wave_mark requests"));
    CK(dev_reserve(&ws.A, &ws.cap_A, (size_t)(tiles * kWmTileBlocks), "wave_mark block sums"));
    CK(ws.stage.upload(ws.reqs, h.data(), sizeof(WmReq) * h.size(), st));   // pinned staging, queued on `stream`: no wait
    const int nf = (int)h.size();
    hipLaunchKernelGGL(wave_mark_sum_kernel, dim3((unsigned)tiles), dim3(256), 0, st, ws.reqs, nf, (const short*)pcm_dev, (const int*)len_dev, ws.A);
    CKL("wave_mark_sum");
    if (tagged) {
        hipLaunchKernelGGL(wave_mark_id_add_kernel, dim3((unsigned)tiles), dim3(256), 0, st, ws.reqs, nf, (short*)pcm_dev, (const int*)len_dev,
                           (const int*)ws.A, (const short*)carriers_dev);
        CKL("wave_mark_id_add");
        g_counters[CNT_WAVE_MARK_ID_LAUNCHES] += 2;
        g_counters[CNT_WAVE_MARK_ID_REQUESTS] += nf;
        return 0;
    }
    hipLaunchKernelGGL(wave_mark_add_kernel, dim3((unsigned)tiles), dim3(256), 0, st, ws.reqs, nf, (short*)pcm_dev, (const int*)len_dev,
                       (const int*)ws.A, (const short*)carriers_dev);
    CKL("wave_mark_add");
    g_counters[CNT_WAVE_MARK_LAUNCHES] += 2;
    g_counters[CNT_WAVE_MARK_REQUESTS] += nf;
    return 0;
}

int f5hip_wave_mark(int32_t n, int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev, const int32_t* key_index,
                    const int16_t* carriers_dev, int32_t n_keys, void* stream) {
    return wave_mark_call("wave_mark", n, pcm_dev, in_off, max_len, len_dev, key_index, nullptr, carriers_dev, n_keys, 1, stream);
}

int f5hip_wave_mark_ids(int32_t n, int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev, const int32_t* key_index,
                        const int32_t* id, const int16_t* carriers_dev, int32_t n_keys, void* stream) {
    if (!id) return fail(-1, "wave_mark_ids: bad argument");
    return wave_mark_call("wave_mark_ids", n, pcm_dev, in_off, max_len, len_dev, key_index, id, carriers_dev, n_keys, kWmTagRows, stream);
}

// ------------------------------------------------------------------------------------------------ the detector
__global__ __launch_bounds__(256) void wd_frame_kernel(const RdClip* __restrict__ clips, int n, const float* __restrict__ wave,
                                                       const float* __restrict__ window, const float2* __restrict__ tw, float* __restrict__ fw) {
    __shared__ float2 s[kRdNfft];
    const int row = blockIdx.x, tid = threadIdx.x;
    const RdClip c = clips[last_at_or_before<&RdClip::row0>(clips, n, row)];
    const int m = row - c.row0;
    const float* x = wave + c.off;
    for (int i = tid; i < kRdNfft; i += 256) {
        const long long j = rd_frame_sample(m, i);
        const float v = j >= 0 && j < c.n ? x[j] : 0.0f;
        s[__brev((unsigned)i) >> 22] = make_float2(v * window[i], 0.0f);
    }
    fft1024_lds(s, tw, tid, -1.0f);
    static_assert(kWdBandHi < 256, "wd_frame: thread k holds bin k of the band");
    const bool band = tid >= kWdBandLo && tid <= kWdBandHi;
    float2 U = make_float2(0.0f, 0.0f);
    if (band) {
        const float2 v = s[tid];
        const float inv = 1.0f / sqrtf(v.x * v.x + v.y * v.y + kWdEps);
        U = make_float2(v.x * inv, v.y * inv);
    }
    __syncthreads();
    for (int i = tid; i < kRdNfft; i += 256) s[i] = make_float2(0.0f, 0.0f);
    __syncthreads();
    if (band) {
        s[__brev((unsigned)tid) >> 22] = U;
        s[__brev((unsigned)(kRdNfft - tid)) >> 22] = make_float2(U.x, -U.y);
    }
    fft1024_lds(s, tw, tid, 1.0f);
    for (int i = tid; i < kRdNfft; i += 256) fw[(size_t)row * kRdNfft + i] = s[i].x * (window[i] * (1.0f / kRdNfft));
}

__global__ __launch_bounds__(256) void wd_fold_kernel(const RdClip* __restrict__ clips, const float* __restrict__ fw, float* __restrict__ Z) {
    const RdClip c = clips[blockIdx.y];
    const int m = blockIdx.x * 256 + threadIdx.x;
    float acc = 0.0f;
    for (long long j = m; j < c.n; j += kWmPeriod) {
        const int m0 = rd_sample_frame0(j);
        float u = 0.0f;
#pragma unroll
        for (int d = 0; d < kRdFramesPerSample; d++) u += fw[(size_t)(c.row0 + m0 + d) * kRdNfft + rd_sample_offset(j, m0 + d)];
        acc += u;
    }
    Z[(size_t)blockIdx.y * kWmPeriod + m] = acc;
}

__global__ __launch_bounds__(256) void wd_corr_kernel(int n, int n_keys, const float* __restrict__ Z, const short* __restrict__ carriers,
                                                      float* __restrict__ r) {
    __shared__ float4 zs[kWdChunk];                                      // the group's four Z values of a residue
    __shared__ float cw[kWdChunk + kWdOffTile];                          // c[(m0 + o0 + i) mod P]
    static_assert(kWdGroup == 4 && kWdOffTile == 512, "wd_corr: a thread owns 2 offsets x 4 clips");
    const int tid = threadIdx.x;
    const int o0 = blockIdx.x * kWdOffTile, key = blockIdx.y, clip0 = blockIdx.z * kWdGroup;
    const short* c = carriers + (size_t)key * kWmPeriod;
    float acc[2][kWdGroup];
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int g = 0; g < kWdGroup; g++) acc[q][g] = 0.0f;
    for (int m0 = 0; m0 < kWmPeriod; m0 += kWdChunk) {
        __syncthreads();
        for (int i = tid; i < kWdChunk; i += 256) {
            float z[kWdGroup];
#pragma unroll
            for (int g = 0; g < kWdGroup; g++) z[g] = clip0 + g < n ? Z[(size_t)(clip0 + g) * kWmPeriod + m0 + i] : 0.0f;
            zs[i] = make_float4(z[0], z[1], z[2], z[3]);
        }
        for (int i = tid; i < kWdChunk + kWdOffTile; i += 256) cw[i] = (float)c[(m0 + o0 + i) & (kWmPeriod - 1)];
        __syncthreads();
#pragma unroll 8
        for (int mm = 0; mm < kWdChunk; mm++) {
            const float4 z = zs[mm];
            const float c0 = cw[mm + tid], c1 = cw[mm + tid + 256];
            acc[0][0] = fmaf(z.x, c0, acc[0][0]); acc[0][1] = fmaf(z.y, c0, acc[0][1]);
            acc[0][2] = fmaf(z.z, c0, acc[0][2]); acc[0][3] = fmaf(z.w, c0, acc[0][3]);
            acc[1][0] = fmaf(z.x, c1, acc[1][0]); acc[1][1] = fmaf(z.y, c1, acc[1][1]);
            acc[1][2] = fmaf(z.z, c1, acc[1][2]); acc[1][3] = fmaf(z.w, c1, acc[1][3]);
        }
    }
#pragma unroll
    for (int g = 0; g < kWdGroup; g++) {
        if (clip0 + g >= n) break;
        float* row = r + ((size_t)(clip0 + g) * n_keys + key) * kWmPeriod + o0;
        row[tid] = acc[0][g];
        row[tid + 256] = acc[1][g];
    }
}

// mean and population deviation of a row of r [P] in fp64 by a block of 256 threads: thread t adds offsets t, t + 256, ... ascending, then
// block_sum's fixed tree; every thread returns both
F5_DEVICE void wd_moments(const float* __restrict__ row, double* red, int tid, double* mean_out, double* sigma_out) {
    constexpr int kPer = kWmPeriod / 256;
    double sum = 0.0;
    for (int i = 0; i < kPer; i++) sum += (double)row[tid + 256 * i];
    const double mean = block_sum(red, tid, sum) / (double)kWmPeriod;
    double sq = 0.0;
    for (int i = 0; i < kPer; i++) {
        const double d = (double)row[tid + 256 * i] - mean;
        sq += d * d;
    }
    *mean_out = mean;
    *sigma_out = sqrt(block_sum(red, tid, sq) / (double)kWmPeriod);
}

// the maximum of row[(base - step * s) mod P] over s = 0 .. count - 1 (count a multiple of 256) with ties to the smaller s (wd_better), by a
// block of 256 threads: thread t holds s = t, t + 256, ..., then a fixed tree; the value is left in bv[0] and s in bi[0] for every thread
F5_DEVICE void wd_grid_max(const float* __restrict__ row, int base, int step, int count, float* bv, int* bi, int tid) {
    float best = row[(base - step * tid) & (kWmPeriod - 1)];
    int at = tid;
    for (int s = tid + 256; s < count; s += 256) {
        const float v = row[(base - step * s) & (kWmPeriod - 1)];
        if (wd_better(v, s, best, at)) { best = v; at = s; }
    }
    __syncthreads();                                                     // (bv, bi of an earlier call have been read)
    bv[tid] = best; bi[tid] = at;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s && wd_better(bv[tid + s], bi[tid + s], bv[tid], bi[tid])) { bv[tid] = bv[tid + s]; bi[tid] = bi[tid + s]; }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void wd_score_kernel(const RdClip* __restrict__ clips, int n_keys, const float* __restrict__ r,
                                                       float* __restrict__ scores) {
    __shared__ double red[256];
    __shared__ float bv[256];
    __shared__ int bi[256];
    const int tid = threadIdx.x;
    const int clip = blockIdx.x / n_keys;
    float* out = scores + 4 * (size_t)blockIdx.x;
    if (clips[clip].n < kWdMinSamples) {                                 // (the same for the whole block)
        if (tid < 4) out[tid] = 0.0f;
        return;
    }
    const float* row = r + (size_t)blockIdx.x * kWmPeriod;
    double mean, sigma;
    wd_moments(row, red, tid, &mean, &sigma);
    wd_grid_max(row, 0, -1, kWmPeriod, bv, bi, tid);                     // every offset: s is the offset
    if (tid == 0) {
        out[0] = sigma > 0.0 ? (float)(((double)bv[0] - mean) / sigma) : 0.0f;
        out[1] = (float)bi[0];
        out[2] = bv[0];
        out[3] = (float)sigma;
    }
}

__global__ __launch_bounds__(256) void watermark_id_score_kernel(const RdClip* __restrict__ clips, int n_keys, const float* __restrict__ r,
                                                                 float* __restrict__ rows) {
    __shared__ double red[256];
    __shared__ float bv[256];
    __shared__ int bi[256];
    const int tid = threadIdx.x;
    const int clip = blockIdx.x / n_keys;
    float* out = rows + kWdIdRowWords * (size_t)blockIdx.x;
    if (clips[clip].n < kWdMinSamples) {                                 // (the same for the whole block)
        if (tid < kWdIdRowWords) out[tid] = 0.0f;
        return;
    }
    const float* row = r + (size_t)blockIdx.x * kWmTagRows * kWmPeriod;  // the key's row of r; its sub-keys' rows follow it
    double mean, sigma;
    wd_moments(row, red, tid, &mean, &sigma);
    wd_grid_max(row, 0, -1, kWmPeriod, bv, bi, tid);
    const int o = bi[0];
    if (tid == 0) {
        out[0] = sigma > 0.0 ? (float)(((double)bv[0] - mean) / sigma) : 0.0f;
        out[1] = (float)o;
        out[2] = bv[0];
        out[3] = (float)sigma;
    }
    for (int d = 0; d < kWmIdSymbols; d++) {
        const float* rd = row + (size_t)(1 + d) * kWmPeriod;
        wd_moments(rd, red, tid, &mean, &sigma);
        wd_grid_max(rd, o, kWmIdStep, kWmIdSymbolCount, bv, bi, tid);    // offset wd_id_offset(o, s)
        if (tid == 0) {
            out[4 + 2 * d] = (float)bi[0];
            out[5 + 2 * d] = sigma > 0.0 ? (float)(((double)bv[0] - mean) / sigma) : 0.0f;
        }
    }
}

struct WdWorkspace {
    WorkspaceUse use;
    RdClip* clips = nullptr; size_t cap_clips = 0;
    float* fw = nullptr; size_t cap_fw = 0;
    float* Z = nullptr; size_t cap_Z = 0;
    float* r = nullptr; size_t cap_r = 0;
    HostStage stage;
};

// The three launches f5hip_watermark_detect and f5hip_watermark_read_ids share, under the caller's name: the call's checks, then frame, fold
// and correlate over n_rows carrier rows -> ws.r [n][n_rows][P], ws.clips; then score(ws), the caller's own launch over them (an int, 0 =
// success), inside the same turn of the workspace
template <typename Score>
static int wd_correlate(const char* op, int32_t n, const float* wave_dev, const int64_t* offset, const int32_t* n_samples, int32_t n_rows,
                        const int16_t* carriers_dev, const float* out_dev, hipStream_t st, Score score) {
    std::vector<RdClip> h;
    long long rows = 0, total = 0;
    int bad = 0;
    switch (rd_layout(n, offset, n_samples, h, &rows, &total, &bad)) {
        case RD_OK: break;
        case RD_NO_CLIPS: return fail(-1, "%s: at least one clip (got %d)", op, n);
        case RD_NULL: return fail(-1, "%s: bad argument", op);
        case RD_LENGTH: return fail(-1, "%s: clip %d has %d samples (1 .. %d)", op, bad, n_samples[bad], kRdMaxSamples);
        case RD_OFFSET: return fail(-1, "%s: clip %d starts at %lld", op, bad, (long long)offset[bad]);
        case RD_OVERLAP: return fail(-1, "%s: clip %d overlaps another clip of the call", op, bad);
        default: return fail(-1, "%s: the clips of the call exceed 2^31 - 1 frames", op);
    }
    if (!wave_dev || !carriers_dev || !out_dev) return fail(-1, "%s: bad argument", op);
    if ((reinterpret_cast<uintptr_t>(wave_dev) & 3) || (reinterpret_cast<uintptr_t>(carriers_dev) & 15) || (reinterpret_cast<uintptr_t>(out_dev) & 3))
        return fail(-1, "%s: the carriers must be 16-byte aligned, the samples and the scores 4-byte", op);
    if ((n + kWdGroup - 1) / kWdGroup > 65535) return fail(-1, "%s: at most %d clips in a call", op, 65535 * kWdGroup);
    RdWorkspace* const tables = device_workspace<RdWorkspace>("watermark_detect");   // the window and the twiddles of the denoiser's FFT
    WdWorkspace* const wsp = device_workspace<WdWorkspace>("watermark_detect");
    if (!tables || !wsp) return -6;
    WdWorkspace& ws = *wsp;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(rd_tables(*tables));
    CK(dev_reserve(&ws.clips, &ws.cap_clips, (size_t)n, "watermark_detect clips"));
    CK(dev_reserve(&ws.fw, &ws.cap_fw, (size_t)rows * kRdNfft, "watermark_detect frames"));
    CK(dev_reserve(&ws.Z, &ws.cap_Z, (size_t)n * kWmPeriod, "watermark_detect folds"));
    CK(dev_reserve(&ws.r, &ws.cap_r, (size_t)n * n_rows * kWmPeriod, "watermark_detect correlations"));
    CK(ws.stage.upload(ws.clips, h.data(), sizeof(RdClip) * (size_t)n, st));   // pinned staging, queued on `stream`: no wait

    hipLaunchKernelGGL(wd_frame_kernel, dim3((unsigned)rows), dim3(256), 0, st, ws.clips, n, wave_dev, tables->window, tables->twiddle, ws.fw);
    CKL("wd_frame");
    hipLaunchKernelGGL(wd_fold_kernel, dim3(kWmPeriod / 256, (unsigned)n), dim3(256), 0, st, ws.clips, (const float*)ws.fw, ws.Z);
    CKL("wd_fold");
    hipLaunchKernelGGL(wd_corr_kernel, dim3(kWmPeriod / kWdOffTile, (unsigned)n_rows, (unsigned)((n + kWdGroup - 1) / kWdGroup)), dim3(256), 0, st, n,
                       n_rows, (const float*)ws.Z, (const short*)carriers_dev, ws.r);
    CKL("wd_corr");
    return score(ws);
}

int f5hip_watermark_detect(int32_t n, const float* wave_dev, const int64_t* offset, const int32_t* n_samples, int32_t n_keys,
                           const int16_t* carriers_dev, float* scores_dev, void* stream) {
    if (n_keys < 1 || n_keys > kWmKeysMax) return fail(-1, "watermark_detect: 1 .. %d keys in a call (got %d)", kWmKeysMax, n_keys);
    hipStream_t st = (hipStream_t)stream;
    CK(wd_correlate("watermark_detect", n, wave_dev, offset, n_samples, n_keys, carriers_dev, scores_dev, st, [&](WdWorkspace& ws) {
        hipLaunchKernelGGL(wd_score_kernel, dim3((unsigned)(n * n_keys)), dim3(256), 0, st, ws.clips, n_keys, (const float*)ws.r, scores_dev);
        CKL("wd_score");
        return 0;
    }));
    g_counters[CNT_WATERMARK_DETECT_LAUNCHES] += 4;
    g_counters[CNT_WATERMARK_DETECT_CLIPS] += n;
    return 0;
}

int f5hip_watermark_detect_launches(void) { return 4; }

int f5hip_watermark_read_ids(int32_t n, const float* wave_dev, const int64_t* offset, const int32_t* n_samples, int32_t n_keys,
                             const int16_t* carriers_dev, float* rows_dev, void* stream) {
    if (n_keys < 1 || n_keys > kWdIdKeysMax) return fail(-1, "watermark_read_ids: 1 .. %d keys in a call (got %d)", kWdIdKeysMax, n_keys);
    hipStream_t st = (hipStream_t)stream;
    CK(wd_correlate("watermark_read_ids", n, wave_dev, offset, n_samples, n_keys * kWmTagRows, carriers_dev, rows_dev, st, [&](WdWorkspace& ws) {
        hipLaunchKernelGGL(watermark_id_score_kernel, dim3((unsigned)(n * n_keys)), dim3(256), 0, st, ws.clips, n_keys, (const float*)ws.r, rows_dev);
        CKL("watermark_id_score");
        return 0;
    }));
    g_counters[CNT_WATERMARK_READ_IDS_LAUNCHES] += 4;
    g_counters[CNT_WATERMARK_READ_IDS_CLIPS] += n;
    return 0;
}

int f5hip_watermark_read_ids_launches(void) { return 4; }

// ------------------------------------------------------------------------------------------------ the scan of one long recording
static_assert(kWsNfft == kRdNfft && kWsHop == kRdHop && kWsPad == kRdPad && kWsFramesPerSample == kRdFramesPerSample,
              "watermark_scan: the ranges fold the frames wd_frame_kernel writes");
static_assert(kWsMaxSamples % kRdHop == 0 && (long long)(kWsMaxSamples / kRdHop + 3) * kRdNfft < (1LL << 31), "watermark_scan: a frame index fits an int");

// wd_fold_kernel for ranges of whole segments of ONE recording: one thread per (range, residue m).  ranges[i].off is the range's first
// sample (a multiple of P) and ranges[i].n its samples (ws_range_samples: nothing at or past the recording's end is read).  For the range's
// segments ascending, u[j] = its four frames added in ascending frame order, Z[m] = their sum in that order: the order is the range's alone,
// so its row does not depend on the other ranges of the call
__global__ __launch_bounds__(256) void ws_range_fold_kernel(const RdClip* __restrict__ ranges, const float* __restrict__ fw, float* __restrict__ Z) {
    const RdClip c = ranges[blockIdx.y];
    const int m = blockIdx.x * 256 + threadIdx.x;
    const long long end = c.off + c.n;
    float acc = 0.0f;
    for (int k = 0;; k++) {
        const long long j = ws_fold_sample(c.off, m, k);
        if (j >= end) break;
        const int f0 = ws_sample_frame0(j);
        float u = 0.0f;
#pragma unroll
        for (int d = 0; d < kWsFramesPerSample; d++) u += fw[(size_t)(f0 + d) * kWsNfft + ws_sample_offset(j, f0 + d)];
        acc += u;
    }
    Z[(size_t)blockIdx.y * kWmPeriod + m] = acc;
}

struct WsWorkspace {
    WorkspaceUse use;
    RdClip* table = nullptr; size_t cap_table = 0;                       // entry 0: the recording (wd_frame_kernel's clip), then the ranges
    HostStage stage;
};

// Launches: wd_frame_kernel and ws_range_fold_kernel once, then wd_corr_kernel and the score kernel once per slab of ws_slab_ranges(rows)
// ranges: 2 + 2 ws_slabs(n_ranges, rows), a function of (n_ranges, n_keys, with_ids) alone; a call of one slab launches four.
int f5hip_watermark_scan(const float* wave_dev, int64_t n_samples, int32_t n_ranges, const int32_t* first_segment, const int32_t* n_segments,
                         int32_t n_keys, int32_t with_ids, const int16_t* carriers_dev, float* rows_dev, void* stream) {
    const char* op = "watermark_scan";
    if (with_ids != 0 && with_ids != 1) return fail(-1, "%s: with_ids is 0 or 1 (got %d)", op, with_ids);
    const int keys_max = with_ids ? kWdIdKeysMax : kWmKeysMax;
    if (n_keys < 1 || n_keys > keys_max) return fail(-1, "%s: 1 .. %d keys in a call%s (got %d)", op, keys_max, with_ids ? " with ids" : "", n_keys);
    if (n_samples < 1 || n_samples > kWsMaxSamples) return fail(-1, "%s: the recording has %lld samples (1 .. %d)", op, (long long)n_samples, kWsMaxSamples);
    if (n_ranges < 1 || n_ranges > kWsRangesMax) return fail(-1, "%s: 1 .. %d ranges in a call (got %d)", op, kWsRangesMax, n_ranges);
    if (!wave_dev || !first_segment || !n_segments || !carriers_dev || !rows_dev) return fail(-1, "%s: bad argument", op);
    if ((reinterpret_cast<uintptr_t>(wave_dev) & 3) || (reinterpret_cast<uintptr_t>(carriers_dev) & 15) || (reinterpret_cast<uintptr_t>(rows_dev) & 3))
        return fail(-1, "%s: the carriers must be 16-byte aligned, the samples and the rows 4-byte", op);
    const int S = ws_segments(n_samples), F = ws_frames(n_samples);
    std::vector<RdClip> h((size_t)n_ranges + 1, RdClip());
    h[0].n = (int)n_samples; h[0].F = F;
    for (int i = 0; i < n_ranges; i++) {
        if (!ws_range_ok(n_samples, first_segment[i], n_segments[i]))
            return fail(-1, "%s: range %d is %d segments from segment %d of a recording of %d", op, i, n_segments[i], first_segment[i], S);
        h[(size_t)i + 1].off = ws_range_first(first_segment[i]);
        h[(size_t)i + 1].n = ws_range_samples(n_samples, first_segment[i], n_segments[i]);
    }
    const int rows_per_key = with_ids ? kWmTagRows : 1, n_rows = n_keys * rows_per_key, words = with_ids ? kWdIdRowWords : 4;
    const int per_slab = ws_slab_ranges(n_rows), slabs = ws_slabs(n_ranges, n_rows);
    RdWorkspace* const tables = device_workspace<RdWorkspace>("watermark_detect");   // the window and the twiddles of the denoiser's FFT
    WdWorkspace* const wdp = device_workspace<WdWorkspace>("watermark_detect");      // fw, Z and r are the detector's buffers
    WsWorkspace* const wsp = device_workspace<WsWorkspace>("watermark_scan");
    if (!tables || !wdp || !wsp) return -6;
    WdWorkspace& wd = *wdp;
    WsWorkspace& ws = *wsp;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn_wd(wd.use, st), turn(ws.use, st);
    CK(turn_wd.rc);
    CK(turn.rc);
    CK(rd_tables(*tables));
    CK(dev_reserve(&ws.table, &ws.cap_table, h.size(), "watermark_scan ranges"));
    CK(dev_reserve(&wd.fw, &wd.cap_fw, (size_t)F * kRdNfft, "watermark_scan frames"));
    CK(dev_reserve(&wd.Z, &wd.cap_Z, (size_t)n_ranges * kWmPeriod, "watermark_scan folds"));
    CK(dev_reserve(&wd.r, &wd.cap_r, (size_t)(n_ranges < per_slab ? n_ranges : per_slab) * n_rows * kWmPeriod, "watermark_scan correlations"));
    CK(ws.stage.upload(ws.table, h.data(), sizeof(RdClip) * h.size(), st));   // pinned staging, queued on `stream`: no wait
    const RdClip* ranges = ws.table + 1;

    hipLaunchKernelGGL(wd_frame_kernel, dim3((unsigned)F), dim3(256), 0, st, (const RdClip*)ws.table, 1, wave_dev, tables->window, tables->twiddle, wd.fw);
    CKL("wd_frame");
    hipLaunchKernelGGL(ws_range_fold_kernel, dim3(kWmPeriod / 256, (unsigned)n_ranges), dim3(256), 0, st, ranges, (const float*)wd.fw, wd.Z);
    CKL("ws_range_fold");
    for (int s = 0; s < slabs; s++) {
        const int r0 = s * per_slab, nr = n_ranges - r0 < per_slab ? n_ranges - r0 : per_slab;
        hipLaunchKernelGGL(wd_corr_kernel, dim3(kWmPeriod / kWdOffTile, (unsigned)n_rows, (unsigned)((nr + kWdGroup - 1) / kWdGroup)), dim3(256), 0, st, nr,
                           n_rows, (const float*)wd.Z + (size_t)r0 * kWmPeriod, (const short*)carriers_dev, wd.r);
        CKL("wd_corr");
        float* out = rows_dev + (size_t)r0 * n_keys * words;
        if (with_ids) {
            hipLaunchKernelGGL(watermark_id_score_kernel, dim3((unsigned)(nr * n_keys)), dim3(256), 0, st, ranges + r0, n_keys, (const float*)wd.r, out);
            CKL("watermark_id_score");
        } else {
            hipLaunchKernelGGL(wd_score_kernel, dim3((unsigned)(nr * n_keys)), dim3(256), 0, st, ranges + r0, n_keys, (const float*)wd.r, out);
            CKL("wd_score");
        }
    }
    g_counters[CNT_WATERMARK_SCAN_LAUNCHES] += 2 + 2 * slabs;
    g_counters[CNT_WATERMARK_SCAN_RANGES] += n_ranges;
    return 0;
}

int f5hip_watermark_scan_launches(void) { return 4; }

int f5hip_watermark_scan_slabs(int32_t n_ranges, int32_t n_keys, int32_t with_ids) {
    if (n_ranges < 1 || n_keys < 1 || n_keys > (with_ids ? kWdIdKeysMax : kWmKeysMax)) return fail(-1, "watermark_scan_slabs: bad argument");
    return ws_slabs(n_ranges, n_keys * (with_ids ? kWmTagRows : 1));
}
