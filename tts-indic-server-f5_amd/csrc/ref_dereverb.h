// The per-voice dereverberator of uploaded reference clips on the device: weighted prediction error (WPE; Nakatani, Yoshioka, Kinoshita,
// Miyoshi, Juang 2010), a delayed linear prediction fitted and subtracted per frequency bin, for n clips of their own lengths in ONE call, in
// place on f5hip_ref_frontend's packed output.  Included at the end of f5hip.hip (same translation unit).  The definition is
// audio_prep.dereverb_reference; the geometry is ref_dereverb_core.h, which a host program compiles too.
//
//   rd_stft_kernel      ref_denoise.h's, as it stands: X float2 [rows][513], P = |X|^2 [rows][516]
//   rv_wpe_kernel       one workgroup per (clip, 8 bins), one wave per bin, all three iterations: a bin's problem touches no other bin, so
//                       its Gram matrix, right-hand side and filter never leave the CU, and only the Y plane goes through memory
//       floor           1e-3 mean_f P + 1e-20: lanes over frames, a fixed butterfly over the lanes
//       Gram            frames in chunks of kRvChunk, ascending.  The wave stages its bin's X over the chunk and the 19 frames in front of it in
//                       LDS once; x~ is a delay line, so all 16 taps of a frame are 16 neighbouring slots.  With U = [Re x~ | Im x~] (32 real
//                       columns) U^T diag(1 / lam) U holds every block of the Hermitian R: one v_mfma_f32_32x32x2_f32 per two frames, lane
//                       (column c, frame parity h) feeding U[f][c] / lam[f] and U[f][c], fp32 operands, the 32 x 32 accumulator carried in
//                       registers over the clip's chunks.  p rides along on the VALU: the same lane's U / lam times Re X[f] and Im X[f]
//       solve           R = Re-Re + Im-Im + i (Im-Re - Re-Im) blocks, the diagonal load, then a 16 x 16 complex Cholesky factorisation and the
//                       two triangular solves in the wave's LDS
//       filter          Y[f] = X[f] - sum_j conj(g_j) x~_j[f], lanes over the chunk's frames, taps from the staged delay line, j ascending
//   rv_inverse_kernel   one block per frame row: the Hermitian fill of Y, fft1024_lds with sign +1, times w[i] / 1024 -> fw [rows][1024]
//   rd_ola_kernel       ref_denoise.h's, as it stands
// FOUR launches whatever n.  A clip's result depends on that clip alone: a wave adds its bin's frames in ascending order in one accumulator,
// so nothing is added across clips or in an order that depends on the batch.
#pragma once
#include "ref_denoise.h"
#include "ref_dereverb_core.h"

typedef float rv_acc16 __attribute__((ext_vector_type(16)));

struct RvWave {                              // one wave's LDS: its bin's staged chunk and its 16 x 16 system
    float2 xs[kRvStage];                     // X of frames base - 19 .. base + kRvChunk - 1
    float ps[kRvPow];                        // |Y|^2 of frames base - 1 .. base + kRvChunk, clamped to the clip
    float w[kRvChunk];                       // 1 / lam, 0 past the clip's last frame
    union {
        float G[kRvCols][kRvCols + 1];       // U^T diag(1 / lam) U
        struct { float re[kRvTaps][kRvTaps + 1], im[kRvTaps][kRvTaps + 1]; } L;   // R, then its Cholesky factor (lower triangle)
    } m;
    float pp[2][64];                         // per lane: sum U / lam Re X, sum U / lam Im X
    float2 b[kRvTaps];                       // p, then the forward solve's y
    float2 g[kRvTaps];
};
static_assert(sizeof(RvWave) * kRvGroupBins <= 64 * 1024, "rv_wpe_kernel's static LDS");
static_assert(kRvChunk % 2 == 0 && kRvCols == 32, "one 32x32x2 MFMA takes two frames of 32 columns");

F5_DEVICE void rv_stage(RvWave& s, const float2* __restrict__ Xc, int base, int F, int lane) {
    for (int q = lane; q < kRvStage; q += 64) {
        const int f = rv_stage_frame(base, q);
        s.xs[q] = f >= 0 && f < F ? Xc[(size_t)f * kRdBins] : make_float2(0.0f, 0.0f);
    }
}

__global__ __launch_bounds__(kRvGroupBins * 64) void rv_wpe_kernel(const RdClip* __restrict__ clips, const float2* __restrict__ X,
                                                                   const float* __restrict__ P, float2* Y) {
    __shared__ RvWave lds[kRvGroupBins];
    const int ci = blockIdx.x / kRvGroups, grp = blockIdx.x % kRvGroups;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const RdClip c = clips[ci];
    const bool live = grp * kRvGroupBins + wv < kRdBins;
    // a wave past the last bin works on the last bin's X and writes nothing, so every barrier below is met by the whole workgroup
    const int k = live ? grp * kRvGroupBins + wv : kRdBins - 1;
    RvWave& s = lds[wv];
    const float2* Xc = X + (size_t)c.row0 * kRdBins + k;
    float2* Yc = Y + (size_t)c.row0 * kRdBins + k;
    const int F = c.F, chunks = rv_chunks(F);
    const int col = lane & 31, half = lane >> 5, tap = col & (kRvTaps - 1);
    const bool imag = col >= kRvTaps;

    float sum = 0.0f;
    for (int m = lane; m < F; m += 64) sum += P[(size_t)(c.row0 + m) * kRdPStride + k];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    const float floor_ = kRvFloorRel * (sum / (float)F) + kRvTiny;

    for (int it = 0; it < kRvIters; it++) {
        const float2* Ys = it > 0 && live ? Yc : Xc;          // the first iteration starts from Y = X
        rv_acc16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.0f;
        float pre = 0.0f, pim = 0.0f;
        for (int ch = 0; ch < chunks; ch++) {
            const int base = ch * kRvChunk, frames = min(kRvChunk, F - base);
            rv_stage(s, Xc, base, F, lane);
            for (int q = lane; q < kRvPow; q += 64) {
                const float2 v = Ys[(size_t)rv_pow_frame(base, q, F) * kRdBins];
                s.ps[q] = v.x * v.x + v.y * v.y;
            }
            __syncthreads();
            for (int t = lane; t < kRvChunk; t += 64)
                s.w[t] = t < frames ? 1.0f / fmaxf((s.ps[t] + s.ps[t + 1] + s.ps[t + 2]) / 3.0f, floor_) : 0.0f;
            __syncthreads();
            for (int t0 = 0; t0 < frames; t0 += 2) {
                const int t = t0 + half;
                const float2 xv = s.xs[rv_tap_slot(t, tap)], own = s.xs[rv_own_slot(t)];
                const float u = imag ? xv.y : xv.x, a = u * s.w[t];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, u, acc, 0, 0, 0);
                pre = fmaf(a, own.x, pre);
                pim = fmaf(a, own.y, pim);
            }
            __syncthreads();
        }

        // accumulator register r of lane (col, half) is row 8 (r / 4) + 4 half + r % 4, column col
#pragma unroll
        for (int r = 0; r < 16; r++) s.m.G[8 * (r / 4) + 4 * half + (r % 4)][col] = acc[r];
        s.pp[0][lane] = pre;
        s.pp[1][lane] = pim;
        __syncthreads();
        float rr[4], ri[4], tr = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int a = (lane + 64 * q) >> 4, b = lane & 15;
            rr[q] = s.m.G[a][b] + s.m.G[a + kRvTaps][b + kRvTaps];
            ri[q] = s.m.G[a + kRvTaps][b] - s.m.G[a][b + kRvTaps];
        }
        for (int a = 0; a < kRvTaps; a++) tr += s.m.G[a][a] + s.m.G[a + kRvTaps][a + kRvTaps];
        const float load = kRvLoadRel * tr / (float)kRvTaps + kRvTiny;
        float2 p = make_float2(0.0f, 0.0f);
        if (lane < kRvTaps) {      // p_j = sum x~_j conj(X) / lam: the two frame parities of the Re column and of the Im column
            p.x = (s.pp[0][lane] + s.pp[0][lane + 32]) + (s.pp[1][lane + 16] + s.pp[1][lane + 48]);
            p.y = (s.pp[0][lane + 16] + s.pp[0][lane + 48]) - (s.pp[1][lane] + s.pp[1][lane + 32]);
        }
        __syncthreads();           // G is read; R takes its place
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int a = (lane + 64 * q) >> 4, b = lane & 15;
            s.m.L.re[a][b] = a == b ? rr[q] + load : rr[q];
            s.m.L.im[a][b] = a == b ? 0.0f : ri[q];
        }
        if (lane < kRvTaps) s.b[lane] = p;
        __syncthreads();

        for (int kk = 0; kk < kRvTaps; kk++) {                 // R = L L^H, column by column
            const float d = sqrtf(s.m.L.re[kk][kk]);
            __syncthreads();
            if (lane == kk) s.m.L.re[kk][kk] = d;
            else if (lane > kk && lane < kRvTaps) { s.m.L.re[lane][kk] /= d; s.m.L.im[lane][kk] /= d; }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = (lane + 64 * q) >> 4, j = lane & 15;
                if (j > kk && i >= j) {
                    const float ar = s.m.L.re[i][kk], ai = s.m.L.im[i][kk], br = s.m.L.re[j][kk], bi = s.m.L.im[j][kk];
                    s.m.L.re[i][j] -= ar * br + ai * bi;
                    s.m.L.im[i][j] -= ai * br - ar * bi;
                }
            }
            __syncthreads();
        }
        for (int kk = 0; kk < kRvTaps; kk++) {                 // L y = p
            const float d = s.m.L.re[kk][kk];
            const float2 y = make_float2(s.b[kk].x / d, s.b[kk].y / d);
            __syncthreads();
            if (lane == kk) s.b[kk] = y;
            else if (lane > kk && lane < kRvTaps) {
                const float lr = s.m.L.re[lane][kk], li = s.m.L.im[lane][kk];
                s.b[lane].x -= lr * y.x - li * y.y;
                s.b[lane].y -= lr * y.y + li * y.x;
            }
            __syncthreads();
        }
        for (int kk = kRvTaps - 1; kk >= 0; kk--) {            // L^H g = y
            const float d = s.m.L.re[kk][kk];
            const float2 gk = make_float2(s.b[kk].x / d, s.b[kk].y / d);
            __syncthreads();
            if (lane == kk) s.g[kk] = gk;
            else if (lane < kk) {
                const float lr = s.m.L.re[kk][lane], li = s.m.L.im[kk][lane];
                s.b[lane].x -= lr * gk.x + li * gk.y;
                s.b[lane].y -= lr * gk.y - li * gk.x;
            }
            __syncthreads();
        }

        for (int ch = 0; ch < chunks; ch++) {                  // Y = X - g^H x~
            const int base = ch * kRvChunk, frames = min(kRvChunk, F - base);
            rv_stage(s, Xc, base, F, lane);
            __syncthreads();
            for (int t = lane; t < frames; t += 64) {
                float2 e = make_float2(0.0f, 0.0f);
#pragma unroll
                for (int j = 0; j < kRvTaps; j++) {
                    const float2 g = s.g[j], x = s.xs[rv_tap_slot(t, j)];
                    e.x += g.x * x.x + g.y * x.y;
                    e.y += g.x * x.y - g.y * x.x;
                }
                const float2 own = s.xs[rv_own_slot(t)];
                if (live) Yc[(size_t)(base + t) * kRdBins] = make_float2(own.x - e.x, own.y - e.y);
            }
            __syncthreads();       // the staged chunk is read, and this workgroup's Y is visible to its next iteration
        }
    }
}

__global__ __launch_bounds__(256) void rv_inverse_kernel(const float2* __restrict__ Y, const float* __restrict__ window,
                                                         const float2* __restrict__ tw, float* __restrict__ fw) {
    __shared__ float2 s[kRdNfft];
    const int row = blockIdx.x, tid = threadIdx.x;
    for (int k = tid; k < kRdBins; k += 256) {
        const float2 v = Y[(size_t)row * kRdBins + k];
        const float im = (k == 0 || k == kRdNfft / 2) ? 0.0f : v.y;   // irfft ignores the imaginary part of DC / Nyquist
        s[__brev((unsigned)k) >> 22] = make_float2(v.x, im);
        if (k > 0 && k < kRdNfft / 2) s[__brev((unsigned)(kRdNfft - k)) >> 22] = make_float2(v.x, -im);
    }
    fft1024_lds(s, tw, tid, 1.0f);
    for (int i = tid; i < kRdNfft; i += 256) fw[(size_t)row * kRdNfft + i] = s[i].x * (window[i] * (1.0f / kRdNfft));
}

struct RvWorkspace {
    RdWorkspace rd;                 // clips, X, P, fw, the tables, the staging and the turn: the denoiser's fields, this call's own buffers
    float2* Y = nullptr; size_t cap_Y = 0;
};

int f5hip_ref_dereverb_launches(void) { return 4; }
int f5hip_ref_dereverb_chunk(void) { return kRvChunk; }

int f5hip_ref_dereverb(int32_t n, const int64_t* offset, const int32_t* n_samples, float* wave_dev, void* stream) {
    std::vector<RdClip> h;
    long long rows = 0, total = 0;
    int bad = 0;
    switch (rv_layout(n, offset, n_samples, h, &rows, &total, &bad)) {
        case RD_OK: break;
        case RD_NO_CLIPS: return fail(-1, "ref_dereverb: at least one clip (got %d)", n);
        case RD_NULL: return fail(-1, "ref_dereverb: bad argument");
        case RD_LENGTH: return fail(-1, "ref_dereverb: clip %d has %d samples (1 .. %d)", bad, n_samples[bad], kRdMaxSamples);
        case RD_OFFSET: return fail(-1, "ref_dereverb: clip %d starts at %lld", bad, (long long)offset[bad]);
        case RD_OVERLAP: return fail(-1, "ref_dereverb: clip %d overlaps another clip of the call", bad);
        default: return fail(-1, "ref_dereverb: the clips of the call exceed 2^31 - 1 frames");
    }
    if (!wave_dev) return fail(-1, "ref_dereverb: bad argument");
    RvWorkspace* const wsp = device_workspace<RvWorkspace>("ref_dereverb");
    if (!wsp) return -6;
    RdWorkspace& ws = wsp->rd;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(rd_tables(ws));
    CK(dev_reserve(&ws.clips, &ws.cap_clips, (size_t)n, "ref_dereverb clips"));
    CK(dev_reserve(&ws.X, &ws.cap_X, (size_t)rows * kRdBins, "ref_dereverb spectra"));
    CK(dev_reserve(&ws.P, &ws.cap_P, (size_t)rows * kRdPStride, "ref_dereverb powers"));
    CK(dev_reserve(&ws.fw, &ws.cap_fw, (size_t)rows * kRdNfft, "ref_dereverb frames"));
    CK(dev_reserve(&wsp->Y, &wsp->cap_Y, (size_t)rows * kRdBins, "ref_dereverb filtered spectra"));
    CK(ws.stage.upload(ws.clips, h.data(), sizeof(RdClip) * (size_t)n, st));   // pinned staging, queued on `stream`: no wait

    hipLaunchKernelGGL(rd_stft_kernel, dim3((unsigned)rows), dim3(256), 0, st, ws.clips, n, wave_dev, ws.window, ws.twiddle, ws.X, ws.P);
    CKL("rd_stft");
    hipLaunchKernelGGL(rv_wpe_kernel, dim3((unsigned)n * kRvGroups), dim3(kRvGroupBins * 64), 0, st, ws.clips, ws.X, ws.P, wsp->Y);
    CKL("rv_wpe");
    hipLaunchKernelGGL(rv_inverse_kernel, dim3((unsigned)rows), dim3(256), 0, st, wsp->Y, ws.window, ws.twiddle, ws.fw);
    CKL("rv_inverse");
    hipLaunchKernelGGL(rd_ola_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ws.clips, n, total, ws.fw, wave_dev);
    CKL("rd_ola");
    g_counters[CNT_REF_DEREVERB_LAUNCHES] += 4;
    g_counters[CNT_REF_DEREVERB_CLIPS] += n;
    return 0;
}
