// The per-voice denoiser of uploaded reference clips on the device: quantile-based noise estimation (Stahl, Fischer, Bippus 2000) with power
// spectral subtraction, for n clips of their own lengths in ONE call, in place on f5hip_ref_frontend's packed output.  Included at the end
// of f5hip.hip (same translation unit).  The definition is audio_prep.denoise_reference; the geometry is ref_denoise_core.h, which a host
// program compiles too.
//
//   rd_stft_kernel     one block per frame row of the packed batch (the clip by bisection of the first rows): the frame times
//                      w[i] = sin(pi i / 1024) through fft1024_lds; X float2 [rows][513], P = re^2 + im^2 [rows][516]
//   rd_floor_kernel    one block per (clip, 64 bins): floor[k] = the r-th smallest of the clip's P[.][k], exactly.  Non-negative floats order
//                      like their bit patterns, so the value is found bit by bit from the top: 31 counting passes, lanes across bins (coalesced
//                      rows of P), the clip's frames split over the block's waves, their counts added in LDS as integers
//   rd_gain_kernel     one block per frame row: S from the nine P cells in a fixed order, G = max(1/8, (S - 6.75 floor) / S), the Hermitian
//                      fill, fft1024_lds with sign +1, times w[i] / 1024 -> fw [rows][1024]
//   rd_ola_kernel      one thread per clip sample: its four frames added in ascending frame order, halved, written over the clip
// FOUR launches whatever n.  A clip's result depends on that clip alone: nothing is added across clips or in an order that depends on the
// batch, and the order statistic does not depend on any order of addition at all.
#pragma once
#include "ragged_util.h"
#include "ref_denoise_core.h"

constexpr int kRdFloorBins = 64;                                               // bins per block of the floor launch: one per lane
constexpr int kRdFloorChunks = (kRdBins + kRdFloorBins - 1) / kRdFloorBins;    // 9
constexpr int kRdFloorWaves = 16;                                              // waves per block of the floor launch: the clip's frames are split over them

__global__ __launch_bounds__(256) void rd_stft_kernel(const RdClip* __restrict__ clips, int n, const float* __restrict__ wave,
                                                      const float* __restrict__ window, const float2* __restrict__ tw, float2* __restrict__ X,
                                                      float* __restrict__ P) {
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
    for (int k = tid; k < kRdBins; k += 256) {
        const float2 v = s[k];
        X[(size_t)row * kRdBins + k] = v;
        P[(size_t)row * kRdPStride + k] = v.x * v.x + v.y * v.y;
    }
}

__global__ __launch_bounds__(kRdFloorWaves * 64) void rd_floor_kernel(const RdClip* __restrict__ clips, const float* __restrict__ P, float* __restrict__ floor_) {
    __shared__ int cnt[kRdFloorWaves][kRdFloorBins];
    const int ci = blockIdx.x / kRdFloorChunks, chunk = blockIdx.x % kRdFloorChunks;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const RdClip c = clips[ci];
    const int k = chunk * kRdFloorBins + lane;
    const bool live = k < kRdBins;
    const unsigned* col = reinterpret_cast<const unsigned*>(P) + (size_t)c.row0 * kRdPStride + (live ? k : 0);
    unsigned prefix = 0;                       // the bits of the answer found so far (those above `bit`)
    int r = rd_rank(c.F);                      // its rank among the values that share them
    for (int bit = 30; bit >= 0; bit--) {
        const unsigned want = prefix >> bit;   // a candidate with a 0 at `bit`: v >> bit == prefix >> bit
        int zeros = 0;
        if (live)
            for (int m = wv; m < c.F; m += kRdFloorWaves) zeros += (col[(size_t)m * kRdPStride] >> bit) == want ? 1 : 0;
        cnt[wv][lane] = zeros;
        __syncthreads();
        int total = 0;
#pragma unroll
        for (int w = 0; w < kRdFloorWaves; w++) total += cnt[w][lane];
        __syncthreads();
        if (r >= total) { r -= total; prefix |= 1u << bit; }
    }
    if (live && wv == 0) floor_[(size_t)ci * kRdPStride + k] = __uint_as_float(prefix);
}

__global__ __launch_bounds__(256) void rd_gain_kernel(const RdClip* __restrict__ clips, int n, const float2* __restrict__ X, const float* __restrict__ P,
                                                      const float* __restrict__ floor_, const float* __restrict__ window,
                                                      const float2* __restrict__ tw, float* __restrict__ fw) {
    __shared__ float2 s[kRdNfft];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int ci = last_at_or_before<&RdClip::row0>(clips, n, row);
    const RdClip c = clips[ci];
    const int m = row - c.row0;
    const float* Pc = P + (size_t)c.row0 * kRdPStride;
    for (int k = tid; k < kRdBins; k += 256) {
        float S = 0.0f;
        for (int dm = -1; dm <= 1; dm++) {
            const float* pr = Pc + (size_t)rd_clamp(m + dm, c.F) * kRdPStride;
            for (int dk = -1; dk <= 1; dk++) S += pr[rd_clamp(k + dk, kRdBins)];
        }
        S = S / 9.0f;
        const float G = S > 0.0f ? fmaxf(kRdMinGain, (S - kRdSubtract * floor_[(size_t)ci * kRdPStride + k]) / S) : kRdMinGain;
        const float2 v = X[(size_t)row * kRdBins + k];
        const float re = G * v.x, im = (k == 0 || k == kRdNfft / 2) ? 0.0f : G * v.y;   // irfft ignores the imaginary part of DC / Nyquist
        s[__brev((unsigned)k) >> 22] = make_float2(re, im);
        if (k > 0 && k < kRdNfft / 2) s[__brev((unsigned)(kRdNfft - k)) >> 22] = make_float2(re, -im);
    }
    fft1024_lds(s, tw, tid, 1.0f);
    for (int i = tid; i < kRdNfft; i += 256) fw[(size_t)row * kRdNfft + i] = s[i].x * (window[i] * (1.0f / kRdNfft));
}

__global__ __launch_bounds__(256) void rd_ola_kernel(const RdClip* __restrict__ clips, int n, long long total, const float* __restrict__ fw,
                                                     float* __restrict__ wave) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const RdClip c = clips[last_at_or_before<&RdClip::out0>(clips, n, g)];
    const long long j = g - c.out0;
    const int m0 = rd_sample_frame0(j);
    float acc = 0.0f;
#pragma unroll
    for (int d = 0; d < kRdFramesPerSample; d++) acc += fw[(size_t)(c.row0 + m0 + d) * kRdNfft + rd_sample_offset(j, m0 + d)];
    wave[c.off + j] = 0.5f * acc;
}

struct RdWorkspace {
    RdClip* clips = nullptr; size_t cap_clips = 0;
    float2* X = nullptr; size_t cap_X = 0;
    float* P = nullptr; size_t cap_P = 0;
    float* fw = nullptr; size_t cap_fw = 0;
    float* floor_ = nullptr; size_t cap_floor = 0;
    float* window = nullptr;        // sin(pi i / 1024): the square root of the periodic Hann window
    float2* twiddle = nullptr;
    HostStage stage;
    WorkspaceUse use;               // of the denoiser's own buffers; window and twiddle never change once built, and their readers take no turn
};

static int rd_tables(RdWorkspace& ws) {
    if (ws.window && ws.twiddle) return 0;
    std::vector<float> w(kRdNfft);
    std::vector<float2> tw(kRdNfft / 2);
    for (int i = 0; i < kRdNfft; i++) w[i] = (float)sin(M_PI * (double)i / (double)kRdNfft);
    for (int k = 0; k < kRdNfft / 2; k++) {
        tw[k].x = (float)cos(2.0 * M_PI * (double)k / (double)kRdNfft);
        tw[k].y = (float)sin(2.0 * M_PI * (double)k / (double)kRdNfft);
    }
    if (!ws.window && upload_f32(&ws.window, w.data(), w.size())) return -4;
    if (!ws.twiddle) {
        if (hipMalloc((void**)&ws.twiddle, sizeof(float2) * tw.size()) != hipSuccess) { ws.twiddle = nullptr; return fail(-4, "hipMalloc twiddle"); }
        if (hipMemcpy(ws.twiddle, tw.data(), sizeof(float2) * tw.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(-4, "H2D twiddle");
    }
    return 0;
}

int f5hip_ref_denoise(int32_t n, const int64_t* offset, const int32_t* n_samples, float* wave_dev, void* stream) {
    std::vector<RdClip> h;
    long long rows = 0, total = 0;
    int bad = 0;
    switch (rd_layout(n, offset, n_samples, h, &rows, &total, &bad)) {
        case RD_OK: break;
        case RD_NO_CLIPS: return fail(-1, "ref_denoise: at least one clip (got %d)", n);
        case RD_NULL: return fail(-1, "ref_denoise: bad argument");
        case RD_LENGTH: return fail(-1, "ref_denoise: clip %d has %d samples (1 .. %d)", bad, n_samples[bad], kRdMaxSamples);
        case RD_OFFSET: return fail(-1, "ref_denoise: clip %d starts at %lld", bad, (long long)offset[bad]);
        case RD_OVERLAP: return fail(-1, "ref_denoise: clip %d overlaps another clip of the call", bad);
        default: return fail(-1, "ref_denoise: the clips of the call exceed 2^31 - 1 frames");
    }
    if (!wave_dev) return fail(-1, "ref_denoise: bad argument");
    RdWorkspace* const wsp = device_workspace<RdWorkspace>("ref_denoise");
    if (!wsp) return -6;
    RdWorkspace& ws = *wsp;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(rd_tables(ws));
    CK(dev_reserve(&ws.clips, &ws.cap_clips, (size_t)n, "ref_denoise clips"));
    CK(dev_reserve(&ws.X, &ws.cap_X, (size_t)rows * kRdBins, "ref_denoise spectra"));
    CK(dev_reserve(&ws.P, &ws.cap_P, (size_t)rows * kRdPStride, "ref_denoise powers"));
    CK(dev_reserve(&ws.fw, &ws.cap_fw, (size_t)rows * kRdNfft, "ref_denoise frames"));
    CK(dev_reserve(&ws.floor_, &ws.cap_floor, (size_t)n * kRdPStride, "ref_denoise noise floors"));
    CK(ws.stage.upload(ws.clips, h.data(), sizeof(RdClip) * (size_t)n, st));   // pinned staging, queued on `stream`: no wait

    hipLaunchKernelGGL(rd_stft_kernel, dim3((unsigned)rows), dim3(256), 0, st, ws.clips, n, wave_dev, ws.window, ws.twiddle, ws.X, ws.P);
    CKL("rd_stft");
    hipLaunchKernelGGL(rd_floor_kernel, dim3((unsigned)n * kRdFloorChunks), dim3(kRdFloorWaves * 64), 0, st, ws.clips, ws.P, ws.floor_);
    CKL("rd_floor");
    hipLaunchKernelGGL(rd_gain_kernel, dim3((unsigned)rows), dim3(256), 0, st, ws.clips, n, ws.X, ws.P, ws.floor_, ws.window, ws.twiddle, ws.fw);
    CKL("rd_gain");
    hipLaunchKernelGGL(rd_ola_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ws.clips, n, total, ws.fw, wave_dev);
    CKL("rd_ola");
    g_counters[CNT_REF_DENOISE_LAUNCHES] += 4;
    g_counters[CNT_REF_DENOISE_CLIPS] += n;
    return 0;
}
