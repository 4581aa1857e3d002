// Vocos (vocos 0.1.0, charactr/vocos-mel-24khz geometry) mel -> waveform decoder and the torchaudio-style
// mel front-end, on the same GEMM / LayerNorm kernels as the DiT plus LDS radix-2 FFT kernels for
// iSTFT / STFT.  Included at the end of f5hip.hip (same translation unit).
//
// decode(mel[B,100,T]), or a ragged batch of items with their own T (decode_ragged: one packed row space):
//   x = Conv1d(100->512,k7,p3)(mel) -> LN -> 8 x [dwconv k7 -> LN -> 512->1536 -> GELU(erf) -> 1536->512 -> gamma* -> +res]
//   -> LN -> Linear(512->1026) -> (mag = min(exp(.),1e2), phase) -> irfft(1024) * hann -> overlap-add / envelope
#pragma once
#include "ragged_util.h"

struct VocosBlock {
    float *dw_w = nullptr, *dw_b = nullptr, *ln_w = nullptr, *ln_b = nullptr, *gamma = nullptr;
    PackedW pw1, pw2;
};

struct f5hip_vocos {
    f5hip_vocos_config cfg;
    int nsplit = 2;
    ParamStore params;
    bool finalized = false;
    PackedW embed, head;
    float *norm_w = nullptr, *norm_b = nullptr, *fnorm_w = nullptr, *fnorm_b = nullptr;
    std::vector<VocosBlock> blk;
    float* window = nullptr;     // periodic hann [n_fft]
    float2* twiddle = nullptr;   // (cos, sin)(2 pi k / n_fft), k < n_fft/2
    // workspace
    int cap_rows = 0;
    void* ws = nullptr;
    float *x = nullptr, *y = nullptr, *fw = nullptr;
    Plane2 melp, tn, hid;
    int* meta = nullptr;
    size_t cap_meta = 0;   // ints in meta
};

// ---------------------------------------------------------------------------------------- FFT in LDS
// In-place radix-2 decimation-in-time FFT of 1024 complex points held in LDS in bit-reversed order.
// sign = +1: sum_k X[k] e^{+2 pi i k n / N} (inverse, unnormalised); sign = -1: forward.  256 threads.
F5_DEVICE void fft1024_lds(float2* s, const float2* __restrict__ tw, int tid, float sign) {
#pragma unroll 1
    for (int stage = 0; stage < 10; stage++) {
        const int half = 1 << stage;
        __syncthreads();
#pragma unroll
        for (int b = tid; b < 512; b += 256) {
            const int grp = b >> stage, pos = b & (half - 1);
            const int i0 = (grp << (stage + 1)) + pos, i1 = i0 + half;
            float2 w = tw[pos << (9 - stage)];
            w.y *= sign;
            const float2 a = s[i0], c = s[i1];
            const float tx = c.x * w.x - c.y * w.y, ty = c.x * w.y + c.y * w.x;
            s[i0] = make_float2(a.x + tx, a.y + ty);
            s[i1] = make_float2(a.x - tx, a.y - ty);
        }
    }
    __syncthreads();
}

// mel [B][C][T] fp32 -> rows (frame-major) split bf16 [M_pad][128]
__global__ __launch_bounds__(128) void mel_to_rows_kernel(const float* mel, int C, int T, const int* row_seq, const int* row_pos,
                                                          int M, __bf16* hi, __bf16* lo) {
    const int row = blockIdx.x, c = threadIdx.x;
    if (row >= M) return;
    const int b = row_seq[row];
    float v = 0.0f;
    if (b >= 0 && c < C) v = mel[((size_t)b * C + c) * T + row_pos[row]];
    __bf16 h, l;
    split_bf16(v, h, l);
    hi[(size_t)row * 128 + c] = h;
    lo[(size_t)row * 128 + c] = l;
}

// ISTFT head, per frame: y[row] = [log-mag (513) | phase (513)] -> windowed irfft frame fw[row][1024]
__global__ __launch_bounds__(256) void istft_frame_kernel(const float* y, int ldy, const int* row_seq, int M, const float* window,
                                                          const float2* tw, float* fw) {
    __shared__ float2 s[1024];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= M || row_seq[row] < 0) return;
    const float* yr = y + (size_t)row * ldy;
    for (int k = tid; k <= 512; k += 256) {
        float mag = fminf(expf(yr[k]), 100.0f);   // torch.clip(exp(mag), max=1e2)
        const float ph = yr[513 + k];
        float re = mag * cosf(ph), im = mag * sinf(ph);
        if (k == 0 || k == 512) im = 0.0f;        // irfft ignores the imaginary part of DC / Nyquist
        s[__brev((unsigned)k) >> 22] = make_float2(re, im);
        if (k > 0 && k < 512) s[__brev((unsigned)(1024 - k)) >> 22] = make_float2(re, -im);
    }
    fft1024_lds(s, tw, tid, 1.0f);
    for (int n = tid; n < 1024; n += 256) fw[(size_t)row * 1024 + n] = s[n].x * (1.0f / 1024.0f) * window[n];
}

// overlap-add + window-envelope normalisation + centre trim (torch.istft, center=True), per item of a packed batch: item b has T_b = item_T[b]
// frames starting at row seq_row0[b] and owns out[item_out0[b] .. item_out0[b + 1]) = hop * (T_b - 1) samples.  One thread per output
// sample over the packed output; the item is found by bisection of item_out0 [n + 1].
__global__ __launch_bounds__(256) void istft_ola_kernel(const float* fw, const int* seq_row0, const int* item_T, const int* item_out0, int n,
                                                        int hop, const float* window, float* out) {
    const int gidx = blockIdx.x * 256 + threadIdx.x;
    if (gidx >= item_out0[n]) return;
    int lo = 0, hi = n - 1;                        // last item whose output starts at or before gidx
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (item_out0[mid] <= gidx) lo = mid; else hi = mid - 1;
    }
    const int b = lo, T = item_T[b];
    const int sidx = gidx - item_out0[b];
    const int p = sidx + 512;
    int t_hi = p / hop; if (t_hi > T - 1) t_hi = T - 1;
    int t_lo = (p - 1023 + hop - 1) / hop; if (t_lo < 0) t_lo = 0;
    float val = 0.0f, env = 0.0f;
    for (int t = t_lo; t <= t_hi; t++) {
        const int n_ = p - t * hop;
        val += fw[(size_t)(seq_row0[b] + t) * 1024 + n_];
        env += window[n_] * window[n_];
    }
    out[gidx] = val / env;
}

// One frame of the mel front-ends, by a block of 256 threads: frame t of the wave w [nw] -> out[m * stride], m < n_mels.  The two kernels
// below differ only in where a block finds its wave and puts its row, so an item's frame has the same bits from either.
F5_DEVICE void mel_frame(float2* s /*[1024] LDS*/, float* mag /*[520] LDS*/, const float* w, int nw, int t, int hop, int n_mels, const float* window,
                         const float2* tw, const float* fb /*[513][n_mels]*/, float* out, size_t stride, int pad, float mag_eps) {
    const int tid = threadIdx.x;
    for (int n = tid; n < 1024; n += 256) {
        int idx = t * hop - pad + n;               // reflect padding by `pad` samples on both sides
        if (idx < 0) idx = -idx;
        if (idx >= nw) idx = 2 * (nw - 1) - idx;
        s[__brev((unsigned)n) >> 22] = make_float2(w[idx] * window[n], 0.0f);
    }
    fft1024_lds(s, tw, tid, -1.0f);
    for (int k = tid; k <= 512; k += 256) mag[k] = sqrtf(s[k].x * s[k].x + s[k].y * s[k].y + mag_eps);   // power = 1
    __syncthreads();
    if (tid < n_mels) {
        float acc = 0.0f;
        for (int k = 0; k <= 512; k++) acc += fb[k * n_mels + tid] * mag[k];
        // log(clamp(acc, 1e-5)), clamped on the log side: the device logf is ~2 ulp (1.6e-6) off at 1e-5, and silent bins are to hold the
        // fp32 value of log(1e-5) that the reference's front-end produces
        out[(size_t)tid * stride] = fmaxf(logf(acc), -11.512925148f);
    }
}

// STFT magnitude -> HTK mel filterbank -> log(clamp(., 1e-5)); one block per (frame, batch); mel [batch][n_mels][T]
__global__ __launch_bounds__(256) void mel_frame_kernel(const float* wave, int nw, int T, int hop, int n_mels, const float* window,
                                                        const float2* tw, const float* fb /*[513][n_mels]*/, float* mel, int pad, float mag_eps) {
    __shared__ float2 s[1024];
    __shared__ float mag[520];
    const int t = blockIdx.x, b = blockIdx.y;
    mel_frame(s, mag, wave + (size_t)b * nw, nw, t, hop, n_mels, window, tw, fb, mel + (size_t)b * n_mels * T + t, (size_t)T, pad, mag_eps);
}

// The same for n clips of their own lengths in one launch (f5hip_mel_spectrogram_ragged): one block per frame of the packed output
// mel [sum T][n_mels] (frame-major: the sampler's cond layout); the block finds its clip by bisection of the clips' first rows.  Each clip
// is read through its own pointer and reflect-padded at its own bounds.
struct MelItem { const float* w; int nw, row0; };   // a clip, its samples, its first row of the packed output
__global__ __launch_bounds__(256) void mel_frame_ragged_kernel(const MelItem* __restrict__ items, int n, int hop, int n_mels, const float* window,
                                                               const float2* tw, const float* fb, float* mel, int pad, float mag_eps) {
    __shared__ float2 s[1024];
    __shared__ float mag[520];
    const int row = blockIdx.x;
    const MelItem it = items[last_at_or_before<&MelItem::row0>(items, n, row)];
    mel_frame(s, mag, it.w, it.nw, row - it.row0, hop, n_mels, window, tw, fb, mel + (size_t)row * n_mels, 1, pad, mag_eps);
}

// ---------------------------------------------------------------------------------------- host side
static int make_fft_tables(float** window, float2** twiddle, int n_fft) {
    std::vector<float> w(n_fft);
    std::vector<float2> tw(n_fft / 2);
    for (int n = 0; n < n_fft; n++) w[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)n / (double)n_fft));   // periodic hann
    for (int k = 0; k < n_fft / 2; k++) {
        tw[k].x = (float)cos(2.0 * M_PI * (double)k / (double)n_fft);
        tw[k].y = (float)sin(2.0 * M_PI * (double)k / (double)n_fft);
    }
    if (upload_f32(window, w.data(), w.size())) return -4;
    if (hipMalloc((void**)twiddle, sizeof(float2) * tw.size()) != hipSuccess) return fail(-4, "hipMalloc twiddle");
    if (hipMemcpy(*twiddle, tw.data(), sizeof(float2) * tw.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(-4, "H2D twiddle");
    return 0;
}

f5hip_vocos* f5hip_vocos_create(const f5hip_vocos_config* cfg) {
    if (!cfg) { set_error("null config"); return nullptr; }
    if (cfg->n_fft != 1024 || cfg->hop_length != 256 || cfg->in_channels > 128 || cfg->dim % 128 || cfg->intermediate_dim % 128 ||
        (cfg->gemm_planes != 1 && cfg->gemm_planes != 2)) {
        set_error("unsupported Vocos geometry (need n_fft 1024, hop 256, in_channels <= 128, dim %% 128 == 0)");
        return nullptr;
    }
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) { set_error("no HIP device: libf5hip has no CPU fallback"); return nullptr; }
    f5hip_vocos* v = new f5hip_vocos();
    v->cfg = *cfg;
    v->nsplit = cfg->gemm_planes;
    return v;
}

void f5hip_vocos_destroy(f5hip_vocos* v) {
    if (!v) return;
    free_packed(v->embed); free_packed(v->head);
    for (float* p : {v->norm_w, v->norm_b, v->fnorm_w, v->fnorm_b, v->window}) dev_free(p);
    dev_free(v->twiddle);
    for (auto& b : v->blk) {
        for (float* p : {b.dw_w, b.dw_b, b.ln_w, b.ln_b, b.gamma}) dev_free(p);
        free_packed(b.pw1); free_packed(b.pw2);
    }
    dev_free(v->ws); dev_free(v->meta);
    delete v;
}

int f5hip_vocos_load_param(f5hip_vocos* v, const char* name, const float* data, int64_t numel) {
    return v ? v->params.load(v->finalized, name, data, numel) : fail(-1, "load_param: bad argument");
}

int f5hip_vocos_finalize(f5hip_vocos* v) {
    if (!v) return fail(-1, "null vocoder");
    if (v->finalized) return 0;
    const f5hip_vocos_config& c = v->cfg;
    const ParamStore& P = v->params;
    const int C = c.in_channels, D = c.dim, I = c.intermediate_dim, NO = c.n_fft + 2;
    {   // embed Conv1d(C -> D, k=7) as a dense implicit GEMM: K = 7 taps x 128 (channels padded)
        GET_PARAM(w, P, "backbone.embed.weight", (int64_t)D * C * 7); GET_PARAM(b, P, "backbone.embed.bias", D);
        std::vector<float> wp((size_t)D * 7 * 128, 0.0f);
        for (int co = 0; co < D; co++)
            for (int ci = 0; ci < C; ci++)
                for (int tap = 0; tap < 7; tap++) wp[(size_t)co * 896 + tap * 128 + ci] = (*w)[((size_t)co * C + ci) * 7 + tap];
        if (pack_linear(v->embed, wp.data(), D, 896, 896, b->data())) return -4;
    }
    GET_PARAM(nw, P, "backbone.norm.weight", D); GET_PARAM(nb, P, "backbone.norm.bias", D);
    GET_PARAM(fw_, P, "backbone.final_layer_norm.weight", D); GET_PARAM(fb_, P, "backbone.final_layer_norm.bias", D);
    if (upload_f32(&v->norm_w, nw->data(), D) || upload_f32(&v->norm_b, nb->data(), D) || upload_f32(&v->fnorm_w, fw_->data(), D) ||
        upload_f32(&v->fnorm_b, fb_->data(), D)) return -4;
    v->blk.resize(c.num_layers);
    for (int i = 0; i < c.num_layers; i++) {
        std::string p = "backbone.convnext." + std::to_string(i) + ".";
        VocosBlock& b = v->blk[i];
        GET_PARAM(dw, P, p + "dwconv.weight", (int64_t)D * 7); GET_PARAM(db, P, p + "dwconv.bias", D);
        GET_PARAM(lw, P, p + "norm.weight", D); GET_PARAM(lb, P, p + "norm.bias", D);
        GET_PARAM(w1, P, p + "pwconv1.weight", (int64_t)I * D); GET_PARAM(b1, P, p + "pwconv1.bias", I);
        GET_PARAM(w2, P, p + "pwconv2.weight", (int64_t)D * I); GET_PARAM(b2, P, p + "pwconv2.bias", D);
        GET_PARAM(gm, P, p + "gamma", D);
        if (upload_f32(&b.dw_w, dw->data(), dw->size()) || upload_f32(&b.dw_b, db->data(), D) || upload_f32(&b.ln_w, lw->data(), D) ||
            upload_f32(&b.ln_b, lb->data(), D) || upload_f32(&b.gamma, gm->data(), D)) return -4;
        if (pack_linear(b.pw1, w1->data(), I, D, D, b1->data())) return -4;
        if (pack_linear(b.pw2, w2->data(), D, I, I, b2->data())) return -4;
    }
    {
        GET_PARAM(w, P, "head.out.weight", (int64_t)NO * D); GET_PARAM(b, P, "head.out.bias", NO);
        if (pack_linear(v->head, w->data(), NO, D, D, b->data())) return -4;
    }
    if (make_fft_tables(&v->window, &v->twiddle, c.n_fft)) return -4;
    v->params.host.clear();
    v->finalized = true;
    return 0;
}

// Parity taps of one decode (f5hip_vocos_decode_taps): where to stop and where the valid rows of the workspace go
struct VocosTaps { int n_blocks; float *x, *y, *fw; };

// Copies the items' valid rows (item b: frames[b] rows from slab row seq_row0[b]) of src [rows][ld], `width` floats each, to dst packed
static int vocos_copy_rows(const float* src, int ld, int width, int n, const int32_t* frames, const int* seq_row0, float* dst, hipStream_t st) {
    for (int b = 0; b < n; b++) {
        if (hipMemcpy2DAsync(dst, sizeof(float) * width, src + (size_t)seq_row0[b] * ld, sizeof(float) * ld, sizeof(float) * width, frames[b],
                             hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(-6, "vocos taps: copy");
        dst += (size_t)frames[b] * width;
    }
    return 0;
}

// n items, item i with frames[i] frames at mel_dev + i * C * t_stride (channel stride t_stride); every item gets its own 128-row padded slab,
// so the embed conv and the depthwise convs see zeros at their item's bounds (row_start / row_end) and every kernel works row by row.
// Output packed: item i at wave_dev + hop * sum_{j<i} (frames[j] - 1).  With `taps` the same launches stop behind taps->n_blocks ConvNeXt blocks
// (< 0: none left out) and the valid rows of the residual stream -- behind a whole decode also of the head output and the windowed frames --
// are copied out.
static int vocos_decode_items(f5hip_vocos* v, int n, const int32_t* frames, int t_stride, const float* mel_dev, float* wave_dev, hipStream_t st,
                              const VocosTaps* taps = nullptr) {
    const f5hip_vocos_config& c = v->cfg;
    const int D = c.dim, I = c.intermediate_dim, LDY = 1152;
    long long m_ll = 0, l_ll = 0;
    for (int b = 0; b < n; b++) {
        if (frames[b] < 2 || frames[b] > t_stride) return fail(-1, "vocos_decode: item %d has %d frames (need 2 .. %d)", b, frames[b], t_stride);
        m_ll += ceil_to(frames[b], 128);
        l_ll += (long long)c.hop_length * (frames[b] - 1);
    }
    if (m_ll > (1LL << 24) || l_ll > 2147483647LL) return fail(-1, "vocos_decode: batch too large (%lld rows)", m_ll);
    const int M = (int)m_ll;
    const size_t meta_n = (size_t)M * 4 + (size_t)n * 3 + 1;
    if (M > v->cap_rows) {
        if (alloc_workspace(&v->ws, "vocos workspace", [&](Arena& a) {
                v->x = a.f32((size_t)M * D); v->y = a.f32((size_t)M * LDY); v->fw = a.f32((size_t)M * 1024);
                v->melp = a.plane2((size_t)M * 128 + 1024); v->tn = a.plane2((size_t)M * D); v->hid = a.plane2((size_t)M * I);
            })) { v->cap_rows = 0; return -5; }
        v->cap_rows = M;
    }
    if (meta_n > v->cap_meta) {
        dev_free(v->meta);
        if (hipMalloc((void**)&v->meta, sizeof(int) * meta_n) != hipSuccess) { v->meta = nullptr; v->cap_meta = 0; return fail(-5, "hipMalloc vocos meta"); }
        v->cap_meta = meta_n;
    }
    std::vector<int> h(meta_n, 0);
    int* row_seq = &h[0]; int* row_pos = row_seq + M; int* row_start = row_pos + M; int* row_end = row_start + M;
    int* seq_row0 = row_end + M; int* item_T = seq_row0 + n; int* item_out0 = item_T + n;
    for (int r = 0; r < M; r++) row_seq[r] = -1;
    for (int b = 0, r0 = 0; b < n; b++) {
        const int T = frames[b];
        seq_row0[b] = r0; item_T[b] = T;
        item_out0[b + 1] = item_out0[b] + c.hop_length * (T - 1);
        for (int t = 0; t < T; t++) { const int r = r0 + t; row_seq[r] = b; row_pos[r] = t; row_start[r] = r0; row_end[r] = r0 + T; }
        r0 += ceil_to(T, 128);
    }
    if (upload_sync(st, v->meta, h) != hipSuccess) return fail(-6, "vocos metadata upload");
    const int *d_row_seq = v->meta, *d_row_pos = v->meta + M, *d_row_start = v->meta + 2 * M, *d_row_end = v->meta + 3 * M;
    const int *d_seq_row0 = v->meta + 4 * M, *d_item_T = d_seq_row0 + n, *d_item_out0 = d_item_T + n;

    prof_begin(PROF_VOCOS, st);
    hipLaunchKernelGGL(mel_to_rows_kernel, dim3(M), dim3(128), 0, st, mel_dev, c.in_channels, t_stride, d_row_seq, d_row_pos, M, v->melp.hi, v->melp.lo);
    CKL("mel_to_rows");
    // embed conv -> x (fp32), then LayerNorm in place
    GemmArgs e = gemm_base(v->melp, 128, v->embed, M);
    e.conv_kpt = 4; e.conv_center = 3; e.conv_group_cols = 0; e.row_seq_start = d_row_start; e.row_seq_end = d_row_end;
    e.out_f32 = v->x; e.ldo = D;
    CK(run_gemm_n(v->nsplit, M, e, v->embed, EPI_GENERIC, true, 128, st));
    LnArgs ln = ln_args(v->x, D, M, D, v->norm_w, v->norm_b, 0.0f, 1e-6f);
    ln.out_f32 = v->x; ln.ldof = D;
    CK(run_ln(ln, st));
    const int nb = taps && taps->n_blocks >= 0 ? taps->n_blocks : c.num_layers;
    for (int i = 0; i < nb; i++) {
        VocosBlock& b = v->blk[i];
        LnArgs l2 = ln_args(v->x, D, M, D, b.ln_w, b.ln_b, 0.0f, 1e-6f);
        l2.dw_w = b.dw_w; l2.dw_b = b.dw_b; l2.row_seq_start = d_row_start; l2.row_seq_end = d_row_end;
        l2.out_hi = v->tn.hi; l2.out_lo = v->tn.lo; l2.ldo = D;
        CK(run_ln(l2, st));
        GemmArgs g1 = gemm_base(v->tn, D, b.pw1, M);
        g1.act = ACT_GELU_ERF; g1.out_hi = v->hid.hi; g1.out_lo = v->hid.lo; g1.ldob = I;
        CK(run_gemm_n(v->nsplit, M, g1, b.pw1, EPI_GENERIC, false, 128, st));
        GemmArgs g2 = gemm_base(v->hid, I, b.pw2, M);
        g2.mul = b.gamma; g2.res = v->x; g2.ldres = D; g2.out_f32 = v->x; g2.ldo = D;
        CK(run_gemm_n(v->nsplit, M, g2, b.pw2, EPI_GENERIC, false, 64, st));
    }
    if (taps && taps->n_blocks >= 0) {
        prof_end(PROF_VOCOS, st);
        return vocos_copy_rows(v->x, D, D, n, frames, seq_row0, taps->x, st);
    }
    LnArgs lf = ln_args(v->x, D, M, D, v->fnorm_w, v->fnorm_b, 0.0f, 1e-6f);
    lf.out_hi = v->tn.hi; lf.out_lo = v->tn.lo; lf.ldo = D;
    CK(run_ln(lf, st));
    GemmArgs hd = gemm_base(v->tn, D, v->head, M);
    hd.out_f32 = v->y; hd.ldo = LDY;
    CK(run_gemm_n(v->nsplit, M, hd, v->head, EPI_GENERIC, false, 128, st));
    hipLaunchKernelGGL(istft_frame_kernel, dim3(M), dim3(256), 0, st, v->y, LDY, d_row_seq, M, v->window, v->twiddle, v->fw);
    CKL("istft_frame");
    const int L = (int)l_ll;
    hipLaunchKernelGGL(istft_ola_kernel, dim3((L + 255) / 256), dim3(256), 0, st, v->fw, d_seq_row0, d_item_T, d_item_out0, n, c.hop_length,
                       v->window, wave_dev);
    CKL("istft_ola");
    prof_end(PROF_VOCOS, st);
    if (taps) {   // the stream behind the last block is still in x: the final norm writes operand planes
        CK(vocos_copy_rows(v->x, D, D, n, frames, seq_row0, taps->x, st));
        CK(vocos_copy_rows(v->y, LDY, c.n_fft + 2, n, frames, seq_row0, taps->y, st));
        CK(vocos_copy_rows(v->fw, 1024, 1024, n, frames, seq_row0, taps->fw, st));
    }
    return 0;
}

int f5hip_vocos_decode(f5hip_vocos* v, int32_t batch, int32_t frames, const float* mel_dev, float* wave_dev, void* stream) {
    if (!v || !v->finalized) return fail(-1, "vocoder not finalized");
    if (batch <= 0 || frames < 2 || !mel_dev || !wave_dev) return fail(-1, "vocos_decode: bad argument");
    const std::vector<int32_t> f(batch, frames);   // uniform items: output item b at hop * b * (frames - 1), i.e. [batch][hop * (frames - 1)]
    return vocos_decode_items(v, batch, f.data(), frames, mel_dev, wave_dev, (hipStream_t)stream);
}

int f5hip_vocos_decode_ragged(f5hip_vocos* v, int32_t n, const int32_t* frames, const float* mel_dev, float* wave_dev, void* stream) {
    if (!v || !v->finalized) return fail(-1, "vocoder not finalized");
    if (n <= 0 || !frames || !mel_dev || !wave_dev) return fail(-1, "vocos_decode_ragged: bad argument");
    int t_max = 0;
    for (int b = 0; b < n; b++) t_max = std::max(t_max, (int)frames[b]);
    return vocos_decode_items(v, n, frames, t_max, mel_dev, wave_dev, (hipStream_t)stream);
}

int f5hip_vocos_decode_taps(f5hip_vocos* v, int32_t n, const int32_t* frames, const float* mel_dev, int32_t n_blocks, float* x_dev, float* y_dev,
                            float* fw_dev, float* wave_dev, void* stream) {
    if (!v || !v->finalized) return fail(-1, "vocoder not finalized");
    if (n <= 0 || !frames || !mel_dev || !x_dev) return fail(-1, "vocos_decode_taps: bad argument");
    if (n_blocks < -1 || n_blocks > v->cfg.num_layers) return fail(-1, "vocos_decode_taps: n_blocks = %d (need -1 .. %d)", n_blocks, v->cfg.num_layers);
    if (n_blocks < 0 && (!y_dev || !fw_dev || !wave_dev)) return fail(-1, "vocos_decode_taps: a whole decode needs y_dev, fw_dev and wave_dev");
    int t_max = 0;
    for (int b = 0; b < n; b++) t_max = std::max(t_max, (int)frames[b]);
    const VocosTaps taps{n_blocks, x_dev, y_dev, fw_dev};
    return vocos_decode_items(v, n, frames, t_max, mel_dev, wave_dev, (hipStream_t)stream, &taps);
}

// ---------------------------------------------------------------------------------------- mel front-end
struct MelTables { int n_fft = 0, n_mels = 0, sr = 0; float* window = nullptr; float2* twiddle = nullptr; float* fb = nullptr; };
static MelTables g_mel, g_mel_bv;   // one set per front-end

// mel scales: HTK, and Slaney's (linear below 1 kHz, logarithmic above)
static double hz_to_mel_htk(double f) { return 2595.0 * log10(1.0 + f / 700.0); }
static double mel_to_hz_htk(double m) { return 700.0 * (pow(10.0, m / 2595.0) - 1.0); }
static double hz_to_mel_slaney(double f) { const double f_sp = 200.0 / 3, min_log_hz = 1000.0; return f >= min_log_hz ? min_log_hz / f_sp + log(f / min_log_hz) / (log(6.4) / 27.0) : f / f_sp; }
static double mel_to_hz_slaney(double m) { const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp; return m >= min_log_mel ? min_log_hz * exp(log(6.4) / 27.0 * (m - min_log_mel)) : f_sp * m; }

// [nf][n_mels] triangular filters over nf bins from 0 to fmax, their corners equally spaced on the mel scale; slaney: each scaled to unit area
static std::vector<float> mel_filterbank(int nf, int n_mels, double fmax, double (*hz_to_mel)(double), double (*mel_to_hz)(double), bool slaney) {
    const double m0 = hz_to_mel(0.0), m1 = hz_to_mel(fmax);
    std::vector<double> mf(n_mels + 2);
    for (int i = 0; i < n_mels + 2; i++) mf[i] = mel_to_hz(m0 + (m1 - m0) * (double)i / (double)(n_mels + 1));
    std::vector<float> fb((size_t)nf * n_mels, 0.0f);
    for (int k = 0; k < nf; k++) {
        const double f = fmax * (double)k / (double)(nf - 1);
        for (int j = 0; j < n_mels; j++) {
            const double lower = (f - mf[j]) / (mf[j + 1] - mf[j]), upper = (mf[j + 2] - f) / (mf[j + 2] - mf[j + 1]);
            const double w = std::max(0.0, std::min(lower, upper));
            fb[(size_t)k * n_mels + j] = (float)(slaney ? w * (2.0 / (mf[j + 2] - mf[j])) : w);
        }
    }
    return fb;
}
// torchaudio.functional.melscale_fbanks(n_freqs = 513, f_min = 0, f_max = sr/2, n_mels, sr, norm=None, "htk")
static std::vector<float> htk_filterbank(int nf, int n_mels, int sr) { return mel_filterbank(nf, n_mels, sr / 2, hz_to_mel_htk, mel_to_hz_htk, false); }
// librosa.filters.mel(sr, n_fft, n_mels, fmin=0, fmax=sr/2, htk=False, norm="slaney")
static std::vector<float> slaney_filterbank(int nf, int n_mels, int sr) { return mel_filterbank(nf, n_mels, sr / 2.0, hz_to_mel_slaney, mel_to_hz_slaney, true); }

// The tables t of one mel front-end (window, twiddles, filterbank(n_fft / 2 + 1, n_mels, sr)), rebuilt when (n_fft, n_mels, sr) changes
static int mel_tables(MelTables& t, std::vector<float> (*filterbank)(int, int, int), int n_fft, int n_mels, int sr) {
    if (t.n_fft != n_fft || t.n_mels != n_mels || t.sr != sr) {
        dev_free(t.window); dev_free(t.twiddle); dev_free(t.fb);
        t = MelTables();
        if (make_fft_tables(&t.window, &t.twiddle, n_fft)) return -4;
        const std::vector<float> fb = filterbank(n_fft / 2 + 1, n_mels, sr);
        if (upload_f32(&t.fb, fb.data(), fb.size())) return -4;
        t.n_fft = n_fft; t.n_mels = n_mels; t.sr = sr;
    }
    return 0;
}

// One mel front-end: its tables, then mel_frame_kernel over T frames at hop, the wave reflect-padded by `pad`
static int mel_frames(MelTables& t, std::vector<float> (*filterbank)(int, int, int), int batch, int n_samples, const float* wave_dev, float* mel_dev,
                      int n_fft, int hop, int n_mels, int sr, int pad, int T, float mag_eps, const char* name, hipStream_t st) {
    CK(mel_tables(t, filterbank, n_fft, n_mels, sr));
    prof_begin(PROF_OTHER, st);
    hipLaunchKernelGGL(mel_frame_kernel, dim3(T, batch), dim3(256), 0, st, wave_dev, n_samples, T, hop, n_mels, t.window, t.twiddle, t.fb, mel_dev, pad, mag_eps);
    prof_end(PROF_OTHER, st);
    CKL(name);
    return 0;
}

int f5hip_mel_spectrogram(int32_t batch, int32_t n_samples, const float* wave_dev, float* mel_dev, int32_t n_fft, int32_t hop_length,
                          int32_t n_mels, int32_t sample_rate, void* stream) {
    if (n_fft != 1024 || n_mels < 1 || n_mels > 256) return fail(-1, "mel_spectrogram: only n_fft = 1024, 1 <= n_mels <= 256");
    if (hop_length < 1 || hop_length > n_fft || sample_rate < 2) return fail(-1, "mel_spectrogram: need 1 <= hop_length <= n_fft, sample_rate >= 2");
    if (batch <= 0 || n_samples <= n_fft / 2 || !wave_dev || !mel_dev) return fail(-1, "mel_spectrogram: bad argument");
    return mel_frames(g_mel, htk_filterbank, batch, n_samples, wave_dev, mel_dev, n_fft, hop_length, n_mels, sample_rate, n_fft / 2,
                      1 + n_samples / hop_length, 0.0f, "mel_frame", (hipStream_t)stream);
}

// ---- BigVGAN-style mel (F/model/modules.py:30-72): librosa Slaney filterbank, center=False after a reflect pad of (n_fft - hop) / 2
int f5hip_mel_spectrogram_bigvgan(int32_t batch, int32_t n_samples, const float* wave_dev, float* mel_dev, int32_t n_fft, int32_t hop_length,
                                  int32_t n_mels, int32_t sample_rate, void* stream) {
    if (n_fft != 1024 || n_mels < 1 || n_mels > 256) return fail(-1, "mel_spectrogram_bigvgan: only n_fft = 1024, 1 <= n_mels <= 256");
    if (hop_length < 1 || hop_length > n_fft || sample_rate < 2) return fail(-1, "mel_spectrogram_bigvgan: need 1 <= hop_length <= n_fft, sample_rate >= 2");
    if (batch <= 0 || n_samples < n_fft || !wave_dev || !mel_dev) return fail(-1, "mel_spectrogram_bigvgan: bad argument");
    const int pad = (n_fft - hop_length) / 2;
    return mel_frames(g_mel_bv, slaney_filterbank, batch, n_samples, wave_dev, mel_dev, n_fft, hop_length, n_mels, sample_rate, pad,
                      (n_samples + 2 * pad - n_fft) / hop_length + 1, 1e-9f, "mel_frame (bigvgan)", (hipStream_t)stream);
}

// ---- both front-ends for n clips of their own lengths, one launch (F5HipModel.prepare_voices: the reference mels of a batch's new voices)
struct MelRaggedWorkspace { MelItem* items = nullptr; size_t cap_items = 0; WorkspaceUse use; };

int f5hip_mel_spectrogram_ragged(int32_t n, const int32_t* n_samples, const float* const* wave_dev, float* mel_dev, int32_t n_fft, int32_t hop_length,
                                 int32_t n_mels, int32_t sample_rate, int32_t variant, void* stream) {
    if (variant != 0 && variant != 1) return fail(-1, "mel_spectrogram_ragged: unknown variant %d (0 vocos, 1 bigvgan)", variant);
    if (n_fft != 1024 || n_mels < 1 || n_mels > 256) return fail(-1, "mel_spectrogram_ragged: only n_fft = 1024, 1 <= n_mels <= 256");
    if (hop_length < 1 || hop_length > n_fft || sample_rate < 2) return fail(-1, "mel_spectrogram_ragged: need 1 <= hop_length <= n_fft, sample_rate >= 2");
    if (n < 1 || !n_samples || !wave_dev || !mel_dev) return fail(-1, "mel_spectrogram_ragged: bad argument");
    const int pad = variant ? (n_fft - hop_length) / 2 : n_fft / 2;
    std::vector<MelItem> h(n);
    long long rows = 0;
    for (int i = 0; i < n; i++) {
        const int nw = n_samples[i];
        if (!wave_dev[i] || (variant ? nw < n_fft : nw <= n_fft / 2))
            return fail(-1, "mel_spectrogram_ragged: clip %d has %d samples (needs %s %d) or no data", i, nw, variant ? ">=" : ">", variant ? n_fft : n_fft / 2);
        if (reinterpret_cast<uintptr_t>(wave_dev[i]) & 3) return fail(-1, "mel_spectrogram_ragged: clip %d is not 4-byte aligned", i);
        h[i] = MelItem{wave_dev[i], nw, (int)rows};
        rows += variant ? (nw + 2 * pad - n_fft) / hop_length + 1 : 1 + nw / hop_length;   // the single-clip rule of the variant (>= 1)
        if (rows * n_mels > 2147483647LL) return fail(-1, "mel_spectrogram_ragged: the output exceeds 2^31 - 1 values");
    }
    MelTables& t = variant ? g_mel_bv : g_mel;
    CK(mel_tables(t, variant ? slaney_filterbank : htk_filterbank, n_fft, n_mels, sample_rate));
    MelRaggedWorkspace* const ws = device_workspace<MelRaggedWorkspace>("mel_spectrogram_ragged");
    if (!ws) return -6;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws->use, st);
    CK(turn.rc);
    CK(dev_reserve(&ws->items, &ws->cap_items, (size_t)n, "mel_spectrogram_ragged clips"));
    if (upload_sync(st, ws->items, h) != hipSuccess) return fail(-6, "mel_spectrogram_ragged metadata upload");
    prof_begin(PROF_OTHER, st);
    hipLaunchKernelGGL(mel_frame_ragged_kernel, dim3((unsigned)rows), dim3(256), 0, st, ws->items, n, hop_length, n_mels, t.window, t.twiddle, t.fb, mel_dev,
                       pad, variant ? 1e-9f : 0.0f);
    prof_end(PROF_OTHER, st);
    CKL("mel_frame_ragged");
    g_counters[CNT_MEL_RAGGED_LAUNCHES]++;
    g_counters[CNT_MEL_RAGGED_ITEMS] += n;
    return 0;
}
