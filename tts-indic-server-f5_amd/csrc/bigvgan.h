// BigVGAN v2 generator (NVIDIA/BigVGAN `bigvgan_v2_24khz_100band_256x` geometry) on the split-bf16
// implicit-GEMM conv kernel (gemm.h) plus three HBM-streaming kernels.  Included at the end of f5hip.hip.
//
// Layout: channel-last rows, one row per time step, batch items are "sequences" of pitch P_i = ceil128(T) * prod(rates so far)
// rows (T_i = T * prod valid), so a ConvTranspose1d with stride r writes [rows_in][r * C_out] == [rows_in * r][C_out].
//   conv_pre / resblock convs : Conv1d as implicit GEMM, K = taps x C_pad32, dilation = row shift per tap
//   ups[i] (k = 2r, stride r, pad r/2): 3-tap implicit GEMM over inputs t-1, t, t+1 with N = r * C_out (phase-major
//       columns); phase p uses taps (t, t-1) if p < r/2 else (t, t+1) -- the third tap's weights are zero
//   Activation1d(SnakeBeta): fused [2x Kaiser-sinc upsample -> x + sin^2(x e^a)/(e^b + 1e-9) -> 2x low-pass downsample], one lane
//       per (channel, run of 16 time steps), everything in registers (aa_snake2_kernel)
// Ragged calls (f5hip_bigvgan_forward_ragged): item i has its own pitch ceil128(T_i) * prod(rates so far), so no tile is spent on the rows
//       between a short item's end and the longest item's; every kernel finds an item's rows through small tables (BvRagged): per stage
//       one [start, end) per 128-row block of the first stage (the conv GEMMs' row predicate: tile -> block is one division), and one
//       entry per item in first-stage rows, scaled by prod(rates so far) (snake, conv_post: grid z = item).
// Operand precision (f5hip_bigvgan_config.gemm_planes): 2 = split bf16 (three MFMAs per product, the parity default), 3 = one fp16
//       plane (a third of the MFMA work and half the activation-plane traffic), 1 = plain bf16.
#pragma once

struct BvConv { PackedW w; int k = 0, dil = 1, c_in = 0, c_out = 0, c_in_pad = 0; };
struct BvRes { BvConv c1[3], c2[3]; float* alpha[6] = {}; float* beta[6] = {}; };

struct f5hip_bigvgan {
    f5hip_bigvgan_config cfg;
    int nsplit = 2;
    ParamStore params;
    bool finalized = false;
    int n_up = 0, c0 = 0;
    BvConv pre;
    std::vector<BvConv> ups;
    std::vector<BvRes> res;
    float *post_alpha = nullptr, *post_beta = nullptr, *post_w = nullptr;
    // workspace
    size_t cap = 0;
    void* ws = nullptr;
    float *X = nullptr, *Y[3] = {}, *S = nullptr, *Tm = nullptr;
    Plane2 act, melp;
    float filt_h[12] = {};
    int* meta = nullptr;   // tables of a ragged call (BvRagged)
    size_t cap_meta = 0;
};

// Row layout of a ragged call.  Item order in rows: first the items whose pitch ceil128(T) is a multiple of 256 (rows_a first-stage rows),
// then the others (rows_b) -- the two first-stage convolutions choose conv5.h or gemm.h by that, exactly as a call of the item alone does.
//   items[j] = (first row, T, frames of the items before it in the CALLER's order = wave offset / total_up, index in the caller's order),
//              in rows of the FIRST stage (one per mel frame): at a later stage they are multiplied by `scale` = prod(rates so far)
//   nblk first-stage blocks of 128 rows; block b belongs to one item: blk_mel[b] = its index in the caller's order, and per stage s
//   start(s)[b], end(s)[b] = its first row and the end of its valid rows at that stage (GemmArgs::row_seq_start / row_seq_end with seq_blk);
//   start_b / end_b = the first stage's for the blocks behind rows_a, relative to row rows_a
struct BvRagged {
    int n = 0, t_stride = 0, rows_a = 0, rows_b = 0, nblk = 0;
    const int4* items = nullptr;
    const int *blk_mel = nullptr, *bounds = nullptr, *start_b = nullptr, *end_b = nullptr;
    const int* start(int s) const { return bounds + (size_t)2 * s * nblk; }
    const int* end(int s) const { return start(s) + nblk; }
};

// ------------------------------------------------------------------------------------------------ kernels
struct AaFilt { float f[12]; };

// Anti-aliased SnakeBeta activation (alias_free_torch Activation1d, up = down = 2, 12 taps), x fp32 [rows][ldx], uniform sequences of pitch
// P rows with T valid.  Register-resident: a lane owns one channel and R consecutive time steps.  It loads the R + 10
// inputs its outputs depend on (row index clamped = the replicate padding of the up-sampler; for a fixed register the lanes of a
// segment read consecutive channels of one row, so the loads coalesce), forms the 2R + 10 up-sampled snake values (index clamped
// to [0, 2T) = the replicate padding of the down-sampler: values past the end repeat the last one, values before 0 repeat value 0)
// and the R low-passed outputs.  No LDS, no barrier: ~44 VALU operations and 2.6 v_sin per output instead of ~25 LDS reads (the round-1
// LDS-tiled kernel, removed).
//   (items != null: ragged sequences, see BvRagged)
//   grid (C / cw, ceil(T / (nseg R)), sequences), 256 lanes = nseg segments x cw channels (cw | C, cw <= 64)
//   OUT: 0 = fp32, 1 = split bf16 planes, 2 = one fp16 plane
template <int R, int OUT>
__global__ __launch_bounds__(256) void aa_snake2_kernel(const float* __restrict__ x, int ldx, int C, int cw, int nseg, int P, int T,
                                                        const float* __restrict__ alpha_log, const float* __restrict__ beta_log, AaFilt flt,
                                                        __bf16* __restrict__ out_hi, __bf16* __restrict__ out_lo, float* __restrict__ out_f32, int ldo,
                                                        const int4* __restrict__ items, int scale) {
    const int tid = threadIdx.x;
    const int seg = tid / cw, c = blockIdx.x * cw + (tid - seg * cw);
    const int t0 = (blockIdx.y * nseg + seg) * R;
    size_t seq0 = (size_t)blockIdx.z * P;
    if (items) {   // ragged: sequence z is item z, rows [items[z].x, + items[z].y) * scale (the grid's y covers the longest item)
        const int4 it = items[blockIdx.z];
        seq0 = (size_t)it.x * scale;
        T = it.y * scale;
    }
    if (seg >= nseg || t0 >= T || c >= C) return;
    const float* xb = x + seq0 * ldx + c;
    float xv[R + 10];
#pragma unroll
    for (int i = 0; i < R + 10; i++) {
        int ti = t0 - 5 + i;
        ti = ti < 0 ? 0 : (ti > T - 1 ? T - 1 : ti);
        xv[i] = xb[(size_t)ti * ldx];
    }
    const float ea = expf(alpha_log[c]) * 0.15915494309189535f;   // radians -> revolutions for v_sin_f32
    const float ib = 1.0f / (expf(beta_log[c]) + 1e-9f);
    float f2[12];
#pragma unroll
    for (int k = 0; k < 12; k++) f2[k] = 2.0f * flt.f[k];   // ratio * conv_transpose1d
    const int lim = 2 * (T - t0) + 4;   // up-sampled index j = 2 t0 - 5 + i is inside [0, 2T) for 5 - 2 t0 <= i <= lim
    float a[2 * R + 10];
    float prev = 0.0f;
#pragma unroll
    for (int i = 0; i < 2 * R + 10; i++) {
        const int i0 = i >> 1, odd = (i & 1) ^ 1;   // j odd <=> i even
        float u = 0.0f;
#pragma unroll
        for (int q = 0; q < 6; q++) u += xv[i0 + q] * f2[11 - odd - 2 * q];
        const float rev = u * ea;
        const float sn = __builtin_amdgcn_sinf(rev - rintf(rev));
        float av = u + ib * sn * sn;
        av = i > lim ? prev : av;
        prev = av;
        a[i] = av;
    }
    if (t0 == 0) {
#pragma unroll
        for (int i = 0; i < 5; i++) a[i] = a[5];
    }
#pragma unroll
    for (int tt = 0; tt < R; tt++) {
        float v = 0.0f;
#pragma unroll
        for (int k = 0; k < 12; k++) v += a[2 * tt + k] * flt.f[k];
        if (t0 + tt < T) {
            const size_t o = (seq0 + t0 + tt) * ldo + c;
            if constexpr (OUT == 0) out_f32[o] = v;
            if constexpr (OUT == 1) {
                __bf16 h, l;
                split_bf16(v, h, l);
                out_hi[o] = h;
                out_lo[o] = l;
            }
            if constexpr (OUT == 2) reinterpret_cast<_Float16*>(out_hi)[o] = sat_f16(v);
        }
    }
}

// mean of the three AMP blocks of a stage (n_in == 3; n_in == 1 is a plain conversion of y0), 4 channels per lane: (y0 + y1 + y2) / 3 ->
// fp32 rows and / or the operand planes of the next up-sampler (mode 1 split bf16, 2 fp16, 3 plain bf16; ldo >= C, padding channels
// are left as they are)
__global__ __launch_bounds__(256) void bv_mean3_kernel(const float* __restrict__ y0, const float* __restrict__ y1, const float* __restrict__ y2, int n_in, size_t rows,
                                                       int C, float* __restrict__ out_f32, __bf16* __restrict__ out_hi, __bf16* __restrict__ out_lo, int ldo, int mode) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int c4 = C >> 2;
    if (i >= rows * c4) return;
    const size_t row = i / c4;
    const int c = (int)(i - row * c4) * 4;
    f32x4 s = reinterpret_cast<const f32x4*>(y0)[i];
    if (n_in == 3) s = (s + reinterpret_cast<const f32x4*>(y1)[i] + reinterpret_cast<const f32x4*>(y2)[i]) * (1.0f / 3.0f);
    if (out_f32) reinterpret_cast<f32x4*>(out_f32)[i] = s;
    if (mode == 0) return;
    const float y[4] = {s[0], s[1], s[2], s[3]};
    __bf16* dh = out_hi + row * ldo + c;
    if (mode == 2) { store_f16x4(dh, y); return; }
    bf16x4 h, l;
    split_bf16x4(y, h, l);
    *reinterpret_cast<bf16x4*>(dh) = h;
    if (mode == 1) *reinterpret_cast<bf16x4*>(out_lo + row * ldo + c) = l;
}

// mel [B][C][T] fp32 -> rows (b * P + t) of 128 split-bf16 channels (rows >= T and channels >= C are zero)
__global__ __launch_bounds__(128) void bv_mel_rows_kernel(const float* mel, int C, int T, int P, __bf16* hi, __bf16* lo, int f16) {
    const int row = blockIdx.x, c = threadIdx.x;
    const int b = row / P, t = row - b * P;
    float v = 0.0f;
    if (t < T && c < C) v = mel[((size_t)b * C + c) * T + t];
    if (f16) { reinterpret_cast<_Float16*>(hi)[(size_t)row * 128 + c] = sat_f16(v); return; }
    __bf16 h, l;
    split_bf16(v, h, l);
    hi[(size_t)row * 128 + c] = h;
    if (lo) lo[(size_t)row * 128 + c] = l;
}

// the same for a ragged call: mel [n][C][t_stride], row -> its block's item (BvRagged); nothing beyond an item's T columns is read
__global__ __launch_bounds__(128) void bv_mel_rows_ragged_kernel(const float* mel, int C, int t_stride, const int* blk_start, const int* blk_end, const int* blk_mel,
                                                                 __bf16* hi, __bf16* lo, int f16) {
    const int row = blockIdx.x, c = threadIdx.x;
    const int t = row - blk_start[row >> 7];
    float v = 0.0f;
    if (row < blk_end[row >> 7] && c < C) v = mel[((size_t)blk_mel[row >> 7] * C + c) * t_stride + t];
    if (f16) { reinterpret_cast<_Float16*>(hi)[(size_t)row * 128 + c] = sat_f16(v); return; }
    __bf16 h, l;
    split_bf16(v, h, l);
    hi[(size_t)row * 128 + c] = h;
    if (lo) lo[(size_t)row * 128 + c] = l;
}

// conv_post: Conv1d(C -> 1, k = 7, pad 3, no bias) + clamp(-1, 1);  a fp32 [rows][lda] -> wave [B][T].  256 outputs per workgroup: the
// 262 input rows go through LDS (row pitch C + 1 floats: the lanes of a wave read consecutive rows, an odd pitch is conflict-free),
// the weights are read as broadcasts.  Dynamic LDS = (262 (C + 1) + 7 C) floats.
// items != null (ragged, BvRagged): sequence b is item b, its wave starts at items[b].z * scale and the grid's x covers the longest item.
__global__ __launch_bounds__(256) void bv_conv_post_kernel(const float* __restrict__ a, int lda, int C, int P, int T, const float* __restrict__ w /*[C][7]*/,
                                                           float* __restrict__ wave, const int4* __restrict__ items, int scale) {
    extern __shared__ float bvp_sm[];
    float* tile = bvp_sm;
    float* ws = bvp_sm + 262 * (C + 1);
    const int b = blockIdx.y, t0 = blockIdx.x * 256, tid = threadIdx.x;
    int row0 = b * P;
    size_t w0 = (size_t)b * T;
    if (items) {
        const int4 it = items[b];
        row0 = it.x * scale; T = it.y * scale; w0 = (size_t)it.z * scale;
        if (t0 >= T) return;   // (the whole workgroup: a shorter item's tail)
    }
    for (int i = tid; i < 262 * C; i += 256) {
        const int r = i / C, c = i - r * C, ti = t0 - 3 + r;
        tile[r * (C + 1) + c] = (ti >= 0 && ti < T) ? a[(size_t)(row0 + ti) * lda + c] : 0.0f;
    }
    for (int i = tid; i < 7 * C; i += 256) {
        const int k = i / C, c = i - k * C;
        ws[i] = w[c * 7 + k];
    }
    __syncthreads();
    const int t = t0 + tid;
    if (t >= T) return;
    float acc = 0.0f;
    for (int k = 0; k < 7; k++) {
        const float* row = tile + (tid + k) * (C + 1);
        const float* wk = ws + k * C;
        for (int c = 0; c < C; c++) acc += wk[c] * row[c];
    }
    wave[w0 + t] = fminf(fmaxf(acc, -1.0f), 1.0f);
}

// the same operator without the LDS tile (channel counts whose tile would not fit)
__global__ __launch_bounds__(256) void bv_conv_post_naive_kernel(const float* a, int lda, int C, int P, int T, const float* w /*[C][7]*/, float* wave,
                                                                 const int4* items, int scale) {
    const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    int row0 = b * P;
    size_t w0 = (size_t)b * T;
    if (items) {
        const int4 it = items[b];
        row0 = it.x * scale; T = it.y * scale; w0 = (size_t)it.z * scale;
    }
    if (t >= T) return;
    float acc = 0.0f;
    for (int k = 0; k < 7; k++) {
        const int ti = t + k - 3;
        if (ti < 0 || ti >= T) continue;
        const float* row = a + (size_t)(row0 + ti) * lda;
        for (int c = 0; c < C; c++) acc += w[c * 7 + k] * row[c];
    }
    wave[w0 + t] = fminf(fmaxf(acc, -1.0f), 1.0f);
}

// ------------------------------------------------------------------------------------------------ host side
f5hip_bigvgan* f5hip_bigvgan_create(const f5hip_bigvgan_config* cfg) {
    if (!cfg) { set_error("null config"); return nullptr; }
    if (cfg->num_upsamples < 1 || cfg->num_upsamples > 8 || cfg->num_mels > 128 || cfg->upsample_initial_channel % (1 << cfg->num_upsamples) ||
        (cfg->gemm_planes < 1 || cfg->gemm_planes > 3)) { set_error("unsupported BigVGAN geometry"); return nullptr; }
    for (int i = 0; i < cfg->num_upsamples; i++)
        if (cfg->upsample_kernel_sizes[i] != 2 * cfg->upsample_rates[i] || cfg->upsample_rates[i] % 2) {
            set_error("BigVGAN: only kernel = 2 * stride, even stride up-samplers are supported"); return nullptr;
        }
    if ((cfg->upsample_initial_channel >> cfg->num_upsamples) % 4) { set_error("BigVGAN: final channel count must be a multiple of 4"); return nullptr; }
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) { set_error("no HIP device: libf5hip has no CPU fallback"); return nullptr; }
    f5hip_bigvgan* v = new f5hip_bigvgan();
    v->cfg = *cfg; v->nsplit = cfg->gemm_planes; v->n_up = cfg->num_upsamples; v->c0 = cfg->upsample_initial_channel;
    return v;
}

static void bv_free_conv(BvConv& c) { free_packed(c.w); }

void f5hip_bigvgan_destroy(f5hip_bigvgan* v) {
    if (!v) return;
    bv_free_conv(v->pre);
    for (auto& u : v->ups) bv_free_conv(u);
    for (auto& r : v->res) {
        for (int j = 0; j < 3; j++) { bv_free_conv(r.c1[j]); bv_free_conv(r.c2[j]); }
        for (int a = 0; a < 6; a++) { dev_free(r.alpha[a]); dev_free(r.beta[a]); }
    }
    for (float* p : {v->post_alpha, v->post_beta, v->post_w}) dev_free(p);
    dev_free(v->ws);
    dev_free(v->meta);
    delete v;
}

int f5hip_bigvgan_load_param(f5hip_bigvgan* v, const char* name, const float* data, int64_t numel) {
    return v ? v->params.load(v->finalized, name, data, numel) : fail(-1, "load_param: bad argument");
}

// Conv1d weight [co][ci][k] -> [co][tap][ci_pad]
static int bv_pack_conv(BvConv& c, const std::vector<float>& w, const float* bias, int co, int ci, int k, int dil, bool f16) {
    c.k = k; c.dil = dil; c.c_in = ci; c.c_out = co; c.c_in_pad = ceil_to(ci, 32);
    const int K = k * c.c_in_pad;
    std::vector<float> wp((size_t)co * K, 0.0f);
    for (int o = 0; o < co; o++)
        for (int i = 0; i < ci; i++)
            for (int t = 0; t < k; t++) wp[(size_t)o * K + t * c.c_in_pad + i] = w[((size_t)o * ci + i) * k + t];
    return pack_linear(c.w, wp.data(), co, K, K, bias, co <= 64 ? 64 : 128, f16);
}

// kaiser_sinc_filter1d(cutoff 0.25, half_width 0.3, 12) of alias_free_torch/filter.py, evaluated in double and rounded to fp32
static void bv_aa_filter(float out[12]) {
    const int ks = 12, half = 6;
    const double cutoff = 0.25, hw = 0.3, delta_f = 4 * hw, A = 2.285 * (half - 1) * M_PI * delta_f + 7.95;
    const double beta = A > 50.0 ? 0.1102 * (A - 8.7) : (A >= 21.0 ? 0.5842 * pow(A - 21.0, 0.4) + 0.07886 * (A - 21.0) : 0.0);
    auto i0 = [](double x) { double s = 1.0, t = 1.0; for (int k = 1; k < 50; k++) { t *= (x / (2.0 * k)) * (x / (2.0 * k)); s += t; } return s; };
    double f[12], sum = 0.0;
    for (int n = 0; n < ks; n++) {
        const double r = 2.0 * n / (ks - 1) - 1.0;                       // torch.kaiser_window(periodic=False)
        const double win = i0(beta * sqrt(1.0 - r * r)) / i0(beta);
        const double tm = (n - half) + 0.5, xx = 2 * cutoff * tm;
        const double sinc = fabs(xx) < 1e-12 ? 1.0 : sin(M_PI * xx) / (M_PI * xx);
        f[n] = 2 * cutoff * win * sinc;
        sum += f[n];
    }
    for (int n = 0; n < ks; n++) out[n] = (float)(f[n] / sum);
}

// ConvTranspose1d(ci -> co, k = 2 r, stride r, padding r / 2), weight [ci][co][k], as the 3-tap implicit GEMM over inputs t - 1, t, t + 1:
// [r co][tap][ci_pad] with phase-major columns n = p co + o.  Output row r t + p takes input t through tap p + r / 2, and input t - 1
// (p < r / 2, tap p + 3 r / 2) or t + 1 (p >= r / 2, tap p - r / 2); the third tap's weights stay zero
static int bv_pack_ups(BvConv& u, const float* w, const float* b, int ci, int co, int r, bool f16) {
    const int k = 2 * r;
    u.k = 3; u.dil = 1; u.c_in = ci; u.c_out = r * co; u.c_in_pad = ceil_to(ci, 32);
    const int K = 3 * u.c_in_pad;
    std::vector<float> wp((size_t)r * co * K, 0.0f), bp((size_t)r * co);
    for (int p = 0; p < r; p++)
        for (int o = 0; o < co; o++) {
            const size_t n = (size_t)p * co + o;
            bp[n] = b[o];
            for (int i2 = 0; i2 < ci; i2++) {
                const float* wr = &w[((size_t)i2 * co + o) * k];   // ConvTranspose1d weight [c_in][c_out][k]
                wp[n * K + 1 * u.c_in_pad + i2] = wr[p + r / 2];                       // input t
                if (p < r / 2) wp[n * K + 0 * u.c_in_pad + i2] = wr[p + 3 * r / 2];   // input t - 1
                else wp[n * K + 2 * u.c_in_pad + i2] = wr[p - r / 2];                  // input t + 1
            }
        }
    return pack_linear(u.w, wp.data(), r * co, K, K, bp.data(), r * co <= 64 ? 64 : 128, f16);
}

int f5hip_bigvgan_finalize(f5hip_bigvgan* v) {
    if (!v) return fail(-1, "null vocoder");
    if (v->finalized) return 0;
    const f5hip_bigvgan_config& c = v->cfg;
    const ParamStore& P = v->params;
    const bool f16 = v->nsplit == 3;
    {
        GET_PARAM(w, P, "conv_pre.weight", (int64_t)v->c0 * c.num_mels * 7); GET_PARAM(b, P, "conv_pre.bias", v->c0);
        // input rows are mel frames padded to 128 channels
        BvConv& p = v->pre; p.k = 7; p.dil = 1; p.c_in = c.num_mels; p.c_out = v->c0; p.c_in_pad = 128;
        std::vector<float> wp((size_t)v->c0 * 7 * 128, 0.0f);
        for (int o = 0; o < v->c0; o++)
            for (int i = 0; i < c.num_mels; i++)
                for (int t = 0; t < 7; t++) wp[(size_t)o * 896 + t * 128 + i] = (*w)[((size_t)o * c.num_mels + i) * 7 + t];
        if (pack_linear(p.w, wp.data(), v->c0, 896, 896, b->data(), 128, f16)) return -4;
    }
    v->ups.resize(v->n_up);
    v->res.resize(v->n_up * 3);
    for (int i = 0; i < v->n_up; i++) {
        const int ci = v->c0 >> i, co = v->c0 >> (i + 1), r = c.upsample_rates[i], k = 2 * r;
        GET_PARAM(w, P, "ups." + std::to_string(i) + ".0.weight", (int64_t)ci * co * k);
        GET_PARAM(b, P, "ups." + std::to_string(i) + ".0.bias", co);
        if (bv_pack_ups(v->ups[i], w->data(), b->data(), ci, co, r, f16)) return -4;
        for (int j = 0; j < 3; j++) {
            BvRes& rb = v->res[i * 3 + j];
            const int kk = c.resblock_kernel_sizes[j];
            const std::string q = "resblocks." + std::to_string(i * 3 + j) + ".";
            for (int d = 0; d < 3; d++) {
                GET_PARAM(w1, P, q + "convs1." + std::to_string(d) + ".weight", (int64_t)co * co * kk); GET_PARAM(b1, P, q + "convs1." + std::to_string(d) + ".bias", co);
                GET_PARAM(w2, P, q + "convs2." + std::to_string(d) + ".weight", (int64_t)co * co * kk); GET_PARAM(b2, P, q + "convs2." + std::to_string(d) + ".bias", co);
                if (bv_pack_conv(rb.c1[d], *w1, b1->data(), co, co, kk, c.resblock_dilations[j * 3 + d], f16)) return -4;
                if (bv_pack_conv(rb.c2[d], *w2, b2->data(), co, co, kk, 1, f16)) return -4;
            }
            for (int a = 0; a < 6; a++) {
                GET_PARAM(al, P, q + "activations." + std::to_string(a) + ".act.alpha", co); GET_PARAM(be, P, q + "activations." + std::to_string(a) + ".act.beta", co);
                if (upload_f32(&rb.alpha[a], al->data(), co) || upload_f32(&rb.beta[a], be->data(), co)) return -4;
            }
        }
    }
    {
        const int ch = v->c0 >> v->n_up;
        GET_PARAM(al, P, "activation_post.act.alpha", ch); GET_PARAM(be, P, "activation_post.act.beta", ch); GET_PARAM(w, P, "conv_post.weight", (int64_t)ch * 7);
        if (upload_f32(&v->post_alpha, al->data(), ch) || upload_f32(&v->post_beta, be->data(), ch) || upload_f32(&v->post_w, w->data(), ch * 7)) return -4;
    }
    bv_aa_filter(v->filt_h);
    v->params.host.clear();
    v->finalized = true;
    return 0;
}

// GemmArgs of the Conv1d c over M rows of operand planes A (sequences of pitch P rows, T of them valid): out [M][c_out] = conv + bias + res.
// blk > 0: ragged sequences, bounds [start, end) per block of blk rows (GemmArgs::seq_blk), every one of them starting at a multiple of P rows
static GemmArgs conv_args(const BvConv& c, const Plane2& A, int M, int P, int T, const float* res, float* out, const int* start = nullptr,
                          const int* end = nullptr, int blk = 0) {
    GemmArgs g = gemm_base(A, c.c_in_pad, c.w, M);
    g.conv_kpt = c.c_in_pad / 32; g.conv_center = (c.k - 1) / 2; g.conv_dil = c.dil; g.seq_pitch = P; g.seq_valid = T;
    g.row_seq_start = start; g.row_seq_end = end; g.seq_blk = blk;
    g.res = res; g.ldres = c.c_out; g.out_f32 = out; g.ldo = c.c_out;
    return g;
}

// nsplit: operand planes (2 split bf16, 3 fp16, 1 bf16); conv5.h first where it covers the shape (nsplit >= 2), else gemm.h
static int bv_conv(int nsplit, const BvConv& c, const Plane2& A, int M, int P, int T, const float* res, float* out, hipStream_t st,
                   const int* start = nullptr, const int* end = nullptr, int blk = 0) {
    GemmArgs g = conv_args(c, A, M, P, T, res, out, start, end, blk);
    return run_conv(nsplit, g, c.w, nsplit >= 2, true, c.w.n_pad % 128 ? 64 : 128, st);
}

// Activation1d over fp32 rows x [M][ch] (sequences of pitch P rows, T valid): out_mode 0 -> fp32 rows out_f32 [M][ldo], 1 -> split-bf16
// planes hi / lo [M][ldo], 2 -> one fp16 plane hi [M][ldo].  One lane per (channel, 16 time steps): cw channels x nseg segments fill the
// 256 lanes of a workgroup (cw | ch, cw <= 64).  items != null: the n_items ragged sequences of BvRagged at `scale`, T = the longest one's rows
static int bv_snake_launch(const float* x, int ch, int M, int P, int T, const float* alpha, const float* beta, const AaFilt& f, int out_mode,
                           __bf16* hi, __bf16* lo, float* out_f32, int ldo, hipStream_t st, const int4* items = nullptr, int n_items = 0, int scale = 0) {
    constexpr int R = 16;
    int cw = ch < 64 ? ch : 64;
    while (ch % cw) cw--;
    if (ch == 96) cw = 32;   // 8 segments of 32 channels fill the 256 lanes; 64 would leave a half-empty second column block
    const int nseg = 256 / cw;
    const dim3 grid(ch / cw, (T + nseg * R - 1) / (nseg * R), items ? n_items : M / P);
    if (out_mode == 0) hipLaunchKernelGGL((aa_snake2_kernel<R, 0>), grid, dim3(256), 0, st, x, ch, ch, cw, nseg, P, T, alpha, beta, f, (__bf16*)nullptr, (__bf16*)nullptr, out_f32, ldo, items, scale);
    else if (out_mode == 2) hipLaunchKernelGGL((aa_snake2_kernel<R, 2>), grid, dim3(256), 0, st, x, ch, ch, cw, nseg, P, T, alpha, beta, f, hi, (__bf16*)nullptr, (float*)nullptr, ldo, items, scale);
    else hipLaunchKernelGGL((aa_snake2_kernel<R, 1>), grid, dim3(256), 0, st, x, ch, ch, cw, nseg, P, T, alpha, beta, f, hi, lo, (float*)nullptr, ldo, items, scale);
    CKL("aa_snake2");
    return 0;
}

// Activation1d over fp32 rows x [M][ch] -> the conv operand planes (out == nullptr) or fp32 rows out [M][ch]
static int bv_snake(f5hip_bigvgan* v, const float* x, int ch, int cpad, int M, int P, int T, const float* alpha, const float* beta, float* out,
                    hipStream_t st, const BvRagged* rg = nullptr, int scale = 0) {
    AaFilt f;
    memcpy(f.f, v->filt_h, sizeof(f.f));
    const int4* items = rg ? rg->items : nullptr;
    const int n = rg ? rg->n : 0;
    if (out) return bv_snake_launch(x, ch, M, P, T, alpha, beta, f, 0, nullptr, nullptr, out, ch, st, items, n, scale);
    return bv_snake_launch(x, ch, M, P, T, alpha, beta, f, v->nsplit == 3 ? 2 : 1, v->act.hi, v->act.lo, nullptr, cpad, st, items, n, scale);
}

// Dynamic LDS of bv_conv_post_kernel at C channels
static size_t bv_conv_post_lds(int C) { return (size_t)(262 * (C + 1) + 7 * C) * sizeof(float); }

// conv_post + clamp over fp32 rows a [batch P][lda] -> wave [batch][T].  variant 0: the LDS kernel when its tile fits in 48 KB, else the
// naive kernel (what the generator runs); 1: the LDS kernel (fails when it would not fit); 2: the naive kernel
// items != null: `batch` ragged items (BvRagged) at `scale`, T = the longest one's rows, wave packed
static int bv_conv_post(const float* a, int lda, int C, int batch, int P, int T, const float* w, float* wave, int variant, hipStream_t st,
                        const int4* items = nullptr, int scale = 0) {
    const size_t lds = bv_conv_post_lds(C);
    if (variant == 1 && lds > 48 * 1024) return fail(-1, "conv_post: the LDS kernel's tile does not fit at C = %d", C);
    if (variant == 1 || (variant == 0 && lds <= 48 * 1024))
        hipLaunchKernelGGL(bv_conv_post_kernel, dim3((T + 255) / 256, batch), dim3(256), lds, st, a, lda, C, P, T, w, wave, items, scale);
    else hipLaunchKernelGGL(bv_conv_post_naive_kernel, dim3((T + 255) / 256, batch), dim3(256), 0, st, a, lda, C, P, T, w, wave, items, scale);
    CKL("conv_post");
    return 0;
}

// Workspace for M0 first-stage rows.  Largest stage: rows_i * C_i with rows_i = M0 * prod(rates), C_i = c0 >> (i+1)
static int bv_reserve(f5hip_bigvgan* v, size_t M0) {
    const f5hip_bigvgan_config& c = v->cfg;
    size_t max_f32 = M0 * v->c0, max_act = M0 * ceil_to(v->c0, 32);
    size_t rows = M0;
    for (int i = 0; i < v->n_up; i++) {
        rows *= c.upsample_rates[i];
        const int ch = v->c0 >> (i + 1);
        max_f32 = std::max(max_f32, rows * ch);
        max_act = std::max(max_act, rows * ceil_to(ch, 32));
    }
    if (max_f32 <= v->cap) return 0;
    if (alloc_workspace(&v->ws, "BigVGAN workspace", [&](Arena& a) {
            v->X = a.f32(max_f32); v->S = a.f32(max_f32); v->Tm = a.f32(max_f32);
            for (int j = 0; j < 3; j++) v->Y[j] = a.f32(max_f32);
            v->act = a.plane2(max_act + 4096); v->melp = a.plane2(M0 * 128 + 4096);
        })) { v->cap = 0; return -5; }
    v->cap = max_f32;
    return 0;
}

// The generator over M0 first-stage rows.  rg == null: uniform sequences of pitch P0 rows with T0 valid, mel [M0 / P0][num_mels][T0] ->
// wave [M0 / P0][total_up T0].  rg != null: the ragged layout rg (tables on the device), mel [n][num_mels][t_stride] -> packed wave; every
// stage is still ONE launch per operator for all items, but for the two first-stage convolutions (conv_pre, ups[0]), which run once over
// the items of 256-aligned pitch and once over the others.
static int bv_generate(f5hip_bigvgan* v, int M0, int P0, int T0, const BvRagged* rg, const float* mel_dev, float* wave_dev, hipStream_t st) {
    const f5hip_bigvgan_config& c = v->cfg;
    const int plane_mode = v->nsplit == 3 ? 2 : (v->nsplit == 2 ? 1 : 3);   // bv_mean3_kernel's output mode
    CK(bv_reserve(v, (size_t)M0));
    prof_begin(PROF_VOCOS, st);
    // mel [B][num_mels][T] -> rows [M0][128] operand planes (uniform sequences: row = b * P0 + t)
    if (rg) hipLaunchKernelGGL(bv_mel_rows_ragged_kernel, dim3(M0), dim3(128), 0, st, mel_dev, c.num_mels, rg->t_stride, rg->start(0), rg->end(0), rg->blk_mel, v->melp.hi, v->melp.lo, v->nsplit == 3 ? 1 : 0);
    else hipLaunchKernelGGL(bv_mel_rows_kernel, dim3(M0), dim3(128), 0, st, mel_dev, c.num_mels, T0, P0, v->melp.hi, v->melp.lo, v->nsplit == 3 ? 1 : 0);
    CKL("bv_mel_rows");
    int M = M0, P = P0, T = T0, scale = 1;
    int ch = v->c0;
    // a convolution at stage s (s up-samplers so far), residual res
    auto conv = [&](const BvConv& cv, int s, const float* res, float* out) -> int {
        if (!rg) return bv_conv(v->nsplit, cv, v->act, M, P, T, res, out, st);
        return bv_conv(v->nsplit, cv, v->act, M, P, T, res, out, st, rg->start(s), rg->end(s), 128 * scale);
    };
    // a convolution over first-stage rows: ragged items of 256-aligned pitch (conv5.h takes them, as it does when such an item is alone), then the rest
    auto conv0 = [&](const BvConv& cv, const Plane2& A, float* out) -> int {
        if (!rg) return bv_conv(v->nsplit, cv, A, M, P, T, nullptr, out, st);
        if (rg->rows_a) CK(bv_conv(v->nsplit, cv, A, rg->rows_a, 256, 0, nullptr, out, st, rg->start(0), rg->end(0), 128));
        if (rg->rows_b)
            CK(bv_conv(v->nsplit, cv, rows_from(A, (size_t)rg->rows_a * cv.c_in_pad), rg->rows_b, 128, 0, nullptr, out + (size_t)rg->rows_a * cv.c_out, st,
                       rg->start_b, rg->end_b, 128));
        return 0;
    };
    CK(conv0(v->pre, v->melp, v->S));   // S = conv_pre(mel)
    {   // operand planes of ups[0]
        const size_t n4 = (size_t)M * ch / 4;
        hipLaunchKernelGGL(bv_mean3_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, v->S, v->S, v->S, 1, (size_t)M, ch, (float*)nullptr, v->act.hi, v->act.lo,
                           ceil_to(ch, 32), plane_mode);
        CKL("bv planes");
    }
    for (int i = 0; i < v->n_up; i++) {
        const int r = c.upsample_rates[i], co = ch / 2, cpad = ceil_to(co, 32);
        // ups[i]: 3-tap implicit GEMM over the planes of the previous stage -> X viewed as [M][r*co] == [M*r][co]
        if (i == 0) CK(conv0(v->ups[0], v->act, v->X));
        else CK(conv(v->ups[i], i, nullptr, v->X));
        M *= r; P *= r; T *= r; scale *= r; ch = co;
        if (cpad != ch) {   // padded channels of the A operand must read as zero
            if (hipMemsetAsync(v->act.hi, 0, (size_t)M * cpad * 2, st) != hipSuccess || (v->nsplit == 2 && hipMemsetAsync(v->act.lo, 0, (size_t)M * cpad * 2, st) != hipSuccess))
                return fail(-6, "bigvgan memset");
        }
        for (int j = 0; j < 3; j++) {
            const BvRes& rb = v->res[i * 3 + j];
            float* y = v->Y[j];
            for (int d = 0; d < 3; d++) {
                const float* in = d == 0 ? v->X : y;   // AMPBlock1: x = x + convs2[d](act(convs1[d](act(x))))
                CK(bv_snake(v, in, ch, cpad, M, P, T, rb.alpha[2 * d], rb.beta[2 * d], nullptr, st, rg, scale));
                CK(conv(rb.c1[d], i + 1, nullptr, v->Tm));
                CK(bv_snake(v, v->Tm, ch, cpad, M, P, T, rb.alpha[2 * d + 1], rb.beta[2 * d + 1], nullptr, st, rg, scale));
                CK(conv(rb.c2[d], i + 1, in, y));
            }
        }
        // mean of the three blocks: the last stage keeps fp32 rows for activation_post, the others only feed the next up-sampler
        const bool last = i == v->n_up - 1;
        const size_t n4 = (size_t)M * ch / 4;
        hipLaunchKernelGGL(bv_mean3_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, v->Y[0], v->Y[1], v->Y[2], 3, (size_t)M, ch, last ? v->S : (float*)nullptr,
                           v->act.hi, v->act.lo, cpad, last ? 0 : plane_mode);
        CKL("bv_mean3");
    }
    // activation_post -> fp32 (Tm), conv_post + clamp -> wave [B][T] (ragged: packed)
    CK(bv_snake(v, v->S, ch, ch, M, P, T, v->post_alpha, v->post_beta, v->Tm, st, rg, scale));
    CK(bv_conv_post(v->Tm, ch, ch, rg ? rg->n : M / P, P, T, v->post_w, wave_dev, 0, st, rg ? rg->items : nullptr, scale));
    prof_end(PROF_VOCOS, st);
    return 0;
}

int f5hip_bigvgan_forward(f5hip_bigvgan* v, int32_t batch, int32_t frames, const float* mel_dev, float* wave_dev, void* stream) {
    if (!v || !v->finalized) return fail(-1, "vocoder not finalized");
    if (batch <= 0 || frames <= 0 || !mel_dev || !wave_dev) return fail(-1, "bigvgan_forward: bad argument");
    const int P0 = ceil_to(frames, 128);
    return bv_generate(v, batch * P0, P0, frames, nullptr, mel_dev, wave_dev, (hipStream_t)stream);
}

// Every item gets its own rows (BvRagged); the tables go up once, on the caller's stream, and every stage then runs as for a uniform batch:
// the launch count does not depend on n.  No value of mel_dev beyond column frames[i] of item i is read.
int f5hip_bigvgan_forward_ragged(f5hip_bigvgan* v, int32_t n, const int32_t* frames, const float* mel_dev, float* wave_dev, void* stream) {
    if (!v || !v->finalized) return fail(-1, "vocoder not finalized");
    if (n <= 0 || n > 65535 || !frames || !mel_dev || !wave_dev) return fail(-1, "bigvgan_forward_ragged: bad argument");
    hipStream_t st = (hipStream_t)stream;
    long long total_up = 1, m0 = 0, rows_a = 0;
    for (int i = 0; i < v->n_up; i++) total_up *= v->cfg.upsample_rates[i];
    int t_max = 0;
    for (int i = 0; i < n; i++) {
        if (frames[i] <= 0) return fail(-1, "bigvgan_forward_ragged: item %d has %d frames", i, frames[i]);
        const int p = ceil_to(frames[i], 128);
        m0 += p;
        if (p % 256 == 0) rows_a += p;
        t_max = std::max(t_max, (int)frames[i]);
    }
    if (m0 * total_up > 2147483647LL) return fail(-1, "bigvgan_forward_ragged: batch too large (%lld rows)", m0 * total_up);
    const int M0 = (int)m0, nblk = M0 / 128, nblk_a = (int)rows_a / 128, nblk_b = nblk - nblk_a, ns = v->n_up + 1;
    // device tables, one int buffer: items [n] int4, blk_mel [nblk], per stage start [nblk] + end [nblk], start_b [nblk_b], end_b [nblk_b]
    const size_t meta_n = (size_t)n * 4 + nblk + (size_t)ns * 2 * nblk + (size_t)2 * nblk_b;
    if (meta_n > v->cap_meta) {
        dev_free(v->meta);
        if (hipMalloc((void**)&v->meta, sizeof(int) * meta_n) != hipSuccess) { v->meta = nullptr; v->cap_meta = 0; return fail(-5, "hipMalloc bigvgan meta"); }
        v->cap_meta = meta_n;
    }
    std::vector<int> h(meta_n, 0);
    int* items = &h[0]; int* blk_mel = items + 4 * n; int* bounds = blk_mel + nblk; int* start_b = bounds + (size_t)ns * 2 * nblk; int* end_b = start_b + nblk_b;
    {
        std::vector<int> prefix(n + 1, 0);
        for (int i = 0; i < n; i++) prefix[i + 1] = prefix[i] + frames[i];
        int j = 0, r0 = 0;
        for (int pass = 0; pass < 2; pass++)   // the items of 256-aligned pitch first
            for (int i = 0; i < n; i++) {
                const int p = ceil_to(frames[i], 128);
                if ((p % 256 == 0) != (pass == 0)) continue;
                items[4 * j] = r0; items[4 * j + 1] = frames[i]; items[4 * j + 2] = prefix[i]; items[4 * j + 3] = i;
                for (int b = r0 / 128; b < (r0 + p) / 128; b++) {
                    blk_mel[b] = i;
                    int scale = 1;
                    for (int s = 0; s < ns; s++) {
                        bounds[(size_t)2 * s * nblk + b] = r0 * scale; bounds[(size_t)(2 * s + 1) * nblk + b] = (r0 + frames[i]) * scale;
                        if (s < v->n_up) scale *= v->cfg.upsample_rates[s];
                    }
                    if (pass) { start_b[b - nblk_a] = r0 - (int)rows_a; end_b[b - nblk_a] = r0 - (int)rows_a + frames[i]; }
                }
                r0 += p; j++;
            }
    }
    CK(bv_reserve(v, (size_t)M0));   // (before the upload: nothing is queued when the allocation fails)
    if (upload_sync(st, v->meta, h) != hipSuccess) return fail(-6, "bigvgan metadata upload");
    BvRagged rg;
    rg.n = n; rg.t_stride = t_max; rg.rows_a = (int)rows_a; rg.rows_b = M0 - (int)rows_a; rg.nblk = nblk;
    rg.items = reinterpret_cast<const int4*>(v->meta);
    rg.blk_mel = v->meta + 4 * n; rg.bounds = rg.blk_mel + nblk; rg.start_b = rg.bounds + (size_t)ns * 2 * nblk; rg.end_b = rg.start_b + nblk_b;
    return bv_generate(v, M0, 256, t_max, &rg, mel_dev, wave_dev, st);
}
