// Per-kernel unit operators of the C ABI (include/f5hip.h, "unit ops"): each runs ONE production kernel through the same dispatcher the
// sampler uses, on fp32 device tensors, so that `pytest -m gpu` can pin every hot kernel against a plain fp32 reference and the
// tools can time it in isolation.  Included at the end of f5hip.hip (same translation unit as the dispatcher).
#pragma once

struct OpBufs {
    std::vector<void*> ptrs;
    ~OpBufs() { for (void* p : ptrs) if (p) (void)hipFree(p); }
    template <typename T> T* get(size_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return (T*)p;
    }
};

// n elements of T, every byte `pad` (0x00: zeros; 0xff: NaN in fp32, bf16 and fp16)
template <typename T> static T* op_filled(OpBufs& b, size_t n, int pad, hipStream_t st) {
    T* p = b.get<T>(n);
    if (p) (void)hipMemsetAsync(p, pad, n * sizeof(T), st);
    return p;
}

// device fp32 [R][C] -> operand planes [R_pad][C] (prec 3: one fp16 plane; 2: split bf16; 1: bf16 hi only is read)
static void op_pack_planes(const float* src, int R, int C, int R_pad, __bf16* hi, __bf16* lo, bool f16, hipStream_t st) {
    hipLaunchKernelGGL(pack_weight_kernel, dim3(R_pad), dim3(256), 0, st, src, R, C, C, hi, f16 ? (__bf16*)nullptr : lo, C);
}

// Stamp buffer of the diagnostics kernels, [4096 workgroups][16] words, zeroed and then written by launch(d, rep) for rep = 0, 1, 2.  h: its host
// copy (left empty when the buffer cannot be allocated); ng: workgroups up to the last that stamped; tmin / tmax: first start, last end.
template <typename Launch>
static int collect_stamps(OpBufs& b, hipStream_t st, Launch launch, std::vector<unsigned long long>& h, int& ng, unsigned long long& tmin,
                          unsigned long long& tmax) {
    const int maxg = 4096;
    unsigned long long* d = b.get<unsigned long long>((size_t)maxg * 16);
    if (!d) return 0;
    (void)hipMemsetAsync(d, 0, sizeof(unsigned long long) * maxg * 16, st);
    for (int rep = 0; rep < 3; rep++) CK(launch(d, rep));
    (void)hipStreamSynchronize(st);
    h.resize((size_t)maxg * 16);
    (void)hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost);
    for (int g2 = 0; g2 < maxg; g2++) if (h[(size_t)g2 * 16]) { ng = g2 + 1; tmin = std::min(tmin, h[(size_t)g2 * 16]); tmax = std::max(tmax, std::max(h[(size_t)g2 * 16 + 6], h[(size_t)g2 * 16 + 14])); }
    return 0;
}

// one stderr line: fmt with the arguments `head`, then the min, median and max of v (nothing when v is empty)
template <typename... Head>
static void print_spread(std::vector<double> v, const char* fmt, Head... head) {
    if (v.empty()) return;
    std::sort(v.begin(), v.end());
    fprintf(stderr, fmt, head..., v.front(), v[v.size() / 2], v.back());
}

// diagnostics of the W-direct gemm5 kernels (F5HIP_GEMM5_STAMPS=1, tools/gemm5_stamps.py): s_memrealtime stamps (100 MHz) of wave 0 (consumer)
// and wave 4 (loader) of every workgroup
template <typename Launch>
static int gemm5_stamp_report(OpBufs& b, int M, int N, int K, hipStream_t st, Launch launch) {
    std::vector<unsigned long long> h;
    int ng = 0;
    unsigned long long tmin = ~0ull, tmax = 0;
    CK(collect_stamps(b, st, launch, h, ng, tmin, tmax));
    if (h.empty()) return 0;
    const char* names[7] = {"start", "tile0 landed (loader)", "k-loop end", "E1 passed", "E2 passed (slab done)", "row phase issued", "stores drained"};
    fprintf(stderr, "[gemm5 stamps] M %d N %d K %d: %d workgroups, first start -> last end %.2f us\n", M, N, K, ng, (tmax - tmin) * 0.01);
    for (int w = 0; w < 2; w++)
        for (int i = 0; i < 7; i++) {
            std::vector<double> v;
            for (int g2 = 0; g2 < ng; g2++) { const unsigned long long t = h[(size_t)g2 * 16 + w * 8 + i]; if (t) v.push_back((t - tmin) * 0.01); }
            print_spread(v, "[gemm5 stamps]   wave %d  %-26s min %6.2f  median %6.2f  max %6.2f us after the first workgroup started\n", w * 4, names[i]);
        }
    // epilogue duration (E1 -> end of the row phase) by column slab of the tile (XCD-blocked order of gemm5_tile_of_block, 16 column slabs)
    if (ng == 256) {
        for (int tn = 0; tn < 16; tn++) {
            std::vector<double> v;
            for (int g2 = 0; g2 < ng; g2++) {
                const int tile = (g2 & 7) * (ng >> 3) + (g2 >> 3);
                if (tile % 16 == tn) v.push_back((h[(size_t)g2 * 16 + 5] - h[(size_t)g2 * 16 + 3]) * 0.01);
            }
            print_spread(v, "[gemm5 stamps]   column slab %2d: epilogue min %5.2f median %5.2f max %5.2f us\n", tn);
        }
    }
    return 0;
}

// diagnostics of gemm6 (F5HIP_GEMM6_STAMPS=1, tools/gemm6_stamps.py): per-workgroup time line from the kernel's run-time stamps
template <typename Launch>
static int gemm6_stamp_report(OpBufs& b, int M, int N, int K, hipStream_t st, Launch launch) {
    std::vector<unsigned long long> h;
    int ng = 0;
    unsigned long long tmin = ~0ull, tmax = 0;
    CK(collect_stamps(b, st, launch, h, ng, tmin, tmax));
    if (h.empty()) return 0;
    fprintf(stderr, "[gemm6 stamps] M %d N %d K %d: %d workgroups, first start -> last end %.2f us\n", M, N, K, ng, (tmax - tmin) * 0.01);
    const char* names[6] = {"k-loop", "quarter 0", "quarter 1", "quarter 2", "quarter 3", "store drain"};
    for (int w = 0; w < 2; w++)
        for (int i = 0; i < 6; i++) {
            std::vector<double> v;
            for (int g2 = 0; g2 < ng; g2++) {
                const unsigned long long t0 = h[(size_t)g2 * 16 + w * 8 + i], t1 = h[(size_t)g2 * 16 + w * 8 + i + 1];
                if (t0 && t1) v.push_back((t1 - t0) * 0.01);
            }
            print_spread(v, "[gemm6 stamps]   wave %d  %-12s duration min %6.2f  median %6.2f  max %6.2f us\n", w * 4, names[i]);
        }
    {   // the shader clock the k-loops ran at: s_memtime cycles over s_memrealtime (100 MHz) ticks
        std::vector<double> v;
        for (int g2 = 0; g2 < ng; g2++) {
            const unsigned long long cyc = h[(size_t)g2 * 16 + 7], t0 = h[(size_t)g2 * 16], t1 = h[(size_t)g2 * 16 + 1];
            if (cyc && t1 > t0) v.push_back((double)cyc / ((double)(t1 - t0) * 10.0));   // cycles per ns = GHz
        }
        print_spread(v, "[gemm6 stamps]   shader clock during the k-loop: min %.2f  median %.2f  max %.2f GHz  (the 2.5 PFLOP/s roof is 2.4 GHz x 4096 FLOP / clk / CU x 256 CUs)\n");
    }
    {   // start times: how the rounds lay out
        std::vector<double> v;
        for (int g2 = 0; g2 < ng; g2++) v.push_back((h[(size_t)g2 * 16] - tmin) * 0.01);
        std::sort(v.begin(), v.end());
        fprintf(stderr, "[gemm6 stamps]   workgroup start: 25 %% %.2f  50 %% %.2f  75 %% %.2f  90 %% %.2f  last %.2f us\n", v[ng / 4], v[ng / 2], v[3 * ng / 4], v[9 * ng / 10], v.back());
    }
    return 0;
}

// f5hip_op_gemm and f5hip_op_gemm_rowmul: row_mod_host null = EPI_GENERIC with the multiplier vector mul_dev [N] (or none); else
// EPI_GENERIC_ROWMUL, row r multiplied by mul_dev + row_mod_host[r] * mod_ld
static int op_gemm_run(int32_t M, int32_t N, int32_t K, const float* a_dev, const float* w_dev, const float* bias_dev, int32_t prec, int32_t act,
                       const float* mul_dev, const int32_t* row_mod_host, int32_t mod_ld, const float* res_dev, const uint8_t* row_keep_host,
                       float* out_dev, uint16_t* out16_dev, int32_t w_copies, int32_t iters, double* avg_us, void* stream, int32_t bn) {
    const int epi = row_mod_host ? EPI_GENERIC_ROWMUL : EPI_GENERIC;
    if (M <= 0 || N <= 0 || K <= 0 || K % 32 || N % 4 || !a_dev || !w_dev || prec < 1 || prec > 3 || (!out_dev && !out16_dev))
        return fail(-1, "op_gemm: bad argument (need K %% 32 == 0, N %% 4 == 0, prec 1..3)");
    if (bn == 0) bn = 128;
    if (bn != 64 && bn != 128) return fail(-1, "op_gemm: bn must be 0, 64 or 128 (got %d)", bn);
    if (out16_dev && (res_dev || out_dev)) return fail(-1, "op_gemm: the 16-bit output is the (no residual, no fp32 output) epilogue");
    hipStream_t st = (hipStream_t)stream;
    const int M_pad = (M + 127) / 128 * 128, N_pad = (N + 127) / 128 * 128;
    const bool f16 = prec == 3;
    if (w_copies < 1) w_copies = 1;
    // F5HIP_GEMM3_THIN=0|1: this call's gemm3 launches take the 128-row / the 32-row instance whatever the dispatch rule says (timing both
    // on one shape: tools/thin_tiles_bench.py); the path never sets it
    struct ThinForce {
        ThinForce() { const char* e = getenv("F5HIP_GEMM3_THIN"); g_thin_force = e && *e ? (atoi(e) != 0) : -1; }
        ~ThinForce() { g_thin_force = -1; }
    } thin_force;
    OpBufs b;
    Plane2 A;
    A.hi = b.get<__bf16>((size_t)M_pad * K); A.lo = b.get<__bf16>((size_t)M_pad * K);
    float* bias = b.get<float>(N_pad);
    int *keep = nullptr, *row_mod = nullptr;
    if (!A.hi || !A.lo || !bias) return fail(-5, "op_gemm: hipMalloc");
    std::vector<PackedW> Ws(w_copies);
    for (auto& W : Ws) {
        W.hi = b.get<__bf16>((size_t)N_pad * K); W.lo = f16 ? nullptr : b.get<__bf16>((size_t)N_pad * K);
        if (!W.hi || (!f16 && !W.lo)) return fail(-5, "op_gemm: hipMalloc weights");
        W.n = N; W.k = K; W.n_pad = N_pad; W.k_pad = K; W.ld = K; W.bias = bias; W.f16 = f16;
        op_pack_planes(w_dev, N, K, N_pad, W.hi, W.lo, f16, st);
        if (f16 && N >= 2048 && pack_frag(W, st)) return -5;   // like the model's FF1 weights: fragment order for the W-direct kernels (freed with b)
        if (W.frag) b.ptrs.push_back(W.frag);
    }
    op_pack_planes(a_dev, M, K, M_pad, A.hi, A.lo, f16, st);
    (void)hipMemsetAsync(bias, 0, sizeof(float) * N_pad, st);
    if (bias_dev) (void)hipMemcpyAsync(bias, bias_dev, sizeof(float) * N, hipMemcpyDeviceToDevice, st);
    if (row_keep_host) {
        keep = b.get<int>(M_pad);
        std::vector<int> hk(M_pad, 0);
        for (int i = 0; i < M; i++) hk[i] = row_keep_host[i];
        if (!keep || upload_sync(st, keep, hk) != hipSuccess) return fail(-6, "op_gemm: row_keep upload");
    }
    if (row_mod_host) {   // (the padding rows name modulation row 0; no kernel reads a multiplier for them)
        row_mod = b.get<int>(M_pad);
        std::vector<int> hm(M_pad, 0);
        std::copy(row_mod_host, row_mod_host + M, hm.begin());
        if (!row_mod || upload_sync(st, row_mod, hm) != hipSuccess) return fail(-6, "op_gemm: row_mod upload");
    }
    auto args_for = [&](const PackedW& W) {
        GemmArgs g = gemm_base(A, K, W, M);
        g.act = act; g.mul = mul_dev; g.res = res_dev; g.ldres = N; g.row_keep = keep;
        if (row_mod) { g.row_mod = row_mod; g.mod_ld = mod_ld; }
        if (out16_dev) { g.out_hi = (__bf16*)out16_dev; g.ldob = N; g.f16_out = 1; }
        else { g.out_f32 = out_dev; g.ldo = N; }
        return g;
    };
    {
        GemmArgs g = args_for(Ws[0]);
        CK(run_gemm_n(prec, M_pad, g, Ws[0], epi, false, bn, st));
    }
    auto stamped = [&](unsigned long long* d, int rep) {   // the diagnostics' launches cycle through the weight copies too
        GemmArgs g = args_for(Ws[rep % w_copies]);
        g.stamps = d;
        return run_gemm_n(prec, M_pad, g, Ws[rep % w_copies], epi, false, bn, st);
    };
    if (getenv("F5HIP_GEMM5_STAMPS")) CK(gemm5_stamp_report(b, M, N, K, st, stamped));
    if (getenv("F5HIP_GEMM6_STAMPS")) CK(gemm6_stamp_report(b, M, N, K, st, stamped));
    if (iters > 0 && avg_us) {
        // timing: the residual epilogue accumulates in place, so time into a scratch output
        float* scratch = b.get<float>((size_t)M * N);
        if (!scratch) return fail(-5, "op_gemm: hipMalloc scratch");
        CK(time_launches(3, iters, avg_us, st, [&](int i) {
            const PackedW& W = Ws[i % w_copies];
            GemmArgs g = args_for(W);
            if (!out16_dev) { g.out_f32 = scratch; if (res_dev) g.res = scratch; }
            return run_gemm_n(prec, M_pad, g, W, epi, false, bn, st);
        }));
    }
    if (hipStreamSynchronize(st) != hipSuccess) return fail(-7, "op_gemm: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

extern "C" int f5hip_op_gemm(int32_t M, int32_t N, int32_t K, const float* a_dev, const float* w_dev, const float* bias_dev, int32_t prec,
                             int32_t act, const float* mul_dev, const float* res_dev, const uint8_t* row_keep_host, float* out_dev,
                             uint16_t* out16_dev, int32_t w_copies, int32_t iters, double* avg_us, void* stream, int32_t bn) {
    return op_gemm_run(M, N, K, a_dev, w_dev, bias_dev, prec, act, mul_dev, nullptr, 0, res_dev, row_keep_host, out_dev, out16_dev, w_copies, iters,
                       avg_us, stream, bn);
}

// The gated residual projection of a mixed-grid call, out = ((A W^T + bias), rows with row_keep == 0 zeroed) * mul[row_mod[r]] + res: the
// EPI_GENERIC_ROWMUL kernels, which are the (no activation, residual, fp32 output) epilogue only
extern "C" int f5hip_op_gemm_rowmul(int32_t M, int32_t N, int32_t K, const float* a_dev, const float* w_dev, const float* bias_dev, int32_t prec,
                                    const float* mul_dev, const int32_t* row_mod_host, int32_t mod_ld, int32_t n_mod_rows, const float* res_dev,
                                    const uint8_t* row_keep_host, float* out_dev, void* stream, int32_t bn) {
    if (!mul_dev || !row_mod_host || !res_dev || !out_dev || mod_ld < N || mod_ld % 4 || n_mod_rows <= 0 || ((uintptr_t)mul_dev & 15))
        return fail(-1, "op_gemm_rowmul: bad argument (need mul, row_mod, res and out; mod_ld >= N, mod_ld %% 4 == 0, mul 16-byte aligned)");
    for (int i = 0; i < M; i++)
        if (row_mod_host[i] < 0 || row_mod_host[i] >= n_mod_rows) return fail(-1, "op_gemm_rowmul: row_mod[%d] = %d out of range", i, row_mod_host[i]);
    return op_gemm_run(M, N, K, a_dev, w_dev, bias_dev, prec, ACT_NONE, mul_dev, row_mod_host, mod_ld, res_dev, row_keep_host, out_dev, nullptr, 1, 0,
                       nullptr, stream, bn);
}

// Fused QKV projection with its epilogue (bias, rotary on head 0, q / 8, V transposed): F/model/modules.py:409-426.
//   a_dev fp32 [M][D], w_dev fp32 [3 D][D] (to_q | to_k | to_v rows), bias_dev [3 D], row_pos host int32 [M]
//   qk_dev  bf16 [M_pad][2 D] (q pre-scaled by 1/8 | k), vt_dev bf16 [D][M_pad], M_pad = ceil128(M)
extern "C" int f5hip_op_qkv(int32_t M, int32_t D, const float* a_dev, const float* w_dev, const float* bias_dev, const int32_t* row_pos,
                            int32_t prec, uint16_t* qk_dev, uint16_t* vt_dev, int32_t iters, double* avg_us, void* stream) {
    if (M <= 0 || D <= 0 || D % 128 || !a_dev || !w_dev || !bias_dev || !row_pos || !qk_dev || !vt_dev || prec < 1 || prec > 3)
        return fail(-1, "op_qkv: bad argument (need D %% 128 == 0)");
    hipStream_t st = (hipStream_t)stream;
    const int M_pad = (M + 127) / 128 * 128, N = 3 * D, N_pad = (N + 127) / 128 * 128;
    const bool f16 = prec == 3;
    OpBufs b;
    Plane2 A; PackedW W;
    A.hi = b.get<__bf16>((size_t)M_pad * D); A.lo = b.get<__bf16>((size_t)M_pad * D);
    W.hi = b.get<__bf16>((size_t)N_pad * D); W.lo = f16 ? nullptr : b.get<__bf16>((size_t)N_pad * D);
    float* bias = b.get<float>(N_pad);
    std::vector<float> hc, hs;
    rope_tables(hc, hs);
    float* rc = b.get<float>(hc.size()); float* rs = b.get<float>(hs.size());
    int* pos = b.get<int>(M_pad);
    if (!A.hi || !A.lo || !W.hi || (!f16 && !W.lo) || !bias || !rc || !rs || !pos) return fail(-5, "op_qkv: hipMalloc");
    W.n = N; W.k = D; W.n_pad = N_pad; W.k_pad = D; W.ld = D; W.bias = bias; W.f16 = f16;
    std::vector<int> hp(M_pad, 0);
    for (int i = 0; i < M; i++) { if (row_pos[i] < 0 || row_pos[i] > 4096) return fail(-1, "op_qkv: row_pos out of range"); hp[i] = row_pos[i]; }
    if (upload_sync(st, rc, hc, rs, hs, pos, hp) != hipSuccess) return fail(-6, "op_qkv: table upload");
    op_pack_planes(w_dev, N, D, N_pad, W.hi, W.lo, f16, st);
    if (f16 && pack_frag(W, st)) return -5;
    if (W.frag) b.ptrs.push_back(W.frag);
    op_pack_planes(a_dev, M, D, M_pad, A.hi, A.lo, f16, st);
    (void)hipMemsetAsync(bias, 0, sizeof(float) * N_pad, st);
    (void)hipMemcpyAsync(bias, bias_dev, sizeof(float) * N, hipMemcpyDeviceToDevice, st);
    GemmArgs g = gemm_base(A, D, W, M);
    g.D = D; g.row_pos = pos; g.rope_cos = rc; g.rope_sin = rs; g.qk = (__bf16*)qk_dev; g.vt = (__bf16*)vt_dev; g.ldvt = M_pad;
    if (getenv("F5HIP_GEMM5_STAMPS"))
        CK(gemm5_stamp_report(b, M, N, D, st, [&](unsigned long long* d, int) {
            GemmArgs g2 = g;
            g2.stamps = d;
            return run_gemm_n(prec, M_pad, g2, W, EPI_QKV, false, 128, st);
        }));
    CK(time_launches(1, iters, avg_us, st, [&](int) { return run_gemm_n(prec, M_pad, g, W, EPI_QKV, false, 128, st); }));   // the warm-up launch writes the output
    if (hipStreamSynchronize(st) != hipSuccess) return fail(-7, "op_qkv: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

// LayerNorm + modulation y = LN(x) (gain_off + scale) + shift (F/model/modules.py:285-290), or x-transformers RMSNorm (rms = 1): fp32 in, fp32 out
extern "C" int f5hip_op_layernorm(int32_t M, int32_t D, const float* x_dev, const float* scale_dev, const float* shift_dev, float gain_off, float eps,
                                  int32_t rms, float* out_dev, void* stream) {
    if (M <= 0 || D <= 0 || D % 4 || !x_dev || !scale_dev || !shift_dev || !out_dev) return fail(-1, "op_layernorm: bad argument");
    hipStream_t st = (hipStream_t)stream;
    LnArgs ln = ln_args(x_dev, D, M, D, scale_dev, shift_dev, gain_off, eps);
    ln.rms = rms; ln.out_f32 = out_dev; ln.ldof = D;
    CK(run_ln(ln, st));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- attention unit op
__global__ __launch_bounds__(256) void op_pack_qkv_kernel(const float* q, const float* k, const float* v, int D, const int* row_src, int M_pad,
                                                          __bf16* qk, __bf16* vt) {
    const int row = blockIdx.x, src = row_src[row];
    for (int c = threadIdx.x; c < D; c += 256) {
        const float qv = src >= 0 ? q[(size_t)src * D + c] * F5_Q_SCALE : 0.0f;   // q is pre-scaled by log2(e) / 8 like the QKV epilogue's
        const float kv = src >= 0 ? k[(size_t)src * D + c] : 0.0f;
        const float vv = src >= 0 ? v[(size_t)src * D + c] : 0.0f;
        // fp16 bits, saturated, like the QKV epilogue's outputs
        reinterpret_cast<_Float16*>(qk)[(size_t)row * 2 * D + c] = sat_f16(qv);
        reinterpret_cast<_Float16*>(qk)[(size_t)row * 2 * D + D + c] = sat_f16(kv);
        reinterpret_cast<_Float16*>(vt)[(size_t)c * M_pad + vt_col(row)] = sat_f16(vv);
    }
}
// the attention output back into frame order as fp32: hi + lo (split-bf16 planes), hi alone (lo == null: the bf16 plane), or hi read as one fp16 plane
__global__ __launch_bounds__(256) void op_unpack_planes_kernel(const __bf16* hi, const __bf16* lo, int f16, int D, const int* frame_row, float* out) {
    const int f = blockIdx.x, row = frame_row[f];
    for (int c = threadIdx.x; c < D; c += 256) {
        const size_t i = (size_t)row * D + c;
        out[(size_t)f * D + c] = f16 ? (float)reinterpret_cast<const _Float16*>(hi)[i] : (float)hi[i] + (lo ? (float)lo[i] : 0.0f);
    }
}

// f5hip_op_layernorm's modulation through the PLANE stores of ln_finish, what the GEMMs read: out_format 0 = split-bf16 planes (hi + lo),
// 1 = one fp16 plane, read back as fp32.  row_mod_host null: the plain ln_kernel instance, scale / shift [D]; else the ROW_MOD instance: row r
// takes scale_dev / shift_dev + row_mod_host[r] * mod_ld (two column offsets into one [n_mod_rows][mod_ld] table).  The planes start as NaN.
extern "C" int f5hip_op_layernorm_planes(int32_t M, int32_t D, const float* x_dev, const float* scale_dev, const float* shift_dev,
                                         const int32_t* row_mod_host, int32_t mod_ld, int32_t n_mod_rows, float gain_off, float eps,
                                         int32_t out_format, float* out_dev, void* stream) {
    if (M <= 0 || D <= 0 || D % 4 || !x_dev || !scale_dev || !shift_dev || !out_dev || out_format < 0 || out_format > 1)
        return fail(-1, "op_layernorm_planes: bad argument");
    if (row_mod_host) {
        if (mod_ld < D || mod_ld % 4 || n_mod_rows <= 0 || (((uintptr_t)scale_dev | (uintptr_t)shift_dev) & 15))
            return fail(-1, "op_layernorm_planes: need mod_ld >= D, mod_ld %% 4 == 0 and 16-byte aligned scale / shift");
        for (int i = 0; i < M; i++)
            if (row_mod_host[i] < 0 || row_mod_host[i] >= n_mod_rows) return fail(-1, "op_layernorm_planes: row_mod[%d] = %d out of range", i, row_mod_host[i]);
    }
    hipStream_t st = (hipStream_t)stream;
    OpBufs b;
    const size_t n = (size_t)M * D;
    __bf16* hi = op_filled<__bf16>(b, n, 0xff, st); __bf16* lo = op_filled<__bf16>(b, n, 0xff, st);
    int* idx = b.get<int>(2 * (size_t)M);   // the rows in order (op_unpack_planes_kernel's frame_row) | row_mod
    if (!hi || !lo || !idx) return fail(-5, "op_layernorm_planes: hipMalloc");
    std::vector<int> h(2 * (size_t)M, 0);
    for (int i = 0; i < M; i++) { h[i] = i; if (row_mod_host) h[M + i] = row_mod_host[i]; }
    if (upload_sync(st, idx, h) != hipSuccess) return fail(-6, "op_layernorm_planes: upload");
    LnArgs ln = ln_args(x_dev, D, M, D, scale_dev, shift_dev, gain_off, eps);
    ln.out_hi = hi; ln.out_lo = out_format == 0 ? lo : nullptr; ln.ldo = D; ln.f16_out = out_format == 1;
    if (row_mod_host) { ln.row_mod = idx + M; ln.mod_ld = mod_ld; }
    CK(run_ln(ln, st, row_mod_host != nullptr));
    hipLaunchKernelGGL(op_unpack_planes_kernel, dim3(M), dim3(256), 0, st, hi, ln.out_lo, ln.f16_out, D, idx, out_dev);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(-7, "op_layernorm_planes: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

// One (pseudo-)sequence of the attention unit ops: query rows row0 .. + len (frames frame0 .. + len of the caller's q / k / v / out) over the
// key rows kv_row0 .. + kvlen and then, when kv2_len > 0, kv2_row0 .. + kv2_len (the two-range attn3 kernels)
struct AttnSeq { int row0, len, frame0, kv_row0, kvlen, kv2_row0 = 0, kv2_len = 0; };

// The attention unit ops over `seqs`, whose query rows tile a layout padded to 128 rows per (pseudo-)sequence: q / k / v fp32 frames are packed
// into the rows, attn3 runs (timed like the other ops: the warm-up launch writes the output) with AttnArgs::shape_invariant = `invariant`
// and the output format `out_format` (0: split-bf16 planes, 1: one fp16 plane, 2: the bf16 hi plane alone), and the output is read back
// into frame order.  qk, V^T and the output planes carry 256 zeroed slack rows: the last query tile may read (never store) past the padded rows.
static int attention_op(const char* name, const std::vector<AttnSeq>& seqs, int heads, const float* q_dev, const float* k_dev, const float* v_dev,
                        float* out_dev, int iters, double* avg_us, int invariant, int out_format, hipStream_t st) {
    if (invariant < -1 || invariant > 1 || out_format < 0 || out_format > 2) return fail(-1, "%s: bad shape_invariant / out_format", name);
    const int NS = (int)seqs.size(), D = heads * 64;
    int M_pad = 0, F = 0, max_len = 0;
    bool seg2 = false;
    for (const AttnSeq& s : seqs) {
        M_pad = std::max(M_pad, ceil_to(s.row0 + s.len, 128)); F += s.len; max_len = std::max(max_len, s.len);
        seg2 |= s.kv2_len > 0;
    }
    const int ld = M_pad + 256;
    std::vector<int> row_src(M_pad, -1), frame_row(F), meta(6 * NS);
    for (int i = 0; i < NS; i++) {
        const AttnSeq& s = seqs[i];
        for (int j = 0; j < s.len; j++) { row_src[s.row0 + j] = s.frame0 + j; frame_row[s.frame0 + j] = s.row0 + j; }
        const int fields[6] = {s.row0, s.len, s.kvlen, s.kv_row0, s.kv2_row0, s.kv2_len};   // AttnArgs::seq_row0 .. seq_kv2_len
        for (int a = 0; a < 6; a++) meta[a * NS + i] = fields[a];
    }
    OpBufs b;
    __bf16* qk = b.get<__bf16>((size_t)ld * 2 * D); __bf16* vt = b.get<__bf16>((size_t)D * ld);
    __bf16* ohi = b.get<__bf16>((size_t)ld * D); __bf16* olo = b.get<__bf16>((size_t)ld * D);
    int* d_rs = b.get<int>(M_pad); int* d_fr = b.get<int>(F); int* d_meta = b.get<int>(6 * NS);
    if (!qk || !vt || !ohi || !olo || !d_rs || !d_fr || !d_meta) return fail(-5, "%s: hipMalloc", name);
    if (hipMemsetAsync(qk, 0, sizeof(__bf16) * (size_t)ld * 2 * D, st) != hipSuccess || hipMemsetAsync(vt, 0, sizeof(__bf16) * (size_t)D * ld, st) != hipSuccess ||
        upload_sync(st, d_rs, row_src, d_fr, frame_row, d_meta, meta) != hipSuccess)
        return fail(-6, "%s: upload", name);
    hipLaunchKernelGGL(op_pack_qkv_kernel, dim3(M_pad), dim3(256), 0, st, q_dev, k_dev, v_dev, D, d_rs, ld, qk, vt);
    AttnArgs at; memset(&at, 0, sizeof(at));
    at.qk = qk; at.vt = vt; at.D = D; at.ldvt = ld; at.seq_row0 = d_meta; at.seq_len = d_meta + NS; at.seq_kvlen = d_meta + 2 * NS;
    if (seg2) { at.seq_kv_row0 = d_meta + 3 * NS; at.seq_kv2_row0 = d_meta + 4 * NS; at.seq_kv2_len = d_meta + 5 * NS; }
    at.out_hi = ohi; at.out_lo = out_format == 0 ? olo : nullptr; at.f16_out = out_format == 1; at.shape_invariant = invariant;
    CK(time_launches(1, iters, avg_us, st, [&](int) {
        const hipError_t e = f5_launch_attn3(at, max_len, heads, NS, st);
        return e == hipSuccess ? 0 : fail(-7, "%s launch: %s", name, hipGetErrorString(e));
    }));
    hipLaunchKernelGGL(op_unpack_planes_kernel, dim3(F), dim3(256), 0, st, ohi, at.out_lo, at.f16_out, D, d_fr, out_dev);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(-7, "%s: %s", name, hipGetErrorString(hipGetLastError()));
    return 0;
}

// softmax(q k^T / 8 + key-padding mask) v per (sequence, head), head dim 64 (F/model/modules.py:424-436): q / k / v fp32 [sum(seq_len)][64 heads]
// are rounded to fp16 like the QKV epilogue's outputs (q after the log2(e) / 8 scale); out fp32 [sum(seq_len)][64 heads] = the output in
// format out_format (attention_op).  impl must be 3 (attn3, the production kernel).
extern "C" int f5hip_op_attention(int32_t n_seq, const int32_t* seq_len, const int32_t* kv_len, int32_t heads, const float* q_dev,
                                  const float* k_dev, const float* v_dev, float* out_dev, int32_t impl, int32_t iters, double* avg_us, void* stream,
                                  int32_t shape_invariant, int32_t out_format) {
    if (n_seq <= 0 || !seq_len || heads <= 0 || !q_dev || !k_dev || !v_dev || !out_dev || impl != 3) return fail(-1, "op_attention: bad argument");
    std::vector<AttnSeq> seqs;
    for (int i = 0, r0 = 0, f0 = 0; i < n_seq; i++) {
        if (seq_len[i] <= 0 || seq_len[i] > 4096 || (kv_len && (kv_len[i] <= 0 || kv_len[i] > seq_len[i]))) return fail(-1, "op_attention: bad lengths");
        seqs.push_back({r0, seq_len[i], f0, r0, kv_len ? kv_len[i] : seq_len[i]});
        r0 += ceil_to(seq_len[i], 128); f0 += seq_len[i];
    }
    return attention_op("op_attention", seqs, heads, q_dev, k_dev, v_dev, out_dev, iters, avg_us, shape_invariant, out_format, (hipStream_t)stream);
}

// Joint attention of the MMDiT blocks (JointAttnProcessor, F/model/modules.py:496-522): per sequence the queries and the keys are the
// audio rows followed by the text rows; padding is masked on the audio keys only (x_kvlen <= x_len valid audio keys, every text key).
// q / k / v / out fp32 [sum(x_len) + sum(c_len)][64 heads]: all audio frames sequence by sequence, then all text tokens sequence by
// sequence.  Runs the two-range attn3 kernels over 2 n_seq pseudo-sequences (audio queries, text queries) that share the key ranges.
extern "C" int f5hip_op_joint_attention(int32_t n_seq, const int32_t* x_len, const int32_t* x_kvlen, const int32_t* c_len, int32_t heads,
                                        const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, void* stream,
                                        int32_t shape_invariant, int32_t out_format) {
    if (n_seq <= 0 || !x_len || !c_len || heads <= 0 || !q_dev || !k_dev || !v_dev || !out_dev) return fail(-1, "op_joint_attention: bad argument");
    int Mx = 0, Fx = 0;   // audio rows and frames come first, the text rows and tokens behind them
    for (int i = 0; i < n_seq; i++) {
        if (x_len[i] <= 0 || x_len[i] > 4096 || c_len[i] <= 0 || c_len[i] > 4096 || (x_kvlen && (x_kvlen[i] <= 0 || x_kvlen[i] > x_len[i])))
            return fail(-1, "op_joint_attention: bad lengths");
        Mx += ceil_to(x_len[i], 128); Fx += x_len[i];
    }
    std::vector<AttnSeq> seqs;   // pseudo-sequence 2 i: the audio queries of sequence i, 2 i + 1: its text queries
    for (int i = 0, rx = 0, rc = Mx, fx = 0, fc = Fx; i < n_seq; i++) {
        const int kv = x_kvlen ? x_kvlen[i] : x_len[i];
        seqs.push_back({rx, x_len[i], fx, rx, kv, rc, c_len[i]});
        seqs.push_back({rc, c_len[i], fc, rx, kv, rc, c_len[i]});
        rx += ceil_to(x_len[i], 128); rc += ceil_to(c_len[i], 128); fx += x_len[i]; fc += c_len[i];
    }
    return attention_op("op_joint_attention", seqs, heads, q_dev, k_dev, v_dev, out_dev, 0, nullptr, shape_invariant, out_format, (hipStream_t)stream);
}

// One Conv1d of the BigVGAN kind over channel-last rows -- batch sequences of pitch P rows, T valid -- through the library's two paths:
// impl 0 = gemm.h implicit GEMM (A window re-read per tap), 5 = conv5.h (window once in LDS).  x_dev fp32 [batch * P][c_in],
// w_host [c_out][c_in][k], out_dev fp32 [batch * P][c_out] (= conv + bias + res).  prec 2 = split bf16, 3 = fp16.
// stamps_host (optional, impl 5, wide shapes): [blocks][16] cycle stamps of the diagnostics kernel (conv5.h).
extern "C" int f5hip_op_conv1d(int32_t batch, int32_t P, int32_t T, int32_t c_in, int32_t c_out, int32_t k, int32_t dil, const float* x_dev,
                               const float* w_host, const float* bias_host, const float* res_dev, float* out_dev, int32_t prec, int32_t impl,
                               int32_t iters, double* avg_us, uint64_t* stamps_host, int32_t stamp_blocks, void* stream) {
    if (batch <= 0 || P <= 0 || T <= 0 || T > P || P % 128 || c_in <= 0 || c_in % 4 || c_out <= 0 || k < 1 || !(k & 1) || dil < 1 || !x_dev || !w_host || !out_dev ||
        (prec != 2 && prec != 3) || (impl != 0 && impl != 5))
        return fail(-1, "op_conv1d: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int M = batch * P, cpad = ceil_to(c_in, 32);
    BvConv c;
    const std::vector<float> w(w_host, w_host + (size_t)c_out * c_in * k);
    std::vector<float> bias(c_out, 0.0f);
    if (bias_host) bias.assign(bias_host, bias_host + c_out);
    if (bv_pack_conv(c, w, bias.data(), c_out, c_in, k, dil, prec == 3)) return -4;
    OpBufs b;
    Plane2 A;
    A.hi = b.get<__bf16>((size_t)M * cpad + 4096); A.lo = b.get<__bf16>((size_t)M * cpad + 4096);
    unsigned long long* stamps = stamps_host ? b.get<unsigned long long>((size_t)stamp_blocks * 16) : nullptr;
    if (!A.hi || !A.lo || (stamps_host && !stamps)) { bv_free_conv(c); return fail(-5, "op_conv1d: hipMalloc"); }
    (void)hipMemsetAsync(A.hi, 0, ((size_t)M * cpad + 4096) * 2, st);
    (void)hipMemsetAsync(A.lo, 0, ((size_t)M * cpad + 4096) * 2, st);
    const size_t n4 = (size_t)M * c_in / 4;
    hipLaunchKernelGGL(bv_mean3_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, x_dev, x_dev, x_dev, 1, (size_t)M, c_in, (float*)nullptr, A.hi, A.lo, cpad,
                       prec == 3 ? 2 : 1);
    auto run = [&](float* out, const float* res, unsigned long long* stm) {   // impl 5: conv5 or an error, never the gemm.h fallback
        GemmArgs g = conv_args(c, A, M, P, T, res, out);
        g.stamps = stm;
        return run_conv(prec, g, c.w, impl == 5, false, c.w.n_pad % 128 ? 64 : 128, st);
    };
    int rc = run(out_dev, res_dev, nullptr);
    if (!rc && iters > 0 && avg_us) {
        float* scratch = b.get<float>((size_t)M * c_out);
        rc = scratch ? time_launches(3, iters, avg_us, st, [&](int) { return run(scratch, nullptr, nullptr); }) : fail(-5, "op_conv1d: hipMalloc scratch");
        if (!rc && stamps) {
            (void)hipMemsetAsync(stamps, 0, (size_t)stamp_blocks * 16 * 8, st);
            rc = run(scratch, nullptr, stamps);
            if (!rc && (hipMemcpyAsync(stamps_host, stamps, (size_t)stamp_blocks * 16 * 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess))
                rc = fail(-6, "op_conv1d: stamp download");
        }
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(-6, "op_conv1d: sync");
    bv_free_conv(c);
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------- BigVGAN unit ops
// operand planes -> fp32, n elements: hi + lo (split bf16) or hi read as one fp16 plane
__global__ __launch_bounds__(256) void op_planes_to_f32_kernel(const __bf16* hi, const __bf16* lo, int f16, size_t n, float* out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = f16 ? (float)reinterpret_cast<const _Float16*>(hi)[i] : (float)hi[i] + (float)lo[i];
}

// Activation1d(SnakeBeta) of the generator (bv_snake_launch: aa_snake2_kernel) over fp32 rows x [batch P][C], uniform sequences of pitch P
// with T valid.  out_format 0: fp32 straight into out_dev; 1 / 2: split-bf16 / fp16 planes of out_rows rows, loaded from out_dev first (so
// what the kernel does not write comes back as it was, up to that rounding) and read back into out_dev as fp32.
extern "C" int f5hip_op_bigvgan_snake(int32_t batch, int32_t P, int32_t T, int32_t C, const float* x_dev, const float* alpha_log_dev,
                                      const float* beta_log_dev, int32_t out_format, float* out_dev, int64_t out_rows, void* stream) {
    if (batch <= 0 || P <= 0 || T <= 0 || T > P || C <= 0 || C % 4 || !x_dev || !alpha_log_dev || !beta_log_dev || !out_dev || out_format < 0 ||
        out_format > 2 || out_rows < (int64_t)batch * P)
        return fail(-1, "op_bigvgan_snake: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int M = batch * P;
    AaFilt f;
    bv_aa_filter(f.f);
    OpBufs b;   // freed after the final synchronisation
    int rc;
    if (out_format == 0) {
        rc = bv_snake_launch(x_dev, C, M, P, T, alpha_log_dev, beta_log_dev, f, 0, nullptr, nullptr, out_dev, C, st);
    } else {
        const size_t n = (size_t)out_rows * C, n4 = n / 4;
        __bf16* hi = b.get<__bf16>(n); __bf16* lo = b.get<__bf16>(n);
        if (!hi || !lo) return fail(-5, "op_bigvgan_snake: hipMalloc");
        hipLaunchKernelGGL(bv_mean3_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, out_dev, out_dev, out_dev, 1, (size_t)out_rows, C, (float*)nullptr,
                           hi, lo, C, out_format == 2 ? 2 : 1);
        rc = bv_snake_launch(x_dev, C, M, P, T, alpha_log_dev, beta_log_dev, f, out_format, hi, lo, nullptr, C, st);
        if (!rc) hipLaunchKernelGGL(op_planes_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, hi, lo, out_format == 2 ? 1 : 0, n, out_dev);
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(-7, "op_bigvgan_snake: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

// One up-sampler of the generator: ConvTranspose1d(c_in -> c_out, k = 2 r, stride r, padding r / 2) + bias, packed by bv_pack_ups and run by
// bv_conv (conv5.h where it covers the shape, else gemm.h).  x_dev fp32 [batch P][c_in] (P % 128 == 0, T valid), w_host [c_in][c_out][2 r],
// bias_host [c_out] or NULL; out_dev fp32 [batch P r][c_out].  prec 2 = split bf16, 3 = one fp16 plane.
extern "C" int f5hip_op_bigvgan_upsample(int32_t batch, int32_t P, int32_t T, int32_t c_in, int32_t c_out, int32_t r, const float* x_dev,
                                         const float* w_host, const float* bias_host, float* out_dev, int32_t prec, void* stream) {
    if (batch <= 0 || P <= 0 || T <= 0 || T > P || P % 128 || c_in <= 0 || c_in % 4 || c_out <= 0 || r < 2 || r % 2 || !x_dev || !w_host || !out_dev ||
        (prec != 2 && prec != 3))
        return fail(-1, "op_bigvgan_upsample: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int M = batch * P, cpad = ceil_to(c_in, 32);
    std::vector<float> bias(c_out, 0.0f);
    if (bias_host) bias.assign(bias_host, bias_host + c_out);
    BvConv u;
    if (bv_pack_ups(u, w_host, bias.data(), c_in, c_out, r, prec == 3)) return -4;
    OpBufs b;
    Plane2 A;
    A.hi = b.get<__bf16>((size_t)M * cpad + 4096); A.lo = b.get<__bf16>((size_t)M * cpad + 4096);
    if (!A.hi || !A.lo) { bv_free_conv(u); return fail(-5, "op_bigvgan_upsample: hipMalloc"); }
    (void)hipMemsetAsync(A.hi, 0, ((size_t)M * cpad + 4096) * 2, st);
    (void)hipMemsetAsync(A.lo, 0, ((size_t)M * cpad + 4096) * 2, st);
    const size_t n4 = (size_t)M * c_in / 4;
    hipLaunchKernelGGL(bv_mean3_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, x_dev, x_dev, x_dev, 1, (size_t)M, c_in, (float*)nullptr, A.hi, A.lo, cpad,
                       prec == 3 ? 2 : 1);
    int rc = bv_conv(prec, u, A, M, P, T, nullptr, out_dev, st);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(-6, "op_bigvgan_upsample: sync");
    bv_free_conv(u);
    return rc;
}

// conv_post + clamp of the generator (bv_conv_post): a_dev fp32 [batch P][C] (T valid rows per sequence), w_dev fp32 [C][7] (conv_post.weight),
// wave_dev fp32 [batch][T].  variant 0: the generator's choice, 1: the LDS kernel (fails when its tile exceeds 48 KB), 2: the naive kernel.
extern "C" int f5hip_op_bigvgan_conv_post(int32_t batch, int32_t P, int32_t T, int32_t C, const float* a_dev, const float* w_dev, int32_t variant,
                                          float* wave_dev, void* stream) {
    if (batch <= 0 || P <= 0 || T <= 0 || T > P || C <= 0 || !a_dev || !w_dev || !wave_dev || variant < 0 || variant > 2)
        return fail(-1, "op_bigvgan_conv_post: bad argument");
    hipStream_t st = (hipStream_t)stream;
    int rc = bv_conv_post(a_dev, C, C, batch, P, T, w_dev, wave_dev, variant, st);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(-7, "op_bigvgan_conv_post: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------- BigVGAN unit ops, ragged forms
// The layouts of f5hip_bigvgan_forward_ragged, described by the caller in rows of the stage the op runs at; the ops build the tables the
// kernels take (BvRagged) and launch as bv_generate does.

// One [start, end) per block of blk rows over M rows from n items (item i: rows [row0[i], row0[i] + rows[i]), the first valid[i] valid; rows
// null: ceil(valid / align) align).  Every item starts at, and spans, a multiple of `align` rows (a multiple of blk), and every block belongs
// to exactly one item.  tab = start [M / blk], end [M / blk].
static int op_block_table(const char* name, int n, const int32_t* row0, const int32_t* rows, const int32_t* valid, int M, int blk, int align,
                          std::vector<int>& tab) {
    const int nblk = M / blk;
    tab.assign((size_t)2 * nblk, -1);
    for (int i = 0; i < n; i++) {
        const long long r0 = row0[i], v = valid[i], p = rows ? rows[i] : (v + align - 1) / align * align;
        if (r0 < 0 || v <= 0 || v > p || r0 + p > M) return fail(-1, "%s: item %d (rows %lld + %lld, %lld valid) outside the %d rows", name, i, r0, p, v, M);
        if (r0 % align || p % align) return fail(-1, "%s: item %d (rows %lld + %lld) is not aligned to %d rows", name, i, r0, p, align);
        for (int b = (int)(r0 / blk); b < (int)((r0 + p) / blk); b++) {
            if (tab[b] >= 0) return fail(-1, "%s: block %d belongs to two items", name, b);
            tab[b] = (int)r0; tab[nblk + b] = (int)(r0 + v);
        }
    }
    for (int b = 0; b < nblk; b++)
        if (tab[b] < 0) return fail(-1, "%s: block %d belongs to no item", name, b);
    return 0;
}

// int4 items of BvRagged from n items given in rows at `scale`: (row0, valid, wave offset (0 when off is null), index) / scale.  Every
// item lies inside the M rows, its wave inside wave_len samples, and all three are multiples of scale.  t_max = the longest item's rows.
static int op_item_table(const char* name, int n, const int32_t* row0, const int32_t* valid, const int32_t* off, int scale, long long M, long long wave_len,
                         std::vector<int>& h, int& t_max) {
    if (n <= 0 || n > 65535 || !row0 || !valid || scale <= 0) return fail(-1, "%s: bad item table", name);
    h.assign((size_t)4 * n, 0);
    t_max = 0;
    for (int i = 0; i < n; i++) {
        const long long r0 = row0[i], v = valid[i], o = off ? off[i] : 0;
        if (r0 < 0 || v <= 0 || r0 + v > M || o < 0 || (off && o + v > wave_len)) return fail(-1, "%s: item %d out of range", name, i);
        if (r0 % scale || v % scale || o % scale) return fail(-1, "%s: item %d is not a multiple of scale %d", name, i, scale);
        h[4 * i] = (int)(r0 / scale); h[4 * i + 1] = (int)(v / scale); h[4 * i + 2] = (int)(o / scale); h[4 * i + 3] = i;
        t_max = std::max(t_max, (int)v);
    }
    return 0;
}

// f5hip_op_conv1d over ragged items: bounds per block of blk rows (GemmArgs::seq_blk), as bv_generate's convolutions pass them.  ups_rate > 0:
// the 3-tap form of an up-sampler (w_host [c_in][c_out][2 ups_rate], out_dev [M ups_rate][c_out], no residual; k and dil are not read).
extern "C" int f5hip_op_conv1d_ragged(int32_t n_items, const int32_t* item_row0, const int32_t* item_rows, const int32_t* item_valid, int32_t M,
                                      int32_t blk, int32_t c_in, int32_t c_out, int32_t k, int32_t dil, int32_t ups_rate, const float* x_dev,
                                      const float* w_host, const float* bias_host, const float* res_dev, float* out_dev, int32_t prec,
                                      int32_t impl, void* stream) {
    const bool ups = ups_rate > 0;
    if (n_items <= 0 || !item_row0 || !item_valid || M <= 0 || blk <= 0 || blk % 128 || M % blk || c_in <= 0 || c_in % 4 || c_out <= 0 || !x_dev || !w_host ||
        !out_dev || (prec != 2 && prec != 3) || (impl != 0 && impl != 5) || ups_rate < 0 ||
        (ups ? (ups_rate < 2 || ups_rate % 2 || res_dev != nullptr) : (k < 1 || !(k & 1) || dil < 1)))
        return fail(-1, "op_conv1d_ragged: bad argument");
    // conv5.h takes a tile's bounds from its first row: the 256-row tile must lie in one item, so blk is 128 (two entries per tile, the
    // items 256-aligned) or a multiple of 256
    if (impl == 5 && (M % 256 || (blk != 128 && blk % 256))) return fail(-1, "op_conv1d_ragged: blk %d does not fit the 256-row tile of conv5", blk);
    const int align = impl == 5 && blk == 128 ? 256 : blk;
    std::vector<int> tab;
    CK(op_block_table("op_conv1d_ragged", n_items, item_row0, item_rows, item_valid, M, blk, align, tab));
    hipStream_t st = (hipStream_t)stream;
    const int cpad = ceil_to(c_in, 32), nblk = M / blk;
    std::vector<float> bias(c_out, 0.0f);
    if (bias_host) bias.assign(bias_host, bias_host + c_out);
    BvConv c;
    if (ups) {
        if (bv_pack_ups(c, w_host, bias.data(), c_in, c_out, ups_rate, prec == 3)) return -4;
    } else {
        const std::vector<float> w(w_host, w_host + (size_t)c_out * c_in * k);
        if (bv_pack_conv(c, w, bias.data(), c_out, c_in, k, dil, prec == 3)) return -4;
    }
    OpBufs b;
    Plane2 A;
    A.hi = op_filled<__bf16>(b, (size_t)M * cpad + 4096, 0, st); A.lo = op_filled<__bf16>(b, (size_t)M * cpad + 4096, 0, st);
    int* d_tab = b.get<int>(tab.size());
    if (!A.hi || !A.lo || !d_tab) { bv_free_conv(c); return fail(-5, "op_conv1d_ragged: hipMalloc"); }
    int rc = upload_sync(st, d_tab, tab) != hipSuccess ? fail(-6, "op_conv1d_ragged: upload") : 0;
    if (!rc) {
        const size_t n4 = (size_t)M * c_in / 4;
        hipLaunchKernelGGL(bv_mean3_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, x_dev, x_dev, x_dev, 1, (size_t)M, c_in, (float*)nullptr, A.hi, A.lo,
                           cpad, prec == 3 ? 2 : 1);
        GemmArgs g = conv_args(c, A, M, align, 0, res_dev, out_dev, d_tab, d_tab + nblk, blk);
        rc = run_conv(prec, g, c.w, impl == 5, false, c.w.n_pad % 128 ? 64 : 128, st);   // impl 5: conv5 or an error, never the gemm.h fallback
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(-6, "op_conv1d_ragged: sync");
    bv_free_conv(c);
    return rc;
}

// f5hip_op_bigvgan_snake over ragged items (grid z = item, bv_snake_launch with items / scale); x_dev fp32 [M][C], out_dev as in the uniform op
extern "C" int f5hip_op_bigvgan_snake_ragged(int32_t n_items, const int32_t* item_row0, const int32_t* item_valid, int32_t scale, int32_t M, int32_t C,
                                             const float* x_dev, const float* alpha_log_dev, const float* beta_log_dev, int32_t out_format,
                                             float* out_dev, int64_t out_rows, void* stream) {
    if (M <= 0 || C <= 0 || C % 4 || !x_dev || !alpha_log_dev || !beta_log_dev || !out_dev || out_format < 0 || out_format > 2 || out_rows < M)
        return fail(-1, "op_bigvgan_snake_ragged: bad argument");
    std::vector<int> h;
    int t_max = 0;
    CK(op_item_table("op_bigvgan_snake_ragged", n_items, item_row0, item_valid, nullptr, scale, M, 0, h, t_max));
    hipStream_t st = (hipStream_t)stream;
    AaFilt f;
    bv_aa_filter(f.f);
    OpBufs b;   // freed after the final synchronisation
    int* items = b.get<int>(h.size());
    if (!items) return fail(-5, "op_bigvgan_snake_ragged: hipMalloc");
    if (upload_sync(st, items, h) != hipSuccess) return fail(-6, "op_bigvgan_snake_ragged: upload");
    const int4* it = reinterpret_cast<const int4*>(items);
    int rc;
    if (out_format == 0) {
        rc = bv_snake_launch(x_dev, C, M, 0, t_max, alpha_log_dev, beta_log_dev, f, 0, nullptr, nullptr, out_dev, C, st, it, n_items, scale);
    } else {
        const size_t n = (size_t)out_rows * C, n4 = n / 4;
        __bf16* hi = b.get<__bf16>(n); __bf16* lo = b.get<__bf16>(n);
        if (!hi || !lo) return fail(-5, "op_bigvgan_snake_ragged: hipMalloc");
        hipLaunchKernelGGL(bv_mean3_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, out_dev, out_dev, out_dev, 1, (size_t)out_rows, C, (float*)nullptr,
                           hi, lo, C, out_format == 2 ? 2 : 1);
        rc = bv_snake_launch(x_dev, C, M, 0, t_max, alpha_log_dev, beta_log_dev, f, out_format, hi, lo, nullptr, C, st, it, n_items, scale);
        if (!rc) hipLaunchKernelGGL(op_planes_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, hi, lo, out_format == 2 ? 1 : 0, n, out_dev);
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(-7, "op_bigvgan_snake_ragged: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

// f5hip_op_bigvgan_conv_post over ragged items (grid y = item): a_dev fp32 [M][C]; item i writes wave_dev [item_wave_off[i], + item_valid[i])
// of the wave_len samples and nothing else
extern "C" int f5hip_op_bigvgan_conv_post_ragged(int32_t n_items, const int32_t* item_row0, const int32_t* item_valid, const int32_t* item_wave_off,
                                                 int32_t scale, int32_t M, int32_t C, const float* a_dev, const float* w_dev, int32_t variant,
                                                 float* wave_dev, int64_t wave_len, void* stream) {
    if (M <= 0 || C <= 0 || !a_dev || !w_dev || !wave_dev || !item_wave_off || wave_len <= 0 || variant < 0 || variant > 2)
        return fail(-1, "op_bigvgan_conv_post_ragged: bad argument");
    std::vector<int> h;
    int t_max = 0;
    CK(op_item_table("op_bigvgan_conv_post_ragged", n_items, item_row0, item_valid, item_wave_off, scale, M, wave_len, h, t_max));
    hipStream_t st = (hipStream_t)stream;
    OpBufs b;
    int* items = b.get<int>(h.size());
    if (!items) return fail(-5, "op_bigvgan_conv_post_ragged: hipMalloc");
    if (upload_sync(st, items, h) != hipSuccess) return fail(-6, "op_bigvgan_conv_post_ragged: upload");
    int rc = bv_conv_post(a_dev, C, C, n_items, 0, t_max, w_dev, wave_dev, variant, st, reinterpret_cast<const int4*>(items), scale);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(-7, "op_bigvgan_conv_post_ragged: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

// bv_mean3_kernel: (y0 + y1 + y2) / 3 (n_in 3) or y0 (n_in 1) over fp32 rows [rows][C] -> fp32 rows out_f32_dev [rows][C] (or null) and / or,
// mode 1 / 2 / 3, split-bf16 / fp16 / bf16 planes of pitch ldo.  The planes are loaded from planes_dev fp32 [rows][ldo] first and read
// back into it as fp32 (hi + lo; the lo plane starts as zero in mode 3), so the padding channels come back as they were, up to the format.
extern "C" int f5hip_op_bigvgan_mean3(int64_t rows, int32_t C, int32_t n_in, const float* y0_dev, const float* y1_dev, const float* y2_dev,
                                      int32_t mode, int32_t ldo, float* out_f32_dev, float* planes_dev, void* stream) {
    if (rows <= 0 || C <= 0 || C % 4 || (n_in != 1 && n_in != 3) || !y0_dev || (n_in == 3 && (!y1_dev || !y2_dev)) || mode < 0 || mode > 3 ||
        (mode == 0 ? !out_f32_dev : (!planes_dev || ldo < C || ldo % 4)) || rows * (int64_t)std::max(C, ldo) / 4 > (int64_t)256 * 2147483647)
        return fail(-1, "op_bigvgan_mean3: bad argument");
    hipStream_t st = (hipStream_t)stream;
    OpBufs b;
    __bf16 *hi = nullptr, *lo = nullptr;
    const size_t n = mode ? (size_t)rows * ldo : 0;
    if (mode) {
        hi = b.get<__bf16>(n); lo = op_filled<__bf16>(b, n, 0, st);
        if (!hi || !lo) return fail(-5, "op_bigvgan_mean3: hipMalloc");
        hipLaunchKernelGGL(bv_mean3_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, planes_dev, planes_dev, planes_dev, 1, (size_t)rows, ldo,
                           (float*)nullptr, hi, lo, ldo, mode);
    }
    const size_t n4 = (size_t)rows * C / 4;
    hipLaunchKernelGGL(bv_mean3_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, y0_dev, n_in == 3 ? y1_dev : y0_dev, n_in == 3 ? y2_dev : y0_dev, n_in,
                       (size_t)rows, C, out_f32_dev, hi, lo, ldo, mode);
    if (mode) hipLaunchKernelGGL(op_planes_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, hi, lo, mode == 2 ? 1 : 0, n, planes_dev);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(-7, "op_bigvgan_mean3: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

// bv_mel_rows_kernel (item_row0 null: n uniform sequences of pitch M0 / n rows, mel_dev [n][C][T]) or bv_mel_rows_ragged_kernel (item i:
// item_frames[i] frames from row item_row0[i], a multiple of 128; mel_dev [n][C][T], T = the column stride; every 128-row block belongs to
// one item) -> out_dev fp32 [M0][128], the planes (split bf16 hi + lo, or the fp16 plane) the kernel wrote over planes of NaN.
extern "C" int f5hip_op_bigvgan_mel_rows(int32_t n, const int32_t* item_row0, const int32_t* item_frames, int32_t T, int32_t M0, int32_t C,
                                         const float* mel_dev, int32_t f16, float* out_dev, void* stream) {
    if (n <= 0 || T <= 0 || M0 <= 0 || C <= 0 || C > 128 || !mel_dev || !out_dev || (item_row0 ? (!item_frames || M0 % 128) : (M0 % n || M0 / n < T)))
        return fail(-1, "op_bigvgan_mel_rows: bad argument");
    hipStream_t st = (hipStream_t)stream;
    OpBufs b;
    const size_t ne = (size_t)M0 * 128;
    __bf16* hi = op_filled<__bf16>(b, ne, 0xff, st); __bf16* lo = op_filled<__bf16>(b, ne, 0xff, st);
    if (!hi || !lo) return fail(-5, "op_bigvgan_mel_rows: hipMalloc");
    if (item_row0) {
        const int nblk = M0 / 128;
        std::vector<int> tab, h((size_t)3 * nblk, 0);
        for (int i = 0; i < n; i++)
            if (item_frames[i] > T) return fail(-1, "op_bigvgan_mel_rows: item %d has %d frames, the column stride is %d", i, item_frames[i], T);
        CK(op_block_table("op_bigvgan_mel_rows", n, item_row0, nullptr, item_frames, M0, 128, 128, tab));
        std::copy(tab.begin(), tab.end(), h.begin());
        for (int i = 0; i < n; i++)
            for (int r = item_row0[i]; r < item_row0[i] + item_frames[i]; r += 128) h[(size_t)2 * nblk + r / 128] = i;
        int* d = b.get<int>(h.size());
        if (!d) return fail(-5, "op_bigvgan_mel_rows: hipMalloc");
        if (upload_sync(st, d, h) != hipSuccess) return fail(-6, "op_bigvgan_mel_rows: upload");
        hipLaunchKernelGGL(bv_mel_rows_ragged_kernel, dim3(M0), dim3(128), 0, st, mel_dev, C, T, d, d + nblk, d + 2 * nblk, hi, lo, f16 ? 1 : 0);
    } else {
        hipLaunchKernelGGL(bv_mel_rows_kernel, dim3(M0), dim3(128), 0, st, mel_dev, C, T, M0 / n, hi, lo, f16 ? 1 : 0);
    }
    hipLaunchKernelGGL(op_planes_to_f32_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, hi, lo, f16 ? 1 : 0, ne, out_dev);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(-7, "op_bigvgan_mel_rows: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- DiT input-side unit ops
// frame f of x [n][C] -> row frame_row[f] of dst (pitch ldd), and its split-bf16 planes (pitch ldd) when hi is not null
__global__ __launch_bounds__(256) void op_scatter_rows_kernel(const float* x, int C, int n, const int* frame_row, float* dst, __bf16* hi, __bf16* lo,
                                                              int ldd) {
    const int f = blockIdx.x;
    if (f >= n) return;
    const size_t r = (size_t)frame_row[f];
    for (int c = threadIdx.x; c < C; c += 256) {
        const float v = x[(size_t)f * C + c];
        if (dst) dst[r * ldd + c] = v;
        if (hi) {
            __bf16 h, l;
            split_bf16(v, h, l);
            hi[r * ldd + c] = h;
            lo[r * ldd + c] = l;
        }
    }
}

// row frame_row[f] of planes (pitch lds) -> dst [n][C] as fp32: hi + lo, or hi alone when lo is null (what a one-plane bf16 consumer reads)
__global__ __launch_bounds__(256) void op_gather_planes_kernel(const __bf16* hi, const __bf16* lo, int lds, int C, int n, const int* frame_row, float* dst) {
    const int f = blockIdx.x;
    if (f >= n) return;
    const size_t r = (size_t)frame_row[f];
    for (int c = threadIdx.x; c < C; c += 256) dst[(size_t)f * C + c] = (float)hi[r * lds + c] + (lo ? (float)lo[r * lds + c] : 0.0f);
}

// The packed layout the backbone builds for n_seq sequences of seq_len frames with `lead` leading rows each (seq_rows / set_seq_bounds), on the
// device: row_start, row_end, row_seq [R]; frame_row [frames]; seq_row0, seq_len [n_seq] (first row and rows of a sequence, lead included)
struct OpLayout { int R = 0, frames = 0; int *row_start = nullptr, *row_end, *row_seq, *frame_row, *seq_row0, *seq_len; std::vector<int> h; };
static int op_layout(OpBufs& b, int n_seq, const int32_t* seq_len, int lead, OpLayout& L, hipStream_t st) {
    L.R = 0; L.frames = 0;
    for (int s = 0; s < n_seq; s++) {
        if (seq_len[s] <= 0 || seq_len[s] > 4096) return fail(-1, "seq_len[%d] = %d out of range", s, seq_len[s]);
        L.R += seq_rows(seq_len[s], lead); L.frames += seq_len[s];
    }
    const int R = L.R, F = L.frames;
    L.h.assign((size_t)3 * R + F + 2 * n_seq, 0);
    int *rs = L.h.data(), *re = rs + R, *rq = re + R, *fr = rq + R, *s0 = fr + F, *sl = s0 + n_seq;
    for (int r = 0; r < R; r++) rq[r] = -1;
    for (int s = 0, r0 = 0, f0 = 0; s < n_seq; s++) {
        set_seq_bounds(rs, re, rq, r0, lead, seq_len[s], s);
        for (int i = 0; i < seq_len[s]; i++) fr[f0 + i] = r0 + lead + i;
        s0[s] = r0; sl[s] = lead + seq_len[s];
        r0 += seq_rows(seq_len[s], lead); f0 += seq_len[s];
    }
    int* d = b.get<int>(L.h.size());
    if (!d) return fail(-5, "op layout: hipMalloc");
    if (hipMemcpyAsync(d, L.h.data(), sizeof(int) * L.h.size(), hipMemcpyHostToDevice, st) != hipSuccess) return fail(-6, "op layout: upload");
    L.row_start = d; L.row_end = d + R; L.row_seq = d + 2 * R; L.frame_row = d + 3 * R; L.seq_row0 = L.frame_row + F; L.seq_len = L.seq_row0 + n_seq;
    return 0;
}

// ConvPositionEmbedding of the backbone (run_conv_pos_embed, weights packed by pack_conv_pos): out = h0 + Mish(conv2(Mish(conv1(h0)))) over
// n_seq sequences of seq_len frames, x_dev fp32 [frames][D] (packed).  Weights in nn.Conv1d layout w [D][D / 16][31], bias [D] (host).
// lead = 1: the UNetT layout (a time-token row heads every sequence).  impl 5 = conv5.h (prec 2, lead 0), 0 = gemm.h; prec 2 = split bf16,
// 1 = bf16.  pad_nan: the padding rows, the time-token rows and the slack past the last row of every internal buffer hold NaN instead of 0.
// c1_dev (or null) fp32 [frames][D]: stage 1 as the second convolution reads it (hi + lo; the hi plane alone at prec 1).
extern "C" int f5hip_op_conv_pos_embed(int32_t n_seq, const int32_t* seq_len, int32_t lead, int32_t D, const float* x_dev, const float* w1_host,
                                       const float* b1_host, const float* w2_host, const float* b2_host, int32_t impl, int32_t prec, int32_t pad_nan,
                                       float* out_dev, float* c1_dev, void* stream) {
    if (n_seq <= 0 || !seq_len || lead < 0 || lead > 1 || D <= 0 || D % 128 || D / 16 > 64 || !x_dev || !w1_host || !b1_host || !w2_host || !b2_host ||
        !out_dev || (impl != 0 && impl != 5) || (prec != 1 && prec != 2) || (impl == 5 && (prec != 2 || lead)))
        return fail(-1, "op_conv_pos_embed: bad argument");
    hipStream_t st = (hipStream_t)stream;
    OpBufs b;
    OpLayout L;
    CK(op_layout(b, n_seq, seq_len, lead, L, st));
    const size_t n = (size_t)L.R * D, slack = 256;
    const int pad = pad_nan ? 0xff : 0;
    float* h0 = op_filled<float>(b, n + slack, pad, st);
    float* h = op_filled<float>(b, n + slack, pad, st);
    Plane2 hn, c1;
    hn.hi = op_filled<__bf16>(b, n + slack, pad, st); hn.lo = op_filled<__bf16>(b, n + slack, pad, st);
    c1.hi = op_filled<__bf16>(b, n + slack, pad, st); c1.lo = op_filled<__bf16>(b, n + slack, pad, st);
    if (!h0 || !h || !hn.hi || !hn.lo || !c1.hi || !c1.lo) return fail(-5, "op_conv_pos_embed: hipMalloc");
    hipLaunchKernelGGL(op_scatter_rows_kernel, dim3(L.frames), dim3(256), 0, st, x_dev, D, L.frames, L.frame_row, h0, hn.hi, hn.lo, D);
    CKL("op scatter");
    PackedW w1, w2;
    int rc = pack_conv_pos(w1, w1_host, b1_host, D);
    if (!rc) rc = pack_conv_pos(w2, w2_host, b2_host, D);
    if (!rc) rc = run_conv_pos_embed(prec, impl == 5, D, L.R, hn, c1, h0, h, w1, w2, L.row_start, L.row_end, st);
    if (!rc) {
        hipLaunchKernelGGL(gather_rows_kernel, dim3(L.frames), dim3(128), 0, st, h, D, D, L.frames, L.frame_row, out_dev, D);
        if (c1_dev) hipLaunchKernelGGL(op_gather_planes_kernel, dim3(L.frames), dim3(256), 0, st, c1.hi, prec == 2 ? c1.lo : nullptr, D, D, L.frames,
                                       L.frame_row, c1_dev);
        if (hipGetLastError() != hipSuccess) rc = fail(-7, "op_conv_pos_embed: gather launch");
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(-7, "op_conv_pos_embed: %s", hipGetErrorString(hipGetLastError()));
    free_packed(w1); free_packed(w2);
    return rc;
}

// One ConvNeXtV2 text block of the backbone (run_text_block, split-bf16 GEMMs) in place over n_seq sequences of seq_len tokens, x_dev fp32
// [tokens][Td] (packed).  params_host: 10 host fp32 arrays in the module's layout -- dwconv.weight [Td][1][7], dwconv.bias, norm.weight,
// norm.bias [Td], pwconv1.weight [2 Td][Td], pwconv1.bias, grn.gamma, grn.beta [2 Td], pwconv2.weight [Td][2 Td], pwconv2.bias [Td].
// pad_nan: the padding rows of every internal buffer hold NaN instead of 0.  out_dev fp32 [tokens][Td]; the stage taps (each fp32 or
// null) as the next kernel reads them: tap_ln [tokens][Td] dwconv + LayerNorm (hi + lo), tap_ty [tokens][2 Td] pwconv1 + GELU, tap_grn
// [tokens][2 Td] GRN (hi + lo); f5hip_op_convnext_block_gx also tap_gx [n_seq][2 Td], the GRN column norms (grn_stats_kernel's output).
static int op_convnext_block_run(int32_t n_seq, const int32_t* seq_len, int32_t Td, const float* x_dev, const float* const* params_host, int32_t pad_nan,
                                 float* out_dev, float* tap_ln_dev, float* tap_ty_dev, float* tap_grn_dev, float* tap_gx_dev, void* stream) {
    if (n_seq <= 0 || !seq_len || Td <= 0 || Td % 32 || Td > 1536 || !x_dev || !params_host || !out_dev) return fail(-1, "op_convnext_block: bad argument");
    for (int i = 0; i < 10; i++) if (!params_host[i]) return fail(-1, "op_convnext_block: parameter %d is null", i);
    hipStream_t st = (hipStream_t)stream;
    OpBufs b;
    OpLayout L;
    CK(op_layout(b, n_seq, seq_len, 0, L, st));
    const size_t n = (size_t)L.R * Td;
    const int pad = pad_nan ? 0xff : 0;
    float* te = op_filled<float>(b, n, pad, st);
    float* ty = op_filled<float>(b, 2 * n, pad, st);
    float* gx = op_filled<float>(b, (size_t)n_seq * 2 * Td, pad, st);
    Plane2 tn, tg;
    tn.hi = op_filled<__bf16>(b, n, pad, st); tn.lo = op_filled<__bf16>(b, n, pad, st);
    tg.hi = op_filled<__bf16>(b, 2 * n, pad, st); tg.lo = op_filled<__bf16>(b, 2 * n, pad, st);
    if (!te || !ty || !gx || !tn.hi || !tn.lo || !tg.hi || !tg.lo) return fail(-5, "op_convnext_block: hipMalloc");
    hipLaunchKernelGGL(op_scatter_rows_kernel, dim3(L.frames), dim3(256), 0, st, x_dev, Td, L.frames, L.frame_row, te, (__bf16*)nullptr,
                       (__bf16*)nullptr, Td);
    CKL("op scatter");
    const float* const* P = params_host;
    TextBlock tb;
    int rc = upload_f32(&tb.dw_w, P[0], (size_t)Td * 7) || upload_f32(&tb.dw_b, P[1], Td) || upload_f32(&tb.ln_w, P[2], Td) ||
             upload_f32(&tb.ln_b, P[3], Td) || upload_f32(&tb.gamma, P[6], 2 * Td) || upload_f32(&tb.beta, P[7], 2 * Td) ||
             pack_linear(tb.pw1, P[4], 2 * Td, Td, Td, P[5]) || pack_linear(tb.pw2, P[8], Td, 2 * Td, 2 * Td, P[9]) ? -4 : 0;
    if (!rc) rc = run_text_block(2, tb, Td, L.R, n_seq, te, tn, ty, tg, gx, L.row_start, L.row_end, L.row_seq, L.seq_row0, L.seq_len, nullptr,
                                 nullptr, 0, st);
    if (!rc) {
        hipLaunchKernelGGL(gather_rows_kernel, dim3(L.frames), dim3(128), 0, st, te, Td, Td, L.frames, L.frame_row, out_dev, Td);
        if (tap_ln_dev) hipLaunchKernelGGL(op_gather_planes_kernel, dim3(L.frames), dim3(256), 0, st, tn.hi, tn.lo, Td, Td, L.frames, L.frame_row, tap_ln_dev);
        if (tap_ty_dev) hipLaunchKernelGGL(gather_rows_kernel, dim3(L.frames), dim3(128), 0, st, ty, 2 * Td, 2 * Td, L.frames, L.frame_row, tap_ty_dev, 2 * Td);
        if (tap_grn_dev) hipLaunchKernelGGL(op_gather_planes_kernel, dim3(L.frames), dim3(256), 0, st, tg.hi, tg.lo, 2 * Td, 2 * Td, L.frames, L.frame_row,
                                            tap_grn_dev);
        if (tap_gx_dev) (void)hipMemcpyAsync(tap_gx_dev, gx, sizeof(float) * (size_t)n_seq * 2 * Td, hipMemcpyDeviceToDevice, st);
        if (hipGetLastError() != hipSuccess) rc = fail(-7, "op_convnext_block: gather launch");
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(-7, "op_convnext_block: %s", hipGetErrorString(hipGetLastError()));
    for (float* p : {tb.dw_w, tb.dw_b, tb.ln_w, tb.ln_b, tb.gamma, tb.beta}) dev_free(p);
    free_packed(tb.pw1); free_packed(tb.pw2);
    return rc;
}
extern "C" int f5hip_op_convnext_block(int32_t n_seq, const int32_t* seq_len, int32_t Td, const float* x_dev, const float* const* params_host,
                                       int32_t pad_nan, float* out_dev, float* tap_ln_dev, float* tap_ty_dev, float* tap_grn_dev, void* stream) {
    return op_convnext_block_run(n_seq, seq_len, Td, x_dev, params_host, pad_nan, out_dev, tap_ln_dev, tap_ty_dev, tap_grn_dev, nullptr, stream);
}
extern "C" int f5hip_op_convnext_block_gx(int32_t n_seq, const int32_t* seq_len, int32_t Td, const float* x_dev, const float* const* params_host,
                                          int32_t pad_nan, float* out_dev, float* tap_ln_dev, float* tap_ty_dev, float* tap_grn_dev,
                                          float* tap_gx_dev, void* stream) {
    return op_convnext_block_run(n_seq, seq_len, Td, x_dev, params_host, pad_nan, out_dev, tap_ln_dev, tap_ty_dev, tap_grn_dev, tap_gx_dev, stream);
}

// ---------------------------------------------------------------------------------------------------------------- ODE step and time-table unit ops
// What f5hip_op_cfg_step and f5hip_op_cfg_mixed share: checks every frame's rows and unit, stages urow_c | urow_u | frame_unit | the scalar
// strength spread over the frames (floats) [U each] | unit_op | unit_dt (floats) [n_units each] in one upload and xs_dev as the bf16 planes
// the kernel writes, launches cfg_step_kernel once (launch_cfg_step, the sampler's own launch) and reads the planes back as hi + lo.
// cb: the caller's state, slopes, pred and strengths (frame_cfg null: every frame takes `cfg`); its rows and planes are filled in here.
// frame_unit_host null: `op` and `dt` for every frame; else unit_op_host (null: `op` for every unit) and unit_dt_host [n_units].
static int op_cfg_launch(const char* name, CfgBufs cb, int U, int rows, const int32_t* urow_c_host, const int32_t* urow_u_host, float cfg, int op,
                         float dt, const int32_t* frame_unit_host, const int32_t* unit_op_host, const float* unit_dt_host, int n_units, int n_act,
                         float* xs_dev, hipStream_t st) {
    if (!frame_unit_host) n_units = 0;
    for (int u = 0; u < U; u++)
        if (urow_c_host[u] < 0 || urow_c_host[u] >= rows || urow_u_host[u] < -1 || urow_u_host[u] >= rows ||
            (frame_unit_host && (frame_unit_host[u] < 0 || frame_unit_host[u] >= n_units)))
            return fail(-1, "%s: frame %d: row or unit out of range", name, u);
    OpBufs b;
    const size_t n = (size_t)rows * 128, o_unit = 2 * (size_t)U, o_cfg = 3 * (size_t)U, o_op = 4 * (size_t)U, o_dt = o_op + n_units;
    cb.xs.hi = b.get<__bf16>(n); cb.xs.lo = b.get<__bf16>(n);
    int* meta = b.get<int>(o_dt + n_units);
    if (!cb.xs.hi || !cb.xs.lo || !meta) return fail(-5, "%s: hipMalloc", name);
    std::vector<int> hm(o_dt + n_units, 0);
    for (int u = 0; u < U; u++) {
        hm[u] = urow_c_host[u]; hm[U + u] = urow_u_host[u];
        if (frame_unit_host) hm[o_unit + u] = frame_unit_host[u];
        memcpy(&hm[o_cfg + u], &cfg, sizeof(float));
    }
    for (int k = 0; k < n_units; k++) hm[o_op + k] = unit_op_host ? unit_op_host[k] : op;
    if (n_units) memcpy(&hm[o_dt], unit_dt_host, sizeof(float) * n_units);
    if (upload_sync(st, meta, hm) != hipSuccess) return fail(-6, "%s: upload", name);
    hipLaunchKernelGGL(split_rows_kernel, dim3(rows), dim3(256), 0, st, (const float*)xs_dev, 128, 128, rows, (const int*)nullptr, cb.xs.hi, cb.xs.lo, 128, 0);
    CKL("op cfg split");
    cb.urow_c = meta; cb.urow_u = meta + U;
    if (!cb.frame_cfg) cb.frame_cfg = reinterpret_cast<const float*>(meta + o_cfg);
    launch_cfg_step(cb, U, op, dt, frame_unit_host ? meta + o_unit : nullptr, meta + o_op, reinterpret_cast<const float*>(meta + o_dt), n_act, st);
    CKL("op cfg step");
    hipLaunchKernelGGL(op_planes_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cb.xs.hi, cb.xs.lo, 0, n, xs_dev);
    CKL("op cfg planes");
    if (hipStreamSynchronize(st) != hipSuccess) return fail(-7, "%s: %s", name, hipGetErrorString(hipGetLastError()));
    return 0;
}

// One launch of the sampler's CFG combine + ODE update (cfg_step_kernel) on the caller's buffers, plus (final_flags_host not null)
// final_select_kernel.  U frames of `mel` channels; pred_dev and xs_dev fp32 [rows][128]; urow_c / urow_u host int32 [U] (urow_u -1: the
// frame has no unconditional row).  method 0: xout = xbase + dt v -- xout == xbase the Euler step in place (CFG_OP_EULER), else the midpoint
// rule's half step with xout as its scratch state, xbase untouched (CFG_OP_MID_HALF); 2: RK4 stage `stage` + 1 of 4 in place on xbase (xout
// must be xbase or null), k1 / k2 / k3 [U][mel]; -1: no step.
// The form: cfg_frame_dev null = scalar cfg, spread over the frames here; else per-frame strengths [U]; frame_unit_host + unit_dt_host
// [n_units] (with cfg_frame_dev) = the per-unit instance with the one op for every unit, frames of units >= n_act left alone.
// xs_dev is split into the bf16 planes the kernel writes, and read back as hi + lo.
// Final select: out_dev [U][mel] = final_flags_host[u] ? cond_dev : xbase (after the step).
extern "C" int f5hip_op_cfg_step(int32_t method, int32_t stage, int32_t U, int32_t mel, int32_t rows, float* xout_dev, float* xbase_dev,
                                 const float* pred_dev, const int32_t* urow_c_host, const int32_t* urow_u_host, float cfg, const float* cfg_frame_dev,
                                 float dt, const int32_t* frame_unit_host, const float* unit_dt_host, int32_t n_units, int32_t n_act, float* k1_dev,
                                 float* k2_dev, float* k3_dev, float* xs_dev, const uint8_t* final_flags_host, const float* cond_dev, float* out_dev,
                                 void* stream) {
    const bool step = method >= 0, rk4 = method == 2, unit_dt = frame_unit_host != nullptr;
    if (U <= 0 || mel <= 0 || mel > 128 || !xbase_dev || (method != -1 && method != 0 && method != 2))
        return fail(-1, "op_cfg_step: bad argument (method -1, 0 or 2; mel <= 128)");
    if (step && (rows <= 0 || !pred_dev || !urow_c_host || !urow_u_host || !xs_dev || (rk4 ? stage < 0 || stage > 3 || !k1_dev || !k2_dev || !k3_dev ||
                 (xout_dev && xout_dev != xbase_dev) : !xout_dev)))
        return fail(-1, "op_cfg_step: missing buffer of the step (rk4: stage 0..3, k1..k3, in place)");
    if (unit_dt && (!unit_dt_host || !cfg_frame_dev || n_units <= 0 || n_act < 0 || n_act > n_units))
        return fail(-1, "op_cfg_step: the per-unit form needs unit_dt, cfg_frame and 0 <= n_act <= n_units");
    if (final_flags_host && (!cond_dev || !out_dev)) return fail(-1, "op_cfg_step: the final select needs cond and out");
    hipStream_t st = (hipStream_t)stream;
    if (step) {
        const int op = rk4 ? CFG_OP_RK4_1 + stage : xout_dev == xbase_dev ? CFG_OP_EULER : CFG_OP_MID_HALF;
        const CfgBufs cb{xbase_dev, rk4 ? k1_dev : xout_dev, k2_dev, k3_dev, pred_dev, nullptr, nullptr, cfg_frame_dev, {}, mel};
        CK(op_cfg_launch("op_cfg_step", cb, U, rows, urow_c_host, urow_u_host, cfg, op, dt, frame_unit_host, nullptr, unit_dt_host, n_units, n_act, xs_dev, st));
    }
    if (final_flags_host) {
        OpBufs b;
        int* flags = b.get<int>(U);
        std::vector<int> hf(final_flags_host, final_flags_host + U);
        if (!flags || upload_sync(st, flags, hf) != hipSuccess) return fail(-6, "op_cfg_step: flag upload");
        hipLaunchKernelGGL(final_select_kernel, dim3(U), dim3(128), 0, st, (const float*)xbase_dev, cond_dev, (const int*)flags, mel, U, out_dev);
        CKL("op_cfg_step final_select");
        if (hipStreamSynchronize(st) != hipSuccess) return fail(-7, "op_cfg_step: %s", hipGetErrorString(hipGetLastError()));
    }
    return 0;
}

// One launch of the per-unit instance of cfg_step_kernel (what a sampler call with per-unit columns launches after every forward) on the
// caller's buffers: buffers as in f5hip_op_cfg_step; frame_unit_host [U], unit_op_host / unit_dt_host [n_units] the op code (CfgOp, 0..7) and
// step size of every unit for this forward; the frames of units >= n_act, or with op 0, are left as they are.  k1_dev is the midpoint rule's
// xmid too.
extern "C" int f5hip_op_cfg_mixed(int32_t U, int32_t mel, int32_t rows, float* xstate_dev, const float* pred_dev, const int32_t* urow_c_host,
                                  const int32_t* urow_u_host, const float* cfg_frame_dev, const int32_t* frame_unit_host, const int32_t* unit_op_host,
                                  const float* unit_dt_host, int32_t n_units, int32_t n_act, float* k1_dev, float* k2_dev, float* k3_dev, float* xs_dev,
                                  void* stream) {
    if (U <= 0 || mel <= 0 || mel > 128 || rows <= 0 || !xstate_dev || !pred_dev || !urow_c_host || !urow_u_host || !cfg_frame_dev || !frame_unit_host ||
        !unit_op_host || !unit_dt_host || !k1_dev || !k2_dev || !k3_dev || !xs_dev)
        return fail(-1, "op_cfg_mixed: bad argument (mel <= 128, every buffer)");
    if (n_units <= 0 || n_act < 0 || n_act > n_units) return fail(-1, "op_cfg_mixed: needs 0 <= n_act <= n_units");
    for (int k = 0; k < n_units; k++)
        if (unit_op_host[k] < CFG_OP_NONE || unit_op_host[k] >= CFG_OP_COUNT) return fail(-1, "op_cfg_mixed: unit_op[%d] = %d (0..7)", k, unit_op_host[k]);
    const CfgBufs cb{xstate_dev, k1_dev, k2_dev, k3_dev, pred_dev, nullptr, nullptr, cfg_frame_dev, {}, mel};
    return op_cfg_launch("op_cfg_mixed", cb, U, rows, urow_c_host, urow_u_host, 0.0f, CFG_OP_NONE, 0.0f, frame_unit_host, unit_op_host, unit_dt_host, n_units,
                         n_act, xs_dev, (hipStream_t)stream);
}

// row_tp_kernel of a mixed-grid call: row_tp_host[r] = unit_tp_host[row_unit_host[r]] for R rows of n_units units (all host int32)
extern "C" int f5hip_op_row_tp(int32_t R, const int32_t* row_unit_host, int32_t n_units, const int32_t* unit_tp_host, int32_t* row_tp_host, void* stream) {
    if (R <= 0 || n_units <= 0 || !row_unit_host || !unit_tp_host || !row_tp_host) return fail(-1, "op_row_tp: bad argument");
    for (int r = 0; r < R; r++)
        if (row_unit_host[r] < 0 || row_unit_host[r] >= n_units) return fail(-1, "op_row_tp: row_unit[%d] = %d out of range", r, row_unit_host[r]);
    hipStream_t st = (hipStream_t)stream;
    OpBufs b;
    int* d = b.get<int>((size_t)2 * R + n_units);   // row_unit | row_tp | unit_tp
    if (!d) return fail(-5, "op_row_tp: hipMalloc");
    std::vector<int> h((size_t)2 * R + n_units, -1);
    std::copy(row_unit_host, row_unit_host + R, h.begin());
    std::copy(unit_tp_host, unit_tp_host + n_units, h.begin() + 2 * (size_t)R);
    if (upload_sync(st, d, h) != hipSuccess) return fail(-6, "op_row_tp: upload");
    hipLaunchKernelGGL(row_tp_kernel, dim3((R + 255) / 256), dim3(256), 0, st, (const int*)d, (const int*)(d + 2 * (size_t)R), R, d + R);
    CKL("op_row_tp");
    if (hipMemcpyAsync(row_tp_host, d + R, sizeof(int) * R, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(-7, "op_row_tp: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

// precompute_time of a finalized handle over n_t time points (t_host), and what it left in the handle's tables: sinus_dev fp32 [n_t][256] the
// sinusoid table as uploaded (hi + lo), mod_dev fp32 [n_t][mod_cols] the AdaLN modulation rows (mod_cols must be the handle's row width; DiT
// and MMDiT) or null, temb_dev fp32 [n_t][dim] the time embeddings (UNetT) or null
extern "C" int f5hip_op_time_table(f5hip_dit* m, const float* t_host, int32_t n_t, float* sinus_dev, float* mod_dev, int32_t mod_cols,
                                   float* temb_dev, void* stream) {
    if (!m || !m->finalized) return fail(-1, "model not finalized");
    if (!t_host || n_t <= 0 || !sinus_dev) return fail(-1, "op_time_table: bad argument");
    if (mod_dev && (m->arch == 1 || mod_cols != m->n_adaln)) return fail(-1, "op_time_table: mod has %d columns in this model (got %d)", m->n_adaln, mod_cols);
    if (temb_dev && m->arch != 1) return fail(-1, "op_time_table: only UNetT keeps the time embeddings");
    hipStream_t st = (hipStream_t)stream;
    CK(ensure_workspace(m, 128, 1, 1));
    CK(precompute_time(m, t_host, n_t, st));
    const size_t ns = (size_t)n_t * 256;
    hipLaunchKernelGGL(op_planes_to_f32_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, m->sinp.hi, m->sinp.lo, 0, ns, sinus_dev);
    CKL("op_time_table planes");
    if (mod_dev && hipMemcpyAsync(mod_dev, m->mod, sizeof(float) * (size_t)n_t * m->n_adaln, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return fail(-6, "op_time_table: mod copy");
    if (temb_dev && hipMemcpyAsync(temb_dev, m->temb, sizeof(float) * (size_t)n_t * m->cfg.dim, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return fail(-6, "op_time_table: temb copy");
    if (hipStreamSynchronize(st) != hipSuccess) return fail(-7, "op_time_table: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}
