// HBM/L2-bound row kernels of the DiT / Vocos paths: LayerNorm (+AdaLN modulation, + optional depthwise
// conv k=7 in front), GRN, embedding gather, CFG + ODE update, packing helpers.  One wave (64 lanes) per
// row, float4 loads, wave-shuffle reductions, fp32 statistics, split-bf16 outputs that feed the MFMA GEMMs.
#pragma once
#include "common.h"

#include "ln_row.h"

// Row -> workgroup mapping, XCD-matched (speed only, any bijection is correct): consecutive workgroup ids go round-robin to the 8 XCDs
// and the block GEMMs give XCD x the row slabs of rows [x M / 8, (x + 1) M / 8) (gemm5_tile_of_block) -- both the GEMM that just wrote the
// residual rows this kernel reads and the GEMM that reads the operand rows it writes.  With the same blocking here a row stays in one XCD's L2
// from the residual epilogue through the norm to the next GEMM's first fill instead of crossing the fabric twice.
// ROW_MOD: every row takes its scale / shift from its own modulation row (LnArgs::row_mod; f5hip_cfm_sample_grids)
template <int NV, bool ROW_MOD = false>
__global__ __launch_bounds__(256) void ln_kernel(const LnArgs p) {
    unsigned b = blockIdx.x;
    if ((gridDim.x & 7) == 0) b = (b & 7) * (gridDim.x >> 3) + (b >> 3);
    ln_row<NV, ROW_MOD>(p, b * 4 + (threadIdx.x >> 6), threadIdx.x & 63);
}

// f5hip_cfm_sample_grids: the time point of every row for one forward, row_tp[r] = unit_tp[row_unit[r]] (the row's unit, padding rows included)
__global__ __launch_bounds__(256) void row_tp_kernel(const int* row_unit, const int* unit_tp, int R, int* row_tp) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < R) row_tp[r] = unit_tp[row_unit[r]];
}

// Rotary factors per ROW: out_cos / out_sin [R][32] = table[row_pos[r]][32].  Once per sampler call (the positions do not change over the ODE steps):
// the QKV epilogues then fetch a row's factors with one load instead of two dependent ones (row_pos, then the table) -- the 32 rotary tiles of the C2
// launch finished 2.7 us behind the other 224.
__global__ __launch_bounds__(256) void rope_rows_kernel(const int* row_pos, const float* rope_cos, const float* rope_sin, int R, int max_pos, float* out_cos, float* out_sin) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R * 32) return;
    const int r = i >> 5, j = i & 31;
    const int pos = min(max(row_pos[r], 0), max_pos - 1);
    out_cos[i] = rope_cos[pos * 32 + j];
    out_sin[i] = rope_sin[pos * 32 + j];
}

// ------------------------------------------------------------------------------------------------
// GRN (F/model/modules.py:231-234): Gx[c] = ||y[:, c]||_2 over the frames of one sequence.
// The sum of squares of a column is kept as eight partial sums a8[u]: rows r < (n & ~7) with r % 8 == u in ascending order, then the tail rows
// n & ~7 .. n - 1 into a8[0]; combined by one fixed tree.  One thread per column walking all rows (8 loads in flight) put a 1404-row sequence
// of 1024 columns on 4 workgroups for 61 us of load latency.  Here a workgroup is 32 columns x the eight partial sums, one lane each (32 x
// n_seq workgroups at C = 1024), every lane with 8 loads of its own row class in flight: the same addends in the same order per partial sum.
// Explicit fma: the one-thread-per-column form compiled `a += t * t` to fused multiply-adds, and left to the compiler this form does not
// (it squares two values at a time and adds the rounded products).
__global__ __launch_bounds__(256) void grn_stats_kernel(const float* y, int ldy, int C, const int* seq_row0,
                                                        const int* seq_len, float* gx /*[n_seq][C]*/) {
    __shared__ float part[8][32];
    const int seq = blockIdx.y, cl = threadIdx.x & 31, u = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    const int r0 = seq_row0[seq], n = seq_len[seq], n8 = n & ~7;
    float a = 0.f;
    if (c < C) {
        const float* col = y + (size_t)r0 * ldy + c;
        int r = u;
        for (; r + 56 < n8; r += 64) {
            float t[8];
#pragma unroll
            for (int i = 0; i < 8; i++) t[i] = col[(size_t)(r + 8 * i) * ldy];
#pragma unroll
            for (int i = 0; i < 8; i++) a = __builtin_fmaf(t[i], t[i], a);
        }
        for (; r < n8; r += 8) {
            const float t = col[(size_t)r * ldy];
            a = __builtin_fmaf(t, t, a);
        }
        if (u == 0)
            for (r = n8; r < n; r++) {
                const float t = col[(size_t)r * ldy];
                a = __builtin_fmaf(t, t, a);
            }
    }
    part[u][cl] = a;
    __syncthreads();
    if (u == 0 && c < C) {
        const float acc = ((part[0][cl] + part[1][cl]) + (part[2][cl] + part[3][cl])) + ((part[4][cl] + part[5][cl]) + (part[6][cl] + part[7][cl]));
        gx[(size_t)seq * C + c] = sqrtf(acc);
    }
}

// y' = gamma * (y * Nx) + beta + y,  Nx = Gx / (mean_c(Gx) + 1e-6)  -> split bf16
__global__ __launch_bounds__(256) void grn_apply_kernel(const float* y, int ldy, int C, int M, const int* row_seq,
                                                        const float* gx, const float* gamma, const float* beta,
                                                        __bf16* out_hi, __bf16* out_lo, int ldo) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int seq = row_seq[row];
    if (seq < 0) return;
    const float* g = gx + (size_t)seq * C;
    float s = 0.0f;
    for (int c = lane; c < C; c += 64) s += g[c];
    const float denom = wave_sum(s) / (float)C + 1e-6f;
    for (int c = lane * 4; c < C; c += 256) {
        const float4 yv = *reinterpret_cast<const float4*>(y + (size_t)row * ldy + c);
        const float yy[4] = {yv.x, yv.y, yv.z, yv.w};
        bf16x4 hi, lo;
        float ov[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float nx = g[c + e] / denom;
            ov[e] = gamma[c + e] * (yy[e] * nx) + beta[c + e] + yy[e];
        }
        split_bf16x4(ov, hi, lo);
        *reinterpret_cast<bf16x4*>(out_hi + (size_t)row * ldo + c) = hi;
        if (out_lo) *reinterpret_cast<bf16x4*>(out_lo + (size_t)row * ldo + c) = lo;
    }
}

// ------------------------------------------------------------------------------------------------
// Text embedding gather (F/model/backbones/dit.py:48-64): e[m] = Embedding[id[m]] + pos_table[min(pos, 4095)]
__global__ __launch_bounds__(256) void text_gather_kernel(const float* emb, const float* pos_table, int C, int M,
                                                          const int* row_token, const int* row_pos, int add_pos,
                                                          float* out, int ldo, int max_pos) {
    const int row = blockIdx.x;
    if (row >= M) return;
    const int tok = row_token[row];
    if (tok < 0) return;   // padding row of the packed layout
    const int pos = min(row_pos[row], max_pos);   // get_pos_embed_indices clamps below the table length: 4096 (DiT), 1024 (MMDiT)
    for (int c = threadIdx.x; c < C; c += 256) {
        float v = emb[(size_t)tok * C + c];
        if (add_pos) v += pos_table[(size_t)pos * C + c];
        out[(size_t)row * ldo + c] = v;
    }
}

// fp32 [rows][C] -> split bf16 [rows][ldo] (columns >= C are left untouched: buffers are zero-initialised)
__global__ __launch_bounds__(256) void split_rows_kernel(const float* x, int ldx, int C, int M, const int* row_src,
                                                         __bf16* out_hi, __bf16* out_lo, int ldo, int col0) {
    const int row = blockIdx.x;
    if (row >= M) return;
    const int src = row_src ? row_src[row] : row;
    for (int c = threadIdx.x; c < C; c += 256) {
        __bf16 hi, lo;
        const float v = src >= 0 ? x[(size_t)src * ldx + c] : 0.0f;
        split_bf16(v, hi, lo);
        out_hi[(size_t)row * ldo + col0 + c] = hi;
        if (out_lo) out_lo[(size_t)row * ldo + col0 + c] = lo;
    }
}

// ------------------------------------------------------------------------------------------------
// CFG combine + ODE update (F/model/cfm.py:176 and torchdiffeq's fixed-grid solvers): v = p + (p - p0) * cfg, then one op of a solver (CfgOp).
// pred: [M_pad][ldp] rows of the conditional branch at urow_c[u], unconditional at urow_u[u] (or -1).
// Every op also refreshes the split-bf16 copy of x that feeds the next forward's input projection, for both branches.
// What cfg_step_kernel does to a frame after one forward
enum CfgOp : int {
    CFG_OP_NONE = 0,       // the unit's steps are done: its frames are left as they are
    CFG_OP_EULER = 1,      // x += dt v
    CFG_OP_MID_HALF = 2,   // midpoint, first forward: k1 = x + dt v (dt is half the step), x untouched
    CFG_OP_MID_FULL = 3,   // midpoint, second forward: x += dt v
    CFG_OP_RK4_1 = 4,      // RK4 stage 1 .. 4: CFG_OP_RK4_1 + stage - 1
    CFG_OP_COUNT = 8
};

// The arithmetic of cfg_step_kernel, one helper per piece.
// v = p_c + (p_c - p_u) * cfg for channel c of a frame (v = p_c without an unconditional row)
__device__ __forceinline__ float cfg_velocity(const float* pred, int ldp, int rc, int ru, int c, float cfg) {
    const float pc = pred[(size_t)rc * ldp + c];
    float v = pc;
    if (ru >= 0) v = pc + (pc - pred[(size_t)ru * ldp + c]) * cfg;
    return v;
}

// xout[i] = xbase[i] + dt * v: the Euler step (xout == xbase), the midpoint rule's half step (xout a scratch state) and its full step
__device__ __forceinline__ float euler_update(float* xout, const float* xbase, size_t i, float dt, float v) {
    const float xn = xbase[i] + dt * v;
    xout[i] = xn;
    return xn;
}

// Stage `stage` (1..4) of the fixed-grid RK4 step on element i (torchdiffeq method="rk4": rk4_alt_step_func, the 3/8 rule), after the forward
// of that stage of the interval [t0, t0 + dt]:
//   1: k1 = v(t0, y0)             next input y0 + dt * k1 / 3
//   2: k2 = v(t0 + dt/3, ..)      next input y0 + dt * (k2 - k1 / 3)
//   3: k3 = v(t0 + 2 dt/3, ..)    next input y0 + dt * (k1 - k2 + k3)
//   4: k4 = v(t0 + dt, ..)        y1 = y0 + (k1 + 3 (k2 + k3) + k4) * dt / 8
// Stages 1-3 keep k_s in their [U][mel] buffer and return the next stage's input, which goes only to the split-bf16 copy of x; xstate holds
// y0 until stage 4 writes y1 there.
__device__ __forceinline__ float rk4_stage_update(float* xstate, float* k1, float* k2, float* k3, size_t i, int stage, float dt, float v) {
    const float y0 = xstate[i];
    float xn;
    if (stage == 1) {
        k1[i] = v;
        xn = y0 + dt * v * (1.0f / 3.0f);
    } else if (stage == 2) {
        k2[i] = v;
        xn = y0 + dt * (v - k1[i] * (1.0f / 3.0f));
    } else if (stage == 3) {
        k3[i] = v;
        xn = y0 + dt * (k1[i] - k2[i] + v);
    } else {
        xn = y0 + (k1[i] + 3.0f * (k2[i] + k3[i]) + v) * dt * 0.125f;
        xstate[i] = xn;
    }
    return xn;
}

// split(xn) into channel c of both rows of the frame in the split-bf16 copy of x
__device__ __forceinline__ void store_x_split(__bf16* xs_hi, __bf16* xs_lo, int ldx, int rc, int ru, int c, float xn) {
    __bf16 hi, lo;
    split_bf16(xn, hi, lo);
    xs_hi[(size_t)rc * ldx + c] = hi;
    xs_lo[(size_t)rc * ldx + c] = lo;
    if (ru >= 0) {
        xs_hi[(size_t)ru * ldx + c] = hi;
        xs_lo[(size_t)ru * ldx + c] = lo;
    }
}

// The one update kernel of the sampler, launched once after every forward: one block per frame, the frame's strength from cfg_frame[u].
// kPerUnit = false: every frame takes the op `op` (CfgOp) with step size `dt`.  kPerUnit = true: frame u takes unit_op[frame_unit[u]] and
// unit_dt[frame_unit[u]], this forward's op and step size of its unit by layout position; the frames of units >= n_act, or with
// CFG_OP_NONE, are left as they are.  The op is uniform over a block, so no wave diverges.  k1 is the midpoint rule's scratch state as well
// as RK4's first slope, indexed by frame like k2 / k3: the frames of different units are disjoint, so units of different methods share them.
template <bool kPerUnit>
__global__ __launch_bounds__(128) void cfg_step_kernel(float* xstate /*[U][mel]*/, int mel, int U, const float* pred, int ldp, const int* urow_c,
                                                       const int* urow_u, const float* cfg_frame, int op, float dt, float* k1, float* k2, float* k3,
                                                       __bf16* xs_hi, __bf16* xs_lo, int ldx, const int* frame_unit, const int* unit_op,
                                                       const float* unit_dt, int n_act) {
    const int u = blockIdx.x;
    if (u >= U) return;
    const int c = threadIdx.x;
    if (c >= mel) return;
    if (kPerUnit) {
        const int un = frame_unit[u];
        if (un >= n_act) return;
        op = unit_op[un];
        dt = unit_dt[un];
    }
    if (op <= CFG_OP_NONE || op >= CFG_OP_COUNT) return;
    const int rc = urow_c[u], ru = urow_u[u];
    const float v = cfg_velocity(pred, ldp, rc, ru, c, cfg_frame[u]);
    const size_t i = (size_t)u * mel + c;
    float xn;
    if (op >= CFG_OP_RK4_1) xn = rk4_stage_update(xstate, k1, k2, k3, i, op - CFG_OP_RK4_1 + 1, dt, v);
    else xn = euler_update(op == CFG_OP_MID_HALF ? k1 : xstate, xstate, i, dt, v);
    store_x_split(xs_hi, xs_lo, ldx, rc, ru, c, xn);
}

// out = cond_mask ? cond : x  (F/model/cfm.py:204); one block per utterance frame
__global__ __launch_bounds__(128) void final_select_kernel(const float* xstate, const float* cond, const int* frame_is_cond,
                                                           int mel, int U, float* out) {
    const int u = blockIdx.x, c = threadIdx.x;
    if (u >= U || c >= mel) return;
    out[(size_t)u * mel + c] = frame_is_cond[u] ? cond[(size_t)u * mel + c] : xstate[(size_t)u * mel + c];
}

// fp32 [R][C] (row-major, ld = C) -> split bf16 [R_pad][C_pad] with zero fill; used by the weight packer
// (lo == nullptr: ONE fp16 plane in hi, the weight format of the PREC_F16 GEMMs)
__global__ __launch_bounds__(256) void pack_weight_kernel(const float* w, int R, int C, int ldw, __bf16* hi, __bf16* lo,
                                                          int C_pad) {
    const int r = blockIdx.x;
    for (int c = threadIdx.x; c < C_pad; c += 256) {
        float v = (r < R && c < C) ? w[(size_t)r * ldw + c] : 0.0f;
        if (!lo) {
            reinterpret_cast<_Float16*>(hi)[(size_t)r * C_pad + c] = sat_f16(v);
            continue;
        }
        __bf16 h, l;
        split_bf16(v, h, l);
        hi[(size_t)r * C_pad + c] = h;
        lo[(size_t)r * C_pad + c] = l;
    }
}

// one 16-bit plane [R_pad][ld] (row-major, K = C_pad contiguous) -> MFMA-fragment order (GemmArgs::Wf): thread = one 16-byte chunk
__global__ __launch_bounds__(256) void pack_frag_kernel(const __bf16* src, int R_pad, int K, int ld, __bf16* dst) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;          // chunk index in the destination
    const size_t n_chunks = (size_t)R_pad * K / 8;
    if (idx >= n_chunks) return;
    const int lane = (int)(idx & 63);
    const size_t blk = idx >> 6;
    const int kh = (int)(blk % (size_t)(K / 32)), cb = (int)(blk / (size_t)(K / 32));
    const int row = cb * 16 + (lane & 15), k = kh * 32 + (lane >> 4) * 8;
    *reinterpret_cast<u32x4*>(dst + idx * 8) = *reinterpret_cast<const u32x4*>(src + (size_t)row * ld + k);
}

// dst[f][0..C) = src[frame_row[f]][0..C): packed-row layout -> caller's frame order
__global__ __launch_bounds__(128) void gather_rows_kernel(const float* src, int lds, int C, int n_frames, const int* frame_row,
                                                          float* dst, int ldd) {
    const int f = blockIdx.x;
    if (f >= n_frames) return;
    const int r = frame_row[f];
    for (int c = threadIdx.x; c < C; c += 128) dst[(size_t)f * ldd + c] = src[(size_t)r * lds + c];
}

// UNetT: the time embedding is the first token of every sequence (F/model/backbones/unett.py:184)
__global__ __launch_bounds__(256) void set_time_token_kernel(float* h, int D, const int* seq_row0, const float* temb) {
    float* row = h + (size_t)seq_row0[blockIdx.x] * D;
    for (int c = threadIdx.x; c < D; c += 256) row[c] = temb[c];
}

// f5hip_cfm_sample_grids: the time token of every sequence from its own time point (row_tp of its first row): temb[row_tp[row0]]
__global__ __launch_bounds__(256) void set_time_token_rows_kernel(float* h, int D, const int* seq_row0, const float* temb, const int* row_tp) {
    const int r0 = seq_row0[blockIdx.x];
    float* row = h + (size_t)r0 * D;
    const float* src = temb + (size_t)row_tp[r0] * D;
    for (int c = threadIdx.x; c < D; c += 256) row[c] = src[c];
}
