// gemm8: MXFP8 block GEMM for gfx950 -- the transformer-block projections of gemm_planes == 4 on v_mfma_scale_f32_16x16x128_f8f6f4.
//   C[M,N] = A[M,K] * W[N,K]^T with both operands in MXFP8, fp32 accumulate, the generic epilogues of gemm5.h (GemmArgs of gemm_epilogue.h).
//
// MXFP8 (OCP Microscaling v1.0), the one definition both quantisers below implement and tests/mxfp8_ref.py restates:
//   * a block is 32 consecutive elements ALONG K of one row; it shares one E8M0 scale 2^e and holds 32 E4M3 ("fn": finite only, max 448) codes;
//   * amax = largest magnitude of the block.  amax > 0: e = clamp(floor(log2(amax)) - 8, -127, 127); a block of zeros: e = -127;
//   * element = v * 2^-e (exact), rounded to nearest-even into E4M3 (subnormals down to 2^-9 included), saturating at +-448;
//   * a NaN or an infinity anywhere in the block: every element of the block is the E4M3 NaN (0x7f) under the scale 2^0, so every product
//     with the block, and with it the whole output row, is NaN (A side: enforced in the kernel, the MFMA itself reads 0x7f as finite;
//     W side: weights are taken to be finite).
// Nothing in it depends on the tile, the batch or the call: a row's quantised operand is a function of that row alone.
//
// Operand layout of the instruction (measured on an MI355X with exact-arithmetic probes): of the 128 k of a step, lane
// (row & 15) + 16 g holds k = 16 g .. 16 g + 15 in its first four operand registers and k = 64 + 16 g .. + 15 in the last four, and the scale of
// block b (k = 32 b .. 32 b + 31) is read from lane (row & 15) + 16 b.  A scale block is therefore two lanes' halves: lanes g = 2 (b & 1) and
// 2 (b & 1) + 1, register half b >> 1.
//
// Data movement.  W is quantised once (quant_w8_kernel) and stored in that order: per (16 output columns, 128-deep k-step) one 2 KiB
// fragment block = 2 register halves x 64 lanes x 16 bytes, so a lane's operand is two ds_read_b128 at lane * 16, and its scale register is
// the lane's own byte of the scale plane, which keeps four consecutive k-steps in one dword per (16 columns, lane):
// [n_pad / 16][ceil(K / 512)][64].
// A stays the fp16 plane its producers write.  A tile is 64 rows x (128 or 256) columns, 512 threads:
//   * waves 4-7 (loaders) stream k-steps into a 3-deep LDS ring by LDS-DMA (16 bytes per lane): 16 KiB of fp16 A rows (256 bytes per row, the
//     16-byte chunk XOR-swizzled with row & 15 on the SOURCE side, so the 16 rows a quarter-wave reads at once cover all banks) and the W
//     fragment blocks as they lie in memory (1 KiB pieces, eight full cache lines each);
//   * waves 0-3 (consumers, one per SIMD) own 16 rows x all columns of the tile.  A lane (row = lane & 15, g = lane >> 4) reads the two
//     16-element halves of its row it feeds to the MFMA and quantises them in registers: the amax of each half meets the other half's in
//     lane g ^ 1 (one cross-lane exchange per half), exponent and the packed v_cvt_pk_fp8_f32 conversions are lane-local, and one more
//     exchange puts block g's scale byte into lane g.  No 8-bit tile is written back to LDS: the result IS the MFMA's token-side operand.
//     One conversion serves the 8 / 16 MFMAs of the tile's column blocks, each of which reads its W fragment from LDS right before it is
//     issued.  K = 1024 is 8 k-steps: the fill and the conversion are the loop.
// K order: k-steps in ascending order into one accumulator per (row block, column block); inside a step the instruction's own order.  Neither
// depends on M or the grid.
// The W fragment is the MFMA's A operand (gemm5.h's SWAP layout: a lane holds 4 consecutive features of one token), so the accumulators go to
// the fp32 slab with g5_write_slab and the row phase is gemm5.h's G5GenericTail, chosen through the shared variant table (epi_dispatch).
#pragma once
#include "gemm5.h"

typedef __attribute__((ext_vector_type(8))) int i32x8;

// The definition above in three steps, shared by both quantisers.  Magnitudes are compared as bits: they order like unsigned integers, and a
// NaN or an infinity is the largest of all.
template <int N>
F5_DEVICE unsigned mx8_amax_bits(const float (&v)[N]) {
    unsigned amax = 0;
#pragma unroll
    for (int i = 0; i < N; i++) amax = max(amax, __float_as_uint(v[i]) & 0x7fffffffu);
    return amax;
}
// E8M0 byte e + 127 of a block whose largest magnitude has the bits amax: floor(log2(amax)) = exponent field - 127 (a subnormal or zero amax
// clamps to e = -127 either way), so e + 127 = field - 8; a non-finite block: 127 (2^0)
F5_DEVICE unsigned mx8_scale_byte(unsigned amax) {
    const unsigned field = amax >> 23;
    return amax >= 0x7f800000u ? 127u : (field > 8u ? field - 8u : 0u);
}
// 16 elements of a block with the bits amax and the scale byte sb -> 16 E4M3 codes, k ascending from byte 0 of q[0].
// Measured on an MI355X: the MFMA loses what lies ~15 bits below the largest product of a 128-deep step (a block [256, 3 2^-9] against ones
// gives 256, whichever side holds it), so E4M3 subnormals next to a full-scale element do not reach the sum.
F5_DEVICE void mx8_encode16(const float (&v)[16], unsigned amax, unsigned sb, unsigned (&q)[4]) {
    const float inv = __uint_as_float((254u - sb) << 23);   // 2^-e
#pragma unroll
    for (int d = 0; d < 4; d++) {
        float s[4];
#pragma unroll
        for (int e = 0; e < 4; e++) s[e] = __builtin_amdgcn_fmed3f(v[4 * d + e] * inv, -448.0f, 448.0f);
        const unsigned w = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(s[2], s[3], __builtin_amdgcn_cvt_pk_fp8_f32(s[0], s[1], 0, false), true);
        q[d] = amax >= 0x7f800000u ? 0x7f7f7f7fu : w;
    }
}

// Weight quantiser: w fp32 [N][K] (row stride ldw) -> the fragment-ordered E4M3 plane w8 [n_pad / 16][K / 128][2][64][16] and the scale plane
// s8 (zeroed by the caller) [n_pad / 16][ceil(K / 512)][64] dwords.  One thread per (row, scale block); rows past N are zeros.
__global__ __launch_bounds__(256) void quant_w8_kernel(const float* __restrict__ w, int N, int n_pad, int K, int ldw, unsigned char* __restrict__ w8,
                                                       unsigned char* __restrict__ s8) {
    const int nkb = K >> 5, nk = K >> 7, nk4 = (nk + 3) >> 2;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n_pad * nkb) return;
    const int n = (int)(idx / nkb), kb = (int)(idx % nkb);
    float v[2][16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const f32x4 x = n < N ? *reinterpret_cast<const f32x4*>(w + (size_t)n * ldw + kb * 32 + i * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; e++) v[i >> 2][(i & 3) * 4 + e] = x[e];
    }
    const unsigned amax = max(mx8_amax_bits(v[0]), mx8_amax_bits(v[1])), sb = mx8_scale_byte(amax);
    const int cbk = n >> 4, t = kb >> 2, b = kb & 3, r = n & 15;
    // block b of the step: register half b >> 1 of lanes g = 2 (b & 1) (its first 16 k) and g + 1 (its last 16)
    unsigned char* dst = w8 + ((size_t)(cbk * nk + t) * 2 + (b >> 1)) * 1024 + (r + 32 * (b & 1)) * 16;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        unsigned q[4];
        mx8_encode16(v[h], amax, sb, q);
        *reinterpret_cast<u32x4*>(dst + h * 256) = (u32x4){q[0], q[1], q[2], q[3]};
    }
    s8[((size_t)(cbk * nk4 + (t >> 2)) * 64 + r + 16 * b) * 4 + (t & 3)] = (unsigned char)sb;
}

template <int CB>
struct Gemm8Cfg {
    static constexpr int RB = 4, BM = 64, BN = CB * 16, NST = 3;
    static constexpr int A_BYTES = BM * 256;                 // 64 rows x 128 fp16
    static constexpr int STAGE = A_BYTES + CB * 2048;        // + CB fragment blocks of 16 columns x 128 codes
    static constexpr int PIECES = STAGE / 1024, PPW = PIECES / 4;   // 1 KiB LDS-DMA pieces per k-step, per loader wave
    static constexpr int A_PPW = A_BYTES / 4096;             // the first A_PPW pieces of a loader wave are A rows
    using Slab = Gemm5Cfg<RB, CB, NST>;
    static constexpr int LDS = NST * STAGE > Slab::SLAB ? NST * STAGE : Slab::SLAB;
    static_assert(PIECES % 4 == 0 && 2 * PPW <= 63 && LDS <= 160 * 1024, "bad gemm8 tile");
};

template <int EPI, int CB>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm8_kernel(const GemmArgs p, const unsigned char* __restrict__ w8,
                                                                                               const unsigned int* __restrict__ s8, const int tiles_n) {
    using C = Gemm8Cfg<CB>;
    constexpr int NST = C::NST, STAGE = C::STAGE, PPW = C::PPW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = gemm5_tile_of_block(blockIdx.x, gridDim.x);
    const int m0 = (tile / tiles_n) * C::BM, n0 = (tile % tiles_n) * C::BN;
    const int nk = p.K >> 7, nk4 = (nk + 3) >> 2;
    f32x4 acc[1][CB];

    // Ring protocol.  All NST stages are filled up front.  Barrier B_kt opens k-step kt: behind it "k-step kt has landed" (every loader wave
    // waited for its own pieces) and "every read of k-step kt - 1 has returned" (the consumers waited lgkmcnt(0)), so the loaders issue
    // k-step kt - 1 + NST into that stage at once.  Both groups execute nk barriers.
    if (wave >= 4) {
        const int pw = wave - 4;
        const char* gsrc[PPW];
#pragma unroll
        for (int j = 0; j < PPW; j++) {
            const int pc = pw + 4 * j;
            if (j < C::A_PPW) {   // 4 rows x 256 bytes; the lane fetches the logical chunk that belongs in its physical slot
                const int row = pc * 4 + (lane >> 4), chunk = (lane & 15) ^ (row & 15);
                // rows past M re-read the last valid row: never stored
                gsrc[j] = reinterpret_cast<const char*>(p.A[0] + (size_t)min(m0 + row, p.M - 1) * p.lda) + chunk * 16;
            } else {              // half a fragment block, as it lies in memory
                const int blk = (pc - C::A_BYTES / 1024) >> 1, half = (pc - C::A_BYTES / 1024) & 1;
                gsrc[j] = reinterpret_cast<const char*>(w8) + ((size_t)(n0 / 16 + blk) * nk * 2 + half) * 1024 + lane * 16;
            }
        }
        auto issue_step = [&](int kt) {
            char* dst = smem + (kt % NST) * STAGE + pw * 1024;
#pragma unroll
            for (int j = 0; j < PPW; j++)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc[j] + (size_t)kt * (j < C::A_PPW ? 256 : 2048)),
                                                 (__attribute__((address_space(3))) void*)(dst + j * 4096), 16, 0, 0);
        };
        auto wait_landed = [&](int newer) {   // at most `newer` younger k-steps of this wave still in flight
            if (newer >= 2) wait_vmcnt<2 * PPW>(); else if (newer == 1) wait_vmcnt<PPW>(); else wait_vmcnt<0>();
        };
#pragma unroll
        for (int t = 0; t < NST; t++)
            if (t < nk) issue_step(t);
        for (int kt = 0; kt < nk; kt++) {
            wait_landed(kt == 0 ? min(NST - 1, nk - 1) : min(NST - 2, nk - 1 - kt));
            __builtin_amdgcn_s_barrier();                          // B_kt
            if (kt >= 1 && kt - 1 + NST < nk) issue_step(kt - 1 + NST);
        }
    } else {
        const int r = lane & 15, g = lane >> 4;
#pragma unroll
        for (int j = 0; j < CB; j++) acc[0][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const unsigned int* sp = s8 + (size_t)(n0 / 16) * nk4 * 64 + lane;   // + (j nk4 + kt / 4) 64
        unsigned sw[CB];
        unsigned worst = 0;   // largest magnitude bits this lane met: a non-finite A element makes its whole output row NaN below
        for (int kt = 0; kt < nk; kt++) {
            if ((kt & 3) == 0) {
#pragma unroll
                for (int j = 0; j < CB; j++) sw[j] = sp[(size_t)(j * nk4 + (kt >> 2)) * 64];
            }
            __builtin_amdgcn_s_barrier();                          // B_kt
            const char* st = smem + (kt % NST) * STAGE;
            const char* arow = st + (wave * 16 + r) * 256;
            // register half h: k = 64 h + 16 g .. + 15 of the step = chunks 8 h + 2 g, + 1 of the row; it is half of scale block 2 h + (g >> 1)
            unsigned a8[2][4], amax[2], sb[2];
            float v[2][16];
#pragma unroll
            for (int h = 0; h < 2; h++) {
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const f16x8 x = *reinterpret_cast<const f16x8*>(arow + (((8 * h + 2 * g + q) ^ r) << 4));
#pragma unroll
                    for (int e = 0; e < 8; e++) v[h][q * 8 + e] = (float)x[e];
                }
                amax[h] = mx8_amax_bits(v[h]);
                amax[h] = max(amax[h], (unsigned)__shfl_xor((int)amax[h], 16, 64));   // the block's other half: lane g ^ 1
                worst = max(worst, amax[h]);
                sb[h] = mx8_scale_byte(amax[h]);
                mx8_encode16(v[h], amax[h], sb[h], a8[h]);
            }
            // lane g supplies the scale of block g: register half g >> 1 of lanes 2 (g & 1) and + 1
            const int sa = (__shfl((int)(sb[0] | (sb[1] << 8)), r + 32 * (g & 1), 64) >> (8 * (g >> 1))) & 0xff;
            const i32x8 a8v = {(int)a8[0][0], (int)a8[0][1], (int)a8[0][2], (int)a8[0][3], (int)a8[1][0], (int)a8[1][1], (int)a8[1][2], (int)a8[1][3]};
            const char* wf = st + C::A_BYTES + lane * 16;
            const int sh = (kt & 3) * 8;
#pragma unroll
            for (int j = 0; j < CB; j++) {
                const u32x4 lo = *reinterpret_cast<const u32x4*>(wf + j * 2048), hi = *reinterpret_cast<const u32x4*>(wf + j * 2048 + 1024);
                const i32x8 w = {(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
                acc[0][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, a8v, acc[0][j], 0, 0, 0, (int)(sw[j] >> sh), 0, sa);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // every LDS read of this stage has returned before B_{kt+1}
        }
        // The MFMA reads the E4M3 NaN code as a finite value (measured), so the row is poisoned here: the four lanes of a row (g = 0 .. 3)
        // hold all of its accumulators
        worst = max(worst, (unsigned)__shfl_xor((int)worst, 16, 64));
        worst = max(worst, (unsigned)__shfl_xor((int)worst, 32, 64));
        if (worst >= 0x7f800000u) {
#pragma unroll
            for (int j = 0; j < CB; j++) acc[0][j] += __builtin_nanf("");
        }
    }
    __syncthreads();                                               // E1: the ring is dead
    float* slab = reinterpret_cast<float*>(smem);
    g5_generic_epilogue<C::RB, CB, NST, EPI == EPI_GENERIC_ROWMUL>(p, slab, m0, n0, wave, lane, [&]() {
        if (wave < 4) g5_write_slab<C::RB, CB, NST, 4, 1, CB, true, true>(acc, slab, wave, 1, 0, lane, nullptr);
    });
}

template <int EPI, int CB>
static hipError_t launch_gemm8_t(const GemmArgs& a, const unsigned char* w8, const unsigned int* s8, int n_pad, hipStream_t st) {
    using C = Gemm8Cfg<CB>;
    static unsigned attr_mask = 0;
    if (hipError_t e = f5_set_lds_attr(reinterpret_cast<const void*>(&gemm8_kernel<EPI, CB>), C::LDS, attr_mask); e != hipSuccess) return e;
    const int tiles_m = (a.M + C::BM - 1) / C::BM, tiles_n = n_pad / C::BN;
    hipLaunchKernelGGL((gemm8_kernel<EPI, CB>), dim3(tiles_m * tiles_n), dim3(512), C::LDS, st, a, w8, s8, tiles_n);
    return hipGetLastError();
}
