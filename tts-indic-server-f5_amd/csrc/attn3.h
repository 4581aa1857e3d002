// attn3: flash-style attention forward.  S^T = K Q^T, so a query is a lane and its row statistics are in-register; exp(S) is directly the
// B operand of O^T += V^T P^T.  A wave owns a block of 32 queries; a workgroup = NW waves = one query tile of 32 NW queries; K / V^T
// tiles of 64 keys stream through an LDS ring by LDS-DMA.
//
// History of the inner loop (MI355X, C2 shape N = 1404 x 16 heads x 2, in-kernel stamps and tools/attn_bench.py, profiles/r02_attn_bench.txt):
//   attn2   ~3800 cycles per KV tile and SIMD against ~1000 of MFMA and ~2200 of VALU: the per-tile barrier keeps the two waves of a SIMD
//           in lockstep, so matrix and vector phases add up instead of overlapping;
//   attn3a  each wave carries two score tiles, S_next = K_{j+1} Q^T issued before the softmax of S_cur: 2940 per tile, 45.7 us -- the
//           stamps showed the overlap never happened: a wave is in-order, the 8 score MFMAs went out back to back (the wave sits in MFMA
//           issue for 256+ cycles with its VALU idle), then the max chain ran with the matrix pipe idle, then exp2 + PV;
//   now     (1) fixed-offset softmax (below): a third fewer VALU issue cycles, no data-dependent branch in the loop;
//           (2) half-tile steps (32 keys = one 32 x 32 score block per query block), each ONE straight-line scheduling region in which
//               sched_group_barrier spreads the MFMAs one : two exp2 : four plain VALU;
//           (3) V^T stored in vt_col order (common.h): a PV fragment is one ds_read_b128, no register shuffle; fragment addresses from
//               one lane constant by XOR;
//           (4) fragments prefetched one half tile ahead (no MFMA waits on LDS latency);
//           (5) XCD-aware workgroup numbering: the query tiles of one (sequence, head) share an L2.
//   64 queries per wave (QB = 2 blocks of 32, one wave per SIMD with the 512-register budget, every K / V^T fragment read feeding two MFMAs)
//   measured slower (profiles/r02_attn_bench.txt) and was removed; the per-wave arrays keep their query-block dimension QB = 1.
#pragma once
#include <type_traits>
#include "attn_common.h"

// NW = waves per workgroup (4, 6 or 8), NST = ring stages of 16 KiB.
// SEG2: the keys are two row ranges (AttnArgs::seq_kv_row0 / seq_kv2_*): tile kt covers 64 rows of the first range while kt < nkt1, of the
// second after it; the last tile of EACH range is masked.  SEG2 = false is the single-range kernel of the DiT / UNetT path.
//
// Operands are FP16 (round 3): q (pre-scaled), k, v^T arrive as saturated fp16 from the QKV epilogue and exp(S) is rounded to fp16 for the
// P V product -- v_mfma_f32_32x32x16_f16 issues at the bf16 rate and carries 11 significand bits instead of 8.  tools/attn_ladder.py: on the
// reference's tiny UNetT / MMDiT CFM.sample fixtures bf16 attention operands alone cost 9.7e-4 / 1.08e-3 rms (above north_star's 1e-3),
// fp16 ones 1.2e-4 / 1.4e-4; they were also what made a request's result depend on the batch it ran in.
//
// Softmax with a FIXED per-query offset folded into the score MFMAs.  q arrives scaled by log2(e) / 8 (F5_Q_SCALE), so a score is already
// a base-2 exponent.  Floating point is scale-invariant: the running maximum of online softmax only has to keep exp2 inside the range of
// the P operand, it does not have to be the maximum.  So the offset of a query is fixed BEFORE the loop: A3_OFF_MARGIN above its maximum score
// over 32 SAMPLE keys (16 spread over the whole key range, 16 around the query block's own position -- neighbouring frames are where a
// speech model's attention peaks) and stays put: the first MFMA of every score block takes C = splat(-off) instead of 0, the accumulator
// leaves the matrix pipe as s - off, and exp2 applies to it directly -- per score one exp2, one add, half a convert; no max, no subtract,
// no scale, no rescaling of O, no branch.  fp16 normals span 2^-14 .. 2^16: with the offset 2 binades above the sample maximum the sampled
// keys have P <= 1/4, the true row maximum has P >= 1/4 (samples are keys), and every P within 2^-12 of it is still a normal number.
// Whether every probability stayed below fp16's largest finite value is decided ONCE, after the loop, from the row sums themselves (they are
// accumulated by the matrix pipe from the fp16 probabilities: an overflowed one makes its row sum inf; the inf it put into O is discarded with
// it): if one did not -- a logit more than 18 binades = 12.5 nats above the query's maximum over its sample -- the 32-query BLOCK of that
// query redoes its keys with a plain running-maximum loop, correct for any input and exercised by tests/test_gpu_ops.py (k_gain and hot-block
// cases).  Only queries of the sequence vote (rows past its end belong to its padding or to the next sequence), and the vote and the redo
// are per block, not per workgroup: a block's 32 queries are the same in every variant, so which queries take the redo arithmetic does
// not depend on the launch shape.  Because every variant of the kernel (and both key halves of a BAL block) derives the offset from the
// same sample, variants differ only in the association of fp32 sums.
// (The running-maximum formulation in the hot loop measured 45.7 us at C2 against 41.4 us for the fixed offset, before any of the
// scheduling work.)
#define A3_OFF_MARGIN 2.0f
#define A3_P_LIMIT 0x1p15f
// BAL (NW = 8, 192 queries per workgroup): the SIMD-balanced form of the 6-block tile.  Eight waves put two on every SIMD; waves 0-3 own a
// query block each over all keys, waves 4 / 5 own blocks 4 / 5 over keys 0-31 of every tile and waves 6 / 7 the SAME blocks over keys 32-63,
// so every SIMD carries three half tiles per tile (with six whole-block waves two SIMDs carry four and two carry two, and the per-tile barrier
// makes the four the pace).  The two halves of blocks 4 / 5 keep their own offset, O and l and are merged once at the end through LDS.
template <int NW, bool SEG2 = false, int NST = 5, bool BAL = false>
static __global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn3_fwd_kernel(const AttnArgs p) {
    constexpr int QB = 1;          // 32-query blocks per wave
    constexpr int STAGE = 16384;   // one 64-key tile: 8 KiB of K rows + 8 KiB of V^T rows
    constexpr int P_HI = (16 + NW - 1) / NW, P_LO = 16 / NW;   // 1 KiB pieces of a KV tile per wave (pieces w, w + NW, ...)
    static_assert(!BAL || NW == 8, "BAL is the 8-wave, 6-block form");
    constexpr int QT = BAL ? 192 : 32 * QB * NW;                // queries per workgroup
    __shared__ __attribute__((aligned(16))) char smem[NST * STAGE];
    // Workgroup -> (query tile, head, sequence), XCD-aware: the hardware deals consecutive workgroup ids round-robin to the 8 XCDs, which would
    // put the query tiles of one (sequence, head) -- the workgroups that read the same K / V^T rows -- on 8 different L2s, each of them pulling
    // every row from beyond L2.  Re-number so that an XCD gets a contiguous run of (sequence, head, tile) triples, tile fastest.
    // Round 3: inside an XCD's run the HEAD is the slowest index and the sequence the middle one (it used to be the other way round: an XCD
    // then owned whole sequences, and in a ragged batch the XCD with the longest ones finished last -- 16 sequences of 900..1890 frames: 4x the
    // work on one XCD than on another: 275 us against 212 now).  An XCD now takes a group of heads of EVERY sequence: equal work whatever
    // the lengths.  (Walking the sequences by decreasing cost on top of that measured no different: profiles/r03_attn_ragged_mapping.txt.)
    int bx, by, bz;
    {
        const unsigned gx = gridDim.x, gz = gridDim.z, total = gx * gridDim.y * gz, per = total >> 3;
        const unsigned lin = blockIdx.x + gx * (blockIdx.y + gridDim.y * blockIdx.z);
        const unsigned v = lin < per * 8 ? (lin & 7) * per + (lin >> 3) : lin;
        bx = (int)(v % gx); bz = (int)((v / gx) % gz); by = (int)(v / (gx * gz));
    }
    const int seq = bz, head = by;
    const int len = p.seq_len[seq], kvlen = p.seq_kvlen[seq], row0 = p.seq_row0[seq];
    const int kv_row0 = SEG2 ? p.seq_kv_row0[seq] : row0, kv2_row0 = SEG2 ? p.seq_kv2_row0[seq] : 0, kv2_len = SEG2 ? p.seq_kv2_len[seq] : 0;
    const int nkt1 = (kvlen + 63) >> 6;
    const int q0 = bx * QT;
    if (q0 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, fh = lane >> 5;
    const int D = p.D;
    // BAL roles: 0 = whole tiles, 1 = keys 0-31 of every tile, 2 = keys 32-63; qblk = the 32-query block of the wave
    const int role = !BAL ? 0 : wave < 4 ? 0 : wave < 6 ? 1 : 2;
    const int qblk = !BAL ? wave * QB : wave < 6 ? wave : wave - 2;

    // queries of this wave (rows beyond the sequence stay inside its 128-row padding or the next sequence: finite data, never stored).
    // q0 + QT - 1 can exceed the padded rows of the LAST sequence only by < 256 rows: the workspace has that much slack.
    f16x8 qf[QB][4];
#pragma unroll
    for (int qb = 0; qb < QB; qb++) {
        const __bf16* qrow = p.qk + (size_t)(row0 + q0 + (qblk + qb) * 32 + fr) * (2 * D) + head * 64 + fh * 8;
#pragma unroll
        for (int s = 0; s < 4; s++) qf[qb][s] = *reinterpret_cast<const f16x8*>(qrow + s * 16);
    }
    // The 32 SAMPLE keys that fix the softmax offsets of this wave's queries (below): 16 spread evenly over the (first) key range and 16 at
    // every second position of the wave's own query block, clamped into the range -- all of them valid keys.  Their K
    // rows come straight from global memory in the fragment layout of a score MFMA's A operand (lane = key fr, 8 features per k-step).
    f16x8 ksamp[4];
    {
        const int sidx = fr < 16 ? (fr * kvlen) >> 4 : min(q0 + qblk * 32 + (fr - 16) * 2 * QB, kvlen - 1);
        const __bf16* krow = p.qk + (size_t)(kv_row0 + sidx) * (2 * D) + D + head * 64 + fh * 8;
#pragma unroll
        for (int s = 0; s < 4; s++) ksamp[s] = *reinterpret_cast<const f16x8*>(krow + s * 16);
    }

    // Retire the Q / sample loads BEFORE the first LDS-DMA is issued: with a DMA in flight hipcc can only wait vmcnt(0) for an
    // ordinary VGPR load, and it would put that wait inside the KV loop, draining the ring every tile.  (Issuing tile 0's DMA in front of
    // this point, so that the two latencies overlap, measured no different: profiles/r03_attn_ablate.txt.)
#pragma unroll
    for (int qb = 0; qb < QB; qb++) asm volatile("" ::"v"(qf[qb][0]), "v"(qf[qb][1]), "v"(qf[qb][2]), "v"(qf[qb][3]) : "memory");
    asm volatile("" ::"v"(ksamp[0]), "v"(ksamp[1]), "v"(ksamp[2]), "v"(ksamp[3]) : "memory");

    // LDS-DMA: a KV tile is 8 K pieces + 8 V^T pieces of 1 KiB (8 rows x 128 B); wave w moves pieces w, w + NW, ... (0-7 = K, 8-15 = V^T).
    // Physical 16-B slot (lane & 7) of row r holds logical chunk (lane & 7) ^ ((r >> 1) & 7)  (same swizzle as the fragment reads).
    const int mine = (16 - wave + NW - 1) / NW;
    const char* src[P_HI];
    size_t step[P_HI];
#pragma unroll
    for (int j = 0; j < P_HI; j++) {
        const int pc = wave + NW * j;
        const int prow = (pc & 7) * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ ((prow >> 1) & 7);
        const bool isK = pc < 8;
        src[j] = isK ? reinterpret_cast<const char*>(p.qk + (size_t)(kv_row0 + prow) * (2 * D) + D + head * 64 + chunk * 8)
                     : reinterpret_cast<const char*>(p.vt + (size_t)(head * 64 + prow) * p.ldvt + kv_row0 + chunk * 8);
        step[j] = isK ? (size_t)64 * (2 * D) * 2 : (size_t)64 * 2;   // bytes per KV tile
    }
    auto issue_tile = [&](int kt) {
        char* dst = smem + (kt % NST) * STAGE + wave * 1024;
        // tile kt starts (in rows, relative to kv_row0) at 64 kt in the first range, at kv2_row0 - kv_row0 + 64 (kt - nkt1) in the second
        const long long rel = (!SEG2 || kt < nkt1) ? (long long)kt * 64 : (long long)(kv2_row0 - kv_row0) + (long long)(kt - nkt1) * 64;
#pragma unroll
        for (int j = 0; j < P_HI; j++)
            if (j < P_LO || wave + NW * j < 16)
                attn_lds_dma16(src[j] + rel * (long long)(step[j] / 64), dst + j * NW * 1024);   // (asm: keeps hipcc's lgkmcnt waits exact, see attn_common.h)
    };
    // this wave's pieces of a tile have landed when at most `newer` younger tiles of its own are in flight
    auto wait_landed = [&](int newer) {
        switch (newer * mine) {   // (wave-uniform; vmcnt takes an immediate)
#define A3_W(N) case N: attn_wait_vmcnt<N>(); break;
            A3_W(0) A3_W(1) A3_W(2) A3_W(3) A3_W(4) A3_W(5) A3_W(6) A3_W(7) A3_W(8) A3_W(9) A3_W(10) A3_W(11) A3_W(12) A3_W(13) A3_W(14) A3_W(15) A3_W(16)
            A3_W(17) A3_W(18) A3_W(19) A3_W(20) A3_W(21) A3_W(22) A3_W(23) A3_W(24) A3_W(25) A3_W(26) A3_W(27) A3_W(28) A3_W(29) A3_W(30) A3_W(31) A3_W(32)
#undef A3_W
            default: attn_wait_vmcnt<0>(); break;
        }
    };
    static_assert((NST - 2) * P_HI <= 32, "wait_landed covers 32 outstanding pieces");
    // the same wait with a compile-time tile count: the steady state of the ring.  (The switch above compiles to a chain of ~27 scalar
    // compare / branch pairs; in-kernel stamps showed 240-500 clocks per KV tile between the end of a tile and the end of its wait with
    // every piece long landed -- the hot loop takes this path, the switch serves the first and last tiles.)
    auto wait_landed_steady = [&](auto t_) {
        constexpr int T = decltype(t_)::value;
        if constexpr (P_HI == P_LO) attn_wait_vmcnt<T * P_HI>();
        else if (mine == P_HI) attn_wait_vmcnt<T * P_HI>();
        else attn_wait_vmcnt<T * P_LO>();
    };

    f32x16 oacc[QB][2];
    f32x16 negm[QB];                   // C operand of the first score MFMA of a block = splat(-offset); zero for the first block, fixed after it
    float lrun[QB];
    // Row sums through the matrix pipe (round 3: the loop is bound by VECTOR issue at head dimension 64 -- 32 v_exp, ~75 other VALU per tile and
    // wave against 16 MFMAs -- and the sixteen v_add per half tile were its largest item after the exponentials).  One v_mfma_f32_16x16x32_f16
    // per 16-key k-step with a constant 0 / 1 A operand: seen as a 16 x 16 x 32 B operand, the P^T fragment of lane (fr, fh) is column fr & 15,
    // k-group 2 fh + (fr >> 4), i.e. k-groups {0, 2} carry query fr & 15 and {1, 3} query 16 + (fr & 15); row 0 of A is ones on k-groups {0, 2},
    // row 1 on {1, 3}, the rest zero: D[0][n] and D[1][n] accumulate the row sums of queries n and 16 + n (lanes 0-15, registers 0 and 1).  The
    // sums are those of the fp16-ROUNDED probabilities -- exactly what the P V product multiplies -- and a probability that overflowed fp16 makes
    // its row sum inf, which is the range check (no v_max in the loop either).
    f32x4 lacc[QB];
    f16x8 lones;
    {
        const int m16 = lane & 15, kq = lane >> 4;
        const _Float16 one = ((m16 == 0 && (kq & 1) == 0) || (m16 == 1 && (kq & 1) == 1)) ? (_Float16)1.0f : (_Float16)0.0f;
#pragma unroll
        for (int j = 0; j < 8; j++) lones[j] = one;
    }
#pragma unroll
    for (int qb = 0; qb < QB; qb++) {
        lrun[qb] = 0.0f;
        lacc[qb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < 16; g++) { oacc[qb][0][g] = 0.0f; oacc[qb][1][g] = 0.0f; negm[qb][g] = 0.0f; }
    }

    const int nkt = nkt1 + (SEG2 ? (kv2_len + 63) >> 6 : 0);
    constexpr bool PAIR = true;   // one ring step per TWO tiles (see ring_step)
#pragma unroll
    for (int t = 0; t < (PAIR ? NST : NST - 1); t++)
        if (t < nkt) issue_tile(t);

    // The unit of the inner loop is a HALF tile: 32 keys = one 32 x 32 score block per query block (16 registers; two whole 64-key score
    // tiles in flight cost 64 and pushed the kernel into spills and accumulator copies).
    // Fragment addresses: lds_off128(h * 32 + fr, 2 sI + fh) = fr * 128 + h * 4096 + (((2 sI) ^ (fh ^ sw)) << 4) with sw = (fr >> 1) & 7 -- ONE lane
    // constant, the k-step is an XOR on address bits 5-6, the key half an immediate offset.  The V^T fragments (feature rows, 16-key k-steps in
    // vt_col order) have the same form.
    const unsigned k_lane = (unsigned)(fr * 128 + ((fh ^ ((fr >> 1) & 7)) << 4));
    const unsigned v_lane = k_lane + 8192u;
    auto stage_of = [&](int kt) { return (unsigned)((kt % NST) * STAGE); };
    auto qk_read = [&](f16x8 (&kf)[4], int kt, int h) {
        const unsigned kb = stage_of(kt) + k_lane;
#pragma unroll
        for (int sI = 0; sI < 4; sI++) kf[sI] = *reinterpret_cast<const f16x8*>(smem + (kb ^ (unsigned)(sI << 5)) + h * 4096);
    };
    // S^T block = K_half Q^T - offset (four chained MFMAs; C of the first = negm)
    auto qk_mfma = [&](f32x16& s, const f16x8 (&kf)[4], int qb) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[0], qf[qb][0], negm[qb], 0, 0, 0);
#pragma unroll
        for (int sI = 1; sI < 4; sI++) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[sI], qf[qb][sI], s, 0, 0, 0);
    };
    // V^T fragments of k-step s2 of key half h (16 keys, stored in vt_col order: a lane's 8 keys are contiguous): one 16-byte read per 32 features
    auto v_read = [&](f16x8 (&vf)[2], unsigned vb, int h, int s2) {
#pragma unroll
        for (int dt = 0; dt < 2; dt++) vf[dt] = *reinterpret_cast<const f16x8*>(smem + (vb ^ (unsigned)((h * 2 + s2) << 5)) + dt * 4096);
    };
    // key-padding mask of half h of tile kt (only the last tile of a key range is partial)
    auto mask_half = [&](f32x16& s, int kt, int h) {
        const int valid = ((!SEG2 || kt < nkt1) ? kvlen - kt * 64 : kv2_len - (kt - nkt1) * 64) - h * 32;   // (a tile never straddles the two ranges)
        if (valid < 32) {
#pragma unroll
            for (int g = 0; g < 16; g++) {
                const int key = (g & 3) + 8 * (g >> 2) + 4 * fh;
                if (key >= valid) s[g] = -1e30f;
            }
        }
    };
    auto row_max = [&](const f32x16& s) {
        float m = s[0];
#pragma unroll
        for (int g = 1; g < 16; g++) m = fmaxf(m, s[g]);
        return fmaxf(m, __shfl_xor(m, 32, 64));
    };
    // ring step kt: tile kt + 1 landed (its K feeds the next score block); every wave is past tile kt - 1, so stage (kt - 1) % NST is free.
    // PAIR: one step per TWO tiles -- at even kt tiles kt + 1 and kt + 2 are made visible and the stages of tiles kt - 2 and kt - 1 refilled;
    // half the barriers (38 % of the wave cycles at C2 were parked at s_waitcnt / s_barrier: profiles/r02_pmc_attention_sq.txt).  The prologue
    // fills the whole ring and makes tiles 0-2 visible.  Three resident tiles + two being refilled: five stages are enough, so the 5-stage ring
    // of the batch shapes (two workgroups per CU) steps in pairs too since round 3 (the ring step was 17-18 % of the loop there:
    // profiles/r03_attn_ablate.txt); a refill then has two tile times to land instead of three.
    auto ring_step = [&](int kt) {
        if (PAIR) {
            if ((kt & 1) || kt == 0) return;
            // issued so far: tiles up to kt - 3 + NST (capped at nkt - 1); tiles kt + 1, kt + 2 must have landed
            if (kt - 3 + NST <= nkt - 1) wait_landed_steady(std::integral_constant<int, NST - 5>{});
            else wait_landed(max(0, nkt - 1 - (kt + 2)));
            __builtin_amdgcn_s_barrier();
            if (kt - 2 + NST < nkt) issue_tile(kt - 2 + NST);
            if (kt - 1 + NST < nkt) issue_tile(kt - 1 + NST);
            return;
        }
        if (nkt - 2 - kt >= NST - 3) wait_landed_steady(std::integral_constant<int, NST - 3>{});   // tiles kt + 2 .. kt + NST - 2 may stay in flight
        else wait_landed(nkt - 2 - kt);
        __builtin_amdgcn_s_barrier();
        if (kt + NST - 1 < nkt) issue_tile(kt + NST - 1);
    };
    // ---- one half tile of the FAST loop: straight-line, no branch on the data ------------------------------------------------------------
    // ONE scheduling region: per query block the four score MFMAs of the NEXT half and the four O^T += V^T P^T MFMAs of THIS half, spread one
    // MFMA : two exp2 : a few plain VALU (an in-order wave that issues MFMAs back to back sits in MFMA issue with its VALU idle, and one
    // that runs its VALU in one block leaves the matrix pipe idle); exp2 / row sum / convert of this half (scores are s - off: exp2 directly).
    // The fragments a half tile multiplies were read from LDS during the PREVIOUS half tile (two register sets that swap roles), so no MFMA
    // waits on LDS latency; ring step kt (tile kt + 1 landed and visible) therefore comes at the top of tile kt, before its first half
    // prefetches K rows of tile kt + 1.
    // H: which half of tile kt `sc` holds.  The block produced here is (kt, 1) for H = 0 and (kt + 1, 0) for H = 1.
    // NEXT_TILE: tile kt + 1 exists.  MASK: the score block produced here belongs to a possibly partial tile.
    struct Frags { f16x8 k[4]; f16x8 v[2][2]; };
    auto fast_half = [&](f32x16 (&sc)[QB], int kt, Frags& use, Frags& fill, auto h_t, auto next_tile_t, auto mask_t) {
        constexpr int H = decltype(h_t)::value;
        constexpr bool NEXT_TILE = decltype(next_tile_t)::value, MASK = decltype(mask_t)::value;
        constexpr bool HAS_NEXT = H == 0 || NEXT_TILE;
        if (H == 0) ring_step(kt);
        // prefetch for the following half tile: H = 0 -> (kt, 1) multiplies K(kt + 1, rows 0-31) and V(kt, keys 32-63);
        //                                      H = 1 -> (kt + 1, 0) multiplies K(kt + 1, rows 32-63) and V(kt + 1, keys 0-31)
        if (NEXT_TILE) qk_read(fill.k, kt + 1, H == 0 ? 0 : 1);
        if (H == 0) {
            const unsigned vb = stage_of(kt) + v_lane;
            v_read(fill.v[0], vb, 1, 0);
            v_read(fill.v[1], vb, 1, 1);
        } else if (NEXT_TILE) {
            const unsigned vb = stage_of(kt + 1) + v_lane;
            v_read(fill.v[0], vb, 0, 0);
            v_read(fill.v[1], vb, 0, 1);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int qb = 0; qb < QB; qb++) {
            f32x16 acc;
            if (HAS_NEXT) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(use.k[0], qf[qb][0], negm[qb], 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(use.k[1], qf[qb][1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(use.k[2], qf[qb][2], acc, 0, 0, 0);
            }
            float pe[16];
            f16x8 pf[2];
#pragma unroll
            for (int g = 0; g < 16; g++) pe[g] = __builtin_amdgcn_exp2f(sc[qb][g]);
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) {
#pragma unroll
                for (int j = 0; j < 8; j++) pf[s2][j] = (_Float16)pe[8 * s2 + j];
#pragma unroll
                for (int dt = 0; dt < 2; dt++) oacc[qb][dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(use.v[s2][dt], pf[s2], oacc[qb][dt], 0, 0, 0);
                lacc[qb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(lones, pf[s2], lacc[qb], 0, 0, 0);   // row sums (see lacc)
            }
            if (HAS_NEXT) sc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(use.k[3], qf[qb][3], acc, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < QB * (HAS_NEXT ? 10 : 6); i++) {   // (8 + 2 row-sum MFMAs per query block; the VALU left: 16 v_exp, 8 converts, a few moves)
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x400, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
        }
        if (HAS_NEXT && (SEG2 || MASK)) {
#pragma unroll
            for (int qb = 0; qb < QB; qb++) mask_half(sc[qb], H == 0 ? kt : kt + 1, H == 0 ? 1 : 0);
        }
    };

    // BAL, roles 1 / 2: one half tile per tile -- consumes block (kt, H), produces block (kt + 1, H); fragments read at the top of the step
    // (no prefetch across steps: K rows of tile kt + 2 are not visible yet; the whole-block wave on the same SIMD covers the latency)
    auto half_only = [&](f32x16& sc, int kt, auto h_t, auto next_tile_t) {
        constexpr int H = decltype(h_t)::value;
        constexpr bool NEXT = decltype(next_tile_t)::value;
        ring_step(kt);
        f16x8 kf[4], vf[2][2], pf[2];
        if (NEXT) qk_read(kf, kt + 1, H);
        const unsigned vb = stage_of(kt) + v_lane;
        v_read(vf[0], vb, H, 0);
        v_read(vf[1], vb, H, 1);
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc;
        if (NEXT) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[0], qf[0][0], negm[0], 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[1], qf[0][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[2], qf[0][2], acc, 0, 0, 0);
        }
        float pe[16];
#pragma unroll
        for (int g = 0; g < 16; g++) pe[g] = __builtin_amdgcn_exp2f(sc[g]);
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++) {
#pragma unroll
            for (int j = 0; j < 8; j++) pf[s2][j] = (_Float16)pe[8 * s2 + j];
#pragma unroll
            for (int dt = 0; dt < 2; dt++) oacc[0][dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[s2][dt], pf[s2], oacc[0][dt], 0, 0, 0);
            lacc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(lones, pf[s2], lacc[0], 0, 0, 0);
        }
        if (NEXT) sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[3], qf[0][3], acc, 0, 0, 0);
        // the first exp2 / converts run while the fragments are on their way from LDS, then one MFMA : two exp2 : a few VALU
        __builtin_amdgcn_sched_group_barrier(0x400, 6, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
#pragma unroll
        for (int i = 0; i < (NEXT ? 10 : 6); i++) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x400, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
        }
        if (NEXT) mask_half(sc, kt + 1, H);   // (tests the tile's key count itself)
    };

    f32x16 sa[QB];   // the score blocks of the half tile about to be consumed
    Frags fa, fb;
    const int h_first = (BAL && role == 2) ? 1 : 0;   // the half of tile 0 this wave starts with
    // tile 0 must have landed before the first score block: tiles 1 .. NST - 2 may stay in flight (PAIR: tiles 0-2 landed, 3 .. NST - 1 in flight)
    if (PAIR) wait_landed(max(0, min(NST - 1, nkt - 1) - 2));
    else wait_landed(min(NST - 2, nkt - 1));
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int qb = 0; qb < QB; qb++) {   // the queries' offsets = 2 + their maxima over the sample keys (C = 0: negm is still zero)
        f32x16 ss;
        qk_mfma(ss, ksamp, qb);
        const float m0 = row_max(ss) + A3_OFF_MARGIN;
#pragma unroll
        for (int g = 0; g < 16; g++) negm[qb][g] = -m0;
    }
    {
        f16x8 kf0[4];
        if (BAL && role == 2) qk_read(kf0, 0, 1); else qk_read(kf0, 0, 0);
#pragma unroll
        for (int qb = 0; qb < QB; qb++) {
            qk_mfma(sa[qb], kf0, qb);   // = s - offset
            mask_half(sa[qb], 0, h_first);   // (role 2 with at most 32 keys: nothing valid in its half -- its P are exp2(-1e30) = 0, its O and l stay 0)
        }
    }
    if (!BAL || role == 0) {
        qk_read(fa.k, 0, 1);    // what half (0, 0) multiplies: K rows 32-63 and V keys 0-31 of tile 0
        v_read(fa.v[0], stage_of(0) + v_lane, 0, 0);
        v_read(fa.v[1], stage_of(0) + v_lane, 0, 1);
    }
    using T_ = std::true_type;
    using F_ = std::false_type;
    using H0 = std::integral_constant<int, 0>;
    using H1 = std::integral_constant<int, 1>;
    if (!BAL || role == 0) {
        int kt = 0;
        for (; kt + 2 < nkt; kt++) {   // tiles whose successors are complete tiles: no masks
            fast_half(sa, kt, fa, fb, H0{}, T_{}, F_{});
            fast_half(sa, kt, fb, fa, H1{}, T_{}, F_{});
        }
        for (; kt < nkt; kt++) {   // the last one or two tiles
            if (kt + 1 < nkt) {
                fast_half(sa, kt, fa, fb, H0{}, T_{}, T_{});
                fast_half(sa, kt, fb, fa, H1{}, T_{}, T_{});
            } else {
                fast_half(sa, kt, fa, fb, H0{}, F_{}, T_{});
                fast_half(sa, kt, fb, fa, H1{}, F_{}, F_{});
            }
        }
    } else if (role == 1) {   // (one ring step per tile, like the whole-block waves: the barriers pair up)
        for (int kt = 0; kt + 1 < nkt; kt++) half_only(sa[0], kt, H0{}, T_{});
        half_only(sa[0], nkt - 1, H0{}, F_{});
    } else {
        for (int kt = 0; kt + 1 < nkt; kt++) half_only(sa[0], kt, H1{}, T_{});
        half_only(sa[0], nkt - 1, H1{}, F_{});
    }
    // Did every probability of this block's queries stay in range (l_bad above)?  One bit per 32-query block, set by every wave of the block that
    // saw an overflow (BAL: both key-half waves of blocks 4 / 5).  (The mask lives in the first bytes of the ring -- 5 x 16 KiB is exactly half a
    // CU's LDS, two workgroups per CU -- hence the barriers: everybody done with the ring | mask cleared | bits set | mask read.)
    // the row sums of this wave's queries out of the 16 x 16 accumulators: query fr sits in lane fr & 15, register fr >> 4.  Kept as before as a
    // per-lane partial that the epilogue (and the BAL merge) adds over the two lane halves: the whole sum in lanes 0-31, zero in lanes 32-63.
    bool l_bad = false;
#pragma unroll
    for (int qb = 0; qb < QB; qb++) {
        const float l0 = __shfl(lacc[qb][0], fr & 15, 64), l1 = __shfl(lacc[qb][1], fr & 15, 64);
        const float lq = (fr >> 4) ? l1 : l0;
        // inf (a probability overflowed fp16) or NaN, of a query of the sequence: rows past its end (its padding, or the next sequence's
        // queries in the last tile of a 6- or 8-wave workgroup) must not send a block of this one to the redo
        l_bad = l_bad || (q0 + (qblk + qb) * 32 + fr < len && !(lq <= 3.0e38f));
        lrun[qb] = fh ? 0.0f : lq;
    }
    int* redo_mask = reinterpret_cast<int*>(smem);
    attn_wait_vmcnt<0>();
    __syncthreads();
    if (threadIdx.x == 0) *redo_mask = 0;
    __syncthreads();
    if (__any(l_bad) && lane == 0) atomicOr(redo_mask, 1 << qblk);
    __syncthreads();
    const int mask = *redo_mask;
    const bool redo = (mask >> qblk) & 1;   // this wave's block redoes; every wave takes part in the loop's tile moves and barriers if any does
    __syncthreads();
    if (mask) {   // GENERAL loop: running maximum, any input; plain code, one query block at a time
        float mrun[QB];
#pragma unroll
        for (int qb = 0; qb < QB; qb++) {
            mrun[qb] = -1e30f;
            if (!redo) continue;
            lrun[qb] = 0.0f;
#pragma unroll
            for (int g = 0; g < 16; g++) { oacc[qb][0][g] = 0.0f; oacc[qb][1][g] = 0.0f; negm[qb][g] = 0.0f; }
        }
#pragma unroll
        for (int t = 0; t < NST - 1; t++)
            if (t < nkt) issue_tile(t);
        for (int gk = 0; gk < nkt; gk++) {
            // tile gk landed for everybody; every wave is past tile gk - 1, so its stage can take tile gk + NST - 2
            wait_landed(min(gk == 0 ? NST - 2 : NST - 3, nkt - 1 - gk));   // issued so far: tiles 0 .. NST - 2 at gk = 0, up to gk + NST - 3 after
            __builtin_amdgcn_s_barrier();
            if (gk > 0 && gk + NST - 2 < nkt) issue_tile(gk + NST - 2);
            const unsigned vb = stage_of(gk) + v_lane;
#pragma unroll 1
            for (int h = 0; h < 2; h++) {
                // (waves of blocks that keep their fast-loop result, and BAL's waves 6 / 7, only move tiles and keep the barriers; blocks 4 / 5
                // are redone whole by waves 4 / 5)
                if (!redo || (BAL && role == 2)) break;
                f16x8 kf[4];
                qk_read(kf, gk, h);
#pragma unroll
                for (int qb = 0; qb < QB; qb++) {
                    f32x16 sg;
                    qk_mfma(sg, kf, qb);
                    mask_half(sg, gk, h);
                    const float mnew = fmaxf(mrun[qb], row_max(sg));
                    const float alpha = __builtin_amdgcn_exp2f(mrun[qb] - mnew);
                    mrun[qb] = mnew;
                    float rs = 0.0f;
#pragma unroll
                    for (int g = 0; g < 16; g++) {
                        sg[g] = __builtin_amdgcn_exp2f(sg[g] - mnew);
                        rs += sg[g];
                    }
                    lrun[qb] = lrun[qb] * alpha + rs;
#pragma unroll
                    for (int dt = 0; dt < 2; dt++)
#pragma unroll
                        for (int g = 0; g < 16; g++) oacc[qb][dt][g] *= alpha;
#pragma unroll
                    for (int s2 = 0; s2 < 2; s2++) {
                        f16x8 pf, vf[2];
#pragma unroll
                        for (int j = 0; j < 8; j++) pf[j] = (_Float16)sg[8 * s2 + j];
                        v_read(vf, vb, h, s2);
#pragma unroll
                        for (int dt = 0; dt < 2; dt++) oacc[qb][dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[dt], pf, oacc[qb][dt], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (BAL) {
        // merge the key halves of blocks 4 / 5: waves 6 / 7 hand (offset, l, O) to waves 4 / 5 through LDS (the ring is idle), which bring both to the
        // larger offset -- exact power-of-two factors <= 1 -- and add.  After a redo of its block the whole-block result of wave 4 / 5 stands alone.
        float* mbuf = reinterpret_cast<float*>(smem) + (size_t)(wave & 1) * 34 * 64;
        __syncthreads();
        if (role == 2 && !redo) {
            mbuf[lane] = -negm[0][0];
            mbuf[64 + lane] = lrun[0];
#pragma unroll
            for (int dt = 0; dt < 2; dt++)
#pragma unroll
                for (int g = 0; g < 16; g++) mbuf[(2 + dt * 16 + g) * 64 + lane] = oacc[0][dt][g];
        }
        __syncthreads();
        if (role == 1 && !redo) {
            const float off_a = -negm[0][0], off_b = mbuf[lane];
            const float m = fmaxf(off_a, off_b);
            const float fa_ = __builtin_amdgcn_exp2f(off_a - m), fb_ = __builtin_amdgcn_exp2f(off_b - m);
            lrun[0] = lrun[0] * fa_ + mbuf[64 + lane] * fb_;
#pragma unroll
            for (int dt = 0; dt < 2; dt++)
#pragma unroll
                for (int g = 0; g < 16; g++) oacc[0][dt][g] = oacc[0][dt][g] * fa_ + mbuf[(2 + dt * 16 + g) * 64 + lane] * fb_;
        }
        if (role == 2) return;   // (no barrier after this point)
    }

#pragma unroll
    for (int qb = 0; qb < QB; qb++) {
        const float ltot = lrun[qb] + __shfl_xor(lrun[qb], 32, 64);
        const float inv = 1.0f / ltot;
        const int q = q0 + (qblk + qb) * 32 + fr;
        if (q < len) {
            const size_t obase = (size_t)(row0 + q) * D + head * 64;
#pragma unroll
            for (int dt = 0; dt < 2; dt++)
#pragma unroll
                for (int a = 0; a < 4; a++) {
                    bf16x4 hi4, lo4;
                    float ov[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) ov[e] = oacc[qb][dt][a * 4 + e] * inv;
                    const int d = dt * 32 + 8 * a + 4 * fh;
                    if (p.f16_out) {
                        store_f16x4(p.out_hi + obase + d, ov);
                        continue;
                    }
                    split_bf16x4(ov, hi4, lo4);
                    *reinterpret_cast<bf16x4*>(p.out_hi + obase + d) = hi4;
                    if (p.out_lo) *reinterpret_cast<bf16x4*>(p.out_lo + obase + d) = lo4;
                }
        }
    }
}
