// translation unit: attention forward (attn3.h)
#include "attn3.h"
#include "gemm_launch.h"

// Which attn3 instance: the tile height 32 NW, NW in {4, 6, 8}, that needs the fewest (rounds on the 256 CUs) x (work per workgroup); ties -> the
// larger tile (fewer re-reads of K / V).  The grid is sized for the longest sequence; workgroups past a shorter one's end exit at once.
//   * 192-query tiles (NW = 6) run as the SIMD-balanced 8-wave kernel (attn3.h BAL): eight 240-register waves fill a CU, so it has the CU to
//     itself and takes the 9-stage ring.  f5hip_set_attention_shape_invariant(1) keeps the 6-wave form, whose arithmetic is that of every
//     other variant.
//   * ring depth otherwise: a tile takes 2-4 us from beyond L2 into LDS and is consumed in ~1 us, so 3 tiles in flight (5 stages, 80 KiB: two
//     workgroups per CU when the grid has more than one round) starve a LONE workgroup per CU -- 6- and 8-wave launches of at most 256
//     workgroups get 9 stages (144 KiB, 7 tiles in flight); at NW = 4 the deep ring measured slower (16.8 vs 14.3 us at 2 x 748 x 12 heads).
// Measured and removed: 64 queries per wave (QB = 2, 38.8 against 35.4 us at C2: hipcc parks half of its score blocks in
// AGPRs and a lone in-order wave cannot cover its own waits, which two waves per SIMD do for each other), the ping-pong kernel (11-40 %
// slower, profiles/r03_attn5_pingpong.txt) and 16 x 16 x 32 MFMA blocks with unequal-height waves (profiles/r02_attn_bench.txt).
static int g_attn_shape_invariant = 0;   // f5hip_set_attention_shape_invariant: the default of launches whose AttnArgs::shape_invariant is -1
void f5_set_attn_shape_invariant(int on) { g_attn_shape_invariant = on != 0; }
// Launch counters (test instrumentation, read through f5hip_get_counter): one per instance, in the order of attn3_launch, then two-range launches
static long long g_attn_counters[F5_ATTN_CNT_COUNT] = {};
long long* f5_attn_counters() { return g_attn_counters; }

template <bool SEG2>
static void attn3_launch(const AttnArgs& a, int best, bool deep, bool bal, dim3 grid, hipStream_t st) {
    g_attn_counters[bal ? 0 : best == 8 ? (deep ? 1 : 2) : best == 6 ? (deep ? 3 : 4) : 5]++;
    if (SEG2) g_attn_counters[6]++;
    if (bal) hipLaunchKernelGGL((attn3_fwd_kernel<8, SEG2, 9, true>), grid, dim3(512), 0, st, a);
    else if (best == 8 && deep) hipLaunchKernelGGL((attn3_fwd_kernel<8, SEG2, 9>), grid, dim3(512), 0, st, a);
    else if (best == 8) hipLaunchKernelGGL((attn3_fwd_kernel<8, SEG2, 5>), grid, dim3(512), 0, st, a);
    else if (best == 6 && deep) hipLaunchKernelGGL((attn3_fwd_kernel<6, SEG2, 9>), grid, dim3(384), 0, st, a);
    else if (best == 6) hipLaunchKernelGGL((attn3_fwd_kernel<6, SEG2, 5>), grid, dim3(384), 0, st, a);
    else hipLaunchKernelGGL((attn3_fwd_kernel<4, SEG2, 5>), grid, dim3(256), 0, st, a);
}

hipError_t f5_launch_attn3(const AttnArgs& a, int max_len, int heads, int n_seq, hipStream_t st) {
    if (a.seq_kv2_row0 && (!a.seq_kv_row0 || !a.seq_kv2_len)) return hipErrorInvalidValue;   // two key ranges per (pseudo-)sequence: MMDiT joint attention
    int best = 8;
    long long best_cost = -1;
    for (int nw : {8, 6, 4}) {
        const long long wgs = (long long)((max_len + 32 * nw - 1) / (32 * nw)) * heads * n_seq;
        const long long cost = ((wgs + 255) / 256) * nw;
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = nw; }
    }
    const dim3 grid((max_len + 32 * best - 1) / (32 * best), heads, n_seq);
    const bool deep = best >= 6 && (long long)grid.x * grid.y * grid.z <= 256;
    const bool invariant = a.shape_invariant < 0 ? g_attn_shape_invariant != 0 : a.shape_invariant != 0;
    const bool bal = best == 6 && !invariant;
    if (a.seq_kv2_row0) attn3_launch<true>(a, best, deep, bal, grid, st);
    else attn3_launch<false>(a, best, deep, bal, grid, st);
    return hipGetLastError();
}
