// The true-peak limiter beside the loudness target.  Included by f5hip.hip behind wave_out.h, whose meter it runs as it stands.
// f5hip_wave_loudness_limit: the 24 kHz int16 PCM of n requests, in place -- a request with a ceiling to wave_codec.limit_pcm16, a request
// with a target alone to normalise_loudness_pcm16 (f5hip_wave_loudness's arithmetic), bit for bit; the definition is written down in
// wave_codec.py and include/f5hip.h.  Integers up to the gain's one sqrt: no sum or minimum depends on the order of its terms, so the tiling
// decides no bit.  The request table lists the requests with a target alone, then those with a target and a ceiling, then those with a
// ceiling alone: wave_kweight_kernel and wave_gate_kernel run over the first two groups, wave_truepeak_kernel over the last two.
//   wave_truepeak_kernel     one block of 256 threads per (request with a ceiling, tile of kLmTile = 2048 samples).  The tile and its 6 + 6
//                            sample halo go to LDS as int16 pairs; a thread reads the 20 samples around its 8 outputs as three 16-byte LDS
//                            loads.  An interpolated point is a chain of v_dot2_i32_i16 over aligned pairs: six for an odd output, seven
//                            (the taps moved on by one sample, a zero at each end) for an even one, the taps as literals; m is the largest
//                            of 2^14 |x| and the three |v_p|.  G comes from the request's stats row (n2, S2) and its K_T.  Only where
//                            m G > c 2^30 is there a 64-bit division.  A tile in which that happens writes its r (int32) to the workspace
//                            and sets its flag; any other tile writes its cleared flag alone.
//   wave_limit_apply_kernel  one block per (request, tile).  A request without a ceiling takes wave_gain_kernel's body.  A tile whose flag
//                            and whose neighbours' flags (2 M < kLmTile: one tile on each side) are clear is x <- clip(rint(x G / 2^16)),
//                            wave_gain_kernel's body again with g = G / 2^16 (exact in fp64), and nothing at all for G = 2^16.  Otherwise r
//                            over [t0 - 2 M, t0 + T + 2 M) goes to LDS (2^16 for a cleared tile and outside the wave), the minima over
//                            [j, j + 2^k) are doubled in place up to 256, s[u] = min(span256[u], span256[u + 225]) is the window of 481 --
//                            ten compares an output --, and stored as 2^16 - s.  A thread then owns 8 consecutive outputs and slides the
//                            window over them 8 weights at a time: 16 deficits in registers, the weights as broadcast 16-byte LDS reads,
//                            64 v_mad_u32_u24 a step; a = 2^16 - ceil(D / 2^16); y by a 64-bit product and a rounded floor shift.
// Four launches whatever n; no atomics, no host sync: the request table goes through pinned staging on the stream.
#pragma once

constexpr int kLmTile = 2048;                   // outputs of a block: 8 a thread
constexpr int kLmHold = 240;                    // wave_codec.LIMIT_HOLD
constexpr int kLmWin = 2 * kLmHold + 1;
constexpr int kLmUnity = 1 << 16;
constexpr double kLmGainMax = 4194304.0;        // wave_codec.LIMIT_GAIN_MAX
constexpr int kLmCeilingMin = 11626, kLmCeilingMax = 32767;   // wave_codec.true_peak_ceiling(-9.0), (0.0)
constexpr short kLmTaps[3][12] = {
#include "truepeak_taps.inc"
};
constexpr int kLmWindow[kLmWin] = {
#include "limit_window.inc"
};
constexpr int lm_abs(int v) { return v < 0 ? -v : v; }
constexpr int lm_tap_abs_sum(int p) { int s = 0; for (int k = 0; k < 12; k++) s += lm_abs(kLmTaps[p][k]); return s; }
constexpr long long lm_window_sum() { long long s = 0; for (int k = 0; k < kLmWin; k++) s += kLmWindow[k]; return s; }
constexpr int lm_window_max() { int m = 0; for (int k = 0; k < kLmWin; k++) m = kLmWindow[k] > m ? kLmWindow[k] : m; return m; }
// the bit budget (wave_codec.py states it): |v_p| < 2^30 at every partial sum, m G < 2^52, r >= 181, so a deficit 2^16 - s fits 16 bits and
// the 481 products of a window sum stay below 2^32
static_assert(lm_tap_abs_sum(0) < 32768 && lm_tap_abs_sum(1) < 32768 && lm_tap_abs_sum(2) < 32768, "wave_limit: |v_p| < 2^30");
static_assert(lm_window_sum() == kLmUnity && lm_window_max() < (1 << 16), "wave_limit: the window sums to 2^16");
static_assert((((long long)kLmCeilingMin << 46) >> 52) >= 1, "wave_limit: r > 0");
static_assert(kLmTile % 8 == 0 && kLmTile == 8 * 256 && 2 * kLmHold < kLmTile, "wave_limit tiling: one neighbour tile on each side");
constexpr int kLmRSpan = kLmTile + 4 * kLmHold;         // r staged by a slow tile
constexpr int kLmSSpan = kLmTile + 2 * kLmHold + 8;     // its deficits (the last step of the window reads 7 past the last one it weighs)
constexpr int kLmWPad = (kLmWin + 7) / 8 * 8;           // the weights, zero padded to whole steps

// two int16 taps as one dot2 operand: lo weighs the pair's first sample
constexpr int lm_pair(int lo, int hi) { return (int)(((unsigned)hi << 16) | ((unsigned)lo & 0xffffu)); }
// tap pair w of phase p for an output at an even (shift = 1: 7 pairs, zeros at the ends) or odd (shift = 0: 6 pairs) sample
constexpr int lm_tap(int p, int k) { return k < 0 || k > 11 ? 0 : kLmTaps[p][k]; }
constexpr int lm_tap_pair(int p, int w, int shift) { return lm_pair(lm_tap(p, 2 * w - shift), lm_tap(p, 2 * w + 1 - shift)); }

typedef short lm_short2 __attribute__((ext_vector_type(2)));
F5_DEVICE int lm_dot2(int x, int t, int acc) {
#if __has_builtin(__builtin_amdgcn_sdot2)
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(lm_short2, x), __builtin_bit_cast(lm_short2, t), acc, false);
#else
    return acc + (int)(short)(x & 0xffff) * (int)(short)(t & 0xffff) + (x >> 16) * (t >> 16);
#endif
}

// |v_p| of the output at sample e (0 .. 7) of a thread whose word xw[0] holds samples (-6, -5) relative to its first output
template <int P, int E>
F5_DEVICE int lm_phase(const int (&xw)[12]) {
    int acc = 0;
    if constexpr (E % 2 == 0) {      // x[e - 6 .. e + 7]: words e / 2 .. e / 2 + 6
#pragma unroll
        for (int w = 0; w < 7; w++) acc = lm_dot2(xw[E / 2 + w], lm_tap_pair(P, w, 1), acc);
    } else {                         // x[e - 5 .. e + 6]: words (e + 1) / 2 .. + 5
#pragma unroll
        for (int w = 0; w < 6; w++) acc = lm_dot2(xw[(E + 1) / 2 + w], lm_tap_pair(P, w, 0), acc);
    }
    return abs(acc);
}

template <int E>
F5_DEVICE int lm_reading(const int (&xw)[12]) {
    const int word = xw[3 + E / 2];
    const int x = E % 2 ? word >> 16 : (int)(short)(word & 0xffff);
    return max(max(abs(x) << 14, lm_phase<0, E>(xw)), max(lm_phase<1, E>(xw), lm_phase<2, E>(xw)));
}

template <int E>
F5_DEVICE void lm_readings(const int (&xw)[12], int (&m)[8]) {
    if constexpr (E < 8) {
        m[E] = lm_reading<E>(xw);
        lm_readings<E + 1>(xw, m);
    }
}

// G of a request with a ceiling: Q16, from its stats row when it has a target (wave_codec.limit_gain)
F5_DEVICE long long lm_gain(const LdReq& q, const long long* __restrict__ stats) {
    if (!(q.gain_k > 0.0)) return kLmUnity;
    const long long* row = stats + 4LL * q.req;
    if (row[0] == 0) return kLmUnity;
    return (long long)fmin(rint(65536.0 * sqrt(q.gain_k * (double)row[0] / (double)row[1])), kLmGainMax);
}

// (target no-packed-fp32-ops: kernels new to this library are compiled without the packed fp32 VALU forms; these two are all-integer beside
// the gain, so it changes no instruction)
__global__ __launch_bounds__(256) __attribute__((target("no-packed-fp32-ops"))) void wave_truepeak_kernel(
    const LdReq* __restrict__ reqs, int nf, int ltile_base, const short* __restrict__ pcm, const int* __restrict__ len_dev,
    const long long* __restrict__ stats, int* __restrict__ rws, int* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) int xs[(kLmTile + 16) / 2];   // samples t0 - 6 .. t0 + T + 9 as pairs; the last 4 are never weighed
    const int tid = threadIdx.x;
    const int lt = (int)blockIdx.x + ltile_base;
    const LdReq q = reqs[last_at_or_before<&LdReq::ltile0>(reqs, nf, lt)];
    const int len = ld_len(len_dev, q);
    const long long t0 = (long long)(lt - q.ltile0) * kLmTile;
    if (t0 >= len) {                                                    // a tile past the request's actual length
        if (tid == 0) flags[lt] = 0;
        return;
    }
    const short* x = pcm + q.in_off;
    short* xh = reinterpret_cast<short*>(xs);
    {
        const long long j = t0 + 8 * tid;
        int w4[4] = {0, 0, 0, 0};
        if (j + 8 <= len && (reinterpret_cast<uintptr_t>(x + j) & 15) == 0) {
            const int4 in = *reinterpret_cast<const int4*>(x + j);
            w4[0] = in.x; w4[1] = in.y; w4[2] = in.z; w4[3] = in.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int v = j + e < len ? (int)(unsigned short)x[j + e] : 0;
                w4[e / 2] |= v << (16 * (e % 2));
            }
        }
#pragma unroll
        for (int w = 0; w < 4; w++) xs[3 + 4 * tid + w] = w4[w];
        if (tid < 6) xh[tid] = t0 - 6 + tid >= 0 ? x[t0 - 6 + tid] : (short)0;
        else if (tid < 16) { const long long s = t0 + kLmTile + (tid - 6); xh[6 + kLmTile + (tid - 6)] = s < len ? x[s] : (short)0; }
    }
    __syncthreads();
    int xw[12];
    {
        const int4* src = reinterpret_cast<const int4*>(xs + 4 * tid);
#pragma unroll
        for (int v = 0; v < 3; v++) {
            const int4 in = src[v];                                     // (words 4 tid .. 4 tid + 11 <= 1031: inside xs for every thread)
            xw[4 * v] = in.x; xw[4 * v + 1] = in.y; xw[4 * v + 2] = in.z; xw[4 * v + 3] = in.w;
        }
    }
    int m[8];
    lm_readings<0>(xw, m);
    const long long G = lm_gain(q, stats);
    const long long cs = (long long)q.ceiling << 30;
    int r[8];
    bool over = false;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const long long mg = (long long)m[e] * G;
        r[e] = kLmUnity;
        if (mg > cs && t0 + 8 * tid + e < len) {                        // outside the wave r is 2^16
            r[e] = (int)((unsigned long long)(cs << 16) / (unsigned long long)mg);
            over = true;
        }
    }
    const int flag = __syncthreads_or(over);
    if (tid == 0) flags[lt] = flag;
    if (!flag) return;
    int4* dst = reinterpret_cast<int4*>(rws + (long long)lt * kLmTile + 8 * tid);
    dst[0] = make_int4(r[0], r[1], r[2], r[3]);
    dst[1] = make_int4(r[4], r[5], r[6], r[7]);
}

// y of one sample: clip(x G a / 2^32), half to even (ga = G a < 2^38)
F5_DEVICE short lm_scale(int x, long long ga) {
    const long long p = (long long)x * ga;
    const long long y = (p + (1LL << 31) - 1 + ((p >> 32) & 1)) >> 32;
    return (short)min(max(y, -32768LL), 32767LL);
}

__global__ __launch_bounds__(256) __attribute__((target("no-packed-fp32-ops"))) void wave_limit_apply_kernel(
    const LdReq* __restrict__ reqs, int nf, short* __restrict__ pcm, const int* __restrict__ len_dev, const long long* __restrict__ stats,
    const int* __restrict__ rws, const int* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) int rs[kLmRSpan];
    __shared__ __attribute__((aligned(16))) int ds[kLmSSpan];
    __shared__ __attribute__((aligned(16))) int ww[kLmWPad];
    const int tid = threadIdx.x;
    const int lt = (int)blockIdx.x;
    const LdReq q = reqs[last_at_or_before<&LdReq::ltile0>(reqs, nf, lt)];
    const int len = ld_len(len_dev, q);
    const int tile = lt - q.ltile0;
    const long long t0 = (long long)tile * kLmTile;
    if (t0 >= len) return;
    short* x = pcm + q.in_off;
    if (q.ceiling == 0) {                                               // a target alone: f5hip_wave_loudness's third launch
        const long long* row = stats + 4LL * q.req;
        if (row[0] != 0) ld_gain_tile(x, len, t0, kLmTile, __longlong_as_double(row[3]));
        return;
    }
    const long long G = lm_gain(q, stats);
    const bool slow = flags[lt] || (tile > 0 && flags[lt - 1]) || (tile + 1 < q.ltiles && flags[lt + 1]);
    if (!slow) {
        if (G != kLmUnity) ld_gain_tile(x, len, t0, kLmTile, (double)G * (1.0 / 65536.0));
        return;
    }
    // r over [t0 - 2 M, t0 + T + 2 M): a cleared tile and the outside of the wave read 2^16
    for (int i = tid; i < kLmRSpan; i += 256) {
        const long long j = t0 - 2 * kLmHold + i;
        int v = kLmUnity;
        if (j >= 0 && j < len) {
            const int tj = (int)(j / kLmTile);
            if (flags[q.ltile0 + tj]) v = rws[(long long)(q.ltile0 + tj) * kLmTile + (j - (long long)tj * kLmTile)];
        }
        rs[i] = v;
    }
    for (int i = tid; i < kLmWPad; i += 256) ww[i] = i < kLmWin ? kLmWindow[i] : 0;
    __syncthreads();
    // rs[i] <- min rs[i .. i + width): doubled in place, every thread's reads before anybody's writes
    constexpr int kPer = (kLmRSpan + 255) / 256;
    for (int width = 1; width < 256; width *= 2) {
        int v[kPer];
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const int i = tid + 256 * k;
            v[k] = i + width < kLmRSpan ? min(rs[i], rs[i + width]) : (i < kLmRSpan ? rs[i] : kLmUnity);   // (past the span's end: never read as a window)
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPer; k++) if (tid + 256 * k < kLmRSpan) rs[tid + 256 * k] = v[k];
        __syncthreads();
    }
    // s over [t0 - M, t0 + T + M) as the deficit 2^16 - s: the window of 481 is two spans of 256
    for (int u = tid; u < kLmSSpan; u += 256) ds[u] = u < kLmTile + 2 * kLmHold ? kLmUnity - min(rs[u], rs[u + kLmWin - 256]) : 0;
    __syncthreads();
    unsigned acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int d[16];
    {
        const int4* src = reinterpret_cast<const int4*>(ds + 8 * tid);
        const int4 a = src[0], b = src[1];
        d[8] = a.x; d[9] = a.y; d[10] = a.z; d[11] = a.w; d[12] = b.x; d[13] = b.y; d[14] = b.z; d[15] = b.w;
    }
    for (int k0 = 0; k0 < kLmWPad; k0 += 8) {
        const int4* src = reinterpret_cast<const int4*>(ds + 8 * tid + k0 + 8);
        const int4* wsrc = reinterpret_cast<const int4*>(ww + k0);
        const int4 a = src[0], b = src[1], wa = wsrc[0], wb = wsrc[1];
#pragma unroll
        for (int e = 0; e < 8; e++) d[e] = d[e + 8];
        d[8] = a.x; d[9] = a.y; d[10] = a.z; d[11] = a.w; d[12] = b.x; d[13] = b.y; d[14] = b.z; d[15] = b.w;
        const int w8[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
        for (int kk = 0; kk < 8; kk++)
#pragma unroll
            for (int e = 0; e < 8; e++) acc[e] += __umul24(w8[kk], d[e + kk]);
    }
    const long long j = t0 + 8 * tid;
    if (j >= len) return;
    long long ga[8];
#pragma unroll
    for (int e = 0; e < 8; e++) ga[e] = G * (long long)(kLmUnity - (int)((acc[e] + 65535u) >> 16));
    if (j + 8 <= len && (reinterpret_cast<uintptr_t>(x + j) & 15) == 0) {
        const int4 in = *reinterpret_cast<const int4*>(x + j);
        const int w4[4] = {in.x, in.y, in.z, in.w};
        int o[4];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int lo = lm_scale((int)(short)(w4[w] & 0xffff), ga[2 * w]);
            const int hi = lm_scale(w4[w] >> 16, ga[2 * w + 1]);
            o[w] = (lo & 0xffff) | (hi << 16);
        }
        *reinterpret_cast<int4*>(x + j) = make_int4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; e++) if (j + e < len) x[j + e] = lm_scale((int)x[j + e], ga[e]);
    }
}

struct LmWorkspace {
    LdReq* reqs = nullptr; size_t cap_reqs = 0;
    long long* sub = nullptr; size_t cap_sub = 0;
    int* peaks = nullptr; size_t cap_peaks = 0;
    int* rws = nullptr; size_t cap_rws = 0;
    int* flags = nullptr; size_t cap_flags = 0;
    HostStage stage;
    WorkspaceUse use;
};

int f5hip_wave_loudness_limit_tile(void) { return kLmTile; }
int f5hip_wave_loudness_limit_launches(void) { return 4; }

int f5hip_wave_loudness_limit(int32_t n, int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev,
                              const double* gain_k, const int32_t* ceiling, int64_t* stats_dev, void* stream) {
    if (n < 1 || !ceiling) return fail(-1, "wave_loudness_limit: bad argument");
    bool limited = false;
    for (int i = 0; i < n; i++) {
        if (ceiling[i] != 0 && (ceiling[i] < kLmCeilingMin || ceiling[i] > kLmCeilingMax))
            return fail(-1, "wave_loudness_limit: request %d has ceiling %d (0, or %d .. %d)", i, ceiling[i], kLmCeilingMin, kLmCeilingMax);
        limited = limited || ceiling[i] != 0;
    }
    if (!limited) return f5hip_wave_loudness(n, pcm_dev, in_off, max_len, len_dev, gain_k, stats_dev, stream);   // the call as it stands
    if (!pcm_dev || !in_off || !max_len || !gain_k || !stats_dev) return fail(-1, "wave_loudness_limit: bad argument");
    if ((reinterpret_cast<uintptr_t>(pcm_dev) & 1) || (reinterpret_cast<uintptr_t>(len_dev) & 3) || (reinterpret_cast<uintptr_t>(stats_dev) & 7))
        return fail(-1, "wave_loudness_limit: the samples must be 2-byte aligned, the lengths 4-byte and the stats 8-byte");
    long long total = 0;
    for (int i = 0; i < n; i++) {
        if (max_len[i] < 0) return fail(-1, "wave_loudness_limit: request %d has a negative length bound (%d)", i, max_len[i]);
        if (in_off[i] < 0) return fail(-1, "wave_loudness_limit: request %d has a negative offset", i);
        if (!std::isfinite(gain_k[i])) return fail(-1, "wave_loudness_limit: the gain constant of request %d is not finite", i);
        total += max_len[i];
        if (total > 2147483647LL) return fail(-1, "wave_loudness_limit: the call exceeds 2^31 - 1 samples");
    }
    // the table: a target alone, then a target and a ceiling, then a ceiling alone (an empty request keeps one block of each kind)
    std::vector<LdReq> h;
    long long tiles = 0, ltiles = 0, plain_ltiles = 0;
    int metered = 0, plain = 0;
    for (int group = 0; group < 3; group++) {
        for (int i = 0; i < n; i++) {
            const bool target = gain_k[i] > 0.0, cap = ceiling[i] != 0;
            if ((group == 0 && !(target && !cap)) || (group == 1 && !(target && cap)) || (group == 2 && !(!target && cap))) continue;
            const long long t = target ? std::max<long long>(((long long)max_len[i] + kLdTile - 1) / kLdTile, 1) : 0;
            const long long lt = std::max<long long>(((long long)max_len[i] + kLmTile - 1) / kLmTile, 1);
            h.push_back(LdReq{in_off[i], target ? gain_k[i] : 0.0, max_len[i], i, (int)tiles, (int)t, (int)ltiles, (int)lt, ceiling[i]});
            tiles += t;
            ltiles += lt;
        }
        if (group == 0) { plain = (int)h.size(); plain_ltiles = ltiles; }
        if (group == 1) metered = (int)h.size();
    }
    LmWorkspace* const wsp = device_workspace<LmWorkspace>("wave_loudness_limit");
    if (!wsp) return -6;
    LmWorkspace& ws = *wsp;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(dev_reserve(&ws.reqs, &ws.cap_reqs, h.size(), "wave_loudness_limit requests"));
    CK(dev_reserve(&ws.sub, &ws.cap_sub, (size_t)(2 * tiles) + 1, "wave_loudness_limit sub-block sums"));
    CK(dev_reserve(&ws.peaks, &ws.cap_peaks, (size_t)tiles + 1, "wave_loudness_limit peaks"));
    CK(dev_reserve(&ws.rws, &ws.cap_rws, (size_t)ltiles * kLmTile, "wave_loudness_limit reductions"));
    CK(dev_reserve(&ws.flags, &ws.cap_flags, (size_t)ltiles, "wave_loudness_limit tile flags"));
    CK(ws.stage.upload(ws.reqs, h.data(), sizeof(LdReq) * h.size(), st));   // pinned staging, queued on `stream`: no wait
    const int nf = (int)h.size();
    int launches = 2;
    if (metered) {
        hipLaunchKernelGGL(wave_kweight_kernel, dim3((unsigned)tiles), dim3(kLdThreads), 0, st, ws.reqs, metered, (const short*)pcm_dev, (const int*)len_dev,
                           ws.sub, ws.peaks);
        CKL("wave_kweight");
        hipLaunchKernelGGL(wave_gate_kernel, dim3((unsigned)metered), dim3(256), 0, st, ws.reqs, (const int*)len_dev, ws.sub, ws.peaks,
                           (long long*)stats_dev);
        CKL("wave_gate");
        launches = 4;
    }
    hipLaunchKernelGGL(wave_truepeak_kernel, dim3((unsigned)(ltiles - plain_ltiles)), dim3(256), 0, st, ws.reqs, nf, (int)plain_ltiles,
                       (const short*)pcm_dev, (const int*)len_dev, (const long long*)stats_dev, ws.rws, ws.flags);
    CKL("wave_truepeak");
    hipLaunchKernelGGL(wave_limit_apply_kernel, dim3((unsigned)ltiles), dim3(256), 0, st, ws.reqs, nf, (short*)pcm_dev, (const int*)len_dev,
                       (const long long*)stats_dev, (const int*)ws.rws, (const int*)ws.flags);
    CKL("wave_limit_apply");
    g_counters[CNT_WAVE_LIMIT_LAUNCHES] += launches;
    g_counters[CNT_WAVE_LIMIT_REQUESTS] += nf - plain;
    g_counters[CNT_WAVE_LOUDNESS_REQUESTS] += plain;
    return 0;
}
