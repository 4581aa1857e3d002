// Waveform back-end on the device: the tail of infer_batch_process (F/infer/utils_infer.py:485-519, the cross-fade join) and
// remove_silence_for_generated_wav (:530-539) for n requests in ONE call -- chunk waves in, each request's finished 16-bit PCM out.
// Included at the end of f5hip.hip (same translation unit).  A memory-bound gather: no MFMA, no atomics.
//
//   wave_join_kernel      one block per 3840-sample tile (16 cells of 10 ms) of a request's joined wave; a thread owns 8 consecutive samples:
//                         two 16-byte loads where they lie in one chunk's body and the address allows, one 16-byte store.  A sample of a
//                         fade region is prev[len - F + i] * ramp[F - 1 - i] + next[i] * ramp[i] in fp64, two products and a sum that are
//                         NOT contracted (numpy rounds each; `#pragma clang fp contract(off)`), rounded to fp32; then rint(x * 32768) clipped.  For a request that asked for
//                         silence removal the PCM goes to a scratch buffer and the block also leaves the sum of squares of each of its cells.
//   wave_silence_kernel   one block per flagged request: pydub's detect_silence / detect_nonsilent / split_on_silence (audio_prep.py) with
//                         min_silence_len 1000, silence_thresh -50, keep_silence 500, seek_step 10 on integers -> the kept sample ranges
//   wave_compact_kernel   copies the kept ranges of the scratch PCM to the output
// One launch when no request is flagged, else three, whatever n and the chunk counts.  A request's bits depend on that request alone.
//   wave_encode_kernel    (f5hip_wave_encode) the finished 24 kHz PCM of n requests -> another sample rate and G.711: the resampler of resample.h
//                         run in the other direction on integers, with an encoder behind it.  One block per tile of `tq` polyphase blocks of a
//                         request: the int16 window and -- when it fits -- the tap table in LDS, one thread per output summing
//                         taps[p][k] * xpad[q * of + k] in fp64, k ascending, then rint (half to even), clip, encode; the tile's bytes are
//                         packed in LDS and leave in 16-byte stores.  One launch whatever n.
//
// Exactness.  With every chunk at least 2 F samples long the nested fades of cross_fade_concat never overlap, so joined sample j is either one
// chunk sample or one fade of two chunk samples, and the closed form above is the host's arithmetic operation for operation (ramp[i] =
// i * (1.0 / (F - 1)), ramp[F - 1] = 1.0: np.linspace(0, 1, F)).  The silence test rms <= 10^(-50/20) * 32768 = 103.6 with rms =
// int(sqrt(S / n)) is S < 104^2 n = 10816 n on the integer sum of squares S (n <= 24000: S / n cannot round up across 10816).
// Segments (f5hip_wave_finish_joins: a multi-voice script).  Each chunk carries its own fade-in, F or 0: a chunk with 0 butts against the one
// before it, which is np.concatenate of the cross_fade_concat of each run of fading chunks (infer.join_segments).  The closed form holds where
// every chunk is at least as long as the fades it takes part in (F in, if it fades in, plus F out, if its successor does): then each
// _cross_fade takes n = F on samples no earlier fade touched.  Butt-joined chunks may be a single sample long (a gap is a chunk of zeros), so
// an 8-sample group can span several chunks and the slow path walks them.
#pragma once
#include "ragged_util.h"

struct WfChunk {
    const float* x;
    int len, pos;        // samples; first joined sample the chunk covers (its fade-in included)
    int fade;            // its fade-in: F where it cross-fades into the chunk before it, 0 where it butts against it (and for a first chunk)
};
struct WfReq {
    int chunk0, k;       // its chunks
    int n;               // joined samples
    int flag;            // silence removal
    long long off;       // its first sample in the output (a multiple of 8: 16-byte stores)
    long long joff;      // flagged: its first sample in the scratch PCM
    long long cell0;     // flagged: its first cell sum
    long long cnt0;      // flagged: its silent-window prefix counts
    int bucket0, range0; // flagged: its bucket and range slots
    int tile0;           // its first block of the join launch
    int pad;
};
struct WfFlagged { int req, tile0; };           // a flagged request and its first block of the compaction launch
struct WfRange { int sa, sb, dst; };            // kept samples [sa, sb) of the joined PCM go to dst ..

constexpr int kWfCell = 240;                    // 10 ms at 24 kHz
constexpr int kWfTile = 16 * kWfCell;           // joined samples per join block
constexpr int kWfGroups = kWfTile / 8;          // 8-sample groups per tile, 30 per cell
constexpr int kWfCompactTile = 4096;
constexpr int kWfWindowCells = 100;             // min_silence_len / seek_step
constexpr long long kWfLoud = 104 * 104;        // S >= 10816 n: rms >= 104 > 103.6

F5_DEVICE double wf_ramp(int i, int F, double step) {
#pragma clang fp contract(off)
    return i == F - 1 ? (F > 1 ? 1.0 : 0.0) : (double)i * step;
}

// joined sample j of a request, c its chunk (the last one whose pos <= j)
F5_DEVICE float wf_sample(const WfChunk* __restrict__ ch, int c, int F, double step, int j) {
    // numpy rounds both products and the sum, so nothing here may become an FMA.  Plain * and + under this pragma: hipcc's __dmul_rn and
    // __dadd_rn are inline `x * y` / `x + y` compiled with contraction allowed, and were fused into v_fmac_f64 once inlined.
#pragma clang fp contract(off)
    const WfChunk cur = ch[c];
    const int i = j - cur.pos;
    if (i < cur.fade) {   // (a request's first chunk has none)
        const WfChunk prev = ch[c - 1];
        const double a = (double)prev.x[prev.len - F + i] * wf_ramp(F - 1 - i, F, step);
        const double b = (double)cur.x[i] * wf_ramp(i, F, step);
        return (float)(a + b);
    }
    return cur.x[i];
}

F5_DEVICE int wf_quantise(float v) {   // serve.pcm16: rint(x * 32768) (exact product, half to even), clipped
    const double r = rint((double)v * 32768.0);
    return (int)fmax(fmin(r, 32767.0), -32768.0);
}

__global__ __launch_bounds__(256) void wave_join_kernel(const WfReq* __restrict__ reqs, int n, const WfChunk* __restrict__ chunks, int F, double step,
                                                        short* __restrict__ out, short* __restrict__ joined, long long* __restrict__ cells,
                                                        int* __restrict__ out_len) {
    __shared__ long long part[kWfGroups];
    const int tid = threadIdx.x;
    const int r = last_at_or_before<&WfReq::tile0>(reqs, n, (int)blockIdx.x);
    const WfReq q = reqs[r];
    const int tile = blockIdx.x - q.tile0;
    const WfChunk* ch = chunks + q.chunk0;
    short* dst = q.flag ? joined + q.joff : out + q.off;
    if (tile == 0 && tid == 0 && !q.flag) out_len[r] = q.n;
    for (int g = tid; g < kWfGroups; g += 256) {
        const long long j = (long long)tile * kWfTile + 8 * g;   // (64-bit: the last tile of a request near 2^31 samples ends past INT_MAX)
        long long ss = 0;
        if (j < q.n) {
            int c = last_at_or_before<&WfChunk::pos>(ch, q.k, j);
            const WfChunk cur = ch[c];
            const int i = (int)j - cur.pos;
            const long long body_end = c + 1 < q.k ? ch[c + 1].pos : q.n;   // one past the last joined sample that is this chunk's alone
            int v[8];   // the 8 quantised samples (a sample past the end is 0)
            if (i >= cur.fade && j + 8 <= body_end) {
                const float* p = cur.x + i;
                float f[8];
                if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                    const float4 lo = reinterpret_cast<const float4*>(p)[0], hi4 = reinterpret_cast<const float4*>(p)[1];
                    f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w; f[4] = hi4.x; f[5] = hi4.y; f[6] = hi4.z; f[7] = hi4.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; e++) f[e] = p[e];
                }
#pragma unroll
                for (int e = 0; e < 8; e++) v[e] = wf_quantise(f[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    v[e] = 0;
                    if (j + e < q.n) {
                        while (c + 1 < q.k && ch[c + 1].pos <= j + e) c++;   // (butt-joined chunks may be shorter than the group: several steps)
                        v[e] = wf_quantise(wf_sample(ch, c, F, step, (int)(j + e)));
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 8; e++) ss += (long long)(v[e] * v[e]);
            if (j + 8 <= q.n) {
                int4 w;
                w.x = (v[0] & 0xffff) | (v[1] << 16); w.y = (v[2] & 0xffff) | (v[3] << 16);
                w.z = (v[4] & 0xffff) | (v[5] << 16); w.w = (v[6] & 0xffff) | (v[7] << 16);
                *reinterpret_cast<int4*>(dst + j) = w;
            } else {
#pragma unroll
                for (int e = 0; e < 8; e++)
                    if (j + e < q.n) dst[j + e] = (short)v[e];
            }
        }
        part[g] = ss;
    }
    if (!q.flag) return;
    __syncthreads();
    const long long ci = (long long)tile * (kWfTile / kWfCell) + tid;   // cell of the request
    if (tid < kWfTile / kWfCell && ci * kWfCell < q.n) {
        long long s = 0;
        for (int e = 0; e < kWfCell / 8; e++) s += part[tid * (kWfCell / 8) + e];
        cells[q.cell0 + ci] = s;
    }
}

__global__ __launch_bounds__(256) void wave_silence_kernel(const WfReq* __restrict__ reqs, const WfFlagged* __restrict__ flagged,
                                                           const short* __restrict__ joined, const long long* __restrict__ cells, int* __restrict__ cnt,
                                                           int2* __restrict__ buckets, WfRange* __restrict__ ranges, int* __restrict__ nranges,
                                                           int* __restrict__ out_len) {
    __shared__ long long red[256];
    __shared__ int runsum[256];
    const int tid = threadIdx.x;
    const int r = flagged[blockIdx.x].req;
    const WfReq q = reqs[r];
    const int N = q.n;
    // len(seg) = round(1000 N / 24000), Python's round: half to even
    const int whole = N / 24, rem = N % 24;
    const int len_ms = whole + ((rem > 12 || (rem == 12 && (whole & 1))) ? 1 : 0);
    const int keep_end = (int)min(24LL * len_ms, (long long)N);   // where millisecond slicing ends the wave
    WfRange* rg = ranges + q.range0;
    if (len_ms < 1000) {   // shorter than one window: nothing is silent
        if (tid == 0) { rg[0] = WfRange{0, keep_end, 0}; nranges[r] = 1; out_len[r] = keep_end; }
        return;
    }
    const int last = len_ms - 1000, A = last / 10 + 1, nc = (N + kWfCell - 1) / kWfCell;
    const long long* cell = cells + q.cell0;
    int* pc = cnt + q.cnt0;   // pc[i] = silent windows among the aligned windows 0 .. i - 1 (A + 1 entries)

    // aligned window i starts at 10 i ms = cell i and covers cells [i, i + 100), cut at the wave's end; a thread slides over its run of windows
    const int run = (A + 255) / 256, i0 = min(tid * run, A), i1 = min(i0 + run, A);
    int local = 0;
    if (i0 < i1) {
        long long S = 0;
        for (int c = i0; c < min(i0 + kWfWindowCells, nc); c++) S += cell[c];
        for (int i = i0; i < i1; i++) {
            const long long nwin = min(24LL * (10 * i + 1000), (long long)N) - (long long)kWfCell * i;
            local += S < kWfLoud * nwin ? 1 : 0;
            pc[i + 1] = local;
            S -= cell[i];
            if (i + kWfWindowCells < nc) S += cell[i + kWfWindowCells];
        }
    }
    runsum[tid] = local;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int t = 0; t < 256; t++) { const int v = runsum[t]; runsum[t] = acc; acc += v; }
        pc[0] = 0;
    }
    __syncthreads();
    for (int i = i0; i < i1; i++) pc[i + 1] += runsum[tid];

    // the extra window at `last` when last % 10 != 0: it starts inside a cell, so it is summed from the samples
    const bool extra = last % 10 != 0;
    long long acc = 0;
    if (extra) {
        const short* x = joined + q.joff;
        for (long long s = 24LL * last + tid; s < keep_end; s += 256) acc += (long long)x[s] * x[s];
    }
    const long long extra_sum = block_sum(red, tid, acc);   // (its barriers also publish pc[])
    const bool extra_silent = extra && extra_sum < kWfLoud * (keep_end - 24LL * last);

    // detect_silence opens a new range at a silent start that is neither 10 ms nor at most 1000 ms behind the previous silent start: aligned
    // window i opens one iff none of the 100 windows before it is silent, and closes one iff none of the 100 after it is.  Range starts lie more
    // than 1000 ms apart, and so do range ends: a bucket of 100 windows holds at most one of each.
    const int nb = (A + kWfWindowCells - 1) / kWfWindowCells;
    int2* bk = buckets + q.bucket0;
    for (int b = tid; b < nb; b += 256) {
        int st = -1, en = -1;
        for (int i = kWfWindowCells * b; i < min(kWfWindowCells * (b + 1), A); i++) {
            if (pc[i + 1] == pc[i]) continue;
            if (pc[i] == pc[max(i - kWfWindowCells, 0)]) st = i;
            if (pc[min(i + kWfWindowCells + 1, A)] == pc[i + 1]) en = i;
        }
        bk[b] = make_int2(st, en);
    }
    __syncthreads();
    if (tid != 0) return;

    // detect_nonsilent + split_on_silence over the (few) silent ranges, in order: the non-silent range [p, s] ms keeps the samples
    // [24 max(p - 500, 0), min(24 min(s + 500, len_ms), N)).  With keep_silence 500 and min_silence_len 1000 two padded ranges never overlap.
    int nr = 0, dst = 0, prev_end = 0;
    bool first = true;
    auto nonsilent = [&](int p, int s) {
        const bool empty_head = first && p == 0 && s == 0;   // detect_nonsilent drops a leading [0, 0]
        first = false;
        if (empty_head) return;
        const int a = max(p - 500, 0), b = min(s + 500, len_ms);
        const int sa = 24 * a, sb = (int)min(24LL * b, (long long)N);
        rg[nr++] = WfRange{sa, sb, dst};
        dst += sb - sa;
    };
    bool have = false;            // a silent range whose end the extra window may still move
    int ps = 0, pe = 0, pen = 0, cur = 0;
    for (int b = 0; b < nb; b++) {
        const int2 e = bk[b];
        if (e.x >= 0) cur = 10 * e.x;
        if (e.y >= 0) {
            if (have) { nonsilent(prev_end, ps); prev_end = pe; }
            have = true; ps = cur; pe = 10 * e.y + 1000; pen = e.y;
        }
    }
    if (extra_silent) {
        if (have && last <= 10 * pen + 1000) {
            pe = len_ms;                                   // it continues the last range
        } else {
            if (have) { nonsilent(prev_end, ps); prev_end = pe; }
            have = true; ps = last; pe = len_ms;
        }
    }
    if (have) { nonsilent(prev_end, ps); prev_end = pe; }
    if (!have || pe != len_ms) nonsilent(prev_end, len_ms);
    nranges[r] = nr;
    out_len[r] = dst;
}

__global__ __launch_bounds__(256) void wave_compact_kernel(const WfReq* __restrict__ reqs, const WfFlagged* __restrict__ flagged, int nflag,
                                                           const short* __restrict__ joined, const WfRange* __restrict__ ranges,
                                                           const int* __restrict__ nranges, short* __restrict__ out) {
    const int f = last_at_or_before<&WfFlagged::tile0>(flagged, nflag, (int)blockIdx.x);
    const int r = flagged[f].req;
    const WfReq q = reqs[r];
    const WfRange* rg = ranges + q.range0;
    const int nr = nranges[r];
    if (nr < 1) return;
    const short* src = joined + q.joff;
    short* dst = out + q.off;
    const long long x0 = (long long)(blockIdx.x - flagged[f].tile0) * kWfCompactTile;
    for (int m = 0; m < kWfCompactTile / 256; m++) {
        const long long x = x0 + m * 256 + threadIdx.x;
        if (x >= q.n) break;
        const WfRange k = rg[last_at_or_before<&WfRange::sa>(rg, nr, x)];
        if (x >= k.sa && x < k.sb) dst[k.dst + (int)x - k.sa] = src[x];
    }
}

struct WfWorkspace {
    WfReq* reqs = nullptr; size_t cap_reqs = 0;
    WfChunk* chunks = nullptr; size_t cap_chunks = 0;
    WfFlagged* flagged = nullptr; size_t cap_flagged = 0;
    short* joined = nullptr; size_t cap_joined = 0;
    long long* cells = nullptr; size_t cap_cells = 0;
    int* cnt = nullptr; size_t cap_cnt = 0;
    int2* buckets = nullptr; size_t cap_buckets = 0;
    WfRange* ranges = nullptr; size_t cap_ranges = 0;
    int* nranges = nullptr; size_t cap_nranges = 0;
};

int f5hip_wave_finish_joins(int32_t n, const int32_t* chunks_per_request, const float* const* chunk_dev, const int32_t* chunk_len, int32_t fade,
                            const uint8_t* chunk_fade, const uint8_t* remove_silence, int32_t sample_rate, int16_t* pcm_dev, int32_t* len_dev,
                            void* stream) {
    if (n < 1 || !chunks_per_request || !chunk_dev || !chunk_len || !pcm_dev || !len_dev) return fail(-1, "wave_finish: bad argument");
    if (sample_rate != 24000) return fail(-1, "wave_finish: the sample rate must be 24000 (got %d)", sample_rate);
    if (fade < 0) return fail(-1, "wave_finish: the fade length must not be negative (got %d)", fade);
    if (reinterpret_cast<uintptr_t>(pcm_dev) & 15) return fail(-1, "wave_finish: the output must be 16-byte aligned");
    const int F = fade;
    std::vector<WfReq> h(n);
    std::vector<WfChunk> hc;
    std::vector<WfFlagged> hf;
    long long off = 0, joff = 0, ncell = 0, ncnt = 0, nbucket = 0, nrange = 0, tiles = 0, ctiles = 0, total_in = 0;
    for (int i = 0; i < n; i++) {
        const int k = chunks_per_request[i];
        if (k < 1) return fail(-1, "wave_finish: request %d has %d chunks", i, k);
        WfReq& q = h[i];
        memset(&q, 0, sizeof(q));
        q.chunk0 = (int)hc.size(); q.k = k;
        long long pos = 0;
        for (int c = 0; c < k; c++) {
            const size_t ci = hc.size();
            const int len = chunk_len[ci];
            if (!chunk_dev[ci] || len < 1) return fail(-1, "wave_finish: chunk %d of request %d is empty", c, i);
            // without chunk_fade every join fades; with it chunk c fades into its predecessor where chunk_fade[c] is set, else butts against it
            const int fin = c > 0 && (!chunk_fade || chunk_fade[ci]) ? F : 0;
            const int fout = c + 1 < k && (!chunk_fade || chunk_fade[ci + 1]) ? F : 0;
            if (!chunk_fade && k > 1 && F > 0 && len < 2 * (long long)F)
                return fail(-1, "wave_finish: chunk %d of request %d has %d samples, fewer than 2 x fade = %lld: its fades would overlap", c, i, len,
                            2 * (long long)F);
            if (len < (long long)fin + fout)
                return fail(-1, "wave_finish: chunk %d of request %d has %d samples, fewer than its fades (%d in, %d out): they would overlap", c, i,
                            len, fin, fout);
            if (reinterpret_cast<uintptr_t>(chunk_dev[ci]) & 3) return fail(-1, "wave_finish: chunk %d of request %d is not 4-byte aligned", c, i);
            pos -= fin;   // (pos never decreases along a request: len >= fin + fout; where two chunks share one, the later owns the sample)
            total_in += len;
            if (total_in > 2147483647LL) return fail(-1, "wave_finish: the chunks of the call exceed 2^31 - 1 samples");
            hc.push_back(WfChunk{chunk_dev[ci], len, (int)pos, fin});
            pos += len;
        }
        q.n = (int)pos;   // (<= total_in)
        q.flag = remove_silence && remove_silence[i] ? 1 : 0;
        q.off = off; q.tile0 = (int)tiles;
        off += (pos + 7) & ~7LL;
        tiles += (pos + kWfTile - 1) / kWfTile;
        if (off > 2147483647LL) return fail(-1, "wave_finish: the outputs of the call exceed 2^31 - 1 samples");
        if (q.flag) {
            q.joff = joff; q.cell0 = ncell; q.cnt0 = ncnt; q.bucket0 = (int)nbucket; q.range0 = (int)nrange;
            hf.push_back(WfFlagged{i, (int)ctiles});
            joff += (pos + 7) & ~7LL;
            ncell += (pos + kWfCell - 1) / kWfCell;
            ncnt += pos / kWfCell + 2;       // aligned windows + 1
            nbucket += pos / 24000 + 2;
            nrange += pos / 24000 + 4;       // silent ranges start more than 1000 ms apart; one kept range more than silent ones
            ctiles += (pos + kWfCompactTile - 1) / kWfCompactTile;
        }
    }
    WfWorkspace* const wsp = device_workspace<WfWorkspace>("wave_finish");
    if (!wsp) return -6;
    WfWorkspace& ws = *wsp;
    CK(dev_reserve(&ws.reqs, &ws.cap_reqs, (size_t)n, "wave_finish requests"));
    CK(dev_reserve(&ws.chunks, &ws.cap_chunks, hc.size(), "wave_finish chunks"));
    if (!hf.empty()) {
        CK(dev_reserve(&ws.flagged, &ws.cap_flagged, hf.size(), "wave_finish flags"));
        CK(dev_reserve(&ws.joined, &ws.cap_joined, (size_t)joff, "wave_finish joined PCM"));
        CK(dev_reserve(&ws.cells, &ws.cap_cells, (size_t)ncell, "wave_finish cells"));
        CK(dev_reserve(&ws.cnt, &ws.cap_cnt, (size_t)ncnt, "wave_finish window counts"));
        CK(dev_reserve(&ws.buckets, &ws.cap_buckets, (size_t)nbucket, "wave_finish buckets"));
        CK(dev_reserve(&ws.ranges, &ws.cap_ranges, (size_t)nrange, "wave_finish ranges"));
        CK(dev_reserve(&ws.nranges, &ws.cap_nranges, (size_t)n, "wave_finish range counts"));
    }
    hipStream_t st = (hipStream_t)stream;
    const hipError_t up = hf.empty() ? upload_sync(st, ws.reqs, h, ws.chunks, hc) : upload_sync(st, ws.reqs, h, ws.chunks, hc, ws.flagged, hf);
    if (up != hipSuccess) return fail(-6, "wave_finish metadata upload");

    const double step = F > 1 ? 1.0 / (double)(F - 1) : 0.0;   // np.linspace's step
    hipLaunchKernelGGL(wave_join_kernel, dim3((unsigned)tiles), dim3(256), 0, st, ws.reqs, n, ws.chunks, F, step, (short*)pcm_dev, ws.joined, ws.cells,
                       (int*)len_dev);
    CKL("wave_join");
    g_counters[CNT_WAVE_LAUNCHES]++;
    if (!hf.empty()) {
        hipLaunchKernelGGL(wave_silence_kernel, dim3((unsigned)hf.size()), dim3(256), 0, st, ws.reqs, ws.flagged, ws.joined, ws.cells, ws.cnt, ws.buckets,
                           ws.ranges, ws.nranges, (int*)len_dev);
        CKL("wave_silence");
        hipLaunchKernelGGL(wave_compact_kernel, dim3((unsigned)ctiles), dim3(256), 0, st, ws.reqs, ws.flagged, (int)hf.size(), ws.joined, ws.ranges,
                           ws.nranges, (short*)pcm_dev);
        CKL("wave_compact");
        g_counters[CNT_WAVE_LAUNCHES] += 2;
    }
    g_counters[CNT_WAVE_REQUESTS] += n;
    return 0;
}

int f5hip_wave_finish(int32_t n, const int32_t* chunks_per_request, const float* const* chunk_dev, const int32_t* chunk_len, int32_t fade,
                      const uint8_t* remove_silence, int32_t sample_rate, int16_t* pcm_dev, int32_t* len_dev, void* stream) {
    return f5hip_wave_finish_joins(n, chunks_per_request, chunk_dev, chunk_len, fade, nullptr, remove_silence, sample_rate, pcm_dev, len_dev, stream);
}

// ------------------------------------------------------------------------------------------------ delivery format: sample rate and G.711
// Output j = q nf + p of a request is rint(sum_k (double)taps[p][k] * (double)xpad[q of + k]), k ascending, clipped to int16: xpad = its samples
// with `width` zeros in front and zeros behind (an index predicate against the request's own length, never a read of its neighbour).  The
// samples are integers and the taps fp32, so every product is exact in fp64 and an fma gives the bits of a multiply followed by an add:
// infer.resample_pcm16 (numpy) is this arithmetic operation for operation.  The encoders are CPython's audioop.lin2ulaw / lin2alaw at width 2.
struct WeReq {
    long long in_off;    // its first sample, relative to pcm_dev
    long long out_off;   // its first output byte (a multiple of 16: 16-byte stores)
    int cap;             // upper bound of its length (the length itself without len_dev)
    int tile0;           // its first block
};

constexpr int kWeTileOutputs = 4096;            // outputs a block aims for; a tile holds a multiple of 16 outputs, so it starts on a 16-byte boundary
constexpr int kWeEncodings = 3;                 // 0 pcm16, 1 mu-law, 2 A-law

F5_DEVICE int we_ilog2(int m) { return 31 - __clz(m); }   // floor(log2 m), m >= 1

F5_DEVICE int we_mulaw(int s) {   // audioop.lin2ulaw: 14-bit magnitude, clipped where the bias would leave the last segment, bias 0x21
    const int x = s >> 2, sign = x < 0 ? 0x7F : 0xFF;
    const int m = min(abs(x), 8158) + 0x21, seg = we_ilog2(m) - 5;
    return ((seg << 4) | ((m >> (seg + 1)) & 15)) ^ sign;
}

F5_DEVICE int we_alaw(int s) {    // audioop.lin2alaw: 13-bit, a negative value as -x - 1
    const int x = s >> 3, mask = x >= 0 ? 0xD5 : 0x55;
    const int m = x >= 0 ? x : -x - 1, seg = max(we_ilog2(max(m, 1)) - 4, 0);
    return ((seg << 4) | ((m >> (seg < 2 ? 1 : seg)) & 15)) ^ mask;
}

// RESAMPLE: the tap table staged in LDS (every rate the entry point accepts: a table that does not fit is refused); else new_freq == 24000
// (no taps: the samples themselves)
template <bool RESAMPLE>
__global__ __launch_bounds__(256) void wave_encode_kernel(const WeReq* __restrict__ reqs, int n, const short* __restrict__ pcm,
                                                          const int* __restrict__ len_dev, const float* __restrict__ taps, int of, int nf, int width,
                                                          int L, int tq, int enc, unsigned char* __restrict__ out, int* __restrict__ out_len) {
    extern __shared__ __attribute__((aligned(16))) char we_sm[];
    const int tid = threadIdx.x;
    const int r = last_at_or_before<&WeReq::tile0>(reqs, n, (int)blockIdx.x);
    const WeReq q = reqs[r];
    const int tile = blockIdx.x - q.tile0;
    const int len = len_dev ? min(max(len_dev[r], 0), q.cap) : q.cap;   // (never past what the host sized the buffers for)
    const long long n_out = ((long long)nf * len + of - 1) / of;
    if (tile == 0 && tid == 0) out_len[r] = (int)n_out;
    const int n_local = tq * nf;                                        // outputs of a full tile
    const long long j0 = (long long)tile * n_local;
    if (j0 >= n_out) return;                                            // a tile past the request's actual length (the whole block leaves)

    const int nx = tq * of + 2 * width;                                 // the window of xpad this tile reads: xpad[q0 * of .. q0 * of + nx)
    short* xs = reinterpret_cast<short*>(we_sm);
    unsigned char* ys = reinterpret_cast<unsigned char*>(we_sm + ((2 * nx + 15) & ~15));        // the tile's output bytes
    float* tp = reinterpret_cast<float*>(ys + 2 * n_local);            // (n_local is a multiple of 16: 16-byte aligned)
    const short* x = pcm + q.in_off;
    const long long src0 = (long long)tile * tq * of - width;
    for (int i = tid; i < nx; i += 256) {
        const long long src = src0 + i;
        xs[i] = src >= 0 && src < len ? x[src] : (short)0;
    }
    if (RESAMPLE) stage_taps(tp, taps, nf * L, tid);
    __syncthreads();

    const int valid = (int)min((long long)n_local, n_out - j0);         // outputs of this tile
    for (int jl = tid; jl < valid; jl += 256) {
        int v;
        if (!RESAMPLE) {
            v = xs[jl];
        } else {
            const int ql = jl / nf, p = jl - ql * nf;
            const float* t = tp + p * L;
            const short* xq = xs + ql * of;
            double acc = 0.0;
            for (int k = 0; k < L; k++) acc = fma((double)t[k], (double)xq[k], acc);
            v = (int)fmax(fmin(rint(acc), 32767.0), -32768.0);
        }
        if (enc == 0) reinterpret_cast<short*>(ys)[jl] = (short)v;
        else ys[jl] = (unsigned char)(enc == 1 ? we_mulaw(v) : we_alaw(v));
    }
    __syncthreads();

    const int bps = enc == 0 ? 2 : 1, nbytes = valid * bps;
    unsigned char* dst = out + q.out_off + j0 * bps;                    // (16-byte aligned: out_off and j0 are multiples of 16)
    for (int b = 16 * tid; b < nbytes; b += 16 * 256) {
        if (b + 16 <= nbytes) {
            *reinterpret_cast<int4*>(dst + b) = *reinterpret_cast<const int4*>(ys + b);
        } else {
            for (int e = b; e < nbytes; e++) dst[e] = ys[e];            // the ragged end of the request
        }
    }
}

struct WeWorkspace { WeReq* reqs = nullptr; size_t cap_reqs = 0; };

// (tq, LDS bytes) of a rate pair; tq = 0: window, output tile and tap table do not fit the LDS together
struct WeTile { int tq, lds; };
static WeTile we_tile(const RatePair& rp) {
    const int unit = 16 / rate_gcd(rp.nf, 16);                           // tq * nf must be a multiple of 16
    const long long tq = ((kWeTileOutputs + (long long)rp.nf - 1) / rp.nf + unit - 1) / unit * unit;
    const long long base = ((2 * (tq * rp.of + 2 * rp.width) + 15) & ~15LL) + 2 * tq * rp.nf, table = 4LL * rp.nf * rp.L;
    if (base + table > kLdsMax) return WeTile{0, 0};
    return WeTile{(int)tq, (int)(base + table)};
}

int f5hip_wave_encode_tile(int32_t new_freq) {
    if (new_freq < 1) return 0;
    const RatePair rp = rate_pair(24000, new_freq);
    return we_tile(rp).tq * rp.of;
}

int f5hip_wave_encode(int32_t n, const int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev, int32_t new_freq,
                      int32_t encoding, const float* taps_dev, uint8_t* out_dev, const int64_t* out_off, int32_t* out_len_dev, void* stream) {
    if (n < 1 || !pcm_dev || !in_off || !max_len || !out_dev || !out_off || !out_len_dev) return fail(-1, "wave_encode: bad argument");
    if (encoding < 0 || encoding >= kWeEncodings) return fail(-1, "wave_encode: unknown encoding %d (0 pcm16, 1 mu-law, 2 A-law)", encoding);
    if (new_freq < 1) return fail(-1, "wave_encode: the sample rate must be positive (got %d)", new_freq);
    const bool identity = new_freq == 24000;
    if (!identity && !taps_dev) return fail(-1, "wave_encode: 24000 -> %d Hz needs the tap table", new_freq);
    if ((reinterpret_cast<uintptr_t>(pcm_dev) & 1) || (reinterpret_cast<uintptr_t>(out_dev) & 15))
        return fail(-1, "wave_encode: the input must be 2-byte aligned and the output 16-byte aligned");
    const RatePair rp = rate_pair(24000, new_freq);
    const WeTile t = we_tile(rp);
    if (!t.tq) return fail(-1, "wave_encode: 24000 -> %d Hz is not supported (%d : %d: its tap table does not fit the LDS)", new_freq, rp.of, rp.nf);
    std::vector<WeReq> h(n);
    long long total_in = 0, total_out = 0, tiles = 0;
    for (int i = 0; i < n; i++) {
        if (max_len[i] < 0) return fail(-1, "wave_encode: request %d has a negative length bound (%d)", i, max_len[i]);
        if (out_off[i] < 0 || (out_off[i] & 15)) return fail(-1, "wave_encode: the output offset of request %d is not a multiple of 16 bytes", i);
        const long long n_out = ((long long)rp.nf * max_len[i] + rp.of - 1) / rp.of, nq = (n_out + rp.nf - 1) / rp.nf;
        total_in += max_len[i]; total_out += n_out;
        if (total_in > 2147483647LL || total_out > 2147483647LL) return fail(-1, "wave_encode: the call exceeds 2^31 - 1 samples in or out");
        h[i] = WeReq{in_off[i], out_off[i], max_len[i], (int)tiles};
        tiles += std::max<long long>((nq + t.tq - 1) / t.tq, 1);      // (an empty request keeps one block: it writes its length)
    }
    WeWorkspace* const wsp = device_workspace<WeWorkspace>("wave_encode");
    if (!wsp) return -6;
    WeWorkspace& ws = *wsp;
    CK(dev_reserve(&ws.reqs, &ws.cap_reqs, (size_t)n, "wave_encode requests"));
    static unsigned lds_attr_done = 0;
    if (t.lds > 64 * 1024 && f5_set_lds_attr((const void*)wave_encode_kernel<true>, kLdsMax, lds_attr_done) != hipSuccess)
        return fail(-7, "wave_encode: LDS opt-in");
    hipStream_t st = (hipStream_t)stream;
    if (upload_sync(st, ws.reqs, h) != hipSuccess) return fail(-6, "wave_encode metadata upload");
#define F5_WE_LAUNCH(RESAMPLE)                                                                                                                 \
    hipLaunchKernelGGL(wave_encode_kernel<RESAMPLE>, dim3((unsigned)tiles), dim3(256), t.lds, st, ws.reqs, n, (const short*)pcm_dev, (const int*)len_dev, \
                       taps_dev, rp.of, rp.nf, rp.width, rp.L, t.tq, encoding, (unsigned char*)out_dev, (int*)out_len_dev)
    if (identity) F5_WE_LAUNCH(false);
    else F5_WE_LAUNCH(true);
#undef F5_WE_LAUNCH
    CKL("wave_encode");
    g_counters[CNT_WAVE_ENCODE_LAUNCHES]++;
    g_counters[CNT_WAVE_ENCODE_REQUESTS] += n;
    return 0;
}
