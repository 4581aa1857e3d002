// Waveform back-end on the device: the tail of infer_batch_process (F/infer/utils_infer.py:485-519, the cross-fade join) and
// remove_silence_for_generated_wav (:530-539) for n requests in ONE call -- chunk waves in, each request's finished 16-bit PCM out.
// Included at the end of f5hip.hip (same translation unit).  A memory-bound gather: no MFMA, no atomics (the FLAC encoder's LDS bit buffer excepted).
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
//   wave_flac_*_kernel    (f5hip_wave_flac) the int16 PCM of n requests at the delivery rate -> each request's native FLAC stream, three
//                         launches whatever n: see "delivery format: FLAC" below.
//   wave_kweight / wave_gate / wave_gain_kernel  (f5hip_wave_loudness) the finished 24 kHz PCM of the flagged requests, in place, to their
//                         BS.1770 loudness targets, three launches whatever n: see "loudness" below.
//   wave_wsola / wave_pitch_kernel  (f5hip_wave_prosody) the finished 24 kHz PCM of n requests -> each request's tempo and pitch (WSOLA, then
//                         a rational resampler), two launches whatever n, one without a pitch: see "prosody" below.
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
#include "wave_prosody_core.h"

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
    WorkspaceUse use;
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
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
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

// One tile of one request, by a block of 256 threads: the outputs j0 = tile * tq * nf .. of its n_out, from its samples x[0 .. len), to the bytes
// at dst (the request's first output byte).  What wave_encode_kernel (the pair and the table of the call) and wave_pitch_kernel (those of the
// request) share.  RESAMPLE: the tap table staged in LDS; else the samples themselves.  sm: tq * of + 2 * width shorts, 2 * tq * nf bytes and
// the table, in that order (we_tile).
template <bool RESAMPLE>
F5_DEVICE void we_tile_body(char* sm, const short* __restrict__ x, int len, long long n_out, int tile, const float* __restrict__ taps, int of, int nf,
                            int width, int L, int tq, int enc, unsigned char* __restrict__ dst) {
    const int tid = threadIdx.x;
    const int n_local = tq * nf;                                        // outputs of a full tile
    const long long j0 = (long long)tile * n_local;
    if (j0 >= n_out) return;                                            // a tile past the request's actual length (the whole block leaves)

    const int nx = tq * of + 2 * width;                                 // the window of xpad this tile reads: xpad[q0 * of .. q0 * of + nx)
    short* xs = reinterpret_cast<short*>(sm);
    unsigned char* ys = reinterpret_cast<unsigned char*>(sm + ((2 * nx + 15) & ~15));           // the tile's output bytes
    float* tp = reinterpret_cast<float*>(ys + 2 * n_local);            // (n_local is a multiple of 16: 16-byte aligned)
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
    unsigned char* out = dst + j0 * bps;                                // (16-byte aligned: the request's first byte and j0 are multiples of 16)
    for (int b = 16 * tid; b < nbytes; b += 16 * 256) {
        if (b + 16 <= nbytes) {
            *reinterpret_cast<int4*>(out + b) = *reinterpret_cast<const int4*>(ys + b);
        } else {
            for (int e = b; e < nbytes; e++) out[e] = ys[e];            // the ragged end of the request
        }
    }
}

// RESAMPLE: the tap table staged in LDS (every rate the entry point accepts: a table that does not fit is refused); else new_freq == 24000
// (no taps: the samples themselves)
template <bool RESAMPLE>
__global__ __launch_bounds__(256) void wave_encode_kernel(const WeReq* __restrict__ reqs, int n, const short* __restrict__ pcm,
                                                          const int* __restrict__ len_dev, const float* __restrict__ taps, int of, int nf, int width,
                                                          int L, int tq, int enc, unsigned char* __restrict__ out, int* __restrict__ out_len) {
    extern __shared__ __attribute__((aligned(16))) char we_sm[];
    const int r = last_at_or_before<&WeReq::tile0>(reqs, n, (int)blockIdx.x);
    const WeReq q = reqs[r];
    const int tile = blockIdx.x - q.tile0;
    const int len = len_dev ? min(max(len_dev[r], 0), q.cap) : q.cap;   // (never past what the host sized the buffers for)
    const long long n_out = ((long long)nf * len + of - 1) / of;
    if (tile == 0 && threadIdx.x == 0) out_len[r] = (int)n_out;
    we_tile_body<RESAMPLE>(we_sm, pcm + q.in_off, len, n_out, tile, taps, of, nf, width, L, tq, enc, out + q.out_off);
}

struct WeWorkspace { WeReq* reqs = nullptr; size_t cap_reqs = 0; WorkspaceUse use; };

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
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(dev_reserve(&ws.reqs, &ws.cap_reqs, (size_t)n, "wave_encode requests"));
    static unsigned lds_attr_done = 0;
    if (t.lds > 64 * 1024 && f5_set_lds_attr((const void*)wave_encode_kernel<true>, kLdsMax, lds_attr_done) != hipSuccess)
        return fail(-7, "wave_encode: LDS opt-in");
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

// ------------------------------------------------------------------------------------------------ delivery format: FLAC
// f5hip_wave_flac: the int16 PCM of n requests at the delivery rate -> each request's complete native FLAC stream (RFC 9639), byte for byte
// wave_codec.encode_flac (the subset and the choice rule are written down there and in include/f5hip.h).  Integer arithmetic only.
//   wave_flac_frame_kernel  one block per (request, frame of 4096) up to ceil(max_len / 4096); a block past the request's actual length
//                           leaves.  The block's samples go to LDS; a thread owns 16 consecutive samples, so the 16 threads of a quarter
//                           wave own one Rice partition of 256: the five residual sets are differenced in registers, and for each order the
//                           15 sums sum(u >> k) of a partition are one 16-lane butterfly each.  80 threads pick the parameter of one
//                           (order, partition) pair, every thread then picks the subframe by the rule.  The code lengths are prefix-summed
//                           over the block and each code goes into a zeroed LDS bit buffer with at most two LDS atomicOr: its unary zeros are
//                           there already, so a code is the one bit and the k low bits.  A chosen subframe is never larger than VERBATIM, so
//                           the buffer is sized for that.  CRC-8 by one lane (at most 10 bytes); CRC-16 by all 256: the frame right-aligned
//                           in 256 slices of 33 bytes (zeros in front change nothing with initial value 0), one slice per thread, then a
//                           binary tree a * x^(8 * 33 * 2^j) + b in GF(2)[x] mod 0x18005 -- CRC is linear, so slices combine.  The frame
//                           leaves in 16-byte stores for its slot of a fixed-stride scratch buffer, its size for `sizes`.
//   wave_flac_scan_kernel   one block per request: the exclusive scan of its frame sizes, their minimum and maximum; writes the 42-byte
//                           stream header (total samples, min / max frame size, MD5 zero) and the stream's length.
//   wave_flac_pack_kernel   one block per (request, frame): the frame from its slot to its place behind the header -- a byte-granular
//                           destination: bytes up to the first 4-byte boundary, 4-byte stores, bytes again.
// Three launches whatever n (one when every request is empty by its bound), no host sync between them; a request's bytes depend on that
// request alone.  Vector stores and LDS atomics in plain C++.
// f5hip_wave_flac_levels: the same with a FLAC level per request (wave_codec.encode_flac(x, rate, level)).  A call with a level-1 request
// launches wave_flac_frame_kernel<true>, in which the full blocks of such requests try four LPC candidates (flac_lpc_core.h) beside the five
// fixed orders; every other block of the call, and every call without a level-1 request (<false>: the level-0 code), is as above.  The
// level-0 candidates are a subset of the level-1 ones and VERBATIM still bounds the choice, so the size contract below holds unchanged.
#include "flac_lpc_core.h"

struct FlReq {
    long long in_off;    // its first sample, relative to pcm_dev
    long long out_off;   // its stream's first byte (a multiple of 16)
    int cap;             // upper bound of its length (the length itself without len_dev)
    int frame0;          // its first block of the frame and pack launches = its first scratch slot
    int level;           // 0: fixed predictors; 1: LPC subframes among the candidates of its full blocks (wave_flac_frame_kernel<true>)
    int pad;
};

constexpr int kFlBlock = 4096;
constexpr int kFlHeader = 42;
constexpr int kFlSlot = 8208;                   // bytes of a scratch slot: header 11 + VERBATIM 1 + 8192 + CRC-16 2 = 8206, up to 16
constexpr int kFlWords = kFlSlot / 4;
constexpr int kFlOrders = 5, kFlParams = 15, kFlParts = 16;
constexpr int kFlVerbatim = 5;                  // a block's kind: -1 CONSTANT, 0 .. 4 the fixed order, 5 VERBATIM, 6 + i LPC of order fl1_order(i)
constexpr int kFlSlice = 33;                    // CRC-16 slice of a thread: 256 * 33 >= 8204
// The size contract, in one place: a frame is at most 11 header bytes (2 sync, 2 codes, a frame number below 2^21 in 4, the 16-bit block
// size, CRC-8), a subframe that is at most VERBATIM (1 + 2 b bytes: the choice rule takes FIXED only when it is no larger) and 2 bytes of
// CRC-16, i.e. 2 b + 14.  So every bit position `fl_put` sees lies inside the slot, and a request's frames together stay inside
// f5hip_wave_flac_bound (2 bytes a sample + 16 a frame behind the header), by which the caller sized its part of the output.  The three
// range checks below (`fl_put`'s word index, the clamp of a frame's byte count, the pack kernel's end of the request's part) never fire
// under this contract and decide no byte of a stream; they stay as the backstop that keeps a broken contract -- a changed choice rule,
// a caller's wrong bound -- from writing outside the LDS buffer or the request's part of the output.
static_assert(11 + 1 + 2 * kFlBlock + 2 <= kFlSlot && kFlSlot % 16 == 0 && 256 * kFlSlice >= kFlSlot - 4, "wave_flac slot size");

__host__ __device__ constexpr unsigned fl_gf_mul(unsigned a, unsigned b) {   // a * b in GF(2)[x] mod x^16 + x^15 + x^2 + 1
    unsigned r = 0;
    for (int i = 15; i >= 0; i--) {
        r = ((r << 1) ^ ((r & 0x8000u) ? 0x8005u : 0u)) & 0xffffu;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
__host__ __device__ constexpr unsigned fl_x_pow(int bits) {                   // x^bits mod the polynomial
    unsigned r = 1;
    for (int i = 0; i < bits; i++) r = ((r << 1) ^ ((r & 0x8000u) ? 0x8005u : 0u)) & 0xffffu;
    return r;
}
__host__ __device__ constexpr unsigned fl_slice_pow(int level) {              // x^(8 * kFlSlice * 2^level)
    unsigned r = fl_x_pow(8 * kFlSlice);
    for (int i = 0; i < level; i++) r = fl_gf_mul(r, r);
    return r;
}

F5_DEVICE unsigned fl_crc16_byte(unsigned c, unsigned byte) {
    c ^= byte << 8;
#pragma unroll
    for (int i = 0; i < 8; i++) c = ((c << 1) ^ ((c & 0x8000u) ? 0x8005u : 0u)) & 0xffffu;
    return c;
}
F5_DEVICE unsigned fl_crc8_byte(unsigned c, unsigned byte) {
    c ^= byte;
#pragma unroll
    for (int i = 0; i < 8; i++) c = ((c << 1) ^ ((c & 0x80u) ? 0x07u : 0u)) & 0xffu;
    return c;
}

// nbits (1 .. 32) of v at bit `pos` of the bit buffer w: big-endian words, bit 0 the most significant of word 0; the buffer starts zeroed
F5_DEVICE void fl_put(unsigned* w, int pos, unsigned v, int nbits) {
    const int i = pos >> 5, sh = 32 - (pos & 31) - nbits;
    if (i < 0 || i >= kFlWords) return;
    if (sh >= 0) {
        atomicOr(&w[i], v << sh);
    } else {
        atomicOr(&w[i], v >> -sh);
        if (i + 1 < kFlWords) atomicOr(&w[i + 1], v << (32 + sh));
    }
}
F5_DEVICE unsigned fl_byte(const unsigned* w, int j) { return (w[j >> 2] >> (24 - 8 * (j & 3))) & 255u; }
F5_DEVICE int fl_len(const int* len_dev, int r, int cap) { return len_dev ? min(max(len_dev[r], 0), cap) : cap; }

// sum(u >> k) of a partition of 256 for every k: the thread's 16 codes, then one butterfly over the 16 threads that share the partition
F5_DEVICE void fl_partition_sums(const unsigned* u, int tid, unsigned (*sums)[kFlParts]) {
#pragma unroll
    for (int k = 0; k < kFlParams; k++) {
        unsigned s = 0;
#pragma unroll
        for (int e = 0; e < 16; e++) s += u[e] >> k;
        s += __shfl_xor(s, 8);
        s += __shfl_xor(s, 4);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 1);
        if ((tid & 15) == 0) sums[k][tid >> 4] = s;
    }
}

// the zigzag residuals of the thread's 16 samples under one LPC order: win[12 + e] is sample g0 + e, win[0 .. 11] the twelve before them
// (zeros in front of the block).  Always twelve taps: q is zero behind the order, so the sum is the order's own.
F5_DEVICE void fl_lpc_codes(const int* win, int g0, const Fl1Order& L, int order, unsigned* u) {
    int q[kFl1MaxOrder];
#pragma unroll
    for (int j = 0; j < kFl1MaxOrder; j++) q[j] = L.q[j];
    const int shift = L.shift;
#pragma unroll
    for (int e = 0; e < 16; e++) u[e] = g0 + e >= order ? fl1_residual(win + kFl1MaxOrder + e, q, kFl1MaxOrder, shift) : 0u;
}

// LPC = false is the level-0 encoder.  LPC = true adds, for the full blocks of a request at level 1, the four LPC candidates of
// flac_lpc_core.h: the windowed samples to LDS, the 13 lags per thread over its 16 samples and an int64 reduction over the block, steps 3 and 4
// on one lane, then per order the residuals (their maximum for the guard) and the same partition sums as a fixed order.
template <bool LPC>
__global__ __launch_bounds__(256) void wave_flac_frame_kernel(const FlReq* __restrict__ reqs, int n, const short* __restrict__ pcm,
                                                              const int* __restrict__ len_dev, int rate_code, unsigned* __restrict__ scratch,
                                                              int* __restrict__ sizes) {
    constexpr int kCands = LPC ? kFlOrders + kFl1Orders : kFlOrders;   // FIXED 0 .. 4, then LPC 6, 8, 10, 12
    __shared__ short xs[kFlBlock];
    __shared__ __attribute__((aligned(16))) unsigned bitw[kFlWords];
    __shared__ unsigned sums[kCands][kFlParams][kFlParts];   // sum(u >> k) of the 256 samples of a partition (u = 0 before the candidate's first residual)
    __shared__ unsigned best_s[kCands][kFlParts];
    __shared__ int best_k[kCands][kFlParts];
    __shared__ short xw[LPC ? kFlBlock : 1];                 // the windowed samples
    __shared__ unsigned long long lags[kFl1Lags];
    __shared__ Fl1Order lpc[kFl1Orders];
    __shared__ unsigned lpc_top[kFl1Orders];                 // the largest zigzag residual of an order, for the guard
    __shared__ int wave_total[4];
    __shared__ unsigned wave_crc[4];
    __shared__ int differs;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = last_at_or_before<&FlReq::frame0>(reqs, n, (int)blockIdx.x);
    const FlReq q = reqs[r];
    const int f = blockIdx.x - q.frame0;
    const int len = fl_len(len_dev, r, q.cap);
    const long long s0 = (long long)f * kFlBlock;
    if (s0 >= len) return;                                              // a frame past the request's actual length (the whole block leaves)
    const int b = (int)min((long long)kFlBlock, len - s0);
    const bool full = b == kFlBlock;
    const int parts = full ? kFlParts : 1, orders = min(kFlOrders, b);
    const bool lpc_on = LPC && full && q.level == 1;

    // the thread's 16 samples: two 16-byte loads where the address allows and the block has them all
    const short* x = pcm + q.in_off + s0;
    int h[20];                                                          // h[4 + e] = sample 16 tid + e; h[0 .. 3] the four before them
    const int g0 = 16 * tid;
    if (g0 + 16 <= b && (reinterpret_cast<uintptr_t>(x + g0) & 15) == 0) {
        const int4 lo = reinterpret_cast<const int4*>(x + g0)[0], hi = reinterpret_cast<const int4*>(x + g0)[1];
        const int w8[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int e = 0; e < 8; e++) { h[4 + 2 * e] = (short)(w8[e] & 0xffff); h[5 + 2 * e] = w8[e] >> 16; }
    } else {
#pragma unroll
        for (int e = 0; e < 16; e++) h[4 + e] = g0 + e < b ? (int)x[g0 + e] : 0;
    }
#pragma unroll
    for (int e = 0; e < 16; e++) xs[g0 + e] = (short)h[4 + e];
    for (int i = tid; i < kFlWords; i += 256) bitw[i] = 0;
    if (tid == 0) differs = 0;
    if constexpr (LPC) {
        if (lpc_on) {
#pragma unroll
            for (int e = 0; e < 16; e++) xw[g0 + e] = (short)fl1_windowed(h[4 + e], g0 + e);
            if (tid < kFl1Lags) lags[tid] = 0;
            if (tid < kFl1Orders) lpc_top[tid] = 0;
        }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; e++) h[e] = g0 + e - 4 >= 0 ? (int)xs[g0 + e - 4] : 0;
    {
        const int first = xs[0];
        bool any = false;
#pragma unroll
        for (int e = 0; e < 16; e++) any |= g0 + e < b && h[4 + e] != first;
        if (any) differs = 1;
    }

    // the five residual sets, one after the other: cur[j] is the order's difference at sample g0 - 4 + j, valid from j = order on
    {
        int cur[20];
#pragma unroll
        for (int j = 0; j < 20; j++) cur[j] = h[j];
#pragma unroll
        for (int o = 0; o < kFlOrders; o++) {
            if (o > 0) {
#pragma unroll
                for (int j = 19; j >= 1; j--) cur[j] -= cur[j - 1];
            }
            unsigned u[16];
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int g = g0 + e, res = cur[4 + e];
                u[e] = g >= o && g < b ? (unsigned)((res << 1) ^ (res >> 31)) : 0u;
            }
            fl_partition_sums(u, tid, sums[o]);
        }
    }

    // level 1: the LPC candidates of a full block
    int win[kFl1MaxOrder + 16];                                         // win[12 + e] = sample g0 + e (LPC only)
    if constexpr (LPC) {
        if (lpc_on) {
            {
                int ww[kFl1MaxOrder + 16];
#pragma unroll
                for (int j = 0; j < kFl1MaxOrder + 16; j++) {
                    const int g = g0 - kFl1MaxOrder + j;
                    win[j] = g >= 0 ? (int)xs[g] : 0;
                    ww[j] = g >= 0 ? (int)xw[g] : 0;
                }
#pragma unroll
                for (int j = 0; j < kFl1Lags; j++) {
                    long long s = 0;
#pragma unroll
                    for (int e = 0; e < 16; e++) s += (long long)(ww[kFl1MaxOrder + e] * ww[kFl1MaxOrder + e - j]);   // (a product stays below 2^30)
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
                    if (lane == 0) atomicAdd(&lags[j], (unsigned long long)s);   // (exact integers: any order of summation)
                }
            }
            __syncthreads();
            if (tid == 0) {
                long long R[kFl1Lags];
#pragma unroll
                for (int j = 0; j < kFl1Lags; j++) R[j] = (long long)lags[j];
                fl1_levinson(R, lpc);
            }
            __syncthreads();
            for (int c = 0; c < kFl1Orders; c++) {
                if (!lpc[c].valid) continue;
                unsigned u[16];
                fl_lpc_codes(win, g0, lpc[c], fl1_order(c), u);
                unsigned top = 0;
#pragma unroll
                for (int e = 0; e < 16; e++) top = max(top, u[e]);
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) top = max(top, (unsigned)__shfl_xor((int)top, d));
                if (lane == 0) atomicMax(&lpc_top[c], top);
                fl_partition_sums(u, tid, sums[kFlOrders + c]);
            }
        }
    }
    __syncthreads();

    // the Rice parameter of each (order, partition): the k that minimises S_k = sum(u >> k) + n (1 + k), ties to the smaller k
    if (tid < kCands * kFlParts) {
        const int o = tid >> 4, p = tid & 15;                             // o: the candidate's slot
        bool live = o < orders;
        int warm = o;                                                   // its warm-up samples
        if constexpr (LPC) {
            if (o >= kFlOrders) {
                live = lpc_on && lpc[o - kFlOrders].valid && lpc_top[o - kFlOrders] < kFl1Guard;
                warm = fl1_order(o - kFlOrders);
            }
        }
        if (live && p < parts) {
            const unsigned cnt = full ? 256u - (p == 0 ? warm : 0) : (unsigned)(b - o);
            unsigned bs = 0xffffffffu;
            int bk = 0;
            for (int k = 0; k < kFlParams; k++) {
                unsigned long long s = 0;
                if (full) s = sums[o][k][p];
                else for (int pp = 0; pp < kFlParts; pp++) s += sums[o][k][pp];
                s += (unsigned long long)cnt * (1 + k);
                if (s < bs) { bs = (unsigned)s; bk = k; }                 // (the minimum is far below 2^32: S_14 <= n (64 + 15))
            }
            best_s[o][p] = bs;
            best_k[o][p] = bk;
        }
    }
    __syncthreads();

    // the subframe: CONSTANT (-1) when all samples are equal, else the fixed order with the fewest bits (ties to the lower order), VERBATIM (5)
    // only when strictly smaller
    int kind = 0;
    long long best_bits = 0;
    for (int o = 0; o < orders; o++) {
        long long bits = 8 + 16 * o + 2 + 4;
        for (int p = 0; p < parts; p++) bits += 4 + (long long)best_s[o][p];
        if (o == 0 || bits < best_bits) { best_bits = bits; kind = o; }
    }
    if constexpr (LPC) {
        if (lpc_on) {
            for (int c = 0; c < kFl1Orders; c++) {
                if (!lpc[c].valid || lpc_top[c] >= kFl1Guard) continue;
                const int o = fl1_order(c);
                long long bits = 8 + 16 * o + 4 + 5 + kFl1Precision * o + 2 + 4;
                for (int p = 0; p < parts; p++) bits += 4 + (long long)best_s[kFlOrders + c][p];
                if (bits < best_bits) { best_bits = bits; kind = kFlVerbatim + 1 + c; }
            }
        }
    }
    if (8 + 16LL * b < best_bits) kind = kFlVerbatim;
    if (!differs) kind = -1;

    // the frame header: sync and fixed block size, block-size and rate codes, mono 16 bits, the frame number, b - 1 for a short block, CRC-8
    const int nb = f < 0x80 ? 1 : f < 0x800 ? 2 : f < 0x10000 ? 3 : 4;   // (f < 2^19: a call holds fewer than 2^31 samples)
    const int hlen = 4 + nb + (full ? 0 : 2) + 1;
    if (tid == 0) {
        unsigned char hd[11];
        int m = 0;
        hd[m++] = 0xff; hd[m++] = 0xf8; hd[m++] = (unsigned char)(((full ? 0x0c : 0x07) << 4) | rate_code); hd[m++] = 0x08;
        if (nb == 1) {
            hd[m++] = (unsigned char)f;
        } else {
            hd[m++] = (unsigned char)(((0xff << (8 - nb)) & 0xff) | (f >> (6 * (nb - 1))));
            for (int k = nb - 2; k >= 0; k--) hd[m++] = (unsigned char)(0x80 | ((f >> (6 * k)) & 0x3f));
        }
        if (!full) { hd[m++] = (unsigned char)((b - 1) >> 8); hd[m++] = (unsigned char)((b - 1) & 0xff); }
        unsigned c = 0;
        for (int i = 0; i < m; i++) c = fl_crc8_byte(c, hd[i]);
        hd[m++] = (unsigned char)c;
        for (int i = 0; i < m; i++) fl_put(bitw, 8 * i, hd[i], 8);
    }
    const int base0 = 8 * hlen;
    int nbits;
    if (kind == -1) {
        if (tid == 0) fl_put(bitw, base0 + 8, (unsigned)xs[0] & 0xffffu, 16);   // (the subframe header byte is 0)
        nbits = base0 + 24;
    } else if (kind == kFlVerbatim) {
        if (tid == 0) fl_put(bitw, base0, 0x02u, 8);
#pragma unroll
        for (int e = 0; e < 16; e++)
            if (g0 + e < b) fl_put(bitw, base0 + 8 + 16 * (g0 + e), (unsigned)h[4 + e] & 0xffffu, 16);
        nbits = base0 + 8 + 16 * b;
    } else {
        const bool is_lpc = LPC && kind > kFlVerbatim;
        const int slot = is_lpc ? kind - 1 : kind, o = is_lpc ? fl1_order(kind - kFlVerbatim - 1) : kind;
        const int extra = is_lpc ? 4 + 5 + kFl1Precision * o : 0;        // precision, shift and coefficients of an LPC subframe
        const int p = full ? tid >> 4 : 0, k = best_k[slot][p];
        unsigned u[16];
        if (is_lpc) {
            if constexpr (LPC) fl_lpc_codes(win, g0, lpc[slot - kFlOrders], o, u);
        } else {
            int cur[20];
#pragma unroll
            for (int j = 0; j < 20; j++) cur[j] = h[j];
#pragma unroll
            for (int d = 0; d < kFlOrders - 1; d++) {
                if (d < o) {
#pragma unroll
                    for (int j = 19; j >= 1; j--) cur[j] -= cur[j - 1];
                }
            }
#pragma unroll
            for (int e = 0; e < 16; e++) { const int res = cur[4 + e]; u[e] = (unsigned)((res << 1) ^ (res >> 31)); }
        }
        int mine = 0;                                                    // bits of the thread's codes
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int g = g0 + e;
            if (g >= o && g < b) mine += (int)(u[e] >> k) + 1 + k;
        }
        int incl = mine;                                                 // inclusive scan over the wave, then over the four waves
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_total[wv] = incl;
        __syncthreads();
        int before = incl - mine, total = 0;
        for (int w = 0; w < 4; w++) { if (w < wv) before += wave_total[w]; total += wave_total[w]; }
        const int base = base0 + 8 + 16 * o + extra + 6;                 // behind the subframe header, the warm-up, an LPC subframe's fields, coding method 00 and the partition order
        if (tid == 0) {
            fl_put(bitw, base0, (unsigned)((is_lpc ? 0x20 | (o - 1) : 8 | o) << 1), 8);
            for (int j = 0; j < o; j++) fl_put(bitw, base0 + 8 + 16 * j, (unsigned)xs[j] & 0xffffu, 16);
            if constexpr (LPC) {
                if (is_lpc) {
                    const int at = base0 + 8 + 16 * o;
                    fl_put(bitw, at, (unsigned)(kFl1Precision - 1), 4);
                    fl_put(bitw, at + 4, (unsigned)lpc[slot - kFlOrders].shift & 31u, 5);
                    for (int j = 0; j < o; j++)
                        fl_put(bitw, at + 9 + kFl1Precision * j, (unsigned)lpc[slot - kFlOrders].q[j] & ((1u << kFl1Precision) - 1u), kFl1Precision);
                }
            }
            if (full) fl_put(bitw, base - 4, 4u, 4);
        }
        if (full ? (tid & 15) == 0 : tid == 0) fl_put(bitw, base + 4 * p + before, (unsigned)k, 4);
        int pos = base + 4 * (p + 1) + before;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int g = g0 + e;
            if (g >= o && g < b) {
                const int quot = (int)(u[e] >> k);
                fl_put(bitw, pos + quot, (1u << k) | (u[e] & ((1u << k) - 1u)), k + 1);
                pos += quot + 1 + k;
            }
        }
        nbits = base + 4 * parts + total;
    }
    const int nbytes = min((nbits + 7) >> 3, kFlSlot - 2);              // (never more: a chosen subframe is at most VERBATIM)
    __syncthreads();

    // CRC-16 of the nbytes in front of it: the frame right-aligned in 256 slices, one per thread, combined by a fixed tree
    {
        const int pad = 256 * kFlSlice - nbytes;
        constexpr unsigned pw[8] = {fl_slice_pow(0), fl_slice_pow(1), fl_slice_pow(2), fl_slice_pow(3),
                                    fl_slice_pow(4), fl_slice_pow(5), fl_slice_pow(6), fl_slice_pow(7)};
        unsigned c = 0;
        for (int i = 0; i < kFlSlice; i++) {
            const int j = tid * kFlSlice + i - pad;
            if (j >= 0) c = fl_crc16_byte(c, fl_byte(bitw, j));
        }
#pragma unroll
        for (int level = 0; level < 6; level++) {
            const unsigned other = __shfl_down(c, 1 << level);
            if ((lane & ((2 << level) - 1)) == 0) c = fl_gf_mul(c, pw[level]) ^ other;
        }
        if (lane == 0) wave_crc[wv] = c;
        __syncthreads();
        if (tid == 0) {
            const unsigned a = fl_gf_mul(wave_crc[0], pw[6]) ^ wave_crc[1], bb = fl_gf_mul(wave_crc[2], pw[6]) ^ wave_crc[3];
            fl_put(bitw, 8 * nbytes, fl_gf_mul(a, pw[7]) ^ bb, 16);
        }
        __syncthreads();
    }

    const int total_bytes = nbytes + 2;
    uint4* dst = reinterpret_cast<uint4*>(scratch + (size_t)blockIdx.x * kFlWords);
    for (int i = tid; 16 * i < total_bytes; i += 256) {
        const uint4 v = reinterpret_cast<const uint4*>(bitw)[i];
        dst[i] = make_uint4(__builtin_bswap32(v.x), __builtin_bswap32(v.y), __builtin_bswap32(v.z), __builtin_bswap32(v.w));
    }
    if (tid == 0) sizes[blockIdx.x] = total_bytes;
}

__global__ __launch_bounds__(256) void wave_flac_scan_kernel(const FlReq* __restrict__ reqs, const int* __restrict__ len_dev,
                                                             const int* __restrict__ sizes, unsigned* __restrict__ frame_off, int rate,
                                                             unsigned char* __restrict__ out, int* __restrict__ out_len) {
    __shared__ unsigned runsum[256];
    __shared__ int runmin[256], runmax[256];
    const int tid = threadIdx.x, r = blockIdx.x;
    const FlReq q = reqs[r];
    const int len = fl_len(len_dev, r, q.cap);
    const int frames = (int)(((long long)len + kFlBlock - 1) / kFlBlock);
    const int run = (frames + 255) / 256, i0 = min(tid * run, frames), i1 = min(i0 + run, frames);
    unsigned local = 0;
    int mn = 0x7fffffff, mx = 0;
    for (int i = i0; i < i1; i++) {
        const int s = sizes[q.frame0 + i];
        local += (unsigned)s; mn = min(mn, s); mx = max(mx, s);
    }
    runsum[tid] = local; runmin[tid] = mn; runmax[tid] = mx;
    __syncthreads();
    if (tid == 0) {
        unsigned acc = 0;
        for (int t = 0; t < 256; t++) { const unsigned v = runsum[t]; runsum[t] = acc; acc += v; mn = min(mn, runmin[t]); mx = max(mx, runmax[t]); }
        if (frames == 0) mn = 0;
        // "fLaC", STREAMINFO as the last metadata block, 34 bytes: block size 4096 twice, min / max frame size, rate (20 bits), channels - 1
        // (3), bits - 1 (5), total samples (36), MD5 zero ("not computed")
        unsigned char* o = out + q.out_off;
        const unsigned long long info = ((unsigned long long)rate << 44) | (15ULL << 36) | (unsigned long long)len;
        const unsigned char head[18] = {'f', 'L', 'a', 'C', 0x80, 0, 0, 34, 0x10, 0x00, 0x10, 0x00,
                                        (unsigned char)(mn >> 16), (unsigned char)(mn >> 8), (unsigned char)mn,
                                        (unsigned char)(mx >> 16), (unsigned char)(mx >> 8), (unsigned char)mx};
        for (int i = 0; i < 18; i++) o[i] = head[i];
        for (int i = 0; i < 8; i++) o[18 + i] = (unsigned char)(info >> (56 - 8 * i));
        for (int i = 26; i < kFlHeader; i++) o[i] = 0;
        out_len[r] = kFlHeader + (int)acc;
    }
    __syncthreads();
    unsigned acc = runsum[tid];
    for (int i = i0; i < i1; i++) { frame_off[q.frame0 + i] = acc; acc += (unsigned)sizes[q.frame0 + i]; }
}

__global__ __launch_bounds__(256) void wave_flac_pack_kernel(const FlReq* __restrict__ reqs, int n, const int* __restrict__ len_dev,
                                                             const unsigned char* __restrict__ scratch, const int* __restrict__ sizes,
                                                             const unsigned* __restrict__ frame_off, unsigned char* __restrict__ out) {
    const int tid = threadIdx.x;
    const int r = last_at_or_before<&FlReq::frame0>(reqs, n, (int)blockIdx.x);
    const FlReq q = reqs[r];
    const int f = blockIdx.x - q.frame0;
    if ((long long)f * kFlBlock >= fl_len(len_dev, r, q.cap)) return;
    const unsigned char* src = scratch + (size_t)blockIdx.x * kFlSlot;
    unsigned char* dst = out + q.out_off + kFlHeader + frame_off[blockIdx.x];
    const int nbytes = sizes[blockIdx.x];
    // (never past the request's part of the output, which the host sized by the bound below)
    if ((long long)frame_off[blockIdx.x] + nbytes > 2LL * q.cap + 16LL * (((long long)q.cap + kFlBlock - 1) / kFlBlock)) return;
    const int head = min(nbytes, (int)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3));   // bytes up to the destination's 4-byte boundary
    if (tid < head) dst[tid] = src[tid];
    const int words = (nbytes - head) >> 2;
    for (int i = tid; i < words; i += 256) {
        const unsigned char* s = src + head + 4 * i;
        *reinterpret_cast<unsigned*>(dst + head + 4 * i) = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16) | ((unsigned)s[3] << 24);
    }
    const int done = head + 4 * words;
    if (tid < nbytes - done) dst[done + tid] = src[done + tid];
}

struct FlWorkspace {
    FlReq* reqs = nullptr; size_t cap_reqs = 0;
    unsigned* scratch = nullptr; size_t cap_scratch = 0;
    int* sizes = nullptr; size_t cap_sizes = 0;
    unsigned* frame_off = nullptr; size_t cap_frame_off = 0;
    WorkspaceUse use;
};

static int fl_rate_code(int rate) {
    switch (rate) {
        case 8000: return 4; case 16000: return 5; case 22050: return 6; case 24000: return 7; case 32000: return 8; case 44100: return 9;
        case 48000: return 10; default: return -1;
    }
}

// the stream header, the samples as VERBATIM and 16 bytes of frame around them (header <= 11, subframe header 1, CRC-16 2)
int64_t f5hip_wave_flac_bound(int32_t max_len) {
    if (max_len < 0) return 0;
    return kFlHeader + 2LL * max_len + 16LL * (((long long)max_len + kFlBlock - 1) / kFlBlock);
}

int f5hip_wave_flac(int32_t n, const int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev, int32_t sample_rate,
                    uint8_t* out_dev, const int64_t* out_off, int32_t* out_len_dev, void* stream) {
    return f5hip_wave_flac_levels(n, pcm_dev, in_off, max_len, len_dev, sample_rate, nullptr, out_dev, out_off, out_len_dev, stream);
}

int f5hip_wave_flac_levels(int32_t n, const int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev,
                           int32_t sample_rate, const int32_t* level, uint8_t* out_dev, const int64_t* out_off, int32_t* out_len_dev, void* stream) {
    if (n < 1 || !pcm_dev || !in_off || !max_len || !out_dev || !out_off || !out_len_dev) return fail(-1, "wave_flac: bad argument");
    const int code = fl_rate_code(sample_rate);
    if (code < 0) return fail(-1, "wave_flac: the sample rate must be one of 8000, 16000, 22050, 24000, 32000, 44100, 48000 (got %d)", sample_rate);
    if ((reinterpret_cast<uintptr_t>(pcm_dev) & 1) || (reinterpret_cast<uintptr_t>(out_dev) & 15))
        return fail(-1, "wave_flac: the input must be 2-byte aligned and the output 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(len_dev) & 3) || (reinterpret_cast<uintptr_t>(out_len_dev) & 3))
        return fail(-1, "wave_flac: the lengths must be 4-byte aligned");
    std::vector<FlReq> h(n);
    long long total_in = 0, total_out = 0, frames = 0;
    bool any_lpc = false;
    for (int i = 0; i < n; i++) {
        const int lv = level ? level[i] : 0;
        if (lv != 0 && lv != 1) return fail(-1, "wave_flac: the level of request %d must be 0 or 1 (got %d)", i, lv);
        any_lpc |= lv == 1;
        if (max_len[i] < 0) return fail(-1, "wave_flac: request %d has a negative length bound (%d)", i, max_len[i]);
        if (out_off[i] < 0 || (out_off[i] & 15)) return fail(-1, "wave_flac: the output offset of request %d is not a multiple of 16 bytes", i);
        total_in += max_len[i]; total_out += f5hip_wave_flac_bound(max_len[i]);
        if (total_in > 2147483647LL || total_out > 2147483647LL) return fail(-1, "wave_flac: the call exceeds 2^31 - 1 samples in or bytes out");
        h[i] = FlReq{in_off[i], out_off[i], max_len[i], (int)frames, lv, 0};
        frames += ((long long)max_len[i] + kFlBlock - 1) / kFlBlock;
    }
    FlWorkspace* const wsp = device_workspace<FlWorkspace>("wave_flac");
    if (!wsp) return -6;
    FlWorkspace& ws = *wsp;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(dev_reserve(&ws.reqs, &ws.cap_reqs, (size_t)n, "wave_flac requests"));
    if (frames) {
        CK(dev_reserve(&ws.scratch, &ws.cap_scratch, (size_t)frames * kFlWords, "wave_flac frames"));
        CK(dev_reserve(&ws.sizes, &ws.cap_sizes, (size_t)frames, "wave_flac frame sizes"));
        CK(dev_reserve(&ws.frame_off, &ws.cap_frame_off, (size_t)frames, "wave_flac frame offsets"));
    }
    if (upload_sync(st, ws.reqs, h) != hipSuccess) return fail(-6, "wave_flac metadata upload");
    if (frames) {
        // (the level-0 instantiation unless some request asks for level 1)
        if (any_lpc)
            hipLaunchKernelGGL(wave_flac_frame_kernel<true>, dim3((unsigned)frames), dim3(256), 0, st, ws.reqs, n, (const short*)pcm_dev,
                               (const int*)len_dev, code, ws.scratch, ws.sizes);
        else
            hipLaunchKernelGGL(wave_flac_frame_kernel<false>, dim3((unsigned)frames), dim3(256), 0, st, ws.reqs, n, (const short*)pcm_dev,
                               (const int*)len_dev, code, ws.scratch, ws.sizes);
        CKL("wave_flac_frame");
        g_counters[CNT_WAVE_FLAC_LAUNCHES]++;
    }
    hipLaunchKernelGGL(wave_flac_scan_kernel, dim3((unsigned)n), dim3(256), 0, st, ws.reqs, (const int*)len_dev, ws.sizes, ws.frame_off, (int)sample_rate,
                       (unsigned char*)out_dev, (int*)out_len_dev);
    CKL("wave_flac_scan");
    g_counters[CNT_WAVE_FLAC_LAUNCHES]++;
    if (frames) {
        hipLaunchKernelGGL(wave_flac_pack_kernel, dim3((unsigned)frames), dim3(256), 0, st, ws.reqs, n, (const int*)len_dev,
                           (const unsigned char*)ws.scratch, ws.sizes, ws.frame_off, (unsigned char*)out_dev);
        CKL("wave_flac_pack");
        g_counters[CNT_WAVE_FLAC_LAUNCHES]++;
    }
    g_counters[CNT_WAVE_FLAC_REQUESTS] += n;
    return 0;
}

// ------------------------------------------------------------------------------------------------ loudness: BS.1770 target, in place
// f5hip_wave_loudness: the 24 kHz int16 PCM of n requests, in place, to each flagged request's loudness target -- wave_codec.measure_loudness
// and normalise_loudness_pcm16 bit for bit (the definition is written down there and in include/f5hip.h).  Integers up to one sqrt: no sum
// depends on the order of its terms, so the tiling below decides no bit.
//   wave_kweight_kernel  one block of 192 threads per (flagged request, tile of two 100 ms sub-blocks = 4800 samples).  The tile's samples and
//                        the kLdTaps - 1 before them go to LDS as fp32 (exact), the tap table as fp64.  A thread owns 25 consecutive outputs
//                        (a stride of 25 words: no LDS bank conflict) and keeps the 25 samples they need plus the next 7 in a ring of 32
//                        registers whose slot numbers are compile-time constants (the tap loop is unrolled by 32): a tap costs one broadcast
//                        tap read, one sample read and 25 fp64 FMAs, and no register moves.  fp64 FMA, not a 64-bit integer MAC: |y| <=
//                        sum|h| 32768 < 2^33, so every partial sum is an integer below 2^53 and the FMA is exact, and v_fma_f64 issues at
//                        half the fp32 rate (78.6 TFLOPS fp64 vector in the MI355X data sheet) where the 32 x 32 + 64 integer MAC
//                        (v_mad_i64_i32) is a quarter-rate instruction and h x (32 767 h does not fit 32 bits) leaves no cheaper one.  z = y >> 14
//                        on the integer, z^2 summed per thread, then per sub-block (96 threads each) in int64; the tile's max |x| beside it.
//   wave_gate_kernel     one block per flagged request: E[b] = (e[b] + .. + e[b+3]) >> 8, the absolute gate, the relative gate from the block
//                        sums (int64, a fixed tree: exact anyway), the peak over the tiles; g and the stats row by one thread.
//   wave_gain_kernel     the launch-1 grid again: pcm = clip(rint(x g)), 8 samples in a 16-byte load and store where the address allows.
// Three launches whatever n, none when no request is flagged; no host sync between them; a request's bytes depend on that request alone.
constexpr int kLdTaps = 1024;                   // wave_codec.LOUDNESS_TAPS
constexpr int kLdSub = 2400;                    // 100 ms sub-block
constexpr int kLdRun = 25;                      // consecutive outputs of a thread
constexpr int kLdThreads = 192;                 // 96 threads a sub-block
constexpr int kLdTile = kLdThreads * kLdRun;    // 4800: two sub-blocks
constexpr int kLdRing = 32;                     // the register ring: kLdRun samples in use and kLdRing - kLdRun = 7 read ahead
constexpr int kLdFront = 8;                     // zeros in front of the LDS window: the read-ahead of the last taps lands there
constexpr int kLdWindow = kLdFront + kLdTaps - 1 + kLdTile;
constexpr int kLdYShift = 14, kLdEShift = 8;
constexpr long long kLdGateAbs = 75535;         // floor(10^((-70 + 0.691) / 10) * 9600 * 2^26): wave_codec.LOUDNESS_GATE_ABS
constexpr double kLdPeakCeiling = 29203.0;      // -1 dBFS: wave_codec.LOUDNESS_PEAK_CEILING
__device__ const int kLdTapTable[kLdTaps] = {
#include "loudness_taps.inc"
};
constexpr long long kLdTapAbsSum = 212915;      // sum |h| (loudness_taps.inc states it; tests hold the file to wave_codec.loudness_taps())
// the bit budget: |y| <= sum|h| 2^15 is exact in fp64 and in int64, |z| < 2^19, a sub-block's sum of z^2 < 2^50, a request's gated sum < 2^63
static_assert(kLdTapAbsSum * 32768 < (1LL << 53), "wave_loudness: y must be exact in fp64");
static_assert(((kLdTapAbsSum * 32768) >> kLdYShift) < (1LL << 19), "wave_loudness: |z| < 2^19");
static_assert((double)kLdSub * (double)(1LL << 38) < (double)(1LL << 50), "wave_loudness: e < 2^50");
static_assert(kLdTile == 2 * kLdSub && kLdThreads % 2 == 0 && kLdTaps % kLdRing == 0 && kLdRing - kLdRun <= kLdFront && kLdTile % 8 == 0,
              "wave_loudness tiling");

struct LdReq {
    long long in_off;    // its first sample, relative to pcm_dev
    double gain_k;       // K_T of its target
    int cap;             // upper bound of its length (the length itself without len_dev)
    int req;             // its index in the call: len_dev and stats row
    int tile0;           // its first block of launches 1 and 3 = its first peak slot; its sub-block sums start at 2 * tile0
    int tiles;
};

F5_DEVICE int ld_len(const int* len_dev, const LdReq& q) { return len_dev ? min(max(len_dev[q.req], 0), q.cap) : q.cap; }

F5_DEVICE void ld_taps32(double (&acc)[kLdRun], double (&w)[kLdRing], const double* __restrict__ tp, const float* __restrict__ xq) {
    // one group of 32 taps (tp: its first tap): slot numbers are constants; xq = the thread's first sample minus the group's first tap index
#pragma unroll
    for (int k = 0; k < kLdRing; k++) {
        const double t = tp[k];
        w[(kLdRing + kLdRun - k) & (kLdRing - 1)] = (double)xq[-k - (kLdRing - kLdRun)];   // x[j0 - k - 7]: tap k + 7's first sample
#pragma unroll
        for (int r = 0; r < kLdRun; r++) acc[r] = fma(t, w[(kLdRing + r - k) & (kLdRing - 1)], acc[r]);
    }
}

__global__ __launch_bounds__(kLdThreads) void wave_kweight_kernel(const LdReq* __restrict__ reqs, int nf, const short* __restrict__ pcm,
                                                                  const int* __restrict__ len_dev, long long* __restrict__ sub,
                                                                  int* __restrict__ peaks) {
    __shared__ __attribute__((aligned(16))) double tp[kLdTaps];
    __shared__ float xs[kLdWindow];
    __shared__ long long part[kLdThreads];
    __shared__ int pk[kLdThreads];
    const int tid = threadIdx.x;
    const int f = last_at_or_before<&LdReq::tile0>(reqs, nf, (int)blockIdx.x);
    const LdReq q = reqs[f];
    const int tile = blockIdx.x - q.tile0;
    const int len = ld_len(len_dev, q);
    const long long j0 = (long long)tile * kLdTile;
    if (j0 >= len) {                                                    // a tile past the request's actual length: no sub-block, no sample
        if (tid == 0) peaks[blockIdx.x] = 0;
        return;
    }
    const short* x = pcm + q.in_off;
    int peak = 0;
    for (int i = tid; i < kLdWindow; i += kLdThreads) {
        const long long src = j0 - (kLdTaps - 1) - kLdFront + i;
        const int v = src >= 0 && src < len ? (int)x[src] : 0;
        xs[i] = (float)v;
        if (src >= j0) peak = max(peak, abs(v));
    }
    for (int i = tid; i < kLdTaps; i += kLdThreads) tp[i] = (double)kLdTapTable[i];
    __syncthreads();

    // the thread's 25 outputs start at xb; ring slot (r & 31) holds xb[r] for r = -6 .. 24 before tap 0 (tap 0 fills slot 25 before anything reads it)
    const float* xb = xs + kLdFront + kLdTaps - 1 + tid * kLdRun;
    double acc[kLdRun], w[kLdRing];
#pragma unroll
    for (int r = 0; r < kLdRun; r++) acc[r] = 0.0;
#pragma unroll
    for (int r = kLdRun - kLdRing + 1; r < kLdRun; r++) w[r & (kLdRing - 1)] = (double)xb[r];
    for (int k0 = 0; k0 < kLdTaps; k0 += kLdRing) ld_taps32(acc, w, tp + k0, xb - k0);

    long long ss = 0;
#pragma unroll
    for (int r = 0; r < kLdRun; r++) {
        const long long z = (long long)acc[r] >> kLdYShift;             // (an arithmetic shift: floor)
        ss += z * z;
    }
    part[tid] = ss;
    pk[tid] = peak;
    __syncthreads();
    if (tid < 2) {                                                      // sub-block `tid` of the tile: only a whole one counts
        const long long s = 2LL * tile + tid;
        if ((s + 1) * kLdSub <= len) {
            long long e = 0;
            for (int t = 0; t < kLdThreads / 2; t++) e += part[tid * (kLdThreads / 2) + t];
            sub[2LL * q.tile0 + s] = e;
        }
    } else if (tid == 64) {
        int m = 0;
        for (int t = 0; t < kLdThreads; t++) m = max(m, pk[t]);
        peaks[blockIdx.x] = m;
    }
}

__global__ __launch_bounds__(256) void wave_gate_kernel(const LdReq* __restrict__ reqs, const int* __restrict__ len_dev,
                                                        const long long* __restrict__ sub, const int* __restrict__ peaks,
                                                        long long* __restrict__ stats) {
    __shared__ long long red[256];
    const int tid = threadIdx.x;
    const LdReq q = reqs[blockIdx.x];
    const int len = ld_len(len_dev, q);
    const int ns = len / kLdSub, nb = max(ns - 3, 0);
    const long long* e = sub + 2LL * q.tile0;
    long long n1 = 0, S1 = 0;
    for (int b = tid; b < nb; b += 256) {
        const long long E = (e[b] + e[b + 1] + e[b + 2] + e[b + 3]) >> kLdEShift;
        if (E > kLdGateAbs) { n1++; S1 += E; }
    }
    n1 = block_sum(red, tid, n1);
    S1 = block_sum(red, tid, S1);
    long long n2 = 0, S2 = 0;
    if (n1 > 0) {
        const long long rel = S1 / (10 * n1);
        for (int b = tid; b < nb; b += 256) {
            const long long E = (e[b] + e[b + 1] + e[b + 2] + e[b + 3]) >> kLdEShift;
            if (E > kLdGateAbs && E > rel) { n2++; S2 += E; }
        }
    }
    n2 = block_sum(red, tid, n2);
    S2 = block_sum(red, tid, S2);
    long long peak = 0;
    const int used = (int)(((long long)len + kLdTile - 1) / kLdTile);   // (tiles past the length hold 0 anyway)
    for (int t = tid; t < used; t += 256) peak = max(peak, (long long)peaks[q.tile0 + t]);
    red[tid] = peak;
    __syncthreads();
    if (tid != 0) return;
    for (int t = 1; t < 256; t++) peak = max(peak, red[t]);
    double g = 1.0;
    if (n2 > 0) {   // one correctly rounded fp64 operation per step, as wave_codec.loudness_gain: no product feeds a sum
        g = sqrt(q.gain_k * (double)n2 / (double)S2);
        g = fmin(g, kLdPeakCeiling / (double)peak);
    }
    long long* row = stats + 4LL * q.req;
    row[0] = n2; row[1] = S2; row[2] = peak; row[3] = __double_as_longlong(g);
}

__global__ __launch_bounds__(256) void wave_gain_kernel(const LdReq* __restrict__ reqs, int nf, short* __restrict__ pcm,
                                                        const int* __restrict__ len_dev, const long long* __restrict__ stats) {
    const int f = last_at_or_before<&LdReq::tile0>(reqs, nf, (int)blockIdx.x);
    const LdReq q = reqs[f];
    const long long* row = stats + 4LL * q.req;
    if (row[0] == 0) return;                                            // nothing passed the gates: the request stays as it is
    const double g = __longlong_as_double(row[3]);
    const int len = ld_len(len_dev, q);
    const long long j0 = (long long)(blockIdx.x - q.tile0) * kLdTile;
    short* x = pcm + q.in_off;
    for (int grp = threadIdx.x; grp < kLdTile / 8; grp += 256) {
        const long long j = j0 + 8 * grp;
        if (j >= len) break;
        if (j + 8 <= len && (reinterpret_cast<uintptr_t>(x + j) & 15) == 0) {
            const int4 in = *reinterpret_cast<const int4*>(x + j);
            const int w8[4] = {in.x, in.y, in.z, in.w};
            int o[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int lo = (int)fmax(fmin(rint((double)(short)(w8[e] & 0xffff) * g), 32767.0), -32768.0);
                const int hi = (int)fmax(fmin(rint((double)(w8[e] >> 16) * g), 32767.0), -32768.0);
                o[e] = (lo & 0xffff) | (hi << 16);
            }
            *reinterpret_cast<int4*>(x + j) = make_int4(o[0], o[1], o[2], o[3]);
        } else {
            for (int e = 0; e < 8 && j + e < len; e++) x[j + e] = (short)(int)fmax(fmin(rint((double)x[j + e] * g), 32767.0), -32768.0);
        }
    }
}

struct LdWorkspace {
    LdReq* reqs = nullptr; size_t cap_reqs = 0;
    long long* sub = nullptr; size_t cap_sub = 0;
    int* peaks = nullptr; size_t cap_peaks = 0;
    WorkspaceUse use;
};

int f5hip_wave_loudness_tile(void) { return kLdTile; }

int f5hip_wave_loudness(int32_t n, int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev, const double* gain_k,
                        int64_t* stats_dev, void* stream) {
    if (n < 1 || !pcm_dev || !in_off || !max_len || !gain_k || !stats_dev) return fail(-1, "wave_loudness: bad argument");
    if ((reinterpret_cast<uintptr_t>(pcm_dev) & 1) || (reinterpret_cast<uintptr_t>(len_dev) & 3) || (reinterpret_cast<uintptr_t>(stats_dev) & 7))
        return fail(-1, "wave_loudness: the samples must be 2-byte aligned, the lengths 4-byte and the stats 8-byte");
    std::vector<LdReq> h;
    long long total = 0, tiles = 0;
    for (int i = 0; i < n; i++) {
        if (max_len[i] < 0) return fail(-1, "wave_loudness: request %d has a negative length bound (%d)", i, max_len[i]);
        if (in_off[i] < 0) return fail(-1, "wave_loudness: request %d has a negative offset", i);
        if (!std::isfinite(gain_k[i])) return fail(-1, "wave_loudness: the gain constant of request %d is not finite", i);
        total += max_len[i];
        if (total > 2147483647LL) return fail(-1, "wave_loudness: the call exceeds 2^31 - 1 samples");
        if (!(gain_k[i] > 0.0)) continue;                               // <= 0: the request is left alone
        const long long t = std::max<long long>(((long long)max_len[i] + kLdTile - 1) / kLdTile, 1);   // (an empty request keeps one block)
        h.push_back(LdReq{in_off[i], gain_k[i], max_len[i], i, (int)tiles, (int)t});
        tiles += t;
    }
    if (h.empty()) return 0;
    LdWorkspace* const wsp = device_workspace<LdWorkspace>("wave_loudness");
    if (!wsp) return -6;
    LdWorkspace& ws = *wsp;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(dev_reserve(&ws.reqs, &ws.cap_reqs, h.size(), "wave_loudness requests"));
    CK(dev_reserve(&ws.sub, &ws.cap_sub, (size_t)(2 * tiles), "wave_loudness sub-block sums"));
    CK(dev_reserve(&ws.peaks, &ws.cap_peaks, (size_t)tiles, "wave_loudness peaks"));
    if (upload_sync(st, ws.reqs, h) != hipSuccess) return fail(-6, "wave_loudness metadata upload");
    const int nf = (int)h.size();
    hipLaunchKernelGGL(wave_kweight_kernel, dim3((unsigned)tiles), dim3(kLdThreads), 0, st, ws.reqs, nf, (const short*)pcm_dev, (const int*)len_dev, ws.sub,
                       ws.peaks);
    CKL("wave_kweight");
    hipLaunchKernelGGL(wave_gate_kernel, dim3((unsigned)nf), dim3(256), 0, st, ws.reqs, (const int*)len_dev, ws.sub, ws.peaks, (long long*)stats_dev);
    CKL("wave_gate");
    hipLaunchKernelGGL(wave_gain_kernel, dim3((unsigned)tiles), dim3(256), 0, st, ws.reqs, nf, (short*)pcm_dev, (const int*)len_dev,
                       (const long long*)stats_dev);
    CKL("wave_gain");
    g_counters[CNT_WAVE_LOUDNESS_LAUNCHES] += 3;
    g_counters[CNT_WAVE_LOUDNESS_REQUESTS] += nf;
    return 0;
}

// ------------------------------------------------------------------------------------------------ prosody: tempo and pitch of the finished PCM
// f5hip_wave_prosody: the 24 kHz int16 PCM of n requests -> each request's time-scale modified PCM, bit for bit wave_codec.shift_pcm16 (the
// definition is written down there and in include/f5hip.h; the index geometry, the tie rule and the blend are wave_prosody_core.h, which
// tools/wave_prosody_check.cpp runs on the CPU under sanitizers).  Integers only in the first launch, the resampler's exact fp64 in the second.
//   wave_wsola_kernel  one workgroup of 256 threads per request, its frames in sequence: frame k's start depends on frame k - 1's.  Per frame
//                      the 1440 source samples that hold every candidate, xt[p_k - D .. p_k + D + L), go to LDS biased by 32768 (unsigned
//                      order, the same differences) -- twice, the second copy one sample on, so that a candidate at an odd offset reads
//                      aligned 32-bit words too -- beside the target xt[s_{k-1} + H ..).  The 481 candidates go across the threads, two a
//                      thread that share the target's 16-byte reads; a cost is 480 v_sad_u16, two differences each.  Lanes 2 j and 2 j + 1
//                      read word j + w of the even and of the odd copy, which lie 32 banks apart: no LDS bank conflict.  ONE min-reduction
//                      over the packed key cost * 2^9 + rank(d) (64-bit shuffles, then 4 words of LDS), so the choice does not depend on lane
//                      order.  Frame k's placement finalises the H outputs of frame k - 1, blended from the LDS copies -- no second read of
//                      the samples, no accumulator buffer, no atomics --, 8 samples in a 16-byte vector store.  A request with P == Q is
//                      copied through.  A request with a pitch leaves its stretched PCM in the workspace for the second launch, and so does one that
//                      keeps its formants (wave_formant.h), for the three launches of f5hip_wave_prosody_formants.
//   wave_pitch_kernel  wave_encode_kernel's tile body (we_tile_body) with the rate pair p : q, the tile size and the tap table of the
//                      REQUEST: one block per tile of a pitched request, its table (below 11 KB) staged in LDS from the one device table
//                      that holds all twelve.
// Two launches whatever n, one when no request has a pitch; no host sync between them; a request's bytes depend on that request alone.
constexpr int kPrThreads = 256;
constexpr int kPrWords = kPrWindow / 2;         // 720 words hold the window
constexpr int kPrOddBase = 736;                 // the odd copy's first word: 32 banks on from the even copy's (736 = 11 * 64 + 32)
static_assert(kPrOddBase >= kPrWords && kPrOddBase % 64 == 32 && kPrFrame % 8 == 0 && kPrHop % 8 == 0 && kPrCands <= 2 * kPrThreads, "wave_prosody tiling");
static_assert(960LL * 65535 < (1LL << 26) && 2 * kPrSearch < 512, "wave_prosody: the packed key");
__device__ const int kPrRiseTable[kPrHop] = {
#include "wsola_window.inc"
};

struct PrReq {
    long long in_off;    // its first sample, relative to pcm_dev
    long long out_off;   // its first output sample (a multiple of 8: 16-byte stores)
    long long mid_off;   // pitched: its first stretched sample in the workspace (a multiple of 8)
    int cap;             // upper bound of its length (the length itself without len_dev)
    int req;             // its index in the call: len_dev and out_len
    int P, Q;            // the stretch
    int of, nf, width, L;// pitched: p : q and its tap table's shape; of == 0: no pitch
    int tq, tap_off;     // pitched: polyphase blocks per tile, its table's first float in the device table
    int tile0;           // pitched: its first block of the second launch
    int keep;            // it keeps its formants (wave_formant.h): its stretched PCM stays in the workspace like a pitched request's, of == 0
};

F5_DEVICE int pr_len(const int* len_dev, const PrReq& q) { return len_dev ? min(max(len_dev[q.req], 0), q.cap) : q.cap; }

__global__ __launch_bounds__(kPrThreads) void wave_wsola_kernel(const PrReq* __restrict__ reqs, const short* __restrict__ pcm,
                                                                const int* __restrict__ len_dev, short* __restrict__ out, short* __restrict__ mid,
                                                                int* __restrict__ out_len) {
    __shared__ __attribute__((aligned(16))) unsigned wn[kPrOddBase + kPrWords];    // the window: even copy, then the odd copy
    __shared__ __attribute__((aligned(16))) unsigned tg[kPrFrame / 2];             // the target
    __shared__ int rise[kPrHop];
    __shared__ unsigned long long red[kPrThreads / 64];
    const int tid = threadIdx.x;
    const PrReq q = reqs[blockIdx.x];
    const int len = pr_len(len_dev, q);
    const PrGeom g = pr_geom(len, q.P, q.Q);
    const short* x = pcm + q.in_off;
    short* y = (q.of | q.keep) ? mid + q.mid_off : out + q.out_off;
    if (!q.of && tid == 0) out_len[q.req] = (int)g.m;
    if (q.P == q.Q) {                                                   // neutral: copied through (g.m == len)
        const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
        for (long long j = 8LL * tid; j < len; j += 8 * kPrThreads) {
            if (vec && j + 8 <= len) {
                *reinterpret_cast<int4*>(y + j) = *reinterpret_cast<const int4*>(x + j);
            } else {
                for (int e = 0; e < 8 && j + e < len; e++) y[j + e] = x[j + e];
            }
        }
        return;
    }
    unsigned short* const ev16 = reinterpret_cast<unsigned short*>(wn);
    unsigned short* const od16 = reinterpret_cast<unsigned short*>(wn + kPrOddBase);
    unsigned short* const tg16 = reinterpret_cast<unsigned short*>(tg);
    for (int i = tid; i < kPrHop; i += kPrThreads) rise[i] = kPrRiseTable[i];
    if (tid == 0) od16[kPrWindow - 1] = 0x8000;                         // (the sample behind the window: never part of a candidate)

    // the thread's two candidates c = d + D: c0 = tid and c1 = tid + 256 (the threads past the last candidate repeat it and drop the result)
    const int c0 = tid, c1 = min(tid + kPrThreads, kPrCands - 1);
    const unsigned* const b0 = wn + ((c0 & 1) ? kPrOddBase : 0) + (c0 >> 1);
    const unsigned* const b1 = wn + ((c1 & 1) ? kPrOddBase : 0) + (c1 >> 1);
    long long s = -kPrHop;                                              // s_0
    for (long long k = 1; k < g.K; k++) {
        const long long pk = pr_nominal(g, k), t = s + kPrHop;
        for (int i = tid; i < kPrWindow; i += kPrThreads) {
            const unsigned short v = (unsigned short)pr_source(x, len, pk - kPrSearch + i);
            ev16[i] = v;
            if (i > 0) od16[i - 1] = v;
        }
        for (int i = tid; i < kPrFrame; i += kPrThreads) tg16[i] = (unsigned short)pr_source(x, len, t + i);
        __syncthreads();

        unsigned a0 = 0, a1 = 0;
        const uint4* t4 = reinterpret_cast<const uint4*>(tg);
#pragma unroll 4
        for (int w = 0; w < kPrFrame / 8; w++) {
            const uint4 tv = t4[w];
            a0 = __builtin_amdgcn_sad_u16(b0[4 * w], tv.x, a0); a1 = __builtin_amdgcn_sad_u16(b1[4 * w], tv.x, a1);
            a0 = __builtin_amdgcn_sad_u16(b0[4 * w + 1], tv.y, a0); a1 = __builtin_amdgcn_sad_u16(b1[4 * w + 1], tv.y, a1);
            a0 = __builtin_amdgcn_sad_u16(b0[4 * w + 2], tv.z, a0); a1 = __builtin_amdgcn_sad_u16(b1[4 * w + 2], tv.z, a1);
            a0 = __builtin_amdgcn_sad_u16(b0[4 * w + 3], tv.w, a0); a1 = __builtin_amdgcn_sad_u16(b1[4 * w + 3], tv.w, a1);
        }
        unsigned long long key = pr_key(a0, c0 - kPrSearch);
        if (tid + kPrThreads < kPrCands) key = min(key, pr_key(a1, c1 - kPrSearch));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned long long)__shfl_xor(key, o));
        if ((tid & 63) == 0) red[tid >> 6] = key;
        __syncthreads();
        key = min(min(red[0], red[1]), min(red[2], red[3]));
        const int c = pr_key_offset(key) + kPrSearch;
        s = pk + c - kPrSearch;

        // frame k - 1's H outputs: its falling half (the target's first H samples) over frame k's rising half (the window from c on)
        if (tid < kPrHop / 8) {
            const int i0 = 8 * tid;
            const long long j0 = (k - 1) * kPrHop + i0;
            if (j0 < g.m) {
                int v[8];
#pragma unroll
                for (int e = 0; e < 8; e++) v[e] = pr_blend(rise[i0 + e], pr_unbias(tg16[i0 + e]), pr_unbias(ev16[c + i0 + e]));
                if (j0 + 8 <= g.m) {                                    // (y + j0 is 16-byte aligned: the request's first sample and j0 are multiples of 8)
                    *reinterpret_cast<int4*>(y + j0) = make_int4((v[0] & 0xffff) | (v[1] << 16), (v[2] & 0xffff) | (v[3] << 16),
                                                                 (v[4] & 0xffff) | (v[5] << 16), (v[6] & 0xffff) | (v[7] << 16));
                } else {
                    for (int e = 0; e < 8 && j0 + e < g.m; e++) y[j0 + e] = (short)v[e];
                }
            }
        }
        __syncthreads();                                                // the next frame overwrites the window and the target
    }
}

__global__ __launch_bounds__(256) void wave_pitch_kernel(const PrReq* __restrict__ reqs, int np, const int* __restrict__ len_dev,
                                                         const short* __restrict__ mid, const float* __restrict__ taps, short* __restrict__ out,
                                                         int* __restrict__ out_len) {
    extern __shared__ __attribute__((aligned(16))) char pr_sm[];
    const int f = last_at_or_before<&PrReq::tile0>(reqs, np, (int)blockIdx.x);
    const PrReq q = reqs[f];
    const int tile = blockIdx.x - q.tile0;
    const long long m = pr_geom(pr_len(len_dev, q), q.P, q.Q).m;        // what the first launch left in the workspace
    const long long n_out = ((long long)q.nf * m + q.of - 1) / q.of;
    if (tile == 0 && threadIdx.x == 0) out_len[q.req] = (int)n_out;
    we_tile_body<true>(pr_sm, mid + q.mid_off, (int)m, n_out, tile, taps + q.tap_off, q.of, q.nf, q.width, q.L, q.tq, 0,
                       reinterpret_cast<unsigned char*>(out + q.out_off));
}

struct PrWorkspace {
    PrReq* reqs = nullptr; size_t cap_reqs = 0;
    PrReq* pitched = nullptr; size_t cap_pitched = 0;
    short* mid = nullptr; size_t cap_mid = 0;
    WorkspaceUse use;
};

// floats of a pitch step's tap table in the device table (a multiple of 4: every table starts on a 16-byte boundary)
static long long pr_table_floats(int pitch) {
    int p, q;
    pr_pitch_ratio(pitch, &p, &q);
    const RatePair rp = rate_pair(p, q);
    return ((long long)rp.nf * rp.L + 3) & ~3LL;
}

int64_t f5hip_wave_prosody_tap_offset(int32_t pitch) {
    if (pitch < -kPrPitchMax || pitch > kPrPitchMax) return -1;
    long long at = 0;
    for (int s = -kPrPitchMax; s <= kPrPitchMax; s++) {
        if (s == 0) continue;
        if (s == pitch) return at;
        at += pr_table_floats(s);
    }
    return at;   // pitch == 0: the whole table
}

// a request that keeps its formants, as the WSOLA launch left it: what wave_formant.h's three launches start from
struct PrKept {
    long long mid_off, out_off;
    int cap, req, P, Q, pitch;
};

// f5hip_wave_prosody, and with `keep` (per request; null: nobody) the first part of f5hip_wave_prosody_formants: a flagged request is
// stretched by its (P, Q) into the workspace and listed in `kept`; then then(mid), the caller's own launches over the workspace's stretched
// PCM (an int, 0 = success), inside the same turn of the workspace
template <typename Then>
static int wave_prosody_run(int32_t n, const int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev,
                            const int32_t* stretch_p, const int32_t* stretch_q, const int32_t* pitch, const uint8_t* keep, const float* taps_dev,
                            int16_t* out_dev, const int64_t* out_off, int32_t* out_len_dev, std::vector<PrKept>* kept, void* stream, Then then) {
    if (n < 1 || !pcm_dev || !in_off || !max_len || !stretch_p || !stretch_q || !pitch || !out_dev || !out_off || !out_len_dev)
        return fail(-1, "wave_prosody: bad argument");
    if ((reinterpret_cast<uintptr_t>(pcm_dev) & 1) || (reinterpret_cast<uintptr_t>(len_dev) & 3) || (reinterpret_cast<uintptr_t>(taps_dev) & 15) ||
        (reinterpret_cast<uintptr_t>(out_dev) & 15) || (reinterpret_cast<uintptr_t>(out_len_dev) & 3))
        return fail(-1, "wave_prosody: the samples must be 2-byte aligned, the lengths 4-byte, the tap table and the output 16-byte");
    std::vector<PrReq> h(n), hp;
    long long total_in = 0, total_out = 0, mid = 0, tiles = 0, changed = 0;
    int lds = 0;
    for (int i = 0; i < n; i++) {
        if (max_len[i] < 0) return fail(-1, "wave_prosody: request %d has a negative length bound (%d)", i, max_len[i]);
        if (in_off[i] < 0) return fail(-1, "wave_prosody: request %d has a negative offset", i);
        if (out_off[i] < 0 || (out_off[i] & 7)) return fail(-1, "wave_prosody: the output offset of request %d is not a multiple of 8 samples", i);
        if (stretch_p[i] < 1 || stretch_q[i] < 1) return fail(-1, "wave_prosody: the stretch of request %d is not a pair of positive terms (%d/%d)", i, stretch_p[i], stretch_q[i]);
        if (!pr_stretch_ok(stretch_p[i], stretch_q[i]))
            return fail(-1, "wave_prosody: request %d stretches by %d/%d: outside 1/2 to 2 (terms up to %d)", i, stretch_p[i], stretch_q[i], kPrMaxTerm);
        if (pitch[i] < -kPrPitchMax || pitch[i] > kPrPitchMax) return fail(-1, "wave_prosody: request %d has a pitch of %d semitones (-6 to 6)", i, pitch[i]);
        PrReq& q = h[i];
        memset(&q, 0, sizeof(q));
        q.in_off = in_off[i]; q.out_off = out_off[i]; q.cap = max_len[i]; q.req = i; q.P = stretch_p[i]; q.Q = stretch_q[i];
        long long m = pr_geom(max_len[i], q.P, q.Q).m;
        if (m > 2147483647LL) return fail(-1, "wave_prosody: the call exceeds 2^31 - 1 samples in or out");
        if (keep && keep[i]) {
            if (!pitch[i]) return fail(-1, "wave_prosody: request %d keeps its formants without a pitch", i);
            q.keep = 1; q.mid_off = mid;
            mid += (m + 7) & ~7LL;
            kept->push_back(PrKept{q.mid_off, q.out_off, q.cap, i, q.P, q.Q, pitch[i]});
        } else if (pitch[i]) {
            if (!taps_dev) return fail(-1, "wave_prosody: request %d has a pitch: the call needs the tap table", i);
            int p, qq;
            pr_pitch_ratio(pitch[i], &p, &qq);
            const RatePair rp = rate_pair(p, qq);
            const WeTile t = we_tile(rp);
            if (!t.tq) return fail(-7, "wave_prosody: the tile of pitch %d does not fit the LDS", pitch[i]);
            q.of = rp.of; q.nf = rp.nf; q.width = rp.width; q.L = rp.L; q.tq = t.tq;
            q.tap_off = (int)f5hip_wave_prosody_tap_offset(pitch[i]);
            q.mid_off = mid; q.tile0 = (int)tiles;
            mid += (m + 7) & ~7LL;
            m = ((long long)rp.nf * m + rp.of - 1) / rp.of;
            tiles += std::max<long long>(((m + rp.nf - 1) / rp.nf + t.tq - 1) / t.tq, 1);   // (an empty request keeps one block: it writes its length)
            lds = std::max(lds, t.lds);
            hp.push_back(q);
        }
        changed += q.P != q.Q || pitch[i] != 0;
        total_in += max_len[i]; total_out += m;
        if (total_in > 2147483647LL || total_out > 2147483647LL || mid > 2147483647LL)
            return fail(-1, "wave_prosody: the call exceeds 2^31 - 1 samples in or out");
    }
    PrWorkspace* const wsp = device_workspace<PrWorkspace>("wave_prosody");
    if (!wsp) return -6;
    PrWorkspace& ws = *wsp;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(dev_reserve(&ws.reqs, &ws.cap_reqs, (size_t)n, "wave_prosody requests"));
    if (!hp.empty() || (kept && !kept->empty())) CK(dev_reserve(&ws.mid, &ws.cap_mid, (size_t)std::max<long long>(mid, 8), "wave_prosody stretched PCM"));
    if (!hp.empty()) {
        CK(dev_reserve(&ws.pitched, &ws.cap_pitched, hp.size(), "wave_prosody pitched requests"));
        static unsigned lds_attr_done = 0;
        if (lds > 64 * 1024 && f5_set_lds_attr((const void*)wave_pitch_kernel, kLdsMax, lds_attr_done) != hipSuccess)
            return fail(-7, "wave_prosody: LDS opt-in");
    }
    const hipError_t up = hp.empty() ? upload_sync(st, ws.reqs, h) : upload_sync(st, ws.reqs, h, ws.pitched, hp);
    if (up != hipSuccess) return fail(-6, "wave_prosody metadata upload");
    hipLaunchKernelGGL(wave_wsola_kernel, dim3((unsigned)n), dim3(kPrThreads), 0, st, ws.reqs, (const short*)pcm_dev, (const int*)len_dev, (short*)out_dev,
                       ws.mid, (int*)out_len_dev);
    CKL("wave_wsola");
    g_counters[CNT_WAVE_PROSODY_LAUNCHES]++;
    if (!hp.empty()) {
        hipLaunchKernelGGL(wave_pitch_kernel, dim3((unsigned)tiles), dim3(256), lds, st, ws.pitched, (int)hp.size(), (const int*)len_dev, (const short*)ws.mid,
                           taps_dev, (short*)out_dev, (int*)out_len_dev);
        CKL("wave_pitch");
        g_counters[CNT_WAVE_PROSODY_LAUNCHES]++;
    }
    g_counters[CNT_WAVE_PROSODY_REQUESTS] += changed;
    return then((const short*)ws.mid);
}

int f5hip_wave_prosody(int32_t n, const int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev,
                       const int32_t* stretch_p, const int32_t* stretch_q, const int32_t* pitch, const float* taps_dev, int16_t* out_dev,
                       const int64_t* out_off, int32_t* out_len_dev, void* stream) {
    return wave_prosody_run(n, pcm_dev, in_off, max_len, len_dev, stretch_p, stretch_q, pitch, nullptr, taps_dev, out_dev, out_off, out_len_dev, nullptr,
                            stream, [](const short*) { return 0; });
}
