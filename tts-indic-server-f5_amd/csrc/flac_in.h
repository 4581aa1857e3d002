// ------------------------------------------------------------------------------------------------ FLAC in: uploads decoded on the device
// f5hip_flac_decode: n native FLAC streams (RFC 9639), packed at arbitrary byte offsets in one device buffer -> each stream's samples as
// int32 planes [channels, total], bit for bit wave_codec.read_flac (the definition; flac_in_core.h holds the arithmetic, which
// tools/flac_in_check.cpp runs on the CPU under sanitizers).  FIVE launches whatever the batch, no host sync between them:
//   flac_in_scan_kernel     one thread per byte offset, a block per chunk of kFiChunk bytes.  An offset inside a stream whose bytes are a
//                           valid frame header (sync, reserved codes, coded number, CRC-8) is a candidate; a block-wide prefix sum numbers the
//                           chunk's candidates and sums their slot sizes (channels * block words).  Per byte: its candidate's number in the
//                           chunk (or none); per chunk: the candidates' offsets and slot prefixes, their count and the slots' total.
//   flac_in_offsets_kernel  one block: the exclusive scan of the chunks' counts and slot totals.  Candidate ids and slot addresses thereby
//                           follow from byte offsets alone: no atomic decides where anything lives.
//   flac_in_frame_kernel    one wavefront per candidate, false candidates included.  Lane 0 parses the subframes in stream order (Rice codes
//                           are serial) into the slot: warm-up samples and residuals.  The wave then restores them: the LPC / fixed
//                           prediction is one product per lane (lane j holds coefficient j and sample i-1-j) and a butterfly sum in int64,
//                           residuals and results move in registers 64 at a time; the wasted-bits shift and the CONSTANT fill run over the
//                           lanes; the CRC-16 is one slice of the frame per lane, folded by the GF(2) tree of wave_flac_frame_kernel.
//                           Leaves (end offset, status).
//   flac_in_chain_kernel    one wave per stream: from the first byte after the metadata, frame -> the candidate at its end offset, checking
//                           the numbering, the block sizes and the cap, and giving each visited frame its sample offset.  A frame counts
//                           iff the chain reaches it, so false syncs are never visited.  Leaves the stream's status and total.
//   flac_in_pack_kernel     one block per candidate: a visited frame's planes, stereo decorrelation undone, to [channels, n] of its stream.
// A stream outside the limits (channels > 2, bits outside 8 .. 24) has status FI_NEEDS_HOST before any launch; a frame over 16 384 samples, a
// candidate beyond the pool or the record table, or a stream longer than its output gives the same status on the way.  The caller decodes
// every stream whose status is not FI_OK on the host (ops.flac_decode: wave_codec.read_flac), so a refusal is raised by the definition.
#include "flac_in_core.h"

constexpr long long kFiPoolSlack = 64LL * kFiMaxChannels * kFiMaxBlock;   // words of slot pool for false candidates
constexpr int kFiGrid = 2048;                                             // waves of the frame launch, blocks of the pack launch

F5_DEVICE int fi_find_stream(const FiStream* streams, int n, long long pos) {   // the stream whose frames hold byte pos, or -1
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (streams[mid].begin <= pos) lo = mid; else hi = mid - 1;
    }
    const FiStream& s = streams[lo];
    return (pos >= s.begin && pos < s.end && s.status == FI_OK) ? lo : -1;
}

__global__ __launch_bounds__(1024) void flac_in_scan_kernel(const FiStream* __restrict__ streams, int n, const uint8_t* __restrict__ data, long long nbytes,
                                                            unsigned short* __restrict__ cand_local, unsigned short* __restrict__ chunk_list,
                                                            unsigned* __restrict__ chunk_slot, int* __restrict__ chunk_count,
                                                            long long* __restrict__ chunk_words) {
    __shared__ unsigned cnt[2][kFiChunk];
    __shared__ unsigned words[2][kFiChunk];
    const int t = threadIdx.x;
    const long long pos = (long long)blockIdx.x * kFiChunk + t;
    unsigned is = 0, w = 0;
    if (pos < nbytes) {
        const int s = fi_find_stream(streams, n, pos);
        if (s >= 0) {
            const FiStream st = streams[s];
            FiHeader h;
            if (fi_header(data + pos, st.end - pos, st.rate, st.bits, h)) {
                is = 1;
                w = h.block <= kFiMaxBlock ? (unsigned)(st.channels * h.block) : 0u;
            }
        }
    }
    cnt[0][t] = is; words[0][t] = w;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kFiChunk; d <<= 1) {                       // inclusive scan, double-buffered
        const unsigned c = cnt[cur][t] + (t >= d ? cnt[cur][t - d] : 0u), x = words[cur][t] + (t >= d ? words[cur][t - d] : 0u);
        cnt[cur ^ 1][t] = c; words[cur ^ 1][t] = x;
        cur ^= 1;
        __syncthreads();
    }
    const unsigned local = cnt[cur][t] - is, before = words[cur][t] - w;
    if (pos < nbytes) cand_local[pos] = is ? (unsigned short)local : (unsigned short)0xFFFF;
    if (is) {
        chunk_list[(long long)blockIdx.x * kFiChunk + local] = (unsigned short)t;
        chunk_slot[(long long)blockIdx.x * kFiChunk + local] = before;
    }
    if (t == kFiChunk - 1) { chunk_count[blockIdx.x] = (int)cnt[cur][t]; chunk_words[blockIdx.x] = (long long)words[cur][t]; }
}

__global__ __launch_bounds__(256) void flac_in_offsets_kernel(const int* __restrict__ chunk_count, const long long* __restrict__ chunk_words, int nchunks,
                                                              int* __restrict__ cbase, long long* __restrict__ sbase) {
    __shared__ long long part_c[256], part_w[256];
    const int t = threadIdx.x, per = (nchunks + 255) / 256, lo = min(t * per, nchunks), hi = min(lo + per, nchunks);
    long long c = 0, w = 0;
    for (int i = lo; i < hi; i++) { c += chunk_count[i]; w += chunk_words[i]; }
    part_c[t] = c; part_w[t] = w;
    __syncthreads();
    if (t == 0) {
        long long ac = 0, aw = 0;
        for (int i = 0; i < 256; i++) { const long long pc = part_c[i], pw = part_w[i]; part_c[i] = ac; part_w[i] = aw; ac += pc; aw += pw; }
        cbase[nchunks] = (int)min(ac, 2147483647LL);
    }
    __syncthreads();
    c = part_c[t]; w = part_w[t];
    for (int i = lo; i < hi; i++) { cbase[i] = (int)min(c, 2147483647LL); sbase[i] = w; c += chunk_count[i]; w += chunk_words[i]; }
}

// Candidate id -> (its byte offset, its slot's first word); ids are dense, chunk after chunk.
F5_DEVICE void fi_candidate(int id, const int* cbase, const long long* sbase, const unsigned short* chunk_list, const unsigned* chunk_slot, int nchunks,
                            long long* pos, long long* slot) {
    int lo = 0, hi = nchunks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cbase[mid] <= id) lo = mid; else hi = mid - 1;
    }
    const long long at = (long long)lo * kFiChunk + (id - cbase[lo]);
    *pos = (long long)lo * kFiChunk + chunk_list[at];
    *slot = sbase[lo] + chunk_slot[at];
}

F5_DEVICE unsigned fi_x_pow_rt(int bits) {                       // x^bits mod the CRC-16 polynomial, by squaring
    unsigned r = 1, sq = 2;
    for (; bits; bits >>= 1) { if (bits & 1) r = fl_gf_mul(r, sq); sq = fl_gf_mul(sq, sq); }
    return r;
}

// CRC-16 of bytes [0, len) at p by the wave: one right-aligned slice per lane, combined by a * x^(8 * slice * 2^level) + b.  Lane 0's result.
F5_DEVICE unsigned fi_wave_crc16(const uint8_t* p, long long len, int lane) {
    const long long slice = (len + 63) / 64, pad = 64 * slice - len;
    unsigned c = 0;
    for (long long i = 0; i < slice; i++) {
        const long long j = lane * slice + i - pad;
        if (j >= 0) c = fl_crc16_byte(c, p[j]);
    }
    unsigned pw = fi_x_pow_rt((int)(8 * slice));
    for (int level = 0; level < 6; level++) {
        const unsigned other = __shfl_down(c, 1 << level);
        if ((lane & ((2 << level) - 1)) == 0) c = fl_gf_mul(c, pw) ^ other;
        pw = fl_gf_mul(pw, pw);
    }
    return c;
}

// fi_restore's predicted case by the wave; true when every sample stayed inside s.depth bits.  Products are below 2^15 * 2^31 and at most 32
// are summed, so the int64 sums are exact whatever the stream holds.
F5_DEVICE bool fi_wave_restore(int32_t* x, int b, const FiSub* s, int lane) {
    const int o = s->order, depth = s->depth, shift = s->shift;
    int steps = 0;
    while ((1 << steps) < o) steps++;
    const long long coef = lane < o ? s->coef[lane] : 0;
    int hist = lane < o ? x[o - 1 - lane] : 0;
    int bad = (lane < o && !fi_in_depth(hist, depth)) ? 1 : 0;
    for (int base = o; base < b; base += 64) {
        const int cnt = min(64, b - base);
        const int res = lane < cnt ? x[base + lane] : 0;
        int out = 0;
        for (int t = 0; t < cnt; t++) {
            long long acc = coef * hist;
            for (int k = 0; k < steps; k++) acc += __shfl_xor(acc, 1 << k);
            const long long v = (long long)__shfl(res, t) + (acc >> shift);
            bad |= fi_in_depth(v, depth) ? 0 : 1;                                   // lane 0 holds the sum of all products
            const int v0 = __shfl((int)v, 0);
            hist = __shfl_up(hist, 1);
            if (lane == 0) hist = v0;
            if (lane == t) out = v0;
        }
        if (lane < cnt) x[base + lane] = out;
    }
    return __any(bad && lane < max(o, 1)) == 0;
}

__global__ __launch_bounds__(64) void flac_in_frame_kernel(const FiStream* __restrict__ streams, int n, const uint8_t* __restrict__ data,
                                                           const int* __restrict__ cbase, const long long* __restrict__ sbase,
                                                           const unsigned short* __restrict__ chunk_list, const unsigned* __restrict__ chunk_slot, int nchunks,
                                                           int maxc, long long pool_words, int32_t* __restrict__ pool, FiFrame* __restrict__ frames) {
    __shared__ FiSub subs[kFiMaxChannels];
    __shared__ FiHeader hd;
    __shared__ FiFrame rec;
    const int lane = threadIdx.x;
    const int total = min(cbase[nchunks], maxc);
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
        __syncthreads();
        if (lane == 0) {
            long long pos, slot;
            fi_candidate(id, cbase, sbase, chunk_list, chunk_slot, nchunks, &pos, &slot);
            const int s = fi_find_stream(streams, n, pos);
            rec.pos = pos; rec.end = pos; rec.slot = slot; rec.out_pos = -1; rec.status = FI_BAD; rec.block = 0; rec.code = 0; rec.stream = s;
            if (s >= 0 && fi_header(data + pos, streams[s].end - pos, streams[s].rate, streams[s].bits, hd)) {
                rec.block = hd.block; rec.code = hd.code;
                if (hd.block > kFiMaxBlock || slot + (long long)streams[s].channels * hd.block > pool_words) rec.status = FI_NEEDS_HOST;
                else rec.status = fi_frame_parse(data, pos, streams[s], hd, pool + slot, subs, &rec.end);
            }
        }
        __syncthreads();
        if (rec.status == FI_OK) {
            const int b = rec.block, channels = streams[rec.stream].channels;
            bool ok = true;
            for (int c = 0; c < channels; c++) {
                int32_t* x = pool + rec.slot + (long long)c * b;
                const FiSub* s = &subs[c];
                if (s->kind == 2) ok = fi_wave_restore(x, b, s, lane) && ok;
                __syncthreads();
                const int first = x[0], wasted = s->wasted, kind = s->kind;
                __syncthreads();
                for (int i = lane; i < b; i += 64) {
                    const int v = kind == 0 ? first : x[i];
                    x[i] = (int32_t)((long long)v * (1LL << wasted));
                }
            }
            const unsigned crc = fi_wave_crc16(data + rec.pos, rec.end - rec.pos, lane);
            if (lane == 0) {
                const unsigned stored = ((unsigned)data[rec.end] << 8) | data[rec.end + 1];
                if (!ok || crc != stored) rec.status = FI_BAD;
                rec.end += 2;
            }
        }
        __syncthreads();
        if (lane == 0) frames[id] = rec;
    }
}

__global__ __launch_bounds__(64) void flac_in_chain_kernel(const FiStream* __restrict__ streams, const uint8_t* __restrict__ data,
                                                           const unsigned short* __restrict__ cand_local, const int* __restrict__ cbase, int maxc,
                                                           FiFrame* __restrict__ frames, int32_t* __restrict__ status_out) {
    if (threadIdx.x != 0) return;
    const FiStream st = streams[blockIdx.x];
    int status = st.status;
    long long count = 0, index = 0, pos = st.begin;
    FiHeader first;
    first.variable = 0; first.block = 0;
    while (status == FI_OK && pos < st.end) {
        const unsigned local = cand_local[pos];
        FiHeader h;
        if (local == 0xFFFFu || !fi_header(data + pos, st.end - pos, st.rate, st.bits, h)) { status = FI_BAD; break; }
        const long long id = (long long)cbase[pos / kFiChunk] + local;
        if (id >= maxc) { status = FI_NEEDS_HOST; break; }
        if (index == 0) first = h;
        const FiFrame f = frames[id];
        status = fi_chain_step(st, h, first, f, index, count);
        if (status != FI_OK || f.end <= pos) { if (status == FI_OK) status = FI_BAD; break; }
        frames[id].out_pos = count;
        count += h.block; index += 1; pos = f.end;
    }
    if (status == FI_OK && st.total && st.total != count) status = FI_BAD;
    status_out[2 * blockIdx.x] = status;
    status_out[2 * blockIdx.x + 1] = (int32_t)count;
}

__global__ __launch_bounds__(256) void flac_in_pack_kernel(const FiStream* __restrict__ streams, const int* __restrict__ cbase, int nchunks, int maxc,
                                                           const FiFrame* __restrict__ frames, const int32_t* __restrict__ pool, int32_t* __restrict__ out,
                                                           int32_t* __restrict__ status_out) {
    const int total = min(cbase[nchunks], maxc);
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
        const FiFrame f = frames[id];
        if (f.out_pos < 0 || f.status != FI_OK) continue;
        const FiStream st = streams[f.stream];
        if (f.out_pos + f.block > st.cap) continue;                                 // (the chain admitted it, so never)
        const int32_t* a = pool + f.slot;
        int32_t* o = out + st.out_off + f.out_pos;
        bool bad = false;
        if (st.channels == 1) {
            for (int i = threadIdx.x; i < f.block; i += 256) o[i] = a[i];
        } else {
            const int32_t* b = a + f.block;
            for (int i = threadIdx.x; i < f.block; i += 256) {
                int32_t l, r;
                if (!fi_unstereo(f.code, a[i], b[i], st.bits, &l, &r)) bad = true;
                o[i] = l; o[(long long)st.cap + i] = r;
            }
        }
        if (bad) atomicOr(&status_out[2 * f.stream], FI_BAD);                      // (the same value whichever thread gets there first)
    }
}

struct FiWorkspace {
    FiStream* streams = nullptr; size_t cap_streams = 0;
    unsigned short* cand_local = nullptr; size_t cap_local = 0;
    unsigned short* chunk_list = nullptr; size_t cap_list = 0;
    unsigned* chunk_slot = nullptr; size_t cap_slot = 0;
    int* chunk_count = nullptr; size_t cap_count = 0;
    long long* chunk_words = nullptr; size_t cap_words = 0;
    int* cbase = nullptr; size_t cap_cbase = 0;
    long long* sbase = nullptr; size_t cap_sbase = 0;
    FiFrame* frames = nullptr; size_t cap_frames = 0;
    int32_t* pool = nullptr; size_t cap_pool = 0;
    WorkspaceUse use;
};

// samples per channel the output must have room for: STREAMINFO's total, or for a stream that does not name it twice its bytes plus a block;
// never more than 64 samples per byte plus a block
int64_t f5hip_flac_decode_bound(int64_t total, int64_t stream_bytes, int64_t max_samples) {
    if (total < 0 || stream_bytes < 0 || max_samples < 0) return 0;
    const long long guess = 2LL * stream_bytes + kFiMaxBlock, most = 64LL * stream_bytes + kFiMaxBlock;
    long long want = total ? total : guess;
    if (want > most) want = most;                         // (memory stays in proportion to the upload, whatever STREAMINFO declares)
    return want < max_samples ? want : max_samples;
}

int f5hip_flac_decode(int32_t n, const uint8_t* data_dev, int64_t nbytes, const int64_t* begin, const int64_t* end, const int32_t* info,
                      const int64_t* total, const int64_t* max_samples, int32_t* out_dev, const int64_t* out_off, int32_t* status_dev, void* stream) {
    if (n < 1 || !data_dev || !begin || !end || !info || !total || !max_samples || !out_dev || !out_off || !status_dev)
        return fail(-1, "flac_decode: bad argument");
    if (nbytes < 1 || nbytes > 2147483647LL - kFiChunk) return fail(-1, "flac_decode: the packed buffer must hold 1 .. 2^31 - 1025 bytes (got %lld)", (long long)nbytes);
    if ((reinterpret_cast<uintptr_t>(out_dev) & 3) || (reinterpret_cast<uintptr_t>(status_dev) & 3)) return fail(-1, "flac_decode: the outputs must be 4-byte aligned");
    std::vector<FiStream> h(n);
    long long pool_words = kFiPoolSlack, prev_end = 0;
    for (int i = 0; i < n; i++) {
        const int32_t* f = info + 8 * i;   // channels, bits, rate, min_block, max_block, cap, needs_host, 0
        if (begin[i] < prev_end || end[i] < begin[i] || end[i] > nbytes)
            return fail(-1, "flac_decode: stream %d's bytes [%lld, %lld) overlap the stream before it or leave the buffer of %lld", i, (long long)begin[i],
                        (long long)end[i], (long long)nbytes);
        prev_end = end[i];
        if (f[0] < 1 || f[0] > 8 || f[1] < 4 || f[1] > 32 || f[2] < 1 || f[3] < 0 || f[3] > 65535 || f[4] < 0 || f[4] > 65535 || f[5] < 0 || total[i] < 0 ||
            max_samples[i] < 0 || out_off[i] < 0)
            return fail(-1, "flac_decode: stream %d's STREAMINFO fields are out of range", i);
        const bool host = f[6] != 0 || f[0] > kFiMaxChannels || f[1] < kFiMinBits || f[1] > kFiMaxBits;
        FiStream s;
        s.begin = begin[i]; s.end = end[i]; s.out_off = out_off[i]; s.total = total[i]; s.max_samples = max_samples[i]; s.cap = f[5];
        s.channels = f[0]; s.bits = f[1]; s.rate = f[2]; s.min_block = f[3]; s.max_block = f[4]; s.status = host ? FI_NEEDS_HOST : FI_OK;
        h[i] = s;
        if (!host) pool_words += (long long)f[0] * f[5];
        if (pool_words > (1LL << 40)) return fail(-1, "flac_decode: the call's streams declare more samples than one call takes");
    }
    const int nchunks = (int)((nbytes + kFiChunk - 1) / kFiChunk);
    const int maxc = (int)(nbytes / 8 + 1024);
    FiWorkspace* const wsp = device_workspace<FiWorkspace>("flac_decode");
    if (!wsp) return -6;
    FiWorkspace& ws = *wsp;
    hipStream_t st = (hipStream_t)stream;
    WorkspaceTurn turn(ws.use, st);
    CK(turn.rc);
    CK(dev_reserve(&ws.streams, &ws.cap_streams, (size_t)n, "flac_decode streams"));
    CK(dev_reserve(&ws.cand_local, &ws.cap_local, (size_t)nbytes, "flac_decode candidate map"));
    CK(dev_reserve(&ws.chunk_list, &ws.cap_list, (size_t)nchunks * kFiChunk, "flac_decode candidate lists"));
    CK(dev_reserve(&ws.chunk_slot, &ws.cap_slot, (size_t)nchunks * kFiChunk, "flac_decode slot prefixes"));
    CK(dev_reserve(&ws.chunk_count, &ws.cap_count, (size_t)nchunks, "flac_decode chunk counts"));
    CK(dev_reserve(&ws.chunk_words, &ws.cap_words, (size_t)nchunks, "flac_decode chunk slot totals"));
    CK(dev_reserve(&ws.cbase, &ws.cap_cbase, (size_t)nchunks + 1, "flac_decode candidate bases"));
    CK(dev_reserve(&ws.sbase, &ws.cap_sbase, (size_t)nchunks, "flac_decode slot bases"));
    CK(dev_reserve(&ws.frames, &ws.cap_frames, (size_t)maxc, "flac_decode frame records"));
    CK(dev_reserve(&ws.pool, &ws.cap_pool, (size_t)pool_words, "flac_decode slot pool"));
    if (upload_sync(st, ws.streams, h) != hipSuccess) return fail(-6, "flac_decode metadata upload");
    hipLaunchKernelGGL(flac_in_scan_kernel, dim3((unsigned)nchunks), dim3(kFiChunk), 0, st, ws.streams, n, (const uint8_t*)data_dev, (long long)nbytes,
                       ws.cand_local, ws.chunk_list, ws.chunk_slot, ws.chunk_count, ws.chunk_words);
    CKL("flac_in_scan");
    hipLaunchKernelGGL(flac_in_offsets_kernel, dim3(1), dim3(256), 0, st, ws.chunk_count, ws.chunk_words, nchunks, ws.cbase, ws.sbase);
    CKL("flac_in_offsets");
    const unsigned grid = (unsigned)(maxc < kFiGrid ? maxc : kFiGrid);
    hipLaunchKernelGGL(flac_in_frame_kernel, dim3(grid), dim3(64), 0, st, ws.streams, n, (const uint8_t*)data_dev, ws.cbase, ws.sbase, ws.chunk_list,
                       ws.chunk_slot, nchunks, maxc, pool_words, ws.pool, ws.frames);
    CKL("flac_in_frame");
    hipLaunchKernelGGL(flac_in_chain_kernel, dim3((unsigned)n), dim3(64), 0, st, ws.streams, (const uint8_t*)data_dev, ws.cand_local, ws.cbase, maxc, ws.frames,
                       (int32_t*)status_dev);
    CKL("flac_in_chain");
    hipLaunchKernelGGL(flac_in_pack_kernel, dim3(grid), dim3(256), 0, st, ws.streams, ws.cbase, nchunks, maxc, ws.frames, ws.pool, (int32_t*)out_dev,
                       (int32_t*)status_dev);
    CKL("flac_in_pack");
    g_counters[CNT_FLAC_DECODE_LAUNCHES] += 5;
    g_counters[CNT_FLAC_DECODE_STREAMS] += n;
    return 0;
}
