// The device FLAC decoder's steps (csrc/flac_in.h: scan, offsets, frame, chain, pack) run serially on the CPU over csrc/flac_in_core.h, the
// same text the kernels compile.  Built with -fsanitize=address,undefined, this is the evidence for the core's bounds: every stream lives in a
// heap block of exactly its size and every pool and output in one of exactly the size the library would give it, so a read past a stream's
// end or a write past a slot is a sanitizer report.  tests/test_flac_in_core.py builds and runs it.
//
//   flac_in_check OUT FILE...      one line "status count channels" per FILE on stdout; the int32 planes [channels, count] of every stream
//                                  with status 0 appended to OUT, in order
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tts-indic-server-f5_amd/csrc/flac_in_core.h"

static const long long kMaxSeconds = 600;                      // wave_codec.FLAC_MAX_SECONDS
static const long long kPoolSlack = 64LL * kFiMaxChannels * kFiMaxBlock;

// wave_codec.flac_stream_info: false for a refusal
static bool stream_info(const uint8_t* d, long long n, FiStream& st, long long& first) {
    if (n < 4 || memcmp(d, "fLaC", 4)) return false;
    long long pos = 4;
    bool have = false;
    const uint8_t* info = nullptr;
    for (;;) {
        if (pos + 4 > n) return false;
        const int kind = d[pos] & 0x7F, last = d[pos] >> 7;
        const long long size = ((long long)d[pos + 1] << 16) | (d[pos + 2] << 8) | d[pos + 3];
        pos += 4;
        if (pos + size > n) return false;
        if (!have) {
            if (kind != 0 || size != 34) return false;
            info = d + pos; have = true;
        }
        pos += size;
        if (last) break;
    }
    unsigned long long word = 0;
    for (int i = 10; i < 18; i++) word = (word << 8) | info[i];
    st.min_block = (info[0] << 8) | info[1]; st.max_block = (info[2] << 8) | info[3];
    st.rate = (int)(word >> 44); st.channels = (int)((word >> 41) & 7) + 1; st.bits = (int)((word >> 36) & 31) + 1;
    st.total = (long long)(word & ((1ULL << 36) - 1));
    if (st.bits < 4 || st.rate == 0) return false;
    st.max_samples = kMaxSeconds * st.rate;
    if (st.total > st.max_samples) return false;
    first = pos;
    return true;
}

static long long decode_bound(long long total, long long bytes, long long max_samples) {   // f5hip_flac_decode_bound
    long long want = total ? total : 2 * bytes + kFiMaxBlock;
    if (want > 64 * bytes + kFiMaxBlock) want = 64 * bytes + kFiMaxBlock;
    return want < max_samples ? want : max_samples;
}

static unsigned crc16(const uint8_t* p, long long n) {
    unsigned c = 0;
    for (long long i = 0; i < n; i++) c = fi_crc16_byte(c, p[i]);
    return c;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: flac_in_check OUT FILE...\n"); return 2; }
    FILE* out = fopen(argv[1], "wb");
    if (!out) { perror(argv[1]); return 2; }
    for (int a = 2; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { perror(argv[a]); return 2; }
        fseek(f, 0, SEEK_END);
        const long long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t* data = (uint8_t*)malloc(n ? n : 1);             // exactly the stream: the sanitizer guards its end
        if (n && fread(data, 1, n, f) != (size_t)n) { perror(argv[a]); return 2; }
        fclose(f);

        FiStream st;
        memset(&st, 0, sizeof(st));
        long long first = 0;
        int status = FI_OK;
        long long count = 0;
        int32_t* planes = nullptr;
        if (!stream_info(data, n, st, first)) status = FI_BAD;
        else if (st.channels > kFiMaxChannels || st.bits < kFiMinBits || st.bits > kFiMaxBits) status = FI_NEEDS_HOST;
        if (status == FI_OK) {
            st.begin = first; st.end = n; st.out_off = 0; st.status = FI_OK;
            st.cap = (int)decode_bound(st.total, st.end - st.begin, st.max_samples);
            const long long pool_words = kPoolSlack + (long long)st.channels * st.cap;
            const long long maxc = n / 8 + 1024;
            // scan + offsets: candidates in offset order, their slots one behind the other
            std::vector<int> cand(n, -1);
            std::vector<long long> cpos, cslot;
            long long words = 0;
            for (long long pos = st.begin; pos < st.end; pos++) {
                FiHeader h;
                if (!fi_header(data + pos, st.end - pos, st.rate, st.bits, h)) continue;
                cand[pos] = (int)cpos.size();
                cpos.push_back(pos); cslot.push_back(words);
                words += h.block <= kFiMaxBlock ? (long long)st.channels * h.block : 0;
            }
            const long long total = (long long)cpos.size() < maxc ? (long long)cpos.size() : maxc;
            int32_t* pool = (int32_t*)malloc(sizeof(int32_t) * pool_words);
            std::vector<FiFrame> frames(total);
            // frame
            for (long long id = 0; id < total; id++) {
                FiFrame rec;
                FiHeader hd;
                FiSub subs[kFiMaxChannels];
                const long long pos = cpos[id], slot = cslot[id];
                rec.pos = pos; rec.end = pos; rec.slot = slot; rec.out_pos = -1; rec.status = FI_BAD; rec.block = 0; rec.code = 0; rec.stream = 0;
                if (fi_header(data + pos, st.end - pos, st.rate, st.bits, hd)) {
                    rec.block = hd.block; rec.code = hd.code;
                    if (hd.block > kFiMaxBlock || slot + (long long)st.channels * hd.block > pool_words) rec.status = FI_NEEDS_HOST;
                    else rec.status = fi_frame_parse(data, pos, st, hd, pool + slot, subs, &rec.end);
                }
                if (rec.status == FI_OK) {
                    bool ok = true;
                    for (int c = 0; c < st.channels && ok; c++) ok = fi_restore(pool + slot + (long long)c * rec.block, rec.block, subs[c]);
                    const unsigned stored = ((unsigned)data[rec.end] << 8) | data[rec.end + 1];
                    if (!ok || crc16(data + pos, rec.end - pos) != stored) rec.status = FI_BAD;
                    rec.end += 2;
                }
                frames[id] = rec;
            }
            // chain
            {
                long long index = 0, pos = st.begin;
                FiHeader firsth;
                memset(&firsth, 0, sizeof(firsth));
                while (status == FI_OK && pos < st.end) {
                    FiHeader h;
                    if (cand[pos] < 0 || !fi_header(data + pos, st.end - pos, st.rate, st.bits, h)) { status = FI_BAD; break; }
                    const long long id = cand[pos];
                    if (id >= maxc) { status = FI_NEEDS_HOST; break; }
                    if (index == 0) firsth = h;
                    const FiFrame fr = frames[id];
                    status = fi_chain_step(st, h, firsth, fr, index, count);
                    if (status != FI_OK || fr.end <= pos) { if (status == FI_OK) status = FI_BAD; break; }
                    frames[id].out_pos = count;
                    count += h.block; index += 1; pos = fr.end;
                }
                if (status == FI_OK && st.total && st.total != count) status = FI_BAD;
            }
            // pack
            planes = (int32_t*)malloc(sizeof(int32_t) * ((long long)st.channels * st.cap + 1));
            for (long long id = 0; id < total; id++) {
                const FiFrame& fr = frames[id];
                if (fr.out_pos < 0 || fr.status != FI_OK || fr.out_pos + fr.block > st.cap) continue;
                const int32_t* pa = pool + fr.slot;
                int32_t* o = planes + fr.out_pos;
                if (st.channels == 1) {
                    for (int i = 0; i < fr.block; i++) o[i] = pa[i];
                } else {
                    const int32_t* pb = pa + fr.block;
                    for (int i = 0; i < fr.block; i++) {
                        int32_t l, r;
                        if (!fi_unstereo(fr.code, pa[i], pb[i], st.bits, &l, &r)) status |= FI_BAD;
                        o[i] = l; o[(long long)st.cap + i] = r;
                    }
                }
            }
            free(pool);
        }
        printf("%d %lld %d\n", status, status == FI_OK ? count : 0LL, st.channels);
        if (status == FI_OK)
            for (int c = 0; c < st.channels; c++) fwrite(planes + (long long)c * st.cap, sizeof(int32_t), count, out);
        free(planes);
        free(data);
    }
    fclose(out);
    return 0;
}
