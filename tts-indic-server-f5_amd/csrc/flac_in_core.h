// FLAC in, the part with no HIP in it: the bit reader and the per-frame arithmetic of the device decoder (flac_in.h, f5hip_flac_decode),
// as inline functions that a plain host compiler takes too.  tools/flac_in_check.cpp runs the same scan / frame / chain / pack steps
// serially over files under AddressSanitizer and UBSan; that CPU run is the evidence for the bounds below.  The definition of every rule
// here is wave_codec.read_flac: a stream is accepted by the one iff by the other, with the same samples.
//
// Bounds, in one place:
//   reads   every byte read goes through FiBits (bounded by `end`, the stream's last bit) or fi_header (bounded by `avail`)
//   unary   fi_unary stops at `end`
//   writes  a subframe writes x[0 .. b) of its plane; the caller hands planes of b words (its slot is channels * b)
//   loops   every loop runs to the header's block size b <= kFiMaxBlock, to an order <= 32 or to a partition count <= b
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FI_HD __host__ __device__ inline
#else
#define FI_HD inline
#endif

constexpr int kFiMaxBlock = 16384;      // the device's limits: larger blocks, more channels and other depths are decoded on the host
constexpr int kFiMaxChannels = 2;
constexpr int kFiMinBits = 8, kFiMaxBits = 24;
constexpr int kFiChunk = 1024;          // bytes per scan block: candidates are numbered chunk by chunk

enum { FI_OK = 0, FI_BAD = 1, FI_NEEDS_HOST = 2 };

struct FiStream {            // one stream of the call, filled on the host from STREAMINFO
    long long begin, end;    // its frames: bytes [begin, end) of the packed buffer
    long long out_off;       // its planes in the output: channel c at out_off + c * cap
    long long total;         // STREAMINFO's total samples, 0: unknown
    long long max_samples;   // the cap on decoded samples (FLAC_MAX_SECONDS * rate)
    int cap;                 // samples per channel the output has room for
    int channels, bits, rate, min_block, max_block;
    int status;              // FI_NEEDS_HOST before any launch for a stream outside the limits
};

struct FiHeader {
    int variable, block, rate, code, channels, bits, size;   // size: header bytes, CRC-8 included
    unsigned long long number;
};

struct FiSub {               // one parsed subframe: its plane holds warm-up samples and residuals until fi_restore
    int kind;                // 0 CONSTANT, 1 VERBATIM, 2 predicted
    int order, shift, wasted, depth;   // depth: bits of a sample before the wasted-bits shift
    int coef[32];
};

struct FiFrame {             // what the frame step leaves per candidate
    long long pos, end;      // its first byte and the byte after its CRC-16
    long long slot;          // its planes in the pool: channel c at slot + c * block
    long long out_pos;       // its first sample in the stream, -1 until the chain visits it
    int status, block, code, stream;
};

FI_HD unsigned fi_crc8_byte(unsigned c, unsigned byte) {
    c ^= byte;
    for (int i = 0; i < 8; i++) c = ((c << 1) ^ ((c & 0x80u) ? 0x07u : 0u)) & 0xffu;
    return c;
}
FI_HD unsigned fi_crc16_byte(unsigned c, unsigned byte) {
    c ^= byte << 8;
    for (int i = 0; i < 8; i++) c = ((c << 1) ^ ((c & 0x8000u) ? 0x8005u : 0u)) & 0xffffu;
    return c;
}

// The frame header at p, of which `avail` bytes may be read.  False: no frame starts here (sync, a reserved code, the coded number,
// the CRC-8, or fewer bytes than the header needs).
FI_HD bool fi_header(const uint8_t* p, long long avail, int info_rate, int info_bits, FiHeader& h) {
    if (avail < 6 || p[0] != 0xFF || (p[1] & 0xFE) != 0xF8) return false;
    h.variable = p[1] & 1;
    const int bs = p[2] >> 4, rc = p[2] & 15, ch = p[3] >> 4, sz = (p[3] >> 1) & 7;
    if (bs == 0 || rc == 15 || ch > 10 || sz == 3 || (p[3] & 1)) return false;
    const unsigned lead = p[4];
    int extra;
    if (lead < 0x80) extra = 0;
    else if (lead < 0xC0 || lead > (h.variable ? 0xFEu : 0xFCu)) return false;
    else extra = lead < 0xE0 ? 1 : lead < 0xF0 ? 2 : lead < 0xF8 ? 3 : lead < 0xFC ? 4 : lead < 0xFE ? 5 : 6;
    const int tail = (bs == 6 ? 1 : bs == 7 ? 2 : 0) + (rc == 12 ? 1 : rc == 13 || rc == 14 ? 2 : 0);
    const int size = 5 + extra + tail + 1;
    if (avail < size) return false;
    unsigned long long number = extra ? (lead & (0x7Fu >> (extra + 1))) : lead;
    int at = 5;
    for (int i = 0; i < extra; i++, at++) {
        if ((p[at] >> 6) != 2) return false;
        number = (number << 6) | (p[at] & 0x3Fu);
    }
    int block;
    if (bs == 6) { block = p[at] + 1; at += 1; }
    else if (bs == 7) { block = ((p[at] << 8) | p[at + 1]) + 1; at += 2; }
    else block = bs == 1 ? 192 : bs <= 5 ? 576 << (bs - 2) : 256 << (bs - 8);
    if (block > 65535) return false;
    int rate;
    if (rc == 0) rate = info_rate;
    else if (rc == 12) { rate = p[at] * 1000; at += 1; }
    else if (rc == 13) { rate = (p[at] << 8) | p[at + 1]; at += 2; }
    else if (rc == 14) { rate = ((p[at] << 8) | p[at + 1]) * 10; at += 2; }
    else {
        const int table[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
        rate = table[rc];
    }
    unsigned c = 0;
    for (int i = 0; i < at; i++) c = fi_crc8_byte(c, p[i]);
    if (c != p[at]) return false;
    const int sizes[8] = {0, 8, 12, 0, 16, 20, 24, 32};
    h.block = block; h.rate = rate; h.code = ch; h.channels = ch < 8 ? ch + 1 : 2; h.bits = sz ? sizes[sz] : info_bits;
    h.size = size; h.number = number;
    return true;
}

struct FiBits {
    const uint8_t* p;        // bit 0 is the most significant bit of p[0]
    long long pos, end;      // in bits; nothing at or past `end` is read
    bool ok;                 // false once a read ran past `end`
};

FI_HD uint64_t fi_read(FiBits& r, int n) {                     // n in 0 .. 40
    if (n == 0) return 0;
    if (!r.ok || r.pos + n > r.end) { r.ok = false; return 0; }
    const long long first = r.pos >> 3;
    const int lead = (int)(r.pos & 7), bytes = (lead + n + 7) >> 3;   // <= 6
    uint64_t v = 0;
    for (int i = 0; i < bytes; i++) v = (v << 8) | r.p[first + i];
    r.pos += n;
    return (v >> (8 * bytes - lead - n)) & ((1ULL << n) - 1ULL);
}
FI_HD long long fi_signed(FiBits& r, int n) {                  // n in 0 .. 40
    if (n == 0) return 0;
    const uint64_t v = fi_read(r, n);
    return (v >> (n - 1)) ? (long long)v - (long long)(1ULL << n) : (long long)v;
}
// zero bits up to the next one bit, which is consumed; -1 (and !ok) when the stream ends first
FI_HD long long fi_unary(FiBits& r) {
    if (!r.ok) return -1;
    long long pos = r.pos;
    while (pos < r.end) {
        const int lead = (int)(pos & 7);
        const unsigned rest = (unsigned)(r.p[pos >> 3] << lead) & 0xFFu;    // the byte's bits from `pos` on, left-aligned in 8
        if (rest) {
            int z = 0;
            while (!((rest << z) & 0x80u)) z++;
            pos += z;
            if (pos >= r.end) break;
            const long long zeros = pos - r.pos;
            r.pos = pos + 1;
            return zeros;
        }
        pos += 8 - lead;
    }
    r.ok = false;
    return -1;
}

// The residuals of a predicted subframe of order o into x[o .. b).  False: a refusal (a reserved method, a partition order that does not
// fit, a residual outside 32 bits, the stream's end).
FI_HD bool fi_residual(FiBits& r, int32_t* x, int b, int o) {
    const int method = (int)fi_read(r, 2);
    if (!r.ok || method > 1) return false;
    const int pbits = 4 + method, porder = (int)fi_read(r, 4);
    if (!r.ok || (b & ((1 << porder) - 1)) || (b >> porder) < o) return false;
    const int plen = b >> porder;
    int i = o;
    for (int part = 0; part < (1 << porder); part++) {
        const int n = plen - (part == 0 ? o : 0);
        const int k = (int)fi_read(r, pbits);
        if (!r.ok) return false;
        if (k == (1 << pbits) - 1) {
            const int raw = (int)fi_read(r, 5);
            for (int j = 0; j < n; j++, i++) x[i] = (int32_t)fi_signed(r, raw);
            if (!r.ok) return false;
            continue;
        }
        for (int j = 0; j < n; j++, i++) {
            const long long q = fi_unary(r);
            const uint64_t low = fi_read(r, k);
            if (!r.ok) return false;
            const uint64_t u = ((uint64_t)q << k) | low;          // q < 2^40 bits of stream, k <= 30
            if (u > 0xFFFFFFFFULL) return false;
            x[i] = (int32_t)((u & 1) ? -(long long)(u >> 1) - 1 : (long long)(u >> 1));
        }
    }
    return true;
}

// One subframe of b samples at `depth` bits: the header into s, warm-up samples and residuals (or the VERBATIM samples, or the CONSTANT
// value at x[0]) into x[0 .. b).  depth <= kFiMaxBits + 1, so everything fits an int32.
FI_HD bool fi_subframe(FiBits& r, int32_t* x, int b, int depth, FiSub& s) {
    if (fi_read(r, 1) || !r.ok) return false;
    const int type = (int)fi_read(r, 6);
    int wasted = (int)fi_read(r, 1);
    if (wasted) {
        const long long z = fi_unary(r);
        if (!r.ok || z >= 64) return false;
        wasted = (int)z + 1;
    }
    if (!r.ok) return false;
    depth -= wasted;
    if (depth < 1) return false;
    s.wasted = wasted; s.depth = depth; s.order = 0; s.shift = 0;
    if (type == 0) {
        s.kind = 0;
        x[0] = (int32_t)fi_signed(r, depth);
        return r.ok;
    }
    if (type == 1) {
        s.kind = 1;
        for (int i = 0; i < b && r.ok; i++) x[i] = (int32_t)fi_signed(r, depth);
        return r.ok;
    }
    int o;
    if (type >= 8 && type <= 12) o = type - 8;
    else if (type >= 32) o = type - 31;
    else return false;
    if (o > b) return false;
    s.kind = 2; s.order = o;
    for (int i = 0; i < o; i++) x[i] = (int32_t)fi_signed(r, depth);
    if (!r.ok) return false;
    if (type < 32) {
        const int fixed[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
        for (int j = 0; j < o; j++) s.coef[j] = fixed[o][j];
    } else {
        const int precision = (int)fi_read(r, 4) + 1;
        if (!r.ok || precision == 16) return false;
        const int shift = (int)fi_signed(r, 5);
        if (!r.ok || shift < 0) return false;
        s.shift = shift;
        for (int j = 0; j < o; j++) s.coef[j] = (int)fi_signed(r, precision);
        if (!r.ok) return false;
    }
    return fi_residual(r, x, b, o);
}

FI_HD bool fi_in_depth(long long v, int depth) { return v >= -(1LL << (depth - 1)) && v <= (1LL << (depth - 1)) - 1; }

// Warm-up + residuals -> samples, in place, then the wasted-bits shift.  False at the first sample outside s.depth bits: nothing is built
// on such a value, so the int64 sums stay below 32 * 2^15 * 2^25.
FI_HD bool fi_restore(int32_t* x, int b, const FiSub& s) {
    if (s.kind == 0) {
        for (int i = 1; i < b; i++) x[i] = x[0];
    } else if (s.kind == 2) {
        for (int i = 0; i < s.order; i++) if (!fi_in_depth(x[i], s.depth)) return false;
        for (int i = s.order; i < b; i++) {
            long long acc = 0;
            for (int j = 0; j < s.order; j++) acc += (long long)s.coef[j] * x[i - 1 - j];
            const long long v = (long long)x[i] + (acc >> s.shift);
            if (!fi_in_depth(v, s.depth)) return false;
            x[i] = (int32_t)v;
        }
    }
    if (s.wasted) for (int i = 0; i < b; i++) x[i] = (int32_t)((long long)x[i] * (1LL << s.wasted));
    return true;
}

FI_HD bool fi_side(int code, int channel) { return ((code == 8 || code == 10) && channel == 1) || (code == 9 && channel == 0); }

// The subframes of the frame at `pos` (header h) of stream st into planes of h.block words at `slot`, bounded by the stream's end.
// Returns the status and, when FI_OK, *body_end: the byte where the CRC-16 stands.
FI_HD int fi_frame_parse(const uint8_t* data, long long pos, const FiStream& st, const FiHeader& h, int32_t* slot, FiSub* subs, long long* body_end) {
    if (h.channels != st.channels || h.bits != st.bits) return FI_BAD;
    if (h.block > kFiMaxBlock) return FI_NEEDS_HOST;
    FiBits r;
    r.p = data + pos + h.size; r.pos = 0; r.end = 8 * (st.end - pos - h.size); r.ok = true;
    for (int c = 0; c < h.channels; c++)
        if (!fi_subframe(r, slot + (long long)c * h.block, h.block, h.bits + (fi_side(h.code, c) ? 1 : 0), subs[c])) return FI_BAD;
    const long long end = pos + h.size + ((r.pos + 7) >> 3);
    if (end + 2 > st.end) return FI_BAD;
    *body_end = end;
    return FI_OK;
}

// One step of the chain: the frame at `pos` (header h, record f) as frame `index` of stream st after `count` samples, whose first frame
// had header `first`.  Returns the stream's status so far.
FI_HD int fi_chain_step(const FiStream& st, const FiHeader& h, const FiHeader& first, const FiFrame& f, long long index, long long count) {
    if (h.channels != st.channels || h.bits != st.bits || h.rate != st.rate) return FI_BAD;
    if (h.variable != first.variable) return FI_BAD;
    if (h.number != (unsigned long long)(h.variable ? count : index)) return FI_BAD;
    if (st.max_block && h.block > st.max_block) return FI_BAD;
    if (count + h.block > st.max_samples) return FI_BAD;
    if (f.status != FI_OK) return f.status;
    if (f.end < st.end) {
        if (h.block < st.min_block) return FI_BAD;
        if (!h.variable && h.block != first.block) return FI_BAD;
    }
    if (count + h.block > st.cap) return FI_NEEDS_HOST;
    return FI_OK;
}

// Sample i of a frame's two coded planes a, b -> (left, right); false when either leaves `bits`.
FI_HD bool fi_unstereo(int code, long long a, long long b, int bits, int32_t* left, int32_t* right) {
    long long l = a, r = b;
    if (code == 8) r = a - b;
    else if (code == 9) l = a + b;
    else if (code == 10) {
        const long long m = a * 2 + (b & 1);
        l = (m + b) >> 1; r = (m - b) >> 1;
    }
    *left = (int32_t)l; *right = (int32_t)r;
    return code < 8 || (fi_in_depth(l, bits) && fi_in_depth(r, bits));
}
