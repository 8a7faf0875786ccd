// flac_core.hpp — the frame-level FLAC decode shared by the host decoder (host_flac.hip), the CPU
// phased decode (sdsp_debug_flac_decode_phased) and the device kernels (k_flac.hip).
//
// Everything here is `__host__ __device__` under hipcc and plain inline C++ under any other
// compiler (tools/flac_core_check.cpp builds it with the host sanitizers).  The functions work on
// caller-supplied buffers only: no allocation, no std::vector, no std::string.
//
// Bounds, which hold for every input:
//   * every loop is bounded by a header field (block size <= 65536, channels <= 8, order <= 32,
//     partitions <= 2^15) or by the length of the file's bytes;
//   * every read goes through Bits / the (pointer, length) pair of the CRCs and is checked against
//     the end of the file's bytes;
//   * every write goes through Work (the candidate's own integer work range, `cap` samples) or to
//     the `bs` floats the caller reserved for the frame; decode_frame refuses a frame whose
//     channels x block size exceeds `cap` before the first write.
// A malformed stream ends as "frame rejected" (false / 0), never as an out-of-range access.
//
// Arithmetic is the host decoder's: 64-bit samples, a 128-bit LPC sum, wrapping shifts.  A stream
// whose CRCs hold may still carry residuals far outside its bits per sample; host and device then
// compute the same wrapped values, because they run this same code.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FLAC_HD __host__ __device__ inline
#else
#define FLAC_HD inline
#endif

namespace flac_core {

// Big-endian bit reader over p[0 .. n) with a held 64-bit window: the 8 bytes at byte `cat`, loaded
// again only when a read leaves them (pos never moves back).  Running past the end sets `bad` and
// returns 0; every caller checks `bad` before it accepts anything read after that point.
struct Bits {
    const uint8_t* p;
    size_t n, pos;  // pos in bits
    bool bad;
    uint64_t cw;  // window(cat)
    size_t cat;   // cat * 8 <= pos
    FLAC_HD Bits(const uint8_t* d, size_t len) : p(d), n(len), pos(0), bad(false), cw(0), cat(0) { cw = window(0); }
    // the 8 bytes at byte offset `at`, first byte in the top bits; bytes past the end read as 0
    FLAC_HD uint64_t window(size_t at) const {
        uint64_t w = 0;
        if (at + 8 <= n) {
            uint64_t le;
            __builtin_memcpy(&le, p + at, 8);
            return __builtin_bswap64(le);
        }
        for (size_t i = 0; i < 8; i++) w = (w << 8) | (at + i < n ? (uint64_t)p[at + i] : 0u);
        return w;
    }
    FLAC_HD uint64_t get(int k) {  // 0 <= k <= 57
        if (k <= 0) return 0;
        if (pos + (size_t)k > n * 8) {
            bad = true;
            pos = n * 8;
            return 0;
        }
        size_t off = pos - cat * 8;
        if (off + (size_t)k > 64) {  // k <= 57 fits behind any bit of the window's first byte
            cat = pos >> 3;
            cw = window(cat);
            off = pos & 7;
        }
        pos += (size_t)k;
        return (cw << off) >> (64 - k);
    }
    FLAC_HD int64_t sget(int k) {  // two's complement, k <= 57
        if (k <= 0) return 0;
        const uint64_t v = get(k);
        return (v >> (k - 1)) & 1u ? (int64_t)(v - (1ull << k)) : (int64_t)v;
    }
    FLAC_HD uint64_t unary() {  // zeros before the terminating 1
        uint64_t q = 0;
        for (;;) {  // each turn but the first loads a new window, takes what is left of the held one, or returns
            if (pos >= n * 8) {
                bad = true;
                return 0;
            }
            size_t off = pos - cat * 8;
            if (off >= 64) {
                cat = pos >> 3;
                cw = window(cat);
                off = pos & 7;
            }
            const uint64_t w = cw << off;
            if (w == 0) {  // zeros up to the end of the window (bytes past the end read as 0)
                q += (uint64_t)(64 - off);
                pos += 64 - off;
                continue;
            }
            const int lz = __builtin_clzll(w);  // the 1 bit is a real bit: padding holds none
            q += (uint64_t)lz;
            pos += (size_t)lz + 1;
            return q;
        }
    }
    FLAC_HD void align() { pos = (pos + 7) & ~(size_t)7; }
};

FLAC_HD uint8_t crc8(const uint8_t* d, size_t n) {  // polynomial x^8 + x^2 + x + 1
    uint8_t c = 0;
    for (size_t i = 0; i < n; i++) {
        c ^= d[i];
        for (int b = 0; b < 8; b++) c = (uint8_t)((c & 0x80) ? (c << 1) ^ 0x07 : c << 1);
    }
    return c;
}
// Polynomial x^16 + x^15 + x^2 + 1, a byte per step: with t = (c >> 8) ^ byte, t(x) x^16 mod P is
// (parity(t) ? 0x8003 : 0) ^ (t << 2) ^ (t << 1) (the bitwise remainder, folded; checked against the
// bit-at-a-time form for every (c, byte) in tools/flac_core_check.cpp).
FLAC_HD uint16_t crc16(const uint8_t* d, size_t n) {
    uint32_t c = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t t = ((c >> 8) ^ d[i]) & 0xFFu;
        const uint32_t par = (uint32_t)__builtin_popcount(t) & 1u;
        c = ((c << 8) ^ (par ? 0x8003u : 0u) ^ (t << 2) ^ (t << 1)) & 0xFFFFu;
    }
    return (uint16_t)c;
}

// A candidate's integer work range: sample i of channel c is p[(c * bs + i) * stride], `cap` samples
// in all.  The host uses stride 1; a wave of the device kernel interleaves its 64 lanes (stride 64,
// p offset by the lane) so that lanes advancing together touch adjacent addresses.
struct Work {
    int64_t* p;
    size_t stride, cap;
    FLAC_HD int64_t& at(size_t i) const { return p[i * stride]; }
    FLAC_HD Work channel(size_t c, uint32_t bs) const { return Work{p + c * bs * stride, stride, cap - c * bs}; }
};

// The LPC sum, sum of c[j] * s[j] over up to 32 taps, as the 128-bit integer the decoder has always
// used, from two 64-bit partial sums.  Proof that it is the same integer: a coefficient is read with
// sget(prec), prec <= 15, so |c| <= 2^14; with s = (s >> 32) * 2^32 + (s mod 2^32) (arithmetic shift,
// so this holds for negative s too), c * s = c * (s >> 32) * 2^32 + c * (s mod 2^32).  Each term of
// `lo` is below 2^46 in magnitude and each term of `hi` at most 2^45, so 32 of them stay inside 64
// bits, and value() = hi * 2^32 + lo is exactly the sum of the full products.
struct LpcSum {
    int64_t lo = 0, hi = 0;
    FLAC_HD void add(int64_t c, int64_t s) {
        lo += c * (int64_t)(uint32_t)(uint64_t)s;
        hi += c * (s >> 32);
    }
    FLAC_HD __int128 value() const { return (__int128)hi * ((__int128)1 << 32) + lo; }
};

// residual of one subframe into s[order .. bs), false when malformed
FLAC_HD bool residual(Bits& b, int order, uint32_t bs, const Work& s) {
    const uint64_t method = b.get(2);
    if (method > 1) return false;
    const int pbits = method == 0 ? 4 : 5;
    const uint64_t esc = method == 0 ? 15 : 31;
    const int porder = (int)b.get(4);
    const uint32_t parts = 1u << porder;
    if ((bs >> porder) << porder != bs || (bs >> porder) < (uint32_t)order) return false;
    uint32_t i = (uint32_t)order;
    for (uint32_t pi = 0; pi < parts; pi++) {
        const uint32_t cnt = (bs >> porder) - (pi == 0 ? (uint32_t)order : 0u);
        const uint64_t k = b.get(pbits);
        if (k == esc) {
            const int nb = (int)b.get(5);
            for (uint32_t j = 0; j < cnt; j++) s.at(i++) = b.sget(nb);
        } else {
            for (uint32_t j = 0; j < cnt; j++) {
                const uint64_t q = b.unary();
                if (q > (1ull << 40)) return false;
                const uint64_t u = (q << k) | b.get((int)k);
                s.at(i++) = (int64_t)(u >> 1) ^ -(int64_t)(u & 1);
                if (b.bad) return false;  // no more samples of a frame that is already lost
            }
        }
        if (b.bad) return false;
    }
    return true;
}

// one subframe of `bps` bits per sample into s[0 .. bs); bs <= s.cap is the caller's (decode_frame)
FLAC_HD bool subframe(Bits& b, int bps, uint32_t bs, const Work& s) {
    if (bs > s.cap) return false;
    if (b.get(1) != 0) return false;
    const int type = (int)b.get(6);
    int wasted = 0;
    if (b.get(1)) {
        const uint64_t u = b.unary();
        if (b.bad || u >= 64) return false;  // wasted >= bps for every legal bps
        wasted = (int)u + 1;
    }
    if (b.bad || wasted >= bps) return false;
    const int w = bps - wasted;
    if (type == 0) {  // CONSTANT
        const int64_t v = b.sget(w);
        for (uint32_t i = 0; i < bs; i++) s.at(i) = v;
    } else if (type == 1) {  // VERBATIM
        for (uint32_t i = 0; i < bs && !b.bad; i++) s.at(i) = b.sget(w);
    } else if (type >= 8 && type <= 12) {  // FIXED
        const int order = type - 8;
        if ((uint32_t)order > bs) return false;
        for (int i = 0; i < order; i++) s.at((size_t)i) = b.sget(w);
        if (!residual(b, order, bs, s)) return false;
        // the last four samples in registers: a sample does not wait for the previous one to come
        // back from memory
        int64_t h1 = order >= 1 ? s.at((size_t)(order - 1)) : 0, h2 = order >= 2 ? s.at((size_t)(order - 2)) : 0;
        int64_t h3 = order >= 3 ? s.at((size_t)(order - 3)) : 0, h4 = order >= 4 ? s.at((size_t)(order - 4)) : 0;
        for (uint32_t i = (uint32_t)order; order > 0 && i < bs; i++) {
            const int64_t r = s.at(i);
            int64_t v;
            switch (order) {
                case 1: v = r + h1; break;
                case 2: v = r + 2 * h1 - h2; break;
                case 3: v = r + 3 * h1 - 3 * h2 + h3; break;
                default: v = r + 4 * h1 - 6 * h2 + 4 * h3 - h4; break;
            }
            s.at(i) = v;
            h4 = h3;
            h3 = h2;
            h2 = h1;
            h1 = v;
        }
    } else if (type >= 32) {  // LPC
        const int order = type - 31;
        if ((uint32_t)order > bs) return false;
        for (int i = 0; i < order; i++) s.at((size_t)i) = b.sget(w);
        const int prec = (int)b.get(4) + 1;
        if (prec == 16) return false;  // 0b1111 is invalid
        const int shift = (int)b.sget(5);
        if (shift < 0) return false;
        int64_t c[32];
        for (int j = 0; j < order; j++) c[j] = b.sget(prec);
        if (!residual(b, order, bs, s)) return false;
        if (order <= 8) {
            // the common orders: coefficients and the last 8 samples in registers (every index below
            // is a constant once unrolled; absent taps are 0 x 0), so a sample does not wait for the
            // previous one to come back from memory
            int64_t cc[8], h[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                cc[j] = j < order ? c[j] : 0;
                h[j] = j < order ? s.at((size_t)(order - 1 - j)) : 0;
            }
            for (uint32_t i = (uint32_t)order; i < bs; i++) {
                LpcSum acc;
#pragma unroll
                for (int j = 0; j < 8; j++) acc.add(cc[j], h[j]);
                const int64_t v = (int64_t)((uint64_t)s.at(i) + (uint64_t)(int64_t)(acc.value() >> shift));
                s.at(i) = v;
#pragma unroll
                for (int j = 7; j > 0; j--) h[j] = h[j - 1];
                h[0] = v;
            }
        } else {
            for (uint32_t i = (uint32_t)order; i < bs; i++) {
                LpcSum acc;
                for (int j = 0; j < order; j++) acc.add(c[j], s.at(i - 1 - (uint32_t)j));
                s.at(i) = (int64_t)((uint64_t)s.at(i) + (uint64_t)(int64_t)(acc.value() >> shift));
            }
        }
    } else {
        return false;  // reserved
    }
    if (b.bad) return false;
    if (wasted)
        for (uint32_t i = 0; i < bs; i++) s.at(i) = (int64_t)((uint64_t)s.at(i) << wasted);
    return true;
}

// frame header at f[0 .. n); returns its length in bytes (0: no valid header).  si_bps is
// STREAMINFO's bits per sample, which sample-size code 0 refers to.
FLAC_HD size_t frame_header(const uint8_t* f, size_t n, int si_bps, uint32_t* bs, int* bps, int* chan_code) {
    if (n < 6 || f[0] != 0xFF || (f[1] & 0xFE) != 0xF8) return 0;
    Bits b(f, n);
    b.get(16);
    const int bsc = (int)b.get(4), src = (int)b.get(4), chc = (int)b.get(4), ssc = (int)b.get(3);
    if (b.get(1) != 0 || bsc == 0 || src == 15 || chc > 10 || ssc == 3) return 0;
    // UTF-8 coded frame / sample number
    const uint64_t lead = b.get(8);
    int extra = 0;
    if (lead < 0x80) extra = 0;
    else if ((lead & 0xE0) == 0xC0) extra = 1;
    else if ((lead & 0xF0) == 0xE0) extra = 2;
    else if ((lead & 0xF8) == 0xF0) extra = 3;
    else if ((lead & 0xFC) == 0xF8) extra = 4;
    else if ((lead & 0xFE) == 0xFC) extra = 5;
    else if (lead == 0xFE) extra = 6;
    else return 0;
    for (int i = 0; i < extra; i++)
        if ((b.get(8) & 0xC0) != 0x80) return 0;
    if (bsc == 6) *bs = (uint32_t)b.get(8) + 1;
    else if (bsc == 7) *bs = (uint32_t)b.get(16) + 1;
    else if (bsc == 1) *bs = 192;
    else if (bsc <= 5) *bs = 576u << (bsc - 2);
    else *bs = 256u << (bsc - 8);
    if (src == 12) b.get(8);
    else if (src == 13 || src == 14) b.get(16);
    if (b.bad) return 0;
    const size_t hl = b.pos / 8;
    if (hl + 1 > n || crc8(f, hl) != f[hl]) return 0;
    switch (ssc) {
        case 0: *bps = si_bps; break;
        case 1: *bps = 8; break;
        case 2: *bps = 12; break;
        case 4: *bps = 16; break;
        case 5: *bps = 20; break;
        case 6: *bps = 24; break;
        default: *bps = 32; break;  // 7 (3 was refused above)
    }
    *chan_code = chc;
    return hl + 1;
}

FLAC_HD int channels_of(int chan_code) { return chan_code <= 7 ? chan_code + 1 : 2; }

// The frame at d[pos], whose header of hl bytes frame_header accepted: subframes into w, zero
// padding to a byte, CRC-16 over [pos, end).  True with *end set when the frame is whole and its
// CRC holds; the next frame is then looked for at *end + 2.
FLAC_HD bool decode_frame(const uint8_t* d, size_t n, size_t pos, size_t hl, uint32_t bs, int bps, int chc, const Work& w,
                          size_t* end) {
    const int nch = channels_of(chc);
    if (bps < 4 || bps > 32 || bs == 0 || bs > 65536u || pos + hl > n || (size_t)nch * bs > w.cap) return false;
    Bits b(d + pos + hl, n - pos - hl);
    for (int c = 0; c < nch; c++) {
        const bool side = (chc == 8 && c == 1) || (chc == 9 && c == 0) || (chc == 10 && c == 1);
        if (!subframe(b, bps + (side ? 1 : 0), bs, w.channel((size_t)c, bs))) return false;
    }
    b.align();
    const size_t e = pos + hl + b.pos / 8;
    if (e + 2 > n || crc16(d + pos, e - pos) != (uint16_t)((d[e] << 8) | d[e + 1])) return false;
    *end = e;
    return true;
}

// symphonia's S32 buffer (sample << (32 - bps)) and the examples' S32 conversion
FLAC_HD float s32_to_f32(int64_t v, int shift) {
    const int32_t s32 = (int32_t)(uint32_t)((uint64_t)v << shift);
    return (float)s32 / 2147483648.0f;
}

// Stereo un-mixing and the mono f32 of an accepted frame into out[0 .. bs) (stride ostride): one
// channel as is, otherwise the channel sum from -0.0 in channel order divided by the channel count.
FLAC_HD void emit_mono(const Work& w, uint32_t bs, int bps, int chc, float* out, size_t ostride) {
    const int nch = channels_of(chc);
    const int shift = 32 - bps;
    const Work c0 = w.channel(0, bs), c1 = nch > 1 ? w.channel(1, bs) : c0;
    for (uint32_t i = 0; i < bs; i++) {
        if (chc == 8) {
            c1.at(i) = c0.at(i) - c1.at(i);  // left, side -> right
        } else if (chc == 9) {
            c0.at(i) = c0.at(i) + c1.at(i);  // side, right -> left
        } else if (chc == 10) {
            const int64_t side = c1.at(i);
            const int64_t mid = (int64_t)((uint64_t)c0.at(i) << 1) | (side & 1);
            c0.at(i) = (mid + side) >> 1;
            c1.at(i) = (mid - side) >> 1;
        }
        if (nch == 1) {
            out[i * ostride] = s32_to_f32(c0.at(i), shift);
        } else {
            float s = -0.0f;
            for (int c = 0; c < nch; c++) s = s + s32_to_f32(w.channel((size_t)c, bs).at(i), shift);
            out[i * ostride] = s / (float)nch;
        }
    }
}

// The host decoder's scan over one file's candidates (offsets ascending, every offset at which
// frame_header accepts): take the first candidate at or after pos; accepted when its frame decoded
// (ok), then pos = end + 2; otherwise pos = candidate + 1.  out_off[i] receives the frame's first
// sample index in the file's output, or ~0 for a candidate that is not part of the stream.
struct ChainCounts {
    uint64_t samples;
    uint32_t accepted, rejected;
};
FLAC_HD ChainCounts chain_file(const uint32_t* off, const uint8_t* ok, const uint32_t* end, const uint32_t* bs, size_t ncand,
                               size_t start, uint64_t* out_off) {
    ChainCounts r{0, 0, 0};
    size_t pos = start;
    for (size_t i = 0; i < ncand; i++) {
        out_off[i] = ~0ull;
        if ((size_t)off[i] < pos) continue;  // inside an accepted frame: the host never looks here
        if (ok[i]) {
            out_off[i] = r.samples;
            r.samples += bs[i];
            r.accepted++;
            pos = (size_t)end[i] + 2;
        } else {
            r.rejected++;
            pos = (size_t)off[i] + 1;
        }
    }
    return r;
}

}  // namespace flac_core
