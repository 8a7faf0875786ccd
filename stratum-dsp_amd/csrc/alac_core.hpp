// alac_core.hpp — the packet-level Apple Lossless decode shared by the host decoder (host_alac.hip:
// CAF, ISO MP4 and the Matroska A_ALAC track), the CPU phased decode (sdsp_debug_alac_decode_phased)
// and the device kernel (k_alac.hip).
//
// Everything here is `__host__ __device__` under hipcc and plain inline C++ under any other
// compiler (tools/alac_core_check.cpp builds it with the host sanitizers).  The functions work on
// caller-supplied buffers only: no allocation, no std::vector, no std::string.  Errors are codes
// (Err); err_text gives the host decoder's strings.
//
// Bounds, which hold for every input:
//   * every loop is bounded by a cookie or element field (frame length, channels <= 2, numactive
//     <= 31, a zero run <= 65535 that is checked against the frame before it is written) or by the
//     packet length: a loop that consumes bits ends when the reader runs past the packet (`over`);
//   * every read goes through Bits and returns zeros past the end of the packet;
//   * every write goes into the packet's own work range (`channels` arrays of `frame_length` 32-bit
//     values, checked against Work::cap before the first write), into the caller's coefficient
//     store (2 x 32 values) or into the packet's output slot of `frame_length` floats.
// A malformed packet ends as an error code, never as an out-of-range access.
//
// Arithmetic is the reference implementation's 32-bit wrap-around arithmetic.  Three places would
// be signed overflow in plain C++ on damaged input and are written as unsigned (wrapping) sums here,
// once, for both sides: the predictor's coefficient-update step `del0 -= (na - k) * ...`, its
// product, and the negation `-sgn * dd`.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ALAC_HD __host__ __device__ inline
#else
#define ALAC_HD inline
#endif

namespace alac_core {

// ALACSpecificConfig as the decoders use it
struct Config {
    uint32_t frame_length = 4096;
    int32_t bit_depth = 16, pb = 40, mb = 10, kb = 14, channels = 2, max_run = 255;
    uint32_t sample_rate = 44100;
};

enum Err : int32_t {
    OK = 0,
    TRUNCATED,            // "truncated ALAC frame"
    UNSUPPORTED_ELEMENT,  // "unsupported ALAC element <tag>"
    CHANNEL_COUNT,        // "ALAC element exceeds the channel count"
    ELEMENT_HEADER,       // "malformed ALAC element header"
    SAMPLE_COUNT,         // "malformed ALAC sample count"
    COUNT_MISMATCH,       // "ALAC elements disagree on the sample count"
    ELEMENT,              // "malformed ALAC element"
    RESIDUALS,            // "corrupt ALAC residuals"
    PREDICTION_MODE,      // "unsupported ALAC prediction mode <mode>"
    MISSING_CHANNELS,     // "ALAC frame is missing channels"
    WORK_RANGE,           // the caller's work range is too small (never on the host decoder)
};

// the host decoder's text of a code; `detail` is the tag or mode where the text names one
ALAC_HD const char* err_text(int32_t e) {
    switch (e) {
        case TRUNCATED: return "truncated ALAC frame";
        case UNSUPPORTED_ELEMENT: return "unsupported ALAC element ";
        case CHANNEL_COUNT: return "ALAC element exceeds the channel count";
        case ELEMENT_HEADER: return "malformed ALAC element header";
        case SAMPLE_COUNT: return "malformed ALAC sample count";
        case COUNT_MISMATCH: return "ALAC elements disagree on the sample count";
        case ELEMENT: return "malformed ALAC element";
        case RESIDUALS: return "corrupt ALAC residuals";
        case PREDICTION_MODE: return "unsupported ALAC prediction mode ";
        case MISSING_CHANNELS: return "ALAC frame is missing channels";
        case WORK_RANGE: return "ALAC work range too small";
    }
    return "";
}

// MSB-first bit reader over one packet; reads past the end return zeros and set `over`
struct Bits {
    const uint8_t* p;
    size_t n;
    uint64_t pos;
    bool over;
    ALAC_HD Bits(const uint8_t* d, size_t len) : p(d), n(len), pos(0), over(false) {}
    ALAC_HD uint32_t peek32() const {  // the 32 bits at pos (zeros past the end)
        const uint64_t b0 = pos >> 3;
        uint64_t w = 0;
        if (b0 + 5 <= (uint64_t)n) {
            const uint8_t* q = p + (size_t)b0;
            w = ((uint64_t)q[0] << 32) | ((uint64_t)q[1] << 24) | ((uint64_t)q[2] << 16) | ((uint64_t)q[3] << 8) | q[4];
        } else {
            for (int i = 0; i < 5; i++) {
                const uint64_t b = b0 + (uint64_t)i;
                w = (w << 8) | (b < (uint64_t)n ? p[(size_t)b] : 0);
            }
        }
        return (uint32_t)(w >> (8 - (pos & 7)));
    }
    ALAC_HD uint32_t read(int k) {  // k <= 32
        if (k <= 0) return 0;
        const uint32_t v = k >= 32 ? peek32() : peek32() >> (32 - k);
        pos += (uint64_t)k;
        if (pos > 8 * (uint64_t)n) over = true;
        return v;
    }
    ALAC_HD void skip(uint64_t k) {
        pos += k;
        if (pos > 8 * (uint64_t)n) over = true;
    }
};

// The packet's integer work range: `cap` 32-bit values, value i at p[i * stride] (the device
// interleaves the lanes of a wave: stride 64).  Channel array a holds its sample i at a * pitch + i.
struct Work {
    int32_t* p;
    size_t stride, cap, pitch;
    ALAC_HD int32_t& at(int a, int i) const { return p[((size_t)a * pitch + (size_t)i) * stride]; }
};

// The adaptive predictor coefficients of the (up to) two channels of an element: coefficient k of
// channel e at p[(e * 32 + k) * stride] (the device keeps them in LDS, [k][lane]: stride 64).
struct Coefs {
    int16_t* p;
    size_t stride;
    ALAC_HD int16_t& at(int e, int k) const { return p[((size_t)e * 32 + (size_t)k) * stride]; }
};

ALAC_HD int clz32(uint32_t x) { return x ? __builtin_clz(x) : 32; }

// adaptive Golomb parameters (Apple's ag_dec: QBSHIFT 9, MMULSHIFT 2, MDENSHIFT 6, MOFF 16,
// BITOFF 24, escape after a 9-bit prefix, zero runs of up to 65535)
constexpr int QBSHIFT = 9, QB = 1 << QBSHIFT, MMULSHIFT = 2, MDENSHIFT = QBSHIFT - MMULSHIFT - 1,
              MOFF = 1 << (MDENSHIFT - 2), BITOFF = 24, MAX_PREFIX = 9, MAX_DATATYPE_BITS_16 = 16;

// one Golomb value: a unary prefix of ones (escape at 9), then k bits; values v < 2 give pre * m
// and return the k-th bit to the stream
ALAC_HD uint32_t ag_get(Bits& b, uint32_t m, int k, int escape_bits) {
    const uint32_t s = b.peek32();
    const int pre = clz32(~s);
    if (pre >= MAX_PREFIX) {
        b.skip(MAX_PREFIX);
        return b.read(escape_bits);
    }
    b.skip((uint64_t)pre + 1);
    if (k == 1) return (uint32_t)pre;
    const uint32_t v = b.read(k);
    if (v >= 2) return (uint32_t)pre * m + v - 1;
    b.pos -= 1;
    return (uint32_t)pre * m;
}

// dyn_decomp: n signed residuals into channel array a of the work range.  Every turn of the loop
// consumes at least one bit or fails, so it ends within the packet's bits.
ALAC_HD bool ag_decode(Bits& b, const Config& c, int pb_factor, int n, int chan_bits, const Work& w, int a) {
    const uint32_t pb = (uint32_t)(c.pb * pb_factor) / 4;
    const uint32_t wb = (1u << c.kb) - 1;
    uint32_t mb = (uint32_t)c.mb;
    uint32_t zmode = 0;
    int i = 0;
    while (i < n) {
        const uint32_t m0 = mb >> QBSHIFT;
        int k = 31 - clz32(m0 + 3);  // lg3a
        if (k > c.kb) k = c.kb;
        const uint32_t m = (1u << k) - 1;
        const uint32_t v = ag_get(b, m, k, chan_bits);
        const uint32_t nd = v + zmode;
        const int32_t mag = (int32_t)((nd + 1) >> 1);
        w.at(a, i++) = (nd & 1) ? -mag : mag;
        mb = pb * (v + zmode) + mb - ((pb * mb) >> QBSHIFT);
        if (v > 0xffff) mb = 0xffff;
        zmode = 0;
        if (((mb << MMULSHIFT) < (uint32_t)QB) && i < n) {
            zmode = 1;
            const int kz = clz32(mb) - BITOFF + (int)((mb + MOFF) >> MDENSHIFT);
            const uint32_t mz = ((1u << kz) - 1) & wb;
            const uint32_t run = ag_get(b, mz, kz, MAX_DATATYPE_BITS_16);
            if ((uint64_t)i + run > (uint64_t)n) return false;
            for (uint32_t j = 0; j < run; j++) w.at(a, i++) = 0;
            if (run >= 65535) zmode = 0;
            mb = 0;
        }
        if (b.over) return false;
    }
    return true;
}

ALAC_HD int32_t sext(int32_t v, int chan_bits) {
    const int sh = 32 - chan_bits;
    return (int32_t)((uint32_t)v << sh) >> sh;
}
ALAC_HD int32_t sign_of(int32_t v) { return (v > 0) - (v < 0); }

// unpc_block in place over channel array a: the sign-adaptive predictor (numactive 31: first-order
// difference).  out[j] takes pc[j]'s place: the sample at j reads pc[j] and samples before j only.
ALAC_HD void unpredict(const Work& w, int a, int n, const Coefs& cf, int e, int na, int chan_bits, int den_shift) {
    if (n <= 0 || na == 0) return;
    if (na == 31) {
        int32_t prev = w.at(a, 0);
        for (int j = 1; j < n; j++) {
            prev = sext((int32_t)((uint32_t)w.at(a, j) + (uint32_t)prev), chan_bits);
            w.at(a, j) = prev;
        }
        return;
    }
    for (int j = 1; j <= na && j < n; j++)
        w.at(a, j) = sext((int32_t)((uint32_t)w.at(a, j) + (uint32_t)w.at(a, j - 1)), chan_bits);
    const int32_t den_half = den_shift > 0 ? 1 << (den_shift - 1) : 0;
    const int lim = na + 1;
    for (int j = lim; j < n; j++) {
        const int32_t top = w.at(a, j - lim);
        // 32-bit wrap-around arithmetic, as the reference implementation's int32 sums
        uint32_t sum = 0;
        for (int k = 0; k < na; k++)
            sum += (uint32_t)((int64_t)cf.at(e, k) * ((int64_t)w.at(a, j - 1 - k) - (int64_t)top));
        const int32_t del = w.at(a, j);
        uint32_t del0 = (uint32_t)del;  // a wrapping int32
        const int32_t sg = sign_of(del);
        const int32_t pred = (int32_t)(sum + (uint32_t)den_half) >> den_shift;
        w.at(a, j) = sext((int32_t)((uint32_t)del + (uint32_t)top + (uint32_t)pred), chan_bits);
        if (sg > 0) {
            for (int k = na - 1; k >= 0; k--) {
                const int32_t dd = (int32_t)((uint32_t)top - (uint32_t)w.at(a, j - 1 - k));
                const int32_t sgn = sign_of(dd);
                cf.at(e, k) = (int16_t)(cf.at(e, k) - sgn);
                del0 -= (uint32_t)(na - k) * (uint32_t)(int32_t)(((int64_t)sgn * dd) >> den_shift);
                if ((int32_t)del0 <= 0) break;
            }
        } else if (sg < 0) {
            for (int k = na - 1; k >= 0; k--) {
                const int32_t dd = (int32_t)((uint32_t)top - (uint32_t)w.at(a, j - 1 - k));
                const int32_t sgn = sign_of(dd);
                cf.at(e, k) = (int16_t)(cf.at(e, k) + sgn);
                del0 -= (uint32_t)(na - k) * (uint32_t)(int32_t)((-(int64_t)sgn * dd) >> den_shift);
                if ((int32_t)del0 >= 0) break;
            }
        }
    }
}

// integers of the stream's depth -> mono f32 (the examples' conversion)
ALAC_HD float scale_of(int bit_depth) {
    return bit_depth == 16 ? 32768.0f : bit_depth == 32 ? 2147483648.0f : (float)(1u << (bit_depth - 1));
}
ALAC_HD float to_mono(int ch, float scale, int32_t l, int32_t r) {
    if (ch == 1) return (float)l / scale;
    float s = -0.0f;
    s = s + (float)l / scale;
    s = s + (float)r / scale;
    return s / (float)ch;
}

// One ALAC frame (packet) -> its mono f32 samples, sample i at out[i * out_stride], *n_out of them
// (<= c.frame_length, which the caller reserved).  Needs w.cap >= c.channels * c.frame_length and
// w.pitch >= c.frame_length; c is a parsed cookie (frame_length >= 1, channels 1 or 2, kb 1..14).
// Nothing is written to `out` unless the whole packet decodes.  *detail receives the element tag or
// prediction mode of UNSUPPORTED_ELEMENT / PREDICTION_MODE.
ALAC_HD int32_t decode_frame(const uint8_t* d, size_t len, const Config& c, const Work& w, const Coefs& cf, float* out,
                             size_t out_stride, uint32_t* n_out, int32_t* detail) {
    *n_out = 0;
    *detail = 0;
    const int nch_total = c.channels;
    if (nch_total < 1 || nch_total > 2 || c.frame_length == 0 || w.pitch < c.frame_length ||
        w.cap / (size_t)nch_total < w.pitch)
        return WORK_RANGE;
    Bits b(d, len);
    int ch_done = 0;
    int frame_n = -1;
    while (true) {  // every turn consumes at least 3 bits: ends within the packet
        const uint32_t tag = b.read(3);
        if (b.over) return TRUNCATED;
        if (tag == 7) break;  // ID_END
        if (tag == 6) {       // ID_FIL: count + bytes
            uint32_t cnt = b.read(4);
            if (cnt == 15) cnt += b.read(8) - 1;
            b.skip(8ull * cnt);
            continue;
        }
        if (tag == 4) {  // ID_DSE: tag, align flag, count, (align), bytes
            b.read(4);
            const uint32_t align = b.read(1);
            uint32_t cnt = b.read(8);
            if (cnt == 255) cnt += b.read(8);
            if (align) b.skip((8 - (b.pos & 7)) & 7);
            b.skip(8ull * cnt);
            continue;
        }
        if (tag != 0 && tag != 1 && tag != 3) {
            *detail = (int32_t)tag;
            return UNSUPPORTED_ELEMENT;
        }
        const int ech = tag == 1 ? 2 : 1;
        if (ch_done + ech > nch_total) return CHANNEL_COUNT;
        b.read(4);  // element instance tag
        if (b.read(12) != 0) return ELEMENT_HEADER;
        const uint32_t hb = b.read(4);
        const bool partial = hb & 8;
        const int bytes_shifted = (int)((hb >> 1) & 3);
        const bool escape = hb & 1;
        if (bytes_shifted == 3) return ELEMENT_HEADER;
        int n = (int)c.frame_length;
        if (partial) {
            uint32_t v = b.read(16) << 16;
            v |= b.read(16);
            if (v == 0 || v > c.frame_length) return SAMPLE_COUNT;
            n = (int)v;
        }
        if (frame_n < 0)
            frame_n = n;
        else if (n != frame_n)
            return COUNT_MISMATCH;
        const int shift = escape ? 0 : bytes_shifted * 8;  // raw elements carry the full samples
        const int au = ch_done, av = ch_done + 1;          // the element's channel arrays
        int mix_bits = 0, mix_res = 0;
        uint64_t shift_pos = 0;
        if (!escape) {
            const int chan_bits = c.bit_depth - shift + (ech == 2 ? 1 : 0);
            if (chan_bits < 1 || chan_bits > 32) return ELEMENT;
            if (ech == 2) {
                mix_bits = (int)b.read(8);
                mix_res = (int8_t)b.read(8);
                if (mix_bits > 31) return ELEMENT;
            }
            int mode[2], den[2], pbf[2], na[2];
            for (int e = 0; e < ech; e++) {
                const uint32_t h1 = b.read(8), h2 = b.read(8);
                mode[e] = (int)(h1 >> 4);
                den[e] = (int)(h1 & 15);
                pbf[e] = (int)(h2 >> 5);
                na[e] = (int)(h2 & 31);
                for (int k = 0; k < na[e]; k++) cf.at(e, k) = (int16_t)b.read(16);
            }
            if (shift) {
                shift_pos = b.pos;
                b.skip((uint64_t)shift * (uint64_t)ech * (uint64_t)n);
            }
            for (int e = 0; e < ech; e++) {
                if (!ag_decode(b, c, pbf[e], n, chan_bits, w, au + e)) return RESIDUALS;
                if (mode[e] == 0) {
                    unpredict(w, au + e, n, cf, e, na[e], chan_bits, den[e]);
                } else if (mode[e] == 15) {  // a first-order pass, then the FIR predictor
                    unpredict(w, au + e, n, cf, e, 31, chan_bits, 0);
                    unpredict(w, au + e, n, cf, e, na[e], chan_bits, den[e]);
                } else {
                    *detail = mode[e];
                    return PREDICTION_MODE;
                }
            }
        } else {
            // escaped: raw samples of the full bit depth, channels interleaved per sample
            const int bits = c.bit_depth;
            for (int i = 0; i < n && !b.over; i++) {
                for (int e = 0; e < ech; e++) {
                    int32_t val;
                    if (bits <= 16) {
                        val = sext((int32_t)b.read(bits), bits);
                    } else {
                        const int32_t hi = sext((int32_t)b.read(16), 16);
                        val = (int32_t)((uint32_t)hi << (bits - 16)) | (int32_t)b.read(bits - 16);
                    }
                    w.at(au + e, i) = val;
                }
            }
        }
        if (b.over) return TRUNCATED;
        // un-mix (stereo) and restore the shifted low bytes, read again from where they sit in the
        // packet (they lie before the residuals, inside the packet: `over` was checked above)
        Bits sb(d, len);
        sb.pos = shift_pos;
        for (int i = 0; i < n; i++) {
            int32_t l, r = 0;
            if (ech == 2) {
                const int32_t u = w.at(au, i), v = w.at(av, i);
                if (mix_res != 0) {
                    l = (int32_t)((uint32_t)u + (uint32_t)v - (uint32_t)((int32_t)((uint32_t)mix_res * (uint32_t)v) >> mix_bits));
                    r = (int32_t)((uint32_t)l - (uint32_t)v);
                } else {
                    l = u;
                    r = v;
                }
            } else {
                l = w.at(au, i);
            }
            if (shift) {
                l = (int32_t)((uint32_t)l << shift) | (int32_t)sb.read(shift);
                if (ech == 2) r = (int32_t)((uint32_t)r << shift) | (int32_t)sb.read(shift);
            }
            w.at(au, i) = l;
            if (ech == 2) w.at(av, i) = r;
        }
        ch_done += ech;
    }
    if (ch_done != nch_total) return MISSING_CHANNELS;
    const float scale = scale_of(c.bit_depth);
    for (int i = 0; i < frame_n; i++)
        out[(size_t)i * out_stride] = to_mono(nch_total, scale, w.at(0, i), nch_total == 2 ? w.at(1, i) : 0);
    *n_out = (uint32_t)frame_n;
    return OK;
}

// One file's walk over its packets' sample counts (0 = the packet was skipped): the offset of every
// decoded packet in the file's track (~0 for a skipped one); returns the track's length.
ALAC_HD uint64_t layout_file(const uint32_t* cnt, uint64_t n_packets, uint64_t* out_off, uint32_t* decoded,
                             uint32_t* skipped) {
    uint64_t total = 0;
    uint32_t dec = 0, skp = 0;
    for (uint64_t i = 0; i < n_packets; i++) {
        if (cnt[i]) {
            out_off[i] = total;
            total += cnt[i];
            dec++;
        } else {
            out_off[i] = ~0ull;
            skp++;
        }
    }
    *decoded = dec;
    *skipped = skp;
    return total;
}

}  // namespace alac_core
