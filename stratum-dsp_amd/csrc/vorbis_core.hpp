// vorbis_core.hpp — the packet-level Vorbis I decode shared by the host decoder (host_vorbis.hip:
// Ogg and the Matroska A_VORBIS track), the CPU phased decode (vorbis_phased.hpp,
// sdsp_debug_vorbis_decode_phased) and the device kernels (k_vorbis.hip).
//
// Everything here is `__host__ __device__` under hipcc and plain inline C++ under any other
// compiler (tools/vorbis_core_check.cpp builds it with the host sanitizers).  The functions work on
// caller-supplied buffers only: no allocation, no std::vector, no std::string.  Setup parsing (the
// codebook build, the VQ expansion, every error text) stays in host_vorbis.hip, which flattens the
// setup header into the plain structs below; a packet never fails with a text (the host loop skips
// or silences a damaged packet), so the codes here are few.
//
// Arithmetic is the host decoder's, once, for both sides.  No transcendental is evaluated here: the
// pre- / post-twiddles, the FFT twiddles, the window slopes and the inverse-dB table are host-built
// tables (host_vorbis.hip: sdsp_vorbis_tables).  Complex products are written out as
// ar*wr - ai*wi, ar*wi + ai*wr in double, which is what std::complex gives for finite values under
// -ffp-contract=off; the radix-2 network is a fixed graph, so the order in which a stage's
// butterflies run cannot change a value.  Two integer products of floor 1 that would be signed
// overflow in plain C++ on hostile Y values are written as unsigned (wrapping) products.
//
// Bounds, which hold for every input:
//   * every loop is bounded by a header field (block size <= 8192, <= 65 floor points, 8 passes,
//     partitions from begin / end / psize, <= 255 channels, <= 256 coupling steps) or by the
//     packet's bits: a Huffman walk is at most 33 steps and fails when the reader runs over;
//   * every read goes through Bits (zeros past the end, `over` set) or a (pointer, length) pair the
//     host built: a tree walk checks the node against the tree's length;
//   * every write goes into the caller's work range, whose size decode_packet checks before its
//     first write (work_words), into the floor's 65-value Y store, or into the packet's own
//     spectrum block of channels x n/2 floats;
//   * indices from the bitstream: book numbers of floors, residues and mappings are checked at plan
//     time (read_setup refuses a setup that names a missing book, floor, residue or mapping);
//     classifications are `% classes`, in range by construction; a VQ entry is a leaf of the
//     host-built tree, below `entries` by construction; the mode number is checked per packet.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VORBIS_HD __host__ __device__ inline
#else
#define VORBIS_HD inline
#endif

namespace vorbis_core {

enum Err : int32_t {
    OK = 0,
    NOT_AUDIO,   // the host loop skips the packet (empty, not audio, mode number out of range)
    WORK_RANGE,  // the caller's work range is too small (never on the host decoder)
};

VORBIS_HD const char* err_text(int32_t e) {
    switch (e) {
        case NOT_AUDIO: return "not a Vorbis audio packet";
        case WORK_RANGE: return "Vorbis work range too small";
    }
    return "";
}

// ---- the setup header, flattened by the host (host_vorbis.hip) ----
struct Book {
    uint32_t dims, entries;
    uint32_t tree_off, tree_n;  // the decoding tree: tree_n int32 at trees + tree_off
    uint32_t vq_off;            // entries x dims floats at vq + vq_off (lookup 1 / 2)
    int32_t lookup;
};

constexpr int FLOOR_MAX_POINTS = 65;

struct Floor {
    int32_t partitions, multiplier, rangebits, nv;
    uint8_t part_class[32];
    uint8_t class_dim[16], class_sub[16];
    int16_t class_master[16];
    int16_t sub_books[16][8];
    uint16_t X[FLOOR_MAX_POINTS];
    // per point: its low / high neighbour among the earlier points, and the points in x order
    uint8_t lo[FLOOR_MAX_POINTS], hi[FLOOR_MAX_POINTS], order[FLOOR_MAX_POINTS];
};

struct Residue {
    int32_t type;
    uint32_t begin, end, psize;
    int32_t classes, classbook;
    int16_t books[64][8];  // per class, per pass (-1 unused)
};

struct Mapping {
    int32_t submaps, steps;
    uint8_t mag[256], ang[256];
    uint8_t mux[256];
    uint8_t sub_floor[16], sub_residue[16];
};

struct Mode {
    uint8_t blockflag, mapping;
};

struct Setup {
    int32_t channels, bs0, bs1, nmodes;
    const Book* books;
    const int32_t* trees;
    const float* vq;
    const Floor* floors;
    const Residue* residues;
    const Mapping* maps;
    const Mode* modes;
    const float* inv_db;  // 256 entries
};

struct cd {
    double re, im;
};

// the tables of one block size N (M = N/2, H = N/4)
struct BlockTables {
    const cd* pre;          // H: cos / sin of -pi (4k + 1) / (4M)
    const cd* post;         // H: cos / sin of -pi j / M
    const cd* tw;           // H/2: cos / sin of -2 pi k / H
    const float* slope_up;  // N/2: the rising window slope of that length
    const float* slope_dn;  // N/2: the falling one
};

// ---- LSB-first bit reader; past the end it returns zeros for the missing bits and sets `over` ----
struct Bits {
    const uint8_t* p;
    uint64_t n;
    uint64_t pos;
    bool over;
    VORBIS_HD Bits(const uint8_t* d, uint64_t len) : p(d), n(len), pos(0), over(false) {}
    VORBIS_HD uint32_t read(int k) {  // k <= 32
        if (k <= 0) return 0;
        const uint64_t left = 8 * n - pos;
        int take = k;
        if ((uint64_t)k > left) {
            over = true;
            take = (int)left;
            if (take == 0) return 0;
        }
        const uint64_t b0 = pos >> 3;
        const int sh = (int)(pos & 7);
        const int nb = (sh + take + 7) >> 3;  // <= 5, every byte below n
        uint64_t w = 0;
        for (int i = 0; i < nb; i++) w |= (uint64_t)p[b0 + (uint64_t)i] << (8 * i);
        pos += (uint64_t)take;
        w >>= sh;
        return (uint32_t)(take >= 32 ? w : w & ((1ull << take) - 1));
    }
    VORBIS_HD bool bit() { return read(1) != 0; }
};

VORBIS_HD int ilog(uint32_t v) {
    int r = 0;
    while (v) r++, v >>= 1;
    return r;
}

// Huffman tree walk, first bit = codeword MSB, at most 33 steps.  -1: end of packet or an
// unassigned codeword.  The tree is host-built; a node past its length ends the walk.
VORBIS_HD int huff(const Setup& s, const Book& bk, Bits& b) {
    const int32_t* tree = s.trees + bk.tree_off;
    uint32_t node = 0;
    for (int depth = 0; depth < 33; depth++) {
        const uint32_t bit = b.read(1);
        if (b.over) return -1;
        const uint32_t at = 2 * node + bit;
        if (at >= bk.tree_n) return -1;
        const int32_t t = tree[at];
        if (t < 0) return -t - 1;
        if (t == 0) return -1;
        node = (uint32_t)t;
    }
    return -1;
}

// The packet's work range: `cap` 32-bit words, word i at p[i * stride] (the device interleaves the
// lanes of a wave: stride 64).
struct Work {
    uint32_t* p;
    size_t stride, cap;
    VORBIS_HD uint32_t get(size_t i) const { return p[i * stride]; }
    VORBIS_HD void set(size_t i, uint32_t v) const { p[i * stride] = v; }
    VORBIS_HD float getf(size_t i) const {
        const uint32_t x = p[i * stride];
        float f;
        __builtin_memcpy(&f, &x, 4);
        return f;
    }
    VORBIS_HD void setf(size_t i, float f) const {
        uint32_t x;
        __builtin_memcpy(&x, &f, 4);
        p[i * stride] = x;
    }
};
// the layout of a packet's work range: per channel a flag word and a list slot, then the floor
// curves (one 0 .. 255 table index per bin), the classifications and the type-2 interleaved vector
VORBIS_HD size_t work_words(int channels, int n2) { return 2 * (size_t)channels + 3 * (size_t)channels * (size_t)n2; }
constexpr uint32_t CH_UNUSED = 1, CH_SKIP = 2;

// The floor's Y list (then final Y, in place): value k at p[k * stride], FLOOR_MAX_POINTS values
// (the device keeps it in LDS laid out [k][lane]).
struct YStore {
    int32_t* p;
    size_t stride;
    VORBIS_HD int32_t& at(int k) const { return p[(size_t)k * stride]; }
};

// the first bits of a packet: false when the host loop skips it
VORBIS_HD bool packet_header(const Setup& s, Bits& b, uint64_t len, int* mode_no, bool* prev_long, bool* next_long) {
    *mode_no = 0, *prev_long = false, *next_long = false;
    if (len == 0) return false;
    if (b.read(1) != 0) return false;  // not an audio packet
    const int m = (int)b.read(ilog((uint32_t)(s.nmodes - 1)));
    if (b.over || m >= s.nmodes) return false;
    *mode_no = m;
    if (s.modes[m].blockflag) {
        *prev_long = b.bit();
        *next_long = b.bit();
    }
    return true;
}

// curve index of x in [x0, x1) into the work words at `base` (only x < n2 is written)
VORBIS_HD void render_line(int x0, int y0, int x1, int y1, const Work& w, size_t base, int n2) {
    if (x1 <= x0) return;  // setup parsing rejects repeated X values; a zero-width line draws nothing
    const int dy = y1 - y0, adx = x1 - x0;
    int ady = dy < 0 ? -dy : dy;
    const int base_ = dy / adx;
    const int sy = dy < 0 ? base_ - 1 : base_ + 1;
    int y = y0, errv = 0;
    ady -= (base_ < 0 ? -base_ : base_) * adx;
    const int xe = x1 < n2 ? x1 : n2;  // past n2 nothing is written and nothing read afterwards
    if (x0 < n2) w.set(base + (size_t)x0, (uint32_t)(y < 0 ? 0 : y > 255 ? 255 : y));
    for (int x = x0 + 1; x < xe; x++) {
        errv += ady;
        if (errv >= adx) {
            errv -= adx;
            y += sy;
        } else {
            y += base_;
        }
        w.set(base + (size_t)x, (uint32_t)(y < 0 ? 0 : y > 255 ? 255 : y));
    }
}

enum FloorResult : int { FLOOR_USED, FLOOR_UNUSED, FLOOR_BAD };

// floor 1 packet decode + curve synthesis: the inverse-dB table index of every bin into the work
// words [base, base + n2)
VORBIS_HD int floor1_decode(Bits& b, const Setup& s, const Floor& f, int n2, const YStore& Y, const Work& w, size_t base) {
    if (!b.bit()) return FLOOR_UNUSED;
    const int range = f.multiplier == 1 ? 256 : f.multiplier == 2 ? 128 : f.multiplier == 3 ? 86 : 64;
    const int nv = f.nv;
    for (int i = 0; i < nv; i++) Y.at(i) = 0;
    Y.at(0) = (int)b.read(ilog((uint32_t)(range - 1)));
    Y.at(1) = (int)b.read(ilog((uint32_t)(range - 1)));
    int off = 2;
    for (int p = 0; p < f.partitions; p++) {
        const int c = f.part_class[p];  // < 16 (4 bits)
        const int cdim = f.class_dim[c], cbits = f.class_sub[c];
        const int csub = (1 << cbits) - 1;
        int cval = 0;
        if (cbits > 0) {
            cval = huff(s, s.books[f.class_master[c]], b);  // book number checked at plan time
            if (cval < 0) return FLOOR_BAD;
        }
        for (int j = 0; j < cdim; j++) {
            const int book = f.sub_books[c][cval & csub];  // csub <= 7; book number checked at plan time
            cval >>= cbits;
            int y = 0;
            if (book >= 0) {
                y = huff(s, s.books[book], b);
                if (y < 0) return FLOOR_BAD;
            }
            if (off < nv) Y.at(off) = y;  // nv = 2 + the classes' dimensions: in range by construction
            off++;
        }
    }
    if (b.over) return FLOOR_BAD;
    // amplitude synthesis (step 1), the final Y over the coded one in place: a point reads only
    // earlier points
    uint64_t used = 3;  // points 0 .. 63
    bool used64 = false;
    for (int i = 2; i < nv; i++) {
        const int lo = f.lo[i], hi = f.hi[i];
        const int x0 = f.X[lo], y0 = Y.at(lo), x1 = f.X[hi], y1 = Y.at(hi);
        const int dy = y1 - y0, adx = x1 - x0, ady = dy < 0 ? -dy : dy;
        const int e = (int)((uint32_t)ady * (uint32_t)((int)f.X[i] - x0));
        const int o = e / adx;  // adx > 0: the X list does not repeat a value
        const int pred = dy < 0 ? y0 - o : y0 + o;
        const int val = Y.at(i);
        const int highroom = range - pred, lowroom = pred;
        const int room = (int)((uint32_t)(highroom < lowroom ? highroom : lowroom) * 2u);
        if (val != 0) {
            used |= 1ull << lo;  // lo, hi < i <= 64
            used |= 1ull << hi;
            if (i < 64)
                used |= 1ull << i;
            else
                used64 = true;
            if (val >= room)
                Y.at(i) = highroom > lowroom ? val - lowroom + pred : pred - val + highroom - 1;
            else
                Y.at(i) = (val & 1) ? pred - (val + 1) / 2 : pred + val / 2;
        } else {
            Y.at(i) = pred;
        }
    }
    // curve synthesis (step 2): the used points in x order, lines between them
    for (int j = 0; j < n2; j++) w.set(base + (size_t)j, 0);
    int lx = 0, ly = (int)((uint32_t)Y.at(f.order[0]) * (uint32_t)f.multiplier), hx = 0, hy = 0;
    for (int k = 1; k < nv; k++) {
        const int i = f.order[k];
        if (!(i < 64 ? (used >> i) & 1 : used64)) continue;
        hy = (int)((uint32_t)Y.at(i) * (uint32_t)f.multiplier);
        hx = f.X[i];
        if (lx < n2) render_line(lx, ly, hx, hy, w, base, n2);
        lx = hx;
        ly = hy;
    }
    if (hx < n2) render_line(hx, hy, n2, hy, w, base, n2);
    return FLOOR_USED;
}

// One residue vector set: nc vectors of `size` values, decoded as format `type` (0 / 1).  With
// `inter` the one vector is the work range's interleaved vector (residue type 2); otherwise vector j
// is channel work[C + j]'s row of the spectrum block.  The classifications live at work[cls_base ..).
// false: the packet ended (what was decoded stays).
VORBIS_HD bool residue_set(Bits& b, const Setup& s, const Residue& r, const Work& w, int C, int n2, float* spec, int nc,
                           bool inter, uint32_t size, int type) {
    const Book& cb = s.books[r.classbook];  // checked at plan time
    const int cwords = (int)cb.dims;
    const uint32_t lb = r.begin < size ? r.begin : size, le = r.end < size ? r.end : size;
    const uint32_t nread = le > lb ? le - lb : 0;
    const uint32_t parts = nread / r.psize;  // psize >= 1
    if (parts == 0) return true;
    const size_t cls_base = 2 * (size_t)C + (size_t)C * (size_t)n2;
    const size_t inter_base = cls_base + (size_t)C * (size_t)n2;
    // nc * parts <= C * n2: parts <= size / psize, and size is n2 (nc <= C) or C * n2 (nc == 1)
    for (size_t i = 0; i < (size_t)nc * parts; i++) w.set(cls_base + i, 0);
    for (int pass = 0; pass < 8; pass++) {
        uint32_t pc = 0;
        while (pc < parts) {
            if (pass == 0)
                for (int j = 0; j < nc; j++) {
                    if (!inter && (w.get((size_t)w.get((size_t)C + (size_t)j)) & CH_SKIP)) continue;
                    int temp = huff(s, cb, b);
                    if (temp < 0) return false;
                    for (int i = cwords - 1; i >= 0; i--) {
                        // a classification past the last partition is never read: not stored
                        if ((uint64_t)i + pc < parts) w.set(cls_base + (size_t)j * parts + (size_t)i + pc, (uint32_t)(temp % r.classes));
                        temp /= r.classes;
                    }
                }
            for (int i = 0; i < cwords && pc < parts; i++, pc++) {
                for (int j = 0; j < nc; j++) {
                    const uint32_t chn = inter ? 0u : w.get((size_t)C + (size_t)j);
                    if (!inter && (w.get((size_t)chn) & CH_SKIP)) continue;
                    const int book = r.books[w.get(cls_base + (size_t)j * parts + pc)][pass];  // class < classes <= 64
                    if (book < 0) continue;
                    const Book& vb = s.books[book];  // checked at plan time
                    if (vb.lookup == 0 || vb.dims == 0) return false;
                    const float* vq = s.vq + vb.vq_off;
                    float* row = spec + (size_t)chn * (size_t)n2;
                    const uint32_t off = lb + pc * r.psize;  // off + psize <= le <= size
                    const uint32_t dims = vb.dims;
                    if (type == 0) {
                        const uint32_t step = r.psize / dims;
                        for (uint32_t q = 0; q < step; q++) {
                            const int e = huff(s, vb, b);
                            if (e < 0) return false;
                            for (uint32_t k = 0; k < dims; k++) {  // q + k * step < step * dims <= psize
                                const size_t at = (size_t)off + q + (size_t)k * step;
                                const float v = vq[(size_t)e * dims + k];
                                if (inter)
                                    w.setf(inter_base + at, w.getf(inter_base + at) + v);
                                else
                                    row[at] += v;
                            }
                        }
                    } else {
                        uint32_t i2 = 0;
                        while (i2 < r.psize) {
                            const int e = huff(s, vb, b);
                            if (e < 0) return false;
                            for (uint32_t k = 0; k < dims && i2 < r.psize; k++) {
                                const size_t at = (size_t)off + i2++;
                                const float v = vq[(size_t)e * dims + k];
                                if (inter)
                                    w.setf(inter_base + at, w.getf(inter_base + at) + v);
                                else
                                    row[at] += v;
                            }
                        }
                    }
                }
            }
        }
    }
    return true;
}

// residue decode for the nc channels of one submap (listed at work[C ..)); their spectrum rows are
// zero on entry
VORBIS_HD void residue_decode(Bits& b, const Setup& s, const Residue& r, const Work& w, int C, int n2, float* spec, int nc) {
    if (s.books[r.classbook].dims == 0) return;
    if (r.type < 2) {
        residue_set(b, s, r, w, C, n2, spec, nc, false, (uint32_t)n2, r.type);
        return;
    }
    // type 2: the channels interleaved into one vector, decoded as format 1
    bool any = false;
    for (int j = 0; j < nc; j++) any = any || !(w.get((size_t)w.get((size_t)C + (size_t)j)) & CH_SKIP);
    if (!any) return;
    const size_t inter_base = 2 * (size_t)C + 2 * (size_t)C * (size_t)n2;
    for (size_t i = 0; i < (size_t)n2 * (size_t)nc; i++) w.setf(inter_base + i, 0.0f);
    if (!residue_set(b, s, r, w, C, n2, spec, 1, true, (uint32_t)(n2 * nc), 1)) return;
    for (int i = 0; i < n2; i++)
        for (int j = 0; j < nc; j++) spec[(size_t)w.get((size_t)C + (size_t)j) * (size_t)n2 + (size_t)i] += w.getf(inter_base + (size_t)i * nc + j);
}

// One kept audio packet into its spectrum block spec[channels][n/2]: floors, residues, inverse
// coupling, the floor x residue product.  *zeroed: a floor decode failed and the block is silent.
VORBIS_HD int32_t decode_packet(const Setup& s, const uint8_t* pk, uint64_t len, const Work& w, const YStore& Y, float* spec,
                                int32_t* zeroed) {
    *zeroed = 0;
    Bits b(pk, len);
    int mode_no;
    bool pl, nl;
    if (!packet_header(s, b, len, &mode_no, &pl, &nl)) return NOT_AUDIO;
    const Mode md = s.modes[mode_no];
    const int C = s.channels;
    const int n2 = (md.blockflag ? s.bs1 : s.bs0) / 2;
    if (w.cap < work_words(C, n2)) return WORK_RANGE;
    const Mapping& mp = s.maps[md.mapping];  // checked at plan time
    const size_t curve_base = 2 * (size_t)C;
    for (size_t i = 0; i < (size_t)C * (size_t)n2; i++) spec[i] = 0.0f;
    // floors
    bool bad = false;
    for (int c = 0; c < C; c++) w.set((size_t)c, 0);
    for (int c = 0; c < C && !bad; c++) {
        const int sm = mp.mux[c];  // < submaps, checked at plan time
        const int fr = floor1_decode(b, s, s.floors[mp.sub_floor[sm]], n2, Y, w, curve_base + (size_t)c * (size_t)n2);
        bad = fr == FLOOR_BAD;
        w.set((size_t)c, fr == FLOOR_USED ? 0u : CH_UNUSED | CH_SKIP);
    }
    if (bad) {
        *zeroed = 1;
        return OK;
    }
    for (int q = 0; q < mp.steps; q++) {
        const int m = mp.mag[q], a = mp.ang[q];  // < channels, checked at plan time
        if (!(w.get((size_t)m) & CH_UNUSED) || !(w.get((size_t)a) & CH_UNUSED)) {
            w.set((size_t)m, w.get((size_t)m) & ~CH_SKIP);
            w.set((size_t)a, w.get((size_t)a) & ~CH_SKIP);
        }
    }
    for (int sm = 0; sm < mp.submaps; sm++) {
        int nc = 0;
        for (int c = 0; c < C; c++)
            if (mp.mux[c] == sm) w.set((size_t)C + (size_t)nc++, (uint32_t)c);
        // a packet that ends inside the residue keeps what was decoded (the rest is zero)
        residue_decode(b, s, s.residues[mp.sub_residue[sm]], w, C, n2, spec, nc);
    }
    // inverse coupling, last step first
    for (int q = mp.steps; q-- > 0;) {
        float* M = spec + (size_t)mp.mag[q] * (size_t)n2;
        float* A = spec + (size_t)mp.ang[q] * (size_t)n2;
        for (int j = 0; j < n2; j++) {
            const float m = M[j], a = A[j];
            float nm, na;
            if (m > 0.0f) {
                if (a > 0.0f)
                    nm = m, na = m - a;
                else
                    na = m, nm = m + a;
            } else {
                if (a > 0.0f)
                    nm = m, na = m + a;
                else
                    na = m, nm = m - a;
            }
            M[j] = nm;
            A[j] = na;
        }
    }
    // the floor x residue product (an unused channel is silent)
    for (int c = 0; c < C; c++) {
        float* row = spec + (size_t)c * (size_t)n2;
        if (w.get((size_t)c) & CH_UNUSED) {
            for (int j = 0; j < n2; j++) row[j] = 0.0f;
        } else {
            for (int j = 0; j < n2; j++) row[j] = s.inv_db[w.get(curve_base + (size_t)c * (size_t)n2 + (size_t)j)] * row[j];
        }
    }
    return OK;
}

// ---- the inverse MDCT: a DCT-IV of size M = N/2 on an H = N/4-point complex FFT, in double ----
// y[n] = sum_k X[k] cos(2 pi / N (n + 1/2 + N/4)(k + 1/2)), n < N, k < M

VORBIS_HD uint32_t bitrev(uint32_t i, int lg) {
    uint32_t r = 0;
    for (int q = 0; q < lg; q++) r |= ((i >> q) & 1u) << (lg - 1 - q);
    return r;
}

// point k of the pre-twiddled input, stored at its bit-reversed place (the FFT's input permutation)
VORBIS_HD void imdct_pre(const float* X, int M, int lgH, int k, const cd* pre, cd* a) {
    const double ar = (double)X[2 * k], ai = (double)X[M - 1 - 2 * k];
    const cd wv = pre[k];
    cd z;
    z.re = ar * wv.re - ai * wv.im;
    z.im = ar * wv.im + ai * wv.re;
    a[bitrev((uint32_t)k, lgH)] = z;
}

// butterfly t (< H/2) of the stage of length len (2, 4, .. H) of the radix-2 DIT network
VORBIS_HD void fft_butterfly(cd* a, int H, int len, int t, const cd* tw) {
    const int half = len >> 1;
    const int i = (t / half) * len, k = t % half;
    const cd wv = tw[(size_t)k * (size_t)(H / len)];
    const cd u = a[i + k], x = a[i + k + half];
    cd v;
    v.re = x.re * wv.re - x.im * wv.im;
    v.im = x.re * wv.im + x.im * wv.re;
    a[i + k].re = u.re + v.re;
    a[i + k].im = u.im + v.im;
    a[i + k + half].re = u.re - v.re;
    a[i + k + half].im = u.im - v.im;
}

// sample n of the block from the FFT's output: the post-twiddle, the DCT-IV unfolding, the one
// rounding to f32
VORBIS_HD float imdct_out(const cd* a, int M, int n, const cd* post) {
    int m;
    bool neg;
    if (n < M / 2)
        m = n + M / 2, neg = false;
    else if (n < 3 * M / 2)
        m = 3 * M / 2 - 1 - n, neg = true;
    else
        m = n - 3 * M / 2, neg = true;
    // u[2j] = re(a[j] post[j]), u[M - 1 - 2j] = -im(a[j] post[j])
    double u;
    if (!(m & 1)) {
        const int j = m >> 1;
        u = a[j].re * post[j].re - a[j].im * post[j].im;
    } else {
        const int j = (M - 1 - m) >> 1;
        u = -(a[j].re * post[j].im + a[j].im * post[j].re);
    }
    return (float)(neg ? -u : u);
}

// the window of sample i of a block of n (slopes of the block's own size and of the short size)
VORBIS_HD float window_at(int n, int bs0, bool blockflag, bool prev_long, bool next_long, int i, const BlockTables& own,
                          const BlockTables& shrt) {
    int ls, le, rs, re;
    bool lshort = blockflag && !prev_long, rshort = blockflag && !next_long;
    if (lshort)
        ls = n / 4 - bs0 / 4, le = n / 4 + bs0 / 4;
    else
        ls = 0, le = n / 2;
    if (rshort)
        rs = n * 3 / 4 - bs0 / 4, re = n * 3 / 4 + bs0 / 4;
    else
        rs = n / 2, re = n;
    if (i < ls || i >= re) return 0.0f;
    if (i < le) return (lshort ? shrt.slope_up : own.slope_up)[i - ls];
    if (i < rs) return 1.0f;
    return (rshort ? shrt.slope_dn : own.slope_dn)[i - rs];
}

// Output sample i (< prev_n/4 + n/4) of the overlap of the previous windowed block (channels x
// prev_n) and the current one (channels x n): prev + cur per channel, then the mono mix (sums from
// -0.0 in channel order, divided by the channel count; a mono file's samples are copied).
VORBIS_HD float ola_mix(const float* prev, int prev_n, const float* cur, int n, int C, int i) {
    const int L = prev_n / 4 + n / 4;
    const int pi2 = prev_n / 2 + i, ci = i - L + n / 2;
    float s = -0.0f;
    for (int c = 0; c < C; c++) {
        const float pv = pi2 < prev_n ? prev[(size_t)c * (size_t)prev_n + (size_t)pi2] : 0.0f;
        const float cv = ci >= 0 ? cur[(size_t)c * (size_t)n + (size_t)ci] : 0.0f;
        const float v = pv + cv;
        if (C == 1) return v;
        s = s + v;
    }
    return s / (float)C;
}

}  // namespace vorbis_core
