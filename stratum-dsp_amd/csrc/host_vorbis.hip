// host_vorbis.hip — Ogg Vorbis (Vorbis I) for the decode front-end (host_formats.hip hands over
// the first logical stream's packets and the last page's granule position).
//
// The reference decodes Vorbis through symphonia's Vorbis codec (Cargo.toml:15, features =
// ["all"]), whose f32 buffers the examples mix to mono (examples/analyze_file.rs:25-180).  This
// decoder follows the Vorbis I specification: the identification and setup headers (codebooks
// with their Huffman trees and VQ lookup types 1 / 2, floor type 1, residue types 0 / 1 / 2,
// mapping type 0 with square-polar channel coupling, modes), and per audio packet the floor
// curves, the residue vectors, inverse coupling, the floor x residue product, the inverse MDCT
// (here through a DCT-IV on an N/4-point complex FFT), the power-complementary window with its
// short / long transitions and the overlap-add, returning the samples between the previous
// and the current window centres (the first audio packet returns none); the output is cut at
// the last page's granule position.  Floor type 0 (LSP, unused by current encoders) is a
// decoding error.  A lossy decoder's output depends on its arithmetic, so parity with
// symphonia is unpinned: tests/vorbis_enc.py writes spec-conforming streams and the tests check
// the decoded samples against the encoder's own synthesis of the quantised spectra.
//
// The packet-level code (bit reader, Huffman walk, floor 1, residues, coupling, the inverse MDCT,
// the window, the overlap-add with the mono mix) is vorbis_core.hpp, the code the device kernels
// (k_vorbis.hip) run.  Here: the setup header's parse into the core's flat structs, the tables of
// transcendentals the core reads, the plan of a stream, and the packet loop of the host decoder.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "vorbis_host.hpp"

namespace {

bool fail(std::string* err, const std::string& m) {
    *err = m;
    return false;
}

namespace vc = vorbis_core;

// LSB-first bit reader (Vorbis packs fields from the least significant bit of each byte)
using LBits = vc::Bits;
using vc::ilog;

float float32_unpack(uint32_t x) {
    const double mant = (double)(x & 0x1fffff);
    const int e = (int)((x & 0x7fe00000u) >> 21);
    const double v = std::ldexp(mant, e - 788);
    return (float)((x & 0x80000000u) ? -v : v);
}

uint32_t lookup1_values(uint32_t entries, uint32_t dims) {
    uint32_t r = (uint32_t)std::floor(std::pow((double)entries, 1.0 / dims));
    auto pw = [&](uint64_t b) {
        uint64_t acc = 1;
        for (uint32_t i = 0; i < dims; i++) {
            acc *= b;
            if (acc > entries) return acc;
        }
        return acc;
    };
    while (r > 0 && pw(r) > entries) r--;
    while (pw((uint64_t)r + 1) <= entries) r++;
    return r;
}

struct Codebook {
    uint32_t dims = 0, entries = 0;
    std::vector<int> len;           // codeword length per entry (0 = unused)
    std::vector<int32_t> tree;      // binary tree: node 2i / 2i+1 children; >= 0 node, < 0 -(entry+1)
    int lookup = 0;
    std::vector<float> vq;          // entries x dims vector values (lookup 1 / 2)
    bool build(std::string* err) {
        // codeword assignment of the specification (lowest available codeword of each length, in
        // entry order), then a decoding tree walked one bit at a time, first bit = codeword MSB
        uint32_t marker[33] = {0};
        std::vector<uint32_t> code(entries, 0);
        int used = 0, single = -1;
        for (uint32_t i = 0; i < entries; i++)
            if (len[i] > 0) used++, single = (int)i;
        tree.assign(2, 0);
        if (used == 0) return true;
        if (used == 1) {  // a single used entry: codeword '0' of length 1 (both branches decode it)
            tree[0] = tree[1] = -(single + 1);
            return true;
        }
        for (uint32_t i = 0; i < entries; i++) {
            const int l = len[i];
            if (l <= 0) continue;
            const uint32_t entry = marker[l];
            if (l < 32 && (entry >> l)) return fail(err, "Vorbis codebook overspecified");
            code[i] = entry;
            for (int j = l; j > 0; j--) {
                if (marker[j] & 1) {
                    if (j == 1)
                        marker[1]++;
                    else
                        marker[j] = marker[j - 1] << 1;
                    break;
                }
                marker[j]++;
            }
            uint32_t e2 = entry;
            for (int j = l + 1; j < 33; j++) {
                if ((marker[j] >> 1) == e2) {
                    e2 = marker[j];
                    marker[j] = marker[j - 1] << 1;
                } else {
                    break;
                }
            }
        }
        for (uint32_t i = 0; i < entries; i++) {
            const int l = len[i];
            if (l <= 0) continue;
            int node = 0;
            for (int b = l - 1; b >= 0; b--) {
                const int bit = (int)((code[i] >> b) & 1);
                int32_t& slot = tree[(size_t)(2 * node + bit)];
                if (b == 0) {
                    if (slot != 0) return fail(err, "Vorbis codebook collision");
                    slot = -(int32_t)(i + 1);
                } else {
                    if (slot < 0) return fail(err, "Vorbis codebook collision");
                    if (slot == 0) {
                        slot = (int32_t)(tree.size() / 2);
                        tree.push_back(0);
                        tree.push_back(0);
                    }
                    node = tree[(size_t)(2 * node + bit)];
                }
            }
        }
        return true;
    }
};

struct Floor1 {
    int partitions = 0, multiplier = 1, rangebits = 0;
    std::vector<int> part_class, class_dim, class_sub, class_master;
    std::vector<std::vector<int>> sub_books;
    std::vector<int> X;  // x list (values)
};

struct Residue {
    int type = 0;
    uint32_t begin = 0, end = 0, psize = 1;
    int classes = 1, classbook = 0;
    std::vector<std::array<int, 8>> books;  // per class, per pass (-1 unused)
};

struct Mapping {
    int submaps = 1;
    std::vector<int> mag, ang, mux, sub_floor, sub_residue;
};

struct Mode {
    int blockflag = 0, mapping = 0;
};

struct Vorbis {
    int channels = 0;
    uint32_t rate = 0;
    int bs[2] = {0, 0};
    std::vector<Codebook> books;
    std::vector<Floor1> floors;
    std::vector<Residue> residues;
    std::vector<Mapping> maps;
    std::vector<Mode> modes;
};

bool read_setup(LBits& b, Vorbis& v, std::string* err) {
    const int nbooks = (int)b.read(8) + 1;
    v.books.resize((size_t)nbooks);
    for (Codebook& c : v.books) {
        if (b.read(24) != 0x564342) return fail(err, "Vorbis codebook sync lost");
        c.dims = b.read(16);
        c.entries = b.read(24);
        if (c.entries == 0 || c.entries > (1u << 20)) return fail(err, "unsupported Vorbis codebook size");
        c.len.assign(c.entries, 0);
        if (!b.bit()) {  // unordered
            const bool sparse = b.bit();
            for (uint32_t i = 0; i < c.entries; i++) {
                if (sparse && !b.bit()) continue;
                c.len[i] = (int)b.read(5) + 1;
            }
        } else {  // ordered
            uint32_t cur = 0;
            int l = (int)b.read(5) + 1;
            while (cur < c.entries) {
                const uint32_t num = b.read(ilog(c.entries - cur));
                if (cur + num > c.entries || l > 32) return fail(err, "malformed Vorbis codebook");
                for (uint32_t i = 0; i < num; i++) c.len[cur + i] = l;
                cur += num;
                l++;
            }
        }
        c.lookup = (int)b.read(4);
        if (c.lookup == 1 || c.lookup == 2) {
            const float mn = float32_unpack(b.read(32)), dl = float32_unpack(b.read(32));
            const int vbits = (int)b.read(4) + 1;
            const bool seq = b.bit();
            // sizes in 64 bits: entries (24 bits) x dims (16 bits) would wrap in 32
            const uint64_t nvq = (uint64_t)c.entries * (uint64_t)c.dims;
            if (c.dims == 0 || nvq > (1u << 24)) return fail(err, "malformed Vorbis codebook");
            const uint32_t nval = c.lookup == 1 ? lookup1_values(c.entries, c.dims) : (uint32_t)nvq;
            if (nval == 0 || nval > (1u << 24)) return fail(err, "malformed Vorbis codebook");
            std::vector<uint32_t> mult(nval);
            for (uint32_t i = 0; i < nval; i++) mult[i] = b.read(vbits);
            c.vq.assign((size_t)c.entries * c.dims, 0.0f);
            for (uint32_t e = 0; e < c.entries; e++) {
                float last = 0.0f;
                uint32_t div = 1;
                for (uint32_t d = 0; d < c.dims; d++) {
                    const uint32_t off = c.lookup == 1 ? (e / div) % nval : e * c.dims + d;
                    const float val = (float)mult[off] * dl + mn + last;
                    if (seq) last = val;
                    c.vq[(size_t)e * c.dims + d] = val;
                    if (c.lookup == 1) div *= nval;
                }
            }
        } else if (c.lookup != 0) {
            return fail(err, "unsupported Vorbis lookup type");
        }
        if (b.over) return fail(err, "truncated Vorbis setup header");
        if (!c.build(err)) return false;
    }
    const int ntime = (int)b.read(6) + 1;
    for (int i = 0; i < ntime; i++)
        if (b.read(16) != 0) return fail(err, "malformed Vorbis setup header");
    const int nfloors = (int)b.read(6) + 1;
    v.floors.resize((size_t)nfloors);
    for (Floor1& f : v.floors) {
        const int type = (int)b.read(16);
        if (type == 0) return fail(err, "unsupported Vorbis floor type 0");
        if (type != 1) return fail(err, "malformed Vorbis floor");
        f.partitions = (int)b.read(5);
        int maxc = -1;
        for (int i = 0; i < f.partitions; i++) {
            f.part_class.push_back((int)b.read(4));
            maxc = std::max(maxc, f.part_class.back());
        }
        for (int c = 0; c <= maxc; c++) {
            f.class_dim.push_back((int)b.read(3) + 1);
            f.class_sub.push_back((int)b.read(2));
            f.class_master.push_back(f.class_sub.back() ? (int)b.read(8) : -1);
            std::vector<int> sb;
            for (int j = 0; j < (1 << f.class_sub.back()); j++) sb.push_back((int)b.read(8) - 1);
            f.sub_books.push_back(sb);
        }
        f.multiplier = (int)b.read(2) + 1;
        f.rangebits = (int)b.read(4);
        f.X = {0, 1 << f.rangebits};
        for (int i = 0; i < f.partitions; i++)
            for (int j = 0; j < f.class_dim[(size_t)f.part_class[(size_t)i]]; j++) f.X.push_back((int)b.read(f.rangebits));
        {
            // Vorbis I §7.2.2: the X list may not repeat a value (the curve would divide by zero)
            std::vector<int> xs = f.X;
            std::sort(xs.begin(), xs.end());
            if (std::adjacent_find(xs.begin(), xs.end()) != xs.end() || xs.size() > 65) return fail(err, "malformed Vorbis floor");
        }
        for (int bk : f.class_master)
            if (bk >= nbooks) return fail(err, "malformed Vorbis floor");
        for (auto& sb : f.sub_books)
            for (int bk : sb)
                if (bk >= nbooks) return fail(err, "malformed Vorbis floor");
    }
    const int nres = (int)b.read(6) + 1;
    v.residues.resize((size_t)nres);
    for (Residue& r : v.residues) {
        r.type = (int)b.read(16);
        if (r.type > 2) return fail(err, "malformed Vorbis residue");
        r.begin = b.read(24);
        r.end = b.read(24);
        r.psize = b.read(24) + 1;
        r.classes = (int)b.read(6) + 1;
        r.classbook = (int)b.read(8);
        if (r.classbook >= nbooks) return fail(err, "malformed Vorbis residue");
        std::vector<int> casc((size_t)r.classes);
        for (int c = 0; c < r.classes; c++) {
            int lo = (int)b.read(3);
            int hi = b.bit() ? (int)b.read(5) : 0;
            casc[(size_t)c] = hi * 8 + lo;
        }
        r.books.assign((size_t)r.classes, std::array<int, 8>{-1, -1, -1, -1, -1, -1, -1, -1});
        for (int c = 0; c < r.classes; c++)
            for (int j = 0; j < 8; j++)
                if (casc[(size_t)c] & (1 << j)) {
                    r.books[(size_t)c][(size_t)j] = (int)b.read(8);
                    if (r.books[(size_t)c][(size_t)j] >= nbooks) return fail(err, "malformed Vorbis residue");
                }
    }
    const int nmaps = (int)b.read(6) + 1;
    v.maps.resize((size_t)nmaps);
    for (Mapping& m : v.maps) {
        if (b.read(16) != 0) return fail(err, "malformed Vorbis mapping");
        m.submaps = b.bit() ? (int)b.read(4) + 1 : 1;
        if (b.bit()) {
            const int steps = (int)b.read(8) + 1;
            const int w = ilog((uint32_t)(v.channels - 1));
            for (int s = 0; s < steps; s++) {
                m.mag.push_back((int)b.read(w));
                m.ang.push_back((int)b.read(w));
                if (m.mag.back() == m.ang.back() || m.mag.back() >= v.channels || m.ang.back() >= v.channels)
                    return fail(err, "malformed Vorbis coupling");
            }
        }
        if (b.read(2) != 0) return fail(err, "malformed Vorbis mapping");
        m.mux.assign((size_t)v.channels, 0);
        if (m.submaps > 1)
            for (int c = 0; c < v.channels; c++) {
                m.mux[(size_t)c] = (int)b.read(4);
                // Vorbis I §4.2.4: a mux value past the submap count makes the stream undecodable
                if (m.mux[(size_t)c] >= m.submaps) return fail(err, "malformed Vorbis mapping");
            }
        for (int s = 0; s < m.submaps; s++) {
            b.read(8);
            m.sub_floor.push_back((int)b.read(8));
            m.sub_residue.push_back((int)b.read(8));
            if (m.sub_floor.back() >= nfloors || m.sub_residue.back() >= nres) return fail(err, "malformed Vorbis mapping");
        }
    }
    const int nmodes = (int)b.read(6) + 1;
    v.modes.resize((size_t)nmodes);
    for (Mode& md : v.modes) {
        md.blockflag = (int)b.read(1);
        if (b.read(16) != 0 || b.read(16) != 0) return fail(err, "malformed Vorbis mode");
        md.mapping = (int)b.read(8);
        if (md.mapping >= nmaps) return fail(err, "malformed Vorbis mode");
    }
    if (!b.bit() || b.over) return fail(err, "malformed Vorbis setup header");
    return true;
}

// the parsed setup into the core's flat structs (every index was checked by read_setup)
void flatten(const Vorbis& v, sdsp_vorbis_setup* s) {
    s->channels = v.channels;
    s->rate = v.rate;
    s->bs[0] = v.bs[0], s->bs[1] = v.bs[1];
    for (const Codebook& c : v.books) {
        vc::Book b{};
        b.dims = c.dims, b.entries = c.entries, b.lookup = c.lookup;
        b.tree_off = (uint32_t)s->trees.size(), b.tree_n = (uint32_t)c.tree.size();
        s->trees.insert(s->trees.end(), c.tree.begin(), c.tree.end());
        b.vq_off = (uint32_t)s->vq.size();
        s->vq.insert(s->vq.end(), c.vq.begin(), c.vq.end());
        s->books.push_back(b);
    }
    for (const Floor1& f : v.floors) {
        vc::Floor o{};
        o.partitions = f.partitions, o.multiplier = f.multiplier, o.rangebits = f.rangebits, o.nv = (int)f.X.size();
        for (int i = 0; i < f.partitions; i++) o.part_class[i] = (uint8_t)f.part_class[(size_t)i];
        for (size_t c = 0; c < f.class_dim.size(); c++) {
            o.class_dim[c] = (uint8_t)f.class_dim[c];
            o.class_sub[c] = (uint8_t)f.class_sub[c];
            o.class_master[c] = (int16_t)f.class_master[c];
            for (int j = 0; j < 8; j++) o.sub_books[c][j] = j < (int)f.sub_books[c].size() ? (int16_t)f.sub_books[c][(size_t)j] : (int16_t)-1;
        }
        const int nv = o.nv;
        for (int i = 0; i < nv; i++) o.X[i] = (uint16_t)f.X[(size_t)i];
        for (int i = 2; i < nv; i++) {  // the low / high neighbours among the earlier points
            int lo = 0, hi = 1, lx = -1, hx = 1 << 30;
            for (int j = 0; j < i; j++) {
                if (f.X[(size_t)j] < f.X[(size_t)i] && f.X[(size_t)j] > lx) lx = f.X[(size_t)j], lo = j;
                if (f.X[(size_t)j] > f.X[(size_t)i] && f.X[(size_t)j] < hx) hx = f.X[(size_t)j], hi = j;
            }
            o.lo[i] = (uint8_t)lo, o.hi[i] = (uint8_t)hi;
        }
        std::vector<int> order((size_t)nv);
        for (int i = 0; i < nv; i++) order[(size_t)i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return f.X[(size_t)a] < f.X[(size_t)c]; });
        for (int i = 0; i < nv; i++) o.order[i] = (uint8_t)order[(size_t)i];
        s->floors.push_back(o);
    }
    for (const Residue& r : v.residues) {
        vc::Residue o{};
        o.type = r.type, o.begin = r.begin, o.end = r.end, o.psize = r.psize, o.classes = r.classes, o.classbook = r.classbook;
        for (int c = 0; c < 64; c++)
            for (int j = 0; j < 8; j++) o.books[c][j] = c < r.classes ? (int16_t)r.books[(size_t)c][(size_t)j] : (int16_t)-1;
        s->residues.push_back(o);
    }
    for (const Mapping& m : v.maps) {
        vc::Mapping o{};
        o.submaps = m.submaps, o.steps = (int)m.mag.size();
        for (size_t q = 0; q < m.mag.size(); q++) o.mag[q] = (uint8_t)m.mag[q], o.ang[q] = (uint8_t)m.ang[q];
        for (int c = 0; c < v.channels; c++) o.mux[c] = (uint8_t)m.mux[(size_t)c];
        for (int q = 0; q < m.submaps; q++) o.sub_floor[q] = (uint8_t)m.sub_floor[(size_t)q], o.sub_residue[q] = (uint8_t)m.sub_residue[(size_t)q];
        s->maps.push_back(o);
    }
    for (const Mode& md : v.modes) s->modes.push_back(vc::Mode{(uint8_t)md.blockflag, (uint8_t)md.mapping});
}

}  // namespace

// floor 1 inverse dB table: -140 dB .. 0 dB in steps of 140/256 dB (table[255] = 1)
const float* sdsp_vorbis_inv_db() {
    static float tab[256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (int k = 0; k < 256; k++) tab[k] = (float)std::pow(10.0, -(255 - k) * (140.0 / 256.0) / 20.0);
    });
    return tab;
}

// The transcendentals of block size N (M = N/2, H = N/4), each with the expression the decoder has
// always used: the DCT-IV's pre- and post-twiddles, the FFT's twiddles exp(-2 pi i k / H), and the
// two slopes of the power-complementary window of length N/2.
const sdsp_vorbis_tables& sdsp_vorbis_block_tables(int N) {
    static std::mutex mu;
    static std::unique_ptr<sdsp_vorbis_tables> cache[32];
    int lg = 0;
    while ((1 << lg) < N) lg++;
    std::lock_guard<std::mutex> lk(mu);
    std::unique_ptr<sdsp_vorbis_tables>& slot = cache[lg & 31];
    if (slot) return *slot;
    slot.reset(new sdsp_vorbis_tables());
    sdsp_vorbis_tables& t = *slot;
    t.N = N;
    const int M = N / 2, H = M / 2;
    t.pre.resize((size_t)H), t.post.resize((size_t)H), t.tw.resize((size_t)H / 2);
    for (int k = 0; k < H; k++) {
        const double ph = -M_PI * (4.0 * k + 1.0) / (4.0 * M);
        t.pre[(size_t)k] = vc::cd{std::cos(ph), std::sin(ph)};
    }
    for (int j = 0; j < H; j++) {
        const double ph = -M_PI * j / (double)M;
        t.post[(size_t)j] = vc::cd{std::cos(ph), std::sin(ph)};
    }
    const size_t n = (size_t)H;
    for (size_t k = 0; k < n / 2; k++)
        t.tw[k] = vc::cd{std::cos(-2.0 * M_PI * (double)k / (double)n), std::sin(-2.0 * M_PI * (double)k / (double)n)};
    const int len = N / 2;
    t.up.resize((size_t)len), t.dn.resize((size_t)len);
    for (int right = 0; right < 2; right++)
        for (int i = 0; i < len; i++) {
            const double x = ((double)i + 0.5) / (double)len * M_PI / 2.0 + (right ? M_PI / 2.0 : 0.0);
            const double s = std::sin(x);
            (right ? t.dn : t.up)[(size_t)i] = (float)std::sin(M_PI / 2.0 * s * s);
        }
    return t;
}

vorbis_core::Setup sdsp_vorbis_setup::view() const {
    vc::Setup s{};
    s.channels = channels, s.bs0 = bs[0], s.bs1 = bs[1], s.nmodes = (int32_t)modes.size();
    s.books = books.data(), s.trees = trees.data(), s.vq = vq.data(), s.floors = floors.data();
    s.residues = residues.data(), s.maps = maps.data(), s.modes = modes.data(), s.inv_db = sdsp_vorbis_inv_db();
    return s;
}

bool sdsp_vorbis_plan_packets(const std::vector<std::vector<uint8_t>>& packets, int64_t last_granule, sdsp_vorbis_plan* plan,
                              std::string* err) {
    if (packets.size() < 3) return fail(err, "truncated Vorbis stream");
    Vorbis v;
    {
        const std::vector<uint8_t>& h = packets[0];
        if (h.size() < 30) return fail(err, "malformed Vorbis identification header");
        LBits b(h.data() + 7, h.size() - 7);
        if (b.read(32) != 0) return fail(err, "unsupported Vorbis version");
        v.channels = (int)b.read(8);
        v.rate = b.read(32);
        b.read(32), b.read(32), b.read(32);
        v.bs[0] = 1 << b.read(4);
        v.bs[1] = 1 << b.read(4);
        if (v.channels < 1 || v.rate == 0 || v.bs[0] < 64 || v.bs[1] > 8192 || v.bs[0] > v.bs[1] || !b.bit())
            return fail(err, "malformed Vorbis identification header");
    }
    {
        const std::vector<uint8_t>& s = packets[2];
        if (s.size() < 7 || s[0] != 5 || std::memcmp(s.data() + 1, "vorbis", 6) != 0)
            return fail(err, "missing Vorbis setup header");
        LBits b(s.data() + 7, s.size() - 7);
        if (!read_setup(b, v, err)) return false;
    }
    flatten(v, &plan->setup);
    const vc::Setup sv = plan->setup.view();
    // the audio packets' first bits: block size, window shape, place in the output
    size_t kept_bytes = 0;
    for (size_t pi = 3; pi < packets.size(); pi++) kept_bytes += packets[pi].size();
    plan->bytes.reserve(kept_bytes + 8);
    int prev_n = 0;
    uint64_t total = 0;
    for (size_t pi = 3; pi < packets.size(); pi++) {
        const std::vector<uint8_t>& pk = packets[pi];
        LBits b(pk.data(), pk.size());
        int mode_no;
        bool prev_long, next_long;
        if (!vc::packet_header(sv, b, pk.size(), &mode_no, &prev_long, &next_long)) continue;
        const vc::Mode md = plan->setup.modes[(size_t)mode_no];
        sdsp_vorbis_packet p{};
        p.off = plan->bytes.size();
        p.size = (uint32_t)pk.size();
        p.n = (uint16_t)v.bs[md.blockflag];
        p.prev_n = (uint16_t)prev_n;
        p.blockflag = md.blockflag, p.prev_long = prev_long, p.next_long = next_long;
        p.out = total;
        if (prev_n) total += (uint64_t)(prev_n / 4 + p.n / 4);
        prev_n = p.n;
        plan->bytes.insert(plan->bytes.end(), pk.begin(), pk.end());
        plan->packets.push_back(p);
    }
    plan->total = total;
    plan->frames = total;
    if (last_granule >= 0 && (uint64_t)last_granule < total) plan->frames = (uint64_t)last_granule;
    return true;
}

int sdsp_vorbis_plan_ogg(const uint8_t* f, size_t n, sdsp_vorbis_plan* plan, std::string* err) {
    std::vector<std::vector<uint8_t>> packets;
    int64_t last_granule = -1;
    sdsp_ogg_demux(f, n, &packets, &last_granule);
    if (packets.empty()) return fail(err, "no Ogg packets"), -1;
    const std::vector<uint8_t>& h = packets[0];
    if (!(h.size() >= 7 && h[0] == 0x01 && std::memcmp(h.data() + 1, "vorbis", 6) == 0)) return 0;
    return sdsp_vorbis_plan_packets(packets, last_granule, plan, err) ? 1 : -1;
}

// the packet loop: each kept packet's spectra, the inverse MDCT and window of every channel, the
// overlap-add with the previous block straight into the mono track
void sdsp_vorbis_decode_plan(const sdsp_vorbis_plan& plan, std::vector<float>* out) {
    const vc::Setup sv = plan.setup.view();
    const int C = sv.channels, nmax = sv.bs1;
    std::vector<uint32_t> work(vc::work_words(C, nmax / 2));
    const vc::Work w{work.data(), 1, work.size()};
    int32_t ybuf[vc::FLOOR_MAX_POINTS];
    const vc::YStore Y{ybuf, 1};
    std::vector<float> spec((size_t)C * (size_t)(nmax / 2)), prev((size_t)C * (size_t)nmax), cur((size_t)C * (size_t)nmax);
    std::vector<vc::cd> a((size_t)nmax / 4);
    const vc::BlockTables ts = sdsp_vorbis_block_tables(sv.bs0).view();
    out->clear();
    out->reserve(plan.total);
    for (const sdsp_vorbis_packet& p : plan.packets) {
        int32_t zeroed = 0;
        vc::decode_packet(sv, plan.bytes.data() + p.off, p.size, w, Y, spec.data(), &zeroed);
        const int n = p.n, M = n / 2, H = n / 4;
        int lgH = 0;
        while ((1 << lgH) < H) lgH++;
        const vc::BlockTables tb = sdsp_vorbis_block_tables(n).view();
        for (int c = 0; c < C; c++) {
            const float* X = spec.data() + (size_t)c * (size_t)M;
            for (int k = 0; k < H; k++) vc::imdct_pre(X, M, lgH, k, tb.pre, a.data());
            for (int len = 2; len <= H; len <<= 1)
                for (int t = 0; t < H / 2; t++) vc::fft_butterfly(a.data(), H, len, t, tb.tw);
            float* y = cur.data() + (size_t)c * (size_t)n;
            for (int i = 0; i < n; i++)
                y[i] = vc::imdct_out(a.data(), M, i, tb.post) * vc::window_at(n, sv.bs0, p.blockflag, p.prev_long, p.next_long, i, tb, ts);
        }
        if (p.prev_n) {
            const int L = p.prev_n / 4 + n / 4;
            for (int i = 0; i < L; i++) out->push_back(vc::ola_mix(prev.data(), p.prev_n, cur.data(), n, C, i));
        }
        prev.swap(cur);
    }
    out->resize(plan.frames);
}

bool sdsp_decode_vorbis(const std::vector<std::vector<uint8_t>>& packets, int64_t last_granule, std::vector<float>* out,
                        uint32_t* sr, std::string* err) {
    sdsp_vorbis_plan plan;
    if (!sdsp_vorbis_plan_packets(packets, last_granule, &plan, err)) return false;
    sdsp_vorbis_decode_plan(plan, out);
    *sr = plan.setup.rate;
    return true;
}
