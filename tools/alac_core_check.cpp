// alac_core_check — the shared ALAC packet-level code (stratum-dsp_amd/csrc/alac_core.hpp) and the
// shared PCM conversion (pcm_core.hpp) under the host sanitizers, CPU only.  The device kernels run
// this same code, so a read or write out of range, or undefined arithmetic, here is one there.
//
// Writes a set of ALAC streams with a small encoder of its own (SCE / CPE elements, the adaptive
// Golomb coder with zero runs and escapes, the sign-adaptive predictor with numactive 0 / 31 / 4 / 8 /
// 16, modes 0 and 15, stereo mixes, 16 / 20 / 24 / 32 bits with shifted low bytes, raw elements,
// frame lengths 16 to 1024, partial packets) in CAF and ISO MP4, then pushes every stream and a few
// thousand variants (a packet truncated or bit-flipped, the magic cookie bit-flipped, the file
// truncated) through the host decoder (sdsp_decode_audio_bytes) and through the plan and the CPU
// phased decode (alac_phased::decode: every packet into its own slot, offsets, gather) and requires
// the same status, text and bit-identical samples.  Also runs the PCM plans and the planned
// conversion on RIFF/WAVE and AIFF files truncated at every header byte against the host decoder.
// Ends with "alac_core_check: ok" and status 0; any sanitizer report or mismatch is a failure.
//
// Build and run (from the repository root):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ tools/alac_core_check.cpp stratum-dsp_amd/csrc/host_*.hip -o tools/alac_core_check && tools/alac_core_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../stratum-dsp_amd/csrc/alac_phased.hpp"
#include "../stratum-dsp_amd/csrc/flac_host.hpp"
#include "../stratum-dsp_amd/csrc/lossless_host.hpp"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
};

struct BitWriter {
    std::vector<uint8_t> out;
    uint64_t acc = 0;
    int n = 0;
    void put(uint64_t v, int k) {  // k <= 32
        if (k == 0) return;
        acc = (acc << k) | (v & ((1ull << k) - 1));
        n += k;
        while (n >= 8) {
            n -= 8;
            out.push_back((uint8_t)(acc >> n));
        }
        acc &= (1ull << n) - 1;
    }
    void align() {
        if (n) put(0, 8 - n);
    }
};

using Cfg = alac_core::Config;
constexpr int QBSHIFT = 9, MMULSHIFT = 2, MDENSHIFT = 6, MOFF = 16, BITOFF = 24, MAX_PREFIX = 9;

int clz32(uint32_t x) { return x ? __builtin_clz(x) : 32; }
int64_t sext(int64_t v, int bits) {
    v &= (1ll << bits) - 1;
    return (v >> (bits - 1)) ? v - (1ll << bits) : v;
}
int sign_of(int64_t v) { return (v > 0) - (v < 0); }

// one adaptive-Golomb value: pre = x / m ones, a zero, then r + 1 in k bits (r > 0) or k - 1 zero
// bits (r = 0); an escape (9 ones, then x in escape_bits) from pre >= 9
void code(BitWriter& w, uint32_t x, uint32_t m, int k, int escape_bits) {
    const uint32_t pre = m ? x / m : MAX_PREFIX, r = m ? x % m : 0;
    if (pre >= (uint32_t)MAX_PREFIX) {
        w.put((1u << MAX_PREFIX) - 1, MAX_PREFIX);
        w.put(x, escape_bits);
        return;
    }
    w.put((1u << pre) - 1, (int)pre);
    w.put(0, 1);
    if (k == 1) return;
    if (r == 0)
        w.put(0, k - 1);
    else
        w.put(r + 1, k);
}

// dyn_comp: the inverse of the decoder's dyn_decomp (the same state updates)
void ag_encode(BitWriter& w, const std::vector<int64_t>& res, const Cfg& c, int pbf, int chan_bits) {
    const uint32_t pb = (uint32_t)(c.pb * pbf) / 4, wb = (1u << c.kb) - 1;
    uint32_t mb = (uint32_t)c.mb, zmode = 0;
    size_t i = 0;
    const size_t n = res.size();
    while (i < n) {
        int k = 31 - clz32((mb >> QBSHIFT) + 3);
        if (k > c.kb) k = c.kb;
        const uint32_t m = (1u << k) - 1;
        const int64_t x = res[i];
        const uint32_t nd = (uint32_t)(x >= 0 ? 2 * x : -2 * x - 1);
        const uint32_t v = nd - zmode;
        code(w, v, m, k, chan_bits);
        i++;
        mb = pb * (v + zmode) + mb - ((pb * mb) >> QBSHIFT);
        if (v > 0xFFFF) mb = 0xFFFF;
        zmode = 0;
        if (((mb << MMULSHIFT) < (1u << QBSHIFT)) && i < n) {
            zmode = 1;
            const int kz = clz32(mb) - BITOFF + (int)((mb + MOFF) >> MDENSHIFT);
            const uint32_t mz = ((1u << kz) - 1) & wb;
            uint32_t run = 0;
            while (i + run < n && res[i + run] == 0 && run < 65535) run++;
            code(w, run, mz, kz, 16);
            i += run;
            if (run >= 65535) zmode = 0;
            mb = 0;
        }
    }
}

// residuals pc with unpc_block(pc) == out; the coefficients adapt as in the decoder
std::vector<int64_t> predict(const std::vector<int64_t>& out, std::vector<int> coefs, int na, int chan_bits, int den) {
    const int n = (int)out.size();
    std::vector<int64_t> pc((size_t)n, 0);
    if (!n) return pc;
    pc[0] = out[0];
    if (na == 0) return out;
    if (na == 31) {
        for (int j = 1; j < n; j++) pc[j] = sext(out[j] - out[j - 1], chan_bits);
        return pc;
    }
    for (int j = 1; j < n && j <= na; j++) pc[j] = sext(out[j] - out[j - 1], chan_bits);
    const int64_t den_half = den > 0 ? 1ll << (den - 1) : 0;
    const int lim = na + 1;
    for (int j = lim; j < n; j++) {
        const int64_t top = out[j - lim];
        int64_t s = 0;
        for (int k = 0; k < na; k++) s = (s + coefs[k] * (out[j - 1 - k] - top)) & 0xFFFFFFFFll;
        const int64_t pred = sext(s + den_half, 32) >> den;
        const int64_t d = sext(out[j] - top - pred, chan_bits);
        pc[j] = d;
        int64_t del0 = d;
        const int sg = sign_of(d);
        for (int k = na - 1; k >= 0 && sg != 0; k--) {
            const int64_t dd = sext(top - out[j - 1 - k], 32);
            const int sgn = sign_of(dd);
            coefs[k] = (int)sext(coefs[k] - sg * sgn, 16);
            del0 -= (na - k) * ((sg * sgn * dd) >> den);
            if (sg > 0 ? del0 <= 0 : del0 >= 0) break;
        }
    }
    return pc;
}

struct ChSpec {
    int mode = 0, den = 9, pbf = 4;
    std::vector<int> coefs;  // numactive = coefs.size(); 31 zeros: first-order
};
struct Spec {
    bool escape = false;
    int shift = 0;  // bytes
    int mix_bits = 0, mix_res = 0;
    ChSpec ch[2];
};

// one SCE (1 channel) or CPE (2) element, END, padding
std::vector<uint8_t> frame(const Cfg& c, const std::vector<std::vector<int64_t>>& chans, const Spec& sp) {
    BitWriter w;
    const int ech = (int)chans.size(), n = (int)chans[0].size(), shift = 8 * sp.shift, bits = c.bit_depth;
    const bool partial = (uint32_t)n != c.frame_length;
    w.put(ech == 2 ? 1 : 0, 3);
    w.put(0, 4);
    w.put(0, 12);
    w.put((partial ? 8 : 0) | ((sp.escape ? 0 : sp.shift) << 1) | (sp.escape ? 1 : 0), 4);
    if (partial) {
        w.put((uint32_t)n >> 16, 16);
        w.put((uint32_t)n & 0xFFFF, 16);
    }
    if (sp.escape) {
        for (int i = 0; i < n; i++)
            for (int e = 0; e < ech; e++) {
                const int64_t v = chans[e][i];
                if (bits <= 16) {
                    w.put((uint64_t)v, bits);
                } else {
                    w.put((uint64_t)(v >> (bits - 16)), 16);
                    w.put((uint64_t)v & ((1ull << (bits - 16)) - 1), bits - 16);
                }
            }
    } else {
        const int chan_bits = bits - shift + (ech == 2 ? 1 : 0);
        std::vector<std::vector<int64_t>> hi((size_t)ech), lo((size_t)ech), mixed;
        for (int e = 0; e < ech; e++)
            for (int64_t v : chans[e]) {
                hi[e].push_back(v >> shift);
                lo[e].push_back(v & ((1ll << shift) - 1));
            }
        if (ech == 2) {
            std::vector<int64_t> u((size_t)n), v((size_t)n);
            for (int i = 0; i < n; i++) {
                v[i] = hi[0][i] - hi[1][i];
                u[i] = sp.mix_res ? hi[1][i] + ((sp.mix_res * v[i]) >> sp.mix_bits) : hi[0][i];
                if (!sp.mix_res) v[i] = hi[1][i];
            }
            mixed = {u, v};
            w.put((uint64_t)sp.mix_bits, 8);
            w.put((uint64_t)sp.mix_res & 0xFF, 8);
        } else {
            mixed = hi;
        }
        for (int e = 0; e < ech; e++) {
            const ChSpec& ch = sp.ch[e];
            w.put((uint64_t)((ch.mode << 4) | ch.den), 8);
            w.put((uint64_t)((ch.pbf << 5) | (int)ch.coefs.size()), 8);
            for (int q : ch.coefs) w.put((uint64_t)q, 16);
        }
        if (shift)
            for (int i = 0; i < n; i++)
                for (int e = 0; e < ech; e++) w.put((uint64_t)lo[e][i], shift);
        for (int e = 0; e < ech; e++) {
            const ChSpec& ch = sp.ch[e];
            const int na = (int)ch.coefs.size();
            std::vector<int64_t> src;
            for (int64_t x : mixed[e]) src.push_back(sext(x, chan_bits));
            std::vector<int64_t> res = predict(src, ch.coefs, na, chan_bits, ch.den);
            if (ch.mode == 15) res = predict(res, {}, 31, chan_bits, 0);  // the decoder's first-order pass comes first
            ag_encode(w, res, c, ch.pbf, chan_bits);
        }
    }
    w.put(7, 3);
    w.align();
    return w.out;
}

void be(std::vector<uint8_t>& o, uint64_t v, int bytes) {
    for (int i = bytes - 1; i >= 0; i--) o.push_back((uint8_t)(v >> (8 * i)));
}
void tag(std::vector<uint8_t>& o, const char* t) { o.insert(o.end(), t, t + 4); }
void cat(std::vector<uint8_t>& o, const std::vector<uint8_t>& b) { o.insert(o.end(), b.begin(), b.end()); }

std::vector<uint8_t> cookie(const Cfg& c) {
    std::vector<uint8_t> o;
    be(o, c.frame_length, 4);
    o.push_back(0);
    o.push_back((uint8_t)c.bit_depth);
    o.push_back((uint8_t)c.pb);
    o.push_back((uint8_t)c.mb);
    o.push_back((uint8_t)c.kb);
    o.push_back((uint8_t)c.channels);
    be(o, (uint64_t)c.max_run, 2);
    be(o, 0, 4);
    be(o, 0, 4);
    be(o, c.sample_rate, 4);
    return o;
}

using Packets = std::vector<std::vector<uint8_t>>;

// CAF: desc, kuki, pakt, data; *cookie_at receives the cookie's offset in the file
std::vector<uint8_t> caf(const Cfg& c, const Packets& pk, size_t* cookie_at) {
    std::vector<uint8_t> o, desc, pakt, data;
    const double rate = (double)c.sample_rate;
    uint64_t rb;
    std::memcpy(&rb, &rate, 8);
    be(desc, rb, 8);
    tag(desc, "alac");
    for (uint32_t v : {0u, 0u, c.frame_length, (uint32_t)c.channels, 0u}) be(desc, v, 4);
    be(pakt, pk.size(), 8);
    be(pakt, 0, 8);
    be(pakt, 0, 8);
    for (const auto& p : pk) {
        uint8_t tmp[10];
        int k = 0;
        uint64_t v = p.size();
        tmp[k++] = (uint8_t)(v & 0x7F);
        for (v >>= 7; v; v >>= 7) tmp[k++] = (uint8_t)(0x80 | (v & 0x7F));
        while (k) pakt.push_back(tmp[--k]);
    }
    be(data, 0, 4);
    for (const auto& p : pk) cat(data, p);
    tag(o, "caff");
    be(o, 1, 2);
    be(o, 0, 2);
    const std::vector<uint8_t> kuki = cookie(c);
    const char* ids[4] = {"desc", "kuki", "pakt", "data"};
    const std::vector<uint8_t>* bodies[4] = {&desc, &kuki, &pakt, &data};
    for (int i = 0; i < 4; i++) {
        tag(o, ids[i]);
        be(o, bodies[i]->size(), 8);
        if (i == 1) *cookie_at = o.size();
        cat(o, *bodies[i]);
    }
    return o;
}

std::vector<uint8_t> box(const char* t, const std::vector<uint8_t>& body) {
    std::vector<uint8_t> o;
    be(o, 8 + body.size(), 4);
    tag(o, t);
    cat(o, body);
    return o;
}

// ISO MP4 with one audio track, one packet per chunk
std::vector<uint8_t> mp4(const Cfg& c, const Packets& pk, size_t* cookie_at) {
    std::vector<uint8_t> ftyp_b;
    tag(ftyp_b, "M4A ");
    be(ftyp_b, 0, 4);
    tag(ftyp_b, "M4A ");
    const std::vector<uint8_t> ftyp = box("ftyp", ftyp_b);
    auto moov_of = [&](uint64_t first_off, size_t* cookie_in_moov) {
        std::vector<uint8_t> entry(6, 0);
        be(entry, 1, 2);
        be(entry, 0, 8);
        be(entry, (uint64_t)c.channels, 2);
        be(entry, (uint64_t)c.bit_depth, 2);
        be(entry, 0, 4);
        be(entry, (uint64_t)(c.sample_rate & 0xFFFF) << 16, 4);
        std::vector<uint8_t> ab(4, 0);
        cat(ab, cookie(c));
        cat(entry, box("alac", ab));
        std::vector<uint8_t> stsd_b;
        be(stsd_b, 0, 4);
        be(stsd_b, 1, 4);
        cat(stsd_b, box("alac", entry));
        std::vector<uint8_t> stsz_b, stsc_b, stco_b;
        be(stsz_b, 0, 4);
        be(stsz_b, 0, 4);
        be(stsz_b, pk.size(), 4);
        for (const auto& p : pk) be(stsz_b, p.size(), 4);
        be(stsc_b, 0, 4);
        be(stsc_b, 1, 4);
        for (uint32_t v : {1u, 1u, 1u}) be(stsc_b, v, 4);
        be(stco_b, 0, 4);
        be(stco_b, pk.size(), 4);
        uint64_t off = first_off;
        for (const auto& p : pk) {
            be(stco_b, off, 4);
            off += p.size();
        }
        std::vector<uint8_t> stbl_b = box("stsd", stsd_b);
        cat(stbl_b, box("stsc", stsc_b));
        cat(stbl_b, box("stsz", stsz_b));
        cat(stbl_b, box("stco", stco_b));
        std::vector<uint8_t> minf_b = box("stbl", stbl_b);
        std::vector<uint8_t> hdlr_b(8, 0);
        tag(hdlr_b, "soun");
        hdlr_b.resize(hdlr_b.size() + 13, 0);
        std::vector<uint8_t> mdia_b = box("hdlr", hdlr_b);
        cat(mdia_b, box("minf", minf_b));
        const std::vector<uint8_t> moov = box("moov", box("trak", box("mdia", mdia_b)));
        // moov(8) trak(8) mdia(8) hdlr box, minf(8) stbl(8) stsd(8) + 8, entry box header (8) + 28, alac box header (8) + 4
        *cookie_in_moov = 8 + 8 + 8 + (8 + hdlr_b.size()) + 8 + 8 + 8 + 8 + 8 + 28 + 8 + 4;
        return moov;
    };
    size_t cim = 0;
    const size_t moov_len = moov_of(0, &cim).size();
    std::vector<uint8_t> o = ftyp;
    cat(o, moov_of(ftyp.size() + moov_len + 8, &cim));
    *cookie_at = ftyp.size() + cim;
    std::vector<uint8_t> mdat;
    for (const auto& p : pk) cat(mdat, p);
    cat(o, box("mdat", mdat));
    return o;
}

std::vector<int64_t> signal(Rng& r, int n, int bits, bool noise, bool silence) {
    std::vector<int64_t> v((size_t)n);
    const int64_t top = (1ll << (bits - 1)) - 1;
    int64_t x = 0;
    for (int i = 0; i < n; i++) {
        if (noise) {
            v[i] = (int64_t)(r.next() % (uint64_t)(2 * top + 2)) - top - 1;
        } else {
            x += (int64_t)(r.next() % 2001) - 1000 + ((i / 50) % 2 ? 300 : -300);
            if (x > top / 2) x = top / 2;
            if (x < -top / 2) x = -top / 2;
            v[i] = bits > 16 ? x * ((1ll << (bits - 16)) - 1) / 2 + (int64_t)(r.next() & 0xFF) : x;
        }
        if (silence && (i % 700) > 300) v[i] = 0;
    }
    return v;
}

struct Stream {
    std::string name;
    Cfg cfg;
    Packets pk;
};

Stream make(const std::string& name, Rng& r, int bits, int nch, uint32_t fl, int n, const std::vector<Spec>& specs, bool noise,
            bool silence, int kb = 14) {
    Stream s;
    s.name = name;
    s.cfg.frame_length = fl;
    s.cfg.bit_depth = bits;
    s.cfg.channels = nch;
    s.cfg.kb = kb;
    std::vector<std::vector<int64_t>> chans;
    for (int c = 0; c < nch; c++) chans.push_back(signal(r, n, bits, noise, silence));
    size_t k = 0;
    for (int o = 0; o < n; o += (int)fl, k++) {
        std::vector<std::vector<int64_t>> part;
        for (int c = 0; c < nch; c++)
            part.emplace_back(chans[c].begin() + o, chans[c].begin() + std::min<size_t>((size_t)n, (size_t)o + fl));
        s.pk.push_back(frame(s.cfg, part, specs[k % specs.size()]));
    }
    return s;
}

int failures = 0;
uint64_t compared = 0, planned_ok = 0, pcm_checked = 0;

// host decoder and plan + phased decode on the same bytes: the same status, text and samples
void check_alac(const std::string& what, const std::vector<uint8_t>& f) {
    std::vector<float> host;
    uint32_t sr = 0;
    char herr[256] = {0};
    const bool hok = sdsp_decode_audio_bytes(f, &host, &sr, herr, sizeof herr);
    const SdspFormat fm = sdsp_probe_format(f.data(), f.size());
    const bool caf_alac = fm == SdspFormat::CAF && sdsp_caf_is_alac(f.data(), f.size());
    if (!caf_alac && fm != SdspFormat::MP4) return;  // the batch decoder's host fallback
    sdsp_alac_plan pl;
    std::string why;
    const bool pok = caf_alac ? sdsp_alac_plan_caf(f.data(), f.size(), &pl, &why) : sdsp_alac_plan_mp4(f.data(), f.size(), &pl, &why);
    compared++;
    if (pok != hok || (!pok && why != herr)) {
        std::printf("FAIL %s: plan %d '%s' host %d '%s'\n", what.c_str(), (int)pok, why.c_str(), (int)hok, herr);
        failures++;
        return;
    }
    if (!pok) return;
    alac_phased::Result r;
    alac_phased::decode(f.data(), pl, &r);
    planned_ok++;
    const uint32_t psr = pl.cfg.sample_rate ? pl.cfg.sample_rate : 44100u;
    if (psr != sr || r.samples.size() != host.size() ||
        (!host.empty() && std::memcmp(r.samples.data(), host.data(), host.size() * sizeof(float)) != 0)) {
        std::printf("FAIL %s: samples differ (%zu vs %zu)\n", what.c_str(), r.samples.size(), host.size());
        failures++;
    }
}

void check_pcm(const std::string& what, const std::vector<uint8_t>& f) {
    std::vector<float> host;
    uint32_t sr = 0;
    char herr[256] = {0};
    const bool hok = sdsp_decode_audio_bytes(f, &host, &sr, herr, sizeof herr);
    const SdspFormat fm = sdsp_probe_format(f.data(), f.size());
    if (fm != SdspFormat::WAV && fm != SdspFormat::AIFF) return;
    sdsp_pcm_plan pl;
    std::string why;
    const int r = fm == SdspFormat::AIFF ? sdsp_pcm_plan_aiff(f.data(), f.size(), &pl, &why) : sdsp_pcm_plan_wav(f.data(), f.size(), &pl, &why);
    pcm_checked++;
    if (r == 0) return;
    if ((r == 1) != hok || (r < 0 && why != herr)) {
        std::printf("FAIL %s: plan %d '%s' host %d '%s'\n", what.c_str(), r, why.c_str(), (int)hok, herr);
        failures++;
        return;
    }
    if (r < 0) return;
    std::vector<float> got;
    sdsp_pcm_convert_plan(f.data(), pl, &got);
    if (pl.rate != sr || got.size() != host.size() || (!host.empty() && std::memcmp(got.data(), host.data(), host.size() * 4) != 0)) {
        std::printf("FAIL %s: samples differ\n", what.c_str());
        failures++;
    }
}

std::vector<uint8_t> wav(int tagv, int bits, int ch, const std::vector<uint8_t>& pay, bool odd_chunk) {
    std::vector<uint8_t> o;
    auto le = [&](uint64_t v, int n) {
        for (int i = 0; i < n; i++) o.push_back((uint8_t)(v >> (8 * i)));
    };
    tag(o, "RIFF");
    le(0, 4);
    tag(o, "WAVE");
    tag(o, "fmt ");
    le(16, 4);
    le((uint64_t)tagv, 2);
    le((uint64_t)ch, 2);
    le(44100, 4);
    le(0, 4);
    le((uint64_t)(ch * bits / 8), 2);
    le((uint64_t)bits, 2);
    if (odd_chunk) {
        tag(o, "LIST");
        le(3, 4);
        le(0, 4);
    }
    tag(o, "data");
    le(pay.size() + 77, 4);  // overstated: clipped to the file
    cat(o, pay);
    return o;
}

std::vector<uint8_t> aiff(int bits, int ch, const char* comp, int offset, const std::vector<uint8_t>& pay) {
    std::vector<uint8_t> o;
    tag(o, "FORM");
    be(o, 0, 4);
    tag(o, comp ? "AIFC" : "AIFF");
    tag(o, "COMM");
    be(o, comp ? 24 : 18, 4);
    be(o, (uint64_t)ch, 2);
    be(o, 0, 4);
    be(o, (uint64_t)bits, 2);
    be(o, 0x400E, 2);
    be(o, 0xAC44000000000000ull, 8);
    if (comp) {
        tag(o, comp);
        be(o, 0, 2);
    }
    tag(o, "SSND");
    be(o, 8 + (uint64_t)offset + pay.size(), 4);
    be(o, (uint64_t)offset, 4);
    be(o, 0, 4);
    for (int i = 0; i < offset; i++) o.push_back(0xEE);
    cat(o, pay);
    return o;
}

}  // namespace

int main() {
    Rng r{12345};
    ChSpec na0, na31, t4, t8, m15;
    na31.coefs.assign(31, 0);
    t4.coefs = {1024, -512, 256, -128};
    t8.coefs = {600, 300, -100, 50, 20, -10, 5, 2};
    m15.mode = 15, m15.den = 10, m15.pbf = 2;
    m15.coefs = {400, -200, 100, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7};
    auto mono = [](const ChSpec& c) {
        Spec s;
        s.ch[0] = c;
        return s;
    };
    auto stereo = [](const ChSpec& a, const ChSpec& b, int mb, int mr, int shift) {
        Spec s;
        s.ch[0] = a, s.ch[1] = b, s.mix_bits = mb, s.mix_res = mr, s.shift = shift;
        return s;
    };
    Spec esc;
    esc.escape = true;
    std::vector<Stream> streams;
    streams.push_back(make("mono16", r, 16, 1, 1024, 6 * 1024 + 333, {mono(na0), mono(na31), mono(t4), mono(t8), mono(m15), esc}, false, true));
    streams.push_back(make("stereo16_mix0", r, 16, 2, 1024, 3000, {stereo(t4, m15, 0, 0, 0), esc}, false, false));
    streams.push_back(make("stereo16_mix2_1", r, 16, 2, 1024, 3000, {stereo(t4, t8, 2, 1, 0), esc, stereo(na31, t4, 2, 1, 0)}, false, true));
    streams.push_back(make("stereo16_mix3_-2", r, 16, 2, 512, 1500, {stereo(t8, t4, 3, -2, 0)}, false, false));
    streams.push_back(make("mono20", r, 20, 1, 1024, 2500, {mono(t4), esc}, false, false));
    streams.push_back(make("stereo24_shift1", r, 24, 2, 1024, 2500, {stereo(t4, t4, 2, 1, 1), esc}, false, false));
    streams.push_back(make("stereo24_shift2", r, 24, 2, 256, 700, {stereo(t4, na31, 0, 0, 2)}, false, true));
    Spec m32 = mono(t4);
    m32.shift = 2;
    streams.push_back(make("mono32_shift2", r, 32, 1, 1024, 2500, {m32, esc}, false, false));
    streams.push_back(make("noise_kb10", r, 16, 1, 512, 2048, {mono(na0), mono(t4)}, true, false, 10));
    streams.push_back(make("fl16", r, 16, 1, 16, 100, {mono(t4), mono(t8)}, false, false));
    streams.push_back(make("last_1", r, 16, 1, 256, 257, {mono(t4)}, false, false));

    uint64_t variants = 0;
    for (const Stream& s : streams) {
        for (int container = 0; container < 2; container++) {
            size_t ck = 0;
            const std::vector<uint8_t> f = container ? mp4(s.cfg, s.pk, &ck) : caf(s.cfg, s.pk, &ck);
            {  // the clean stream decodes completely
                sdsp_alac_plan pl;
                std::string why;
                const bool ok = container ? sdsp_alac_plan_mp4(f.data(), f.size(), &pl, &why) : sdsp_alac_plan_caf(f.data(), f.size(), &pl, &why);
                alac_phased::Result res;
                if (ok) alac_phased::decode(f.data(), pl, &res);
                if (!ok || res.skipped || res.decoded != s.pk.size()) {
                    std::printf("FAIL %s/%d: clean stream: plan %d '%s', %llu skipped\n", s.name.c_str(), container, (int)ok,
                                why.c_str(), (unsigned long long)res.skipped);
                    failures++;
                }
            }
            check_alac(s.name, f);
            for (int v = 0; v < 160; v++, variants++) {
                Packets pk = s.pk;
                std::vector<uint8_t>& p = pk[r.next() % pk.size()];
                const uint32_t kind = r.next() % 8;
                if (kind == 0) {
                    p.resize(r.next() % (p.size() + 1));  // truncated (possibly empty)
                } else {
                    const int flips = 1 + (int)(r.next() % 3);
                    // early bytes hold the element and predictor headers: flip there half of the time
                    for (int q = 0; q < flips && !p.empty(); q++) {
                        const size_t at = (r.next() & 1) ? r.next() % std::min<size_t>(p.size(), 24) : r.next() % p.size();
                        p[at] ^= (uint8_t)(1u << (r.next() % 8));
                    }
                }
                size_t ck2 = 0;
                check_alac(s.name + " packet variant", container ? mp4(s.cfg, pk, &ck2) : caf(s.cfg, pk, &ck2));
            }
            for (int v = 0; v < 24; v++, variants++) {  // the magic cookie, one bit
                std::vector<uint8_t> g = f;
                g[ck + r.next() % 24] ^= (uint8_t)(1u << (r.next() % 8));
                check_alac(s.name + " cookie variant", g);
            }
            for (int v = 0; v < 16; v++, variants++) {  // the file, cut
                std::vector<uint8_t> g(f.begin(), f.begin() + r.next() % f.size());
                check_alac(s.name + " cut file", g);
            }
        }
    }

    // PCM: every layout, files cut at every byte of the headers and a few places in the data
    std::vector<uint8_t> pay(4 * 3 * 8 * 5 + 7);
    for (auto& b : pay) b = (uint8_t)r.next();
    std::vector<std::vector<uint8_t>> pcm;
    for (int bits : {8, 16, 24, 32})
        for (int ch : {1, 2, 3}) pcm.push_back(wav(1, bits, ch, pay, ch == 2));
    for (int bits : {32, 64}) pcm.push_back(wav(3, bits, 2, pay, bits == 64));
    pcm.push_back(wav(6, 8, 2, pay, false));
    pcm.push_back(wav(1, 12, 1, pay, false));
    for (int bits : {8, 16, 24, 32})
        for (int off : {0, 1, 2, 3}) pcm.push_back(aiff(bits, 1 + off % 2, nullptr, off, pay));
    pcm.push_back(aiff(16, 2, "sowt", 1, pay));
    pcm.push_back(aiff(32, 2, "fl32", 3, pay));
    pcm.push_back(aiff(64, 1, "fl64", 2, pay));
    pcm.push_back(aiff(8, 1, "alaw", 0, pay));
    pcm.push_back(aiff(16, 1, "ima4", 0, pay));
    for (const auto& f : pcm)
        for (size_t cut = 0; cut <= f.size(); cut += (cut < 96 || cut + 16 > f.size()) ? 1 : 37)
            check_pcm("pcm cut " + std::to_string(cut), std::vector<uint8_t>(f.begin(), f.begin() + cut));

    std::printf("streams %zu, variants %llu, compared %llu, planned and decoded %llu, pcm files %llu\n", streams.size() * 2,
                (unsigned long long)variants, (unsigned long long)compared, (unsigned long long)planned_ok,
                (unsigned long long)pcm_checked);
    if (failures) {
        std::printf("alac_core_check: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("alac_core_check: ok\n");
    return 0;
}
