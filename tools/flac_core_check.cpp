// flac_core_check — the shared FLAC frame-level code (stratum-dsp_amd/csrc/flac_core.hpp) under the
// host sanitizers, CPU only.  The device kernels run this same code, so a read or write out of range
// here is one there.
//
// Writes a set of FLAC streams with a small encoder of its own (CONSTANT, VERBATIM, FIXED 0-4 and
// LPC subframes, both Rice methods, partition orders, escaped partitions, mono / mid-side stereo /
// 3 channels, 8 / 16 / 24 / 32 bits, 8- and 16-bit block-size codes, a planted false header), then
// pushes every stream and a few thousand truncated and bit-flipped variants through the host decoder
// (sdsp_decode_flac) and through the four phases (flac_phased::decode: scan every offset, decode
// every candidate, chain, gather) and requires bit-identical samples.  Also checks the byte-wise
// CRC-16 against the bit-at-a-time form for every (state, byte).  Ends with "flac_core_check: ok"
// and status 0; any sanitizer report or mismatch is a failure.
//
// Build and run (from the repository root):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ tools/flac_core_check.cpp stratum-dsp_amd/csrc/host_flac.hip -o tools/flac_core_check && tools/flac_core_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../stratum-dsp_amd/csrc/flac_core.hpp"
#include "../stratum-dsp_amd/csrc/flac_host.hpp"
#include "../stratum-dsp_amd/csrc/flac_phased.hpp"

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
        acc = (acc << k) | (v & ((k == 64 ? 0 : (1ull << k)) - 1));
        n += k;
        while (n >= 8) {
            n -= 8;
            out.push_back((uint8_t)(acc >> n));
        }
        acc &= (1ull << n) - 1;
    }
    void unary(uint32_t q) {
        for (; q >= 16; q -= 16) put(0, 16);
        put(1, (int)q + 1);
    }
    void align() {
        if (n) put(0, 8 - n);
    }
};

uint8_t crc8_bits(const uint8_t* d, size_t n) {
    uint8_t c = 0;
    for (size_t i = 0; i < n; i++) {
        c ^= d[i];
        for (int b = 0; b < 8; b++) c = (uint8_t)((c & 0x80) ? (c << 1) ^ 0x07 : c << 1);
    }
    return c;
}
uint16_t crc16_bits(uint16_t c, const uint8_t* d, size_t n) {
    for (size_t i = 0; i < n; i++) {
        c ^= (uint16_t)(d[i] << 8);
        for (int b = 0; b < 8; b++) c = (uint16_t)((c & 0x8000) ? (c << 1) ^ 0x8005 : c << 1);
    }
    return c;
}

struct Spec {
    int type = 2;  // 0 constant, 1 verbatim, 2 fixed, 3 lpc
    int order = 2, method = 0, porder = 0, escape = -1, shift = 0, prec = 0;
    std::vector<int> coefs;
};

void write_residual(BitWriter& w, const std::vector<int64_t>& res, int order, uint32_t bs, const Spec& sp) {
    w.put((uint64_t)sp.method, 2);
    w.put((uint64_t)sp.porder, 4);
    const int pbits = sp.method == 0 ? 4 : 5;
    size_t i = 0;
    for (uint32_t p = 0; p < (1u << sp.porder); p++) {
        const uint32_t cnt = (bs >> sp.porder) - (p == 0 ? (uint32_t)order : 0u);
        if ((int)p == sp.escape) {
            w.put((1u << pbits) - 1, pbits);
            w.put(31, 5);
            for (uint32_t j = 0; j < cnt; j++) w.put((uint64_t)res[i++], 31);
            continue;
        }
        uint64_t sum = 0;
        for (uint32_t j = 0; j < cnt; j++) sum += (uint64_t)(res[i + j] >= 0 ? 2 * res[i + j] : -2 * res[i + j] - 1);
        int k = 0;
        while (cnt && (sum / cnt) >> (k + 1) && k < 14) k++;
        w.put((uint64_t)k, pbits);
        for (uint32_t j = 0; j < cnt; j++, i++) {
            const uint64_t u = (uint64_t)(res[i] >= 0 ? 2 * res[i] : -2 * res[i] - 1);
            w.unary((uint32_t)(u >> k));
            w.put(u & ((1ull << k) - 1), k);
        }
    }
}

void write_subframe(BitWriter& w, const std::vector<int64_t>& s, int bps, const Spec& sp) {
    const uint32_t bs = (uint32_t)s.size();
    auto putw = [&](int64_t v) {  // bps bits, up to 33
        if (bps > 32) w.put((uint64_t)(v >> 32), bps - 32);
        w.put((uint64_t)v & 0xFFFFFFFFull, bps > 32 ? 32 : bps);
    };
    w.put(0, 1);
    const int code = sp.type == 0 ? 0 : sp.type == 1 ? 1 : sp.type == 2 ? 8 + sp.order : 31 + (int)sp.coefs.size();
    w.put((uint64_t)code, 6);
    w.put(0, 1);
    if (sp.type == 0) {
        putw(s[0]);
    } else if (sp.type == 1) {
        for (int64_t v : s) putw(v);
    } else {
        const int order = sp.type == 2 ? sp.order : (int)sp.coefs.size();
        for (int i = 0; i < order; i++) putw(s[(size_t)i]);
        if (sp.type == 3) {
            w.put((uint64_t)(sp.prec - 1), 4);
            w.put((uint64_t)sp.shift, 5);
            for (int c : sp.coefs) w.put((uint64_t)(int64_t)c, sp.prec);
        }
        std::vector<int64_t> res;
        for (size_t i = (size_t)order; i < bs; i++) {
            int64_t p = 0;
            if (sp.type == 2) {
                static const int F[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
                for (int j = 0; j < order; j++) p += F[order][j] * s[i - 1 - (size_t)j];
            } else {
                for (int j = 0; j < order; j++) p += (int64_t)sp.coefs[(size_t)j] * s[i - 1 - (size_t)j];
                p >>= sp.shift;
            }
            res.push_back(s[i] - p);
        }
        write_residual(w, res, order, bs, sp);
    }
}

// chans: the original channels; mid_side only for two
std::vector<uint8_t> frame(const std::vector<std::vector<int64_t>>& chans, int bps, uint32_t number, bool mid_side,
                           const std::vector<Spec>& specs, int bs_code_bits) {
    const uint32_t bs = (uint32_t)chans[0].size();
    std::vector<std::vector<int64_t>> coded = chans;
    std::vector<int> cb(chans.size(), bps);
    int chc = (int)chans.size() - 1;
    if (mid_side) {
        for (uint32_t i = 0; i < bs; i++) {
            coded[0][i] = (chans[0][i] + chans[1][i]) >> 1;
            coded[1][i] = chans[0][i] - chans[1][i];
        }
        cb[1] = bps + 1;
        chc = 10;
    }
    BitWriter h;
    h.put(0x3FFE, 14);
    h.put(0, 2);
    int bsc = bs_code_bits == 8 ? 6 : bs_code_bits == 16 ? 7 : 0;
    if (!bsc) {
        static const uint32_t T[16] = {0, 192, 576, 1152, 2304, 4608, 0, 0, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768};
        for (int i = 1; i < 16; i++)
            if (T[i] == bs) bsc = i;
        if (!bsc) bsc = bs <= 256 ? 6 : 7;
    }
    h.put((uint64_t)bsc, 4);
    h.put(0, 4);  // the stream's rate
    h.put((uint64_t)chc, 4);
    h.put((uint64_t)(bps == 8 ? 1 : bps == 16 ? 4 : bps == 24 ? 6 : bps == 32 ? 7 : 0), 3);
    h.put(0, 1);
    if (number < 0x80) {
        h.put(number, 8);
    } else {  // two bytes, up to 0x7FF
        h.put(0xC0 | (number >> 6), 8);
        h.put(0x80 | (number & 0x3F), 8);
    }
    if (bsc == 6) h.put(bs - 1, 8);
    if (bsc == 7) h.put(bs - 1, 16);
    std::vector<uint8_t> out = h.out;
    out.push_back(crc8_bits(out.data(), out.size()));
    BitWriter w;
    for (size_t c = 0; c < coded.size(); c++) write_subframe(w, coded[c], cb[c], specs[c % specs.size()]);
    w.align();
    out.insert(out.end(), w.out.begin(), w.out.end());
    const uint16_t crc = crc16_bits(0, out.data(), out.size());
    out.push_back((uint8_t)(crc >> 8));
    out.push_back((uint8_t)crc);
    return out;
}

std::vector<uint8_t> stream(const std::vector<std::vector<uint8_t>>& frames, int nch, int bps) {
    BitWriter si;
    si.put(16, 16);
    si.put(65535, 16);
    si.put(0, 24);
    si.put(0, 24);
    si.put(44100, 20);
    si.put((uint64_t)(nch - 1), 3);
    si.put((uint64_t)(bps - 1), 5);
    si.put(0, 4);
    si.put(0, 32);
    for (int i = 0; i < 4; i++) si.put(0, 32);
    std::vector<uint8_t> out = {'f', 'L', 'a', 'C', 0x80, 0, 0, 34};
    out.insert(out.end(), si.out.begin(), si.out.end());
    for (const auto& f : frames) out.insert(out.end(), f.begin(), f.end());
    return out;
}

std::vector<int64_t> signal(Rng& r, uint32_t n, int bps, int kind) {
    std::vector<int64_t> s(n);
    const int64_t amp = (1ll << (bps - 1)) - 1;
    int64_t v = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (kind == 0) {  // a slow random walk: small residuals
            v += (int64_t)(r.next() % 65) - 32;
            v = v > amp / 2 ? amp / 2 : v < -amp / 2 ? -amp / 2 : v;
            s[i] = v;
        } else {  // full-scale noise
            s[i] = (int64_t)(((uint64_t)r.next() << 1 | (r.next() & 1)) % (2 * (uint64_t)amp + 1)) - amp;
        }
    }
    return s;
}

int failures = 0;

void compare(const std::vector<uint8_t>& f, const char* what, size_t variant) {
    std::vector<float> host;
    uint32_t sr = 0;
    std::string err;
    const bool ok = sdsp_decode_flac(f, &host, &sr, &err);
    sdsp_flac_stream si;
    size_t start = 0;
    std::string err2;
    const bool ok2 = sdsp_flac_parse_stream(f.data(), f.size(), &si, &start, &err2);
    if (ok != ok2 || (!ok && err != err2)) {
        std::printf("MISMATCH %s #%zu: stream parse\n", what, variant);
        failures++;
        return;
    }
    if (!ok) return;
    // the phases read the exact-size copy: a read past the end is a sanitizer report
    std::vector<uint8_t> copy(f);
    flac_phased::Result r;
    flac_phased::decode(copy.data(), copy.size(), start, si.bps, &r);
    if (r.samples.size() != host.size() ||
        (!host.empty() && std::memcmp(r.samples.data(), host.data(), host.size() * sizeof(float)) != 0)) {
        std::printf("MISMATCH %s #%zu: %zu samples phased, %zu host\n", what, variant, r.samples.size(), host.size());
        failures++;
    }
}

}  // namespace

int main() {
    // the byte-wise CRC-16 of flac_core against the bit-at-a-time form, every (state, byte)
    for (uint32_t c = 0; c < 65536; c++)
        for (uint32_t b = 0; b < 256; b++) {
            const uint8_t byte = (uint8_t)b;
            const uint32_t t = ((c >> 8) ^ b) & 0xFFu;
            const uint32_t fold = ((c << 8) ^ ((__builtin_popcount(t) & 1) ? 0x8003u : 0u) ^ (t << 2) ^ (t << 1)) & 0xFFFFu;
            if (fold != crc16_bits((uint16_t)c, &byte, 1)) {
                std::printf("crc16 fold differs at state %u byte %u\n", c, b);
                return 1;
            }
        }
    {
        Rng r{7};
        std::vector<uint8_t> d(4099);
        for (auto& x : d) x = (uint8_t)r.next();
        if (flac_core::crc16(d.data(), d.size()) != crc16_bits(0, d.data(), d.size()) ||
            flac_core::crc8(d.data(), 17) != crc8_bits(d.data(), 17)) {
            std::printf("crc differs\n");
            return 1;
        }
    }

    Rng rng{12345};
    std::vector<std::pair<std::string, std::vector<uint8_t>>> streams;
    auto fixed = [](int order, int method, int porder, int escape = -1) {
        Spec s;
        s.type = 2, s.order = order, s.method = method, s.porder = porder, s.escape = escape;
        return s;
    };
    for (int order = 0; order <= 4; order++)
        for (int method = 0; method < 2; method++) {
            std::vector<std::vector<uint8_t>> fr;
            for (uint32_t k = 0; k < 3; k++)
                fr.push_back(frame({signal(rng, 256, 16, 0)}, 16, k, false, {fixed(order, method, (int)k * 2)}, 0));
            streams.push_back({"fixed", stream(fr, 1, 16)});
        }
    for (int order : {1, 2, 8, 12, 32}) {
        Spec s;
        s.type = 3, s.prec = 12, s.shift = 9, s.method = 1, s.porder = 1;
        for (int j = 0; j < order; j++) s.coefs.push_back((int)(rng.next() % 200) - 100);
        s.coefs[0] = 500;
        streams.push_back({"lpc", stream({frame({signal(rng, 192, 24, 0)}, 24, 0, false, {s}, 0)}, 1, 24)});
    }
    {
        Spec c, v;
        c.type = 0, v.type = 1;
        streams.push_back({"constant_verbatim_escape",
                           stream({frame({std::vector<int64_t>(192, -1234)}, 16, 0, false, {c}, 0),
                                   frame({signal(rng, 192, 16, 1)}, 16, 1, false, {v}, 0),
                                   frame({signal(rng, 256, 16, 0)}, 16, 2, false, {fixed(2, 0, 2, 1)}, 0)},
                                  1, 16)});
        streams.push_back({"stereo_mid_side", stream({frame({signal(rng, 256, 16, 1), signal(rng, 256, 16, 1)}, 16, 0, true,
                                                            {fixed(2, 0, 1), fixed(1, 1, 0)}, 0),
                                                      frame({signal(rng, 256, 16, 0), signal(rng, 256, 16, 0)}, 16, 1, true,
                                                            {fixed(3, 0, 0)}, 0)},
                                                     2, 16)});
        streams.push_back({"three_channels_8bit", stream({frame({signal(rng, 192, 8, 1), signal(rng, 192, 8, 0),
                                                                 signal(rng, 192, 8, 1)}, 8, 0, false, {fixed(1, 0, 0), v}, 0)},
                                                         3, 8)});
        streams.push_back({"bits32", stream({frame({signal(rng, 192, 32, 1)}, 32, 0, false, {v}, 0),
                                             frame({signal(rng, 192, 32, 0)}, 32, 1, false, {fixed(1, 1, 0)}, 0)}, 1, 32)});
        streams.push_back({"block_size_codes", stream({frame({signal(rng, 1, 16, 1)}, 16, 0, false, {v}, 8),
                                                       frame({signal(rng, 17, 16, 0)}, 16, 1, false, {fixed(1, 0, 0)}, 8),
                                                       frame({signal(rng, 16, 16, 0)}, 16, 2, false, {fixed(4, 0, 2)}, 8),
                                                       frame({signal(rng, 4, 16, 0)}, 16, 3, false, {fixed(4, 0, 0)}, 8),
                                                       frame({signal(rng, 300, 16, 0)}, 16, 200, false, {fixed(2, 0, 0)}, 16)},
                                                      1, 16)});
        // a false header (sync, block size 4096, mono 16-bit, number 0, CRC-8) in a VERBATIM payload
        std::vector<int64_t> p = signal(rng, 192, 16, 1);
        uint8_t fh[6] = {0xFF, 0xF8, 0xC9, 0x08, 0x00, 0};
        fh[5] = crc8_bits(fh, 5);
        for (int i = 0; i < 3; i++) p[(size_t)(60 + i)] = (int16_t)((fh[2 * i] << 8) | fh[2 * i + 1]);
        streams.push_back({"false_header", stream({frame({signal(rng, 192, 16, 1)}, 16, 0, false, {v}, 0),
                                                   frame({p}, 16, 1, false, {v}, 0),
                                                   frame({signal(rng, 192, 16, 1)}, 16, 2, false, {v}, 0)}, 1, 16)});
    }

    size_t variants = 0;
    for (const auto& [name, f] : streams) {
        {  // the stream itself must decode to something: the encoder above and the decoders agree
            std::vector<float> host;
            uint32_t sr = 0;
            std::string err;
            if (!sdsp_decode_flac(f, &host, &sr, &err) || host.empty()) {
                std::printf("%s: the undamaged stream does not decode\n", name.c_str());
                return 1;
            }
        }
        compare(f, name.c_str(), 0);
        for (int k = 0; k < 60; k++) {  // truncations
            std::vector<uint8_t> g(f.begin(), f.begin() + (long)(rng.next() % f.size()));
            compare(g, name.c_str(), ++variants);
        }
        for (int k = 0; k < 120; k++) {  // one to three flipped bits
            std::vector<uint8_t> g(f);
            for (uint32_t j = 0, nf = 1 + rng.next() % 3; j < nf; j++) g[rng.next() % g.size()] ^= (uint8_t)(1u << (rng.next() % 8));
            compare(g, name.c_str(), ++variants);
        }
        for (int k = 0; k < 20; k++) {  // a flipped bit and a truncation
            std::vector<uint8_t> g(f.begin(), f.begin() + (long)(f.size() / 2 + rng.next() % (f.size() / 2)));
            g[rng.next() % g.size()] ^= (uint8_t)(1u << (rng.next() % 8));
            compare(g, name.c_str(), ++variants);
        }
    }
    if (failures) {
        std::printf("flac_core_check: %d mismatches\n", failures);
        return 1;
    }
    std::printf("flac_core_check: ok (%zu streams, %zu damaged variants)\n", streams.size(), variants);
    return 0;
}
