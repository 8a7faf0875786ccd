// vorbis_core_check — the shared Vorbis packet-level code (stratum-dsp_amd/csrc/vorbis_core.hpp) and
// the CPU phased decode (vorbis_phased.hpp) under the host sanitizers, CPU only.  The device kernels
// run this same code with the same buffer layouts, so a read or write out of range, or undefined
// arithmetic, here is one there.
//
// Takes a directory of Ogg Vorbis streams (tests/vorbis_streams.py writes its matrix, its
// packet-flipped variants and the audio encoder's streams there) and pushes every stream, and per
// stream a few hundred variants (the file truncated; a bit flipped anywhere, which the page CRC
// catches; a bit flipped inside a page's payload with the CRC recomputed, which reaches the header
// parse and the packet decoder; a page's payload cut short with the lacing and CRC rewritten),
// through the host decoder (sdsp_decode_audio_bytes) and through the plan and the CPU phased decode
// (vorbis_phased::decode), and requires the same status, text and bit-identical samples (two NaNs, which only a damaged
// VQ scale produces, count as equal: their sign and payload follow the compiler's operand order).  Ends with
// "vorbis_core_check: ok" and the counts, status 0; any sanitizer report or mismatch is a failure.
//
// Build and run (from the repository root):
//   python tests/vorbis_streams.py /tmp/vorbis_streams && g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ tools/vorbis_core_check.cpp stratum-dsp_amd/csrc/host_*.hip -o tools/vorbis_core_check -pthread && tools/vorbis_core_check /tmp/vorbis_streams
#include <dirent.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../stratum-dsp_amd/csrc/flac_host.hpp"
#include "../stratum-dsp_amd/csrc/lossless_host.hpp"
#include "../stratum-dsp_amd/csrc/vorbis_phased.hpp"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
};

uint32_t ogg_crc(const uint8_t* p, size_t n) {
    uint32_t crc = 0;
    for (size_t i = 0; i < n; i++) {
        crc ^= (uint32_t)((i >= 22 && i < 26) ? 0 : p[i]) << 24;
        for (int k = 0; k < 8; k++) crc = (crc & 0x80000000u) ? (crc << 1) ^ 0x04C11DB7u : crc << 1;
    }
    return crc;
}

struct Page {
    size_t pos, header, body;  // first byte, header bytes (27 + segments), payload bytes
};

std::vector<Page> pages(const std::vector<uint8_t>& f) {
    std::vector<Page> out;
    size_t pos = 0;
    while (pos + 27 <= f.size() && std::memcmp(f.data() + pos, "OggS", 4) == 0) {
        const size_t nseg = f[pos + 26];
        if (pos + 27 + nseg > f.size()) break;
        size_t body = 0;
        for (size_t i = 0; i < nseg; i++) body += f[pos + 27 + i];
        if (pos + 27 + nseg + body > f.size()) break;
        out.push_back(Page{pos, 27 + nseg, body});
        pos += 27 + nseg + body;
    }
    return out;
}

void set_crc(std::vector<uint8_t>& f, size_t pos, size_t len) {
    const uint32_t c = ogg_crc(f.data() + pos, len);
    for (int i = 0; i < 4; i++) f[pos + 22 + i] = (uint8_t)(c >> (8 * i));
}

uint64_t n_checked = 0, n_decoded = 0, n_errors = 0, n_not_vorbis = 0, n_zeroed = 0, n_nan = 0;

// host decoder against plan + phased decode; exits on the first mismatch
void check(const std::vector<uint8_t>& f, const std::string& what) {
    std::vector<float> host;
    uint32_t hsr = 0;
    char herr[256] = {0};
    const bool hok = sdsp_decode_audio_bytes(f, &host, &hsr, herr, sizeof herr);
    n_checked++;
    sdsp_vorbis_plan pl;
    std::string why;
    const int r = sdsp_probe_format(f.data(), f.size()) == SdspFormat::OGG ? sdsp_vorbis_plan_ogg(f.data(), f.size(), &pl, &why) : 0;
    if (r == 0) {  // the first page was lost or is no Vorbis header any more: the host decoder's file
        n_not_vorbis++;
        return;
    }
    if (r < 0) {
        if (hok || why != herr) {
            std::fprintf(stderr, "%s: plan refuses with '%s', host %s '%s'\n", what.c_str(), why.c_str(), hok ? "decodes" : "says", herr);
            std::exit(1);
        }
        n_errors++;
        return;
    }
    vorbis_phased::Result res;
    vorbis_phased::decode(pl, &res);
    bool same = hok && hsr == pl.setup.rate && host.size() == res.samples.size();
    bool nan = false;
    for (size_t i = 0; same && i < host.size(); i++) {
        uint32_t x, y;
        std::memcpy(&x, &host[i], 4);
        std::memcpy(&y, &res.samples[i], 4);
        // A flipped VQ scale can reach infinity, and inf - inf is a NaN whose sign and payload depend on
        // the operand order the compiler chose at each call site: two NaNs count as equal, all else by bits
        const bool xn = (x & 0x7fffffffu) > 0x7f800000u, yn = (y & 0x7fffffffu) > 0x7f800000u;
        nan = nan || (xn && yn);
        same = (xn && yn) || x == y;
    }
    n_nan += nan;
    if (!same) {
        std::fprintf(stderr, "%s: phased decode differs from the host decoder (host %s '%s', %zu / %zu samples)\n", what.c_str(),
                     hok ? "ok" : "failed", herr, host.size(), res.samples.size());
        if (FILE* fp = std::fopen("vorbis_core_check_mismatch.ogg", "wb")) {  // the stream, for a closer look
            std::fwrite(f.data(), 1, f.size(), fp);
            std::fclose(fp);
        }
        std::exit(1);
    }
    n_decoded++;
    n_zeroed += res.zeroed;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: vorbis_core_check <directory of .ogg streams> [variants per kind, default 60]\n");
        return 2;
    }
    const int per_kind = argc > 2 ? std::atoi(argv[2]) : 60;
    std::vector<std::string> names;
    if (DIR* d = opendir(argv[1])) {
        while (dirent* e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() > 4 && n.substr(n.size() - 4) == ".ogg") names.push_back(n);
        }
        closedir(d);
    }
    std::sort(names.begin(), names.end());
    if (names.empty()) {
        std::fprintf(stderr, "no .ogg files in %s\n", argv[1]);
        return 2;
    }
    Rng rng{12345};
    for (const std::string& name : names) {
        std::vector<uint8_t> f;
        {
            FILE* fp = std::fopen((std::string(argv[1]) + "/" + name).c_str(), "rb");
            if (!fp) return 2;
            uint8_t buf[65536];
            size_t got;
            while ((got = std::fread(buf, 1, sizeof buf, fp)) > 0) f.insert(f.end(), buf, buf + got);
            std::fclose(fp);
        }
        check(f, name);
        const std::vector<Page> pg = pages(f);
        for (int v = 0; v < per_kind; v++) {  // the file truncated
            std::vector<uint8_t> g(f.begin(), f.begin() + rng.next() % f.size());
            check(g, name + " truncated");
        }
        for (int v = 0; v < per_kind; v++) {  // a bit flipped anywhere: the page fails its CRC
            std::vector<uint8_t> g = f;
            g[rng.next() % g.size()] ^= (uint8_t)(1u << (rng.next() % 8));
            check(g, name + " bit flip");
        }
        for (int v = 0; v < 3 * per_kind && !pg.empty(); v++) {  // one to three bits flipped in a payload, CRC made valid again
            std::vector<uint8_t> g = f;
            const Page& p = pg[v < per_kind ? 2 % pg.size() : rng.next() % pg.size()];  // a third of them in the setup header
            if (!p.body) continue;
            for (uint32_t q = 0, nq = 1 + rng.next() % 3; q < nq; q++)
                g[p.pos + p.header + rng.next() % p.body] ^= (uint8_t)(1u << (rng.next() % 8));
            set_crc(g, p.pos, p.header + p.body);
            check(g, name + " payload flip");
        }
        for (int v = 0; v < per_kind && pg.size() > 3; v++) {  // an audio page's last packet cut short
            const Page& p = pg[3 + rng.next() % (pg.size() - 3)];
            const size_t nseg = p.header - 27;
            if (!nseg || !f[p.pos + 27 + nseg - 1]) continue;
            const uint8_t last = f[p.pos + 27 + nseg - 1];
            const uint8_t keep = (uint8_t)(rng.next() % last);
            std::vector<uint8_t> g(f.begin(), f.begin() + p.pos + p.header + p.body - (last - keep));
            g[p.pos + 27 + nseg - 1] = keep;
            set_crc(g, p.pos, p.header + p.body - (last - keep));
            g.insert(g.end(), f.begin() + p.pos + p.header + p.body, f.end());
            check(g, name + " packet cut");
        }
    }
    std::printf("vorbis_core_check: ok (%zu streams, %llu decodes compared: %llu equal samples, %llu equal errors, %llu not Vorbis; "
                "%llu silenced packets, %llu decodes with NaNs)\n",
                names.size(), (unsigned long long)n_checked, (unsigned long long)n_decoded, (unsigned long long)n_errors,
                (unsigned long long)n_not_vorbis, (unsigned long long)n_zeroed, (unsigned long long)n_nan);
    return 0;
}
