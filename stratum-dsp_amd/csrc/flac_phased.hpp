// flac_phased.hpp — the device FLAC decoder's four phases on the CPU (host only), through
// flac_core.hpp as the kernels run it: scan every offset, decode every candidate into its own
// scratch slot, chain, gather.  Used by sdsp_debug_flac_decode_phased (k_flac.hip) and by the
// sanitizer check (tools/flac_core_check.cpp).
#pragma once

#include <cstring>
#include <vector>

#include "flac_core.hpp"

namespace flac_phased {

// candidate word: (bs - 1) | bps << 16 | channel code << 22 | header bytes << 26
inline uint32_t pack(uint32_t bs, int bps, int chc, size_t hl) {
    return (bs - 1) | ((uint32_t)bps << 16) | ((uint32_t)chc << 22) | ((uint32_t)hl << 26);
}

struct Result {
    std::vector<float> samples;
    uint64_t candidates = 0, accepted = 0, rejected = 0;
};

// data[0 .. n) is the whole file, `start` the first byte of its frame region (sdsp_flac_parse_stream)
inline void decode(const uint8_t* data, size_t n, size_t start, int si_bps, Result* r) {
    namespace fc = flac_core;
    // scan: every offset
    std::vector<uint32_t> off, bs, end, pk;
    for (size_t o = start; o < n && o < (1ull << 32); o++) {
        uint32_t b = 0;
        int bps = 0, chc = 0;
        const size_t hl = fc::frame_header(data + o, n - o, si_bps, &b, &bps, &chc);
        if (!hl) continue;
        off.push_back((uint32_t)o);
        bs.push_back(b);
        pk.push_back(pack(b, bps, chc, hl));
    }
    // frames: every candidate into its own scratch slot
    const size_t nc = off.size();
    std::vector<uint64_t> slot(nc + 1, 0), out_off(nc, 0);
    for (size_t i = 0; i < nc; i++) slot[i + 1] = slot[i] + bs[i];
    std::vector<float> scratch(slot[nc]);
    std::vector<uint8_t> ok(nc, 0);
    end.assign(nc, 0);
    std::vector<int64_t> work;
    for (size_t i = 0; i < nc; i++) {
        const int bps = (int)((pk[i] >> 16) & 63u), chc = (int)((pk[i] >> 22) & 15u);
        work.resize((size_t)fc::channels_of(chc) * bs[i]);
        const fc::Work w{work.data(), 1, work.size()};
        size_t e = 0;
        if (fc::decode_frame(data, n, off[i], pk[i] >> 26, bs[i], bps, chc, w, &e)) {
            fc::emit_mono(w, bs[i], bps, chc, scratch.data() + slot[i], 1);
            ok[i] = 1;
            end[i] = (uint32_t)e;
        }
    }
    // chain and gather
    const fc::ChainCounts c = fc::chain_file(off.data(), ok.data(), end.data(), bs.data(), nc, start, out_off.data());
    r->samples.assign(c.samples, 0.0f);
    for (size_t i = 0; i < nc; i++)
        if (out_off[i] != ~0ull) std::memcpy(r->samples.data() + out_off[i], scratch.data() + slot[i], (size_t)bs[i] * sizeof(float));
    r->candidates = nc;
    r->accepted = c.accepted;
    r->rejected = c.rejected;
}

}  // namespace flac_phased
