// vorbis_phased.hpp — the device Vorbis decoder's phases on the CPU (host only), through
// vorbis_core.hpp as the kernels run it and with the kernels' buffer layouts:
//   packets  every kept packet's spectra (channels x n/2 f32) into its place in one spectrum buffer;
//   imdct    every (packet, channel): pre-twiddle, the radix-2 network stage by stage, the windowed
//            block of n f32 into its place in one block buffer (twice the spectrum's place);
//   ola      every output sample on its own: the packet pair by the planned offsets, prev + cur per
//            channel, the mono mix.
// Used by sdsp_debug_vorbis_decode_phased (k_vorbis.hip) and by the sanitizer check
// (tools/vorbis_core_check.cpp).
#pragma once

#include <vector>

#include "vorbis_host.hpp"

namespace vorbis_phased {

struct Result {
    std::vector<float> samples;
    uint64_t packets = 0, zeroed = 0;
};

// the packet that holds output sample j: the last one whose first output sample is <= j (packet 0
// of a file produces none; out[] ascends strictly from packet 1 on)
template <class P>
VORBIS_HD uint32_t find_packet(const P* pk, uint32_t first, uint32_t count, uint64_t j) {
    uint32_t lo = first + 1, hi = first + count;  // answer in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pk[mid].out <= j)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

inline void decode(const sdsp_vorbis_plan& pl, Result* r) {
    namespace vc = vorbis_core;
    const vc::Setup sv = pl.setup.view();
    const int C = sv.channels;
    const size_t np = pl.packets.size();
    std::vector<uint64_t> spec_off(np + 1, 0);
    for (size_t i = 0; i < np; i++) spec_off[i + 1] = spec_off[i] + (uint64_t)C * (pl.packets[i].n / 2);
    // packets
    std::vector<float> spectra(spec_off[np]);
    {
        std::vector<uint32_t> work(vc::work_words(C, sv.bs1 / 2));
        int32_t ybuf[vc::FLOOR_MAX_POINTS];
        for (size_t i = 0; i < np; i++) {
            const sdsp_vorbis_packet& p = pl.packets[i];
            int32_t zeroed = 0;
            vc::decode_packet(sv, pl.bytes.data() + p.off, p.size, vc::Work{work.data(), 1, work.size()}, vc::YStore{ybuf, 1},
                              spectra.data() + spec_off[i], &zeroed);
            r->zeroed += (uint64_t)zeroed;
        }
    }
    // imdct
    std::vector<float> blocks(2 * spec_off[np]);
    {
        std::vector<vc::cd> a((size_t)sv.bs1 / 4);
        const vc::BlockTables ts = sdsp_vorbis_block_tables(sv.bs0).view();
        for (size_t i = 0; i < np; i++) {
            const sdsp_vorbis_packet& p = pl.packets[i];
            const int n = p.n, M = n / 2, H = n / 4;
            int lgH = 0;
            while ((1 << lgH) < H) lgH++;
            const vc::BlockTables tb = sdsp_vorbis_block_tables(n).view();
            for (int c = 0; c < C; c++) {
                const float* X = spectra.data() + spec_off[i] + (size_t)c * (size_t)M;
                for (int k = H; k-- > 0;) vc::imdct_pre(X, M, lgH, k, tb.pre, a.data());
                for (int len = 2; len <= H; len <<= 1)
                    for (int t = H / 2; t-- > 0;) vc::fft_butterfly(a.data(), H, len, t, tb.tw);  // any order within a stage
                float* y = blocks.data() + 2 * spec_off[i] + (size_t)c * (size_t)n;
                for (int q = 0; q < n; q++)
                    y[q] = vc::imdct_out(a.data(), M, q, tb.post) * vc::window_at(n, sv.bs0, p.blockflag, p.prev_long, p.next_long, q, tb, ts);
            }
        }
    }
    // ola
    r->samples.assign(pl.frames, 0.0f);
    for (uint64_t j = 0; j < pl.frames; j++) {
        const uint32_t q = find_packet(pl.packets.data(), 0u, (uint32_t)np, j);
        const sdsp_vorbis_packet& p = pl.packets[q];
        r->samples[j] = vc::ola_mix(blocks.data() + 2 * spec_off[q - 1], p.prev_n, blocks.data() + 2 * spec_off[q], p.n, C, (int)(j - p.out));
    }
    r->packets = np;
}

}  // namespace vorbis_phased
