// alac_phased.hpp — the device ALAC decoder's phases on the CPU (host only), through alac_core.hpp
// as the kernels run it: every packet of the plan into its own slot with its sample count, the walk
// of the counts into offsets, the gather.  Used by sdsp_debug_alac_decode_phased (k_alac.hip) and by
// the sanitizer check (tools/alac_core_check.cpp).
#pragma once

#include <cstring>
#include <vector>

#include "lossless_host.hpp"

namespace alac_phased {

struct Result {
    std::vector<float> samples;
    uint64_t packets = 0, decoded = 0, skipped = 0;
};

// data is the whole file, plan its cookie and packet table (every packet inside the file)
inline void decode(const uint8_t* data, const sdsp_alac_plan& pl, Result* r) {
    namespace ac = alac_core;
    // frames: every packet into its own slot
    const size_t np = pl.packets.size();
    std::vector<std::vector<float>> slots(np);
    std::vector<float> slot;
    std::vector<uint32_t> cnt(np, 0);
    std::vector<int32_t> work;
    for (size_t i = 0; i < np; i++) {
        uint32_t got = 0;
        if (sdsp_alac_decode_packet(pl.cfg, data + pl.packets[i].first, (size_t)pl.packets[i].second, &work, &slot, &got, nullptr)) {
            slots[i].assign(slot.begin(), slot.begin() + got);
            cnt[i] = got;
        }
    }
    // offsets and gather
    std::vector<uint64_t> out_off(np, 0);
    uint32_t dec = 0, skp = 0;
    const uint64_t total = ac::layout_file(cnt.data(), np, out_off.data(), &dec, &skp);
    r->samples.assign(total, 0.0f);
    for (size_t i = 0; i < np; i++)
        if (out_off[i] != ~0ull && cnt[i]) std::memcpy(r->samples.data() + out_off[i], slots[i].data(), (size_t)cnt[i] * sizeof(float));
    r->packets = np;
    r->decoded = dec;
    r->skipped = skp;
}

}  // namespace alac_phased
