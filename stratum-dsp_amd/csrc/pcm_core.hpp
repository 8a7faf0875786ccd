// pcm_core.hpp — the examples' conversion of linear PCM to mono f32, shared by the host decoders
// (RIFF/WAVE in host_decode.hip, AIFF / AIFF-C and CAF lpcm in host_formats.hip), the CPU planned
// conversion (sdsp_debug_pcm_decode_planned) and the device kernel (k_pcm.hip).
//
// `__host__ __device__` under hipcc, plain inline C++ elsewhere (tools/alac_core_check.cpp).  A
// channel sample reaches conv() as the little-endian integer of its `width` bytes as they lie in
// the file (byte 0 in the low bits); conv() swaps a big-endian sample, then applies
//   u8 (v - 128) / 128, s16 / 32768, s24 / 8388608, s32 / 2147483648, f32 as is, f64 -> f32.
// Several channels: summed in channel order from -0.0, then divided by the channel count.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PCM_HD __host__ __device__ inline
#else
#define PCM_HD inline
#endif

namespace pcm_core {

enum Kind : int32_t { U8 = 0, S16, S24, S32, F32, F64 };

struct Layout {
    int32_t kind = S16;
    int32_t big = 0;    // big-endian samples
    int32_t width = 2;  // bytes per channel sample
    int32_t channels = 1;
};

PCM_HD int width_of(int kind) { return kind == U8 ? 1 : kind == S16 ? 2 : kind == S24 ? 3 : kind == F64 ? 8 : 4; }

// the `width` bytes at p as a little-endian integer
PCM_HD uint64_t load(const uint8_t* p, int width) {
    uint64_t v = 0;
    for (int i = 0; i < width; i++) v |= (uint64_t)p[i] << (8 * i);
    return v;
}

// one channel sample -> f32, the reference's per-type conversion
PCM_HD float conv(int kind, bool big, uint64_t raw) {
    const int width = width_of(kind);
    const uint64_t v = big ? __builtin_bswap64(raw) >> (64 - 8 * width) : raw;
    switch (kind) {
        case U8: return ((float)(uint8_t)v - 128.0f) / 128.0f;
        case S16: return (float)(int16_t)(uint16_t)v / 32768.0f;
        case S24: {
            int32_t s = (int32_t)(v & 0xFFFFFFu);
            if (s & 0x800000) s -= 0x1000000;
            return (float)s / 8388608.0f;
        }
        case S32: return (float)(int32_t)(uint32_t)v / 2147483648.0f;
        case F32: {
            const uint32_t u = (uint32_t)v;
            float f;
            __builtin_memcpy(&f, &u, 4);
            return f;
        }
        case F64: {
            double d;
            __builtin_memcpy(&d, &v, 8);
            return (float)d;
        }
    }
    return 0.0f;
}

// one frame -> mono; raw(c) gives channel c's sample bytes as load() does
template <class Raw>
PCM_HD float frame_mono(const Layout& l, Raw raw) {
    if (l.channels == 1) return conv(l.kind, l.big != 0, raw(0));
    float s = -0.0f;
    for (int c = 0; c < l.channels; c++) s = s + conv(l.kind, l.big != 0, raw(c));
    return s / (float)l.channels;
}

// the same from a frame's bytes in memory
PCM_HD float frame_mono_bytes(const Layout& l, const uint8_t* p) {
    return frame_mono(l, [&](int c) { return load(p + (size_t)c * (size_t)l.width, l.width); });
}

}  // namespace pcm_core
