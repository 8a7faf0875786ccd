// k_pcm.hip — linear PCM (RIFF/WAVE, AIFF / AIFF-C) to mono f32 on the device (the PCM stage of
// sdsp_decode_batch_device) and the planned conversion on the CPU (sdsp_debug_pcm_decode_planned).
// The per-sample conversion and the channel mix are pcm_core.hpp, the code the host decoders run.
//
// PCM needs no decode: the host plan (sdsp_pcm_plan_wav / _aiff) gives the sample layout, the data
// offset and the frame count, so the track's length is known before any kernel runs and
// k_pcm_mono writes straight into the call's output buffer.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/stratum_hip_debug.h"
#include "decode_stages.hpp"
#include "pcm_core.hpp"

namespace {

using namespace sdsp;
using namespace sdsp_dec;

constexpr uint32_t PCM_BLOCK_FRAMES = 4096;  // output frames per block

// The `width` (<= 8) bytes at byte address `addr` of the bytes buffer as a little-endian integer,
// from aligned 32-bit loads: the data offset and 3-byte samples make most addresses unaligned.  A
// sample spans at most three words; the loads stay inside the buffer because every file is
// followed by at least 16 bytes.
__device__ inline uint64_t load_sample(const uint32_t* __restrict__ words, uint64_t addr, int width) {
    const uint64_t wi = addr >> 2;
    const uint32_t sh = (uint32_t)(addr & 3u) * 8u;
    const uint32_t span = (uint32_t)(addr & 3u) + (uint32_t)width;
    uint64_t v = words[wi];
    if (span > 4) v |= (uint64_t)words[wi + 1] << 32;
    v >>= sh;
    if (span > 8) v |= (uint64_t)words[wi + 2] << (64 - sh);  // sh > 0 here
    return width == 8 ? v : v & ((1ull << (8 * width)) - 1);
}

// blocks[b] = (file, chunk): the block converts frames [chunk * PCM_BLOCK_FRAMES, + PCM_BLOCK_FRAMES)
// of the file, one output frame per lane-iteration; adjacent lanes read adjacent frames.
__global__ __launch_bounds__(256) void k_pcm_mono(const uint32_t* __restrict__ words, const PcmFile* __restrict__ files,
                                                  const uint2* __restrict__ blocks, float* __restrict__ out) {
    const uint2 bk = blocks[blockIdx.x];
    const PcmFile f = files[bk.x];
    const uint64_t lo = (uint64_t)bk.y * PCM_BLOCK_FRAMES;
    const uint64_t hi = min(lo + (uint64_t)PCM_BLOCK_FRAMES, f.frames);
    const uint64_t stride = (uint64_t)f.lay.width * (uint64_t)f.lay.channels;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += 256u) {
        const uint64_t a = f.src + i * stride;
        out[f.dst + i] = pcm_core::frame_mono(
            f.lay, [&](int c) { return load_sample(words, a + (uint64_t)c * (uint64_t)f.lay.width, f.lay.width); });
    }
}

}  // namespace

namespace sdsp_dec {

void PcmStage::plan(Call& k, uint64_t i, bool aiff) {
    sdsp_pcm_plan pl;
    std::string why;
    const int r = aiff ? sdsp_pcm_plan_aiff(k.files[i], k.sizes[i], &pl, &why) : sdsp_pcm_plan_wav(k.files[i], k.sizes[i], &pl, &why);
    if (r < 0) {
        k.set_err(i, why);
        return;
    }
    const double est = 1.0 * (double)k.sizes[i] + 32.0 + 4.0 * (double)pl.frames;
    if (r == 0 || pl.lay.channels > PCM_MAX_CHANNELS || k.need + est > k.budget) {
        k.fallback.push_back(i);
        return;
    }
    k.need += est;
    k.rates[i] = pl.rate;
    PcmFile f{};
    f.src = k.reserve_bytes(i) + pl.data_off;  // data_off + frames * stride <= the file's size (the plan clips)
    f.frames = pl.frames;
    f.lay = pl.lay;
    ft.push_back(f);
    dev_idx.push_back(i);
}

uint64_t PcmStage::place(Call& k, uint64_t total) {
    for (size_t q = 0; q < ft.size(); q++) {
        ft[q].dst = total;
        k.offsets[dev_idx[q]] = total;
        k.lens[dev_idx[q]] = ft[q].frames;
        total += ft[q].frames;
        device_files++;
    }
    return total;
}

void PcmStage::write(Call& k, DevBuf& b_bytes, float* out) {
    std::vector<uint2> blocks;
    for (size_t q = 0; q < ft.size(); q++)
        for (uint64_t ch = 0; ch * PCM_BLOCK_FRAMES < ft[q].frames; ch++) blocks.push_back(make_uint2((uint32_t)q, (uint32_t)ch));
    if (blocks.empty()) return;
    DevBuf& b_files = k.c.buf("pcm.files");
    DevBuf& b_blocks = k.c.buf("pcm.blocks");
    upload(b_files, ft, k.st);
    upload(b_blocks, blocks, k.st);
    hipLaunchKernelGGL(k_pcm_mono, dim3((unsigned)blocks.size()), dim3(256), 0, k.st, b_bytes.as<uint32_t>(),
                       b_files.as<PcmFile>(), b_blocks.as<uint2>(), out);
    SDSP_HIP_CHECK(hipGetLastError());
}

}  // namespace sdsp_dec

extern "C" {

// The device path's steps on the CPU: plan, then pcm_core over the planned range.
int32_t sdsp_debug_pcm_decode_planned(const uint8_t* data, uint64_t n, float** samples, uint64_t* n_samples,
                                      uint32_t* sample_rate, uint64_t info[4], char* err, uint64_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!data || !samples || !n_samples || !sample_rate) return SDSP_ERR_INVALID_INPUT;
    *samples = nullptr;
    *n_samples = 0;
    try {
        const SdspFormat fm = sdsp_probe_format(data, n);
        sdsp_pcm_plan pl;
        std::string why;
        int r = 0;
        if (fm == SdspFormat::AIFF)
            r = sdsp_pcm_plan_aiff(data, n, &pl, &why);
        else if (fm == SdspFormat::WAV)
            r = sdsp_pcm_plan_wav(data, n, &pl, &why);
        if (r < 0) {
            if (err && errlen) std::snprintf(err, errlen, "%s", why.c_str());
            return SDSP_ERR_DECODING;
        }
        if (r == 0) {
            if (err && errlen) std::snprintf(err, errlen, "not planned: not linear PCM in RIFF/WAVE or AIFF");
            return SDSP_ERR_NOT_IMPLEMENTED;
        }
        std::vector<float> mono;
        sdsp_pcm_convert_plan(data, pl, &mono);
        float* p = (float*)std::malloc(std::max<size_t>(mono.size(), 1) * sizeof(float));
        if (!p) return SDSP_ERR_PROCESSING;
        if (!mono.empty()) std::memcpy(p, mono.data(), mono.size() * sizeof(float));
        *samples = p;
        *n_samples = mono.size();
        *sample_rate = pl.rate;
        if (info) {
            info[0] = (uint64_t)pl.lay.kind | ((uint64_t)(pl.lay.big != 0) << 8);
            info[1] = (uint64_t)pl.lay.channels;
            info[2] = pl.data_off;
            info[3] = pl.frames;
        }
        return SDSP_OK;
    } catch (const std::exception& e) {
        if (err && errlen) std::snprintf(err, errlen, "decoding failed: %s", e.what());
        return SDSP_ERR_DECODING;
    }
}

}  // extern "C"
