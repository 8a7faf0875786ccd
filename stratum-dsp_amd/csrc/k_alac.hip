// k_alac.hip — batched Apple Lossless decode on the device (the ALAC stage of
// sdsp_decode_batch_device) and the same phases on the CPU (sdsp_debug_alac_decode_phased).  The
// packet-level code is alac_core.hpp, the code the host decoder (host_alac.hip) runs.
//
// ALAC packets are independent and the container's sample table names every packet's offset and
// size, so there is no scan: the host plan (sdsp_alac_plan_caf / _mp4) gives the packet table and
//   frames   k_alac_frames: one lane per packet decodes it into the lane's slice of its wave's
//            interleaved work range and, when the packet holds, writes its mono f32 into the
//            packet's slot of frame_length floats; the packet's sample count (0: the host's skip)
//            goes to p_cnt;
//   offsets  k_alac_offsets: one lane per file walks its packets' counts into output offsets and the
//            track's length (alac_core::layout_file), which the host reads back to size the output;
//   gather   k_alac_gather: the decoded slots, copied to the file's contiguous track.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/stratum_hip_debug.h"
#include "alac_core.hpp"
#include "alac_phased.hpp"
#include "decode_stages.hpp"

namespace {

using namespace sdsp;
using namespace sdsp_dec;
namespace ac = alac_core;

// One lane per packet, packets [first, end); a block is one wave.  Wave w of the launch owns
// work[wave_off[w] .. wave_off[w] + 64 * wave_cap[w]) and lane l its elements l, l + 64, ...: value i
// of lane l sits at (i * 64 + l).  The two channels' adaptive coefficients (2 x 32 x int16 per lane,
// indexed at run time and updated every sample) live in LDS laid out [k][lane]: 8 KiB per wave.
__global__ __launch_bounds__(64) void k_alac_frames(const uint8_t* __restrict__ bytes, const AlacFile* __restrict__ files,
                                                    const uint32_t* __restrict__ p_file, const uint32_t* __restrict__ p_off,
                                                    const uint32_t* __restrict__ p_size, const uint64_t* __restrict__ p_slot,
                                                    const uint64_t* __restrict__ wave_off, const uint32_t* __restrict__ wave_cap,
                                                    int32_t* __restrict__ work, float* __restrict__ scratch, uint64_t first,
                                                    uint64_t end, uint32_t* __restrict__ p_cnt) {
    __shared__ int16_t coefs[64 * 64];
    const uint64_t i = first + (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (i >= end) return;
    const uint64_t wv = first / 64u + blockIdx.x;
    const AlacFile f = files[p_file[i]];
    const ac::Work w{work + wave_off[wv] + threadIdx.x, 64, wave_cap[wv], f.cfg.frame_length};
    const ac::Coefs cf{coefs + threadIdx.x, 64};
    uint32_t n = 0;
    int32_t detail = 0;
    const int32_t e = ac::decode_frame(bytes + f.base + p_off[i], p_size[i], f.cfg, w, cf, scratch + p_slot[i], 1, &n, &detail);
    p_cnt[i] = e == ac::OK ? n : 0u;
}

// one lane per file: the packets' counts into offsets in the track, the track's length
__global__ __launch_bounds__(64) void k_alac_offsets(const uint64_t* __restrict__ f_first, const uint32_t* __restrict__ f_npk,
                                                     uint32_t n_files, const uint32_t* __restrict__ p_cnt,
                                                     uint64_t* __restrict__ p_out, uint64_t* __restrict__ f_len,
                                                     uint32_t* __restrict__ f_dec, uint32_t* __restrict__ f_skip) {
    const uint32_t fi = blockIdx.x * 64u + threadIdx.x;
    if (fi >= n_files) return;
    const uint64_t a = f_first[fi];
    uint32_t dec = 0, skp = 0;
    f_len[fi] = ac::layout_file(p_cnt + a, f_npk[fi], p_out + a, &dec, &skp);
    f_dec[fi] = dec;
    f_skip[fi] = skp;
}

// one block per packet: a decoded packet's slot to its place in the file's track
__global__ __launch_bounds__(256) void k_alac_gather(const float* __restrict__ scratch, const uint64_t* __restrict__ p_slot,
                                                     const uint32_t* __restrict__ p_cnt, const uint64_t* __restrict__ p_out,
                                                     const uint32_t* __restrict__ p_file, const uint64_t* __restrict__ f_outoff,
                                                     float* __restrict__ out) {
    const uint64_t i = blockIdx.x;
    const uint64_t o = p_out[i];
    if (o == ~0ull) return;
    const float* src = scratch + p_slot[i];
    float* dst = out + f_outoff[p_file[i]] + o;
    for (uint32_t q = threadIdx.x; q < p_cnt[i]; q += 256u) dst[q] = src[q];
}

}  // namespace

namespace sdsp_dec {

// the container parse; the file goes to the device, to the host decoder (a long frame, past the
// budget) or fails with the host's text
void AlacStage::plan(Call& k, uint64_t i, bool caf) {
    sdsp_alac_plan pl;
    std::string why;
    const bool ok = caf ? sdsp_alac_plan_caf(k.files[i], k.sizes[i], &pl, &why) : sdsp_alac_plan_mp4(k.files[i], k.sizes[i], &pl, &why);
    if (!ok) {
        k.set_err(i, why);
        return;
    }
    const uint64_t fl = pl.cfg.frame_length, npk = pl.packets.size();
    // bytes, then per packet a slot and its share of the output, the packet arrays
    const double est = 1.0 * (double)k.sizes[i] + 32.0 + (double)npk * (8.0 * (double)fl + 40.0);
    if (fl > ALAC_MAX_FRAME_LENGTH || npk >= (1ull << 31) || k.need + est > k.budget) {
        k.fallback.push_back(i);
        return;
    }
    k.need += est;
    k.rates[i] = pl.cfg.sample_rate ? pl.cfg.sample_rate : 44100u;
    AlacFile f{};
    f.base = k.reserve_bytes(i);
    f.cfg = pl.cfg;
    f_first.push_back(p_off.size());
    f_npk.push_back((uint32_t)npk);
    for (const auto& p : pl.packets) {  // inside the file (the plan checked), and the file is < 2^31 bytes
        p_file.push_back((uint32_t)ft.size());
        p_off.push_back((uint32_t)p.first);
        p_size.push_back((uint32_t)p.second);
        p_slot.push_back(scratch_total);
        scratch_total += fl;
    }
    ft.push_back(f);
    dev_idx.push_back(i);
}

void AlacStage::run(Call& k, DevBuf& b_bytes) {
    DeviceCtx& c = k.c;
    hipStream_t st = k.st;
    const size_t nd = ft.size();
    const uint64_t np = p_off.size();
    f_len.assign(nd, 0);
    f_outoff.assign(nd, 0);
    f_dec.assign(nd, 0);
    f_skip.assign(nd, 0);
    if (!nd) return;
    DevBuf& b_files = c.buf("alac.files");
    DevBuf& b_pfile = c.buf("alac.p_file");
    DevBuf& b_poff = c.buf("alac.p_off");
    DevBuf& b_psize = c.buf("alac.p_size");
    DevBuf& b_pslot = c.buf("alac.p_slot");
    DevBuf& b_pcnt = c.buf("alac.p_cnt");
    DevBuf& b_pout = c.buf("alac.p_out");
    DevBuf& b_scratch = c.buf("alac.scratch");  // the slots (the FLAC stage's own hold its frames until its gather)
    upload(b_files, ft, st);
    upload(b_pfile, p_file, st);
    upload(b_poff, p_off, st);
    upload(b_psize, p_size, st);
    upload(b_pslot, p_slot, st);
    b_pcnt.ensure(std::max<uint64_t>(np, 1) * 4);
    b_pout.ensure(std::max<uint64_t>(np, 1) * 8);
    if (np) {
        // ---- frames: passes of whole waves under the work budget ----
        const uint64_t n_waves = (np + 63) / 64;
        std::vector<uint64_t> wave_off(n_waves);
        std::vector<uint32_t> wave_cap(n_waves);
        std::vector<std::pair<uint64_t, uint64_t>> passes;  // wave ranges
        uint64_t work_max = 0, acc = 0, pass0 = 0;
        for (uint64_t w = 0; w < n_waves; w++) {
            uint32_t cap = 0;
            for (uint64_t i = w * 64; i < std::min(np, w * 64 + 64); i++) {
                const ac::Config& cfg = ft[p_file[i]].cfg;
                cap = std::max(cap, (uint32_t)cfg.channels * cfg.frame_length);
            }
            if (acc && (double)(acc + 64ull * cap) * 4.0 > k.work_budget) {
                passes.emplace_back(pass0, w);
                pass0 = w;
                acc = 0;
            }
            wave_cap[w] = cap;
            wave_off[w] = acc;
            acc += 64ull * cap;
            work_max = std::max(work_max, acc);
        }
        passes.emplace_back(pass0, n_waves);
        DevBuf& b_woff = c.buf("alac.wave_off");
        DevBuf& b_wcap = c.buf("alac.wave_cap");
        DevBuf& b_work = c.buf("flac.work");  // the work range is one buffer for both decoders
        upload(b_woff, wave_off, st);
        upload(b_wcap, wave_cap, st);
        b_work.ensure(work_max * 4);
        b_scratch.ensure(scratch_total * 4);
        for (const auto& ps : passes) {
            const uint64_t first = ps.first * 64, end = std::min(np, ps.second * 64);
            hipLaunchKernelGGL(k_alac_frames, dim3((unsigned)(ps.second - ps.first)), dim3(64), 0, st, b_bytes.as<uint8_t>(),
                               b_files.as<AlacFile>(), b_pfile.as<uint32_t>(), b_poff.as<uint32_t>(), b_psize.as<uint32_t>(),
                               b_pslot.as<uint64_t>(), b_woff.as<uint64_t>(), b_wcap.as<uint32_t>(), b_work.as<int32_t>(),
                               b_scratch.as<float>(), first, end, b_pcnt.as<uint32_t>());
            SDSP_HIP_CHECK(hipGetLastError());
        }
    }
    // ---- offsets ----
    DevBuf& b_ffirst = c.buf("alac.f_first");
    DevBuf& b_fnpk = c.buf("alac.f_npk");
    DevBuf& b_flen = c.buf("alac.f_len");
    DevBuf& b_fdec = c.buf("alac.f_dec");
    DevBuf& b_fskip = c.buf("alac.f_skip");
    upload(b_ffirst, f_first, st);
    upload(b_fnpk, f_npk, st);
    b_flen.ensure(nd * 8);
    b_fdec.ensure(nd * 4);
    b_fskip.ensure(nd * 4);
    hipLaunchKernelGGL(k_alac_offsets, dim3((unsigned)((nd + 63) / 64)), dim3(64), 0, st, b_ffirst.as<uint64_t>(),
                       b_fnpk.as<uint32_t>(), (uint32_t)nd, b_pcnt.as<uint32_t>(), b_pout.as<uint64_t>(), b_flen.as<uint64_t>(),
                       b_fdec.as<uint32_t>(), b_fskip.as<uint32_t>());
    SDSP_HIP_CHECK(hipGetLastError());
    SDSP_HIP_CHECK(hipMemcpyAsync(f_len.data(), b_flen.p, nd * 8, hipMemcpyDeviceToHost, st));
    SDSP_HIP_CHECK(hipMemcpyAsync(f_dec.data(), b_fdec.p, nd * 4, hipMemcpyDeviceToHost, st));
    SDSP_HIP_CHECK(hipMemcpyAsync(f_skip.data(), b_fskip.p, nd * 4, hipMemcpyDeviceToHost, st));
}

uint64_t AlacStage::place(Call& k, uint64_t total) {
    for (size_t q = 0; q < ft.size(); q++) {
        f_outoff[q] = total;
        k.offsets[dev_idx[q]] = total;
        k.lens[dev_idx[q]] = f_len[q];
        total += f_len[q];
        device_files++;
        packets += f_npk[q];
        packets_decoded += f_dec[q];
        packets_skipped += f_skip[q];
    }
    return total;
}

void AlacStage::write(Call& k, float* out) {
    const uint64_t np = p_off.size();
    if (!np) return;
    DeviceCtx& c = k.c;
    DevBuf& b_foutoff = c.buf("alac.f_outoff");
    upload(b_foutoff, f_outoff, k.st);
    hipLaunchKernelGGL(k_alac_gather, dim3((unsigned)np), dim3(256), 0, k.st, c.buf("alac.scratch").as<float>(),
                       c.buf("alac.p_slot").as<uint64_t>(), c.buf("alac.p_cnt").as<uint32_t>(), c.buf("alac.p_out").as<uint64_t>(),
                       c.buf("alac.p_file").as<uint32_t>(), b_foutoff.as<uint64_t>(), out);
    SDSP_HIP_CHECK(hipGetLastError());
}

}  // namespace sdsp_dec

extern "C" {

// The device path's phases on the CPU, through alac_core.hpp as the kernels run it: plan, every
// packet into its own slot with its count, offsets, gather.
int32_t sdsp_debug_alac_decode_phased(const uint8_t* data, uint64_t n, float** samples, uint64_t* n_samples,
                                      uint32_t* sample_rate, uint64_t counts[3], char* err, uint64_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!data || !samples || !n_samples || !sample_rate) return SDSP_ERR_INVALID_INPUT;
    *samples = nullptr;
    *n_samples = 0;
    try {
        const SdspFormat fm = sdsp_probe_format(data, n);
        const bool caf = fm == SdspFormat::CAF && sdsp_caf_is_alac(data, n);
        if (!caf && fm != SdspFormat::MP4) {
            if (err && errlen) std::snprintf(err, errlen, "not planned: not an ALAC container");
            return SDSP_ERR_NOT_IMPLEMENTED;
        }
        sdsp_alac_plan pl;
        std::string why;
        if (!(caf ? sdsp_alac_plan_caf(data, n, &pl, &why) : sdsp_alac_plan_mp4(data, n, &pl, &why))) {
            if (err && errlen) std::snprintf(err, errlen, "%s", why.c_str());
            return SDSP_ERR_DECODING;
        }
        alac_phased::Result r;
        alac_phased::decode(data, pl, &r);
        const uint64_t total = r.samples.size();
        float* p = (float*)std::malloc(std::max<size_t>(total, 1) * sizeof(float));
        if (!p) return SDSP_ERR_PROCESSING;
        if (total) std::memcpy(p, r.samples.data(), total * sizeof(float));
        *samples = p;
        *n_samples = total;
        *sample_rate = pl.cfg.sample_rate ? pl.cfg.sample_rate : 44100u;
        if (counts) {
            counts[0] = r.packets;
            counts[1] = r.decoded;
            counts[2] = r.skipped;
        }
        return SDSP_OK;
    } catch (const std::exception& e) {
        if (err && errlen) std::snprintf(err, errlen, "decoding failed: %s", e.what());
        return SDSP_ERR_DECODING;
    }
}

}  // extern "C"
