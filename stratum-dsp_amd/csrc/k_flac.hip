// k_flac.hip — batched FLAC decode on the device (sdsp_decode_flac_batch_device) and the same four
// phases on the CPU (sdsp_debug_flac_decode_phased).  The frame-level code is flac_core.hpp, the
// code the host decoder (host_flac.hip) runs.
//
// The host decoder learns where a frame starts by decoding the one before it.  The batch gets the
// same result without that dependency:
//   scan    k_flac_scan: frame_header at every byte offset of every file's frame region; the hits
//           ("candidates": sync code, legal fields, UTF-8 number, CRC-8) go to a per-file list.
//           The host sorts each file's list by offset and lays out scratch and work ranges.
//   frames  k_flac_frames: one lane per candidate decodes the frame there (subframes, padding,
//           CRC-16) into the lane's slice of its wave's interleaved work range and, when the frame
//           holds, writes its mono f32 into the candidate's scratch slot.
//   chain   k_flac_chain: one lane per file replays the host loop over the sorted candidates: the
//           first candidate at or after pos is accepted when its frame held (pos = end + 2) and
//           passed over otherwise (pos = candidate + 1).  The host loop visits an offset only when
//           frame_header accepts it and moves one byte on any failure, so it meets exactly these
//           candidates in this order; a frame's decode depends on nothing but the file's bytes, so
//           `ok`, `end` and the samples computed ahead of time are the ones the host would compute.
//   gather  k_flac_gather: the accepted slots, copied to the file's contiguous output.
// On the host the phases are FlacStage's steps (decode_stages.hpp): plan, run (scan, frames, chain:
// the files' lengths), place, write (gather at a given base of the call's one output buffer).  Both
// batch entries use them: sdsp_decode_flac_batch_device here, sdsp_decode_batch_device in
// decode_batch.hip.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/stratum_hip_debug.h"
#include "flac_core.hpp"
#include "flac_host.hpp"
#include "decode_stages.hpp"
#include "flac_phased.hpp"
#include "sdsp_runtime.hpp"

namespace {

using namespace sdsp;
using namespace sdsp_dec;
namespace fc = flac_core;

constexpr uint32_t SCAN_BYTES = 16384;  // byte offsets per scan block
constexpr uint32_t PACK_BS = 0xFFFFu;   // candidate word: (bs - 1) | bps << 16 | channel code << 22 | header bytes << 26

__device__ inline uint32_t pack_cand(uint32_t bs, int bps, int chc, size_t hl) {  // flac_phased::pack
    return (bs - 1) | ((uint32_t)bps << 16) | ((uint32_t)chc << 22) | ((uint32_t)hl << 26);
}

// blocks[b] = (file, first offset): the block tries offsets [first, first + SCAN_BYTES) of the file
// that lie in its frame region; `first` is a multiple of 4 and every file starts 16-byte aligned
// with at least 16 readable bytes after its last one, so the aligned word pairs below stay inside
// the bytes buffer.
__global__ __launch_bounds__(256) void k_flac_scan(const uint8_t* __restrict__ bytes, const FlacFile* __restrict__ files,
                                                   const uint2* __restrict__ blocks, uint32_t* __restrict__ cnt,
                                                   uint2* __restrict__ cand) {
    const uint2 bk = blocks[blockIdx.x];
    const FlacFile f = files[bk.x];
    const uint8_t* d = bytes + f.base;
    const uint32_t hi = min(bk.y + SCAN_BYTES, f.size);
    for (uint32_t o = bk.y + threadIdx.x * 4u; o < hi; o += 1024u) {
        const uint32_t w0 = *reinterpret_cast<const uint32_t*>(d + o);
        const uint32_t w1 = *reinterpret_cast<const uint32_t*>(d + o + 4);
        const uint64_t v = (uint64_t)w0 | ((uint64_t)w1 << 32);
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t off = o + j;
            if (((v >> (8 * j)) & 0xFFu) != 0xFFu || ((v >> (8 * j + 8)) & 0xFEu) != 0xF8u) continue;
            if (off < f.start || off >= hi) continue;
            uint32_t bs = 0;
            int bps = 0, chc = 0;
            const size_t hl = fc::frame_header(d + off, (size_t)f.size - off, f.si_bps, &bs, &bps, &chc);
            if (hl == 0) continue;
            const uint32_t slot = atomicAdd(&cnt[bk.x], 1u);
            if (slot < f.cand_cap) cand[f.cand_base + slot] = make_uint2(off, pack_cand(bs, bps, chc, hl));
        }
    }
}

// One lane per candidate, candidates [first, end) of the sorted list; a block is one wave.  Wave w
// of the launch owns work[wave_off[w] .. wave_off[w] + 64 * wave_cap[w]) and lane l its elements
// l, l + 64, ...: sample i of lane l sits at (i * 64 + l).
__global__ __launch_bounds__(64) void k_flac_frames(const uint8_t* __restrict__ bytes, const FlacFile* __restrict__ files,
                                                    const uint32_t* __restrict__ c_file, const uint32_t* __restrict__ c_off,
                                                    const uint32_t* __restrict__ c_pack, const uint64_t* __restrict__ c_slot,
                                                    const uint64_t* __restrict__ wave_off, const uint32_t* __restrict__ wave_cap,
                                                    int64_t* __restrict__ work, float* __restrict__ scratch, uint64_t first,
                                                    uint64_t end, uint8_t* __restrict__ c_ok, uint32_t* __restrict__ c_end) {
    const uint64_t i = first + (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (i >= end) return;
    const uint64_t wv = first / 64u + blockIdx.x;
    const FlacFile f = files[c_file[i]];
    const uint32_t pk = c_pack[i];
    const uint32_t bs = (pk & PACK_BS) + 1;
    const int bps = (int)((pk >> 16) & 63u), chc = (int)((pk >> 22) & 15u);
    const size_t hl = pk >> 26;
    const fc::Work w{work + wave_off[wv] + threadIdx.x, 64, wave_cap[wv]};
    size_t e = 0;
    const bool ok = fc::decode_frame(bytes + f.base, f.size, c_off[i], hl, bs, bps, chc, w, &e);
    if (ok) fc::emit_mono(w, bs, bps, chc, scratch + c_slot[i], 1);
    c_ok[i] = ok ? 1 : 0;
    c_end[i] = ok ? (uint32_t)e : 0u;
}

// one lane per file: the host loop over the file's sorted candidates (flac_core::chain_file)
__global__ __launch_bounds__(64) void k_flac_chain(const FlacFile* __restrict__ files, const uint64_t* __restrict__ f_first,
                                                   const uint32_t* __restrict__ f_ncand, uint32_t n_files,
                                                   const uint32_t* __restrict__ c_off, const uint8_t* __restrict__ c_ok,
                                                   const uint32_t* __restrict__ c_end, const uint32_t* __restrict__ c_bs,
                                                   uint64_t* __restrict__ c_out, uint64_t* __restrict__ f_len,
                                                   uint32_t* __restrict__ f_acc, uint32_t* __restrict__ f_rej) {
    const uint32_t fi = blockIdx.x * 64u + threadIdx.x;
    if (fi >= n_files) return;
    const uint64_t a = f_first[fi];
    const fc::ChainCounts r =
        fc::chain_file(c_off + a, c_ok + a, c_end + a, c_bs + a, f_ncand[fi], files[fi].start, c_out + a);
    f_len[fi] = r.samples;
    f_acc[fi] = r.accepted;
    f_rej[fi] = r.rejected;
}

// one block per candidate: an accepted frame's scratch slot to its place in the file's output
__global__ __launch_bounds__(256) void k_flac_gather(const float* __restrict__ scratch, const uint64_t* __restrict__ c_slot,
                                                     const uint32_t* __restrict__ c_bs, const uint64_t* __restrict__ c_out,
                                                     const uint32_t* __restrict__ c_file, const uint64_t* __restrict__ f_outoff,
                                                     float* __restrict__ out) {
    const uint64_t i = blockIdx.x;
    const uint64_t o = c_out[i];
    if (o == ~0ull) return;
    const float* src = scratch + c_slot[i];
    float* dst = out + f_outoff[c_file[i]] + o;
    for (uint32_t k = threadIdx.x; k < c_bs[i]; k += 256u) dst[k] = src[k];
}

// ---- host side ----

std::mutex g_stats_mu;
std::map<int, sdsp_flac_decode_stats> g_stats;

}  // namespace

namespace sdsp_dec {

// stream-level parse; the file goes to the device, to the host decoder (past the budget) or fails
void FlacStage::plan(Call& k, uint64_t i) {
    sdsp_flac_stream si;
    size_t start = 0;
    std::string why;
    if (!sdsp_flac_parse_stream(k.files[i], k.sizes[i], &si, &start, &why)) {
        k.set_err(i, why);
        return;
    }
    k.rates[i] = si.rate ? si.rate : 44100u;
    // bytes + candidate slots + sorted candidate arrays, then scratch and output by STREAMINFO's
    // sample count (unknown: a generous multiple of the bytes); the scan's real figure is
    // checked again in run()
    const double est =
        3.0 * (double)k.sizes[i] + 8.0 * (si.total_samples ? (double)si.total_samples : 16.0 * (double)k.sizes[i]);
    if (k.need + est > k.budget) {
        k.fallback.push_back(i);
        return;
    }
    k.need += est;
    est_sum += est;
    FlacFile f{};
    f.base = k.reserve_bytes(i);
    f.cand_base = cand_total;
    f.size = (uint32_t)k.sizes[i];
    f.start = (uint32_t)start;
    f.cand_cap = (uint32_t)(k.sizes[i] / 8 + 16);
    f.si_bps = si.bps;
    cand_total += f.cand_cap;
    ft.push_back(f);
    dev_idx.push_back(i);
}

void FlacStage::run(Call& k, DevBuf& b_bytes, hipEvent_t ev_scan, hipEvent_t ev_frames, hipEvent_t ev_chain) {
    DeviceCtx& c = k.c;
    hipStream_t st = k.st;
    const size_t nd = ft.size();
    f_len.assign(nd, 0);
    f_outoff.assign(nd, 0);
    f_acc.assign(nd, 0);
    f_rej.assign(nd, 0);
    on_device.assign(nd, 1);
    // sorted candidates of the device files
    std::vector<uint32_t> c_file, c_off, c_pack, c_bs;
    std::vector<uint64_t> c_slot, f_first(nd, 0);
    std::vector<uint32_t> f_ncand(nd, 0);
    uint64_t scratch_total = 0;
    DevBuf& b_files = c.buf("flac.files");
    if (nd) {
        upload(b_files, ft, st);

        // ---- scan ----
        std::vector<uint2> blocks;
        for (size_t q = 0; q < nd; q++)
            for (uint64_t o = ft[q].start & ~3u; o < ft[q].size; o += SCAN_BYTES) blocks.push_back(make_uint2((uint32_t)q, (uint32_t)o));
        DevBuf& b_blocks = c.buf("flac.blocks");
        DevBuf& b_cnt = c.buf("flac.cnt");
        DevBuf& b_cand = c.buf("flac.cand");
        upload(b_blocks, blocks, st);
        b_cnt.ensure(nd * 4);
        b_cand.ensure(cand_total * 8);
        SDSP_HIP_CHECK(hipMemsetAsync(b_cnt.p, 0, nd * 4, st));
        if (!blocks.empty())
            hipLaunchKernelGGL(k_flac_scan, dim3((unsigned)blocks.size()), dim3(256), 0, st, b_bytes.as<uint8_t>(),
                               b_files.as<FlacFile>(), b_blocks.as<uint2>(), b_cnt.as<uint32_t>(), b_cand.as<uint2>());
        SDSP_HIP_CHECK(hipGetLastError());
        SDSP_HIP_CHECK(hipEventRecord(ev_scan, st));
        std::vector<uint32_t> cnt(nd);
        SDSP_HIP_CHECK(hipMemcpyAsync(cnt.data(), b_cnt.p, nd * 4, hipMemcpyDeviceToHost, st));
        SDSP_HIP_CHECK(hipStreamSynchronize(st));

        // ---- candidates to the host: sort per file, lay out scratch; files past a bound fall back ----
        std::vector<std::vector<uint2>> fc_list(nd);
        for (size_t q = 0; q < nd; q++) {
            if (cnt[q] > ft[q].cand_cap) {  // denser than one per 8 bytes: the list lost entries
                on_device[q] = 0;
                continue;
            }
            fc_list[q].resize(cnt[q]);
            if (cnt[q])
                SDSP_HIP_CHECK(hipMemcpyAsync(fc_list[q].data(), b_cand.as<uint2>() + ft[q].cand_base, (size_t)cnt[q] * 8,
                                              hipMemcpyDeviceToHost, st));
        }
        SDSP_HIP_CHECK(hipStreamSynchronize(st));
        // what plan() committed for these files is given back and the scan's real figure taken
        double used = k.need - est_sum;
        for (size_t q = 0; q < nd; q++) {
            if (!on_device[q]) continue;
            std::vector<uint2>& l = fc_list[q];
            std::sort(l.begin(), l.end(), [](const uint2& a, const uint2& b) { return a.x < b.x; });
            uint64_t sum_bs = 0;
            for (const uint2& e : l) sum_bs += (e.y & PACK_BS) + 1;
            const double real = 3.0 * (double)ft[q].size + 8.0 * (double)sum_bs + 40.0 * (double)l.size();
            if (used + real > k.budget) {  // the candidates' samples need more than STREAMINFO promised
                on_device[q] = 0;
                continue;
            }
            used += real;
            f_first[q] = c_off.size();
            f_ncand[q] = (uint32_t)l.size();
            for (const uint2& e : l) {
                c_file.push_back((uint32_t)q);
                c_off.push_back(e.x);
                c_pack.push_back(e.y);
                c_bs.push_back((e.y & PACK_BS) + 1);
                c_slot.push_back(scratch_total);
                scratch_total += (e.y & PACK_BS) + 1;
            }
        }
        k.need = used;
        for (size_t q = 0; q < nd; q++)
            if (!on_device[q]) k.fallback.push_back(dev_idx[q]);
    } else {
        SDSP_HIP_CHECK(hipEventRecord(ev_scan, st));
    }
    nc = c_off.size();

    DevBuf& b_cfile = c.buf("flac.c_file");
    DevBuf& b_coff = c.buf("flac.c_off");
    DevBuf& b_cpack = c.buf("flac.c_pack");
    DevBuf& b_cbs = c.buf("flac.c_bs");
    DevBuf& b_cslot = c.buf("flac.c_slot");
    DevBuf& b_cok = c.buf("flac.c_ok");
    DevBuf& b_cend = c.buf("flac.c_end");
    DevBuf& b_cout = c.buf("flac.c_out");
    DevBuf& b_scratch = c.buf("flac.scratch");
    if (nc) {
        // ---- frames: passes of whole waves under the work budget ----
        const uint64_t n_waves = (nc + 63) / 64;
        std::vector<uint64_t> wave_off(n_waves);
        std::vector<uint32_t> wave_cap(n_waves);
        std::vector<std::pair<uint64_t, uint64_t>> passes;  // wave ranges
        uint64_t work_max = 0, acc = 0, pass0 = 0;
        for (uint64_t w = 0; w < n_waves; w++) {
            uint32_t cap = 0;
            for (uint64_t i = w * 64; i < std::min(nc, w * 64 + 64); i++)
                cap = std::max(cap, (uint32_t)fc::channels_of((int)((c_pack[i] >> 22) & 15u)) * c_bs[i]);
            if (acc && (double)(acc + 64ull * cap) * 8.0 > k.work_budget) {
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
        DevBuf& b_woff = c.buf("flac.wave_off");
        DevBuf& b_wcap = c.buf("flac.wave_cap");
        DevBuf& b_work = c.buf("flac.work");
        upload(b_cfile, c_file, st);
        upload(b_coff, c_off, st);
        upload(b_cpack, c_pack, st);
        upload(b_cbs, c_bs, st);
        upload(b_cslot, c_slot, st);
        upload(b_woff, wave_off, st);
        upload(b_wcap, wave_cap, st);
        b_cok.ensure(nc);
        b_cend.ensure(nc * 4);
        b_cout.ensure(nc * 8);
        b_work.ensure(work_max * 8);
        b_scratch.ensure(scratch_total * 4);
        for (const auto& ps : passes) {
            const uint64_t first = ps.first * 64, end = std::min(nc, ps.second * 64);
            hipLaunchKernelGGL(k_flac_frames, dim3((unsigned)(ps.second - ps.first)), dim3(64), 0, st, b_bytes.as<uint8_t>(),
                               b_files.as<FlacFile>(), b_cfile.as<uint32_t>(), b_coff.as<uint32_t>(), b_cpack.as<uint32_t>(),
                               b_cslot.as<uint64_t>(), b_woff.as<uint64_t>(), b_wcap.as<uint32_t>(), b_work.as<int64_t>(),
                               b_scratch.as<float>(), first, end, b_cok.as<uint8_t>(), b_cend.as<uint32_t>());
            SDSP_HIP_CHECK(hipGetLastError());
        }
    }
    SDSP_HIP_CHECK(hipEventRecord(ev_frames, st));

    // ---- chain ----
    DevBuf& b_ffirst = c.buf("flac.f_first");
    DevBuf& b_fncand = c.buf("flac.f_ncand");
    DevBuf& b_flen = c.buf("flac.f_len");
    DevBuf& b_facc = c.buf("flac.f_acc");
    DevBuf& b_frej = c.buf("flac.f_rej");
    if (nd) {
        upload(b_ffirst, f_first, st);
        upload(b_fncand, f_ncand, st);
        b_flen.ensure(nd * 8);
        b_facc.ensure(nd * 4);
        b_frej.ensure(nd * 4);
        if (!nc) {  // files without a candidate: the chain still writes their zero counts
            upload(b_coff, c_off, st);
            upload(b_cbs, c_bs, st);
            b_cok.ensure(1);
            b_cend.ensure(4);
            b_cout.ensure(8);
        }
        hipLaunchKernelGGL(k_flac_chain, dim3((unsigned)((nd + 63) / 64)), dim3(64), 0, st, b_files.as<FlacFile>(),
                           b_ffirst.as<uint64_t>(), b_fncand.as<uint32_t>(), (uint32_t)nd, b_coff.as<uint32_t>(),
                           b_cok.as<uint8_t>(), b_cend.as<uint32_t>(), b_cbs.as<uint32_t>(), b_cout.as<uint64_t>(),
                           b_flen.as<uint64_t>(), b_facc.as<uint32_t>(), b_frej.as<uint32_t>());
        SDSP_HIP_CHECK(hipGetLastError());
        SDSP_HIP_CHECK(hipMemcpyAsync(f_len.data(), b_flen.p, nd * 8, hipMemcpyDeviceToHost, st));
        SDSP_HIP_CHECK(hipMemcpyAsync(f_acc.data(), b_facc.p, nd * 4, hipMemcpyDeviceToHost, st));
        SDSP_HIP_CHECK(hipMemcpyAsync(f_rej.data(), b_frej.p, nd * 4, hipMemcpyDeviceToHost, st));
    }
    SDSP_HIP_CHECK(hipEventRecord(ev_chain, st));
}

// the files' places in the one output buffer, from `total` on; returns the new total
uint64_t FlacStage::place(Call& k, uint64_t total) {
    for (size_t q = 0; q < ft.size(); q++) {
        if (!on_device[q]) continue;
        f_outoff[q] = total;
        k.offsets[dev_idx[q]] = total;
        k.lens[dev_idx[q]] = f_len[q];
        total += f_len[q];
        device_files++;
        frames_accepted += f_acc[q];
        frames_rejected += f_rej[q];
    }
    return total;
}

void FlacStage::write(Call& k, float* out) {
    if (!nc) return;
    DeviceCtx& c = k.c;
    DevBuf& b_foutoff = c.buf("flac.f_outoff");
    upload(b_foutoff, f_outoff, k.st);
    hipLaunchKernelGGL(k_flac_gather, dim3((unsigned)nc), dim3(256), 0, k.st, c.buf("flac.scratch").as<float>(),
                       c.buf("flac.c_slot").as<uint64_t>(), c.buf("flac.c_bs").as<uint32_t>(), c.buf("flac.c_out").as<uint64_t>(),
                       c.buf("flac.c_file").as<uint32_t>(), b_foutoff.as<uint64_t>(), out);
    SDSP_HIP_CHECK(hipGetLastError());
}

}  // namespace sdsp_dec

namespace {

int32_t decode_batch(const uint8_t* const* files, const uint64_t* sizes, uint64_t n_files, int32_t device, void* stream,
                     float** d_samples, uint64_t* offsets, uint64_t* lens, uint32_t* rates, int32_t* status, char* errs) {
    const auto t_begin = std::chrono::steady_clock::now();
    sdsp_flac_decode_stats stt{};
    stt.files = n_files;
    DeviceCtx& c = device_ctx(device);
    std::lock_guard<std::mutex> lk(c.mu);
    SDSP_HIP_CHECK(hipSetDevice(device));
    Call k(c, stream ? (hipStream_t)stream : c.stream, device);
    k.files = files, k.sizes = sizes, k.n_files = n_files;
    k.offsets = offsets, k.lens = lens, k.rates = rates, k.status = status, k.errs = errs;
    hipStream_t st = k.st;

    // ---- host setup: stream-level parse, which files the device takes ----
    k.init_budget();
    k.reset_outputs();
    FlacStage flac;
    for (uint64_t i = 0; i < n_files; i++) {
        stt.bytes_in += sizes[i];
        if (!files[i] || !sdsp_is_native_flac(files[i], sizes[i]) || sizes[i] >= (1ull << 31))
            k.fallback.push_back(i);
        else
            flac.plan(k, i);
    }

    hipEvent_t ev[6];
    for (auto& e : ev) SDSP_HIP_CHECK(hipEventCreate(&e));
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < 6; i++) (void)hipEventDestroy(e[i]);
        }
    } evg{ev};

    SDSP_HIP_CHECK(hipEventRecord(ev[0], st));
    DevBuf& b_bytes = k.upload_bytes();
    flac.run(k, b_bytes, ev[1], ev[2], ev[3]);
    stt.candidates = flac.nc;

    // ---- the files the device path did not take: the host decoder (overlaps the kernels) ----
    k.decode_fallbacks();
    SDSP_HIP_CHECK(hipStreamSynchronize(st));

    // ---- output layout, gather, fallback upload ----
    uint64_t total = flac.place(k, 0);
    total = k.place_fallbacks(total);
    stt.device_files = flac.device_files;
    stt.frames_accepted = flac.frames_accepted;
    stt.frames_rejected = flac.frames_rejected;
    stt.host_fallback_files = k.host_tracks.size();
    for (uint64_t i = 0; i < n_files; i++) stt.error_files += status[i] != SDSP_OK;
    stt.samples_out = total;
    float* out = nullptr;  // the caller's: not one of the engine's grow-only buffers
    SDSP_HIP_CHECK(hipMalloc((void**)&out, std::max<uint64_t>(total, 1) * 4));
    try {
        flac.write(k, out);
        SDSP_HIP_CHECK(hipEventRecord(ev[4], st));
        k.upload_fallbacks(out);
        SDSP_HIP_CHECK(hipStreamSynchronize(st));
    } catch (...) {
        (void)hipFree(out);
        throw;
    }
    *d_samples = out;

    float ms = 0;
    SDSP_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    stt.scan_ms = ms;  // upload of the bytes + scan
    SDSP_HIP_CHECK(hipEventElapsedTime(&ms, ev[1], ev[2]));
    stt.frames_ms = ms;  // candidate round trip + frame decode
    SDSP_HIP_CHECK(hipEventElapsedTime(&ms, ev[2], ev[3]));
    stt.chain_ms = ms;
    SDSP_HIP_CHECK(hipEventElapsedTime(&ms, ev[3], ev[4]));
    stt.gather_ms = ms;
    stt.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    std::lock_guard<std::mutex> sl(g_stats_mu);
    g_stats[device] = stt;
    return SDSP_OK;
}

}  // namespace

extern "C" {

int32_t sdsp_decode_flac_batch_device(const uint8_t* const* files, const uint64_t* sizes, uint64_t n_files, int32_t device,
                                      void* stream, float** d_samples, uint64_t* offsets, uint64_t* lens,
                                      uint32_t* sample_rates, int32_t* status, char* errs) {
    if (!d_samples || (n_files && (!files || !sizes || !offsets || !lens || !sample_rates || !status || !errs)))
        return SDSP_ERR_INVALID_INPUT;
    *d_samples = nullptr;
    auto fail_all = [&](const char* msg) {
        for (uint64_t i = 0; i < n_files; i++) {
            status[i] = SDSP_ERR_PROCESSING;
            std::snprintf(errs + 256 * i, 256, "%s", msg);
            offsets[i] = lens[i] = 0;
            sample_rates[i] = 0;
        }
        return (int32_t)SDSP_ERR_PROCESSING;
    };
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail_all("Processing error: no HIP device");
    if (device < 0 || device >= ndev) return fail_all("Processing error: no such HIP device");
    try {
        return decode_batch(files, sizes, n_files, device, stream, d_samples, offsets, lens, sample_rates, status, errs);
    } catch (const std::exception& e) {
        return fail_all((std::string("Processing error: ") + e.what()).c_str());
    }
}

int32_t sdsp_last_flac_decode_stats(int32_t device, sdsp_flac_decode_stats* out) {
    if (!out) return SDSP_ERR_INVALID_INPUT;
    std::lock_guard<std::mutex> sl(g_stats_mu);
    auto it = g_stats.find(device);
    *out = it == g_stats.end() ? sdsp_flac_decode_stats{} : it->second;
    return SDSP_OK;
}

// The four phases on the CPU, through flac_core.hpp as the kernels run it.
int32_t sdsp_debug_flac_decode_phased(const uint8_t* data, uint64_t n, float** samples, uint64_t* n_samples,
                                      uint32_t* sample_rate, uint64_t counts[3], char* err, uint64_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!data || !samples || !n_samples || !sample_rate) return SDSP_ERR_INVALID_INPUT;
    *samples = nullptr;
    *n_samples = 0;
    try {
        sdsp_flac_stream si;
        size_t start = 0;
        std::string why;
        if (!sdsp_flac_parse_stream(data, n, &si, &start, &why)) {
            if (err && errlen) std::snprintf(err, errlen, "%s", why.c_str());
            return SDSP_ERR_DECODING;
        }
        flac_phased::Result r;
        flac_phased::decode(data, n, start, si.bps, &r);
        float* p = (float*)std::malloc(std::max<size_t>(r.samples.size(), 1) * sizeof(float));
        if (!p) return SDSP_ERR_PROCESSING;
        if (!r.samples.empty()) std::memcpy(p, r.samples.data(), r.samples.size() * sizeof(float));
        *samples = p;
        *n_samples = r.samples.size();
        *sample_rate = si.rate ? si.rate : 44100u;
        if (counts) {
            counts[0] = r.candidates;
            counts[1] = r.accepted;
            counts[2] = r.rejected;
        }
        return SDSP_OK;
    } catch (const std::exception& e) {
        if (err && errlen) std::snprintf(err, errlen, "decoding failed: %s", e.what());
        return SDSP_ERR_DECODING;
    }
}

}  // extern "C"
