// k_vorbis.hip — batched Ogg Vorbis decode on the device (the Vorbis stage of
// sdsp_decode_audio_batch_device) and the same phases on the CPU (sdsp_debug_vorbis_decode_phased).
// The packet-level code is vorbis_core.hpp, the code the host decoder (host_vorbis.hip) runs.
//
// A Vorbis audio packet decodes from the setup header and its own bytes; packets meet only in the
// overlap-add of neighbouring windowed blocks, and block sizes, window shapes and output offsets
// follow from each packet's first bits.  So the host plan (sdsp_vorbis_plan_ogg) fixes the whole
// layout, the track lengths included, before any kernel runs:
//   packets  k_vorbis_packets: one lane per packet decodes floors and residues, un-couples,
//            multiplies and writes the packet's spectra (channels x n/2 f32); the lane's scratch is
//            its slice of its wave's interleaved work range, the floor's Y list is in LDS;
//   imdct    k_vorbis_imdct: per (packet, channel) the n/4-point complex FFT in double in LDS and
//            the windowed block of n f32; a workgroup takes as many short blocks as fill its LDS;
//   ola      k_vorbis_ola: one thread per output sample finds its packet pair by the planned
//            offsets, adds prev + cur per channel, mixes to mono and writes the track in place.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/stratum_hip_debug.h"
#include "decode_stages.hpp"
#include "vorbis_core.hpp"
#include "vorbis_phased.hpp"

namespace {

using namespace sdsp;
using namespace sdsp_dec;
namespace vc = vorbis_core;

// the stage's flat tables on the device; bt[lg] is block size 1 << lg (6 .. 13)
struct VorbisDev {
    const vc::Book* books;
    const int32_t* trees;
    const float* vq;
    const vc::Floor* floors;
    const vc::Residue* residues;
    const vc::Mapping* maps;
    const vc::Mode* modes;
    const float* inv_db;
    vc::BlockTables bt[14];
};

__device__ inline vc::Setup setup_of(const VorbisDev& d, const VorbisFile& f) {
    vc::Setup s;
    s.channels = f.channels, s.bs0 = f.bs0, s.bs1 = f.bs1, s.nmodes = f.nmodes;
    s.books = d.books + f.book_off, s.trees = d.trees + f.tree_off, s.vq = d.vq + f.vq_off;
    s.floors = d.floors + f.floor_off, s.residues = d.residues + f.res_off, s.maps = d.maps + f.map_off;
    s.modes = d.modes + f.mode_off, s.inv_db = d.inv_db;
    return s;
}

__host__ __device__ inline int lg2(int n) {
    int lg = 0;
    while ((1 << lg) < n) lg++;
    return lg;
}

// One lane per packet, packets [first, end); a block is one wave.  Wave w of the launch owns
// work[wave_off[w] .. wave_off[w] + 64 * wave_cap[w]) and lane l its words l, l + 64, ...: word i of
// lane l sits at (i * 64 + l).  The floor's Y list (65 x int32 per lane, indexed at run time) lives
// in LDS laid out [k][lane]: 16.25 KiB per wave.
__global__ __launch_bounds__(64) void k_vorbis_packets(VorbisDev d, const uint8_t* __restrict__ bytes,
                                                       const VorbisFile* __restrict__ files, const VorbisPacket* __restrict__ pk,
                                                       const uint64_t* __restrict__ wave_off, const uint32_t* __restrict__ wave_cap,
                                                       uint32_t* __restrict__ work, float* __restrict__ spectra, uint64_t first,
                                                       uint64_t end, uint32_t* __restrict__ p_zero) {
    __shared__ int32_t ylist[vc::FLOOR_MAX_POINTS * 64];
    const uint64_t i = first + (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (i >= end) return;
    const uint64_t wv = first / 64u + blockIdx.x;
    const VorbisPacket p = pk[i];
    const vc::Setup s = setup_of(d, files[p.file]);
    const vc::Work w{work + wave_off[wv] + threadIdx.x, 64, wave_cap[wv]};
    const vc::YStore Y{ylist + threadIdx.x, 64};
    int32_t zeroed = 0;
    const int32_t e = vc::decode_packet(s, bytes + p.off, p.size, w, Y, spectra + p.spec, &zeroed);
    p_zero[i] = (e == vc::OK && zeroed) ? 1u : 0u;
}

constexpr int IMDCT_LDS_POINTS = 2048;  // 32 KiB of double pairs: the largest FFT, or several short ones

// Items [i0, i1) are (packet, channel) pairs of block size n; a workgroup takes G of them (G * n/4
// <= IMDCT_LDS_POINTS), so short blocks share a workgroup.
__global__ __launch_bounds__(256) void k_vorbis_imdct(VorbisDev d, const VorbisFile* __restrict__ files,
                                                      const VorbisPacket* __restrict__ pk, const uint2* __restrict__ items,
                                                      uint32_t i0, uint32_t i1, int n, int G, const float* __restrict__ spectra,
                                                      float* __restrict__ blocks) {
    __shared__ vc::cd a[IMDCT_LDS_POINTS];
    const int M = n / 2, H = n / 4, lgH = lg2(H);
    const uint32_t base = i0 + blockIdx.x * (uint32_t)G;
    if (base >= i1) return;
    const int cnt = (int)min((uint32_t)G, i1 - base);
    const vc::BlockTables tb = d.bt[lg2(n)];
    for (int t = threadIdx.x; t < cnt * H; t += 256) {
        const int g = t / H, k = t - g * H;
        const uint2 it = items[base + g];
        vc::imdct_pre(spectra + pk[it.x].spec + (size_t)it.y * (size_t)M, M, lgH, k, tb.pre, a + g * H);
    }
    __syncthreads();
    for (int len = 2; len <= H; len <<= 1) {
        for (int t = threadIdx.x; t < cnt * (H / 2); t += 256) {
            const int g = t / (H / 2), q = t - g * (H / 2);
            vc::fft_butterfly(a + g * H, H, len, q, tb.tw);
        }
        __syncthreads();
    }
    for (int t = threadIdx.x; t < cnt * n; t += 256) {
        const int g = t / n, q = t - g * n;
        const uint2 it = items[base + g];
        const VorbisPacket p = pk[it.x];
        const int bs0 = files[p.file].bs0;
        const float y = vc::imdct_out(a + g * H, M, q, tb.post);
        blocks[2 * p.spec + (size_t)it.y * (size_t)n + (size_t)q] =
            y * vc::window_at(n, bs0, p.blockflag, p.prev_long, p.next_long, q, tb, d.bt[lg2(bs0)]);
    }
}

// blockIdx.y is the file (of [f0, ..)), blockIdx.x a run of 256 output samples of its track
__global__ __launch_bounds__(256) void k_vorbis_ola(const VorbisFile* __restrict__ files, const VorbisPacket* __restrict__ pk,
                                                    uint32_t f0, const float* __restrict__ blocks, float* __restrict__ out) {
    const VorbisFile f = files[f0 + blockIdx.y];
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= f.frames) return;  // frames > 0: at least two packets
    const uint32_t q = vorbis_phased::find_packet(pk, f.p_first, f.p_count, j);
    const VorbisPacket p = pk[q];
    out[f.out_off + j] = vc::ola_mix(blocks + 2 * pk[q - 1].spec, p.prev_n, blocks + 2 * p.spec, p.n, f.channels, (int)(j - p.out));
}

}  // namespace

namespace sdsp_dec {

// the Ogg demultiplex and the header parse; the file goes to the device, to the host decoder (not
// Vorbis, setup tables past the cap, past the budget) or fails with the host's text
std::vector<VorbisPrepared> VorbisStage::prepare(const Call& k, const std::vector<uint64_t>& idx) {
    std::vector<VorbisPrepared> out(idx.size());
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t q; (q = next++) < idx.size();) {
            VorbisPrepared& p = out[q];
            try {
                p.r = sdsp_vorbis_plan_ogg(k.files[idx[q]], k.sizes[idx[q]], &p.pl, &p.why);
            } catch (const std::exception& e) {  // sizes a damaged header declares can make an allocation fail
                p.r = -2;
                p.why = std::string("decoding failed: ") + e.what();
            }
        }
    };
    const size_t nt = std::min<size_t>({idx.size(), 16, std::max(1u, std::thread::hardware_concurrency())});
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nt; t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    return out;
}

void VorbisStage::plan(Call& k, uint64_t i, VorbisPrepared& pre) {
    sdsp_vorbis_plan& pl = pre.pl;
    const int r = pre.r;
    if (r < 0) {
        k.set_err(i, pre.why);
        return;
    }
    if (r == 0) {  // Ogg FLAC, Opus, anything else: the host decoder and its text
        k.fallback.push_back(i);
        return;
    }
    const sdsp_vorbis_setup& su = pl.setup;
    const uint64_t np = pl.packets.size(), C = (uint64_t)su.channels;
    uint64_t half = 0;  // the sum of n/2 over the kept packets
    for (const auto& p : pl.packets) half += p.n / 2;
    // packet bytes + tables + spectra (4 C n/2) + windowed blocks (4 C n) + packet records and
    // imdct items + output
    const double est = (double)pl.bytes.size() + (double)su.table_bytes() + 12.0 * (double)C * (double)half +
                       (double)np * (sizeof(VorbisPacket) + 4.0 + 8.0 * (double)C) + 4.0 * (double)pl.frames;
    if (su.table_bytes() > VORBIS_MAX_TABLE_BYTES || (pk.size() + np) * C >= (1ull << 31) ||
        k.need + est > k.budget) {
        k.fallback.push_back(i);
        return;
    }
    k.need += est;
    k.rates[i] = su.rate;
    VorbisFile f{};
    f.tree_off = trees.size(), f.vq_off = vq.size();
    f.book_off = (uint32_t)books.size(), f.floor_off = (uint32_t)floors.size(), f.res_off = (uint32_t)residues.size();
    f.map_off = (uint32_t)maps.size(), f.mode_off = (uint32_t)modes.size();
    f.channels = su.channels, f.bs0 = su.bs[0], f.bs1 = su.bs[1], f.nmodes = (int32_t)su.modes.size();
    f.p_first = (uint32_t)pk.size(), f.p_count = (uint32_t)np;
    f.frames = pl.frames;
    books.insert(books.end(), su.books.begin(), su.books.end());
    trees.insert(trees.end(), su.trees.begin(), su.trees.end());
    vq.insert(vq.end(), su.vq.begin(), su.vq.end());
    floors.insert(floors.end(), su.floors.begin(), su.floors.end());
    residues.insert(residues.end(), su.residues.begin(), su.residues.end());
    maps.insert(maps.end(), su.maps.begin(), su.maps.end());
    modes.insert(modes.end(), su.modes.begin(), su.modes.end());
    const uint64_t byte0 = bytes_total;
    bytes_total += pl.bytes.size();
    file_byte0.push_back(byte0);
    for (const auto& p : pl.packets) {
        VorbisPacket q{};
        q.off = byte0 + p.off, q.spec = spec_total, q.out = p.out;
        q.size = p.size, q.file = (uint32_t)ft.size();
        q.n = p.n, q.prev_n = p.prev_n;
        q.blockflag = p.blockflag, q.prev_long = p.prev_long, q.next_long = p.next_long;
        spec_total += C * (p.n / 2);
        pk.push_back(q);
    }
    file_bytes.push_back(std::move(pl.bytes));
    ft.push_back(f);
    dev_idx.push_back(i);
}

void VorbisStage::run(Call& k) {
    DeviceCtx& c = k.c;
    hipStream_t st = k.st;
    const uint64_t np = pk.size();
    p_zero.assign(np, 0);
    if (ft.empty() || !np) return;
    DevBuf& b_bytes = c.buf("vorbis.bytes");
    b_bytes.ensure(std::max<uint64_t>(bytes_total, 1));
    for (size_t q = 0; q < file_bytes.size(); q++)
        if (!file_bytes[q].empty())
            SDSP_HIP_CHECK(hipMemcpyAsync(b_bytes.as<uint8_t>() + file_byte0[q], file_bytes[q].data(), file_bytes[q].size(),
                                          hipMemcpyHostToDevice, st));
    upload(c.buf("vorbis.pk"), pk, st);
    upload(c.buf("vorbis.books"), books, st);
    upload(c.buf("vorbis.trees"), trees, st);
    upload(c.buf("vorbis.vq"), vq, st);
    upload(c.buf("vorbis.floors"), floors, st);
    upload(c.buf("vorbis.residues"), residues, st);
    upload(c.buf("vorbis.maps"), maps, st);
    upload(c.buf("vorbis.modes"), modes, st);
    // the per-block-size tables of the sizes in use and the inverse-dB table, in one buffer
    VorbisDev d{};
    {
        tab.clear();  // doubles: every table starts 8-byte aligned
        size_t at[14][5] = {};
        bool use[14] = {};
        for (const VorbisFile& f : ft) use[lg2(f.bs0)] = use[lg2(f.bs1)] = true;
        auto put = [&](const void* p, size_t bytes_) {
            const size_t o = tab.size();
            tab.resize(o + (bytes_ + 7) / 8);
            std::memcpy(tab.data() + o, p, bytes_);
            return o;
        };
        for (int lg = 6; lg < 14; lg++) {
            if (!use[lg]) continue;
            const sdsp_vorbis_tables& t = sdsp_vorbis_block_tables(1 << lg);
            at[lg][0] = put(t.pre.data(), t.pre.size() * sizeof(vc::cd));
            at[lg][1] = put(t.post.data(), t.post.size() * sizeof(vc::cd));
            at[lg][2] = put(t.tw.data(), t.tw.size() * sizeof(vc::cd));
            at[lg][3] = put(t.up.data(), t.up.size() * 4);
            at[lg][4] = put(t.dn.data(), t.dn.size() * 4);
        }
        const size_t at_db = put(sdsp_vorbis_inv_db(), 256 * 4);
        DevBuf& b_tab = c.buf("vorbis.tables");
        upload(b_tab, tab, st);
        const double* base = b_tab.as<double>();
        for (int lg = 6; lg < 14; lg++)
            if (use[lg])
                d.bt[lg] = vc::BlockTables{(const vc::cd*)(base + at[lg][0]), (const vc::cd*)(base + at[lg][1]),
                                           (const vc::cd*)(base + at[lg][2]), (const float*)(base + at[lg][3]),
                                           (const float*)(base + at[lg][4])};
        d.inv_db = (const float*)(base + at_db);
    }
    d.books = c.buf("vorbis.books").as<vc::Book>(), d.trees = c.buf("vorbis.trees").as<int32_t>();
    d.vq = c.buf("vorbis.vq").as<float>(), d.floors = c.buf("vorbis.floors").as<vc::Floor>();
    d.residues = c.buf("vorbis.residues").as<vc::Residue>(), d.maps = c.buf("vorbis.maps").as<vc::Mapping>();
    d.modes = c.buf("vorbis.modes").as<vc::Mode>();
    DevBuf& b_files = c.buf("vorbis.files");  // out_off is not known yet: the file table goes up again in write()
    upload(b_files, ft, st);
    DevBuf& b_spec = c.buf("vorbis.spectra");
    DevBuf& b_blocks = c.buf("vorbis.blocks");
    DevBuf& b_pzero = c.buf("vorbis.p_zero");
    b_spec.ensure(spec_total * 4);
    b_blocks.ensure(spec_total * 8);
    b_pzero.ensure(np * 4);

    // ---- packets: passes of whole waves under the work budget ----
    {
        const uint64_t n_waves = (np + 63) / 64;
        wave_off.assign(n_waves, 0);
        wave_cap.assign(n_waves, 0);
        std::vector<std::pair<uint64_t, uint64_t>> passes;  // wave ranges
        uint64_t work_max = 0, acc = 0, pass0 = 0;
        for (uint64_t w = 0; w < n_waves; w++) {
            uint32_t cap = 0;
            for (uint64_t i = w * 64; i < std::min(np, w * 64 + 64); i++)
                cap = std::max(cap, (uint32_t)vc::work_words(ft[pk[i].file].channels, pk[i].n / 2));
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
        DevBuf& b_woff = c.buf("vorbis.wave_off");
        DevBuf& b_wcap = c.buf("vorbis.wave_cap");
        DevBuf& b_work = c.buf("flac.work");  // the work range is one buffer for every decoder
        upload(b_woff, wave_off, st);
        upload(b_wcap, wave_cap, st);
        b_work.ensure(work_max * 4);
        for (const auto& ps : passes) {
            const uint64_t first = ps.first * 64, end = std::min(np, ps.second * 64);
            hipLaunchKernelGGL(k_vorbis_packets, dim3((unsigned)(ps.second - ps.first)), dim3(64), 0, st, d,
                               c.buf("vorbis.bytes").as<uint8_t>(), b_files.as<VorbisFile>(), c.buf("vorbis.pk").as<VorbisPacket>(),
                               b_woff.as<uint64_t>(), b_wcap.as<uint32_t>(), b_work.as<uint32_t>(), b_spec.as<float>(), first, end,
                               b_pzero.as<uint32_t>());
            SDSP_HIP_CHECK(hipGetLastError());
        }
    }
    // ---- imdct: the (packet, channel) items by block size, one launch per size ----
    {
        items.clear();
        uint32_t i0[15] = {};
        for (int lg = 6; lg < 14; lg++) {
            i0[lg] = (uint32_t)items.size();
            for (uint64_t i = 0; i < np; i++)
                if (pk[i].n == (1u << lg))
                    for (int ch = 0; ch < ft[pk[i].file].channels; ch++) items.push_back(make_uint2((uint32_t)i, (uint32_t)ch));
        }
        i0[14] = (uint32_t)items.size();
        DevBuf& b_items = c.buf("vorbis.items");
        upload(b_items, items, st);
        for (int lg = 6; lg < 14; lg++) {
            const uint32_t cnt = i0[lg + 1] - i0[lg];
            if (!cnt) continue;
            const int n = 1 << lg;
            const int G = std::min(32, IMDCT_LDS_POINTS / (n / 4));
            hipLaunchKernelGGL(k_vorbis_imdct, dim3((cnt + G - 1) / G), dim3(256), 0, st, d, b_files.as<VorbisFile>(),
                               c.buf("vorbis.pk").as<VorbisPacket>(), b_items.as<uint2>(), i0[lg], i0[lg + 1], n, G, b_spec.as<float>(),
                               b_blocks.as<float>());
            SDSP_HIP_CHECK(hipGetLastError());
        }
    }
    SDSP_HIP_CHECK(hipMemcpyAsync(p_zero.data(), b_pzero.p, np * 4, hipMemcpyDeviceToHost, st));
}

uint64_t VorbisStage::place(Call& k, uint64_t total) {
    for (size_t q = 0; q < ft.size(); q++) {
        ft[q].out_off = total;
        k.offsets[dev_idx[q]] = total;
        k.lens[dev_idx[q]] = ft[q].frames;
        total += ft[q].frames;
        device_files++;
        packets += ft[q].p_count;
    }
    for (uint32_t z : p_zero) packets_zeroed += z;
    return total;
}

void VorbisStage::write(Call& k, float* out) {
    if (ft.empty()) return;
    DeviceCtx& c = k.c;
    DevBuf& b_files = c.buf("vorbis.files");
    upload(b_files, ft, k.st);
    for (size_t f0 = 0; f0 < ft.size(); f0 += 65535) {
        const size_t nf = std::min<size_t>(65535, ft.size() - f0);
        uint64_t longest = 0;
        for (size_t q = f0; q < f0 + nf; q++) longest = std::max(longest, ft[q].frames);
        if (!longest) continue;
        hipLaunchKernelGGL(k_vorbis_ola, dim3((unsigned)((longest + 255) / 256), (unsigned)nf), dim3(256), 0, k.st,
                           b_files.as<VorbisFile>(), c.buf("vorbis.pk").as<VorbisPacket>(), (uint32_t)f0,
                           c.buf("vorbis.blocks").as<float>(), out);
        SDSP_HIP_CHECK(hipGetLastError());
    }
}

}  // namespace sdsp_dec

extern "C" {

// The device path's phases on the CPU, through vorbis_core.hpp as the kernels run it: plan, every
// packet's spectra, every (packet, channel) block, every output sample.  info: packets, zeroed.
int32_t sdsp_debug_vorbis_decode_phased(const uint8_t* data, uint64_t n, float** samples, uint64_t* n_samples,
                                        uint32_t* sample_rate, uint64_t info[2], char* err, uint64_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!data || !samples || !n_samples || !sample_rate) return SDSP_ERR_INVALID_INPUT;
    *samples = nullptr;
    *n_samples = 0;
    try {
        if (sdsp_probe_format(data, n) != SdspFormat::OGG) {
            if (err && errlen) std::snprintf(err, errlen, "not planned: not an Ogg stream");
            return SDSP_ERR_NOT_IMPLEMENTED;
        }
        sdsp_vorbis_plan pl;
        std::string why;
        const int r = sdsp_vorbis_plan_ogg(data, n, &pl, &why);
        if (r == 0) {
            if (err && errlen) std::snprintf(err, errlen, "not planned: not a Vorbis stream");
            return SDSP_ERR_NOT_IMPLEMENTED;
        }
        if (r < 0) {
            if (err && errlen) std::snprintf(err, errlen, "%s", why.c_str());
            return SDSP_ERR_DECODING;
        }
        vorbis_phased::Result res;
        vorbis_phased::decode(pl, &res);
        const uint64_t total = res.samples.size();
        float* p = (float*)std::malloc(std::max<size_t>(total, 1) * sizeof(float));
        if (!p) return SDSP_ERR_PROCESSING;
        if (total) std::memcpy(p, res.samples.data(), total * sizeof(float));
        *samples = p;
        *n_samples = total;
        *sample_rate = pl.setup.rate;
        if (info) {
            info[0] = res.packets;
            info[1] = res.zeroed;
        }
        return SDSP_OK;
    } catch (const std::exception& e) {
        if (err && errlen) std::snprintf(err, errlen, "decoding failed: %s", e.what());
        return SDSP_ERR_DECODING;
    }
}

}  // extern "C"
