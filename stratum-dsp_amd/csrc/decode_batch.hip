// decode_batch.hip — sdsp_decode_batch_device, the batched lossless decode entry, and
// sdsp_decode_audio_batch_device, the same call with Ogg Vorbis on the device too.  Every file is
// probed as the host front-end probes it (sdsp_probe_format) and sent to its stage
// (decode_stages.hpp): native FLAC (k_flac.hip), ALAC in ISO MP4 / CAF (k_alac.hip), linear PCM in
// RIFF/WAVE and AIFF (k_pcm.hip), through the audio entry Ogg Vorbis (k_vorbis.hip); everything else, and what a stage leaves, goes to the host
// decoder and is uploaded.  All tracks land in one caller-owned output buffer.  Also the parts of a
// call the two batch entries share (Call's methods).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "decode_stages.hpp"
#include "flac_host.hpp"

namespace sdsp_dec {

namespace {
std::mutex g_mu;
std::map<int, sdsp_decode_stats> g_stats;
std::map<int, sdsp_audio_decode_stats> g_audio_stats;

// pinned staging for the files' bytes, grow-only, per device (used under the device's lock)
struct Pinned {
    uint8_t* p = nullptr;
    size_t bytes = 0;
    void ensure(size_t n) {
        if (n <= bytes) return;
        if (p) SDSP_HIP_CHECK(hipHostFree(p));
        p = nullptr;
        bytes = 0;
        const size_t want = n + n / 8 + 4096;
        SDSP_HIP_CHECK(hipHostMalloc((void**)&p, want, hipHostMallocDefault));
        note_alloc(want);
        bytes = want;
    }
};
std::map<int, Pinned> g_pinned;
}  // namespace

void Call::set_err(uint64_t i, const std::string& m) {
    status[i] = SDSP_ERR_DECODING;
    std::snprintf(errs + 256 * i, 256, "%s", m.c_str());
    rates[i] = 0;
}

void Call::init_budget() {
    budget = 16e9;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) budget = std::max(1e9, (double)fr * 0.80 / 1.125);
    if (const double gb = test_hooks().hbm_budget_gb.load(); gb > 0.0) budget = std::max(1.0, gb) * 1e9;
    // a wave's work range is at most 64 lanes x 8 channels x 65536 samples x 8 bytes = 256 MiB
    work_budget = std::max(320e6, std::min(budget / 2, 24e9));
    need = work_budget;
}

void Call::reset_outputs() {
    for (uint64_t i = 0; i < n_files; i++) {
        status[i] = SDSP_OK;
        errs[256 * i] = 0;
        offsets[i] = lens[i] = 0;
        rates[i] = 0;
    }
}

DevBuf& Call::upload_bytes() {
    DevBuf& b_bytes = c.buf("flac.bytes");
    const size_t nd = up_idx.size();
    if (!nd) return b_bytes;
    Pinned* pinp;
    {  // other devices' threads may add their entry at the same time; the reference stays valid
        std::lock_guard<std::mutex> pl(g_mu);
        pinp = &g_pinned[device];
    }
    Pinned& pin = *pinp;
    pin.ensure(bytes_total);
    {  // the copy into the staging buffer is memory-bound on one core: a few threads for large batches
        std::atomic<size_t> next{0};
        auto copy = [&]() {
            for (size_t q; (q = next++) < nd;) {
                const uint64_t sz = sizes[up_idx[q]];
                std::memcpy(pin.p + up_base[q], files[up_idx[q]], sz);
                const uint64_t padded = (sz + 15) / 16 * 16 + 16;
                std::memset(pin.p + up_base[q] + sz, 0, padded - sz);
            }
        };
        const size_t nt = bytes_total > (64u << 20) ? std::min<size_t>(8, nd) : 1;
        std::vector<std::thread> pool;
        for (size_t t = 1; t < nt; t++) pool.emplace_back(copy);
        copy();
        for (auto& t : pool) t.join();
    }
    b_bytes.ensure(bytes_total);
    SDSP_HIP_CHECK(hipMemcpyAsync(b_bytes.p, pin.p, bytes_total, hipMemcpyHostToDevice, st));
    return b_bytes;
}

void Call::decode_fallbacks() {
    for (uint64_t i : fallback) {
        std::vector<uint8_t> buf;
        if (files[i]) buf.assign(files[i], files[i] + sizes[i]);
        HostTrack t;
        t.file = i;
        char why[256] = {0};
        uint32_t sr = 0;
        bool ok = false;
        try {
            ok = sdsp_decode_audio_bytes(buf, &t.mono, &sr, why, sizeof why);
        } catch (const std::exception& e) {  // sizes a damaged header declares can make an allocation fail
            std::snprintf(why, sizeof why, "decoding failed: %s", e.what());
        }
        if (!ok) {
            set_err(i, why);
            continue;
        }
        rates[i] = sr;
        host_tracks.push_back(std::move(t));
    }
}

uint64_t Call::place_fallbacks(uint64_t total) {
    for (HostTrack& t : host_tracks) {
        offsets[t.file] = total;
        lens[t.file] = t.mono.size();
        total += t.mono.size();
    }
    return total;
}

void Call::upload_fallbacks(float* out) {
    for (HostTrack& t : host_tracks)
        if (!t.mono.empty())
            SDSP_HIP_CHECK(hipMemcpyAsync(out + offsets[t.file], t.mono.data(), t.mono.size() * 4, hipMemcpyHostToDevice, st));
}

namespace {

// `audio`: the call came through sdsp_decode_audio_batch_device, which also sends Ogg Vorbis to its
// stage; through the lossless entry an Ogg file stays a host fallback
int32_t decode_batch(bool audio, const uint8_t* const* files, const uint64_t* sizes, uint64_t n_files, int32_t device, void* stream,
                     float** d_samples, uint64_t* offsets, uint64_t* lens, uint32_t* rates, int32_t* status, char* errs) {
    const auto t_begin = std::chrono::steady_clock::now();
    sdsp_audio_decode_stats stt{};
    stt.files = n_files;
    DeviceCtx& c = device_ctx(device);
    std::lock_guard<std::mutex> lk(c.mu);
    SDSP_HIP_CHECK(hipSetDevice(device));
    Call k(c, stream ? (hipStream_t)stream : c.stream, device);
    k.files = files, k.sizes = sizes, k.n_files = n_files;
    k.offsets = offsets, k.lens = lens, k.rates = rates, k.status = status, k.errs = errs;
    hipStream_t st = k.st;

    // ---- host plans: which stage takes each file ----
    k.init_budget();
    k.reset_outputs();
    FlacStage flac;
    AlacStage alac;
    PcmStage pcm;
    VorbisStage vorbis;
    std::vector<VorbisPrepared> ogg_plans;  // the audio entry's Ogg files, in file order
    size_t ogg_next = 0;
    if (audio) {
        std::vector<uint64_t> ogg_idx;
        for (uint64_t i = 0; i < n_files; i++)
            if (files[i] && sizes[i] < (1ull << 31) && sdsp_probe_format(files[i], sizes[i]) == SdspFormat::OGG) ogg_idx.push_back(i);
        ogg_plans = VorbisStage::prepare(k, ogg_idx);
    }
    for (uint64_t i = 0; i < n_files; i++) {
        stt.bytes_in += sizes[i];
        if (!files[i] || sizes[i] >= (1ull << 31)) {
            k.fallback.push_back(i);
            continue;
        }
        try {
            switch (sdsp_probe_format(files[i], sizes[i])) {
                case SdspFormat::FLAC: flac.plan(k, i); break;
                case SdspFormat::MP4: alac.plan(k, i, false); break;
                case SdspFormat::CAF:
                    if (sdsp_caf_is_alac(files[i], sizes[i]))
                        alac.plan(k, i, true);
                    else
                        k.fallback.push_back(i);
                    break;
                case SdspFormat::WAV: pcm.plan(k, i, false); break;
                case SdspFormat::AIFF: pcm.plan(k, i, true); break;
                case SdspFormat::OGG:
                    if (audio)
                        vorbis.plan(k, i, ogg_plans[ogg_next++]);
                    else
                        k.fallback.push_back(i);
                    break;
                default: k.fallback.push_back(i);
            }
        } catch (const std::exception& e) {  // sizes a damaged header declares can make an allocation fail
            k.set_err(i, std::string("decoding failed: ") + e.what());
        }
    }

    constexpr int NEV = 10;
    hipEvent_t ev[NEV];
    for (auto& e : ev) SDSP_HIP_CHECK(hipEventCreate(&e));
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < NEV; i++) (void)hipEventDestroy(e[i]);
        }
    } evg{ev};

    // ---- the bytes, then each stage's length-finding kernels ----
    SDSP_HIP_CHECK(hipEventRecord(ev[0], st));
    DevBuf& b_bytes = k.upload_bytes();
    SDSP_HIP_CHECK(hipEventRecord(ev[1], st));
    flac.run(k, b_bytes, ev[7], ev[7], ev[2]);  // its inner phase marks are not reported here
    alac.run(k, b_bytes);
    SDSP_HIP_CHECK(hipEventRecord(ev[3], st));
    vorbis.run(k);
    SDSP_HIP_CHECK(hipEventRecord(ev[8], st));

    // ---- the files no stage took: the host decoder (overlaps the kernels) ----
    k.decode_fallbacks();
    SDSP_HIP_CHECK(hipStreamSynchronize(st));

    // ---- one output allocation: layout, the stages' writes, fallback upload ----
    uint64_t total = flac.place(k, 0);
    total = alac.place(k, total);
    total = pcm.place(k, total);
    total = vorbis.place(k, total);
    total = k.place_fallbacks(total);
    stt.flac_files = flac.device_files;
    stt.alac_files = alac.device_files;
    stt.pcm_files = pcm.device_files;
    stt.vorbis_files = vorbis.device_files;
    stt.vorbis_packets = vorbis.packets;
    stt.vorbis_packets_zeroed = vorbis.packets_zeroed;
    stt.device_files = stt.flac_files + stt.alac_files + stt.pcm_files + stt.vorbis_files;
    stt.host_fallback_files = k.host_tracks.size();
    stt.alac_packets = alac.packets;
    stt.alac_packets_decoded = alac.packets_decoded;
    stt.alac_packets_skipped = alac.packets_skipped;
    for (uint64_t i = 0; i < n_files; i++) stt.error_files += status[i] != SDSP_OK;
    stt.samples_out = total;
    float* out = nullptr;  // the caller's: not one of the engine's grow-only buffers
    SDSP_HIP_CHECK(hipMalloc((void**)&out, std::max<uint64_t>(total, 1) * 4));
    try {
        SDSP_HIP_CHECK(hipEventRecord(ev[4], st));
        flac.write(k, out);
        alac.write(k, out);
        SDSP_HIP_CHECK(hipEventRecord(ev[5], st));
        pcm.write(k, b_bytes, out);
        SDSP_HIP_CHECK(hipEventRecord(ev[6], st));
        vorbis.write(k, out);
        SDSP_HIP_CHECK(hipEventRecord(ev[9], st));
        k.upload_fallbacks(out);
        SDSP_HIP_CHECK(hipStreamSynchronize(st));
    } catch (...) {
        (void)hipFree(out);
        throw;
    }
    *d_samples = out;

    float ms = 0;
    SDSP_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    stt.upload_ms = ms;
    SDSP_HIP_CHECK(hipEventElapsedTime(&ms, ev[1], ev[2]));
    stt.flac_ms = ms;  // scan, candidate round trip, frames, chain
    SDSP_HIP_CHECK(hipEventElapsedTime(&ms, ev[2], ev[3]));
    stt.alac_ms = ms;  // frames, offsets
    SDSP_HIP_CHECK(hipEventElapsedTime(&ms, ev[4], ev[5]));
    stt.gather_ms = ms;  // both gathers
    SDSP_HIP_CHECK(hipEventElapsedTime(&ms, ev[5], ev[6]));
    stt.pcm_ms = ms;
    SDSP_HIP_CHECK(hipEventElapsedTime(&ms, ev[3], ev[8]));
    stt.vorbis_ms = ms;  // uploads, packets, imdct
    SDSP_HIP_CHECK(hipEventElapsedTime(&ms, ev[6], ev[9]));
    stt.vorbis_ms += ms;  // overlap-add
    stt.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    std::lock_guard<std::mutex> sl(g_mu);
    if (audio) {
        g_audio_stats[device] = stt;
    } else {  // the lossless entry's struct is the audio one without the Vorbis fields
        sdsp_decode_stats o{};
        o.files = stt.files, o.device_files = stt.device_files, o.host_fallback_files = stt.host_fallback_files;
        o.error_files = stt.error_files, o.flac_files = stt.flac_files, o.alac_files = stt.alac_files, o.pcm_files = stt.pcm_files;
        o.alac_packets = stt.alac_packets, o.alac_packets_decoded = stt.alac_packets_decoded;
        o.alac_packets_skipped = stt.alac_packets_skipped, o.bytes_in = stt.bytes_in, o.samples_out = stt.samples_out;
        o.upload_ms = stt.upload_ms, o.flac_ms = stt.flac_ms, o.alac_ms = stt.alac_ms, o.pcm_ms = stt.pcm_ms;
        o.gather_ms = stt.gather_ms, o.total_ms = stt.total_ms;
        g_stats[device] = o;
    }
    return SDSP_OK;
}

}  // namespace
}  // namespace sdsp_dec

extern "C" {

static int32_t decode_entry(bool audio, const uint8_t* const* files, const uint64_t* sizes, uint64_t n_files, int32_t device,
                            void* stream, float** d_samples, uint64_t* offsets, uint64_t* lens, uint32_t* sample_rates,
                            int32_t* status, char* errs) {
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
        return sdsp_dec::decode_batch(audio, files, sizes, n_files, device, stream, d_samples, offsets, lens, sample_rates, status,
                                      errs);
    } catch (const std::exception& e) {
        return fail_all((std::string("Processing error: ") + e.what()).c_str());
    }
}

int32_t sdsp_decode_batch_device(const uint8_t* const* files, const uint64_t* sizes, uint64_t n_files, int32_t device,
                                 void* stream, float** d_samples, uint64_t* offsets, uint64_t* lens, uint32_t* sample_rates,
                                 int32_t* status, char* errs) {
    return decode_entry(false, files, sizes, n_files, device, stream, d_samples, offsets, lens, sample_rates, status, errs);
}

int32_t sdsp_decode_audio_batch_device(const uint8_t* const* files, const uint64_t* sizes, uint64_t n_files, int32_t device,
                                       void* stream, float** d_samples, uint64_t* offsets, uint64_t* lens, uint32_t* sample_rates,
                                       int32_t* status, char* errs) {
    return decode_entry(true, files, sizes, n_files, device, stream, d_samples, offsets, lens, sample_rates, status, errs);
}

int32_t sdsp_last_audio_decode_stats(int32_t device, sdsp_audio_decode_stats* out) {
    if (!out) return SDSP_ERR_INVALID_INPUT;
    std::lock_guard<std::mutex> sl(sdsp_dec::g_mu);
    auto it = sdsp_dec::g_audio_stats.find(device);
    *out = it == sdsp_dec::g_audio_stats.end() ? sdsp_audio_decode_stats{} : it->second;
    return SDSP_OK;
}

int32_t sdsp_last_decode_stats(int32_t device, sdsp_decode_stats* out) {
    if (!out) return SDSP_ERR_INVALID_INPUT;
    std::lock_guard<std::mutex> sl(sdsp_dec::g_mu);
    auto it = sdsp_dec::g_stats.find(device);
    *out = it == sdsp_dec::g_stats.end() ? sdsp_decode_stats{} : it->second;
    return SDSP_OK;
}

}  // extern "C"
