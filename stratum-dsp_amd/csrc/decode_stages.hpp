// decode_stages.hpp — the stages of the batched device decode (host only).  One call
// (sdsp_decode_batch_device and sdsp_decode_audio_batch_device in decode_batch.hip,
// sdsp_decode_flac_batch_device in k_flac.hip) is a
// Call plus one stage per format it sends to the device; every stage has the same four steps:
//   plan    on the host: parse the container, commit HBM from the call's budget, reserve the file's
//           place in the bytes buffer (or leave the file to the host decoder, or set its error);
//   run     after the bytes are uploaded: the kernels that find each file's length (PCM and Vorbis
//           know it from the plan: Vorbis decodes here, into its own buffers);
//   place   after the stream is synchronised: offsets and lengths of the stage's files in the
//           call's one output buffer;
//   write   the kernels that write the tracks at those offsets.
// The stages share the context's grow-only buffers (the bytes, the work range), so a second
// identical call allocates nothing.
#pragma once

#include <string>
#include <vector>

#include "../../include/stratum_hip.h"
#include "lossless_host.hpp"
#include "sdsp_runtime.hpp"
#include "vorbis_host.hpp"

namespace sdsp_dec {

using namespace sdsp;

struct HostTrack {  // a file decoded by the host decoder (fallback)
    uint64_t file;
    std::vector<float> mono;
};

struct Call {
    DeviceCtx& c;
    hipStream_t st;
    int device;
    const uint8_t* const* files;
    const uint64_t* sizes;
    uint64_t n_files;
    uint64_t *offsets, *lens;
    uint32_t* rates;
    int32_t* status;
    char* errs;
    double budget = 0, work_budget = 0, need = 0;  // HBM: the call's budget, the work range's share, committed so far
    std::vector<uint64_t> up_idx, up_base;         // files whose bytes go to the device, their first byte there
    uint64_t bytes_total = 0;
    std::vector<uint64_t> fallback;  // files for the host decoder
    std::vector<HostTrack> host_tracks;

    Call(DeviceCtx& ctx, hipStream_t s, int dev) : c(ctx), st(s), device(dev) {}
    // every file starts 16-byte aligned with at least 16 zero bytes after its last one
    uint64_t reserve_bytes(uint64_t i) {
        const uint64_t base = bytes_total;
        bytes_total += (sizes[i] + 15) / 16 * 16 + 16;
        up_idx.push_back(i);
        up_base.push_back(base);
        return base;
    }
    void set_err(uint64_t i, const std::string& m);  // SDSP_ERR_DECODING with the host's text
    void init_budget();
    void reset_outputs();                 // status OK, empty text, zero offsets / lengths / rates
    DevBuf& upload_bytes();               // pinned staging, then one copy into the shared bytes buffer
    void decode_fallbacks();              // the host decoder over `fallback` (overlaps queued kernels)
    uint64_t place_fallbacks(uint64_t total);
    void upload_fallbacks(float* out);
};

template <class T>
inline void upload(DevBuf& b, const std::vector<T>& v, hipStream_t st) {
    b.ensure(std::max<size_t>(v.size(), 1) * sizeof(T));
    if (!v.empty()) SDSP_HIP_CHECK(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
}

// ---- FLAC (k_flac.hip): scan, frames, chain | gather ----
struct FlacFile {
    uint64_t base;       // first byte in the bytes buffer (16-byte aligned)
    uint64_t cand_base;  // first slot of the file's range in the scan's candidate list
    uint32_t size;       // bytes (< 2^31)
    uint32_t start;      // first byte of the frame region
    uint32_t cand_cap;   // slots in that range
    int32_t si_bps;      // STREAMINFO's bits per sample
};

struct FlacStage {
    std::vector<FlacFile> ft;       // device files
    std::vector<uint64_t> dev_idx;  // their indices in the call
    uint64_t cand_total = 0;
    double est_sum = 0;  // HBM plan() committed for these files
    std::vector<uint64_t> f_len, f_outoff;
    std::vector<uint32_t> f_acc, f_rej;
    std::vector<uint8_t> on_device;
    uint64_t nc = 0;  // sorted candidates
    uint64_t device_files = 0, frames_accepted = 0, frames_rejected = 0;

    void plan(Call& k, uint64_t i);
    // records ev_scan after the scan, ev_frames after the frame decode, ev_chain after the chain;
    // synchronises the stream once (the candidate round trip), not at its end
    void run(Call& k, DevBuf& bytes, hipEvent_t ev_scan, hipEvent_t ev_frames, hipEvent_t ev_chain);
    uint64_t place(Call& k, uint64_t total);
    void write(Call& k, float* out);
};

// ---- ALAC (k_alac.hip): frames, offsets | gather ----
struct AlacFile {
    uint64_t base;  // first byte in the bytes buffer
    alac_core::Config cfg;
};

constexpr uint32_t ALAC_MAX_FRAME_LENGTH = 16384;  // longer frames: the host decoder (it takes 2^20)

struct AlacStage {
    std::vector<AlacFile> ft;
    std::vector<uint64_t> dev_idx;
    std::vector<uint32_t> p_file, p_off, p_size;
    std::vector<uint64_t> p_slot, f_first;
    std::vector<uint32_t> f_npk;
    uint64_t scratch_total = 0;
    std::vector<uint64_t> f_len, f_outoff;
    std::vector<uint32_t> f_dec, f_skip;
    uint64_t device_files = 0, packets = 0, packets_decoded = 0, packets_skipped = 0;

    void plan(Call& k, uint64_t i, bool caf);
    void run(Call& k, DevBuf& bytes);
    uint64_t place(Call& k, uint64_t total);
    void write(Call& k, float* out);
};

// ---- linear PCM (k_pcm.hip): | convert and mix ----
struct PcmFile {
    uint64_t src;  // first sample byte in the bytes buffer
    uint64_t dst;  // first sample of the track in the output
    uint64_t frames;
    pcm_core::Layout lay;
};

constexpr int PCM_MAX_CHANNELS = 8;  // wider files: the host decoder

struct PcmStage {
    std::vector<PcmFile> ft;
    std::vector<uint64_t> dev_idx;
    uint64_t device_files = 0;

    void plan(Call& k, uint64_t i, bool aiff);
    uint64_t place(Call& k, uint64_t total);
    void write(Call& k, DevBuf& bytes, float* out);
};

// ---- Ogg Vorbis (k_vorbis.hip): packets, imdct | ola ----
// Lengths follow from the packets' first bits, so the host plan knows them: run() only decodes.
struct VorbisFile {
    uint64_t tree_off, vq_off;  // the file's first entry in the stage's flat setup tables
    uint32_t book_off, floor_off, res_off, map_off, mode_off;
    int32_t channels, bs0, bs1, nmodes;
    uint32_t p_first, p_count;  // its kept packets
    uint64_t out_off, frames;   // the track in the output (place()), its length after the granule cut
};

struct VorbisPacket {
    uint64_t off;   // first byte in the stage's packet bytes
    uint64_t spec;  // first float of its spectra (channels x n/2); its windowed blocks start at 2 * spec
    uint64_t out;   // first output sample in the file's track
    uint32_t size, file;
    uint16_t n, prev_n;
    uint8_t blockflag, prev_long, next_long;
};

// a file whose flattened setup (decode trees, VQ values, floors, residues, mappings, modes) is larger
// goes to the host decoder; libvorbis setups are a few hundred KiB
constexpr uint64_t VORBIS_MAX_TABLE_BYTES = 64ull << 20;

// the host plan of one file, made ahead of the stage's serial plan() on the call's worker threads
struct VorbisPrepared {
    int r = 0;  // sdsp_vorbis_plan_ogg's result, or -2: the plan threw (`why` holds the text)
    std::string why;
    sdsp_vorbis_plan pl;
};

struct VorbisStage {
    std::vector<VorbisFile> ft;
    std::vector<uint64_t> dev_idx;
    std::vector<VorbisPacket> pk;
    std::vector<std::vector<uint8_t>> file_bytes;  // per device file: its kept packets, back to back
    std::vector<uint64_t> file_byte0;              // their first byte in the device's packet bytes
    uint64_t bytes_total = 0;
    std::vector<vorbis_core::Book> books;
    std::vector<int32_t> trees;
    std::vector<float> vq;
    std::vector<vorbis_core::Floor> floors;
    std::vector<vorbis_core::Residue> residues;
    std::vector<vorbis_core::Mapping> maps;
    std::vector<vorbis_core::Mode> modes;
    uint64_t spec_total = 0;
    std::vector<uint32_t> p_zero;  // per packet: a floor decode failed and the block is silent
    // upload sources of run(), kept until the call's stream is synchronised
    std::vector<double> tab;
    std::vector<uint2> items;  // (packet, channel) by block size
    std::vector<uint64_t> wave_off;
    std::vector<uint32_t> wave_cap;
    uint64_t device_files = 0, packets = 0, packets_zeroed = 0;

    // the Ogg files' host plans (demultiplex, headers, every packet's first bits), several at a time
    static std::vector<VorbisPrepared> prepare(const Call& k, const std::vector<uint64_t>& idx);
    void plan(Call& k, uint64_t i, VorbisPrepared& pre);
    void run(Call& k);
    uint64_t place(Call& k, uint64_t total);
    void write(Call& k, float* out);
};

}  // namespace sdsp_dec
