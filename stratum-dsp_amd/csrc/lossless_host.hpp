// lossless_host.hpp — host-side plans of the ALAC and linear-PCM decoders, shared by the decode
// front-end (host_alac.hip, host_formats.hip, host_decode.hip), the batch decoder
// (decode_batch.hip) and the CPU phased decodes (sdsp_debug_alac_decode_phased,
// sdsp_debug_pcm_decode_planned).  A plan is the container parse without the decode: what the
// device receives next to the file's bytes.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "alac_core.hpp"
#include "pcm_core.hpp"

// which decoder the front-end (sdsp_decode_audio_bytes) sends these bytes to, by magic number
enum class SdspFormat { FLAC, AIFF, CAF, OGG, MKV, MP4, MPEG, WAV };
SdspFormat sdsp_probe_format(const uint8_t* d, size_t n);

// ALAC: the magic cookie and the packet table (offset from the start of the file, size)
struct sdsp_alac_plan {
    alac_core::Config cfg;
    std::vector<std::pair<uint64_t, uint64_t>> packets;
};
// true when the front-end sends these CAF bytes to the ALAC decoder (a 'desc' chunk that passes
// the CAF checks and names 'alac'); any other CAF file is the host decoder's
bool sdsp_caf_is_alac(const uint8_t* f, size_t n);
// false with the host decoder's text in err: a missing cookie, moov box or sample table, AAC,
// a packet outside the file
bool sdsp_alac_plan_caf(const uint8_t* f, size_t n, sdsp_alac_plan* plan, std::string* err);
bool sdsp_alac_plan_mp4(const uint8_t* f, size_t n, sdsp_alac_plan* plan, std::string* err);
// one packet through alac_core::decode_frame with host buffers (work: channels x frame_length
// integers, slot: frame_length floats, both resized here); the packet's error text on failure
bool sdsp_alac_decode_packet(const alac_core::Config& c, const uint8_t* d, size_t len, std::vector<int32_t>* work,
                             std::vector<float>* slot, uint32_t* n_out, std::string* err);
// the host decode of a plan: every packet through alac_core::decode_frame, failed packets skipped
void sdsp_alac_decode_plan(const uint8_t* f, const sdsp_alac_plan& plan, std::vector<float>* out, uint32_t* sr);

// linear PCM: sample layout, rate, first byte of the sample data, whole frames in it (clipped to
// the file when a chunk overstates it)
struct sdsp_pcm_plan {
    pcm_core::Layout lay;
    uint32_t rate = 0;
    uint64_t data_off = 0, frames = 0;
};
// 1: planned; 0: not linear PCM (G.711, ADPCM, an unknown tag or compression type: the host
// decoder's, with its own result or text); -1: an error, the host decoder's text in err
int sdsp_pcm_plan_wav(const uint8_t* f, size_t n, sdsp_pcm_plan* plan, std::string* err);
int sdsp_pcm_plan_aiff(const uint8_t* f, size_t n, sdsp_pcm_plan* plan, std::string* err);
// the host conversion of a plan: pcm_core::frame_mono over frames [0, plan.frames)
void sdsp_pcm_convert_plan(const uint8_t* f, const sdsp_pcm_plan& plan, std::vector<float>* out);
