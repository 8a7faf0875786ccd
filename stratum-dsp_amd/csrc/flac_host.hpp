// flac_host.hpp — host-side FLAC entry points shared by the decode front-end and the batch decoder.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

// STREAMINFO as the decoders use it
struct sdsp_flac_stream {
    uint32_t rate = 0;
    int channels = 0, bps = 0;
    uint64_t total_samples = 0;  // 0: unknown
};

bool sdsp_flac_parse_stream(const uint8_t* f, size_t n, sdsp_flac_stream* si, size_t* frames, std::string* err);
bool sdsp_decode_flac(const std::vector<uint8_t>& f, std::vector<float>* out, uint32_t* sr, std::string* err);

// The decode front-end on bytes already in memory (sdsp_decode_audio_file reads the file and calls
// this): false with the reason in err.
bool sdsp_decode_audio_bytes(const std::vector<uint8_t>& buf, std::vector<float>* mono, uint32_t* sr, char* err,
                             uint64_t errlen);
// true when the front-end sends these bytes to the native FLAC decoder ("fLaC", or ID3v2 then "fLaC")
bool sdsp_is_native_flac(const uint8_t* d, size_t n);
