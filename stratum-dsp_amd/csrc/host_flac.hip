// host_flac.hip — native FLAC decoder for the decode front-end (sdsp_decode_audio_file).
//
// The reference decodes FLAC with symphonia 0.5 ("all" features, Cargo.toml:15) and converts each
// decoded buffer in its examples (examples/analyze_batch.rs:30-177, analyze_file.rs:25-180).
// symphonia's FLAC decoder delivers AudioBufferRef::S32 with every sample shifted left by
// 32 - bits_per_sample, which the examples turn into `s as f32 / 2147483648.0` (mono) or the
// channel sum from -0.0 divided by `channels as f32`.  Packets that fail to decode are skipped
// (`Err(DecodeError) => continue`), which this decoder mirrors per frame: a frame whose header
// CRC-8 or frame CRC-16 does not match, or whose subframes are malformed, is dropped and the
// scan resumes at the next frame sync code.  The sample rate is STREAMINFO's
// (codec_params.sample_rate, 44100 when absent).
//
// Format (FLAC, RFC 9639): "fLaC", metadata blocks (STREAMINFO first), then frames: a header
// (sync 0x3FFE, block size / sample rate / channel assignment / sample size codes, UTF-8 coded
// frame or sample number, CRC-8), one subframe per channel (CONSTANT, VERBATIM, FIXED order 0-4,
// LPC order 1-32; wasted bits; Rice or escaped residual partitions), zero padding to a byte and a
// CRC-16.  Stereo decorrelation: left/side, side/right, mid/side.  Decoding is integer-exact
// (64-bit prediction sums), so the f32 output depends only on the conversion above.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "flac_core.hpp"
#include "flac_host.hpp"

// The stream-level part, on the host for every path (host decode, CPU phased decode, device batch):
// ID3v2 skip, "fLaC", the metadata blocks and STREAMINFO.  On success *frames is the offset of the
// first frame; on failure *err is the decode error's text.
bool sdsp_flac_parse_stream(const uint8_t* f, size_t n, sdsp_flac_stream* si, size_t* frames, std::string* err) {
    size_t pos = 0;
    if (n >= 10 && std::memcmp(f, "ID3", 3) == 0) {  // an ID3v2 tag ahead of the stream
        const size_t sz = ((size_t)(f[6] & 0x7F) << 21) | ((size_t)(f[7] & 0x7F) << 14) | ((size_t)(f[8] & 0x7F) << 7) |
                          (size_t)(f[9] & 0x7F);
        pos = 10 + sz + ((f[5] & 0x10) ? 10 : 0);
    }
    if (n < pos + 4 || std::memcmp(f + pos, "fLaC", 4) != 0) {
        *err = "not a FLAC stream";
        return false;
    }
    pos += 4;
    *si = sdsp_flac_stream{};
    bool have_si = false, last = false;
    while (!last) {
        if (pos + 4 > n) {
            *err = "truncated FLAC metadata";
            return false;
        }
        last = (f[pos] & 0x80) != 0;
        const int type = f[pos] & 0x7F;
        const size_t len = ((size_t)f[pos + 1] << 16) | ((size_t)f[pos + 2] << 8) | f[pos + 3];
        pos += 4;
        if (pos + len > n) {
            *err = "truncated FLAC metadata block";
            return false;
        }
        if (type == 0) {
            if (len < 34) {
                *err = "malformed STREAMINFO";
                return false;
            }
            flac_core::Bits b(f + pos, len);
            b.get(16);  // min block size
            b.get(16);  // max block size
            b.get(24);  // min frame size
            b.get(24);  // max frame size
            si->rate = (uint32_t)b.get(20);
            si->channels = (int)b.get(3) + 1;
            si->bps = (int)b.get(5) + 1;
            si->total_samples = b.get(36);
            have_si = true;
        }
        pos += len;
    }
    if (!have_si) {
        *err = "missing STREAMINFO";
        return false;
    }
    if (si->bps < 4 || si->bps > 32) {
        *err = "unsupported FLAC bits per sample " + std::to_string(si->bps);
        return false;
    }
    *frames = pos;
    return true;
}

// Decodes a FLAC stream (f) into mono f32 (the reference examples' conversion) and its rate.
bool sdsp_decode_flac(const std::vector<uint8_t>& f, std::vector<float>* out, uint32_t* sr, std::string* err) {
    sdsp_flac_stream si;
    size_t pos = 0;
    if (!sdsp_flac_parse_stream(f.data(), f.size(), &si, &pos, err)) return false;
    std::vector<int64_t> work;
    out->clear();
    const uint8_t* d = f.data();
    const size_t n = f.size();
    while (pos + 2 <= n) {
        uint32_t bs = 0;
        int bps = 0, chc = 0;
        const size_t hl = flac_core::frame_header(d + pos, n - pos, si.bps, &bs, &bps, &chc);
        if (hl == 0) {  // not a frame start: resynchronise one byte later
            pos++;
            continue;
        }
        const size_t need = (size_t)flac_core::channels_of(chc) * bs;
        if (work.size() < need) work.resize(need);
        const flac_core::Work w{work.data(), 1, work.size()};
        size_t end = 0;
        if (!flac_core::decode_frame(d, n, pos, hl, bs, bps, chc, w, &end)) {
            pos++;  // DecodeError: the packet is skipped (analyze_batch.rs `continue`)
            continue;
        }
        const size_t o = out->size();
        out->resize(o + bs);
        flac_core::emit_mono(w, bs, bps, chc, out->data() + o, 1);
        pos = end + 2;
    }
    *sr = si.rate ? si.rate : 44100u;
    return true;
}
