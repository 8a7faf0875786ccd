// vorbis_host.hpp — the host side of the Vorbis decoders (host only): the flattened setup header,
// the per-block-size tables and the plan of one stream, shared by the host decoder
// (host_vorbis.hip), the CPU phased decode (vorbis_phased.hpp) and the Vorbis stage of the batch
// decoder (k_vorbis.hip).  A plan is everything but the decode: the setup tables, the kept audio
// packets back to back, and every packet's block size, window shape and place in the output.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "vorbis_core.hpp"

// the setup header as vorbis_core reads it (owning)
struct sdsp_vorbis_setup {
    int channels = 0;
    uint32_t rate = 0;
    int bs[2] = {0, 0};
    std::vector<vorbis_core::Book> books;
    std::vector<int32_t> trees;
    std::vector<float> vq;
    std::vector<vorbis_core::Floor> floors;
    std::vector<vorbis_core::Residue> residues;
    std::vector<vorbis_core::Mapping> maps;
    std::vector<vorbis_core::Mode> modes;
    vorbis_core::Setup view() const;  // pointers into this object and the inverse-dB table
    uint64_t table_bytes() const {
        return books.size() * sizeof(vorbis_core::Book) + trees.size() * 4 + vq.size() * 4 +
               floors.size() * sizeof(vorbis_core::Floor) + residues.size() * sizeof(vorbis_core::Residue) +
               maps.size() * sizeof(vorbis_core::Mapping) + modes.size() * sizeof(vorbis_core::Mode);
    }
};

// one kept audio packet (the host loop's skips are dropped: empty, not audio, mode out of range)
struct sdsp_vorbis_packet {
    uint64_t off;   // first byte in sdsp_vorbis_plan::bytes
    uint64_t out;   // first output sample (the prefix sum of prev_n/4 + n/4); the first packet: none
    uint32_t size;  // bytes
    uint16_t n, prev_n;  // block size, the previous kept packet's (0: the first packet, no output)
    uint8_t blockflag, prev_long, next_long;
};

struct sdsp_vorbis_plan {
    sdsp_vorbis_setup setup;
    std::vector<uint8_t> bytes;  // the kept packets back to back
    std::vector<sdsp_vorbis_packet> packets;
    uint64_t total = 0;   // samples the packets produce
    uint64_t frames = 0;  // after the cut at the last page's granule position
};

// the tables of block size N, host-computed once with the decoder's own expressions; the reference
// returned stays valid (one entry per power of two, never freed)
struct sdsp_vorbis_tables {
    int N = 0;
    std::vector<vorbis_core::cd> pre, post, tw;
    std::vector<float> up, dn;
    vorbis_core::BlockTables view() const { return {pre.data(), post.data(), tw.data(), up.data(), dn.data()}; }
};
const sdsp_vorbis_tables& sdsp_vorbis_block_tables(int N);
const float* sdsp_vorbis_inv_db();  // 256 entries

// the first logical stream's packets of an Ogg file and the last granule position (-1: none);
// pages whose CRC fails are dropped
void sdsp_ogg_demux(const uint8_t* f, size_t n, std::vector<std::vector<uint8_t>>* packets, int64_t* last_granule);
// 1: planned; 0: an Ogg stream that is not Vorbis (the host decoder's, with its own result or
// text); -1: an error, the host decoder's text in err
int sdsp_vorbis_plan_ogg(const uint8_t* f, size_t n, sdsp_vorbis_plan* plan, std::string* err);
// the headers (packets 0 and 2) and the audio packets' first bits; false with the host's text
bool sdsp_vorbis_plan_packets(const std::vector<std::vector<uint8_t>>& packets, int64_t last_granule, sdsp_vorbis_plan* plan,
                              std::string* err);
// the host decode of a plan: packet by packet through vorbis_core
void sdsp_vorbis_decode_plan(const sdsp_vorbis_plan& plan, std::vector<float>* out);
