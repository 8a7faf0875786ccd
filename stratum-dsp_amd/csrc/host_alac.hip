// host_alac.hip — Apple Lossless (ALAC) in CAF and ISO MP4 (.m4a) for the decode front-end.
//
// The reference decodes ALAC through symphonia's ALAC codec and CAF / ISO MP4 readers
// (Cargo.toml:15, features = ["all"]); the examples convert the decoded buffer to mono f32
// (examples/analyze_file.rs:25-180).  ALAC is lossless, so a decoder's output is the encoded
// PCM whatever its internals; this one follows Apple's published ALAC format (ALACSpecificConfig
// magic cookie; per frame the SCE / CPE elements, each compressed with the adaptive Golomb coder
// and the sign-adaptive FIR predictor, or escaped as raw samples; "bytes shifted" low bits; the
// stereo un-mixing; the END tag).  Samples reach the examples' conversion as integers of the
// stream's bit depth: 16 -> s / 32768, 20 and 24 -> s / 2^(bits-1) (S24 / S32 buffers give the
// same f32 values for these depths), 32 -> s / 2^31.  One and two channels (SCE, CPE) are
// decoded; other channel layouts are a decoding error.  Parity with symphonia itself is
// unpinned: tests/alac_enc.py writes the test streams from the same format description.
//
// The packet-level decode is alac_core.hpp, the code the device kernel (k_alac.hip) runs; this file
// holds the container parsing.  A container parse yields a plan (the cookie and the packet table,
// lossless_host.hpp) without decoding: the host decoder decodes the plan's packets one after the
// other, the batch decoder sends the plan to the device.
#include <cstring>
#include <string>
#include <vector>

#include "lossless_host.hpp"

namespace {

namespace ac = alac_core;
using AlacConfig = ac::Config;

uint16_t be16(const uint8_t* p) { return (uint16_t)((p[0] << 8) | p[1]); }
uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
uint64_t be64(const uint8_t* p) { return ((uint64_t)be32(p) << 32) | be32(p + 4); }

bool fail(std::string* err, const std::string& m) {
    *err = m;
    return false;
}

// ALACSpecificConfig (24 bytes), possibly behind 'frma' / 'alac' atom headers (CAF 'kuki')
bool parse_cookie(const uint8_t* p, size_t n, AlacConfig* c, std::string* err) {
    if (n >= 12 && std::memcmp(p + 4, "frma", 4) == 0) p += 12, n -= 12;
    if (n >= 12 && std::memcmp(p + 4, "alac", 4) == 0) p += 12, n -= 12;
    if (n < 24) return fail(err, "malformed ALAC magic cookie");
    c->frame_length = be32(p);
    c->bit_depth = p[5];
    c->pb = p[6];
    c->mb = p[7];
    c->kb = p[8];
    c->channels = p[9];
    c->max_run = be16(p + 10);
    c->sample_rate = be32(p + 20);
    if (c->frame_length == 0 || c->frame_length > (1u << 20)) return fail(err, "unsupported ALAC frame length");
    if (c->bit_depth != 16 && c->bit_depth != 20 && c->bit_depth != 24 && c->bit_depth != 32)
        return fail(err, "unsupported ALAC bit depth " + std::to_string(c->bit_depth));
    if (c->channels < 1 || c->channels > 2) return fail(err, "unsupported ALAC channel count " + std::to_string(c->channels));
    if (c->kb < 1 || c->kb > 14) return fail(err, "malformed ALAC magic cookie");
    return true;
}

// the text of a packet's error code (the examples skip such a packet, so nothing prints it; the
// tools do)
std::string frame_error(int32_t code, int32_t detail) {
    std::string m = ac::err_text(code);
    if (code == ac::UNSUPPORTED_ELEMENT || code == ac::PREDICTION_MODE) m += std::to_string(detail);
    return m;
}

// every packet of the table lies inside the file
bool check_packets(size_t size, const std::vector<std::pair<uint64_t, uint64_t>>& pk, std::string* err) {
    for (const auto& p : pk)
        if (p.first > size || p.second > size - p.first) return fail(err, "ALAC packet outside the file");
    return true;
}

// CAF variable-length integer (pakt table)
bool caf_vlq(const uint8_t* p, size_t n, size_t* pos, uint64_t* v) {
    *v = 0;
    for (int i = 0; i < 10; i++) {
        if (*pos >= n) return false;
        const uint8_t b = p[(*pos)++];
        *v = (*v << 7) | (b & 0x7f);
        if (!(b & 0x80)) return true;
    }
    return false;
}

}  // namespace

// one packet through the core with host buffers; the error text where it fails
bool sdsp_alac_decode_packet(const ac::Config& c, const uint8_t* d, size_t len, std::vector<int32_t>* work,
                             std::vector<float>* slot, uint32_t* n_out, std::string* err) {
    work->resize((size_t)c.channels * c.frame_length);
    slot->resize(c.frame_length);
    int16_t coefs[64];
    int32_t detail = 0;
    const ac::Work w{work->data(), 1, work->size(), c.frame_length};
    const int32_t e = ac::decode_frame(d, len, c, w, ac::Coefs{coefs, 1}, slot->data(), 1, n_out, &detail);
    if (e != ac::OK && err) *err = frame_error(e, detail);
    return e == ac::OK;
}

// packets -> mono; a packet that fails to decode is skipped (the examples skip DecodeError)
void sdsp_alac_decode_plan(const uint8_t* f, const sdsp_alac_plan& plan, std::vector<float>* out, uint32_t* sr) {
    std::vector<int32_t> work;
    std::vector<float> slot;
    out->clear();
    for (const auto& p : plan.packets) {
        uint32_t n = 0;
        std::string why;
        if (sdsp_alac_decode_packet(plan.cfg, f + p.first, (size_t)p.second, &work, &slot, &n, &why))
            out->insert(out->end(), slot.begin(), slot.begin() + n);
    }
    *sr = plan.cfg.sample_rate ? plan.cfg.sample_rate : 44100u;
}

// CAF with format 'alac': desc, kuki (the magic cookie), pakt (packet sizes), data
bool sdsp_alac_plan_caf(const uint8_t* f, size_t fsize, sdsp_alac_plan* plan, std::string* err) {
    AlacConfig& c = plan->cfg;
    plan->packets.clear();
    bool have_cookie = false;
    const uint8_t* pakt = nullptr;
    uint64_t pakt_len = 0;
    uint64_t data_off = 0, data_len = 0;
    bool have_data = false;
    size_t pos = 8;
    while (pos + 12 <= fsize) {
        const uint8_t* ck = f + pos;
        const int64_t slen = (int64_t)be64(ck + 4);
        const uint64_t avail = fsize - (pos + 12);
        const uint64_t body = (slen < 0 || (uint64_t)slen > avail) ? avail : (uint64_t)slen;
        if (std::memcmp(ck, "kuki", 4) == 0) {
            if (!parse_cookie(ck + 12, (size_t)body, &c, err)) return false;
            have_cookie = true;
        } else if (std::memcmp(ck, "pakt", 4) == 0) {
            pakt = ck + 12;
            pakt_len = body;
        } else if (std::memcmp(ck, "data", 4) == 0) {
            if (body < 4) return fail(err, "malformed data chunk");
            data_off = pos + 16;
            data_len = body - 4;
            have_data = true;
        }
        if (slen < 0) break;
        pos += 12 + (uint64_t)slen;
    }
    if (!have_cookie) return fail(err, "missing ALAC magic cookie");
    if (!have_data) return fail(err, "missing data chunk");
    if (!pakt || pakt_len < 24) return fail(err, "missing packet table");
    const uint64_t npk = be64(pakt);
    std::vector<std::pair<uint64_t, uint64_t>>& pk = plan->packets;
    size_t q = 24;
    uint64_t off = data_off;
    for (uint64_t i = 0; i < npk; i++) {
        uint64_t sz;
        if (!caf_vlq(pakt, (size_t)pakt_len, &q, &sz)) return fail(err, "malformed packet table");
        if (off + sz > data_off + data_len) return fail(err, "packet table exceeds the data chunk");
        pk.push_back({off, sz});
        off += sz;
    }
    return check_packets(fsize, pk, err);
}

bool sdsp_decode_caf_alac(const std::vector<uint8_t>& f, std::vector<float>* out, uint32_t* sr, std::string* err) {
    sdsp_alac_plan plan;
    if (!sdsp_alac_plan_caf(f.data(), f.size(), &plan, err)) return false;
    sdsp_alac_decode_plan(f.data(), plan, out, sr);
    return true;
}

namespace {
// ISO BMFF box walk: calls fn(type, body, body_len) for each box in [p, p + n)
template <class Fn>
bool boxes(const uint8_t* p, uint64_t n, Fn fn) {
    uint64_t pos = 0;
    while (pos + 8 <= n) {
        uint64_t sz = be32(p + pos);
        uint64_t hdr = 8;
        if (sz == 1) {
            if (pos + 16 > n) return false;
            sz = be64(p + pos + 8);
            hdr = 16;
        } else if (sz == 0) {
            sz = n - pos;
        }
        if (sz < hdr || pos + sz > n) return false;
        if (!fn(p + pos + 4, p + pos + hdr, sz - hdr)) return false;
        pos += sz;
    }
    return true;
}
}  // namespace

// ISO MP4 / M4A: the first audio track's sample table (stsd 'alac', stsz, stsc, stco / co64)
bool sdsp_alac_plan_mp4(const uint8_t* fdata, size_t fsize, sdsp_alac_plan* plan, std::string* err) {
    plan->packets.clear();
    const uint8_t* moov = nullptr;
    uint64_t moov_n = 0;
    boxes(fdata, fsize, [&](const uint8_t* t, const uint8_t* b, uint64_t n) {
        if (std::memcmp(t, "moov", 4) == 0) moov = b, moov_n = n;
        return true;
    });
    if (!moov) return fail(err, "malformed ISO MP4 file: missing moov box");
    std::string codec;
    bool found = false;
    AlacConfig& c = plan->cfg;
    std::vector<uint32_t> sizes;
    std::vector<uint64_t> chunk_off;
    std::vector<uint32_t> stsc;  // triples: first chunk, samples per chunk, description index
    std::string why;
    boxes(moov, moov_n, [&](const uint8_t* t, const uint8_t* b, uint64_t n) {
        if (found || std::memcmp(t, "trak", 4) != 0) return true;
        const uint8_t* mdia = nullptr;
        uint64_t mdia_n = 0;
        boxes(b, n, [&](const uint8_t* t2, const uint8_t* b2, uint64_t n2) {
            if (std::memcmp(t2, "mdia", 4) == 0) mdia = b2, mdia_n = n2;
            return true;
        });
        if (!mdia) return true;
        bool audio = false;
        const uint8_t* stbl = nullptr;
        uint64_t stbl_n = 0;
        boxes(mdia, mdia_n, [&](const uint8_t* t3, const uint8_t* b3, uint64_t n3) {
            if (std::memcmp(t3, "hdlr", 4) == 0 && n3 >= 12 && std::memcmp(b3 + 8, "soun", 4) == 0) audio = true;
            if (std::memcmp(t3, "minf", 4) == 0)
                boxes(b3, n3, [&](const uint8_t* t4, const uint8_t* b4, uint64_t n4) {
                    if (std::memcmp(t4, "stbl", 4) == 0) stbl = b4, stbl_n = n4;
                    return true;
                });
            return true;
        });
        if (!audio || !stbl) return true;
        found = true;
        boxes(stbl, stbl_n, [&](const uint8_t* t5, const uint8_t* b5, uint64_t n5) {
            if (std::memcmp(t5, "stsd", 4) == 0 && n5 >= 16) {
                // first sample entry: size, format, 6 reserved + data ref index, then the audio
                // sample entry (20 bytes) and its child boxes
                const uint8_t* e = b5 + 8;
                const uint64_t esz = be32(e);
                codec.assign((const char*)e + 4, 4);
                if (codec == "alac" && esz >= 36 && 8 + esz <= n5)
                    boxes(e + 36, esz - 36, [&](const uint8_t* t6, const uint8_t* b6, uint64_t n6) {
                        if (std::memcmp(t6, "alac", 4) == 0 && n6 >= 28)
                            if (!parse_cookie(b6 + 4, (size_t)n6 - 4, &c, &why)) codec = "bad";
                        return true;
                    });
            } else if (std::memcmp(t5, "stsz", 4) == 0 && n5 >= 12) {
                const uint32_t fixed = be32(b5 + 4), cnt = be32(b5 + 8);
                if (fixed)
                    sizes.assign(cnt, fixed);
                else
                    for (uint32_t i = 0; i < cnt && 12 + 4 * (uint64_t)i + 4 <= n5; i++) sizes.push_back(be32(b5 + 12 + 4 * i));
            } else if (std::memcmp(t5, "stco", 4) == 0 && n5 >= 8) {
                const uint32_t cnt = be32(b5 + 4);
                for (uint32_t i = 0; i < cnt && 8 + 4 * (uint64_t)i + 4 <= n5; i++) chunk_off.push_back(be32(b5 + 8 + 4 * i));
            } else if (std::memcmp(t5, "co64", 4) == 0 && n5 >= 8) {
                const uint32_t cnt = be32(b5 + 4);
                for (uint32_t i = 0; i < cnt && 8 + 8 * (uint64_t)i + 8 <= n5; i++) chunk_off.push_back(be64(b5 + 8 + 8 * i));
            } else if (std::memcmp(t5, "stsc", 4) == 0 && n5 >= 8) {
                const uint32_t cnt = be32(b5 + 4);
                for (uint32_t i = 0; i < cnt && 8 + 12 * (uint64_t)i + 12 <= n5; i++)
                    for (int k = 0; k < 3; k++) stsc.push_back(be32(b5 + 8 + 12 * i + 4 * k));
            }
            return true;
        });
        return true;
    });
    if (!found) return fail(err, "ISO MP4 file without an audio track");
    if (codec == "bad") return fail(err, why);
    if (codec == "mp4a") return fail(err, "unsupported codec: AAC (ISO MP4)");
    if (codec != "alac") return fail(err, "unsupported codec: ISO MP4 '" + codec + "'");
    if (stsc.empty() || chunk_off.empty()) return fail(err, "malformed sample table");
    // sample -> (offset, size) through the sample-to-chunk runs
    std::vector<std::pair<uint64_t, uint64_t>>& pk = plan->packets;
    size_t s = 0;
    const size_t runs = stsc.size() / 3;
    for (size_t r = 0; r < runs && s < sizes.size(); r++) {
        const uint64_t first = stsc[3 * r], per = stsc[3 * r + 1];
        const uint64_t last = r + 1 < runs ? stsc[3 * (r + 1)] : (uint64_t)chunk_off.size() + 1;
        if (first < 1 || last < first) return fail(err, "malformed sample table");
        for (uint64_t ch = first; ch < last && ch <= chunk_off.size() && s < sizes.size(); ch++) {
            uint64_t off = chunk_off[(size_t)ch - 1];
            for (uint64_t k = 0; k < per && s < sizes.size(); k++, s++) {
                pk.push_back({off, sizes[s]});
                off += sizes[s];
            }
        }
    }
    return check_packets(fsize, pk, err);
}

bool sdsp_decode_mp4(const std::vector<uint8_t>& f, std::vector<float>* out, uint32_t* sr, std::string* err) {
    sdsp_alac_plan plan;
    if (!sdsp_alac_plan_mp4(f.data(), f.size(), &plan, err)) return false;
    sdsp_alac_decode_plan(f.data(), plan, out, sr);
    return true;
}

// ALAC from a magic cookie and a list of packets (the Matroska A_ALAC track, host_mkv.hip)
bool sdsp_decode_alac_packets(const std::vector<uint8_t>& cookie, const std::vector<std::vector<uint8_t>>& packets,
                              std::vector<float>* out, uint32_t* sr, std::string* err) {
    sdsp_alac_plan plan;
    if (!parse_cookie(cookie.data(), cookie.size(), &plan.cfg, err)) return false;
    std::vector<uint8_t> flat;
    for (const auto& p : packets) {
        plan.packets.push_back({flat.size(), p.size()});
        flat.insert(flat.end(), p.begin(), p.end());
    }
    sdsp_alac_decode_plan(flat.data(), plan, out, sr);
    return true;
}
