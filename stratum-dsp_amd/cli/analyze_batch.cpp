// analyze_batch — batch front-end with the reference example's interface and output
// (examples/analyze_batch.rs): files are decoded on host worker threads (--jobs, default
// CPU threads - 1), then analysed on the GPUs as one batch per sample rate through
// sdsp_analyze_batch (sharded over --devices, default every visible GPU), each result scored
// with compute_confidence, printed in input order as text lines or JSONL, with the same
// summary on stderr.
//
//
// --gpu-decode (opt-in; the output is the same): the workers only read the files' bytes.  The files
// are cut into chunks under a device-memory bound, and each chunk is decoded on a GPU by
// sdsp_decode_audio_batch_device (native FLAC, ALAC in M4A / CAF, WAV and AIFF PCM, Ogg Vorbis by HIP
// kernels; every other format by the host decoder inside that call) and analysed from the device buffer
// (sdsp_analyze_batch_device), one call per sample rate the decoder returned: no host PCM exists
// and host memory holds the files' bytes only.  Chunks go round-robin over the devices of
// --devices, one host thread per device.
//
// --overview N / --overview-frames K (opt-in; JSONL only): each line's object gets one more member
// at its end, "overview": the track's overview envelope (include/stratum_hip.h, sdsp_overview) in N
// columns, or one column per K frames, with the low / mid / high bands split at 250 Hz and 4 kHz.
// The analysis then runs through sdsp_analyze_batch_device_overview: from the decoder's device
// buffer with --gpu-decode, otherwise from the decoded tracks uploaded to the first device of
// --devices, one call per sample rate and at most 512 tracks or 8 GB.
//
// --key-timeline SEC[:OVERLAP[:MINCONF]] (opt-in; JSONL only): each line's object gets a
// "key_timeline" member (include/stratum_hip.h, sdsp_key_timeline): the key of every SEC-second
// segment (overlapping by OVERLAP seconds, default SEC / 4), the primary key and the key changes
// whose confidence exceeds MINCONF (default -1: every change; 0.2 is the reference's constant), with
// key names.  It runs through sdsp_analyze_batch_device_with like --overview and combines with it
// in one analysis.
// --levels [LIST] (opt-in; JSONL only): each line's object gets a "levels" member
// (include/stratum_hip.h, sdsp_levels): the loudness metadata of each normalisation method in LIST
// (out of peak,rms,loudness,silence; all four without a list), -inf as null, and the silence
// regions as [start_sample, end_sample, seconds].  It combines with the other two in one analysis.
// --tempo-map[=LIST] (opt-in; JSONL only): each line's object gets a "tempo_map" member
// (include/stratum_hip.h, sdsp_tempo_map): the tempo segments with what the Bayesian refinement did in
// each, the time signature with its three scores, and the consensus onsets (LIST out of
// segments,onsets; both without a list).  It combines with the other three in one analysis.
// --sections[=CELL_SEC[:K[:GAP[:EWEIGHT[:MINSTRENGTH]]]]] (opt-in; JSONL only): each line's object gets a
// "sections" member (include/stratum_hip.h, sdsp_sections): the sections between the structural
// boundaries with their energies, each start snapped to a downbeat within one cell, and the novelty
// and energy curves per cell.  Defaults 0.5 s, K 16, GAP 8, EWEIGHT 1, MINSTRENGTH 0.5.
//
//   analyze_batch [--jobs N] [--devices MASK] [--json] [--gpu-decode] [--overview N | --overview-frames K]
//                 [--key-timeline SEC[:OVERLAP[:MINCONF]]] [--levels [LIST]] [--tempo-map[=LIST]]
//                 [--sections[=CELL_SEC[:K[:GAP[:EWEIGHT[:MINSTRENGTH]]]]]] [--loudness[=true-peak,curves]]
//                 <file1> <file2> ...
// --loudness[=LIST] (opt-in; JSONL only): each line's object gets a "loudness" member
// (include/stratum_hip.h, sdsp_r128): BS.1770 integrated loudness, loudness range, maximum momentary
// and short-term loudness and the sample peak; LIST out of true-peak (the 4x true peak) and curves
// (the momentary and short-term mean squares per block).
// --fingerprint[=CELL_SEC[:MAX_OFFSET_SEC[:MAX_BER]]] (opt-in; JSONL only): each line's object gets a
// "fingerprint" member (include/stratum_hip.h, sdsp_fingerprint): the counts and the words as hex, and
// one last line {"duplicates":[{"a":path,"b":path,"offset_seconds":..,"ber":..}, ...]} lists the pairs
// of files within MAX_BER at their best alignment within MAX_OFFSET_SEC (sample s of a meets sample
// s + offset_seconds * rate of b).  Files are compared within one analysis call: the files of one
// sample rate, at most 512 at a time.  Defaults 0.125 s, 2 s, 0.30; at least 32 words must overlap.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <functional>
#include <mutex>
#include <thread>

#include "cli_common.hpp"

using namespace sdsp_cli;

namespace {

struct Item {
    std::string path;
    std::vector<float> samples;
    std::vector<uint8_t> bytes;  // --gpu-decode: the file's bytes
    uint64_t need = 0;           // --gpu-decode: device bytes the file's decode is expected to take
    bool device = false;         // --gpu-decode: the file goes through sdsp_decode_audio_batch_device
    uint32_t sr = 0;
    bool decoded = false;
    std::string error;
    bool ok = false;
    float bpm = 0, bpm_conf = 0, key_conf = 0, ms = 0;
    std::string key;
    int8_t tr[4] = {-1, -1, -1, -1};
    std::string overview;  // --overview: the "overview" member's value
    std::string timeline;  // --key-timeline: the "key_timeline" member's value
    std::string levels;    // --levels: the "levels" member's value
    std::string tempo_map; // --tempo-map: the "tempo_map" member's value
    std::string sections;  // --sections: the "sections" member's value
    std::string loudness;  // --loudness: the "loudness" member's value
    std::string fingerprint;  // --fingerprint: the "fingerprint" member's value
};
// --fingerprint: one matched pair of files (positions in the argument list, a < b)
struct Dup {
    size_t a, b;
    double offset_seconds;
    float ber;
};

// floats so that an f32 round-trips
void json_floats(std::string& s, const char* name, const float* v, uint64_t n) {
    s += std::string(",\"") + name + "\":[";
    char b[32];
    for (uint64_t i = 0; i < n; i++) {
        std::snprintf(b, sizeof b, i ? ",%.9g" : "%.9g", (double)v[i]);
        s += b;
    }
    s += "]";
}
std::string overview_json(const sdsp_overview& o) {
    char b[320];
    std::snprintf(b, sizeof b,
                  "{\"n_columns\":%llu,\"n_frames\":%llu,\"first_sample\":%llu,\"n_samples\":%llu,\"frame_size\":%u,"
                  "\"hop_size\":%u,\"band_bins\":[%u,%u],\"status\":%d",
                  (unsigned long long)o.n_columns, (unsigned long long)o.n_frames, (unsigned long long)o.first_sample,
                  (unsigned long long)o.n_samples, o.frame_size, o.hop_size, o.band_bins[0], o.band_bins[1], o.status);
    std::string s = b;
    json_floats(s, "smin", o.smin, o.n_columns);
    json_floats(s, "smax", o.smax, o.n_columns);
    json_floats(s, "low", o.low, o.n_columns);
    json_floats(s, "mid", o.mid, o.n_columns);
    json_floats(s, "high", o.high, o.n_columns);
    return s + "}";
}

std::string key_index_name(int32_t key) {
    char b[8] = "";
    if (key >= 0 && key < 24) sdsp_key_name(key / 12, (uint32_t)(key % 12), b, sizeof b);
    return b;
}
std::string key_timeline_json(const sdsp_key_timeline& t) {
    char b[512];
    std::snprintf(b, sizeof b,
                  "{\"n_segments\":%llu,\"n_changes\":%llu,\"n_frames\":%llu,\"first_sample\":%llu,"
                  "\"segment_frames\":%u,\"hop_frames\":%u,\"frame_size\":%u,\"hop_size\":%u,\"status\":%d,"
                  "\"primary_key\":%d,\"primary_key_name\":%s,\"primary_confidence\":%.9g,\"primary_count\":%llu,"
                  "\"segments\":[",
                  (unsigned long long)t.n_segments, (unsigned long long)t.n_changes, (unsigned long long)t.n_frames,
                  (unsigned long long)t.first_sample, t.segment_frames, t.hop_frames, t.frame_size, t.hop_size, t.status,
                  t.primary_key, json_str(key_index_name(t.primary_key)).c_str(), (double)t.primary_confidence,
                  (unsigned long long)t.primary_count);
    std::string s = b;
    for (uint64_t i = 0; i < t.n_segments; i++) {
        const sdsp_key_segment& g = t.segments[i];
        std::snprintf(b, sizeof b,
                      "%s{\"start_frame\":%llu,\"timestamp\":%.9g,\"key\":%d,\"key_name\":%s,\"confidence\":%.9g,"
                      "\"clarity\":%.9g,\"top_keys\":[%d,%d,%d],\"top_scores\":[%.9g,%.9g,%.9g]}",
                      i ? "," : "", (unsigned long long)g.start_frame, (double)g.timestamp, g.key,
                      json_str(key_index_name(g.key)).c_str(), (double)g.confidence, (double)g.clarity, g.top_keys[0],
                      g.top_keys[1], g.top_keys[2], (double)g.top_scores[0], (double)g.top_scores[1],
                      (double)g.top_scores[2]);
        s += b;
    }
    s += "],\"changes\":[";
    for (uint64_t i = 0; i < t.n_changes; i++) {
        const sdsp_key_change& c = t.changes[i];
        std::snprintf(b, sizeof b,
                      "%s{\"segment\":%llu,\"timestamp\":%.9g,\"from_key\":%d,\"from_key_name\":%s,\"to_key\":%d,"
                      "\"to_key_name\":%s,\"confidence\":%.9g}",
                      i ? "," : "", (unsigned long long)c.segment, (double)c.timestamp, c.from_key,
                      json_str(key_index_name(c.from_key)).c_str(), c.to_key, json_str(key_index_name(c.to_key)).c_str(),
                      (double)c.confidence);
        s += b;
    }
    return s + "]}";
}

// an f32 so that it round-trips; -inf (a level of silence, no LUFS value) as null
std::string json_db(float v) {
    if (!std::isfinite(v)) return "null";
    char b[32];
    std::snprintf(b, sizeof b, "%.9g", (double)v);
    return b;
}
std::string levels_json(const sdsp_levels& l) {
    static const char* const names[3] = {"peak", "rms", "loudness"};
    char b[256];
    std::snprintf(b, sizeof b,
                  "{\"status\":%d,\"n_samples\":%llu,\"applied_gain\":%.9g,\"trim_start\":%llu,\"trim_end\":%llu,"
                  "\"frame_size\":%u,\"threshold_db\":%.9g",
                  l.status, (unsigned long long)l.n_samples, (double)l.applied_gain, (unsigned long long)l.trim_start,
                  (unsigned long long)l.trim_end, l.frame_size, (double)l.threshold_db);
    std::string s = b;
    for (int m = 0; m < 3; m++) {
        const sdsp_loudness& e = l.method[m];
        if (!e.measured) continue;
        s += std::string(",\"") + names[m] + "\":{\"status\":" + std::to_string(e.status) +
             ",\"measured_lufs\":" + (e.has_lufs ? json_db(e.measured_lufs) : std::string("null")) +
             ",\"peak_db\":" + json_db(e.peak_db) + ",\"rms_db\":" + json_db(e.rms_db) + ",\"gain_db\":" +
             json_db(e.gain_db) + ",\"gain\":" + json_db(e.gain) + "}";
    }
    s += ",\"n_regions\":" + std::to_string((unsigned long long)l.n_regions) + ",\"regions\":[";
    for (uint64_t i = 0; i < l.n_regions; i++) {
        std::snprintf(b, sizeof b, "%s[%llu,%llu,%.9g]", i ? "," : "", (unsigned long long)l.regions[i].start_sample,
                      (unsigned long long)l.regions[i].end_sample, (double)l.regions[i].duration_seconds);
        s += b;
    }
    return s + "]}";
}

std::string tempo_map_json(const sdsp_tempo_map& m) {
    char b[512];
    std::snprintf(b, sizeof b,
                  "{\"status\":%d,\"has_grid\":%d,\"has_variation\":%d,\"refined\":%d,\"nominal_bpm\":%s,"
                  "\"nominal_confidence\":%s,\"hmm_beats\":%u,\"beats_per_bar\":%u,\"time_signature_confidence\":%.9g,"
                  "\"time_signature_scored\":%d,\"time_signature_scores\":[%.9g,%.9g,%.9g],\"first_sample\":%llu",
                  m.status, m.has_grid, m.has_variation, m.refined, json_db(m.nominal_bpm).c_str(),
                  json_db(m.nominal_confidence).c_str(), m.hmm_beats, m.beats_per_bar, (double)m.time_signature_confidence,
                  m.time_signature_scored, (double)m.time_signature_scores[0], (double)m.time_signature_scores[1],
                  (double)m.time_signature_scores[2], (unsigned long long)m.first_sample);
    std::string s = b;
    // a segment: [start, end, bpm, confidence, is_variable, updated, n_onsets, updated_bpm, updated_confidence, n_beats]
    s += ",\"n_segments\":" + std::to_string((unsigned long long)m.n_segments) + ",\"segments\":[";
    for (uint64_t i = 0; i < m.n_segments; i++) {
        const sdsp_tempo_segment& e = m.segments[i];
        std::snprintf(b, sizeof b, "%s[%.9g,%.9g,%.9g,%.9g,%u,%u,%u,%.9g,%.9g,%u]", i ? "," : "", (double)e.start_time,
                      (double)e.end_time, (double)e.bpm, (double)e.confidence, (unsigned)e.is_variable, (unsigned)e.updated,
                      e.n_onsets, (double)e.updated_bpm, (double)e.updated_confidence, e.n_beats);
        s += b;
    }
    s += "],\"n_onsets\":" + std::to_string((unsigned long long)m.n_onsets) + ",\"onsets\":[";
    for (uint64_t i = 0; i < m.n_onsets; i++) {
        std::snprintf(b, sizeof b, i ? ",%u" : "%u", m.onsets[i]);
        s += b;
    }
    return s + "]}";
}

std::string sections_json(const sdsp_sections& m) {
    char b[512];
    std::snprintf(b, sizeof b,
                  "{\"status\":%d,\"n_cells\":%llu,\"cell_samples\":%llu,\"first_sample\":%llu,\"gmax\":%.9g,"
                  "\"nmax\":%.9g",
                  m.status, (unsigned long long)m.n_cells, (unsigned long long)m.cell_samples,
                  (unsigned long long)m.first_sample, (double)m.gmax, (double)m.nmax);
    std::string s = b;
    // a section: [start_cell, end_cell, start_time, end_time, strength, mean_energy, relative_energy, snapped_time, downbeat]
    s += ",\"n_sections\":" + std::to_string((unsigned long long)m.n_sections) + ",\"sections\":[";
    for (uint64_t i = 0; i < m.n_sections; i++) {
        const sdsp_section& e = m.sections[i];
        std::snprintf(b, sizeof b, "%s[%llu,%llu,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%d]", i ? "," : "",
                      (unsigned long long)e.start_cell, (unsigned long long)e.end_cell, (double)e.start_time,
                      (double)e.end_time, (double)e.strength, (double)e.mean_energy, (double)e.relative_energy,
                      (double)e.snapped_time, e.downbeat);
        s += b;
    }
    s += "],\"n_curve\":" + std::to_string((unsigned long long)m.n_curve);
    for (int k = 0; k < 2; k++) {
        s += k ? "],\"energy\":[" : ",\"novelty\":[";
        const float* v = k ? m.energy : m.novelty;
        for (uint64_t i = 0; i < m.n_curve; i++) {
            std::snprintf(b, sizeof b, i ? ",%.9g" : "%.9g", (double)v[i]);
            s += b;
        }
    }
    return s + "]}";
}

std::string r128_json(const sdsp_r128& m, uint32_t what) {
    char b[768];
    std::snprintf(b, sizeof b,
                  "{\"status\":%d,\"n_samples\":%llu,\"step_samples\":%u,\"n_steps\":%llu,\"integrated_lufs\":%s,"
                  "\"range_lu\":%s,\"range_low_lufs\":%s,\"range_high_lufs\":%s,\"max_momentary_lufs\":%s,"
                  "\"max_short_term_lufs\":%s,\"sample_peak\":%.9g,\"sample_peak_db\":%s,\"n_momentary\":%llu,"
                  "\"n_short_term\":%llu,\"n_gated_momentary\":%llu,\"n_gated_short_term\":%llu",
                  m.status, (unsigned long long)m.n_samples, m.step_samples, (unsigned long long)m.n_steps,
                  m.has_integrated ? json_db(m.integrated_lufs).c_str() : "null",
                  m.has_range ? json_db(m.range_lu).c_str() : "null", m.has_range ? json_db(m.range_low_lufs).c_str() : "null",
                  m.has_range ? json_db(m.range_high_lufs).c_str() : "null", json_db(m.max_momentary_lufs).c_str(),
                  json_db(m.max_short_term_lufs).c_str(), (double)m.sample_peak, json_db(m.sample_peak_db).c_str(),
                  (unsigned long long)m.n_momentary, (unsigned long long)m.n_short_term,
                  (unsigned long long)m.n_gated_momentary, (unsigned long long)m.n_gated_short_term);
    std::string s = b;
    if (what & SDSP_R128_TRUE_PEAK) {
        std::snprintf(b, sizeof b, ",\"true_peak\":%.9g,\"true_peak_dbtp\":%s", (double)m.true_peak,
                      json_db(m.true_peak_dbtp).c_str());
        s += b;
    }
    if (what & SDSP_R128_CURVES) {
        for (int k = 0; k < 2; k++) {
            s += k ? "],\"short_term\":[" : ",\"momentary\":[";
            const float* v = k ? m.short_term : m.momentary;
            const uint64_t n = v ? (k ? m.n_short_term : m.n_momentary) : 0;
            for (uint64_t i = 0; i < n; i++) {
                std::snprintf(b, sizeof b, i ? ",%.9g" : "%.9g", (double)v[i]);
                s += b;
            }
        }
        s += "]";
    }
    return s + "}";
}

std::string fingerprint_json(const sdsp_fingerprint& m) {
    char b[256];
    std::snprintf(b, sizeof b,
                  "{\"status\":%d,\"n_cells\":%llu,\"n_words\":%llu,\"cell_samples\":%llu,\"first_sample\":%llu,"
                  "\"n_matches\":%llu,\"words\":\"",
                  m.status, (unsigned long long)m.n_cells, (unsigned long long)m.n_words, (unsigned long long)m.cell_samples,
                  (unsigned long long)m.first_sample, (unsigned long long)m.n_matches);
    std::string s = b;
    for (uint64_t i = 0; m.words && i < m.n_words; i++) {  // six hex digits per 24-bit word
        std::snprintf(b, sizeof b, "%06x", m.words[i]);
        s += b;
    }
    return s + "\"}";
}

// percentile as the example computes it: sort, index round((len-1) * p)
float percentile(std::vector<float> xs, float p) {
    std::sort(xs.begin(), xs.end());
    const float q = p < 0.0f ? 0.0f : p > 1.0f ? 1.0f : p;
    size_t idx = (size_t)std::roundf((float)(xs.size() - 1) * q);  // f32::round: half away from zero
    if (idx >= xs.size()) idx = xs.size() - 1;
    return xs[idx];
}

// "fLaC", or an ID3v2 tag then "fLaC": the files the decode front-end sends to its native FLAC decoder
bool native_flac(const std::vector<uint8_t>& b) {
    auto at = [&](size_t o) { return b.size() >= o + 4 && std::memcmp(b.data() + o, "fLaC", 4) == 0; };
    if (at(0)) return true;
    if (b.size() < 10 || std::memcmp(b.data(), "ID3", 3) != 0) return false;
    return at(10 + (((size_t)(b[6] & 0x7f) << 21) | ((size_t)(b[7] & 0x7f) << 14) | ((size_t)(b[8] & 0x7f) << 7) |
                    (size_t)(b[9] & 0x7f)));
}

// STREAMINFO's sample rate and sample count for grouping and sizing (0, 0 when the metadata cannot be
// walked: the decoder then reports the file's error)
void flac_streaminfo(const std::vector<uint8_t>& b, uint32_t* rate, uint64_t* total) {
    *rate = 0;
    *total = 0;
    size_t pos = 0;
    if (b.size() >= 10 && std::memcmp(b.data(), "ID3", 3) == 0)
        pos = 10 + (((size_t)(b[6] & 0x7f) << 21) | ((size_t)(b[7] & 0x7f) << 14) | ((size_t)(b[8] & 0x7f) << 7) |
                    (size_t)(b[9] & 0x7f)) + ((b[5] & 0x10) ? 10 : 0);
    pos += 4;
    for (bool last = false; !last;) {
        if (pos + 4 > b.size()) return;
        last = (b[pos] & 0x80) != 0;
        const int type = b[pos] & 0x7F;
        const size_t len = ((size_t)b[pos + 1] << 16) | ((size_t)b[pos + 2] << 8) | b[pos + 3];
        pos += 4;
        if (pos + len > b.size()) return;
        if (type == 0 && len >= 34) {
            const uint8_t* p = b.data() + pos;
            *rate = ((uint32_t)p[10] << 12) | ((uint32_t)p[11] << 4) | (p[12] >> 4);
            *total = ((uint64_t)(p[13] & 0x0F) << 32) | ((uint64_t)p[14] << 24) | ((uint64_t)p[15] << 16) |
                     ((uint64_t)p[16] << 8) | p[17];
            return;
        }
        pos += len;
    }
}

// Device bytes a file's decode is expected to take, from the container's declared length: FLAC by
// STREAMINFO's sample count; RIFF/WAVE and AIFF hold at most one frame per byte (bytes + 4-byte
// samples); a compressed or unknown container a generous multiple of its bytes, as a FLAC file of
// unknown length.  The decoder checks its own budget again.
uint64_t expected_need(const std::vector<uint8_t>& b) {
    const uint64_t n = b.size();
    if (native_flac(b)) {
        uint32_t rate = 0;
        uint64_t total = 0;
        flac_streaminfo(b, &rate, &total);
        return 3 * n + 8 * (total ? total : 16 * n);
    }
    const bool riff = n >= 12 && std::memcmp(b.data(), "RIFF", 4) == 0;
    const bool form = n >= 12 && std::memcmp(b.data(), "FORM", 4) == 0;
    if (riff || form) return 5 * n;
    return 3 * n + 8 * 16 * n;
}

struct Chunk {
    std::vector<size_t> idx;
};

}  // namespace

int main(int argc, char** argv) {
    Args a(argv + 1, argv + argc);
    bool json = false, gpu_decode = false;
    uint64_t jobs = 0;
    uint32_t devices = 0;
    sdsp_overview_request ovreq{0, 0, 250.0f, 4000.0f};
    bool overview = false;
    sdsp_key_timeline_request ktreq{0.0f, 0.0f, 0, 0, -1.0f};
    bool timeline = false;
    sdsp_levels_request lvreq{SDSP_LEVELS_PEAK | SDSP_LEVELS_RMS | SDSP_LEVELS_LOUDNESS | SDSP_LEVELS_SILENCE_MAP};
    bool levels = false;
    sdsp_tempo_map_request tmreq{SDSP_TEMPO_MAP_SEGMENTS | SDSP_TEMPO_MAP_ONSETS};
    bool tempo_map = false;
    sdsp_sections_request screq{};
    screq.what = SDSP_SECTIONS_LIST | SDSP_SECTIONS_CURVE;
    screq.cell_seconds = 0.5f;
    screq.kernel_cells = 16;
    screq.min_gap_cells = 8;
    screq.energy_weight = 1.0f;
    screq.min_strength = 0.5f;
    bool sections = false;
    sdsp_r128_request r128req{SDSP_R128_LOUDNESS};
    bool loudness = false;
    sdsp_fingerprint_request fpreq{};
    fpreq.what = SDSP_FP_WORDS | SDSP_FP_MATCH;
    fpreq.cell_seconds = 0.125f;
    fpreq.max_offset_words = 16;
    fpreq.min_overlap_words = 32;
    fpreq.max_ber = 0.30f;
    bool fingerprint = false;
    std::vector<std::string> paths;
    for (size_t i = 0; i < a.size(); i++) {
        const std::string& s = a[i];
        if (s == "--json") {
            json = true;
        } else if (s == "--gpu-decode") {
            gpu_decode = true;
        } else if (s == "--jobs" || s == "--devices") {
            uint64_t v;
            if (i + 1 >= a.size() || !parse_usize_str(a[i + 1], &v)) {
                std::fprintf(stderr, "Error: %s requires a value\n", s.c_str());
                return 1;
            }
            if (s == "--jobs")
                jobs = std::max<uint64_t>(1, v);
            else
                devices = (uint32_t)v;
            i++;
        } else if (s == "--overview" || s == "--overview-frames") {
            uint64_t v;
            if (i + 1 >= a.size() || !parse_usize_str(a[i + 1], &v) || v == 0 || v > 0xFFFFFFFFull) {
                std::fprintf(stderr, "Error: %s requires a count of at least 1\n", s.c_str());
                return 1;
            }
            (s == "--overview" ? ovreq.columns : ovreq.frames_per_column) = (uint32_t)v;
            overview = true;
            i++;
        } else if (s == "--key-timeline") {
            // SEC[:OVERLAP[:MINCONF]]
            float v[3] = {0.0f, 0.0f, -1.0f};
            int n = 0;
            bool good = i + 1 < a.size() && !a[i + 1].empty();
            for (size_t p0 = 0; good && n < 3;) {
                const std::string& w = a[i + 1];
                const size_t p1 = std::min(w.find(':', p0), w.size());
                char* end = nullptr;
                const std::string part = w.substr(p0, p1 - p0);
                v[n] = std::strtof(part.c_str(), &end);
                good = !part.empty() && end && *end == 0;
                n++;
                if (p1 == w.size()) break;
                p0 = p1 + 1;
                if (n == 3) good = false;  // a fourth part
            }
            if (!good || !(v[0] > 0.0f)) {
                std::fprintf(stderr, "Error: --key-timeline requires SEC[:OVERLAP[:MINCONF]] with SEC > 0\n");
                return 1;
            }
            ktreq.segment_seconds = v[0];
            ktreq.overlap_seconds = n >= 2 ? v[1] : v[0] / 4.0f;
            ktreq.min_change_confidence = v[2];
            timeline = true;
            i++;
        } else if (s == "--levels") {
            // an optional list out of peak,rms,loudness,silence (the next argument when it is such a list)
            levels = true;
            uint32_t what = 0;
            bool list = i + 1 < a.size() && !a[i + 1].empty();
            for (size_t p0 = 0; list;) {
                const std::string& w = a[i + 1];
                const size_t p1 = std::min(w.find(',', p0), w.size());
                const std::string part = w.substr(p0, p1 - p0);
                if (part == "peak") what |= SDSP_LEVELS_PEAK;
                else if (part == "rms") what |= SDSP_LEVELS_RMS;
                else if (part == "loudness") what |= SDSP_LEVELS_LOUDNESS;
                else if (part == "silence") what |= SDSP_LEVELS_SILENCE_MAP;
                else list = false;
                if (p1 == w.size()) break;
                p0 = p1 + 1;
            }
            if (list) {
                lvreq.what = what;
                i++;
            }
        } else if (s == "--tempo-map" || s.rfind("--tempo-map=", 0) == 0) {
            tempo_map = true;
            if (s.size() > 11) {  // =LIST out of segments,onsets
                const std::string w = s.substr(12);
                uint32_t what = 0;
                bool good = !w.empty();
                for (size_t p0 = 0; good;) {
                    const size_t p1 = std::min(w.find(',', p0), w.size());
                    const std::string part = w.substr(p0, p1 - p0);
                    if (part == "segments") what |= SDSP_TEMPO_MAP_SEGMENTS;
                    else if (part == "onsets") what |= SDSP_TEMPO_MAP_ONSETS;
                    else good = false;
                    if (p1 == w.size()) break;
                    p0 = p1 + 1;
                }
                if (!good) {
                    std::fprintf(stderr, "Error: --tempo-map=LIST takes a list out of segments,onsets\n");
                    return 1;
                }
                tmreq.what = what;
            }
        } else if (s == "--sections" || s.rfind("--sections=", 0) == 0) {
            sections = true;
            if (s.size() > 10) {  // =CELL_SEC[:K[:GAP[:EWEIGHT[:MINSTRENGTH]]]]
                const std::string w = s.substr(11);
                double v[5] = {0.5, 16, 8, 1.0, 0.5};
                int n = 0;
                bool good = !w.empty();
                for (size_t p0 = 0; good;) {
                    const size_t p1 = std::min(w.find(':', p0), w.size());
                    char* end = nullptr;
                    const std::string part = w.substr(p0, p1 - p0);
                    good = n < 5 && !part.empty();
                    if (good) v[n] = std::strtod(part.c_str(), &end), good = end && *end == 0;
                    n++;
                    if (p1 == w.size()) break;
                    p0 = p1 + 1;
                }
                if (!good || !(v[0] > 0.0) || !(v[1] >= 1.0 && v[1] <= 64.0) || v[1] != (double)(uint32_t)v[1] ||
                    !(v[2] >= 0.0 && v[2] < 2147483648.0) || v[2] != (double)(uint32_t)v[2] || !(v[3] >= 0.0) || !(v[4] >= 0.0)) {
                    std::fprintf(stderr,
                                 "Error: --sections takes CELL_SEC[:K[:GAP[:EWEIGHT[:MINSTRENGTH]]]] with CELL_SEC > 0, K in "
                                 "[1, 64], whole GAP >= 0, EWEIGHT and MINSTRENGTH >= 0\n");
                    return 1;
                }
                screq.cell_seconds = (float)v[0];
                screq.kernel_cells = (uint32_t)v[1];
                screq.min_gap_cells = (uint32_t)v[2];
                screq.energy_weight = (float)v[3];
                screq.min_strength = (float)v[4];
            }
            screq.snap_seconds = screq.cell_seconds;
        } else if (s == "--fingerprint" || s.rfind("--fingerprint=", 0) == 0) {
            fingerprint = true;
            if (s.size() > 13) {  // =CELL_SEC[:MAX_OFFSET_SEC[:MAX_BER]]
                const std::string w = s.substr(14);
                double v[3] = {0.125, 2.0, 0.30};
                int n = 0;
                bool good = !w.empty();
                for (size_t p0 = 0; good;) {
                    const size_t p1 = std::min(w.find(':', p0), w.size());
                    char* end = nullptr;
                    const std::string part = w.substr(p0, p1 - p0);
                    good = n < 3 && !part.empty();
                    if (good) v[n] = std::strtod(part.c_str(), &end), good = end && *end == 0;
                    n++;
                    if (p1 == w.size()) break;
                    p0 = p1 + 1;
                }
                const double words = good && v[0] > 0.0 ? std::floor(v[1] / v[0] + 0.5) : -1.0;
                if (!good || !(v[0] > 0.0) || !(v[1] >= 0.0) || !(words >= 0.0 && words <= 255.0) || !(v[2] >= 0.0 && v[2] <= 1.0)) {
                    std::fprintf(stderr,
                                 "Error: --fingerprint takes CELL_SEC[:MAX_OFFSET_SEC[:MAX_BER]] with CELL_SEC > 0, "
                                 "MAX_OFFSET_SEC >= 0 and at most 255 cells, MAX_BER in [0, 1]\n");
                    return 1;
                }
                fpreq.cell_seconds = (float)v[0];
                fpreq.max_offset_words = (uint32_t)words;
                fpreq.max_ber = (float)v[2];
            }
        } else if (s == "--loudness" || s.rfind("--loudness=", 0) == 0) {
            loudness = true;
            if (s.size() > 10) {  // =LIST
                const std::string w = s.substr(11);
                bool good = !w.empty();
                for (size_t p0 = 0; good;) {
                    const size_t p1 = std::min(w.find(',', p0), w.size());
                    const std::string part = w.substr(p0, p1 - p0);
                    if (part == "true-peak")
                        r128req.what |= SDSP_R128_TRUE_PEAK;
                    else if (part == "curves")
                        r128req.what |= SDSP_R128_CURVES;
                    else
                        good = false;
                    if (p1 == w.size()) break;
                    p0 = p1 + 1;
                }
                if (!good) {
                    std::fprintf(stderr, "Error: --loudness=LIST takes a list out of true-peak,curves\n");
                    return 1;
                }
            }
        } else if (s == "--help" || s == "-h") {
            std::fprintf(stderr,
                         "Usage: analyze_batch [--jobs N] [--devices MASK] [--json] [--gpu-decode] [--overview N | "
                         "--overview-frames K] [--key-timeline SEC[:OVERLAP[:MINCONF]]] [--levels [LIST]] [--tempo-map[=LIST]] "
                         "[--sections[=CELL_SEC[:K[:GAP[:EWEIGHT[:MINSTRENGTH]]]]]] [--loudness[=LIST]] "
                         "[--fingerprint[=CELL_SEC[:MAX_OFFSET_SEC[:MAX_BER]]]] <file1> <file2> ...\n\n"
                         "--jobs N        Decode workers (default: CPU-1)\n"
                         "--devices MASK  GPU bitmask (default: all visible GPUs)\n"
                         "--json          Emit one JSON object per line (JSONL)\n"
                         "--gpu-decode    Decode on the GPUs: FLAC, ALAC (M4A / CAF), WAV, AIFF and Ogg Vorbis by kernels (same output)\n"
                         "--overview N    With --json: add each track's overview envelope in N columns (\"overview\")\n"
                         "--overview-frames K  ... or in one column per K analysis frames\n"
                         "--key-timeline SEC[:OVERLAP[:MINCONF]]  With --json: add each track's key per SEC-second segment,\n"
                         "                primary key and key changes (\"key_timeline\"); OVERLAP defaults to SEC/4, MINCONF\n"
                         "                to -1 (every change; 0.2 is the reference's threshold)\n"
                         "--levels [LIST] With --json: add each track's loudness metadata and silence regions (\"levels\");\n"
                         "                LIST out of peak,rms,loudness,silence (default: all four)\n"
                         "--tempo-map[=LIST]  With --json: add each track's tempo segments, time signature and consensus\n"
                         "                onsets (\"tempo_map\"); LIST out of segments,onsets (default: both)\n"
                         "--sections[=CELL_SEC[:K[:GAP[:EWEIGHT[:MINSTRENGTH]]]]]  With --json: add each track's sections between\n"
                         "                structural boundaries with their energies, and the novelty and energy curves\n"
                         "                (\"sections\"); defaults 0.5:16:8:1:0.5, starts snapped to downbeats within a cell\n"
                         "--loudness[=LIST]  With --json: add each track's BS.1770 integrated loudness, loudness range, maximum\n"
                         "                momentary and short-term loudness and sample peak (\"loudness\"); LIST out of\n"
                         "                true-peak,curves adds the 4x true peak and the per-block mean squares\n"
                         "--fingerprint[=CELL_SEC[:MAX_OFFSET_SEC[:MAX_BER]]]  With --json: add each track's chroma fingerprint\n"
                         "                (\"fingerprint\": counts and the words as hex) and one last line \"duplicates\" with the\n"
                         "                pairs of files that are the same recording; defaults 0.125:2:0.30\n");
            return 0;
        } else {
            paths.push_back(s);
        }
    }
    if (ovreq.columns && ovreq.frames_per_column) {
        std::fprintf(stderr, "Error: --overview and --overview-frames exclude each other\n");
        return 1;
    }
    if (overview && !json) std::fprintf(stderr, "Note: --overview / --overview-frames add to the --json lines only\n");
    if (timeline && !json) std::fprintf(stderr, "Note: --key-timeline adds to the --json lines only\n");
    if (levels && !json) std::fprintf(stderr, "Note: --levels adds to the --json lines only\n");
    if (tempo_map && !json) std::fprintf(stderr, "Note: --tempo-map adds to the --json lines only\n");
    if (sections && !json) std::fprintf(stderr, "Note: --sections adds to the --json lines only\n");
    if (loudness && !json) std::fprintf(stderr, "Note: --loudness adds to the --json lines only\n");
    if (fingerprint && !json) std::fprintf(stderr, "Note: --fingerprint adds to the --json lines only\n");
    if (paths.empty()) {
        std::fprintf(stderr, "ERROR: Provide at least one audio file path. Use --help for usage.\n");
        return 2;
    }
    if (jobs == 0) {
        const unsigned hc = std::max(1u, std::thread::hardware_concurrency());
        jobs = std::max<uint64_t>(1, hc - 1);
    }
    if (devices == 0) {
        const int nd = sdsp_device_count();
        devices = nd >= 32 ? 0xffffffffu : nd > 0 ? ((1u << nd) - 1) : 1u;
    }
    std::fprintf(stderr, "Batch: %zu files, jobs=%llu\n", paths.size(), (unsigned long long)jobs);
    const auto t0 = std::chrono::steady_clock::now();

    std::vector<Item> items(paths.size());
    std::atomic<size_t> next{0};
    auto worker = [&]() {
        for (size_t i; (i = next++) < items.size();) {
            Item& it = items[i];
            it.path = paths[i];
            if (gpu_decode) {  // read the bytes; the decode happens on the device threads below
                FILE* fp = std::fopen(it.path.c_str(), "rb");
                if (!fp) {
                    it.error = "decode failed: cannot open " + it.path;
                    continue;
                }
                uint8_t chunk[1 << 16];
                size_t got;
                while ((got = std::fread(chunk, 1, sizeof chunk, fp)) > 0) it.bytes.insert(it.bytes.end(), chunk, chunk + got);
                std::fclose(fp);
                it.need = expected_need(it.bytes);
                it.device = true;
                continue;
            }
            float* p = nullptr;
            uint64_t n = 0;
            char err[512];
            if (sdsp_decode_audio_file(it.path.c_str(), &p, &n, &it.sr, err, sizeof err) != 0) {
                it.error = std::string("decode failed: ") + err;
                continue;
            }
            it.samples.assign(p, p + n);
            sdsp_free_samples(p);
            it.decoded = true;
        }
    };
    std::vector<std::thread> pool;
    for (uint64_t j = 0; j < std::min<uint64_t>(jobs, items.size()); j++) pool.emplace_back(worker);
    for (auto& t : pool) t.join();

    sdsp_config cfg;
    sdsp_config_default(&cfg);
    auto take = [&r128req](Item& it, const sdsp_result& r, const sdsp_overview* ov = nullptr,
                           const sdsp_key_timeline* kt = nullptr, const sdsp_levels* lv = nullptr,
                           const sdsp_tempo_map* tm = nullptr, const sdsp_sections* sc = nullptr,
                           const sdsp_r128* ld = nullptr, const sdsp_fingerprint* fp = nullptr) {
        if (fp) it.fingerprint = fingerprint_json(*fp);
        if (ov) it.overview = overview_json(*ov);
        if (kt) it.timeline = key_timeline_json(*kt);
        if (lv) it.levels = levels_json(*lv);
        if (tm) it.tempo_map = tempo_map_json(*tm);
        if (sc) it.sections = sections_json(*sc);
        if (ld) it.loudness = r128_json(*ld, r128req.what);
        if (r.status != 0) {
            it.error = std::string("analysis failed: ") + r.error_message;
            return;
        }
        sdsp_confidence c;
        sdsp_compute_confidence(&r, &c);
        it.ok = true;
        it.bpm = r.bpm;
        it.bpm_conf = c.bpm_confidence;
        it.key = key_name(r);
        it.key_conf = c.key_confidence;
        it.ms = r.processing_time_ms;
        it.tr[0] = r.tempogram_multi_res_triggered;
        it.tr[1] = r.tempogram_multi_res_used;
        it.tr[2] = r.tempogram_percussive_triggered;
        it.tr[3] = r.tempogram_percussive_used;
    };

    // the optional requests of one analysis call over n tracks, and their outputs
    struct Requests {
        std::vector<sdsp_overview> ovs;
        std::vector<sdsp_key_timeline> kts;
        std::vector<sdsp_levels> lvs;
        std::vector<sdsp_tempo_map> tms;
        std::vector<sdsp_sections> scs;
        std::vector<sdsp_r128> lds;
        std::vector<sdsp_fingerprint> fps;
        sdsp_fingerprint_matches fpm{};
        sdsp_request_set_ext3 ext3{};
    };
    auto requests = [&](size_t n) {
        Requests q;
        q.ovs.resize(overview ? n : 0);  // (zeroed; without a request: the plain entry)
        q.kts.resize(timeline ? n : 0);
        q.lvs.resize(levels ? n : 0);
        q.tms.resize(tempo_map ? n : 0);
        q.scs.resize(sections ? n : 0);
        q.lds.resize(loudness ? n : 0);
        q.fps.resize(fingerprint ? n : 0);
        return q;
    };
    auto request_set = [&](Requests& q) {
        sdsp_request_set_ext2& ext2 = q.ext3.base;
        sdsp_request_set& set = ext2.base.base;
        set.struct_size = (uint32_t)sizeof(q.ext3);
        if (overview) set.ov_req = &ovreq, set.overviews = q.ovs.data();
        if (timeline) set.kt_req = &ktreq, set.timelines = q.kts.data();
        if (levels) set.lv_req = &lvreq, set.levels = q.lvs.data();
        if (tempo_map) set.tm_req = &tmreq, set.tempo_maps = q.tms.data();
        if (sections) ext2.base.sc_req = &screq, ext2.base.sections = q.scs.data();
        if (loudness) ext2.r128_req = &r128req, ext2.r128 = q.lds.data();
        if (fingerprint) q.ext3.fp_req = &fpreq, q.ext3.fingerprints = q.fps.data(), q.ext3.fp_matches = &q.fpm;
        return &set;
    };
    auto take_requests = [&](Item& it, const sdsp_result& r, Requests& q, size_t j) {
        take(it, r, overview ? &q.ovs[j] : nullptr, timeline ? &q.kts[j] : nullptr, levels ? &q.lvs[j] : nullptr,
             tempo_map ? &q.tms[j] : nullptr, sections ? &q.scs[j] : nullptr, loudness ? &q.lds[j] : nullptr,
             fingerprint ? &q.fps[j] : nullptr);
        if (overview) sdsp_overview_free(&q.ovs[j]);
        if (timeline) sdsp_key_timeline_free(&q.kts[j]);
        if (levels) sdsp_levels_free(&q.lvs[j]);
        if (tempo_map) sdsp_tempo_map_free(&q.tms[j]);
        if (sections) sdsp_sections_free(&q.scs[j]);
        if (loudness) sdsp_r128_free(&q.lds[j]);
        if (fingerprint) sdsp_fingerprint_free(&q.fps[j]);
    };
    // --fingerprint: the matches of one analysis call into the run's list; at(j): the file of the call's track j
    std::vector<Dup> dups;
    std::mutex dups_mu;
    auto take_matches = [&](Requests& q, uint32_t sr, const std::function<size_t(size_t)>& at) {
        if (!fingerprint) return;
        std::lock_guard<std::mutex> lk(dups_mu);
        for (uint64_t k = 0; q.fpm.matches && k < q.fpm.n_matches; k++) {
            const sdsp_fingerprint_match& m = q.fpm.matches[k];
            Dup d{at((size_t)m.a), at((size_t)m.b), (double)m.offset_samples / (double)std::max<uint32_t>(sr, 1), m.ber};
            if (d.a > d.b) std::swap(d.a, d.b), d.offset_seconds = -d.offset_seconds;
            dups.push_back(d);
        }
        sdsp_fingerprint_matches_free(&q.fpm);
    };

    if (gpu_decode) {
        // chunks of at most 8 GiB of expected device memory and 512 files each (the decoder checks
        // its own budget again and sends what does not fit to the host decoder)
        std::vector<Chunk> chunks;
        uint64_t acc = 0;
        for (size_t i = 0; i < items.size(); i++) {
            if (!items[i].device) continue;
            if (chunks.empty() || chunks.back().idx.size() >= 512 || (acc && acc + items[i].need > (8ull << 30))) {
                chunks.push_back(Chunk{});
                acc = 0;
            }
            chunks.back().idx.push_back(i);
            acc += items[i].need;
        }
        std::vector<int> devs;
        for (int d = 0; d < 32; d++)
            if (devices & (1u << d)) devs.push_back(d);
        auto run_chunk = [&](const Chunk& ch, int dev) {
            const size_t n = ch.idx.size();
            std::vector<const uint8_t*> ptrs(n);
            std::vector<uint64_t> sizes(n), offs(n), lens(n);
            std::vector<uint32_t> rates(n);
            std::vector<int32_t> status(n);
            std::vector<char> errs(256 * n);
            for (size_t k = 0; k < n; k++) {
                ptrs[k] = items[ch.idx[k]].bytes.data();
                sizes[k] = items[ch.idx[k]].bytes.size();
            }
            float* d_samples = nullptr;
            const int32_t rc = sdsp_decode_audio_batch_device(ptrs.data(), sizes.data(), n, dev, nullptr, &d_samples, offs.data(),
                                                              lens.data(), rates.data(), status.data(), errs.data());
            std::map<uint32_t, std::vector<size_t>> by_rate;  // the decoded files, by the rate the decoder returned
            for (size_t k = 0; k < n; k++) {
                Item& it = items[ch.idx[k]];
                std::vector<uint8_t>().swap(it.bytes);
                if (rc != 0 || status[k] != 0) {
                    it.error = std::string("decode failed: ") + (errs.data() + 256 * k);
                    continue;
                }
                it.decoded = true;
                it.sr = rates[k];
                by_rate[rates[k]].push_back(k);
            }
            for (auto& kv : by_rate) {
                const std::vector<size_t>& okk = kv.second;
                std::vector<uint64_t> o2, l2;
                for (size_t k : okk) {
                    o2.push_back(offs[k]);
                    l2.push_back(lens[k]);
                }
                std::vector<sdsp_result> outs(okk.size());
                Requests q = requests(okk.size());
                (void)sdsp_analyze_batch_device_with(d_samples, o2.data(), l2.data(), okk.size(), kv.first, &cfg, dev, nullptr,
                                                     SDSP_STAGES_FULL, outs.data(), request_set(q));
                for (size_t j = 0; j < okk.size(); j++) {
                    take_requests(items[ch.idx[okk[j]]], outs[j], q, j);
                    sdsp_result_free(&outs[j]);
                }
                take_matches(q, kv.first, [&](size_t j) { return ch.idx[okk[j]]; });
            }
            if (d_samples) sdsp_device_free(dev, d_samples);
        };
        std::vector<std::thread> dev_threads;
        for (size_t w = 0; w < devs.size(); w++)
            dev_threads.emplace_back([&, w]() {
                for (size_t c = w; c < chunks.size(); c += devs.size()) run_chunk(chunks[c], devs[w]);
            });
        for (auto& t : dev_threads) t.join();
    }

    std::map<uint32_t, std::vector<size_t>> by_sr;
    for (size_t i = 0; i < items.size(); i++)
        if (items[i].decoded && !items[i].device) by_sr[items[i].sr].push_back(i);
    for (auto& kv : by_sr) {
        const std::vector<size_t>& idx = kv.second;
        std::vector<const float*> ptrs;
        std::vector<uint64_t> lens;
        for (size_t i : idx) {
            ptrs.push_back(items[i].samples.data());
            lens.push_back(items[i].samples.size());
        }
        if (overview || timeline || levels || tempo_map || sections || loudness || fingerprint) {
            // the requests entry reads device-resident tracks: upload each group to the first device of
            // the mask in parts of at most 512 tracks or 2 Gi samples
            int dev = 0;
            while (dev < 31 && !(devices & (1u << dev))) dev++;
            for (size_t k0 = 0; k0 < idx.size();) {
                size_t k1 = k0;
                uint64_t tot = 0;
                while (k1 < idx.size() && k1 - k0 < 512 && (k1 == k0 || tot + lens[k1] <= ((uint64_t)2 << 30))) tot += lens[k1++];
                const size_t n = k1 - k0;
                std::vector<uint64_t> off(n);
                std::vector<sdsp_result> outs(n);
                Requests q = requests(n);
                void* d = nullptr;
                bool up = sdsp_device_malloc(dev, std::max<uint64_t>(tot, 1) * sizeof(float), &d) == 0;
                uint64_t o = 0;
                for (size_t k = k0; k < k1 && up; k++) {
                    off[k - k0] = o;
                    if (lens[k]) up = sdsp_memcpy_h2d(dev, (float*)d + o, ptrs[k], lens[k] * sizeof(float)) == 0;
                    o += lens[k];
                }
                if (up)
                    (void)sdsp_analyze_batch_device_with((const float*)d, off.data(), lens.data() + k0, n, kv.first, &cfg, dev,
                                                         nullptr, SDSP_STAGES_FULL, outs.data(), request_set(q));
                for (size_t k = k0; k < k1; k++) {
                    if (up) {
                        take_requests(items[idx[k]], outs[k - k0], q, k - k0);
                        sdsp_result_free(&outs[k - k0]);
                    } else {
                        items[idx[k]].error = "analysis failed: Processing error: device upload failed";
                    }
                }
                if (up) take_matches(q, kv.first, [&](size_t j) { return idx[k0 + j]; });
                if (d) sdsp_device_free(dev, d);
                k0 = k1;
            }
            continue;
        }
        std::vector<sdsp_result> outs(idx.size());
        // a non-OK return means some chunk failed; every track's own status says which (tracks the
        // library did not analyse carry an error status), so each result is read and freed
        (void)sdsp_analyze_batch(ptrs.data(), lens.data(), idx.size(), kv.first, &cfg, devices, outs.data());
        for (size_t k = 0; k < idx.size(); k++) {
            take(items[idx[k]], outs[k]);
            sdsp_result_free(&outs[k]);
        }
    }

    for (size_t i = 0; i < items.size(); i++) {
        const Item& o = items[i];
        if (json) {
            if (o.ok)
                std::printf("{\"file\":%s,\"bpm\":%.2f,\"bpm_confidence\":%.4f,\"key\":%s,\"key_confidence\":%.4f,"
                            "\"processing_time_ms\":%.2f,\"tempogram_multi_res_triggered\":%s,"
                            "\"tempogram_multi_res_used\":%s,\"tempogram_percussive_triggered\":%s,"
                            "\"tempogram_percussive_used\":%s",
                            json_str(o.path).c_str(), (double)o.bpm, (double)o.bpm_conf, json_str(o.key).c_str(),
                            (double)o.key_conf, (double)o.ms, tri(o.tr[0]), tri(o.tr[1]), tri(o.tr[2]), tri(o.tr[3]));
            else
                std::printf("{\"file\":%s,\"error\":%s", json_str(o.path).c_str(),
                            json_str(o.error.empty() ? "unknown error" : o.error).c_str());
            if (!o.overview.empty()) {
                std::fputs(",\"overview\":", stdout);
                std::fputs(o.overview.c_str(), stdout);
            }
            if (!o.timeline.empty()) {
                std::fputs(",\"key_timeline\":", stdout);
                std::fputs(o.timeline.c_str(), stdout);
            }
            if (!o.levels.empty()) {
                std::fputs(",\"levels\":", stdout);
                std::fputs(o.levels.c_str(), stdout);
            }
            if (!o.tempo_map.empty()) {
                std::fputs(",\"tempo_map\":", stdout);
                std::fputs(o.tempo_map.c_str(), stdout);
            }
            if (!o.sections.empty()) {
                std::fputs(",\"sections\":", stdout);
                std::fputs(o.sections.c_str(), stdout);
            }
            if (!o.loudness.empty()) {
                std::fputs(",\"loudness\":", stdout);
                std::fputs(o.loudness.c_str(), stdout);
            }
            if (!o.fingerprint.empty()) {
                std::fputs(",\"fingerprint\":", stdout);
                std::fputs(o.fingerprint.c_str(), stdout);
            }
            std::fputs("}\n", stdout);
        } else {
            if (o.ok)
                std::printf("[%zu/%zu] %s: BPM=%.2f (conf=%.3f) Key=%s (conf=%.3f) time=%.2fms\n", i + 1, items.size(),
                            o.path.c_str(), (double)o.bpm, (double)o.bpm_conf, o.key.c_str(), (double)o.key_conf,
                            (double)o.ms);
            else
                std::printf("[%zu/%zu] %s: ERROR: %s\n", i + 1, items.size(), o.path.c_str(),
                            o.error.empty() ? "unknown error" : o.error.c_str());
        }
    }
    if (fingerprint && json) {
        std::sort(dups.begin(), dups.end(), [](const Dup& x, const Dup& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
        std::fputs("{\"duplicates\":[", stdout);
        for (size_t k = 0; k < dups.size(); k++)
            std::printf("%s{\"a\":%s,\"b\":%s,\"offset_seconds\":%.9g,\"ber\":%.9g}", k ? "," : "",
                        json_str(items[dups[k].a].path).c_str(), json_str(items[dups[k].b].path).c_str(), dups[k].offset_seconds,
                        (double)dups[k].ber);
        std::fputs("]}\n", stdout);
    }
    std::vector<float> ok_times;
    for (const Item& o : items)
        if (o.ok) ok_times.push_back(o.ms);
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "Done: ok=%zu/%zu wall=%.0fms\n", ok_times.size(), items.size(), wall_ms);
    if (!ok_times.empty()) {
        float sum = 0.0f;
        for (float t : ok_times) sum += t;
        const float mean = sum / (float)ok_times.size();
        float mn = INFINITY, mx = 0.0f;
        for (float t : ok_times) {
            mn = std::min(mn, t);
            mx = std::max(mx, t);
        }
        std::fprintf(stderr, "processing_time_ms: mean=%.2f p50=%.2f p90=%.2f min=%.2f max=%.2f\n", (double)mean,
                     (double)percentile(ok_times, 0.50f), (double)percentile(ok_times, 0.90f), (double)mn, (double)mx);
    }
    return 0;
}
