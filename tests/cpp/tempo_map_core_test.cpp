// Host harness of stratum-dsp_amd/csrc/tempo_map_core.hpp (tests/test_tempo_map_core.py builds it with
// the address and undefined-behaviour sanitizers).  Without arguments: the request checks, the
// penalty steps, the signature pick's ties and fallback, and the segment-capacity bound over a sweep
// of spans, offsets and tempi.
//   layout            sizes and offsets of the public structs, for the ctypes mirrors
//   windows <file>    detect_tempo_variations replayed with tm_window over the beat lists of <file>:
//                     per track "T <segments>", then per segment the bits of start, end, bpm,
//                     confidence and is_variable
//   update <file>     tm_updated_confidence over (likelihood, old tempo, new tempo) triples: bits
//   pick <file>       tm_pick_signature over score triples: beats per bar and the confidence's bits
// <file> (native endian): windows: u64 T; per track f32 nominal, u64 n, n f32 beats.  update / pick:
// u64 N, then N x 3 f32.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stratum-dsp_amd/csrc/levels_core.hpp"
#include "../../stratum-dsp_amd/csrc/tempo_map_core.hpp"

using namespace sdsp;

static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                \
        }                                                           \
    } while (0)

template <class T>
static T rd(FILE* f) {
    T v{};
    if (std::fread(&v, sizeof v, 1, f) != 1) {
        std::printf("FAIL short input\n");
        std::exit(2);
    }
    return v;
}
static std::vector<float> rd_f32(FILE* f, uint64_t n) {
    std::vector<float> v((size_t)n);
    if (n && std::fread(v.data(), sizeof(float), (size_t)n, f) != n) {
        std::printf("FAIL short input\n");
        std::exit(2);
    }
    return v;
}
static uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

static int lower_bound_f(const float* a, int n, float x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
static int upper_bound_f(const float* a, int n, float x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (!(x < a[mid]))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

struct Row {
    float start, end, bpm, conf;
    bool variable;
};
// detect_tempo_variations as k_tempo_map evaluates it: the starts by sequential addition, each
// window by tm_window over its own binary searches.  *windows: the starts visited.
static std::vector<Row> segments(const std::vector<float>& b, float nominal, uint64_t* windows) {
    const int n = (int)b.size();
    *windows = 0;
    if (n < 4) return {{n ? b[0] : 0.0f, n ? b[n - 1] : 0.0f, nominal, 0.5f, false}};
    const float total = b[n - 1] - b[0];
    if (total < 2.0f) return {{b[0], b[n - 1], nominal, 0.8f, false}};
    const float seg_dur = sd_clampf(total / 4.0f, 4.0f, 8.0f);
    const float step = seg_dur - seg_dur * 0.5f;
    std::vector<Row> out;
    for (float cur = b[0]; cur < b[n - 1]; cur += step) {
        ++*windows;
        const float se = sd_minf(cur + seg_dur, b[n - 1]);
        Row r{cur, se, 0.0f, 0.0f, false};
        if (tm_window(b.data(), lower_bound_f(b.data(), n, cur), upper_bound_f(b.data(), n, se), nominal, &r.bpm, &r.conf,
                      &r.variable))
            out.push_back(r);
    }
    if (out.empty()) out.push_back({b[0], b[n - 1], nominal, 0.8f, false});
    return out;
}

// Windows detect_tempo_variations starts between a first beat at b0 and a last one at `last`.
static uint64_t count_windows(float b0, float last) {
    const float total = last - b0;
    if (total < 2.0f) return 1;
    const float seg_dur = sd_clampf(total / 4.0f, 4.0f, 8.0f);
    const float step = seg_dur - seg_dur * 0.5f;
    uint64_t k = 0;
    for (float cur = b0; cur < last; cur += step) k++;
    return k;
}

static void self_checks() {
    // request validation
    CHECK(tempo_map_request_error(0, true, SDSP_STAGES_FULL) != nullptr);
    CHECK(tempo_map_request_error(4, true, SDSP_STAGES_FULL) != nullptr);
    CHECK(tempo_map_request_error(1 | 8, true, SDSP_STAGES_FULL) != nullptr);
    CHECK(tempo_map_request_error(0x80000000u, true, SDSP_STAGES_FULL) != nullptr);
    CHECK(tempo_map_request_error(3, false, SDSP_STAGES_FULL) != nullptr);
    CHECK(tempo_map_request_error(3, true, SDSP_STAGES_BPM_ONLY) != nullptr);
    for (uint32_t w = 1; w <= 3; w++) CHECK(tempo_map_request_error(w, true, SDSP_STAGES_FULL) == nullptr);
    // the request set: a caller whose struct ends before the tempo map pair keeps working
    {
        sdsp_tempo_map_request rq{3};
        sdsp_tempo_map maps[1];
        sdsp_request_set in{}, out;
        in.tm_req = &rq;
        in.tempo_maps = maps;
        in.struct_size = (uint32_t)sizeof(in);
        CHECK(request_set_read(&in, &out) == nullptr && out.tm_req == &rq && out.tempo_maps == maps);
        in.struct_size = (uint32_t)offsetof(sdsp_request_set, tm_req);
        CHECK(request_set_read(&in, &out) == nullptr && out.tm_req == nullptr && out.tempo_maps == nullptr);
        in.struct_size = (uint32_t)(offsetof(sdsp_request_set, tm_req) + sizeof(void*));
        CHECK(request_set_read(&in, &out) == nullptr && out.tm_req == &rq && out.tempo_maps == nullptr);
        in.struct_size = (uint32_t)sizeof(in) + 64;
        CHECK(request_set_read(&in, &out) == nullptr && out.tm_req == &rq && out.tempo_maps == maps);
    }
    // the penalty's steps (bayesian.rs:163-170) and the confidence's cap
    CHECK(tm_penalty(0.0f) == 1.0f && tm_penalty(0.999f) == 1.0f && tm_penalty(1.0f) == 0.8f);
    CHECK(tm_penalty(2.999f) == 0.8f && tm_penalty(3.0f) == 0.5f && tm_penalty(5.0f) == 0.5f);
    CHECK(tm_updated_confidence(1.0f, 120.0f, 120.5f) == 1.0f);
    CHECK(tm_updated_confidence(0.5f, 120.0f, 122.0f) == 0.5f * 0.8f);
    CHECK(tm_updated_confidence(0.0f, 50.0f, 50.0f) == 0.0f);
    // the segment confidence's clamps
    CHECK(tm_segment_confidence(0.0f) == 1.0f && tm_segment_confidence(0.3f) == 0.0f && tm_segment_confidence(7.0f) == 0.0f);
    // the signature pick: the LAST maximum wins, so a three-way tie is 6/8
    {
        uint32_t bpb;
        float conf;
        const float tie[3] = {0.9f, 0.9f, 0.9f}, a[3] = {0.9f, 0.5f, 0.1f}, b[3] = {0.5f, 0.9f, 0.9f}, c[3] = {0.9f, 0.9f, 0.5f};
        tm_pick_signature(tie, &bpb, &conf);
        CHECK(bpb == 6 && conf == 0.9f);
        tm_pick_signature(a, &bpb, &conf);
        CHECK(bpb == 4 && conf == 0.9f);
        tm_pick_signature(b, &bpb, &conf);
        CHECK(bpb == 6);
        tm_pick_signature(c, &bpb, &conf);
        CHECK(bpb == 3);
        const float zero[3] = {0.0f, 0.0f, 0.0f};
        tm_pick_signature(zero, &bpb, &conf);
        CHECK(bpb == 6 && conf == 0.0f);
    }
    // a window: fewer than 3 beats, no positive interval, a regular and an irregular one
    {
        float bpm, conf;
        bool var;
        const float two[2] = {1.0f, 1.5f}, flat[3] = {1.0f, 1.0f, 1.0f}, reg[4] = {0.0f, 0.5f, 1.0f, 1.5f},
                    irr[4] = {0.0f, 0.5f, 1.5f, 1.75f};
        CHECK(!tm_window(two, 0, 2, 120.0f, &bpm, &conf, &var));
        CHECK(!tm_window(flat, 0, 3, 120.0f, &bpm, &conf, &var));
        CHECK(tm_window(reg, 0, 4, 100.0f, &bpm, &conf, &var) && bpm == 120.0f && conf == 1.0f && !var);
        CHECK(tm_window(irr, 0, 4, 100.0f, &bpm, &conf, &var) && var && conf == 0.0f);
    }
    // The capacity bound.  A track of n_trim samples: the onsets span less than n_trim / sr, the
    // first HMM beat is the first onset (b0), the last lies on the grid b0 + k * interval at most
    // 0.054 s (the emission tolerance: exp(-d^2 / (2 * 0.025^2)) > 0.1) past the last onset.
    uint64_t worst_slack = ~0ull, spans = 0;
    for (uint32_t sr : {8000u, 44100u, 96000u}) {
        for (double secs = 0.5; secs < 7300.0; secs += secs < 40.0 ? 0.0371 : secs < 600.0 ? 1.913 : 37.7) {
            const uint64_t n_trim = (uint64_t)(secs * sr);
            const uint64_t cap = tm_segment_capacity(n_trim, sr);
            for (float b0 : {0.0f, 0.013f, 1.7f, 33.3f}) {
                if (b0 >= (float)secs) continue;
                const float span = (float)n_trim / (float)sr - b0;  // the onsets' span, at most
                for (float bpm : {40.0f, 61.3f, 120.0f, 187.7f, 300.0f}) {
                    const float interval = 60.0f / bpm;
                    const float last = b0 + (float)(uint64_t)((span + 0.054f) / interval) * interval;
                    const uint64_t w = count_windows(b0, last);
                    CHECK(w <= cap);
                    if (cap - w < worst_slack) worst_slack = cap - w;
                    spans++;
                }
                // the latest last beat the tolerance allows, whatever the tempo
                const uint64_t w = count_windows(b0, b0 + span + 0.054f);
                CHECK(w <= cap);
                if (cap - w < worst_slack) worst_slack = cap - w;
            }
        }
    }
    // the 2 s step minimum: spans up to 16 s step by exactly 2 s
    for (float total = 2.0f; total <= 16.0f; total += 0.0625f) {
        const uint64_t w = count_windows(5.0f, 5.0f + total);
        const uint64_t halves = (uint64_t)(total / 2.0f);
        CHECK(w == halves + (2.0f * (float)halves < total ? 1 : 0));  // ceil(total / 2): the starts 5 + 2 k are exact
        CHECK(w <= tm_segment_capacity((uint64_t)((5.0f + total) * 44100.0f), 44100));
    }
    CHECK(tm_segment_capacity(0, 44100) >= 1 && tm_segment_capacity(100, 0) >= 1);
    std::printf("%s tempo_map_core (%llu spans, least slack %llu)\n", fails ? "FAILED" : "ok", (unsigned long long)spans,
                (unsigned long long)worst_slack);
}

int main(int argc, char** argv) {
    if (argc == 1) {
        self_checks();
        return fails ? 1 : 0;
    }
    const char* mode = argv[1];
    if (!std::strcmp(mode, "layout")) {
        std::printf("sdsp_tempo_map_request %zu\n", sizeof(sdsp_tempo_map_request));
        std::printf("sdsp_tempo_segment %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sdsp_tempo_segment),
                    offsetof(sdsp_tempo_segment, start_time), offsetof(sdsp_tempo_segment, end_time),
                    offsetof(sdsp_tempo_segment, bpm), offsetof(sdsp_tempo_segment, confidence),
                    offsetof(sdsp_tempo_segment, is_variable), offsetof(sdsp_tempo_segment, updated),
                    offsetof(sdsp_tempo_segment, n_onsets), offsetof(sdsp_tempo_segment, updated_bpm),
                    offsetof(sdsp_tempo_segment, updated_confidence), offsetof(sdsp_tempo_segment, n_beats));
        std::printf("sdsp_tempo_map %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sdsp_tempo_map),
                    offsetof(sdsp_tempo_map, status), offsetof(sdsp_tempo_map, has_grid), offsetof(sdsp_tempo_map, has_variation),
                    offsetof(sdsp_tempo_map, refined), offsetof(sdsp_tempo_map, time_signature_scored),
                    offsetof(sdsp_tempo_map, nominal_bpm), offsetof(sdsp_tempo_map, nominal_confidence),
                    offsetof(sdsp_tempo_map, hmm_beats), offsetof(sdsp_tempo_map, beats_per_bar),
                    offsetof(sdsp_tempo_map, time_signature_confidence), offsetof(sdsp_tempo_map, time_signature_scores),
                    offsetof(sdsp_tempo_map, first_sample), offsetof(sdsp_tempo_map, n_segments),
                    offsetof(sdsp_tempo_map, segments), offsetof(sdsp_tempo_map, n_onsets), offsetof(sdsp_tempo_map, onsets));
        std::printf("sdsp_request_set %zu %zu %zu\n", sizeof(sdsp_request_set), offsetof(sdsp_request_set, tm_req),
                    offsetof(sdsp_request_set, tempo_maps));
        return 0;
    }
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    if (!std::strcmp(mode, "windows")) {
        const uint64_t T = rd<uint64_t>(f);
        for (uint64_t t = 0; t < T; t++) {
            const float nominal = rd<float>(f);
            const std::vector<float> b = rd_f32(f, rd<uint64_t>(f));
            uint64_t windows = 0;
            const std::vector<Row> s = segments(b, nominal, &windows);
            const uint64_t n_trim = b.empty() ? 0 : (uint64_t)(b.back() * 44100.0f);  // ends no earlier than its last beat
            if (windows > tm_segment_capacity(n_trim, 44100)) std::printf("FAIL capacity\n");
            std::printf("T %zu\n", s.size());
            for (const Row& r : s)
                std::printf("%08x %08x %08x %08x %d\n", bits(r.start), bits(r.end), bits(r.bpm), bits(r.conf), (int)r.variable);
        }
    } else if (!std::strcmp(mode, "update") || !std::strcmp(mode, "pick")) {
        const uint64_t N = rd<uint64_t>(f);
        for (uint64_t k = 0; k < N; k++) {
            const std::vector<float> v = rd_f32(f, 3);
            if (mode[0] == 'u') {
                std::printf("%08x\n", bits(tm_updated_confidence(v[0], v[1], v[2])));
            } else {
                uint32_t bpb;
                float conf;
                tm_pick_signature(v.data(), &bpb, &conf);
                std::printf("%u %08x\n", bpb, bits(conf));
            }
        }
    } else {
        return 2;
    }
    std::fclose(f);
    return 0;
}
