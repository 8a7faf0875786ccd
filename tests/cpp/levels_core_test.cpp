// Host harness of stratum-dsp_amd/csrc/levels_core.hpp (tests/test_levels_core.py builds it with the
// address and undefined-behaviour sanitizers).  Without arguments: the request checks, the
// silence map's keep-rule and capacity bound, and the identity-filter lanes of k_levels_fold.
//   layout          sizes and offsets of the public structs, for the ctypes mirrors
//   fold <file>     the folds and the finishing code over the tracks of <file>, one line of bits per
//                   track and method, for tests/levels_ref.py to compare
//   map <file>      lv_silence_map over the frame-RMS rows of <file>
// <file> (native endian): f32 target_peak, target_rms, target_lufs, gate, b0, b1, b2, a1, a2; i64
// block; u64 T; per track u64 n and n f32 samples.  map: f32 thr; u64 min_frames, hop, T; per
// track u64 n, F and F f32 frame RMS values.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stratum-dsp_amd/csrc/levels_core.hpp"

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

// One track's folds in the order k_levels_fold takes them: the first launch's chains, the Loudness
// gain, the second launch's chain.  A sum-of-squares chain is folded twice, by the plain step and as
// the kernel's identity-filter lane beside the biquad; the two must agree bit for bit.
static LvFolds fold_track(const std::vector<float>& x, const LvParams& P) {
    LvFolds f{};
    for (float v : x) f.peak = sd_maxf(f.peak, sd_absf(v));
    const float g_peak = lv_peak_gain(f.peak, P.target_peak);
    auto squares = [&](float g) {
        float plain = 0.0f;
        LvBiquad id{1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float lane = 0.0f;
        for (float v : x) {
            lv_square(plain, v, g);
            const float o = lv_biquad(id, v * g);
            lane += o * o;
        }
        CHECK(sd_bits_f(plain) == sd_bits_f(lane));
        return plain;
    };
    f.ss_raw = squares(1.0f);
    f.ss_peak = squares(g_peak);
    if (P.block > 0) {
        LvBiquad q{P.b0, P.b1, P.b2, P.a1, P.a2, 0.0f, 0.0f};
        LvGated gs{0.0f, 0.0f, 0};
        int64_t cnt = 0;
        for (float v : x) {
            const float o = lv_biquad(q, v * 1.0f);
            gs.bsum += o * o;
            if (++cnt == P.block) {
                lv_close_block(gs, P.block, P.gate);
                cnt = 0;
            }
        }
        if (cnt > 0) lv_close_block(gs, cnt, P.gate);
        f.gsum = gs.gsum;
        f.gn = gs.gn;
    }
    int st;
    f.ss_lufs = squares(lv_lufs_gain(f, P, &st));
    return f;
}

static void print_loudness(uint64_t t, int m, const sdsp_loudness& l) {
    std::printf("%llu %d %d %d %d %08x %08x %08x %08x %08x\n", (unsigned long long)t, m, (int)l.status, (int)l.measured,
                (int)l.has_lufs, sd_bits_f(l.measured_lufs), sd_bits_f(l.peak_db), sd_bits_f(l.rms_db),
                sd_bits_f(l.gain_db), sd_bits_f(l.gain));
}

static int run_fold(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    LvParams P{};
    P.target_peak = rd<float>(f), P.target_rms = rd<float>(f), P.target_lufs = rd<float>(f), P.gate = rd<float>(f);
    P.b0 = rd<float>(f), P.b1 = rd<float>(f), P.b2 = rd<float>(f), P.a1 = rd<float>(f), P.a2 = rd<float>(f);
    P.block = rd<int64_t>(f);
    const uint64_t T = rd<uint64_t>(f);
    for (uint64_t t = 0; t < T; t++) {
        const uint64_t n = rd<uint64_t>(f);
        const std::vector<float> x = rd_f32(f, n);
        const LvFolds fo = fold_track(x, P);
        print_loudness(t, 0, lv_finish_peak(fo, n, P));
        print_loudness(t, 1, lv_finish_rms(fo, n, P));
        print_loudness(t, 2, lv_finish_loudness(fo, n, P));
    }
    std::fclose(f);
    return fails ? 1 : 0;
}

static int run_map(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    const float thr = rd<float>(f);
    const uint64_t min_frames = rd<uint64_t>(f), hop = rd<uint64_t>(f), T = rd<uint64_t>(f);
    for (uint64_t t = 0; t < T; t++) {
        const uint64_t n = rd<uint64_t>(f), F = rd<uint64_t>(f);
        const std::vector<float> r = rd_f32(f, F);
        std::vector<uint64_t> out(2 * (size_t)lv_map_capacity(F, min_frames));  // exactly the kernel's bound
        const uint64_t k = lv_silence_map(r.data(), F, 1, thr, min_frames, hop, n, out.data());
        std::printf("%llu %llu", (unsigned long long)t, (unsigned long long)k);
        for (uint64_t i = 0; i < 2 * k; i++) std::printf(" %llu", (unsigned long long)out[(size_t)i]);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}

static void layout() {
    std::printf("sdsp_levels_request %zu\n", sizeof(sdsp_levels_request));
    std::printf("sdsp_loudness %zu %zu %zu %zu %zu\n", sizeof(sdsp_loudness), offsetof(sdsp_loudness, measured),
                offsetof(sdsp_loudness, has_lufs), offsetof(sdsp_loudness, measured_lufs), offsetof(sdsp_loudness, gain));
    std::printf("sdsp_silence_region %zu %zu\n", sizeof(sdsp_silence_region), offsetof(sdsp_silence_region, duration_seconds));
    std::printf("sdsp_levels %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sdsp_levels), offsetof(sdsp_levels, applied_gain),
                offsetof(sdsp_levels, n_samples), offsetof(sdsp_levels, frame_size), offsetof(sdsp_levels, n_regions),
                offsetof(sdsp_levels, regions), offsetof(sdsp_levels, status));
    std::printf("sdsp_request_set %zu %zu %zu %zu %zu\n", sizeof(sdsp_request_set), offsetof(sdsp_request_set, ov_req),
                offsetof(sdsp_request_set, kt_req), offsetof(sdsp_request_set, lv_req), offsetof(sdsp_request_set, levels));
}

static void requests() {
    CHECK(levels_request_error(0) != nullptr);
    for (uint32_t w = 1; w <= 15; w++) CHECK(levels_request_error(w) == nullptr);
    CHECK(levels_request_error(16) != nullptr);
    CHECK(levels_request_error(8 | 32) != nullptr);
    CHECK(levels_request_error(0x80000000u) != nullptr);

    sdsp_overview_request ov{};
    sdsp_key_timeline_request kt{};
    sdsp_levels_request lv{SDSP_LEVELS_PEAK};
    sdsp_overview o1{};
    sdsp_key_timeline t1{};
    sdsp_levels l1{};
    sdsp_request_set in{};
    in.struct_size = (uint32_t)sizeof(in);
    in.ov_req = &ov, in.overviews = &o1, in.kt_req = &kt, in.timelines = &t1, in.lv_req = &lv, in.levels = &l1;
    sdsp_request_set out;
    CHECK(request_set_read(nullptr, &out) == nullptr && !out.ov_req && !out.kt_req && !out.lv_req);
    CHECK(request_set_read(&in, &out) == nullptr && out.ov_req == &ov && out.overviews == &o1 && out.kt_req == &kt &&
          out.timelines == &t1 && out.lv_req == &lv && out.levels == &l1);
    // an older caller: the struct ends after the timeline pair; the levels fields read as NULL
    in.struct_size = (uint32_t)offsetof(sdsp_request_set, lv_req);
    CHECK(request_set_read(&in, &out) == nullptr && out.kt_req == &kt && out.timelines == &t1 && !out.lv_req && !out.levels);
    // a request without its array is the caller's to refuse: the pointer alone is read
    in.struct_size = (uint32_t)(offsetof(sdsp_request_set, lv_req) + sizeof(void*));
    CHECK(request_set_read(&in, &out) == nullptr && out.lv_req == &lv && !out.levels);
    in.struct_size = (uint32_t)(offsetof(sdsp_request_set, overviews) + sizeof(void*));
    CHECK(request_set_read(&in, &out) == nullptr && out.ov_req == &ov && out.overviews == &o1 && !out.kt_req);
    // smaller than the first pair: refused
    for (uint32_t s : {0u, 4u, (uint32_t)offsetof(sdsp_request_set, overviews),
                       (uint32_t)(offsetof(sdsp_request_set, overviews) + sizeof(void*) - 1)}) {
        in.struct_size = s;
        CHECK(request_set_read(&in, &out) != nullptr);
        CHECK(!out.ov_req && !out.lv_req);
    }
    // a newer caller's larger struct: the fields this library knows
    in.struct_size = (uint32_t)sizeof(in) + 64;
    CHECK(request_set_read(&in, &out) == nullptr && out.lv_req == &lv && out.levels == &l1);
}

static void keep_rule() {
    CHECK(lv_keep_run(0, 1, 8));    // the leading run, whatever its length
    CHECK(!lv_keep_run(3, 10, 8));  // 7 interior frames
    CHECK(lv_keep_run(3, 11, 8));   // 8
    CHECK(lv_keep_run(5, 5, 0));    // (min_frames 0 keeps everything)
    CHECK(lv_frames(1, 2048) == 1 && lv_frames(2047, 2048) == 1 && lv_frames(2048, 2048) == 1 &&
          lv_frames(3071, 2048) == 1 && lv_frames(3072, 2048) == 2);
    CHECK(lv_min_frames(16000, 2048) == 8 && lv_min_frames(44100, 2048) == 22);
    // the capacity bound holds on the densest pattern: a leading silent frame, then runs of exactly
    // min_frames silent frames and one loud frame, and a trailing run
    for (uint64_t mf : {0ull, 1ull, 2ull, 8ull}) {
        for (uint64_t F : {1ull, 2ull, 3ull, 9ull, 10ull, 64ull, 257ull, 1000ull}) {
            std::vector<float> r((size_t)F, 0.0f);
            const uint64_t per = (mf > 1 ? mf : 1) + 1;
            for (uint64_t f = 1; f < F; f += per) r[(size_t)f] = 1.0f;  // loud frames
            std::vector<uint64_t> out(2 * (size_t)lv_map_capacity(F, mf) + 2, ~0ull);
            const uint64_t k = lv_silence_map(r.data(), F, 1, 0.5f, mf, 1024, F * 1024 + 1024, out.data());
            CHECK(k <= lv_map_capacity(F, mf));
            CHECK(out[2 * (size_t)lv_map_capacity(F, mf)] == ~0ull);
            for (uint64_t i = 0; i + 1 < k; i++) CHECK(out[2 * i + 1] < out[2 * i + 2]);  // ascending, disjoint
        }
    }
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "layout")) return layout(), 0;
    if (argc == 3 && !std::strcmp(argv[1], "fold")) return run_fold(argv[2]);
    if (argc == 3 && !std::strcmp(argv[1], "map")) return run_map(argv[2]);
    requests();
    keep_rule();
    if (fails) return 1;
    std::printf("ok levels_core\n");
    return 0;
}
