// Host harness of stratum-dsp_amd/csrc/key_timeline_plan.hpp (tests/test_key_timeline_plan.py builds
// it with the address and undefined-behaviour sanitizers): the segment plan against the formulas of
// include/stratum_hip.h, the requests that are refused, the primary-key and change logic.  With
// arguments "plan <sr> <khop> <seg_s> <ovl_s> <seg_f> <hop_f> <minconf>" it prints one request's
// plan for the Python reference to compare.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../stratum-dsp_amd/csrc/key_timeline_plan.hpp"

using namespace sdsp;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
            fails++;                                                    \
        }                                                               \
    } while (0)

static const char* plan(float ss, float os, uint32_t sf, uint32_t hf, float mc, uint32_t sr, uint32_t khop, uint32_t* L,
                        uint32_t* H) {
    return key_timeline_plan(ss, os, sf, hf, mc, sr, khop, L, H);
}

static void segments() {
    const uint64_t Fs[] = {0, 1, 2, 63, 64, 65, 689, 15500};
    for (uint64_t F : Fs) {
        const uint64_t LH[][2] = {{1, 1}, {2, 1}, {64, 64}, {65, 3}, {F, F}, {F + 1, 1}};
        for (auto& lh : LH) {
            const uint64_t L = lh[0], H = lh[1];
            if (L == 0 || H == 0) {  // (F, F) at F = 0: refused as a request
                uint32_t l, h;
                CHECK(plan(0, 0, (uint32_t)L, (uint32_t)H, -1.0f, 44100, 512, &l, &h) != nullptr);
                CHECK(kt_segments(F, L, H) == 0);
                continue;
            }
            uint32_t l, h;
            CHECK(plan(0, 0, (uint32_t)L, (uint32_t)H, -1.0f, 44100, 512, &l, &h) == nullptr && l == L && h == H);
            const uint64_t S = kt_segments(F, L, H);
            // the definition: the count of s >= 0 with s H + L <= F
            uint64_t want = 0;
            while (want * H + L <= F) want++;
            CHECK(S == want);
            CHECK(S == (F < L ? 0 : (F - L) / H + 1));
            for (uint64_t s = 0; s < S; s++) {
                CHECK(kt_start(s, H) == s * H);
                CHECK(kt_start(s, H) + L <= F);  // inside [0, F)
            }
            if (S) CHECK(kt_start(S, H) + L > F);  // and no further segment fits
            if (L == F + 1) CHECK(S == 0);
            if (L == F && F) CHECK(S == 1);
            if (L == 1 && H == 1) CHECK(S == F);
        }
    }
}

static void seconds_form() {
    uint32_t L, H;
    // 44100 / 512 = 86.1328125 and 48000 / 512 = 93.75, both exact in f32
    CHECK(kt_fps(44100, 512) == 86.1328125f && kt_fps(48000, 512) == 93.75f);
    CHECK(plan(8.0f, 2.0f, 0, 0, -1.0f, 44100, 512, &L, &H) == nullptr && L == 689 && H == 689 - 172);
    CHECK(plan(4.0f, 1.0f, 0, 0, -1.0f, 44100, 512, &L, &H) == nullptr && L == 344 && H == 344 - 86);
    // exactly on an integer frame count: 512 s * 86.1328125 = 44100 frames; 16 s * 93.75 = 1500
    CHECK(plan(512.0f, 0.0f, 0, 0, -1.0f, 44100, 512, &L, &H) == nullptr && L == 44100 && H == 44100);
    CHECK(plan(16.0f, 8.0f, 0, 0, -1.0f, 48000, 512, &L, &H) == nullptr && L == 1500 && H == 750);
    // just below: the next f32 under the exact value truncates to one frame less
    CHECK(plan(std::nextafterf(512.0f, 0.0f), 0.0f, 0, 0, -1.0f, 44100, 512, &L, &H) == nullptr && L == 44099);
    CHECK(plan(std::nextafterf(16.0f, 0.0f), std::nextafterf(8.0f, 0.0f), 0, 0, -1.0f, 48000, 512, &L, &H) == nullptr &&
          L == 1499 && H == 1499 - 749);
    // the product is f32: 0.32 s * 93.75 is 30.000002 in f32 (30 frames), 29.999999... in double
    CHECK(plan(0.32f, 0.0f, 0, 0, -1.0f, 48000, 512, &L, &H) == nullptr && L == (uint32_t)(uint64_t)(0.32f * 93.75f));
    // timestamps
    CHECK(kt_timestamp(0, 517, kt_fps(44100, 512)) == 0.0f);
    CHECK(kt_timestamp(2, 517, kt_fps(44100, 512)) == 1034.0f / 86.1328125f);
}

static void refused() {
    uint32_t L, H;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    auto has = [&](const char* r, const char* s) { return r && std::strstr(r, s); };
    CHECK(has(plan(0, 0, 0, 0, -1.0f, 44100, 512, &L, &H), "neither"));
    CHECK(has(plan(8.0f, 0, 64, 1, -1.0f, 44100, 512, &L, &H), "both"));
    CHECK(has(plan(0, 1.0f, 0, 1, -1.0f, 44100, 512, &L, &H), "both"));
    CHECK(has(plan(inf, 0, 0, 0, -1.0f, 44100, 512, &L, &H), "not finite"));
    CHECK(has(plan(8.0f, nan, 0, 0, -1.0f, 44100, 512, &L, &H), "not finite"));
    CHECK(has(plan(nan, 0, 0, 0, -1.0f, 44100, 512, &L, &H), "not finite"));
    CHECK(has(plan(-8.0f, 0, 0, 0, -1.0f, 44100, 512, &L, &H), "negative"));
    CHECK(has(plan(8.0f, -1.0f, 0, 0, -1.0f, 44100, 512, &L, &H), "negative"));
    CHECK(has(plan(8.0f, 2.0f, 0, 0, nan, 44100, 512, &L, &H), "NaN"));
    CHECK(has(plan(0, 0, 64, 1, nan, 44100, 512, &L, &H), "NaN"));
    CHECK(has(plan(0.01f, 0, 0, 0, -1.0f, 44100, 512, &L, &H), "L == 0"));  // 0.86 frames
    CHECK(has(plan(0, 2.0f, 0, 0, -1.0f, 44100, 512, &L, &H), "L == 0"));
    CHECK(has(plan(8.0f, 8.0f, 0, 0, -1.0f, 44100, 512, &L, &H), "O >= L"));
    CHECK(has(plan(8.0f, 9.0f, 0, 0, -1.0f, 44100, 512, &L, &H), "O >= L"));
    CHECK(has(plan(8.0f, 2.0f, 0, 0, -1.0f, 0, 512, &L, &H), "L == 0"));  // sample rate 0
    CHECK(has(plan(0, 0, 0, 4, -1.0f, 44100, 512, &L, &H), "L == 0"));
    CHECK(has(plan(0, 0, 4, 0, -1.0f, 44100, 512, &L, &H), "H == 0"));
    CHECK(has(plan(0, 0, 0x80000000u, 1, -1.0f, 44100, 512, &L, &H), "2^31"));
    CHECK(has(plan(0, 0, 4, 0x80000000u, -1.0f, 44100, 512, &L, &H), "2^31"));
    CHECK(has(plan(3e7f, 0, 0, 0, -1.0f, 44100, 512, &L, &H), "2^31"));   // 2.58e9 frames
    CHECK(has(plan(3e38f, 0, 0, 0, -1.0f, 44100, 512, &L, &H), "2^31"));  // the product overflows to +inf
    CHECK(L == 0 && H == 0);
    CHECK(plan(0, 0, 0x7FFFFFFFu, 0x7FFFFFFFu, 0.2f, 44100, 512, &L, &H) == nullptr && L == 0x7FFFFFFFu);
    CHECK(plan(8.0f, 2.0f, 0, 0, -inf, 44100, 512, &L, &H) == nullptr);  // an infinite threshold is a threshold
}

static void primary_and_changes() {
    int32_t pk;
    float pc;
    uint64_t pn;
    kt_primary(nullptr, nullptr, 0, &pk, &pc, &pn);
    CHECK(pk == -1 && pc == 0.0f && pn == 0);
    {
        const int32_t k[] = {5};
        const float c[] = {0.25f};
        kt_primary(k, c, 1, &pk, &pc, &pn);
        CHECK(pk == 5 && pc == 0.25f && pn == 1);
    }
    {  // a count tie goes to the key whose first segment is earliest, not to the smaller index
        const int32_t k[] = {7, 3, 3, 7, 1};
        const float c[] = {0.1f, 0.2f, 0.4f, 0.3f, 0.9f};
        kt_primary(k, c, 5, &pk, &pc, &pn);
        CHECK(pk == 7 && pn == 2 && pc == (0.1f + 0.3f) / 2.0f);
        const int32_t k2[] = {3, 7, 7, 3};
        kt_primary(k2, c, 4, &pk, &pc, &pn);
        CHECK(pk == 3 && pn == 2);
    }
    {
        const int32_t k[] = {0, 0, 6, 6, 2};
        const float c[] = {0.2f, 0.2f, 0.2f, 0.6f, 0.0f};
        float cc;
        CHECK(!kt_change(k, c, 1, -1.0f, &cc));
        CHECK(kt_change(k, c, 2, -1.0f, &cc) && cc == 0.2f);
        CHECK(!kt_change(k, c, 2, 0.2f, &cc));  // strict: 0.2 is not > 0.2
        CHECK(kt_change(k, c, 2, std::nextafterf(0.2f, 0.0f), &cc));
        CHECK(!kt_change(k, c, 3, -1.0f, &cc));
        CHECK(kt_change(k, c, 4, 0.2f, &cc) && cc == (0.6f + 0.0f) / 2.0f);
    }
}

int main(int argc, char** argv) {
    if (argc == 9 && !std::strcmp(argv[1], "plan")) {
        uint32_t L, H;
        const char* why = plan(std::strtof(argv[4], nullptr), std::strtof(argv[5], nullptr),
                               (uint32_t)std::strtoull(argv[6], nullptr, 10), (uint32_t)std::strtoull(argv[7], nullptr, 10),
                               std::strtof(argv[8], nullptr), (uint32_t)std::strtoull(argv[2], nullptr, 10),
                               (uint32_t)std::strtoull(argv[3], nullptr, 10), &L, &H);
        if (why) std::printf("refused %s\n", why);
        else std::printf("plan %u %u\n", L, H);
        return 0;
    }
    segments();
    seconds_form();
    refused();
    primary_and_changes();
    if (fails) return 1;
    std::printf("ok key_timeline_plan\n");
    return 0;
}
