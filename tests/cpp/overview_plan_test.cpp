// Host harness for stratum-dsp_amd/csrc/overview_plan.hpp (tests/test_overview_plan.py): the
// column plan of the overview envelope against the formulas of include/stratum_hip.h, written out
// here a second time, and the properties the kernels rely on.  Built stand-alone with
// -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <utility>

#include "../../stratum-dsp_amd/csrc/overview_plan.hpp"

using namespace sdsp;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            g_fail++;                                      \
        }                                                  \
    } while (0)

// one (F, form) case: the formulas, and the partitions of [0, F) and [0, n)
static void check_plan(uint64_t F, uint32_t columns, uint32_t fpc, uint64_t frame_size, uint64_t hop, uint64_t tail) {
    // a length with exactly F frames and `tail` (< hop) samples after the last hop
    const uint64_t n = F == 0 ? frame_size - 1 : (F - 1) * hop + frame_size + tail;
    CHECK(ov_frames(n, frame_size, hop) == F, "F=%llu n=%llu", (unsigned long long)F, (unsigned long long)n);
    const uint64_t C = ov_columns(F, columns, fpc);
    const uint64_t want_C = columns ? (columns < F ? columns : F) : (F + fpc - 1) / fpc;
    CHECK(C == want_C, "C=%llu want %llu (F=%llu columns=%u fpc=%u)", (unsigned long long)C, (unsigned long long)want_C,
          (unsigned long long)F, columns, fpc);
    CHECK((F == 0) == (C == 0), "F=%llu C=%llu", (unsigned long long)F, (unsigned long long)C);
    CHECK(ov_f0(C, F, C, columns, fpc) == F, "f0(C) != F");
    if (C == 0) return;
    CHECK(ov_f0(0, F, C, columns, fpc) == 0, "f0(0) != 0");
    uint64_t longest = 0, next_sample = 0;
    for (uint64_t c = 0; c < C; c++) {
        const uint64_t a = ov_f0(c, F, C, columns, fpc), b = ov_f0(c + 1, F, C, columns, fpc);
        const uint64_t want_a = columns ? (uint64_t)((unsigned __int128)c * F / C) : (c * fpc < F ? c * fpc : F);
        CHECK(a == want_a, "f0(%llu)=%llu want %llu", (unsigned long long)c, (unsigned long long)a, (unsigned long long)want_a);
        CHECK(a < b && b <= F, "column %llu empty or out of order: [%llu, %llu)", (unsigned long long)c,
              (unsigned long long)a, (unsigned long long)b);
        longest = b - a > longest ? b - a : longest;
        uint64_t s0 = 0, s1 = 0;
        ov_sample_range(c, F, C, columns, fpc, hop, n, &s0, &s1);
        CHECK(s0 == next_sample && s0 == a * hop, "column %llu starts at sample %llu, want %llu", (unsigned long long)c,
              (unsigned long long)s0, (unsigned long long)next_sample);
        CHECK(s1 == (c + 1 < C ? b * hop : n) && s0 < s1 && s1 <= n, "column %llu ends at %llu", (unsigned long long)c,
              (unsigned long long)s1);
        next_sample = s1;
    }
    CHECK(next_sample == n, "the sample ranges end at %llu, n = %llu", (unsigned long long)next_sample, (unsigned long long)n);
    CHECK(ov_max_column_frames(F, C, columns, fpc) == longest, "longest column %llu, plan says %llu",
          (unsigned long long)longest, (unsigned long long)ov_max_column_frames(F, C, columns, fpc));
    for (uint32_t piece : {1u, 64u}) {
        const uint64_t np = ov_pieces(F, C, columns, fpc, piece);
        CHECK(np >= 1 && np * piece >= longest && (np == 1 || (np - 1) * piece < longest), "pieces %llu of %u for %llu",
              (unsigned long long)np, piece, (unsigned long long)longest);
    }
}

static void check_bands(void) {
    const uint64_t fs = 2048;
    const uint32_t sr = 44100, B = 1025;
    struct {
        float lo, mid;
        uint32_t b1, b2;
    } cases[] = {
        {0.0f, 0.0f, 0, 0},                    // both edges 0: everything is high
        {0.0f, 4000.0f, 0, 185},               // floor(4000 * 2048 / 44100) = floor(185.76)
        {250.0f, 4000.0f, 11, 185},            // floor(11.61)
        {21.533203125f, 43.06640625f, 1, 2},   // exactly on bins 1 and 2 (k * 44100 / 2048 is exact in f32)
        {43.06640625f, 43.06640625f, 2, 2},    // an empty mid band
        {22050.0f, 22050.0f, 1024, 1024},      // Nyquist: the last bin alone is high
        {22028.466796875f, 22050.0f, 1023, 1024},  // bin 1023 exactly: a mid band one bin wide
        {22050.0f, 30000.0f, 1024, 1025},      // mid above Nyquist: clamped to B, high empty
        {30000.0f, 1e30f, 1025, 1025},         // both above: everything is low
    };
    for (auto& c : cases) {
        uint32_t b1 = 99999, b2 = 99999;
        ov_band_bins(c.lo, c.mid, fs, sr, &b1, &b2);
        CHECK(b1 == c.b1 && b2 == c.b2, "edges %g %g: got %u %u want %u %u", c.lo, c.mid, b1, b2, c.b1, c.b2);
        // the header's formula, directly
        const double v1 = std::floor((double)c.lo * (double)fs / (double)sr), v2 = std::floor((double)c.mid * (double)fs / (double)sr);
        const uint32_t w1 = v1 >= B ? B : (uint32_t)v1;
        const uint32_t w2m = v2 >= B ? B : (uint32_t)v2;
        CHECK(b1 == w1 && b2 == (w2m < w1 ? w1 : w2m), "edges %g %g against the formula", c.lo, c.mid);
        CHECK(b1 <= b2 && b2 <= B, "order");
    }
    uint32_t b1, b2;
    ov_band_bins(100.0f, 200.0f, 1024, 22050, &b1, &b2);  // another frame size and rate
    CHECK(b1 == 4 && b2 == 9, "1024 / 22050: %u %u", b1, b2);
}

static void check_requests(void) {
    const float inf = INFINITY, nan = NAN;
    CHECK(overview_request_error(256, 0, 250.0f, 4000.0f) == nullptr, "columns form");
    CHECK(overview_request_error(0, 7, 0.0f, 0.0f) == nullptr, "frames form, zero edges");
    CHECK(overview_request_error(1, 0, 4000.0f, 4000.0f) == nullptr, "equal edges");
    CHECK(overview_request_error(0, 0, 250.0f, 4000.0f) != nullptr, "both zero");
    CHECK(overview_request_error(4, 4, 250.0f, 4000.0f) != nullptr, "both set");
    CHECK(overview_request_error(4, 0, nan, 4000.0f) != nullptr, "NaN low");
    CHECK(overview_request_error(4, 0, 250.0f, nan) != nullptr, "NaN mid");
    CHECK(overview_request_error(4, 0, 250.0f, inf) != nullptr, "inf mid");
    CHECK(overview_request_error(4, 0, -inf, 4000.0f) != nullptr, "-inf low");
    CHECK(overview_request_error(4, 0, -1.0f, 4000.0f) != nullptr, "negative low");
    CHECK(overview_request_error(4, 0, 0.0f, -1.0f) != nullptr, "negative mid");
    CHECK(overview_request_error(4, 0, 4000.0f, 250.0f) != nullptr, "low > mid");
}

int main(void) {
    const uint64_t Fs[] = {0, 1, 2, 63, 64, 65, 257, 15500};
    int cases = 0;
    for (uint64_t F : Fs) {
        const uint64_t cols[] = {1, 2, F - 1, F, F + 1, 1024};
        const uint64_t fpcs[] = {1, 3, 64, F, F + 1};
        for (uint64_t tail : {(uint64_t)0, (uint64_t)511})
            for (auto fh : {std::pair<uint64_t, uint64_t>{2048, 512}, {1024, 441}}) {
                if (tail >= fh.second) continue;
                for (uint64_t c : cols)
                    if (c >= 1 && c <= 0xFFFFFFFFull) check_plan(F, (uint32_t)c, 0, fh.first, fh.second, tail), cases++;
                for (uint64_t k : fpcs)
                    if (k >= 1) check_plan(F, 0, (uint32_t)k, fh.first, fh.second, tail), cases++;
            }
    }
    // the largest request fields against a long track: nothing wraps
    check_plan(15500, 0xFFFFFFFFu, 0, 2048, 512, 0);
    check_plan(15500, 0, 0xFFFFFFFFu, 2048, 512, 0);
    check_plan((uint64_t)1 << 24, 1000, 0, 2048, 512, 3);
    check_bands();
    check_requests();
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ok overview_plan %d cases\n", cases);
    return 0;
}
