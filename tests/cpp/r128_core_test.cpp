// Host harness of stratum-dsp_amd/csrc/r128_core.hpp (tests/test_r128_core.py builds it with the
// address and undefined-behaviour sanitizers).  Without arguments: the request checks and the reading
// of the request sets of every generation.
//   layout          sizes and offsets of the public structs, for the ctypes mirrors
//   tracks <file>   every field of sdsp_r128 and both curves over the tracks of <file>, as bits, for
//                   tests/r128_ref.py to compare
// <file> (native endian): u32 sample rate, u32 what, u64 T; per track u64 n and n f32 samples.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stratum-dsp_amd/csrc/levels_core.hpp"
#include "../../stratum-dsp_amd/csrc/r128_core.hpp"
#include "../../stratum-dsp_amd/csrc/sections_core.hpp"

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

static void print_bits(const char* tag, const float* v, size_t n) {
    std::printf("%s %zu", tag, n);
    for (size_t i = 0; i < n; i++) std::printf(" %08x", sd_bits_f(v[i]));
    std::printf("\n");
}

static int run_tracks(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    const uint32_t sr = rd<uint32_t>(f), what = rd<uint32_t>(f);
    const uint64_t T = rd<uint64_t>(f);
    CHECK(r128_request_error(what, true, sr) == nullptr);
    const R128Params P = r128_params(sr);
    for (uint64_t t = 0; t < T; t++) {
        const uint64_t n = rd<uint64_t>(f);
        std::vector<float> x((size_t)n);
        if (n && std::fread(x.data(), sizeof(float), (size_t)n, f) != n) return 2;
        const uint64_t J = n / P.step;
        std::vector<float> z((size_t)J), m, s;
        R128Folds fo{};
        if (what & SDSP_R128_LOUDNESS) {
            for (uint64_t j = 0; j < J; j++) z[(size_t)j] = r128_step_energy(x.data(), j, P);
            fo = r128_folds(z.data(), J, P);
            for (uint64_t j = 0; j < r128_n_mom(J); j++) m.push_back(r128_momentary(z.data(), j, P.step));
            for (uint64_t j = 0; j < r128_n_short(J); j++) s.push_back(r128_short_term(z.data(), j, P.step));
        }
        float sp, tp;
        r128_peaks(x.data(), n, P, (what & SDSP_R128_TRUE_PEAK) != 0, &sp, &tp);
        sdsp_r128 o;
        r128_finish(fo, sp, tp, n, what, P, &o);
        std::printf("T %d %d %d %llu %u %llu %llu %llu %llu %llu\n", (int)o.status, (int)o.has_integrated, (int)o.has_range,
                    (unsigned long long)o.n_samples, o.step_samples, (unsigned long long)o.n_steps,
                    (unsigned long long)o.n_momentary, (unsigned long long)o.n_short_term,
                    (unsigned long long)o.n_gated_momentary, (unsigned long long)o.n_gated_short_term);
        const float fl[10] = {o.integrated_lufs, o.range_lu, o.range_low_lufs, o.range_high_lufs, o.max_momentary_lufs,
                              o.max_short_term_lufs, o.sample_peak, o.true_peak, o.sample_peak_db, o.true_peak_dbtp};
        print_bits("F", fl, 10);
        print_bits("C", o.shelf, 5);
        print_bits("H", o.highpass, 5);
        if (!(what & SDSP_R128_CURVES)) m.clear(), s.clear();
        print_bits("M", m.data(), m.size());
        print_bits("S", s.data(), s.size());
    }
    std::fclose(f);
    return fails ? 1 : 0;
}

static void layout() {
    std::printf("sdsp_r128_request %zu %zu\n", sizeof(sdsp_r128_request), offsetof(sdsp_r128_request, what));
#define O(k) offsetof(sdsp_r128, k)
    std::printf("sdsp_r128 %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n",
                sizeof(sdsp_r128), O(status), O(has_integrated), O(has_range), O(integrated_lufs), O(range_lu),
                O(range_low_lufs), O(range_high_lufs), O(max_momentary_lufs), O(max_short_term_lufs), O(sample_peak),
                O(true_peak), O(sample_peak_db), O(true_peak_dbtp), O(n_samples), O(step_samples), O(n_steps),
                O(n_momentary), O(n_short_term), O(n_gated_momentary), O(n_gated_short_term), O(shelf), O(highpass),
                O(momentary), O(short_term));
#undef O
    std::printf("sdsp_request_set_ext2 %zu %zu %zu %zu\n", sizeof(sdsp_request_set_ext2), offsetof(sdsp_request_set_ext2, base),
                offsetof(sdsp_request_set_ext2, r128_req), offsetof(sdsp_request_set_ext2, r128));
    std::printf("older %zu %zu\n", sizeof(sdsp_request_set), sizeof(sdsp_request_set_ext));
}

static void requests() {
    CHECK(r128_request_error(0, true, 44100) != nullptr);
    for (uint32_t w : {1u, 2u, 3u, 5u, 7u}) CHECK(r128_request_error(w, true, 44100) == nullptr);
    CHECK(r128_request_error(4, true, 44100) != nullptr);      // curves without loudness
    CHECK(r128_request_error(4 | 2, true, 44100) != nullptr);
    CHECK(r128_request_error(8, true, 44100) != nullptr);
    CHECK(r128_request_error(1 | 16, true, 44100) != nullptr);
    CHECK(r128_request_error(0x80000001u, true, 44100) != nullptr);
    CHECK(r128_request_error(1, false, 44100) != nullptr);
    CHECK(r128_request_error(1, true, 7999) != nullptr && r128_request_error(1, true, 0) != nullptr);
    CHECK(r128_request_error(1, true, 8000) == nullptr);

    sdsp_sections_request sc{};
    sdsp_sections s1{};
    sdsp_r128_request rq{SDSP_R128_LOUDNESS};
    sdsp_r128 r1{};
    sdsp_levels_request lv{SDSP_LEVELS_PEAK};
    sdsp_levels l1{};
    sdsp_request_set_ext2 in{};
    in.base.base.lv_req = &lv, in.base.base.levels = &l1;
    in.base.sc_req = &sc, in.base.sections = &s1;
    in.r128_req = &rq, in.r128 = &r1;
    const sdsp_request_set* set = &in.base.base;
    const sdsp_r128_request* q;
    sdsp_r128* o;
    const sdsp_sections_request* sq;
    sdsp_sections* so;
    sdsp_request_set plain;
    request_set_ext2_read(nullptr, &q, &o);
    CHECK(!q && !o);
    in.base.base.struct_size = (uint32_t)sizeof(in);
    request_set_ext2_read(set, &q, &o);
    request_set_ext_read(set, &sq, &so);
    CHECK(q == &rq && o == &r1 && sq == &sc && so == &s1);
    CHECK(request_set_read(set, &plain) == nullptr && plain.lv_req == &lv && plain.levels == &l1);
    // callers built against either older struct: the new pair reads as NULL
    in.base.base.struct_size = (uint32_t)sizeof(sdsp_request_set_ext);
    request_set_ext2_read(set, &q, &o);
    request_set_ext_read(set, &sq, &so);
    CHECK(!q && !o && sq == &sc && so == &s1);
    in.base.base.struct_size = (uint32_t)sizeof(sdsp_request_set);
    request_set_ext2_read(set, &q, &o);
    request_set_ext_read(set, &sq, &so);
    CHECK(!q && !o && !sq && !so);
    CHECK(request_set_read(set, &plain) == nullptr && plain.lv_req == &lv);
    // the request pointer alone is covered: the array reads as NULL (the caller is refused for it)
    in.base.base.struct_size = (uint32_t)(offsetof(sdsp_request_set_ext2, r128_req) + sizeof(void*));
    request_set_ext2_read(set, &q, &o);
    CHECK(q == &rq && !o);
    in.base.base.struct_size = (uint32_t)(offsetof(sdsp_request_set_ext2, r128_req) + sizeof(void*) - 1);
    request_set_ext2_read(set, &q, &o);
    CHECK(!q && !o);
    // a newer caller's larger struct: the fields this library knows
    in.base.base.struct_size = (uint32_t)sizeof(in) + 64;
    request_set_ext2_read(set, &q, &o);
    CHECK(q == &rq && o == &r1);
    // the pair lies right behind the older struct
    CHECK(offsetof(sdsp_request_set_ext2, r128_req) == sizeof(sdsp_request_set_ext));
}

static void ranks() {
    CHECK(r128_rank_low(1) == 0 && r128_rank_high(1) == 0);
    CHECK(r128_rank_low(2) == 0 && r128_rank_high(2) == 1);  // (95 + 50) / 100
    CHECK(r128_rank_low(11) == 1 && r128_rank_high(11) == 10);
    CHECK(r128_rank_low(101) == 10 && r128_rank_high(101) == 95);
    CHECK(r128_n_mom(3) == 0 && r128_n_mom(4) == 1 && r128_n_short(29) == 0 && r128_n_short(31) == 2);
    // the rank-counting select equals a sort, ties included
    const R128Params P = r128_params(8000);
    std::vector<float> z(64);
    for (size_t i = 0; i < z.size(); i++) z[i] = (float)((i * 7) % 5 + 1) * 1000.0f;
    const R128Folds f = r128_folds(z.data(), z.size(), P);
    std::vector<float> s;
    for (uint64_t j = 0; j < r128_n_short(z.size()); j++) s.push_back(r128_short_term(z.data(), j, P.step));
    for (size_t i = 1; i < s.size(); i++)
        for (size_t k = i; k > 0 && s[k] < s[k - 1]; k--) std::swap(s[k], s[k - 1]);
    CHECK(f.n_gated_short == s.size());  // (all far above both gates)
    CHECK(sd_bits_f(f.low) == sd_bits_f(s[(size_t)r128_rank_low(s.size())]));
    CHECK(sd_bits_f(f.high) == sd_bits_f(s[(size_t)r128_rank_high(s.size())]));
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "layout")) return layout(), 0;
    if (argc == 3 && !std::strcmp(argv[1], "tracks")) return run_tracks(argv[2]);
    requests();
    ranks();
    if (fails) return 1;
    std::printf("ok r128_core\n");
    return 0;
}
