// Host harness of stratum-dsp_amd/csrc/fingerprint_core.hpp (tests/test_fingerprint_core.py builds it
// with the address and undefined-behaviour sanitizers).  Without arguments: the request checks, the
// ordering rule and the struct reader.
//   layout          sizes and offsets of the public structs, for the ctypes mirrors
//   words <file>    every track of <file> through the core as the kernels use it: per track
//                   "T <n_cells> <n_words>", per cell "C" with the bits of m[0..12), then "W" with the words
//   match <file>    every call of <file>: "P <T>", per pair a < b "a b has o e n", then "M <n>" and per
//                   match "a b o offset_samples e bits <ber bits>"
// <file> (native endian), words: u64 N; per track u64 khop, Cs, F; F x 12 f32 rows.
// match: u64 N; per call u64 T, O, min_overlap, Cs; f32 max_ber; per track u64 first, W; W u32 words.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stratum-dsp_amd/csrc/fingerprint_core.hpp"

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
template <class T>
static std::vector<T> rd_n(FILE* f, uint64_t n) {
    std::vector<T> v((size_t)n);  // exactly sized: an overrun is the sanitizer's to report
    if (n && std::fread(v.data(), sizeof(T), (size_t)n, f) != n) {
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

static sdsp_fingerprint_request good() {
    sdsp_fingerprint_request r{};
    r.what = SDSP_FP_WORDS | SDSP_FP_MATCH;
    r.cell_samples = 5512;
    r.max_offset_words = 16;
    r.min_overlap_words = 32;
    r.max_ber = 0.3f;
    return r;
}
static int32_t refuse(const sdsp_fingerprint_request& r, bool has_out = true, bool has_m = true,
                      int32_t stages = SDSP_STAGES_FULL, uint64_t khop = 512, bool beat = false, uint64_t* cs = nullptr) {
    uint64_t Cs = 0;
    int32_t st = -1;
    const char* why = fingerprint_request_error(r, has_out, has_m, stages, 44100, khop, beat, &Cs, &st);
    CHECK((why == nullptr) == (st == SDSP_OK));
    CHECK((why == nullptr) == (Cs != 0));
    if (cs) *cs = Cs;
    return st;
}

static void self_checks() {
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    uint64_t Cs = 0;
    CHECK(refuse(good(), true, true, SDSP_STAGES_FULL, 512, false, &Cs) == SDSP_OK && Cs == 5512);
    sdsp_fingerprint_request r = good();
    r.cell_samples = 0;
    r.cell_seconds = 0.125f;
    CHECK(refuse(r, true, true, SDSP_STAGES_FULL, 512, false, &Cs) == SDSP_OK && Cs == 5512);
    r.cell_samples = 5512;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);  // both forms
    r = good(), r.cell_samples = 0;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);  // neither
    for (float v : {inf, nan, -0.5f, 1e9f}) {
        r = good(), r.cell_samples = 0, r.cell_seconds = v;
        CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    }
    for (float v : {inf, nan, -0.1f, 1.5f}) {
        r = good(), r.max_ber = v;
        CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    }
    r = good(), r.max_ber = 1.0f, r.max_offset_words = 255, r.min_overlap_words = 0;
    CHECK(refuse(r) == SDSP_OK);
    r = good(), r.max_offset_words = 256;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    for (uint32_t w : {0u, 4u, 7u}) {
        r = good(), r.what = w;
        CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    }
    r = good(), r.cell_samples = 511;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    r.cell_samples = 512;
    CHECK(refuse(r) == SDSP_OK);
    r.cell_samples = (uint64_t)1 << 31;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    r.cell_samples = ((uint64_t)1 << 31) - 1;
    CHECK(refuse(r) == SDSP_OK);
    CHECK(refuse(good(), false) == SDSP_ERR_INVALID_INPUT);        // no output array
    CHECK(refuse(good(), true, false) == SDSP_ERR_INVALID_INPUT);  // SDSP_FP_MATCH without the matches struct
    r = good(), r.what = SDSP_FP_WORDS;
    CHECK(refuse(r, true, false) == SDSP_OK);
    CHECK(refuse(good(), true, true, SDSP_STAGES_BPM_ONLY) == SDSP_ERR_INVALID_INPUT);
    CHECK(refuse(good(), true, true, SDSP_STAGES_FULL, 512, true) == SDSP_ERR_NOT_IMPLEMENTED);
    CHECK(refuse(good(), true, true, SDSP_STAGES_FULL, 8192) == SDSP_ERR_INVALID_INPUT);  // Cs < khop

    // the plan
    CHECK(fp_cells(10, 512, 1024) == 5 && fp_cells(0, 512, 1024) == 0 && fp_cells(43, 512, 22050) == 0 &&
          fp_cells(44, 512, 22050) == 1);
    CHECK(fp_words(0) == 0 && fp_words(2) == 0 && fp_words(3) == 1 && fp_words(300) == 298);
    // the order: the smaller e / n, then the smaller |o|, then the negative offset
    CHECK(fp_before(1, 3, 5, 2, 5, 0) && !fp_before(2, 5, 0, 1, 3, 5));
    CHECK(fp_before(0, 7, -2, 0, 9, 2) && !fp_before(0, 9, 2, 0, 7, -2));
    CHECK(fp_before(2, 4, 1, 1, 2, -3) && fp_before(1, 2, 0, 2, 4, -1));
    CHECK(fp_before(0xFFFFFFFFu, 0xFFFFFFFFu, 1, 0xFFFFFFFFu, 0xFFFFFFFEu, 0));  // the products need 64 bits
    const FpRec none{0, 0, 0, 0}, some{3, 1, 5, 9};
    CHECK(fp_rec_before(some, none) && !fp_rec_before(none, some) && !fp_rec_before(none, none));
    CHECK(fp_min_overlap(0) == 1 && fp_min_overlap(1) == 1 && fp_min_overlap(7) == 7);
    CHECK(fp_offset_samples(100, 40, -4, 5512) == 40 - 4 * 5512 - 100 && fp_offset_samples(0, 7, 2, 10) == 27);
    CHECK(bits(fp_ber(6, 3)) == bits(6.0f / 72.0f) && fp_is_match(some, 1.0f) && !fp_is_match(none, 1.0f));

    // the struct reader: a field is read only when struct_size covers it
    sdsp_request_set_ext3 x{};
    sdsp_fingerprint_request q = good();
    sdsp_fingerprint out{};
    sdsp_fingerprint_matches ms{};
    x.fp_req = &q, x.fingerprints = &out, x.fp_matches = &ms;
    const sdsp_fingerprint_request* a = nullptr;
    sdsp_fingerprint* b = nullptr;
    sdsp_fingerprint_matches* c = nullptr;
    sdsp_request_set& base = x.base.base.base;
    base.struct_size = sizeof(x);
    request_set_ext3_read(&base, &a, &b, &c);
    CHECK(a == &q && b == &out && c == &ms);
    base.struct_size = sizeof(sdsp_request_set_ext2);
    request_set_ext3_read(&base, &a, &b, &c);
    CHECK(!a && !b && !c);
    base.struct_size = sizeof(x) - sizeof(void*);
    request_set_ext3_read(&base, &a, &b, &c);
    CHECK(a == &q && b == &out && !c);
    request_set_ext3_read(nullptr, &a, &b, &c);
    CHECK(!a && !b && !c);
}

static void layout() {
#define OFF(T, f) (unsigned long long)offsetof(T, f)
    std::printf("sdsp_fingerprint_request %zu %llu %llu %llu %llu %llu %llu\n", sizeof(sdsp_fingerprint_request),
                OFF(sdsp_fingerprint_request, what), OFF(sdsp_fingerprint_request, cell_seconds),
                OFF(sdsp_fingerprint_request, cell_samples), OFF(sdsp_fingerprint_request, max_offset_words),
                OFF(sdsp_fingerprint_request, min_overlap_words), OFF(sdsp_fingerprint_request, max_ber));
    std::printf("sdsp_fingerprint %zu %llu %llu %llu %llu %llu %llu %llu\n", sizeof(sdsp_fingerprint),
                OFF(sdsp_fingerprint, status), OFF(sdsp_fingerprint, n_cells), OFF(sdsp_fingerprint, n_words),
                OFF(sdsp_fingerprint, cell_samples), OFF(sdsp_fingerprint, first_sample), OFF(sdsp_fingerprint, n_matches),
                OFF(sdsp_fingerprint, words));
    std::printf("sdsp_fingerprint_match %zu %llu %llu %llu %llu %llu %llu %llu\n", sizeof(sdsp_fingerprint_match),
                OFF(sdsp_fingerprint_match, a), OFF(sdsp_fingerprint_match, b), OFF(sdsp_fingerprint_match, offset_words),
                OFF(sdsp_fingerprint_match, offset_samples), OFF(sdsp_fingerprint_match, bit_errors),
                OFF(sdsp_fingerprint_match, bits_compared), OFF(sdsp_fingerprint_match, ber));
    std::printf("sdsp_fingerprint_matches %zu %llu %llu %llu %llu\n", sizeof(sdsp_fingerprint_matches),
                OFF(sdsp_fingerprint_matches, n_compared), OFF(sdsp_fingerprint_matches, n_pairs),
                OFF(sdsp_fingerprint_matches, n_matches), OFF(sdsp_fingerprint_matches, matches));
    std::printf("sdsp_request_set_ext3 %zu %llu %llu %llu %llu\n", sizeof(sdsp_request_set_ext3),
                OFF(sdsp_request_set_ext3, base), OFF(sdsp_request_set_ext3, fp_req), OFF(sdsp_request_set_ext3, fingerprints),
                OFF(sdsp_request_set_ext3, fp_matches));
#undef OFF
}

static void words(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) std::exit(2);
    const uint64_t N = rd<uint64_t>(f);
    for (uint64_t t = 0; t < N; t++) {
        const uint64_t khop = rd<uint64_t>(f), Cs = rd<uint64_t>(f), F = rd<uint64_t>(f);
        const std::vector<float> rows = rd_n<float>(f, F * 12);
        const uint64_t nc = fp_cells(F, khop, Cs), W = fp_words(nc);
        std::vector<float> m((size_t)nc * 12);
        for (uint64_t c = 0; c < nc; c++)
            for (int i = 0; i < 12; i++)  // as k_fp_cells: one (cell, pitch class) each
                m[(size_t)c * 12 + i] = sc_cell_mean(rows.data() + i, 12, sc_first(c, Cs, khop), sc_first(c + 1, Cs, khop));
        std::vector<uint32_t> w((size_t)W);
        for (uint64_t k = 0; k < W; k++) w[(size_t)k] = fp_word(&m[(size_t)k * 12], &m[(size_t)k * 12 + 12], &m[(size_t)k * 12 + 24]);
        std::printf("T %llu %llu\n", (unsigned long long)nc, (unsigned long long)W);
        for (uint64_t c = 0; c < nc; c++) {
            std::printf("C");
            for (int i = 0; i < 12; i++) std::printf(" %08x", bits(m[(size_t)c * 12 + i]));
            std::printf("\n");
        }
        std::printf("W");
        for (uint32_t v : w) std::printf(" %08x", v);
        std::printf("\n");
    }
    std::fclose(f);
}

static void match(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) std::exit(2);
    const uint64_t N = rd<uint64_t>(f);
    for (uint64_t k = 0; k < N; k++) {
        const uint64_t T = rd<uint64_t>(f), O = rd<uint64_t>(f), mo = rd<uint64_t>(f), Cs = rd<uint64_t>(f);
        const float max_ber = rd<float>(f);
        std::vector<std::vector<uint32_t>> w;
        std::vector<uint64_t> first, who;
        for (uint64_t t = 0; t < T; t++) {
            first.push_back(rd<uint64_t>(f));
            w.push_back(rd_n<uint32_t>(f, rd<uint64_t>(f)));
            who.push_back(t);
        }
        std::vector<FpRec> rec((size_t)(T * T), FpRec{0, 0, 0, 0});
        std::printf("P %llu\n", (unsigned long long)T);
        for (uint64_t a = 0; a < T; a++)
            for (uint64_t b = a + 1; b < T; b++) {
                const FpRec r = fp_best(w[a].data(), w[a].size(), w[b].data(), w[b].size(), (uint32_t)O, (uint32_t)mo);
                rec[(size_t)(a * T + b)] = r;
                std::printf("%llu %llu %u %d %u %u\n", (unsigned long long)a, (unsigned long long)b, r.has, r.o, r.e, r.n);
            }
        // in two bands, as the pipeline takes them
        std::vector<sdsp_fingerprint_match> ms;
        const size_t half = (size_t)(T / 2);
        fp_assemble(rec.data(), who, 0, half, first.data(), Cs, max_ber, &ms);
        fp_assemble(rec.data() + half * T, who, half, (size_t)T, first.data(), Cs, max_ber, &ms);
        std::printf("M %zu\n", ms.size());
        for (const sdsp_fingerprint_match& m : ms)
            std::printf("%llu %llu %d %lld %llu %llu %08x\n", (unsigned long long)m.a, (unsigned long long)m.b, m.offset_words,
                        (long long)m.offset_samples, (unsigned long long)m.bit_errors, (unsigned long long)m.bits_compared,
                        bits(m.ber));
    }
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "layout")) {
        layout();
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "words")) {
        words(argv[2]);
        return fails ? 1 : 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "match")) {
        match(argv[2]);
        return fails ? 1 : 0;
    }
    self_checks();
    std::printf(fails ? "FAILED fingerprint_core\n" : "ok fingerprint_core\n");
    return fails ? 1 : 0;
}
