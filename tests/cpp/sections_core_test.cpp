// Host harness of stratum-dsp_amd/csrc/sections_core.hpp (tests/test_sections_core.py builds it with
// the address and undefined-behaviour sanitizers).  Without arguments: the request checks, the cell
// plan against a brute-force count, the boundary rule's ties and the snap.
//   layout          sizes and offsets of the public structs, for the ctypes mirrors
//   tracks <file>   every track of <file> through the core as the kernels and the host use it: per
//                   track "T <n_cells> <gmax bits> <nmax bits>", per cell "C" with the bits of m[0..12),
//                   g, N and the boundary flag, then "S <n>" and per section its fields (floats as bits)
// <file> (native endian): u64 T; per track u64 khop, hop, Cs, K, G; f32 w, min_strength, snap; u32 sr;
// u64 F, F x 12 f32 rows; u64 Fb, Fb f32 energies; u64 nd, nd f32 downbeats.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stratum-dsp_amd/csrc/levels_core.hpp"
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

static sdsp_sections_request good() {
    sdsp_sections_request r{};
    r.what = SDSP_SECTIONS_LIST | SDSP_SECTIONS_CURVE;
    r.cell_seconds = 0.5f;
    r.kernel_cells = 16;
    r.min_gap_cells = 8;
    r.energy_weight = 1.0f;
    r.min_strength = 0.5f;
    return r;
}
static int32_t refuse(const sdsp_sections_request& r, bool has_out = true, int32_t stages = SDSP_STAGES_FULL,
                      uint64_t khop = 512, uint64_t hop = 512, bool legacy = false, bool beat = false, uint64_t* cs = nullptr) {
    uint64_t Cs = 0;
    int32_t st = -1;
    const char* why = sections_request_error(r, has_out, stages, 44100, khop, hop, legacy, beat, &Cs, &st);
    CHECK((why == nullptr) == (st == SDSP_OK));
    CHECK((why == nullptr) == (Cs != 0));
    if (cs) *cs = Cs;
    return st;
}

static void self_checks() {
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    uint64_t Cs = 0;
    CHECK(refuse(good(), true, SDSP_STAGES_FULL, 512, 512, false, false, &Cs) == SDSP_OK && Cs == 22050);
    sdsp_sections_request r = good();
    r.cell_samples = 22050;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);  // both forms
    r.cell_seconds = 0.0f;
    CHECK(refuse(r, true, SDSP_STAGES_FULL, 512, 512, false, false, &Cs) == SDSP_OK && Cs == 22050);
    r.cell_samples = 0;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);  // neither
    for (float bad : {inf, nan, -1.0f}) {
        for (int k = 0; k < 4; k++) {
            r = good();
            (k == 0 ? r.cell_seconds : k == 1 ? r.energy_weight : k == 2 ? r.min_strength : r.snap_seconds) = bad;
            CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
        }
    }
    r = good(), r.what = 0;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    r = good(), r.what = 4;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    r = good(), r.kernel_cells = 0;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    r = good(), r.kernel_cells = 65;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    r = good(), r.kernel_cells = 64, r.min_gap_cells = 0x7FFFFFFFu;
    CHECK(refuse(r) == SDSP_OK);
    r.min_gap_cells = 0x80000000u;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    r = good(), r.cell_seconds = 0.0f, r.cell_samples = 511;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    r.cell_samples = 600;
    CHECK(refuse(r) == SDSP_OK && refuse(r, true, SDSP_STAGES_FULL, 256, 1024) == SDSP_ERR_INVALID_INPUT);
    r.cell_samples = (uint64_t)1 << 31;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    r.cell_samples = ((uint64_t)1 << 31) - 1;
    CHECK(refuse(r) == SDSP_OK);
    r = good(), r.cell_seconds = 1e9f;
    CHECK(refuse(r) == SDSP_ERR_INVALID_INPUT);
    CHECK(refuse(good(), false) == SDSP_ERR_INVALID_INPUT);
    CHECK(refuse(good(), true, SDSP_STAGES_BPM_ONLY) == SDSP_ERR_INVALID_INPUT);
    CHECK(refuse(good(), true, SDSP_STAGES_FULL, 512, 512, true) == SDSP_ERR_NOT_IMPLEMENTED);
    CHECK(refuse(good(), true, SDSP_STAGES_FULL, 512, 512, false, true) == SDSP_ERR_NOT_IMPLEMENTED);

    // the plan against a brute-force count of the frames whose start lies in each cell
    for (uint64_t Cs2 : {512ull, 513ull, 700ull, 22050ull})
        for (uint64_t hop : {256ull, 512ull}) {
            if (Cs2 < hop) continue;
            const uint64_t F = 1000, n = sc_cells(F, hop, F, hop, Cs2);
            CHECK(n == F * hop / Cs2);
            for (uint64_t c = 0; c < n; c++) {
                uint64_t lo = F, cnt = 0;
                for (uint64_t f = 0; f < F; f++)
                    if (f * hop >= c * Cs2 && f * hop < (c + 1) * Cs2) lo = lo < f ? lo : f, cnt++;
                CHECK(cnt >= 1 && sc_first(c, Cs2, hop) == lo && sc_first(c + 1, Cs2, hop) == lo + cnt);
            }
        }
    CHECK(sc_cells(10, 512, 3, 512, 1024) == 1 && sc_cells(0, 512, 9, 512, 512) == 0);

    // the boundary rule: the first of two equal peaks within G wins; strict before, not after
    std::vector<float> N(30, 0.0f);
    N[10] = N[13] = 2.0f;
    CHECK(sc_is_boundary(N.data(), 30, 10, 8, 0.5f, 2.0f) && !sc_is_boundary(N.data(), 30, 13, 8, 0.5f, 2.0f));
    CHECK(sc_is_boundary(N.data(), 30, 13, 2, 0.5f, 2.0f) && sc_is_boundary(N.data(), 30, 13, 0, 0.5f, 2.0f));
    CHECK(!sc_is_boundary(N.data(), 30, 11, 0, 0.0f, 2.0f));  // N == 0 is never a boundary
    N[20] = 0.9f;
    CHECK(!sc_is_boundary(N.data(), 30, 20, 2, 0.5f, 2.0f) && sc_is_boundary(N.data(), 30, 20, 2, 0.25f, 2.0f));
    CHECK(sc_is_boundary(N.data(), 30, 10, 0x7FFFFFFFu, 0.5f, 2.0f));  // a gap past both ends
    N[29] = 3.0f;
    CHECK(sc_is_boundary(N.data(), 30, 29, 5, 1.0f, 3.0f) && !sc_is_boundary(N.data(), 30, 10, 0x7FFFFFFFu, 0.0f, 3.0f));

    // the snap: nearest, the first on a tie, inclusive distance
    const float downs[4] = {0.5f, 2.0f, 4.0f, 6.0f};
    float s = 0.0f;
    CHECK(sc_snap(downs, 4, 3.0f, 1.5f, &s) == 1 && s == 2.0f);
    CHECK(sc_snap(downs, 4, 3.0f, 1.0f, &s) == 1 && s == 2.0f);
    CHECK(sc_snap(downs, 4, 3.0f, 0.5f, &s) == -1 && s == 3.0f);
    CHECK(sc_snap(downs, 0, 1.0f, 9.0f, &s) == -1 && s == 1.0f);
    CHECK(sc_snap(nullptr, 0, 1.0f, 9.0f, &s) == -1);

    // request_set_ext_read: a caller built before the sections pair (a plain sdsp_request_set) reads as NULL
    sdsp_request_set_ext in{};
    sdsp_request_set out;
    sdsp_sections_request q = good();
    sdsp_sections dummy{};
    const sdsp_sections_request* rq = nullptr;
    sdsp_sections* rs = nullptr;
    in.sc_req = &q;
    in.sections = &dummy;
    in.base.struct_size = (uint32_t)sizeof(in);
    CHECK(request_set_read(&in.base, &out) == nullptr && out.struct_size == sizeof(sdsp_request_set));
    request_set_ext_read(&in.base, &rq, &rs);
    CHECK(rq == &q && rs == &dummy);
    in.base.struct_size = (uint32_t)sizeof(sdsp_request_set);
    request_set_ext_read(&in.base, &rq, &rs);
    CHECK(rq == nullptr && rs == nullptr);
    in.base.struct_size = (uint32_t)(offsetof(sdsp_request_set_ext, sc_req) + sizeof(void*));
    request_set_ext_read(&in.base, &rq, &rs);
    CHECK(rq == &q && rs == nullptr);
    request_set_ext_read(nullptr, &rq, &rs);
    CHECK(rq == nullptr && rs == nullptr);
    static_assert(offsetof(sdsp_request_set_ext, base) == 0 && offsetof(sdsp_request_set_ext, sc_req) == sizeof(sdsp_request_set),
                  "the fifth pair lies right at the end of sdsp_request_set");
}

static int layout() {
    std::printf("sdsp_sections_request %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sdsp_sections_request),
                offsetof(sdsp_sections_request, what), offsetof(sdsp_sections_request, cell_seconds),
                offsetof(sdsp_sections_request, cell_samples), offsetof(sdsp_sections_request, kernel_cells),
                offsetof(sdsp_sections_request, min_gap_cells), offsetof(sdsp_sections_request, energy_weight),
                offsetof(sdsp_sections_request, min_strength), offsetof(sdsp_sections_request, snap_seconds));
    std::printf("sdsp_section %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sdsp_section),
                offsetof(sdsp_section, start_cell), offsetof(sdsp_section, end_cell), offsetof(sdsp_section, start_time),
                offsetof(sdsp_section, end_time), offsetof(sdsp_section, strength), offsetof(sdsp_section, mean_energy),
                offsetof(sdsp_section, relative_energy), offsetof(sdsp_section, snapped_time),
                offsetof(sdsp_section, downbeat));
    std::printf("sdsp_sections %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sdsp_sections),
                offsetof(sdsp_sections, status), offsetof(sdsp_sections, n_cells), offsetof(sdsp_sections, cell_samples),
                offsetof(sdsp_sections, first_sample), offsetof(sdsp_sections, gmax), offsetof(sdsp_sections, nmax),
                offsetof(sdsp_sections, n_sections), offsetof(sdsp_sections, sections), offsetof(sdsp_sections, n_curve),
                offsetof(sdsp_sections, novelty), offsetof(sdsp_sections, energy));
    std::printf("sdsp_request_set_ext %zu %zu %zu %zu\n", sizeof(sdsp_request_set_ext), offsetof(sdsp_request_set_ext, base),
                offsetof(sdsp_request_set_ext, sc_req), offsetof(sdsp_request_set_ext, sections));
    return 0;
}

static int tracks(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::printf("FAIL cannot open %s\n", path);
        return 2;
    }
    const uint64_t T = rd<uint64_t>(f);
    for (uint64_t t = 0; t < T; t++) {
        const uint64_t khop = rd<uint64_t>(f), hop = rd<uint64_t>(f), Cs = rd<uint64_t>(f), K = rd<uint64_t>(f),
                       G = rd<uint64_t>(f);
        const float w = rd<float>(f), min_strength = rd<float>(f), snap = rd<float>(f);
        const uint32_t sr = rd<uint32_t>(f);
        const uint64_t F = rd<uint64_t>(f);
        const std::vector<float> rows = rd_f32(f, F * 12);
        const uint64_t Fb = rd<uint64_t>(f);
        const std::vector<float> E = rd_f32(f, Fb);
        const uint64_t nd = rd<uint64_t>(f);
        const std::vector<float> downs = rd_f32(f, nd);
        const uint64_t n = sc_cells(F, khop, Fb, hop, Cs);
        // exactly sized arrays, so that a read past a cell's frames or past the halo is an ASan error
        std::vector<float> m((size_t)n * 12), g((size_t)n), N((size_t)n, 0.0f), st((size_t)n * SC_ROW);
        std::vector<uint8_t> b((size_t)n, 0);
        for (uint64_t c = 0; c < n; c++) {
            for (int i = 0; i < 12; i++)
                m[(size_t)c * 12 + i] = sc_cell_mean(rows.data() + i, 12, sc_first(c, Cs, khop), sc_first(c + 1, Cs, khop));
            g[(size_t)c] = sc_cell_mean(E.data(), 1, sc_first(c, Cs, hop), sc_first(c + 1, Cs, hop));
        }
        float gmax = 0.0f, nmax = 0.0f;
        for (uint64_t c = 0; c < n; c++) gmax = c ? sd_maxf(gmax, g[(size_t)c]) : g[0];
        for (uint64_t c = 0; c < n; c++) {
            for (int i = 0; i < 12; i++) st[(size_t)c * SC_ROW + i] = m[(size_t)c * 12 + i];
            st[(size_t)c * SC_ROW + 12] = sc_rel_energy(g[(size_t)c], gmax);
        }
        for (uint64_t c = 0; c < n; c++)
            if (sc_scored(c, n, K)) N[(size_t)c] = sc_novelty(st.data(), (int64_t)c, (int)K, w);
        for (uint64_t c = 0; c < n; c++) nmax = c ? sd_maxf(nmax, N[(size_t)c]) : N[0];
        for (uint64_t c = 0; c < n; c++) b[(size_t)c] = sc_is_boundary(N.data(), n, c, G, min_strength, nmax) ? 1 : 0;
        std::printf("T %llu %08x %08x\n", (unsigned long long)n, bits(gmax), bits(nmax));
        for (uint64_t c = 0; c < n; c++) {
            std::printf("C");
            for (int i = 0; i < 12; i++) std::printf(" %08x", bits(m[(size_t)c * 12 + i]));
            std::printf(" %08x %08x %d\n", bits(g[(size_t)c]), bits(N[(size_t)c]), (int)b[(size_t)c]);
        }
        std::vector<sdsp_section> secs;
        if (n) secs = sc_assemble(g.data(), N.data(), b.data(), n, Cs, sr, downs.data(), nd, snap);
        std::printf("S %zu\n", secs.size());
        for (const sdsp_section& e : secs)
            std::printf("%llu %llu %08x %08x %08x %08x %08x %08x %d\n", (unsigned long long)e.start_cell,
                        (unsigned long long)e.end_cell, bits(e.start_time), bits(e.end_time), bits(e.strength),
                        bits(e.mean_energy), bits(e.relative_energy), bits(e.snapped_time), e.downbeat);
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "layout") == 0) return layout();
    if (argc >= 3 && std::strcmp(argv[1], "tracks") == 0) return tracks(argv[2]);
    self_checks();
    if (fails) return 1;
    std::printf("ok sections_core\n");
    return 0;
}
