// sections_core.hpp — the arithmetic of the sections request (include/stratum_hip.h, sdsp_sections),
// shared by the kernels (k_sections.hip), the host pipeline and the stand-alone host harness
// (tests/cpp/sections_core_test.cpp): the cell plan, the per-cell fold, the distance D, one cell's
// novelty, the boundary rule, section assembly, snapping and the request checks.  No HIP runtime
// call; every sum is a sequential f32 fold from 0 in ascending order.  Build with -ffp-contract=off.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/sdsp_libm.h"
#include "../../include/stratum_hip.h"

namespace sdsp {

constexpr uint32_t SC_KNOWN = SDSP_SECTIONS_LIST | SDSP_SECTIONS_CURVE;
constexpr uint32_t SC_KMAX = 64;  // the largest kernel_cells
constexpr int SC_TILE = 64;       // cells per block of k_section_novelty and k_section_pick
constexpr int SC_ROW = 13;        // floats per staged cell: m[0..12), then e (odd: LDS rows on distinct banks)

// ---- the cell plan (integers only) ----
// n_cells of a track with F key frames every khop and Fb base frames every hop
SD_HD uint64_t sc_cells(uint64_t F, uint64_t khop, uint64_t Fb, uint64_t hop, uint64_t Cs) {
    const uint64_t a = F * khop, b = Fb * hop;
    return Cs ? (a < b ? a : b) / Cs : 0;
}
// cell c owns the frames [sc_first(c), sc_first(c + 1)): those whose start f * hop lies in [c Cs, (c + 1) Cs)
SD_HD uint64_t sc_first(uint64_t c, uint64_t Cs, uint64_t hop) { return (c * Cs + hop - 1) / hop; }

// ---- the per-cell fold: the mean of x[f * stride] over the frames [f0, f1), f1 > f0 ----
SD_HD float sc_cell_mean(const float* x, uint64_t stride, uint64_t f0, uint64_t f1) {
    float s = 0.0f;
    for (uint64_t f = f0; f < f1; f++) s += x[f * stride];
    return s / (float)(f1 - f0);
}
SD_HD float sc_rel_energy(float g, float gmax) { return gmax > 0.0f ? g / gmax : 0.0f; }

// ---- distance and novelty over staged rows (SC_ROW floats per cell: m[0..12), e) ----
SD_HD float sc_D(const float* a, const float* b, float w) {
    float d = 0.0f;
    for (int i = 0; i < 12; i++) {
        const float t = a[i] - b[i];
        d += t * t;
    }
    const float te = a[12] - b[12];
    d += w * (te * te);
    return d;
}
// cross: a = c-K..c-1 (outer), b = c..c+K-1 (inner); c indexes `rows`
SD_HD float sc_cross(const float* rows, int64_t c, int K, float w) {
    float s = 0.0f;
    for (int64_t a = c - K; a < c; a++)
        for (int64_t b = c; b < c + K; b++) s += sc_D(rows + a * SC_ROW, rows + b * SC_ROW, w);
    return s;
}
// within [lo, lo + K): a = lo..lo+K-1, b = a+1..lo+K-1
SD_HD float sc_within(const float* rows, int64_t lo, int K, float w) {
    float s = 0.0f;
    for (int64_t a = lo; a < lo + K; a++)
        for (int64_t b = a + 1; b < lo + K; b++) s += sc_D(rows + a * SC_ROW, rows + b * SC_ROW, w);
    return s;
}
SD_HD float sc_combine(float cross, float wp, float wf, int K) {
    const float x = cross / (float)(K * K);
    return K > 1 ? x - (wp + wf) / (float)(K * (K - 1)) : x;
}
// whether cell c has a novelty of its own: c in [K, n_cells - K]
SD_HD bool sc_scored(uint64_t c, uint64_t n_cells, uint64_t K) { return n_cells >= 2 * K && c >= K && c <= n_cells - K; }
// N[c] of one cell over rows that hold [c - K, c + K) around index c
SD_HD float sc_novelty(const float* rows, int64_t c, int K, float w) {
    return sc_combine(sc_cross(rows, c, K, w), sc_within(rows, c - K, K, w), sc_within(rows, c, K, w), K);
}

// ---- the boundary rule over a track's N[0, n_cells) ----
SD_HD bool sc_is_boundary(const float* N, uint64_t n_cells, uint64_t c, uint64_t G, float min_strength, float nmax) {
    const float v = N[c];
    if (!(v > 0.0f) || !(v >= min_strength * nmax)) return false;
    const uint64_t lo = c > G ? c - G : 0;
    const uint64_t hi = n_cells - 1 - c > G ? c + G : n_cells - 1;
    for (uint64_t j = lo; j < c; j++)
        if (!(v > N[j])) return false;
    for (uint64_t j = c + 1; j <= hi; j++)
        if (!(v >= N[j])) return false;
    return true;
}

// ---- section assembly and snapping (host) ----
// the end of the section that starts at `start`: the next boundary, or n_cells
inline uint64_t sc_section_end(const uint8_t* boundary, uint64_t n_cells, uint64_t start) {
    uint64_t e = start + 1;
    while (e < n_cells && !boundary[e]) e++;
    return e;
}
inline float sc_time(uint64_t cell, uint64_t Cs, uint32_t sr) { return (float)(cell * Cs) / (float)sr; }
// the downbeat nearest to t (the first on a tie) when it lies within snap, else -1; *snapped its time, or t
inline int32_t sc_snap(const float* downs, uint64_t n, float t, float snap, float* snapped) {
    *snapped = t;
    int64_t best = -1;
    float bd = 0.0f;
    for (uint64_t j = 0; j < n; j++) {
        const float d = sd_absf(downs[j] - t);
        if (best < 0 || d < bd) best = (int64_t)j, bd = d;
    }
    if (best < 0 || best > INT32_MAX || !(bd <= snap)) return -1;
    *snapped = downs[best];
    return (int32_t)best;
}

// The sections of a track from its cell energies g, novelty N and boundary flags (n_cells > 0 of
// each): the runs between boundaries with their times, strength, mean and relative energy, and the
// snap of each start to the downbeats.
inline std::vector<sdsp_section> sc_assemble(const float* g, const float* N, const uint8_t* boundary, uint64_t n_cells,
                                             uint64_t Cs, uint32_t sr, const float* downs, uint64_t n_downs, float snap) {
    std::vector<sdsp_section> secs;
    float top = 0.0f;
    for (uint64_t s0 = 0; s0 < n_cells;) {
        const uint64_t s1 = sc_section_end(boundary, n_cells, s0);
        sdsp_section e{};
        e.start_cell = s0;
        e.end_cell = s1;
        e.start_time = sc_time(s0, Cs, sr);
        e.end_time = sc_time(s1, Cs, sr);
        e.strength = s0 ? N[s0] : 0.0f;
        e.mean_energy = sc_cell_mean(g, 1, s0, s1);
        e.downbeat = sc_snap(downs, n_downs, e.start_time, snap, &e.snapped_time);
        top = secs.empty() ? e.mean_energy : sd_maxf(top, e.mean_energy);
        secs.push_back(e);
        s0 = s1;
    }
    for (sdsp_section& e : secs) e.relative_energy = top > 0.0f ? e.mean_energy / top : 0.0f;
    return secs;
}

// ---- request checks (before any device is touched) ----
// The pairs of sdsp_request_set_ext past its base that the caller's struct_size covers (the caller's
// struct begins with `set`); the others stay NULL.
inline void request_set_ext_read(const sdsp_request_set* set, const sdsp_sections_request** sc_req,
                                 sdsp_sections** sections) {
    *sc_req = nullptr;
    *sections = nullptr;
    if (!set) return;
    const sdsp_request_set_ext* x = reinterpret_cast<const sdsp_request_set_ext*>(set);
    const size_t have = set->struct_size;
    if (have >= offsetof(sdsp_request_set_ext, sc_req) + sizeof(void*)) *sc_req = x->sc_req;
    if (have >= offsetof(sdsp_request_set_ext, sections) + sizeof(void*)) *sections = x->sections;
}
inline bool sc_bad_float(float x) { return !sd_isfinite_f(x) || x < 0.0f; }
// Why a request cannot run (NULL: it can) with the status to refuse it with, and its Cs.  khop, hop:
// the key STFT's and the base pass's hops; legacy: force_legacy_bpm; beat_rows: the chroma rows are
// beats (enable_key_beat_synchronous without enable_key_log_frequency).
inline const char* sections_request_error(const sdsp_sections_request& r, bool has_out, int32_t stages, uint32_t sr,
                                          uint64_t khop, uint64_t hop, bool legacy, bool beat_rows, uint64_t* Cs_out,
                                          int32_t* status) {
    *Cs_out = 0;
    *status = SDSP_ERR_INVALID_INPUT;
    if (r.what == 0) return "Invalid input: sections request with what == 0";
    if (r.what & ~SC_KNOWN) return "Invalid input: sections request with unknown bits";
    if (!has_out) return "Invalid input: sections request without a sections array";
    if (sc_bad_float(r.cell_seconds) || sc_bad_float(r.energy_weight) || sc_bad_float(r.min_strength) ||
        sc_bad_float(r.snap_seconds))
        return "Invalid input: sections request with a float that is not finite or is negative";
    const bool sec = r.cell_seconds != 0.0f, smp = r.cell_samples != 0;
    if (!sec && !smp) return "Invalid input: sections request sets neither cell_seconds nor cell_samples";
    if (sec && smp) return "Invalid input: sections request sets both cell_seconds and cell_samples";
    if (r.kernel_cells == 0 || r.kernel_cells > SC_KMAX) return "Invalid input: sections kernel_cells outside [1, 64]";
    if (r.min_gap_cells >= (1u << 31)) return "Invalid input: sections min_gap_cells of 2^31 or more";
    uint64_t Cs = r.cell_samples;
    if (sec) {
        const float p = r.cell_seconds * (float)sr;  // (>= 0 and not NaN here)
        Cs = p < 4294967296.0f ? (uint64_t)p : (uint64_t)1 << 32;
    }
    if (Cs >= ((uint64_t)1 << 31)) return "Invalid input: sections cell of 2^31 samples or more";
    if (Cs < khop || Cs < hop || Cs == 0) return "Invalid input: sections cell shorter than a hop (Cs < max(khop, hop_size))";
    if (stages == SDSP_STAGES_BPM_ONLY) return "Invalid input: sections request with SDSP_STAGES_BPM_ONLY (no key path)";
    *status = SDSP_ERR_NOT_IMPLEMENTED;
    if (legacy) return "Not implemented: sections with force_legacy_bpm (no feature pass, no frame energies)";
    if (beat_rows) return "Not implemented: sections with beat-synchronous chroma (the rows are beats, not frames)";
    *status = SDSP_OK;
    *Cs_out = Cs;
    return nullptr;
}

}  // namespace sdsp
