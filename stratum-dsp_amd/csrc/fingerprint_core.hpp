// fingerprint_core.hpp — the arithmetic of the fingerprint request (include/stratum_hip.h,
// sdsp_fingerprint), shared by the kernels (k_fingerprint.hip), the host pipeline and the stand-alone
// host harness (tests/cpp/fingerprint_core_test.cpp): the word of three cell rows, n(o) and e(o) of
// one offset, the best-offset and match rules, offset_samples, list assembly and the request checks.
// The cell plan and the per-cell fold are sections_core.hpp's (sc_cells, sc_first, sc_cell_mean).
// No HIP runtime call.  Build with -ffp-contract=off.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/sdsp_libm.h"
#include "../../include/stratum_hip.h"
#include "sections_core.hpp"

namespace sdsp {

constexpr uint32_t FP_KNOWN = SDSP_FP_WORDS | SDSP_FP_MATCH;
constexpr uint32_t FP_OMAX = 255;               // the largest max_offset_words
constexpr uint64_t FP_WMAX = (uint64_t)1 << 27; // words per track the u32 error count holds (24 W < 2^32)

// ---- the plan (integers only): the sections request's cell rule over key frames alone ----
SD_HD uint64_t fp_cells(uint64_t F, uint64_t khop, uint64_t Cs) { return sc_cells(F, khop, F, khop, Cs); }
SD_HD uint64_t fp_words(uint64_t n_cells) { return n_cells >= 3 ? n_cells - 2 : 0; }

// ---- the word of three consecutive cell rows m[w], m[w + 1], m[w + 2] (12 floats each) ----
SD_HD uint32_t fp_word(const float* r0, const float* r1, const float* r2) {
    uint32_t word = 0;
    for (int i = 0; i < 12; i++) {
        const int j = i == 11 ? 0 : i + 1;
        const float d0 = r0[i] - r0[j], d1 = r1[i] - r1[j], d2 = r2[i] - r2[j];
        if (d1 - d0 > 0.0f) word |= 1u << i;
        if (d2 - d0 > 0.0f) word |= 1u << (12 + i);
    }
    return word;
}

// ---- one pair at one offset ----
SD_HD uint32_t fp_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }
// the positions of offset o: [fp_lo(o), fp_hi(Wa, Wb, o)), empty when hi <= lo
SD_HD int64_t fp_lo(int64_t o) { return o < 0 ? -o : 0; }
SD_HD int64_t fp_hi(int64_t Wa, int64_t Wb, int64_t o) { return Wa < Wb - o ? Wa : Wb - o; }
// whether position p with the words a = A[p], b = B[p + o] is counted, and its bit errors
SD_HD bool fp_counted(uint32_t a, uint32_t b) { return (a | b) != 0; }
SD_HD void fp_count(const uint32_t* A, uint64_t Wa, const uint32_t* B, uint64_t Wb, int32_t o, uint64_t* e, uint64_t* n) {
    uint64_t ee = 0, nn = 0;
    const int64_t hi = fp_hi((int64_t)Wa, (int64_t)Wb, o);
    for (int64_t p = fp_lo(o); p < hi; p++) {
        const uint32_t a = A[p], b = B[p + o];
        if (!fp_counted(a, b)) continue;
        nn++;
        ee += fp_popc(a ^ b);
    }
    *e = ee;
    *n = nn;
}

// ---- the best offset ----
// A pair's record: its best offset with e and n there; has == 0 (and the rest 0) without an
// eligible offset.  The dense output of k_fp_match and of sdsp_debug_fingerprint_match.
struct FpRec {
    int32_t o;
    uint32_t has, e, n;
};
// whether (e1, n1, o1) comes before (e2, n2, o2): the smaller e / n, then the smaller |o|, then the
// negative offset.  n1, n2 > 0.  A strict total order over distinct offsets, so a reduction in any
// order finds the same record.
SD_HD bool fp_before(uint32_t e1, uint32_t n1, int32_t o1, uint32_t e2, uint32_t n2, int32_t o2) {
    const uint64_t l = (uint64_t)e1 * n2, r = (uint64_t)e2 * n1;
    if (l != r) return l < r;
    const int32_t a1 = o1 < 0 ? -o1 : o1, a2 = o2 < 0 ? -o2 : o2;
    if (a1 != a2) return a1 < a2;
    return o1 < o2;
}
SD_HD bool fp_rec_before(const FpRec& x, const FpRec& y) {
    if (!x.has || !y.has) return x.has && !y.has;
    return fp_before(x.e, x.n, x.o, y.e, y.n, y.o);
}
SD_HD uint32_t fp_min_overlap(uint32_t min_overlap_words) { return min_overlap_words > 1 ? min_overlap_words : 1; }
SD_HD FpRec fp_best(const uint32_t* A, uint64_t Wa, const uint32_t* B, uint64_t Wb, uint32_t O, uint32_t min_overlap_words) {
    FpRec best{0, 0, 0, 0};
    const uint32_t need = fp_min_overlap(min_overlap_words);
    for (int32_t o = -(int32_t)O; o <= (int32_t)O; o++) {
        uint64_t e, n;
        fp_count(A, Wa, B, Wb, o, &e, &n);
        if (n < need) continue;
        const FpRec c{o, 1, (uint32_t)e, (uint32_t)n};
        if (fp_rec_before(c, best)) best = c;
    }
    return best;
}
SD_HD float fp_ber(uint32_t e, uint32_t n) { return (float)e / (float)((uint64_t)24 * n); }
SD_HD bool fp_is_match(const FpRec& r, float max_ber) { return r.has && fp_ber(r.e, r.n) <= max_ber; }
// sample s of a's caller buffer meets sample s + offset_samples of b's
SD_HD int64_t fp_offset_samples(uint64_t first_a, uint64_t first_b, int32_t o, uint64_t Cs) {
    return ((int64_t)first_b + (int64_t)o * (int64_t)Cs) - (int64_t)first_a;
}

// ---- list assembly (host) ----
// Appends to *out the matches of a band of dense records: `who` the compared tracks' indices in the
// call, ascending; the band holds the rows [r0, r1) of them, the pair of who[i], who[j] (i < j) at
// rec[(i - r0) * who.size() + j]; first[t] each call track's trim start.  Bands taken in ascending
// order leave the list sorted by (a, b).
inline void fp_assemble(const FpRec* rec, const std::vector<uint64_t>& who, size_t r0, size_t r1, const uint64_t* first,
                        uint64_t Cs, float max_ber, std::vector<sdsp_fingerprint_match>* out) {
    const size_t NC = who.size();
    for (size_t i = r0; i < r1 && i < NC; i++)
        for (size_t j = i + 1; j < NC; j++) {
            const FpRec& r = rec[(i - r0) * NC + j];
            if (!fp_is_match(r, max_ber)) continue;
            sdsp_fingerprint_match m{};
            m.a = who[i];
            m.b = who[j];
            m.offset_words = r.o;
            m.offset_samples = fp_offset_samples(first[who[i]], first[who[j]], r.o, Cs);
            m.bit_errors = r.e;
            m.bits_compared = (uint64_t)24 * r.n;
            m.ber = fp_ber(r.e, r.n);
            out->push_back(m);
        }
}

// ---- request checks (before any device is touched) ----
// The fields of sdsp_request_set_ext3 past its base that the caller's struct_size covers (the
// caller's struct begins with `set`); the others stay NULL.
inline void request_set_ext3_read(const sdsp_request_set* set, const sdsp_fingerprint_request** req,
                                  sdsp_fingerprint** out, sdsp_fingerprint_matches** matches) {
    *req = nullptr;
    *out = nullptr;
    *matches = nullptr;
    if (!set) return;
    const sdsp_request_set_ext3* x = reinterpret_cast<const sdsp_request_set_ext3*>(set);
    const size_t have = set->struct_size;
    if (have >= offsetof(sdsp_request_set_ext3, fp_req) + sizeof(void*)) *req = x->fp_req;
    if (have >= offsetof(sdsp_request_set_ext3, fingerprints) + sizeof(void*)) *out = x->fingerprints;
    if (have >= offsetof(sdsp_request_set_ext3, fp_matches) + sizeof(void*)) *matches = x->fp_matches;
}
// Why a request cannot run (NULL: it can) with the status to refuse it with, and its Cs.  khop: the
// key STFT's hop; beat_rows: the chroma rows are beats (enable_key_beat_synchronous without
// enable_key_log_frequency).
inline const char* fingerprint_request_error(const sdsp_fingerprint_request& r, bool has_out, bool has_matches,
                                             int32_t stages, uint32_t sr, uint64_t khop, bool beat_rows, uint64_t* Cs_out,
                                             int32_t* status) {
    *Cs_out = 0;
    *status = SDSP_ERR_INVALID_INPUT;
    if (r.what == 0) return "Invalid input: fingerprint request with what == 0";
    if (r.what & ~FP_KNOWN) return "Invalid input: fingerprint request with unknown bits";
    if (!has_out) return "Invalid input: fingerprint request without a fingerprints array";
    if ((r.what & SDSP_FP_MATCH) && !has_matches) return "Invalid input: SDSP_FP_MATCH without a matches struct";
    if (sc_bad_float(r.cell_seconds) || sc_bad_float(r.max_ber))
        return "Invalid input: fingerprint request with a float that is not finite or is negative";
    if (r.max_ber > 1.0f) return "Invalid input: fingerprint max_ber above 1";
    const bool sec = r.cell_seconds != 0.0f, smp = r.cell_samples != 0;
    if (!sec && !smp) return "Invalid input: fingerprint request sets neither cell_seconds nor cell_samples";
    if (sec && smp) return "Invalid input: fingerprint request sets both cell_seconds and cell_samples";
    if (r.max_offset_words > FP_OMAX) return "Invalid input: fingerprint max_offset_words above 255";
    uint64_t Cs = r.cell_samples;
    if (sec) {
        const float p = r.cell_seconds * (float)sr;  // (>= 0 and not NaN here)
        Cs = p < 4294967296.0f ? (uint64_t)p : (uint64_t)1 << 32;
    }
    if (Cs >= ((uint64_t)1 << 31)) return "Invalid input: fingerprint cell of 2^31 samples or more";
    if (Cs < khop || Cs == 0) return "Invalid input: fingerprint cell shorter than the key hop (Cs < khop)";
    if (stages == SDSP_STAGES_BPM_ONLY) return "Invalid input: fingerprint request with SDSP_STAGES_BPM_ONLY (no key path)";
    *status = SDSP_ERR_NOT_IMPLEMENTED;
    if (beat_rows) return "Not implemented: fingerprint with beat-synchronous chroma (the rows are beats, not frames)";
    *status = SDSP_OK;
    *Cs_out = Cs;
    return nullptr;
}

}  // namespace sdsp
