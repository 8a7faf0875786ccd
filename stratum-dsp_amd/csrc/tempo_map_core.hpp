// tempo_map_core.hpp — the sequential arithmetic of the tempo map request (include/stratum_hip.h,
// sdsp_tempo_map) that the beat grid itself never needed, shared by the kernel (k_tempo_map.hip),
// the host pipeline and the stand-alone host harness (tests/cpp/tempo_map_core_test.cpp): one
// window of detect_tempo_variations with its confidence (tempo_variation.rs:130-199), the
// tracker's penalty and confidence (bayesian.rs:143-176), the signature pick with its confidence
// (time_signature.rs:120-149), the segment capacity and the request checks.  No HIP runtime call;
// every sum is the reference's sequential f32 fold.  Build with -ffp-contract=off.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sdsp_libm.h"
#include "../../include/stratum_hip.h"

namespace sdsp {

constexpr float TM_EPS = 1e-10f;  // `const EPSILON: f32 = 1e-10`
constexpr uint32_t TM_KNOWN = SDSP_TEMPO_MAP_SEGMENTS | SDSP_TEMPO_MAP_ONSETS;

// One segment as the kernel writes it (sdsp_tempo_segment with 32-bit flags).
struct TmSeg {
    float start, end, bpm, conf;
    uint32_t variable, updated, n_onsets;
    float ubpm, uconf;
    uint32_t n_beats;
};
// One track's map without its lists.  ok: 1 a grid, 0 none, -1 the segments outgrew their capacity.
struct TmOut {
    int32_t ok, has_var, refined, hmm_beats, bpb, ts_scored, n_seg;
    float ts_conf, score[3];
};

// tempo_variation.rs:186: confidence = max(1 - min(cv / 0.3, 1), 0)
SD_HD float tm_segment_confidence(float cv) { return sd_maxf(1.0f - sd_minf(cv / 0.3f, 1.0f), 0.0f); }

// One window of detect_tempo_variations over its beats b[i0, i1) (those in [start, end]): false
// when it emits nothing (fewer than 3 beats, or no positive interval), else bpm, confidence and
// is_variable (cv > 0.15), with the mean and the variance folded in beat order.
SD_HD bool tm_window(const float* b, int i0, int i1, float nominal, float* bpm, float* conf, bool* variable) {
    if (i1 - i0 < 3) return false;
    float sum = 0.0f;
    int cnt = 0;
    for (int k = i0 + 1; k < i1; k++) {
        const float d = b[k] - b[k - 1];
        if (d > 0.0f) {
            sum += d;
            cnt++;
        }
    }
    if (cnt == 0) return false;
    const float mean = sum / (float)cnt;
    float vs = 0.0f;
    for (int k = i0 + 1; k < i1; k++) {
        const float d = b[k] - b[k - 1];
        if (d > 0.0f) {
            const float dd = d - mean;
            vs += dd * dd;
        }
    }
    const float var = vs / (float)cnt;
    const float sd = __builtin_sqrtf(var);
    const float cv = mean > TM_EPS ? sd / mean : 0.0f;
    *bpm = mean > TM_EPS ? 60.0f / mean : nominal;
    *conf = tm_segment_confidence(cv);
    *variable = cv > 0.15f;
    return true;
}

// bayesian.rs:163-176: the tracker's confidence after an update that moved old_bpm to new_bpm with
// the winning likelihood best_l (0 when no candidate had a positive one)
SD_HD float tm_penalty(float change) { return change < 1.0f ? 1.0f : change < 3.0f ? 0.8f : 0.5f; }
SD_HD float tm_updated_confidence(float best_l, float old_bpm, float new_bpm) {
    return sd_minf(best_l * tm_penalty(sd_absf(new_bpm - old_bpm)), 1.0f);
}

// time_signature.rs:120-149 over the scores of 4/4, 3/4, 6/8: max_by(partial_cmp) keeps the LAST
// maximum; the confidence is the winning score clamped to [0, 1]
SD_HD void tm_pick_signature(const float sc[3], uint32_t* bpb, float* conf) {
    uint32_t best = 4;
    float bs = sc[0];
    if (!(sc[1] < bs)) {
        best = 3;
        bs = sc[1];
    }
    if (!(sc[2] < bs)) {
        best = 6;
        bs = sc[2];
    }
    *bpb = best;
    *conf = sd_clampf(bs, 0.0f, 1.0f);
}
// the fallback (fewer than 8 beats, or no positive interval): (4, 0.5), nothing scored
constexpr uint32_t TM_TS_FALLBACK_BPB = 4;
constexpr float TM_TS_FALLBACK_CONF = 0.5f;

// Segments a track of n_trim samples can have.  The windows start every step = seg_dur / 2 >= 2 s
// (seg_dur = clamp(span / 4, 4, 8)) from the first HMM beat while the start lies before the last
// one; the HMM beats lie on a grid over the onsets' span (< n_trim / sr) that ends less than one
// emission tolerance (0.054 s) past the last onset, so at most floor(n_trim / (2 sr)) + 2 windows
// start inside it.  Two more absorb the rounding of the f32 accumulation `cur += step`
// (tests/cpp/tempo_map_core_test.cpp sweeps it); the kernel refuses a track that would outgrow this.
SD_HD uint64_t tm_segment_capacity(uint64_t n_trim, uint32_t sr) {
    return n_trim / (2 * (uint64_t)(sr > 0 ? sr : 1)) + 4;
}

// ---- request checks (before any device is touched) ----
inline const char* tempo_map_request_error(uint32_t what, bool has_out, int32_t stages) {
    if (what == 0) return "Invalid input: tempo map request with what == 0";
    if (what & ~TM_KNOWN) return "Invalid input: tempo map request with unknown bits";
    if (!has_out) return "Invalid input: tempo map request without a tempo map array";
    if (stages == SDSP_STAGES_BPM_ONLY) return "Invalid input: tempo map request with SDSP_STAGES_BPM_ONLY (no beat stage)";
    return nullptr;
}

}  // namespace sdsp
