// levels_core.hpp — the arithmetic of the levels request (include/stratum_hip.h, sdsp_levels), shared
// by the kernels (k_levels.hip), the host pipeline and the stand-alone host harness
// (tests/cpp/levels_core_test.cpp): the fold steps, the folds -> sdsp_loudness of each method
// (normalization.rs:262-470), the silence map's keep-rule (silence.rs:183-231) and the request checks.
// No HIP runtime call; every log and pow is sdsp_libm.h's, every sum the reference's sequential f32
// fold.  Build with -ffp-contract=off: the folds must not become FMAs.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sdsp_libm.h"
#include "../../include/stratum_hip.h"

namespace sdsp {

constexpr float LV_EPS = 1e-10f;  // normalization.rs:87
constexpr uint32_t LV_KNOWN = SDSP_LEVELS_PEAK | SDSP_LEVELS_RMS | SDSP_LEVELS_LOUDNESS | SDSP_LEVELS_SILENCE_MAP;

// normalize()'s constants for the fixed {-14 LUFS, 1 dB} configuration and a sample rate
// (loudness_params fills them)
struct LvParams {
    float target_peak;  // 10^((0 - headroom) / 20)
    float target_rms;   // 10^((target_lufs + 3 - headroom) / 20)
    float target_lufs;  // -14
    float gate;         // 10^((-70 + 0.691) / 10)
    int64_t block;      // 400-ms block, samples (0: "Sample rate too low for LUFS calculation")
    float b0, b1, b2, a1, a2;
};

// ---- fold steps ----
// KWeightingFilter::process (Direct Form II transposed, normalization.rs:161-167)
struct LvBiquad {
    float b0, b1, b2, a1, a2;
    float x1, x2;
};
SD_HD float lv_biquad(LvBiquad& s, float v) {
    const float o = s.b0 * v + s.x1;
    s.x1 = s.b1 * v + s.x2 - s.a1 * o;
    s.x2 = s.b2 * v - s.a2 * o;
    return o;
}
// one term of sum((x * g)^2): the sample as the reference stores it after its gain, squared
SD_HD void lv_square(float& sum, float v, float g) {
    const float y = v * g;
    sum += y * y;
}
// a 400-ms block's end: its mean square joins the gated sum when above the gate (:213-239)
struct LvGated {
    float bsum, gsum;
    int32_t gn;
};
SD_HD void lv_close_block(LvGated& s, int64_t len, float gate) {
    const float ms = s.bsum / (float)len;
    if (ms > gate) {
        s.gsum += ms;
        s.gn++;
    }
    s.bsum = 0.0f;
}

// ---- the folds of one track, as k_levels writes them ----
struct LvFolds {
    float peak;     // max |x|
    float ss_raw;   // sum x^2
    float gsum;     // sum of the gated blocks' mean squares of the K-weighted signal
    int32_t gn;     // gated blocks
    float ss_peak;  // sum (x * g_peak)^2
    float ss_lufs;  // sum (x * g_lufs)^2
};

SD_HD float lv_db(float v) { return 20.0f * sd_log10f(v); }
SD_HD float lv_rms_db(float ss, uint64_t n) {  // :303-308
    const float rms = __builtin_sqrtf(ss / (float)n);
    return rms > LV_EPS ? lv_db(rms) : -SD_INF_F;
}
SD_HD sdsp_loudness lv_quiet() {  // :277-282, :342-347
    sdsp_loudness m{};
    m.status = SDSP_OK;
    m.measured = 1;
    m.measured_lufs = -SD_INF_F;  // None
    m.peak_db = -SD_INF_F;
    m.rms_db = -SD_INF_F;
    m.gain_db = 0.0f;
    m.gain = 1.0f;
    return m;
}

// the gain normalize_peak multiplies by (1.0f where it applies none)
SD_HD float lv_peak_gain(float peak, float target_peak) {
    return peak > LV_EPS ? sd_minf(target_peak / peak, 1.0f / peak) : 1.0f;
}
// normalize_peak :262-322
SD_HD sdsp_loudness lv_finish_peak(const LvFolds& f, uint64_t n, const LvParams& P) {
    sdsp_loudness m = lv_quiet();
    if (f.peak <= LV_EPS) return m;
    m.peak_db = lv_db(f.peak);
    m.gain_db = lv_db(P.target_peak / f.peak);  // of target / peak, not of the applied minimum
    m.gain = lv_peak_gain(f.peak, P.target_peak);
    m.rms_db = lv_rms_db(f.ss_peak, n);  // of the normalised samples
    return m;
}
// normalize_rms :325-398 (target_rms_db = target_lufs + 3)
SD_HD sdsp_loudness lv_finish_rms(const LvFolds& f, uint64_t n, const LvParams& P) {
    sdsp_loudness m = lv_quiet();
    const float rms = __builtin_sqrtf(f.ss_raw / (float)n);
    if (rms <= LV_EPS) return m;
    m.rms_db = lv_db(rms);  // of the raw samples
    m.peak_db = lv_db(f.peak);
    const float g = P.target_rms / rms;
    if (f.peak * g > 1.0f) {
        m.gain = 1.0f / f.peak;
        m.gain_db = lv_db(m.gain);
    } else {
        m.gain = g;
        m.gain_db = lv_db(g);
    }
    return m;
}
// calculate_lufs' tail (:241-258): 0 = every block under the gate (-inf), 1 = *lufs, -1 = the
// NumericalError branch (unreachable: a gated mean exceeds the gate, about 1.17e-7 > 1e-10)
SD_HD int lv_lufs(const LvFolds& f, float* lufs) {
    if (f.gn == 0) return 0;
    const float mean = f.gsum / (float)f.gn;
    if (mean <= LV_EPS) return -1;
    *lufs = -0.691f + 10.0f * sd_log10f(mean);
    return 1;
}
// the gain normalize_lufs multiplies by (the Peak gain when every block is gated); *st as lv_lufs
SD_HD float lv_lufs_gain(const LvFolds& f, const LvParams& P, int* st) {
    float lufs = 0.0f;
    *st = lv_lufs(f, &lufs);
    if (*st == 0) return lv_peak_gain(f.peak, P.target_peak);
    if (*st < 0) return 1.0f;
    const float g = sd_powf(10.0f, (P.target_lufs - lufs) / 20.0f);
    return f.peak * g > P.target_peak ? P.target_peak / f.peak : g;
}
// normalize_lufs :401-484; f.ss_lufs is the fold under lv_lufs_gain's gain
SD_HD sdsp_loudness lv_finish_loudness(const LvFolds& f, uint64_t n, const LvParams& P) {
    sdsp_loudness m = lv_quiet();
    if (P.block == 0) {
        m.status = SDSP_ERR_INVALID_INPUT;  // "Sample rate too low for LUFS calculation"
        return m;
    }
    float lufs = 0.0f;
    const int st = lv_lufs(f, &lufs);
    if (st == 0) return lv_finish_peak(f, n, P);  // measured_lufs None
    if (st < 0) {
        m.status = SDSP_ERR_NUMERICAL;
        return m;
    }
    m.has_lufs = 1;
    m.measured_lufs = lufs;
    m.gain_db = P.target_lufs - lufs;
    const float g = sd_powf(10.0f, m.gain_db / 20.0f);
    m.peak_db = lv_db(f.peak);
    if (f.peak * g > P.target_peak) {
        m.gain = P.target_peak / f.peak;
        m.gain_db = lv_db(m.gain);
    } else {
        m.gain = g;
    }
    m.rms_db = lv_rms_db(f.ss_lufs, n);  // of the normalised samples
    return m;
}

// ---- silence map (silence.rs:183-231) ----
// A run of silent frames [start_f, end_f), ended by a non-silent frame or by the last frame
// (end_f = num_frames): kept from min_frames on, or when it starts the track.  (The in-loop test
// `silence_end_frame == num_frames` is never true: a run found inside the loop ends at a frame.)
SD_HD bool lv_keep_run(uint64_t start_f, uint64_t end_f, uint64_t min_frames) {
    return end_f - start_f >= min_frames || start_f == 0;
}
// detect_and_trim's frame count for n > 0 samples and its minimum run
SD_HD uint64_t lv_frames(uint64_t n, uint64_t fs) { return n >= fs ? (n - fs) / (fs / 2) + 1 : 1; }
SD_HD uint64_t lv_min_frames(uint32_t sr, uint64_t fs) {
    const uint64_t min_samples = sd_f2u64((float)500u / 1000.0f * (float)sr);
    return (min_samples + (fs / 2) - 1) / (fs / 2);
}
// regions a track of F frames can keep: the leading and the trailing run, and interior runs of at
// least min_frames silent frames followed by a non-silent one
SD_HD uint64_t lv_map_capacity(uint64_t F, uint64_t min_frames) {
    return F / ((min_frames > 1 ? min_frames : 1) + 1) + 2;
}
// The map of one track from its frame RMS (frame f at rms[f * stride]), sequentially as the
// reference walks it; out: (start, end) sample pairs, at most lv_map_capacity of them.  Returns
// the count.  The kernel (k_silence_map) finds the same runs in parallel and applies lv_keep_run.
SD_HD uint64_t lv_silence_map(const float* rms, uint64_t F, uint64_t stride, float thr, uint64_t min_frames,
                              uint64_t hop, uint64_t n, uint64_t* out) {
    uint64_t k = 0, start = 0;
    bool in = false;
    for (uint64_t f = 0; f < F; f++) {
        const bool silent = rms[f * stride] <= thr;
        if (silent && !in) {
            in = true;
            start = f;
        } else if (!silent && in) {
            in = false;
            if (lv_keep_run(start, f, min_frames)) out[2 * k] = start * hop, out[2 * k + 1] = f * hop, k++;
        }
    }
    if (in && lv_keep_run(start, F, min_frames)) out[2 * k] = start * hop, out[2 * k + 1] = n, k++;
    return k;
}

// ---- request checks (before any device is touched) ----
inline const char* levels_request_error(uint32_t what) {
    if (what == 0) return "Invalid input: levels request with what == 0";
    if (what & ~LV_KNOWN) return "Invalid input: levels request with unknown bits";
    return nullptr;
}
// The caller's sdsp_request_set as this library's: fields past the caller's struct_size read as NULL.
// Returns the refusal, or nullptr with *out filled (set == NULL: no request).
inline const char* request_set_read(const sdsp_request_set* set, sdsp_request_set* out) {
    *out = sdsp_request_set{};
    out->struct_size = (uint32_t)sizeof(sdsp_request_set);
    if (!set) return nullptr;
    if (set->struct_size < offsetof(sdsp_request_set, overviews) + sizeof(void*))
        return "Invalid input: sdsp_request_set.struct_size smaller than the first request pair";
    const size_t have = set->struct_size < sizeof(sdsp_request_set) ? set->struct_size : sizeof(sdsp_request_set);
    auto has = [&](size_t off) { return off + sizeof(void*) <= have; };
    if (has(offsetof(sdsp_request_set, ov_req))) out->ov_req = set->ov_req;
    if (has(offsetof(sdsp_request_set, overviews))) out->overviews = set->overviews;
    if (has(offsetof(sdsp_request_set, kt_req))) out->kt_req = set->kt_req;
    if (has(offsetof(sdsp_request_set, timelines))) out->timelines = set->timelines;
    if (has(offsetof(sdsp_request_set, lv_req))) out->lv_req = set->lv_req;
    if (has(offsetof(sdsp_request_set, levels))) out->levels = set->levels;
    if (has(offsetof(sdsp_request_set, tm_req))) out->tm_req = set->tm_req;
    if (has(offsetof(sdsp_request_set, tempo_maps))) out->tempo_maps = set->tempo_maps;
    return nullptr;
}

}  // namespace sdsp
