// r128_core.hpp — the arithmetic of the programme loudness request (include/stratum_hip.h, sdsp_r128),
// shared by the kernels (k_r128.hip), the host pipeline and the stand-alone host harness
// (tests/cpp/r128_core_test.cpp): the coefficients, the filter step, the block folds, the gates, the
// order statistics and the finishing logs, and the request checks.  No HIP runtime call; every log is
// sdsp_libm.h's, every sum the contract's sequential f32 fold.  Build with -ffp-contract=off: the
// filter and the folds must not become FMAs.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sdsp_libm.h"
#include "../../include/stratum_hip.h"

namespace sdsp {

constexpr uint32_t R128_KNOWN = SDSP_R128_LOUDNESS | SDSP_R128_TRUE_PEAK | SDSP_R128_CURVES;
constexpr uint32_t R128_MIN_SR = 8000;
constexpr int R128_TAPS = 12;   // taps per phase of the true-peak interpolator
constexpr int R128_AHEAD = 5;   // x[i + k - R128_AHEAD], k in [0, R128_TAPS)
constexpr int R128_MOM = 4, R128_SHORT = 30;  // steps per momentary / short-term block

// One call's constants: both biquads (b0 b1 b2 a1 a2), the absolute gate, the interpolator.
struct R128Params {
    float shelf[5], hp[5];
    float gate;                 // Ga = 10^((-70 + 0.691) / 10), as LvParams::gate
    uint32_t step;              // sr / 10
    float h[3][R128_TAPS];      // phases 1, 2, 3 of 4
};

// ---- the coefficients (host, in double, rounded to f32) ----
inline void r128_biquad_tail(double K, double Q, double* a0, float* a) {
    *a0 = 1.0 + K / Q + K * K;
    a[0] = (float)(2.0 * (K * K - 1.0) / *a0);
    a[1] = (float)((1.0 - K / Q + K * K) / *a0);
}
inline R128Params r128_params(uint32_t sr) {
    const double pi = 3.14159265358979323846;
    R128Params P{};
    {
        const double K = tan(pi * 1681.974450955533 / (double)sr), Vh = pow(10.0, 3.999843853973347 / 20.0),
                     Vb = pow(Vh, 0.4996667741545416), Q = 0.7071752369554196;
        double a0;
        r128_biquad_tail(K, Q, &a0, P.shelf + 3);
        P.shelf[0] = (float)((Vh + Vb * K / Q + K * K) / a0);
        P.shelf[1] = (float)(2.0 * (K * K - Vh) / a0);
        P.shelf[2] = (float)((Vh - Vb * K / Q + K * K) / a0);
    }
    {
        const double K = tan(pi * 38.13547087602444 / (double)sr), Q = 0.5003270373238773;
        double a0;
        r128_biquad_tail(K, Q, &a0, P.hp + 3);
        P.hp[0] = 1.0f, P.hp[1] = -2.0f, P.hp[2] = 1.0f;
    }
    P.gate = sd_powf(10.0f, (-70.0f + 0.691f) / 10.0f);
    P.step = sr / 10;
    for (int p = 1; p <= 3; p++)
        for (int k = 0; k < R128_TAPS; k++) {
            const double t = (double)(k - R128_AHEAD) - (double)p / 4.0;  // (never 0)
            P.h[p - 1][k] = (float)(sin(pi * t) / (pi * t) * (0.5 + 0.5 * cos(pi * t / 6.0)));
        }
    return P;
}

// ---- the filter step (Direct Form II transposed) ----
struct R128Biquad {
    float x1, x2;
};
SD_HD float r128_biquad(R128Biquad& s, const float* c, float v) {
    const float o = c[0] * v + s.x1;
    s.x1 = (c[1] * v + s.x2) - c[3] * o;
    s.x2 = c[2] * v - c[4] * o;
    return o;
}
// Both stages of one chain: shelf, then high-pass.
struct R128Chain {
    R128Biquad sh, hp;
};
SD_HD float r128_kweight(R128Chain& q, const float* shelf, const float* hp, float v) {
    return r128_biquad(q.hp, hp, r128_biquad(q.sh, shelf, v));
}
// z[j] of a track on the host (the harness and small callers; k_r128_steps runs the same steps).
inline float r128_step_energy(const float* x, uint64_t j, const R128Params& P) {
    R128Chain q{};
    const uint64_t step = P.step, a = (j > 0 ? j - 1 : 0) * step, own = j * step, e = (j + 1) * step;
    float z = 0.0f;
    for (uint64_t i = a; i < e; i++) {
        const float o = r128_kweight(q, P.shelf, P.hp, x[i]);
        if (i >= own) z += o * o;
    }
    return z;
}

// ---- blocks ----
SD_HD uint64_t r128_n_mom(uint64_t J) { return J >= R128_MOM ? J - (R128_MOM - 1) : 0; }
SD_HD uint64_t r128_n_short(uint64_t J) { return J >= R128_SHORT ? J - (R128_SHORT - 1) : 0; }
SD_HD float r128_block(const float* z, uint64_t j, int len, uint32_t step) {
    float s = 0.0f;
    for (int k = 0; k < len; k++) s += z[j + (uint64_t)k];
    return s / (float)((uint32_t)len * step);
}
SD_HD float r128_momentary(const float* z, uint64_t j, uint32_t step) { return r128_block(z, j, R128_MOM, step); }
SD_HD float r128_short_term(const float* z, uint64_t j, uint32_t step) { return r128_block(z, j, R128_SHORT, step); }

// ---- gates and ordered means: one block at a time, in block order ----
struct R128Mean {
    float sum;
    uint64_t n;
};
SD_HD void r128_mean_add(R128Mean& a, float e, bool pass) {
    if (pass) {
        a.sum += e;
        a.n++;
    }
}
SD_HD float r128_mean(const R128Mean& a) { return a.sum / (float)a.n; }
// rank of the low and the high order statistic among M survivors
SD_HD uint64_t r128_rank_low(uint64_t M) { return ((M - 1) * 10 + 50) / 100; }
SD_HD uint64_t r128_rank_high(uint64_t M) { return ((M - 1) * 95 + 50) / 100; }

// ---- what the per-track kernel writes ----
struct R128Folds {
    float gated_sum;          // sum of the m above both gates
    uint64_t n_gated;         // their count
    float low, high;          // e[rank_low], e[rank_high] of the short-term survivors
    uint64_t n_gated_short;   // M
    float max_m, max_s;       // largest m and s (0 without a block)
};

// The folds of one track from its z[0..J) on the host, sequentially; k_r128_track gives the same.
// The order statistics by rank counting over bit patterns (non-negative floats order as their bits):
// the smallest v with #{e <= v} > rank is e[rank].
SD_HD bool r128_short_pass(float s, float ga, float gr) { return s > ga && s > gr; }
inline R128Folds r128_folds(const float* z, uint64_t J, const R128Params& P) {
    R128Folds f{};
    const uint64_t nm = r128_n_mom(J), ns = r128_n_short(J);
    R128Mean a{0.0f, 0};
    for (uint64_t j = 0; j < nm; j++) {
        const float m = r128_momentary(z, j, P.step);
        r128_mean_add(a, m, m > P.gate);
        f.max_m = j == 0 ? m : sd_maxf(f.max_m, m);
    }
    if (a.n) {
        const float gr = r128_mean(a) * 0.1f;
        R128Mean g{0.0f, 0};
        for (uint64_t j = 0; j < nm; j++) {
            const float m = r128_momentary(z, j, P.step);
            r128_mean_add(g, m, m > P.gate && m > gr);
        }
        f.gated_sum = g.sum;
        f.n_gated = g.n;
    }
    R128Mean b{0.0f, 0};
    for (uint64_t j = 0; j < ns; j++) {
        const float s = r128_short_term(z, j, P.step);
        r128_mean_add(b, s, s > P.gate);
        f.max_s = j == 0 ? s : sd_maxf(f.max_s, s);
    }
    if (b.n) {
        const float gr = r128_mean(b) * 0.01f;
        uint64_t M = 0;
        for (uint64_t j = 0; j < ns; j++) M += r128_short_pass(r128_short_term(z, j, P.step), P.gate, gr);
        f.n_gated_short = M;
        if (M) {
            const uint64_t rank[2] = {r128_rank_low(M), r128_rank_high(M)};
            float* out[2] = {&f.low, &f.high};
            for (int w = 0; w < 2; w++) {
                uint32_t lo = 0, hi = 0x7f800000u;  // the answer lies in [lo, hi]
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo) / 2;
                    uint64_t c = 0;
                    for (uint64_t j = 0; j < ns; j++) {
                        const float s = r128_short_term(z, j, P.step);
                        c += r128_short_pass(s, P.gate, gr) && sd_bits_f(s) <= mid;
                    }
                    if (c > rank[w]) hi = mid; else lo = mid + 1;
                }
                *out[w] = sd_from_bits_f(lo);
            }
        }
    }
    return f;
}

// ---- peaks ----
// one interpolated value: phase p (1..3) at sample i, from x[i - 5 .. i + 6] in w[0..12)
SD_HD float r128_interp(const float* h, const float* w) {
    float s = 0.0f;
    for (int k = 0; k < R128_TAPS; k++) s += h[k] * w[k];
    return s;
}
inline void r128_peaks(const float* x, uint64_t n, const R128Params& P, bool tp, float* sample_peak, float* true_peak) {
    float sp = 0.0f, t = 0.0f;
    for (uint64_t i = 0; i < n; i++) sp = sd_maxf(sp, sd_absf(x[i]));
    if (tp) {
        t = sp;
        for (uint64_t i = 0; i < n; i++) {
            float w[R128_TAPS];
            for (int k = 0; k < R128_TAPS; k++) {
                const int64_t at = (int64_t)i + k - R128_AHEAD;
                w[k] = at >= 0 && (uint64_t)at < n ? x[at] : 0.0f;
            }
            for (int p = 0; p < 3; p++) t = sd_maxf(t, sd_absf(r128_interp(P.h[p], w)));
        }
    }
    *sample_peak = sp;
    *true_peak = t;
}

// ---- the finishing logs: folds and peaks -> sdsp_r128 (the curves are the caller's) ----
SD_HD float r128_lufs(float e) { return -0.691f + 10.0f * sd_log10f(e); }
SD_HD float r128_db(float v) { return 20.0f * sd_log10f(v); }
inline void r128_finish(const R128Folds& f, float sample_peak, float true_peak, uint64_t n, uint32_t what,
                        const R128Params& P, sdsp_r128* o) {
    *o = sdsp_r128{};
    o->status = SDSP_OK;
    o->n_samples = n;
    o->step_samples = P.step;
    for (int k = 0; k < 5; k++) o->shelf[k] = P.shelf[k], o->highpass[k] = P.hp[k];
    o->sample_peak = sample_peak;
    o->sample_peak_db = r128_db(sample_peak);
    o->true_peak = (what & SDSP_R128_TRUE_PEAK) ? true_peak : 0.0f;
    o->true_peak_dbtp = r128_db(o->true_peak);
    o->integrated_lufs = o->max_momentary_lufs = o->max_short_term_lufs = -SD_INF_F;
    if (!(what & SDSP_R128_LOUDNESS)) return;
    const uint64_t J = n / P.step;
    o->n_steps = J;
    o->n_momentary = r128_n_mom(J);
    o->n_short_term = r128_n_short(J);
    o->n_gated_momentary = f.n_gated;
    o->n_gated_short_term = f.n_gated_short;
    if (f.n_gated) {
        o->has_integrated = 1;
        o->integrated_lufs = r128_lufs(f.gated_sum / (float)f.n_gated);
    }
    if (f.n_gated_short) {
        o->has_range = 1;
        o->range_low_lufs = r128_lufs(f.low);
        o->range_high_lufs = r128_lufs(f.high);
        o->range_lu = o->range_high_lufs - o->range_low_lufs;
    }
    if (o->n_momentary) o->max_momentary_lufs = r128_lufs(f.max_m);
    if (o->n_short_term) o->max_short_term_lufs = r128_lufs(f.max_s);
}

// ---- request checks (before any device is touched) ----
// The pair of sdsp_request_set_ext2 past its base, when the caller's struct_size covers it (the
// caller's struct begins with `set`); else NULL.
inline void request_set_ext2_read(const sdsp_request_set* set, const sdsp_r128_request** req, sdsp_r128** out) {
    *req = nullptr;
    *out = nullptr;
    if (!set) return;
    const sdsp_request_set_ext2* x = reinterpret_cast<const sdsp_request_set_ext2*>(set);
    const size_t have = set->struct_size;
    if (have >= offsetof(sdsp_request_set_ext2, r128_req) + sizeof(void*)) *req = x->r128_req;
    if (have >= offsetof(sdsp_request_set_ext2, r128) + sizeof(void*)) *out = x->r128;
}
inline const char* r128_request_error(uint32_t what, bool has_out, uint32_t sr) {
    if (what == 0) return "Invalid input: loudness request with what == 0";
    if (what & ~R128_KNOWN) return "Invalid input: loudness request with unknown bits";
    if ((what & SDSP_R128_CURVES) && !(what & SDSP_R128_LOUDNESS))
        return "Invalid input: loudness request with SDSP_R128_CURVES but without SDSP_R128_LOUDNESS";
    if (!has_out) return "Invalid input: loudness request without an r128 array";
    if (sr < R128_MIN_SR) return "Invalid input: loudness request with a sample rate under 8000 Hz";
    return nullptr;
}

}  // namespace sdsp
