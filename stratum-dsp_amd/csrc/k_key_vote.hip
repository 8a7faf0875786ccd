// k_key_vote.hip — the key decision (reference src/lib.rs:961-1559):
//
//   k_key_vote  median smoothing, frame weights, segment voting,         smoothing.rs:37-94, src/lib.rs:1211-1436,
//               detect_key_weighted, key clarity                          key/detector.rs:68-313, key_clarity.rs:51-93
//
// One workgroup per track over the chroma rows and frame energies of k_hpcp / k_hpcp_band
// (k_hpcp.hip), with the near-decision certificate (kc_*) over k_hpcp_band's energy bounds.
#include "block_utils.hpp"
#include "kernels.hpp"

namespace sdsp {

// KeyParams::near_check: whether a weight perturbation of the size the block-folded energies make
// could change one of key_from_raw's discrete decisions on these raw scores: the within-mode
// argmax (a top-two gap of at most KV_NEAR_CONF relative) or the normalisation guard.  The argmax
// is what fixes the winners' normalised scores (exactly 1 each), so ties between the final
// winners are exact and stay exact while these decisions hold.
__device__ bool key_raw_near(const float raw[24]) {
    bool near = false;
    for (int m = 0; m < 2; m++) {
        float t1 = 0.0f, t2 = 0.0f;  // the fold keeps 0 as the floor, as key_from_raw's max does
        for (int k = 0; k < 12; k++) {
            const float v = raw[12 * m + k];
            if (v > t1) {
                t2 = t1;
                t1 = v;
            } else if (v > t2) {
                t2 = v;
            }
        }
        near |= t1 > 0.0f && !(t1 - t2 > KV_NEAR_CONF * t1);
        near |= sd_absf(t1 - 1e-9f) <= KV_NEAR_REL * 1e-9f;
    }
    return near;
}

__device__ void key_from_raw(const float raw[24], float sorted[24], int order[24]) {
    float sc[24];
    for (int k = 0; k < 24; k++) sc[k] = raw[k];
    float mM = 0.0f, mm = 0.0f;
    for (int k = 0; k < 12; k++) mM = sd_maxf(mM, sc[k]);
    for (int k = 0; k < 12; k++) mm = sd_maxf(mm, sc[12 + k]);
    if (mM > 1e-9f && mm > 1e-9f) {
        for (int k = 0; k < 12; k++) sc[k] /= mM;
        for (int k = 0; k < 12; k++) sc[12 + k] /= mm;
    }
    int tM = 0, tm = 0;
    for (int k = 1; k < 12; k++)
        if (!(sc[k] < sc[tM])) tM = k;
    for (int k = 1; k < 12; k++)
        if (!(sc[12 + k] < sc[12 + tm])) tm = k;
    const float tMs = sc[tM], tms = sc[12 + tm];
    const int cof_pos[12] = {0, 7, 2, 9, 4, 11, 6, 1, 8, 3, 10, 5};  // position of tonic on the circle
    float rs[24];
    for (int k = 0; k < 24; k++) {
        rs[k] = sc[k];
        const bool major = k < 12;
        const int ref_t = major ? tM : tm;
        const float ref_s = major ? tMs : tms;
        if (ref_s > 1e-9f) {
            const int tp = cof_pos[k % 12], rp = cof_pos[ref_t];
            const int ad = tp > rp ? tp - rp : rp - tp;
            const int dist = ad < 12 - ad ? ad : 12 - ad;
            if (dist <= 2) rs[k] += ref_s * (0.20f * (1.0f - (float)dist * 0.5f));
        }
    }
    for (int k = 0; k < 24; k++) order[k] = k;
    for (int a = 1; a < 24; a++) {  // stable insertion sort, desc
        const int o = order[a];
        int b = a;
        while (b > 0 && rs[order[b - 1]] < rs[o]) {
            order[b] = order[b - 1];
            b--;
        }
        order[b] = o;
    }
    for (int k = 0; k < 24; k++) sorted[k] = rs[order[k]];
}

__device__ float clarity_of(const float* s) {
    const float best = s[0];
    float sum = 0.0f;
    for (int i = 0; i < 24; i++) sum += s[i];
    const float avg = sum / 24.0f;
    float mn = s[0], mx = s[0];
    for (int i = 1; i < 24; i++) {
        if (s[i] < mn) mn = s[i];
        if (!(s[i] < mx)) mx = s[i];
    }
    const float range = mx - mn;
    return range > 1e-10f ? sd_clampf((best - avg) / range, 0.0f, 1.0f) : 0.0f;
}

// cof_pos above maps a tonic to its circle-of-fifths position: the reference searches
// circle_of_fifths = [0,7,2,9,4,11,6,1,8,3,10,5] for the tonic (detector.rs:214-224); that
// array is its own inverse, so position(t) = circle_of_fifths[t].

// stable sort desc of a 24-entry score table by key index, (best - second) / best
__device__ void from_table(const float* acc, float sorted[24], int order[24], float* conf) {
    for (int k = 0; k < 24; k++) order[k] = k;
    for (int a = 1; a < 24; a++) {
        const int o = order[a];
        int b = a;
        while (b > 0 && acc[order[b - 1]] < acc[o]) {
            order[b] = order[b - 1];
            b--;
        }
        order[b] = o;
    }
    for (int k = 0; k < 24; k++) sorted[k] = acc[order[k]];
    *conf = sorted[0] > 0.0f ? sd_clampf((sorted[0] - sorted[1]) / sorted[0], 0.0f, 1.0f) : 0.0f;
}

// detect_key_weighted_mode_heuristic on a base result (detector.rs:326-506): sorted/order become
// the post-bonus table (stable re-sort of the base order), *chosen the possibly mode-flipped key
// index (mode * 12 + tonic) and *conf its confidence.  avg_in: the raw weighted chroma sums,
// wsum: their weight total.
__device__ void mode_heuristic(float sorted[24], int order[24], const float* avg_in, float wsum, const KeyParams& P,
                               int* chosen, float* conf) {
    *chosen = order[0];
    *conf = sorted[0] > 0.0f ? sd_clampf((sorted[0] - sorted[1]) / sorted[0], 0.0f, 1.0f) : 0.0f;
    const float flip_ratio = sd_clampf(P.mh_flip, 0.0f, 1.0f);
    const bool mode_flip = flip_ratio > 0.0f;
    if (!P.mh_bonus && !mode_flip) return;
    if (wsum <= 1e-9f) return;
    float avg[12];
    float sum = -0.0f;
    for (int i = 0; i < 12; i++) {
        avg[i] = avg_in[i];
        sum += avg[i];
    }
    if (sum > 1e-9f)
        for (int i = 0; i < 12; i++) avg[i] /= sum;
    if (P.mh_bonus) {
        const float bw = sd_maxf(P.mh_bonus_w, 0.0f);
        if (bw > 0.0f)
            for (int i = 0; i < 24; i++)
                if (order[i] >= 12) {
                    const int tonic = order[i] - 12;
                    sorted[i] += wsum * bw * (avg[(tonic + 11) % 12] - avg[(tonic + 10) % 12]);
                }
    }
    for (int a = 1; a < 24; a++) {  // stable insertion sort of the base-ordered table, desc
        const float v = sorted[a];
        const int o = order[a];
        int b = a;
        while (b > 0 && sorted[b - 1] < v) {
            sorted[b] = sorted[b - 1];
            order[b] = order[b - 1];
            b--;
        }
        sorted[b] = v;
        order[b] = o;
    }
    float maj_s[12], min_s[12];
    for (int i = 0; i < 24; i++) {
        if (order[i] < 12)
            maj_s[order[i]] = sorted[i];
        else
            min_s[order[i] - 12] = sorted[i];
    }
    const int best = order[0], tonic = best % 12;
    const bool best_major = best < 12;
    const float p_min3 = avg[(tonic + 3) % 12], p_maj3 = avg[(tonic + 4) % 12];
    const float p_min6 = avg[(tonic + 8) % 12], p_maj6 = avg[(tonic + 9) % 12];
    const float p_min7 = avg[(tonic + 10) % 12], p_maj7 = avg[(tonic + 11) % 12];
    const float margin = sd_maxf(P.mh_margin, 0.0f);
    float minor_score = 0.0f, major_score = 0.0f;
    const float third = sd_absf(p_min3 - p_maj3);
    if (p_min3 > p_maj3 * (1.0f + margin))
        minor_score += third * 2.0f;
    else if (p_maj3 > p_min3 * (1.0f + margin))
        major_score += third * 2.0f;
    const float sixth = sd_absf(p_min6 - p_maj6);
    if (p_min6 > p_maj6 * (1.0f + margin))
        minor_score += sixth * 1.0f;
    else if (p_maj6 > p_min6 * (1.0f + margin))
        major_score += sixth * 1.0f;
    const float seventh = sd_absf(p_min7 - p_maj7);
    if (p_min7 > p_maj7 * (1.0f + margin))
        minor_score += seventh * 1.0f;
    else if (p_maj7 > p_min7 * (1.0f + margin))
        major_score += seventh * 1.0f;
    const float total = minor_score + major_score;
    const bool minor_pref = total > 1e-9f ? minor_score > major_score * (1.0f + margin * 0.5f) : false;
    const bool major_pref = total > 1e-9f ? major_score > minor_score * (1.0f + margin * 0.5f) : false;
    int ch = best;
    if (mode_flip) {
        if (best_major && minor_pref) {
            if (maj_s[tonic] > 0.0f && min_s[tonic] >= maj_s[tonic] * flip_ratio) ch = 12 + tonic;
        } else if (!best_major && major_pref) {
            if (min_s[tonic] > 0.0f && maj_s[tonic] >= min_s[tonic] * flip_ratio) ch = tonic;
        }
    }
    const float cs = ch < 12 ? maj_s[ch] : min_s[ch - 12];
    float other = 0.0f;
    for (int i = 0; i < 24; i++)
        if (order[i] != ch) other = sd_maxf(other, sorted[i]);
    *chosen = ch;
    *conf = cs > 0.0f ? sd_clampf((cs - other) / cs, 0.0f, 1.0f) : 0.0f;
}

constexpr int KV_MAXSCALE = 8;

// ---- the rigorous near-decision certificate (KeyParams::near_check, cert_fixed = 0) ----
// k_hpcp_band bounds each frame's energy by |e_ref - e| <= d_f e (energy_delta).  With p the energy
// power, the reference's frame weight is w'_f = c w_f (1 + eps_f), |eps_f| <= eta_f (kc_eta), c the
// factor (med / med')^p its median carries for every frame alike: every decision below is invariant
// under a common factor of the weights, so only eta_f and the roundings matter.  Every raw score is
// R_x = sequential sum over frames of RN(w_f D_fx) (D_fx the frame's template dot, identical on both
// sides), so |R'_x - c R_x| <= c (V_x (1 + 2u) + N_x) with V_x = sum_f eta_f w_f D_fx and
// N_x = u (2.0001 R_x + (1 + K) SS_x), SS_x the sum of the fold's partial sums (both sides' roundings;
// K bounds the reference's partial sums against c times ours).
constexpr double KC_U = 0x1p-24;
constexpr int KC_CAP = 32;
struct KcCand {
    int64_t st;     // the table's frames [st, st + len) of the slice
    int len, w, k;  // the mode's argmax W and a competitor k (key indices)
    float slack;    // G - N_W - N_k - 1.01 u R_W: what E_Wk must stay below
};
// a non-negative double rounded up to f32
__device__ __forceinline__ float kc_up(double x) {
    float d = (float)x;
    if ((double)d < x) d = __uint_as_float(__float_as_uint(d) + 1u);
    return d;
}
__device__ __forceinline__ double kc_noise(double R, double SS, double K) { return KC_U * (2.0001 * R + (1.0 + K) * SS); }
// eta_f for an energy bound d and energy power p: the weight ratio w'/(c w) lies in [e^-L, e^L] with
// L = p d / (1 - d) (the energy) + 2.0001 u p (the two e / med roundings) + 2.0001 (u + 2^-40) (the
// two powf evaluations: double exp / log, then one rounding) + 2.0001 u (the two tonal products);
// e^L - 1 <= L / (1 - L)
__device__ __forceinline__ double kc_eta(double d, double p) {
    const double L = p * d / (1.0 - d) + 2.0001 * KC_U * p + 2.0001 * (KC_U + 0x1p-40) + 2.0001 * KC_U;
    return L / (1.0 - L);
}
// The within-mode argmaxes (key_from_raw's last maximum W) of the reference equal this table's when,
// for every other key k of the mode, G = R_W - R_k > N_W + N_k + E_Wk + 1.01 u R_W (the margin keeps
// RN(R'_k / R'_W) below 1, so the normalised scores cannot tie), where E_Wk = sum_f eta_f w_f
// |D_fW - D_fk| <= V_W + V_k.  Pairs that fail even with E_Wk = 0 are flagged; pairs that only the
// loose V_W + V_k fails are queued for the pair pass (kc_pair_pass), which computes E_Wk.
__device__ __noinline__ int kc_argmax(const float* raw, const float* SS, const float* V, double sf, double K, int64_t st, int len,
                         KcCand* list, int* nlist) {
    int bits = 0;
    for (int m = 0; m < 2; m++) {
        int W = 0;
        for (int k = 1; k < 12; k++)
            if (!(raw[12 * m + k] < raw[12 * m + W])) W = k;
        const double RW = raw[12 * m + W];
        if (!(RW > 0.0)) continue;  // an all-zero mode: every product is +0 on both sides
        const double NW = kc_noise(RW, SS[12 * m + W] * sf, K), VW = V[12 * m + W] * sf;
        for (int k = 0; k < 12; k++) {
            if (k == W) continue;
            const double Rk = raw[12 * m + k], G = RW - Rk;
            const double need0 = NW + kc_noise(Rk, SS[12 * m + k] * sf, K) + 1.01 * KC_U * RW;
            if (G > need0 + (VW + V[12 * m + k] * sf) * (1.0 + 2.0001 * KC_U)) continue;
            const int q = G > need0 ? atomicAdd(nlist, 1) : KC_CAP;
            if (q < KC_CAP) {
                float sl = (float)(G - need0);
                if ((double)sl > G - need0) sl = __uint_as_float(__float_as_uint(sl) - 1u);  // round down
                list[q] = KcCand{st, len, 12 * m + W, 12 * m + k, sl};
            } else {
                bits |= KV_NEAR_ARGMAX;
            }
        }
    }
    return bits;
}
// The clarity gate of one segment (src/lib.rs:1379-1380, key_clarity.rs:51-93), given that both
// within-mode argmaxes hold (kc_argmax): each mode's top is normalised to exactly 1 and gets the
// same bonus on both sides, so best = RN(1 + 0.2f) exactly, and every other post-bonus score rs_x
// moves by at most beta_x = B_x + 2.0001 u (sc_x + rs_x), B_x = (A_x + sc_x A_W) / (R_W - A_W)
// bounding |R'_x / R'_W - R_x / R_W| (A_x = V_x (1 + 2u) + N_x).  The sum over the sorted table
// (whose order may differ) moves by sum beta + 2 * 23 u sum rs, the minimum by max beta, and
// clarity = (best - avg) / (best - min) by the returned bound.  beta_x is written per key.
__device__ __noinline__ double kc_clarity(const float* raw, const float* SS, const float* V, double sf, double K, const float* sorted,
                             const int* order, float* beta, int* bits) {
    auto Ax = [&](int x) { return V[x] * sf * (1.0 + 2.0001 * KC_U) + kc_noise(raw[x], SS[x] * sf, K); };
    int Wm[2];
    double AW[2];
    for (int m = 0; m < 2; m++) {
        int W = 0;
        for (int k = 1; k < 12; k++)
            if (!(raw[12 * m + k] < raw[12 * m + W])) W = k;
        Wm[m] = 12 * m + W;
        AW[m] = Ax(Wm[m]);
        // the normalisation guard (max > 1e-9, detector.rs:165) with the common factor's range is
        // checked by the caller; here an unnormalised table is simply not certified
        if (!(raw[Wm[m]] > 1e-9f) || !((double)raw[Wm[m]] - AW[m] > 0.0)) {
            *bits |= KV_NEAR_RANGE;
            return 1.0;
        }
    }
    double sb = 0.0, bmax = 0.0;
    for (int i = 0; i < 24; i++) {
        const int x = order[i];
        const int W = Wm[x / 12];
        double b = 0.0;
        if (x != W) {
            const double M = raw[W], sc = (double)raw[x] / M, aw = AW[x / 12];
            b = (Ax(x) + sc * aw) / (M - aw) + 2.0001 * KC_U * (sc + (double)sorted[i]);
        }
        beta[x] = kc_up(b);
        sb += b;
        bmax = b > bmax ? b : bmax;
    }
    double srs = 0.0, mn = sorted[0];
    for (int i = 0; i < 24; i++) {
        srs += (double)sorted[i];
        mn = (double)sorted[i] < mn ? (double)sorted[i] : mn;
    }
    const double best = sorted[0], range = best - mn, avg = srs / 24.0, num = best - avg;
    const double dsum = sb + 2.0 * 23.0 * KC_U * srs * 1.01;
    const double davg = dsum / 24.0 + 2.0 * KC_U * __builtin_fabs(avg) * 1.01;
    const double dnum = davg + 2.0 * KC_U * __builtin_fabs(num) * 1.01;
    const double drange = bmax + 2.0 * KC_U * range * 1.01;
    if (!(range - drange > 1e-6)) {
        *bits |= KV_NEAR_RANGE;
        return 1.0;
    }
    const double cl0 = __builtin_fabs(num / range);
    return (dnum + cl0 * drange) / (range - drange) + 2.0 * KC_U * cl0 * 1.01 + 1e-15;
}

// threads per track in k_key_vote.  1024 halves the kernel's serial time (its frame loops are
// latency-bound) but triples it in the two-stream pipeline (16.9 vs 5.5 ms per launch): a
// 1024-thread workgroup needs most of a CU's VGPRs at once, and beside the 8192-point STFT's
// 256-VGPR waves such a CU seldom comes free
#ifndef KV_THREADS
#define KV_THREADS 256
#endif
#ifndef KV_SMALL_ITEMS
#define KV_SMALL_ITEMS 96
#endif
#ifdef SDSP_KV_PROF
#define KV_T(i) do { if (threadIdx.x == 0) kv_t[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define KV_T(i) do { } while (0)
#endif
template <int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4))) void k_key_vote(const int* __restrict__ tracks, int n_items,
                                                  const uint64_t* __restrict__ frame_pfx, float* __restrict__ chroma_raw,
                                                  const float* __restrict__ energy, float* __restrict__ chroma_s,
                                                  float* __restrict__ weights, float* __restrict__ seg_scratch,
                                                  const uint64_t* __restrict__ seg_off, const float* __restrict__ tmpl,
                                                  KeyParams P, KeyOut* __restrict__ out, KeyDbg* __restrict__ dbg,
                                                  const float* __restrict__ edel, float* __restrict__ wdel) {
    __shared__ int hist[256];
    __shared__ int misc[4];
    __shared__ int redi[NT / 64];
    __shared__ float acc[48];
    __shared__ int use_w_s, used_s, near_s;
    __shared__ float totw_s;
    __shared__ float tpl[48][12];
    __shared__ int sc_len[KV_MAXSCALE], sc_pfx[KV_MAXSCALE + 1];
    __shared__ float sc_w[KV_MAXSCALE];
    // the certificate (cert): argmax pairs for the pair pass, the slice's largest energy bound and
    // eta, per-key vote bounds, the full slice's partial-sum totals and sensitivities
    __shared__ KcCand kc_list[KC_CAP];
    __shared__ int kc_n;
    __shared__ unsigned int kc_dmax, kc_emax;
    __shared__ float kc_pa[24], kc_ss[24], kc_v[24];
    __shared__ int kc_w;
    __shared__ double kc_red[NT / 64];
    __shared__ float kc_crs;  // the common factor's relative range (the median's), for absolute thresholds
    const bool cert = P.near_check && !P.cert_fixed && edel && wdel;
#ifdef SDSP_KV_PROF
    uint64_t kv_t[12] = {};
#endif
    KV_T(0);
    const int it = blockIdx.x;
    const int trk = tracks[it];
    const int64_t F_all = (int64_t)(frame_pfx[trk + 1] - frame_pfx[trk]);
    const uint64_t g0 = frame_pfx[trk];
    float* cr = chroma_raw + g0 * 12;
    for (int k = threadIdx.x; k < 576; k += blockDim.x) tpl[k / 12][k % 12] = tmpl[k];
    if (threadIdx.x == 0) {  // published by the barriers below before any reader
        near_s = 0;
        kc_n = 0;
        kc_dmax = 0u;
        kc_emax = 0u;
    }
    if (F_all <= 0) {
        if (threadIdx.x == 0) out[trk] = KeyOut{0, 0, 0.0f, 0.0f, 0, 0, 0, 0};
        return;
    }
    // chroma sharpening (src/lib.rs:1200-1208 -> chroma/normalization.rs:41-65), in place
    if (P.sharpen > 1.0f) {
        for (int64_t f = threadIdx.x; f < F_all; f += blockDim.x) {
            float* c = cr + f * 12;
            float sq = 0.0f;
            for (int i = 0; i < 12; i++) {
                c[i] = sd_powf(c[i], P.sharpen);
                sq += c[i] * c[i];
            }
            const float nrm = __builtin_sqrtf(sq);
            if (nrm > 1e-10f) {
                for (int i = 0; i < 12; i++) c[i] /= nrm;
            } else {
                const float u = 1.0f / __builtin_sqrtf(12.0f);
                for (int i = 0; i < 12; i++) c[i] = u;
            }
        }
        __syncthreads();
    }
    // median smoothing, window 5 (src/lib.rs:1211-1213 -> smoothing.rs:37-94)
    float* cs_all = chroma_s + g0 * 12;
    // interior frames: the 5 values sorted by odd-even transposition (adjacent compare-exchanges
    // that swap only when the later value is strictly smaller: a stable sort, so its output equals
    // the insertion sort's element for element), branch-free; the edges keep the insertion sort
    auto cx = [](float& a, float& b) {
        const bool sw = b < a;
        const float lo = sw ? b : a, hi = sw ? a : b;
        a = lo;
        b = hi;
    };
    for (int64_t q = threadIdx.x; q < F_all * 12; q += blockDim.x) {
        const int64_t f = (int64_t)((uint32_t)q / 12u);  // F_all * 12 < 2^32
        const int s = (int)((uint32_t)q - 12u * (uint32_t)f);
        if (F_all > 5 && f >= 2 && f + 2 < F_all) {
            const float* c = cr + (f - 2) * 12 + s;
            float v0 = c[0], v1 = c[12], v2 = c[24], v3 = c[36], v4 = c[48];
#pragma unroll
            for (int r = 0; r < 5; r++) {
                if (r % 2 == 0) {
                    cx(v0, v1);
                    cx(v2, v3);
                } else {
                    cx(v1, v2);
                    cx(v3, v4);
                }
            }
            cs_all[q] = v2;
        } else if (F_all > 5) {
            float v[5];
            int n = 0;
            for (int o = -2; o <= 2; o++) {
                const int64_t fi = f + o;
                if (fi >= 0 && fi < F_all) v[n++] = cr[fi * 12 + s];
            }
            for (int a = 1; a < n; a++) {
                const float x = v[a];
                int b = a;
                while (b > 0 && x < v[b - 1]) {
                    v[b] = v[b - 1];
                    b--;
                }
                v[b] = x;
            }
            cs_all[q] = v[n / 2];
        } else {
            cs_all[q] = cr[q];
        }
    }
    __syncthreads();
    KV_T(1);
    // optional edge trim (src/lib.rs:1215-1232): keep the middle frames
    int64_t t0 = 0, F = F_all;
    if (P.edge_trim && F_all >= 200) {
        const float frac = sd_clampf(P.edge_frac, 0.0f, 0.49f);
        const int64_t st = (int64_t)sd_roundf((float)F_all * frac);
        const int64_t en_ = (int64_t)sd_roundf((float)F_all * (1.0f - frac));
        if (en_ > st + 50 && en_ <= F_all) {
            t0 = st;
            F = en_ - st;
        }
    }
    const float* cs = cs_all + t0 * 12;
    const float* en = energy + g0 + t0;
    float* w = weights + g0 + t0;
    const float* ed = cert ? edel + g0 + t0 : nullptr;
    float* wd = cert ? wdel + g0 + t0 : nullptr;
    // frame weights over the slice (src/lib.rs:1236-1287)
    if (P.weighting) {
        const float med = sd_maxf(block_select_kth(en, (int)F, (int)(F / 2), hist, misc), 1e-12f);
        const float ln12 = sd_logf(12.0f);
        int used_local = 0, rng_local = 0;
        uint32_t dmax_local = 0u, emax_local = 0u;
        for (int64_t f = threadIdx.x; f < F; f += blockDim.x) {
            const float* ch = cs + f * 12;
            float sum = 0.0f;
            for (int k = 0; k < 12; k++) sum += ch[k];
            float tonal = 0.0f;
            if (!(sum <= 1e-12f)) {
                float ent = 0.0f;
                for (int k = 0; k < 12; k++) {
                    const float p = ch[k] / sum;
                    if (p > 1e-12f) ent -= p * sd_logf(p);
                }
                tonal = sd_clampf(1.0f - (ent / ln12), 0.0f, 1.0f);
            }
            if (tonal < P.min_tonal) tonal = 0.0f;
            const float e_norm = sd_maxf(en[f] / med, 0.0f);
            const float wt = sd_powf(tonal, sd_maxf(P.tonal_pow, 0.0f));
            const float we = sd_powf(e_norm, sd_maxf(P.energy_pow, 0.0f));
            const float ww = sd_maxf(wt * we, 0.0f);
            w[f] = ww;
            used_local += ww > 0.0f;
            if (cert) {  // eta_f w_f, and the range the certificate assumes
                const double d = ed[f];
                const double eta = d < 0.25 ? kc_eta(d, sd_maxf(P.energy_pow, 0.0f)) : 1.0;
                wd[f] = ww > 0.0f ? kc_up(eta * (double)ww) : 0.0f;
                // an energy whose quotient or weight could underflow on one side only, or no bound
                if (!(d < 0.25) || (en[f] > 0.0f && !(e_norm >= 0x1p-100f) && we != 1.0f) ||
                    (ww > 0.0f && !(ww >= 0x1p-100f)) || !(ww < 0x1p100f))
                    rng_local = 1;
                dmax_local = max(dmax_local, __float_as_uint((float)d));
                emax_local = max(emax_local, __float_as_uint(kc_up(eta)));
            }
        }
        if (cert) {  // one LDS atomic per wave (the maxima of non-negative floats as bit patterns)
            const uint32_t dm = wave_max_u32(dmax_local), em = wave_max_u32(emax_local);
            const bool rg = __builtin_amdgcn_ballot_w64(rng_local != 0) != 0;
            if ((threadIdx.x & 63) == 0) {
                if (rg) atomicOr(&near_s, KV_NEAR_RANGE);
                atomicMax(&kc_dmax, dm);
                atomicMax(&kc_emax, em);
            }
        }
        const int used = block_sum_i(used_local, redi);
        __syncthreads();
        __shared__ float sbuf[SEQ_CH];
        const float sw = block_seq_sum(w, F, sbuf);  // weights.iter().sum(), in order
        if (threadIdx.x == 0) {
            use_w_s = !(sw <= 1e-12f || used < 10);
            // the unweighted fallback (src/lib.rs:1278-1285) is decided by a sum of energy-derived weights:
            // sw' = c sw (1 +- eta_max) +- both folds' roundings, c in [(1 + d_max)^-p, (1 - d_max)^-p]
            float mrel = KV_NEAR_REL;
            if (cert) {
                const double dm = __uint_as_float(kc_dmax), em = __uint_as_float(kc_emax);
                const double L = sd_maxf(P.energy_pow, 0.0f) * dm / (1.0 - dm);
                const double cr = (L < 0.5 ? L / (1.0 - L) : 1.0);
                kc_crs = kc_up(cr);
                mrel = sd_maxf(mrel, kc_up(((1.0 + cr) * (1.0 + em) * (1.0 + 3.0 * (double)F * KC_U) - 1.0) * 1.01));
            }
            if (P.near_check && sd_absf(sw - 1e-12f) <= mrel * 1e-12f) atomicOr(&near_s, KV_NEAR_WSUM);
        }
    } else if (threadIdx.x == 0) {
        use_w_s = 0;
    }
    __syncthreads();
    KV_T(2);
    const bool use_w = use_w_s;
    const int toff = P.tset == 1 ? 24 : 0;  // template rows of the selected set
    if (dbg) {  // debug_track_id: weighted pitch-class sums over the slice, in frame order (src/lib.rs:1473-1491)
        if (threadIdx.x < 12) {
            float a = 0.0f;
            for (int64_t f = 0; f < F; f++) {
                const float wt = use_w ? w[f] : 1.0f;
                if (wt <= 0.0f) continue;
                a += wt * cs[f * 12 + threadIdx.x];
            }
            acc[threadIdx.x] = a;
        }
        if (threadIdx.x == 32) {
            int u = 0;
            for (int64_t f = 0; f < F; f++) u += (use_w ? w[f] : 1.0f) > 0.0f;
            dbg[it].frames = (int)F;
            dbg[it].used = u;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float sa = 0.0f;
            for (int k = 0; k < 12; k++) sa += acc[k];
            for (int k = 0; k < 12; k++) dbg[it].agg[k] = sa > 1e-12f ? acc[k] / sa : acc[k];
        }
        __syncthreads();
    }
    // the final score table for the debug dump (KeyDetectionResult::top_keys)
    auto put_dbg = [&](const float* sorted, const int* order, int key) {
        if (!dbg) return;
        for (int k = 0; k < 24; k++) {
            dbg[it].tab[k] = sorted[k];
            dbg[it].order[k] = order[k];
        }
        dbg[it].key = key;
    };
    // Both folds below skip frames of weight <= 0 (detector.rs:992, 351).  Every term is >= +0
    // (chroma, templates and weights are non-negative), so a skipped frame is folded as +0, which
    // leaves the sum bit-identical; the loops then carry no branch and their loads pipeline
    // across frames.
    auto wsd = [&](int64_t f0, int64_t n, int row) {  // weighted_sum_dot, detector.rs:984-1001
        float a = 0.0f;
        const float* t = tpl[row];
        float tr[12];
#pragma unroll
        for (int k = 0; k < 12; k++) tr[k] = t[k];
#pragma unroll 4
        for (int64_t f = f0; f < f0 + n; f++) {
            const float* c = cs + f * 12;
            float d = 0.0f;
#pragma unroll
            for (int k = 0; k < 12; k++) d += c[k] * tr[k];
            if (use_w) {
                const float wt = w[f];
                a += wt > 0.0f ? wt * d : 0.0f;
            } else {
                a += d;
            }
        }
        return a;
    };
    // weighted_sum_dot with the certificate's companions: *ss = the sum of the fold's partial sums,
    // *vv = sum_f eta_f w_f D_f (f32 sums of non-negative terms; the readers inflate them by (n + 1) u)
    auto wsd3 = [&](int64_t f0, int64_t n, int row, float* ss, float* vv) {
        float a = 0.0f, sa = 0.0f, v = 0.0f;
        const float* t = tpl[row];
        float tr[12];
#pragma unroll
        for (int k = 0; k < 12; k++) tr[k] = t[k];
#pragma unroll 4
        for (int64_t f = f0; f < f0 + n; f++) {
            const float* c = cs + f * 12;
            float d = 0.0f;
#pragma unroll
            for (int k = 0; k < 12; k++) d += c[k] * tr[k];
            const float wt = w[f];
            a += wt > 0.0f ? wt * d : 0.0f;
            sa += a;
            v = __builtin_fmaf(wd[f], d, v);
        }
        *ss = sa;
        *vv = v;
        return a;
    };
    // the certificate's inflation of those f32 sums, and K (kc_noise) for a table of n frames
    auto kc_sf = [](int64_t n) { return 1.0 + 1.0001 * (double)(n + 1) * KC_U; };
    auto kc_K = [&](int64_t n) { return (1.0 + (double)__uint_as_float(kc_emax)) * (1.0 + 3.0 * (double)n * KC_U); };
    // the pair pass (kc_argmax's queue): E_Wk = sum_f eta_f w_f |D_fW - D_fk| over the pair's frames
    // by the whole workgroup, in double; a pair is certified when E_Wk (1 + 1e-6) < its slack
    auto kc_pair_pass = [&]() {
        __syncthreads();
        const int nc = kc_n < KC_CAP ? kc_n : KC_CAP;
        for (int q = 0; q < nc; q++) {
            const KcCand cd = kc_list[q];
            const float* tW = tpl[toff + cd.w];
            const float* tK = tpl[toff + cd.k];
            double e = 0.0;
            for (int64_t f = cd.st + threadIdx.x; f < cd.st + cd.len; f += blockDim.x) {
                const float wf = wd[f];
                if (!(wf > 0.0f)) continue;
                const float* c = cs + f * 12;
                float dW = 0.0f, dK = 0.0f;
#pragma unroll
                for (int k = 0; k < 12; k++) dW += c[k] * tW[k];
#pragma unroll
                for (int k = 0; k < 12; k++) dK += c[k] * tK[k];
                e += (double)wf * __builtin_fabs((double)dW - (double)dK);
            }
            for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
            if ((threadIdx.x & 63) == 0) kc_red[threadIdx.x >> 6] = e;
            __syncthreads();
            if (threadIdx.x == 0) {
                double tot = 0.0;
                for (int r = 0; r < (int)(blockDim.x >> 6); r++) tot += kc_red[r];
                if (!(tot * (1.0 + 1e-6) < (double)cd.slack)) atomicOr(&near_s, KV_NEAR_ARGMAX);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) kc_n = 0;
        __syncthreads();
    };
    // the normalisation guard (max > 1e-9, detector.rs:165) under the common factor: the reference's
    // mode top lies in [(R_W - A_W) / (1 + cr), (R_W + A_W)(1 + cr)]
    auto kc_guard = [&](const float* raw, const float* SS, const float* V, double sf, double K) {
        int bits = 0;
        for (int m = 0; m < 2; m++) {
            int W = 0;
            for (int k = 1; k < 12; k++)
                if (!(raw[12 * m + k] < raw[12 * m + W])) W = k;
            const double R = raw[12 * m + W];
            const double A = V[12 * m + W] * sf * (1.0 + 2.0001 * KC_U) + kc_noise(R, SS[12 * m + W] * sf, K);
            const double cr = kc_crs, t = (double)1e-9f, lo = (R - A) / (1.0 + cr), hi = (R + A) * (1.0 + cr);
            if (!(lo > t) && !(hi <= t)) bits |= KV_NEAR_RANGE;
        }
        return bits;
    };
    // the heuristic's weighted chroma sums (detector.rs:344-368): i < 12 -> avg[i], 12 -> wsum
    auto avg_sum = [&](int64_t f0, int64_t n, int i) {
        if (!use_w && i == 12) return (float)n;
        float a = 0.0f;
#pragma unroll 4
        for (int64_t f = f0; f < f0 + n; f++) {
            const float wt = use_w ? w[f] : 1.0f;
            const float term = i == 12 ? wt : (use_w ? wt * cs[f * 12 + i] : cs[f * 12 + i]);
            a += (use_w && wt <= 0.0f) ? 0.0f : term;
        }
        return a;
    };
    auto write_out = [&](int key, float conf, float clarity, int used) {
        KeyOut r{};
        r.mode = key < 12 ? 0 : 1;
        r.tonic = key % 12;
        r.conf = conf;
        r.clarity = clarity;
        r.ok = 1;
        r.used_segments = used;
        r.weights_used = use_w;
        // the key is the argmax of the accumulated scores: a relative gap in (0, margin] could flip
        // it (an exact tie of winners is structural and stays exact, key_raw_near)
        r.near = P.near_check ? (near_s | ((conf > 0.0f && !(conf > KV_NEAR_CONF)) ? KV_NEAR_FINAL : 0)) : 0;
        out[trk] = r;
    };
    // full-slice detection: detect_key_weighted (+ the mode heuristic)
    auto detect_full = [&](int used_segments) {
        __syncthreads();
        const bool kc = cert && use_w;  // without weights nothing depends on the energies
        if (threadIdx.x < 24)
            acc[threadIdx.x] = kc ? wsd3(0, F, toff + threadIdx.x, &kc_ss[threadIdx.x], &kc_v[threadIdx.x])
                                  : wsd(0, F, toff + threadIdx.x);
        if (P.mh_on && threadIdx.x >= 24 && threadIdx.x < 37) acc[threadIdx.x] = avg_sum(0, F, threadIdx.x - 24);
        __syncthreads();
        if (kc) {  // the slice's within-mode argmaxes (its final key and confidence are structural)
            if (threadIdx.x == 0) {
                float raw[24];
                for (int k = 0; k < 24; k++) raw[k] = acc[k];
                const int b = kc_argmax(raw, kc_ss, kc_v, kc_sf(F), kc_K(F), 0, (int)F, kc_list, &kc_n) |
                              kc_guard(raw, kc_ss, kc_v, kc_sf(F), kc_K(F));
                if (b) atomicOr(&near_s, b);
            }
            kc_pair_pass();
        }
        if (threadIdx.x == 0) {
            float raw[24], sorted[24];
            int order[24];
            for (int k = 0; k < 24; k++) raw[k] = acc[k];
            if (P.near_check && key_raw_near(raw)) atomicOr(&near_s, KV_NEAR_ARGMAX);
            key_from_raw(raw, sorted, order);
            int key = order[0];
            float conf = sorted[0] > 0.0f ? sd_clampf((sorted[0] - sorted[1]) / sorted[0], 0.0f, 1.0f) : 0.0f;
            if (P.mh_on) mode_heuristic(sorted, order, acc + 24, acc[36], P, &key, &conf);
            write_out(key, conf, clarity_of(sorted), used_segments);
            put_dbg(sorted, order, key);
        }
    };
    if (P.ensemble) {  // detect_key_ensemble (detector.rs:881-978), src/lib.rs:1289-1299
        if (threadIdx.x < 48) acc[threadIdx.x] = wsd(0, F, threadIdx.x);
        __syncthreads();
        if (threadIdx.x == 0) {
            const float tot = P.kk_w + P.tp_w;
            const float kn = tot > 1e-9f ? P.kk_w / tot : 0.5f;
            const float tn = tot > 1e-9f ? P.tp_w / tot : 0.5f;
            float raw[24], sorted[24], sa[24], sb[24], comb[24];
            int order[24];
            for (int k = 0; k < 24; k++) raw[k] = acc[k];
            key_from_raw(raw, sorted, order);
            for (int i = 0; i < 24; i++) sa[order[i]] = sorted[i];
            for (int k = 0; k < 24; k++) raw[k] = acc[24 + k];
            key_from_raw(raw, sorted, order);
            for (int i = 0; i < 24; i++) sb[order[i]] = sorted[i];
            for (int k = 0; k < 24; k++) comb[k] = kn * sa[k] + tn * sb[k];
            float conf;
            from_table(comb, sorted, order, &conf);
            write_out(order[0], conf, clarity_of(sorted), 0);
            put_dbg(sorted, order, order[0]);
        }
        return;
    }
    // segment lists: multi-scale (detector.rs:546-719) or segment voting (src/lib.rs:1331-1436)
    int mode = 0;  // 0 full, 1 multi-scale, 2 segment voting
    if (P.ms_on && P.ms_n > 0) {
        int mn = P.ms_len[0];
        for (int i = 1; i < P.ms_n; i++) mn = min(mn, P.ms_len[i]);
        if (F >= mn) mode = 1;
    }
    if (mode == 0 && P.seg_voting && F >= P.seg_len) mode = 2;
    if (mode == 0) {
        detect_full(0);
        return;
    }
    if (threadIdx.x == 0) {
        int n = 0;
        for (int si = 0; si < (mode == 1 ? P.ms_n : 1); si++) {
            const int len = mode == 1 ? P.ms_len[si] : P.seg_len;
            const int hop = mode == 1 ? max(P.ms_hop, 1) : P.seg_hop;
            const float sw = mode == 1 ? (si < P.ms_nw ? P.ms_w[si] : 1.0f) : 1.0f;
            sc_len[si] = len;
            sc_w[si] = sw;
            sc_pfx[si] = n;
            if (!(len == 0 || len > F || sw <= 0.0f)) n += (int)((F - len) / hop) + 1;
        }
        sc_pfx[mode == 1 ? P.ms_n : 1] = n;
    }
    __syncthreads();
    const int nsc = mode == 1 ? P.ms_n : 1;
    const int nseg = sc_pfx[nsc];
    auto seg_of = [&](int sg, int64_t* start, int* len, float* sw) {
        int si = 0;
        while (si + 1 < nsc && sc_pfx[si + 1] <= sg) si++;
        const int hop = mode == 1 ? max(P.ms_hop, 1) : P.seg_hop;
        *start = (int64_t)(sg - sc_pfx[si]) * hop;
        *len = sc_len[si];
        *sw = sc_w[si];
    };
    float* S = seg_scratch + seg_off[it];
    const bool kc2 = cert && use_w && mode == 2;  // segment voting under the certificate
    for (int q = threadIdx.x; q < nseg * 24; q += blockDim.x) {
        int64_t st;
        int len;
        float sw;
        seg_of(q / 24, &st, &len, &sw);
        float* row = S + (size_t)(q / 24) * KV_ROW;
        if (kc2)
            row[q % 24] = wsd3(st, len, toff + q % 24, &row[64 + q % 24], &row[88 + q % 24]);
        else
            row[q % 24] = wsd(st, len, toff + q % 24);  // raw score
    }
    if (P.mh_on)
        for (int q = threadIdx.x; q < nseg * 13; q += blockDim.x) {
            int64_t st;
            int len;
            float sw;
            seg_of(q / 13, &st, &len, &sw);
            const int i = q % 13;
            S[(size_t)(q / 13) * KV_ROW + (i == 12 ? 51 : 52 + i)] = avg_sum(st, len, i);
        }
    __syncthreads();
    KV_T(3);
    for (int sg = threadIdx.x; sg < nseg; sg += blockDim.x) {
        float* row = S + (size_t)sg * KV_ROW;
        float raw[24], sorted[24];
        int order[24];
        for (int k = 0; k < 24; k++) raw[k] = row[k];
        if (P.near_check && key_raw_near(raw)) atomicOr(&near_s, KV_NEAR_ARGMAX);
        int64_t st;
        int len;
        float sw;
        seg_of(sg, &st, &len, &sw);
        if (kc2) {
            const int b = kc_argmax(raw, row + 64, row + 88, kc_sf(len), kc_K(len), st, len, kc_list, &kc_n) |
                          kc_guard(raw, row + 64, row + 88, kc_sf(len), kc_K(len));
            if (b) atomicOr(&near_s, b);
        }
        key_from_raw(raw, sorted, order);
        if (P.mh_on) {
            int key;
            float conf;
            mode_heuristic(sorted, order, row + 52, row[51], P, &key, &conf);
        }
        const float cl = clarity_of(sorted);
        float kc_dcl = 0.0f;
        if (kc2) {  // the clarity bound; the per-key score bounds replace the partial-sum totals
            float beta[24];
            int b = 0;
            kc_dcl = kc_up(kc_clarity(raw, row + 64, row + 88, kc_sf(len), kc_K(len), sorted, order, beta, &b));
            if (b) atomicOr(&near_s, b);
            for (int k = 0; k < 24; k++) row[64 + k] = beta[k];
            row[112] = kc_dcl;
        }
        for (int k = 0; k < 24; k++) {
            row[k] = sorted[k];
            row[24 + k] = (float)order[k];
        }
        row[48] = cl;
        const float gate = mode == 1 ? P.ms_min_cl : P.min_clarity;
        row[49] = cl >= gate ? 1.0f : 0.0f;
        if (P.near_check && sd_absf(cl - gate) <= sd_maxf(KV_NEAR_CLARITY, kc_dcl))
            atomicOr(&near_s, KV_NEAR_GATE);  // the segment gate (src/lib.rs:1380)
        row[50] = cl * sw;
    }
    __syncthreads();
    KV_T(4);
    if (kc2) kc_pair_pass();
    KV_T(5);
    if (threadIdx.x < 24) {
        const int key = threadIdx.x;
        float a = 0.0f;
        double pa = 0.0;  // the certificate: the sum of the fold's partial sums
        for (int sg = 0; sg < nseg; sg++) {
            const float* row = S + (size_t)sg * KV_ROW;
            if (row[49] == 0.0f) continue;
            for (int k = 0; k < 24; k++)
                if ((int)row[24 + k] == key) {
                    a += row[k] * row[50];
                    pa += (double)a;
                    break;
                }
        }
        acc[key] = a;
        if (kc2) kc_pa[key] = kc_up(pa);
    }
    if (threadIdx.x == 32) {
        int u = 0;
        float tw = 0.0f;
        for (int sg = 0; sg < nseg; sg++)
            if (S[(size_t)sg * KV_ROW + 49] != 0.0f) {
                u++;
                tw += S[(size_t)sg * KV_ROW + 50];
            }
        used_s = u;
        totw_s = tw;
    }
    __syncthreads();
    KV_T(6);
    const int used = used_s;
    const float totw = totw_s;
    if (used == 0 || (mode == 1 && totw <= 1e-12f)) {
        detect_full(used);
        return;
    }
    // the certificate's final key (src/lib.rs:1412-1424): acc_x = sum over the used segments of
    // RN(rs_x cl), so for the leader W and a competitor k the reference's difference moves by at most
    // sum (|rs_W - rs_k| dcl + (beta_W + beta_k)(cl + dcl))(1 + 4u) + 2.0001 u (rs_W + rs_k) cl (the
    // products) + 2.0001 u 1.01 (its partial sums): the segment clarity's error enters scaled by the
    // pair's score difference, not by the scores
    if (kc2) {
        if (threadIdx.x == 0) {
            float sorted[24], conf;
            int order[24];
            from_table(acc, sorted, order, &conf);
            kc_w = order[0];
        }
        __syncthreads();
        const int W = kc_w, k = threadIdx.x;
        if (k < 24 && k != W) {
            double D = 0.0;
            // a structural tie: in every used segment both keys hold a certified mode top (the same
            // RN(1 + 0.2f), bound 0), so the reference forms the same products for both and ties too
            bool tie = true;
            for (int sg = 0; sg < nseg; sg++) {
                const float* row = S + (size_t)sg * KV_ROW;
                if (row[49] == 0.0f) continue;
                double rW = 0.0, rK = 0.0;
                for (int j = 0; j < 24; j++) {
                    const int o = (int)row[24 + j];
                    rW = o == W ? (double)row[j] : rW;
                    rK = o == k ? (double)row[j] : rK;
                }
                const double cw = row[50], dc = row[112], bw = row[64 + W], bk = row[64 + k];
                tie = tie && rW == rK && bw == 0.0 && bk == 0.0;
                D += (__builtin_fabs(rW - rK) * dc + (bw + bk) * (cw + dc)) * (1.0 + 4.0001 * KC_U) +
                     2.0001 * KC_U * (rW + rK) * cw;
            }
            D += 2.0001 * KC_U * 1.01 * ((double)kc_pa[W] + (double)kc_pa[k]);
            if (!tie && !((double)acc[W] - (double)acc[k] > D + 1.01 * KC_U * (double)acc[W]))
                atomicOr(&near_s, KV_NEAR_FINAL);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float tab[24], sorted[24];
        int order[24];
        for (int k = 0; k < 24; k++) tab[k] = mode == 1 ? acc[k] / totw : acc[k];
        float conf;
        from_table(tab, sorted, order, &conf);
        write_out(order[0], conf, clarity_of(sorted), used);
        put_dbg(sorted, order, order[0]);
    }
    KV_T(7);
#ifdef SDSP_KV_PROF
    if (threadIdx.x == 0 && (blockIdx.x % 64) == 0)
        printf("kvprof blk %d nseg %d smooth %.1f weights %.1f segs %.1f segkey %.1f pair %.1f acc %.1f final %.1f us\n",
               (int)blockIdx.x, nseg, (kv_t[1] - kv_t[0]) * 0.01, (kv_t[2] - kv_t[1]) * 0.01, (kv_t[3] - kv_t[2]) * 0.01,
               (kv_t[4] - kv_t[3]) * 0.01, (kv_t[5] - kv_t[4]) * 0.01, (kv_t[6] - kv_t[5]) * 0.01, (kv_t[7] - kv_t[6]) * 0.01);
#endif
}

// ---- launcher ----
void launch_key_vote(const int* tracks, int n_items, const uint64_t* frame_pfx, float* chroma_raw,
                     const float* energy, float* chroma_s, float* weights, float* seg_scratch, const uint64_t* seg_off,
                     const float* tmpl, const KeyParams& P, KeyOut* out, hipStream_t st, KeyDbg* dbg,
                     const float* edel, float* wdel, bool alone, int force_threads) {
    if (n_items == 0) return;
    // force_threads (the stage probe's, include/stratum_hip_debug.h): that instantiation, whatever
    // the launch; 0 is the selection below
    if (force_threads == 1024 || force_threads == 512 || force_threads == KV_THREADS) {
        auto* k = force_threads == 1024 ? k_key_vote<1024> : force_threads == 512 ? k_key_vote<512> : k_key_vote<KV_THREADS>;
        hipLaunchKernelGGL(k, dim3(n_items), dim3(force_threads), 0, st, tracks, n_items, frame_pfx, chroma_raw, energy,
                           chroma_s, weights, seg_scratch, seg_off, tmpl, P, out, dbg, edel, wdel);
        return;
    }
    // a few tracks (the exact reruns of near-decision tracks, one-track calls) or a launch with
    // nothing beside it (the call's last sub-batch, `alone`): the latency of one track's workgroup
    // is the launch, and 1024 threads cut it (the segment scores in one round instead of three);
    // other sub-batches keep 256 threads, which fit beside the key-stream STFT
    // (a 1,024-thread workgroup fills its CU's 4 waves per SIMD: more tracks than CUs take two
    // rounds, so a lone launch of more tracks than CUs runs 512 threads, two workgroups per CU)
    int cus = 0;
    if (alone && n_items > KV_SMALL_ITEMS) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            cus = 0;
    }
    if (n_items <= KV_SMALL_ITEMS || (alone && n_items <= cus))
        hipLaunchKernelGGL(k_key_vote<1024>, dim3(n_items), dim3(1024), 0, st, tracks, n_items, frame_pfx, chroma_raw,
                           energy, chroma_s, weights, seg_scratch, seg_off, tmpl, P, out, dbg, edel, wdel);
    else if (alone)
        hipLaunchKernelGGL(k_key_vote<512>, dim3(n_items), dim3(512), 0, st, tracks, n_items, frame_pfx, chroma_raw,
                           energy, chroma_s, weights, seg_scratch, seg_off, tmpl, P, out, dbg, edel, wdel);
    else
        hipLaunchKernelGGL(k_key_vote<KV_THREADS>, dim3(n_items), dim3(KV_THREADS), 0, st, tracks, n_items, frame_pfx,
                           chroma_raw, energy, chroma_s, weights, seg_scratch, seg_off, tmpl, P, out, dbg, edel, wdel);
}

}  // namespace sdsp
