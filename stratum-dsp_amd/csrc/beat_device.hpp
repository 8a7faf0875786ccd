// beat_device.hpp — the wave-level device functions of the beat stage, shared by k_beat.hip (the
// beat grid) and k_tempo_map.hip (the tempo map request).  Each is the reference restated for one
// wavefront per track (src/features/beat_tracking/):
//
//   HmmBeatTracker::track_beats   hmm.rs:121-441            hmm_track
//   detect_tempo_variations       tempo_variation.rs:95-227 SegGen / seg_init / seg_next
//   BayesianBeatTracker           bayesian.rs:104-272       bayes_update
//   detect_time_signature         time_signature.rs:161-199 score_ts
//
// Device code only (included after kernels.hpp).  k_beat.hip's header comment says how the lanes
// split the work and why every list the kernels walk sits in LDS.
#pragma once
#include "kernels.hpp"

namespace sdsp {

// first index with a[i] >= x (a ascending)
__device__ inline int lower_bound_f(const float* a, int n, float x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
// first index with a[i] > x
__device__ inline int upper_bound_f(const float* a, int n, float x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (!(x < a[mid]))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__device__ inline float nearest_dist(const float* on, int n, float t) {
    const int i = lower_bound_f(on, n, t);
    float md = SD_INF_F;
    if (i < n) md = sd_minf(md, sd_absf(on[i] - t));
    if (i > 0) md = sd_minf(md, sd_absf(on[i - 1] - t));
    return md;
}

// hmm.rs:121-441, all lanes of the wave (uniform arguments); returns the number of beats or
// -1 (Err).  *overflow is set when more than `cap` beats would be emitted.
__device__ int hmm_track(float bpm, const float* on, int n, float* out, int cap, int* overflow) {
    if (bpm <= EPS || bpm > 300.0f) return -1;
    if (n <= 0) return -1;
    const int lane = threadIdx.x & 63;
    const float start = on[0], end = on[n - 1];
    const float interval = 60.0f / bpm;
    const uint64_t nf = sd_f2u64(__builtin_ceilf((end - start) / interval)) + 1;
    const float sigma = 0.05f / 2.0f;
    const float sigma_sq = sigma * sigma;
    int nb = 0;
    for (uint64_t t0 = 0; t0 < nf; t0 += 64) {
        const uint64_t t = t0 + (uint64_t)lane;
        bool keep = false;
        float ft = 0.0f;
        if (t < nf) {
            ft = start + ((float)t * interval);
            const float md = nearest_dist(on, n, ft);
            const float dsq = md * md;
            const float em = sd_expf(-dsq / (2.0f * sigma_sq));
            keep = em > 0.1f;
        }
        const unsigned long long bal = __ballot(keep);
        const int pos = nb + __popcll(bal & ((1ull << lane) - 1ull));
        const int cnt = __popcll(bal);
        if (keep && pos < cap) out[pos] = ft;
        if (nb + cnt > cap) {
            *overflow = 1;
            return cap;
        }
        nb += cnt;
    }
    return nb;
}

struct SegGen {
    const float* b;
    int n;
    float seg_dur, step, cur, last;
    float nominal;
    bool single;  // the single-segment fallback cases
    int phase;    // 0 = running, 1 = emitted single, 2 = done
};

struct Seg {
    float start, end, bpm;
    bool variable;
};

// Replays detect_tempo_variations (tempo_variation.rs:95-227) one segment at a time.
// Returns false when exhausted.  *err set when the reference returns Err.
__device__ bool seg_next(SegGen& g, Seg* s, bool* any_emitted) {
    const float* b = g.b;
    const int n = g.n;
    if (g.phase == 2) return false;
    if (g.single) {
        if (g.phase == 1) {
            g.phase = 2;
            return false;
        }
        g.phase = 1;
        s->start = n == 0 ? 0.0f : b[0];
        s->end = n == 0 ? 0.0f : b[n - 1];
        s->bpm = g.nominal;
        s->variable = false;
        *any_emitted = true;
        return true;
    }
    while (g.cur < g.last) {
        const float cur = g.cur;
        const float se = sd_minf(cur + g.seg_dur, g.last);
        g.cur += g.step;
        const int i0 = lower_bound_f(b, n, cur);
        const int i1 = upper_bound_f(b, n, se);
        if (i1 - i0 < 3) continue;
        float sum = 0.0f;
        int cnt = 0;
        for (int k = i0 + 1; k < i1; k++) {
            const float d = b[k] - b[k - 1];
            if (d > 0.0f) {
                sum += d;
                cnt++;
            }
        }
        if (cnt == 0) continue;
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
        const float cv = mean > EPS ? sd / mean : 0.0f;
        s->start = cur;
        s->end = se;
        s->bpm = mean > EPS ? 60.0f / mean : g.nominal;
        s->variable = cv > 0.15f;
        *any_emitted = true;
        return true;
    }
    // exhausted; if nothing was emitted the reference returns one nominal segment
    if (!*any_emitted) {
        g.single = true;
        g.phase = 1;
        s->start = b[0];
        s->end = b[n - 1];
        s->bpm = g.nominal;
        s->variable = false;
        *any_emitted = true;
        return true;
    }
    g.phase = 2;
    return false;
}

__device__ bool seg_init(SegGen& g, const float* b, int n, float nominal) {
    g.b = b;
    g.n = n;
    g.nominal = nominal;
    g.phase = 0;
    g.single = false;
    if (n < 4) {
        g.single = true;
        return true;
    }
    if (nominal <= EPS) return false;  // Err
    const float total = b[n - 1] - b[0];
    if (total < 2.0f) {
        g.single = true;
        return true;
    }
    g.seg_dur = sd_clampf(total / 4.0f, 4.0f, 8.0f);
    const float overlap = g.seg_dur * 0.5f;
    g.step = g.seg_dur - overlap;
    g.cur = b[0];
    g.last = b[n - 1];
    return true;
}

// bayesian.rs:104-178, all lanes (uniform arguments); returns false on Err.  Lane c
// evaluates the c-th candidate tempo (cb advanced by c sequential +0.5 steps, exactly the
// reference's loop variable) with the likelihood folded over the onsets in order; the winner
// is the first candidate reaching the maximum (the reference's strict `lik > best`).
__device__ bool bayes_update(float* cur_bpm, const float* on, int n, float* out_bpm) {
    if (n <= 0) return false;
    if (*cur_bpm <= EPS || *cur_bpm > 300.0f) return false;
    const int lane = threadIdx.x & 63;
    const float lo = sd_maxf(*cur_bpm - 5.0f, 60.0f), hi = sd_minf(*cur_bpm + 5.0f, 180.0f);
    const float sig_sq = 0.05f * 0.05f;
    float cb = lo;
    for (int k = 0; k < lane; k++) cb += 0.5f;
    float lik = -1.0f;  // lanes past `hi` take no part
    if (cb <= hi) {
        const float bi = 60.0f / cb;
        const float st0 = on[0];
        float ll = 0.0f;
        int32_t valid = 0;
        for (int k = 0; k < n; k++) {
            const float o = on[k];
            const int32_t idx = sd_f2i32(sd_roundf((o - st0) / bi));
            const float et = st0 + ((float)idx * bi);
            const float d = sd_absf(o - et);
            ll += -(d * d) / (2.0f * sig_sq);
            valid++;
        }
        lik = valid == 0 ? 0.0f : sd_expf(ll / (float)valid);
    }
    // (lo >= 60 so the reference's `cb <= EPS -> Err` never fires; with 64 lanes and at most
    // 21 candidates every candidate is covered)
    const float m = wave_max(lik);
    float best_bpm = *cur_bpm;
    if (m > 0.0f) {
        const unsigned long long bal = __ballot(lik == m);
        const int w = __ffsll((long long)bal) - 1;
        best_bpm = __shfl(cb, w, 64);
    }
    *cur_bpm = best_bpm;
    *out_bpm = best_bpm;
    return true;
}

__device__ float score_ts(const float* b, int nb, int bpb, float mean, int n_iv) {
    if (n_iv < bpb) return 0.0f;
    // intervals with d > 0, visited in order; autocorrelation at lag bpb over that list
    // (materialised implicitly: iv(k) = k-th positive difference)
    float acc = 0.0f;
    int32_t cnt = 0;
    // walk two cursors over positive differences
    int ka = 1, kb = 1, seen_b = 0;
    // advance kb to the bpb-th positive interval
    while (seen_b < bpb && kb < nb) {
        if (b[kb] - b[kb - 1] > 0.0f) seen_b++;
        kb++;
    }
    // now kb is one past the (bpb)-th positive interval; iv index of kb's next positive = bpb
    for (int i = 0; i + bpb < n_iv; i++) {
        while (!(b[ka] - b[ka - 1] > 0.0f)) ka++;
        while (!(b[kb] - b[kb - 1] > 0.0f)) kb++;
        const float d = sd_absf((b[ka] - b[ka - 1]) - (b[kb] - b[kb - 1]));
        acc += 1.0f / (1.0f + d / mean);
        cnt++;
        ka++;
        kb++;
    }
    if (cnt == 0) return 0.0f;
    const float ac = acc / (float)cnt;
    float vs = 0.0f;
    for (int k = 1; k < nb; k++) {
        const float d = b[k] - b[k - 1];
        if (d > 0.0f) {
            const float dd = d - mean;
            vs += dd * dd;
        }
    }
    const float var = vs / (float)n_iv;
    const float cv = mean > EPS ? __builtin_sqrtf(var) / mean : 1.0f;
    const float cons = 1.0f / (1.0f + cv);
    return sd_minf(ac * 0.7f + cons * 0.3f, 1.0f);
}

// LDS: 32 KB per one-wave workgroup, so k_beat fits on a CU beside the key stream's STFT.  Every
// list the kernel walks sequentially lives in LDS when it fits (a dependent global load costs
// microseconds on a chip whose HBM the key stream saturates; an LDS load ~100 cycles):
constexpr int BEAT_LDS_ON = 4096;    // onsets (then, after the segment loop, the sort keys)
constexpr int BEAT_LDS_B = 2048;     // HMM beats, when the HMM grid has at most this many frames
constexpr int BEAT_SORT_MAX = 2048;  // LDS bitonic sort capacity (larger: serial merge sort); the
                                     // sorted refined beats stay in LDS
static_assert(BEAT_SORT_MAX * 8 <= BEAT_LDS_ON * 4, "sort keys alias the onset buffer");

}  // namespace sdsp
