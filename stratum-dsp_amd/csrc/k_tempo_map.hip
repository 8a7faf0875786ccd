// k_tempo_map.hip — the tempo map request (include/stratum_hip.h, sdsp_tempo_map), one wavefront
// per track, queued behind k_beat: what generate_beat_grid computes and drops (reference
// src/features/beat_tracking/mod.rs:140-219):
//
//   the whole-track HMM beats      hmm.rs:121-441 (beat_device.hpp's hmm_track, re-run: k_beat keeps
//                                  them in LDS or scratch only while it runs)
//   the tempo segments             tempo_variation.rs:95-227
//   the tracker chain              bayesian.rs:104-178, with the confidence k_beat never needed
//   the time signature's scores    time_signature.rs:90-199, over the published beats
//
// Work mapping.  The windows of detect_tempo_variations are independent once their starts are
// known: lane l of a round evaluates window 64 r + l, its start reached by l sequential additions
// of the step from the round's base (the reference's `cur += seg_dur - overlap`, bit for bit), with
// its own binary searches and its own in-order folds over the HMM beats in LDS
// (tempo_map_core.hpp's tm_window).  The emitting lanes compact their segments in window order by
// ballot.  The tracker chain is sequential across the variable segments (its tempo carries), so
// the wave walks a round's variable segments in lane order, all lanes on one segment: candidates on
// lanes as in k_beat, then the re-track's beat count with frames on lanes.  The three signature
// scores sit on three lanes.  Every sum is the reference's sequential f32 fold.
//
// LDS: 24 KB (the onsets, then the published beats in their place; the HMM beats), inside k_beat's
// 32 KB so the kernel fits beside the key stream's STFT.  Lists that outgrow it live in k_beat's
// scratch, which is free once k_beat has run.
#include "beat_device.hpp"
#include "tempo_map_core.hpp"

namespace sdsp {

// hmm_track (hmm.rs:121-441) without the list: the number of beats, or -1 (Err)
__device__ int hmm_count(float bpm, const float* on, int n) {
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
        if (t < nf) {
            const float ft = start + ((float)t * interval);
            const float md = nearest_dist(on, n, ft);
            const float dsq = md * md;
            const float em = sd_expf(-dsq / (2.0f * sigma_sq));
            keep = em > 0.1f;
        }
        nb += __popcll(__ballot(keep));
    }
    return nb;
}

// bayes_update (beat_device.hpp) that also hands out the winning likelihood, the reference's
// best_likelihood: 0 when no candidate had a positive one (bayesian.rs:121-136)
__device__ bool bayes_update_lik(float* cur_bpm, const float* on, int n, float* out_bpm, float* out_lik) {
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
    const float m = wave_max(lik);
    float best_bpm = *cur_bpm;
    if (m > 0.0f) {
        const unsigned long long bal = __ballot(lik == m);
        const int w = __ffsll((long long)bal) - 1;
        best_bpm = __shfl(cb, w, 64);
    }
    *cur_bpm = best_bpm;
    *out_bpm = best_bpm;
    *out_lik = m > 0.0f ? m : 0.0f;
    return true;
}

__global__ __launch_bounds__(64) void k_tempo_map(int n_tracks, const uint32_t* __restrict__ onsets,
                                                  const uint64_t* __restrict__ on_off, const int* __restrict__ on_n,
                                                  uint32_t sr, const float* __restrict__ bpm_in,
                                                  float* __restrict__ scratch, const uint64_t* __restrict__ beat_off,
                                                  const int* __restrict__ beat_cap, const float* __restrict__ beats,
                                                  const BeatOut* __restrict__ bout, const uint64_t* __restrict__ seg_off,
                                                  TmSeg* __restrict__ segs, TmOut* __restrict__ out) {
    SDSP_LATENCY_CRITICAL();
    __shared__ float s_on[BEAT_LDS_ON];
    __shared__ float s_hb[BEAT_LDS_B];
    const int trk = blockIdx.x;
    const int lane = threadIdx.x;
    if (trk >= n_tracks) return;
    TmOut r{};
    auto finish = [&]() {
        if (lane == 0) out[trk] = r;
    };
    const BeatOut bo = bout[trk];
    if (bo.ok <= 0) {  // no grid (or a list outgrew k_beat's capacity: the track fails)
        finish();
        return;
    }
    const float bpm = bpm_in[trk];
    const int n = on_n[trk];
    const int cap = beat_cap[trk];
    // k_beat's scratch layout per track: [onsets_s | hmm | refined | tmp], each `cap` floats (cap >= n)
    float* ons = scratch + beat_off[trk] * 4;
    float* hb = ons + cap;
    const uint32_t* os = onsets + on_off[trk];
    float* onp = n <= BEAT_LDS_ON ? s_on : ons;
    for (int k = lane; k < n; k += 64) onp[k] = (float)os[k] / (float)sr;
    __syncthreads();
    {
        const float interval = 60.0f / bpm;
        const uint64_t nfr = sd_f2u64(__builtin_ceilf((onp[n - 1] - onp[0]) / interval)) + 1;
        if (bpm > EPS && nfr <= (uint64_t)BEAT_LDS_B) hb = s_hb;
    }
    int overflow = 0;
    const int nh = hmm_track(bpm, onp, n, hb, cap, &overflow);
    __syncthreads();
    SegGen g;
    if (nh <= 0 || overflow || !seg_init(g, hb, nh, bpm)) {  // (k_beat stopped here too: not reached with ok = 1)
        finish();
        return;
    }
    const int seg_cap = (int)(seg_off[trk + 1] - seg_off[trk]);
    TmSeg* so = segs + seg_off[trk];
    int nseg = 0, beats_const = 0, beats_var = 0;
    bool has_var = false;
    if (!g.single) {
        float cur_bpm = bpm;  // the tracker's tempo, carried across the variable segments
        float base = g.cur;
        int started = 0;
        bool more = true;
        while (more) {
            float cur = base;
            for (int k = 0; k < lane; k++) cur += g.step;
            const bool valid = cur < g.last;
            base = __shfl(cur, 63, 64) + g.step;
            more = __shfl((int)valid, 63, 64) != 0;
            started += __popcll(__ballot(valid));
            if (started > seg_cap) {  // more windows than tm_segment_capacity proves possible
                r.ok = -1;
                finish();
                return;
            }
            TmSeg sg{};
            bool emit = false;
            if (valid) {
                const float se = sd_minf(cur + g.seg_dur, g.last);
                const int i0 = lower_bound_f(hb, nh, cur);
                const int i1 = upper_bound_f(hb, nh, se);
                bool var = false;
                emit = tm_window(hb, i0, i1, bpm, &sg.bpm, &sg.conf, &var);
                if (emit) {
                    sg.start = cur;
                    sg.end = se;
                    sg.variable = var;
                    sg.n_beats = var ? 0u : (uint32_t)(i1 - i0);  // a constant segment passes these HMM beats on
                }
            }
            const unsigned long long bal = __ballot(emit);
            const int pos = nseg + __popcll(bal & ((1ull << lane) - 1ull));
            const int cnt = __popcll(bal);  // <= the windows started, so nseg + cnt <= seg_cap
            unsigned long long vb = __ballot(emit && sg.variable != 0);
            has_var = has_var || vb != 0;
            while (vb) {  // mod.rs:167-199, the round's variable segments in order
                const int w = __ffsll((long long)vb) - 1;
                vb &= vb - 1;
                const float s0 = __shfl(sg.start, w, 64), s1 = __shfl(sg.end, w, 64);
                const int i0 = lower_bound_f(onp, n, s0);
                const int i1 = upper_bound_f(onp, n, s1);
                if (i1 > i0) {
                    const float old = cur_bpm;
                    float ub, lik;
                    if (!bayes_update_lik(&cur_bpm, onp + i0, i1 - i0, &ub, &lik)) {  // Err -> no grid (k_beat: ok = 0)
                        r = TmOut{};
                        finish();
                        return;
                    }
                    const int got = hmm_count(ub, onp + i0, i1 - i0);
                    if (lane == w) {
                        sg.updated = 1;
                        sg.n_onsets = (uint32_t)(i1 - i0);
                        sg.ubpm = ub;
                        sg.uconf = tm_updated_confidence(lik, old, ub);
                        sg.n_beats = got > 0 ? (uint32_t)got : 0u;
                    }
                }
            }
            if (emit) {
                so[pos] = sg;
                if (sg.variable)
                    beats_var += (int)sg.n_beats;
                else
                    beats_const += (int)sg.n_beats;
            }
            nseg += cnt;
        }
    }
    if (nseg == 0) {  // the single-segment fallbacks (tempo_variation.rs:108-125, 214-222)
        if (seg_cap < 1) {
            r.ok = -1;
            finish();
            return;
        }
        if (lane == 0) {
            TmSeg sg{};
            sg.start = hb[0];
            sg.end = hb[nh - 1];
            sg.bpm = bpm;
            sg.conf = nh < 4 ? 0.5f : 0.8f;
            so[0] = sg;
        }
        nseg = 1;
    }
    beats_const = wave_sum_i(beats_const);
    beats_var = wave_sum_i(beats_var);
    if (!has_var) {  // n_beats counts what went into the refined list: nothing without variation
        __threadfence();
        __syncthreads();
        for (int k = lane; k < nseg; k += 64) so[k].n_beats = 0;
    }
    __syncthreads();  // the onsets are not read below: the published beats take their place
    // time signature (time_signature.rs:90-149) over the published beats: lanes 0/1/2 score 4/4, 3/4, 6/8
    const int nfin = bo.n_beats;
    const float* fin = beats + beat_off[trk];
    if (nfin <= BEAT_LDS_ON) {
        for (int k = lane; k < nfin; k += 64) s_on[k] = fin[k];
        __syncthreads();
        fin = s_on;
    }
    r.bpb = (int32_t)TM_TS_FALLBACK_BPB;
    r.ts_conf = TM_TS_FALLBACK_CONF;
    if (nfin >= 8) {
        float sum = 0.0f;
        int niv = 0;
        for (int k = 1; k < nfin; k++) {
            const float d = fin[k] - fin[k - 1];
            if (d > 0.0f) {
                sum += d;
                niv++;
            }
        }
        if (niv > 0) {
            const float mean = sum / (float)niv;
            float sc = 0.0f;
            if (lane < 3) sc = score_ts(fin, nfin, lane == 0 ? 4 : lane == 1 ? 3 : 6, mean, niv);
            const float s3[3] = {__shfl(sc, 0, 64), __shfl(sc, 1, 64), __shfl(sc, 2, 64)};
            uint32_t bpb;
            tm_pick_signature(s3, &bpb, &r.ts_conf);
            r.bpb = (int32_t)bpb;
            r.ts_scored = 1;
            for (int k = 0; k < 3; k++) r.score[k] = s3[k];
        }
    }
    r.ok = 1;
    r.has_var = has_var ? 1 : 0;
    r.refined = has_var && beats_const + beats_var > 0 ? 1 : 0;
    r.hmm_beats = nh;
    r.n_seg = nseg;
    finish();
}

void launch_tempo_map(int n_tracks, const uint32_t* onsets, const uint64_t* on_off, const int* on_n, uint32_t sr,
                      const float* bpm, float* scratch, const uint64_t* beat_off, const int* beat_cap,
                      const float* beats, const BeatOut* bout, const uint64_t* seg_off, TmSeg* segs, TmOut* out,
                      hipStream_t st) {
    if (n_tracks == 0) return;
    hipLaunchKernelGGL(k_tempo_map, dim3(n_tracks), dim3(64), 0, st, n_tracks, onsets, on_off, on_n, sr, bpm, scratch,
                       beat_off, beat_cap, beats, bout, seg_off, segs, out);
}

// The tracks' consensus onsets gathered into one dense array for the download (the lists sit
// `lists x frames` apart on the device).
__global__ __launch_bounds__(64) void k_onset_gather(int n_tracks, const uint32_t* __restrict__ onsets,
                                                     const uint64_t* __restrict__ on_off, const int* __restrict__ on_n,
                                                     const uint64_t* __restrict__ pfx, uint32_t* __restrict__ dense) {
    const int t = blockIdx.x;
    if (t >= n_tracks) return;
    const uint64_t cnt = pfx[t + 1] - pfx[t];  // the host's copy of on_n[t]: the bound of this track's slot
    const uint32_t* src = onsets + on_off[t];
    uint32_t* dst = dense + pfx[t];
    for (uint64_t k = threadIdx.x; k < cnt; k += 64) dst[k] = src[k];
}

void launch_onset_gather(int n_tracks, const uint32_t* onsets, const uint64_t* on_off, const int* on_n,
                         const uint64_t* pfx, uint32_t* dense, hipStream_t st) {
    if (n_tracks == 0) return;
    hipLaunchKernelGGL(k_onset_gather, dim3(n_tracks), dim3(64), 0, st, n_tracks, onsets, on_off, on_n, pfx, dense);
}

}  // namespace sdsp
