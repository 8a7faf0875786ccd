// k_beat.hip — beat grid, one wavefront per track (reference src/features/beat_tracking/):
//
//   HmmBeatTracker::track_beats   hmm.rs:121-441
//   detect_tempo_variations       tempo_variation.rs:95-227
//   BayesianBeatTracker           bayesian.rs:104-272
//   detect_time_signature         time_signature.rs:90-199
//   generate_beat_grid, downbeats, stability   beat_tracking/mod.rs:108-485
//
// The reference's O(frames x onsets) nearest-onset scans become binary searches over the
// sorted onsets (|o - t| is monotone on each side of t in f32, so the nearest neighbour's
// distance is exactly the reference's minimum).  The 64 lanes of the track's wave split the
// independent work: HMM frames (ordered compaction by ballot), Bayesian candidate tempos
// (one lane each, each likelihood folded sequentially as in the reference), the refined-beat
// sort (bitonic with index tie-break == the reference's stable sort) and the three
// time-signature scores.  Sequential folds (interval means, variances, autocorrelation) stay
// on one lane in the reference's order.  The onsets are staged in LDS when they fit.
// The Viterbi pass is not run: the emission is identical for all five states (hmm.rs:264-294),
// so the extracted beats cannot depend on the path and Viterbi cannot fail.
#include "beat_device.hpp"

namespace sdsp {

// Stable ascending sort of a[0..n) into dst[0..n) (the reference's sort_by(partial_cmp) on NaN-free
// data): bitonic over (value, index) keys in LDS, the index breaking ties.  n <= 2*cap_pow2 slots.
__device__ void wave_sort_stable(const float* a, float* dst, int n, float* kv, int* ki, int npow2) {
    const int lane = threadIdx.x & 63;
    for (int i = lane; i < npow2; i += 64) {
        kv[i] = i < n ? a[i] : SD_INF_F;
        ki[i] = i < n ? i : 0x7fffffff;
    }
    __syncthreads();
    for (int k = 2; k <= npow2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < npow2; i += 64) {
                const int l = i ^ j;
                if (l > i) {
                    const bool up = (i & k) == 0;
                    const float vi = kv[i], vl = kv[l];
                    const int ii = ki[i], il = ki[l];
                    const bool gt = (vi > vl) || (vi == vl && ii > il);
                    if (gt == up) {
                        kv[i] = vl;
                        kv[l] = vi;
                        ki[i] = il;
                        ki[l] = ii;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int i = lane; i < n; i += 64) dst[i] = kv[i];
    __syncthreads();
}

// stable bottom-up merge sort (partial_cmp semantics on NaN-free data)
__device__ void merge_sort_f(float* a, float* tmp, int n) {
    for (int w = 1; w < n; w <<= 1) {
        for (int lo = 0; lo < n; lo += 2 * w) {
            const int mid = lo + w < n ? lo + w : n;
            const int hi = lo + 2 * w < n ? lo + 2 * w : n;
            int i = lo, j = mid, k = lo;
            while (i < mid && j < hi) tmp[k++] = (a[j] < a[i]) ? a[j++] : a[i++];
            while (i < mid) tmp[k++] = a[i++];
            while (j < hi) tmp[k++] = a[j++];
        }
        for (int k = 0; k < n; k++) a[k] = tmp[k];
    }
}

__global__ __launch_bounds__(64) void k_beat(const int* __restrict__ tracks, int n_items,
                                             const uint32_t* __restrict__ onsets, const uint64_t* __restrict__ on_off,
                                             const int* __restrict__ on_n, uint32_t sr,
                                             const float* __restrict__ bpm_in, const float* __restrict__ conf_in,
                                             float* __restrict__ scratch, const uint64_t* __restrict__ beat_off,
                                             const int* __restrict__ beat_cap, float* __restrict__ beats,
                                             float* __restrict__ downs, BeatOut* __restrict__ out) {
    SDSP_LATENCY_CRITICAL();
    __shared__ float s_on[BEAT_LDS_ON];
    __shared__ float s_hb[BEAT_LDS_B];
    __shared__ float s_rb[BEAT_SORT_MAX];
    float* const s_kv = s_on;  // the onsets are not read after the segment loop
    int* const s_ki = reinterpret_cast<int*>(s_on + BEAT_SORT_MAX);
    const int it = blockIdx.x;
    const int lane = threadIdx.x;
    const int trk = tracks[it];
    BeatOut r{0, 0, 0.0f, 0};
    const float bpm = bpm_in[trk];
    const int n = on_n[trk];
    const int cap = beat_cap[trk];
    // scratch layout per track: [onsets_s | hmm | refined | tmp], each `cap` floats (cap >= n)
    float* ons = scratch + beat_off[trk] * 4;
    float* hb = ons + cap;
    float* rb = hb + cap;
    float* tmp = rb + cap;
    float* ob = beats + beat_off[trk];
    float* od = downs + beat_off[trk];
    auto finish = [&]() {
        if (lane == 0) out[trk] = r;
    };
    int overflow = 0;
    if (!(bpm > 0.0f && n >= 2)) {  // src/lib.rs:913, 944-957
        finish();
        return;
    }
    if (bpm > 300.0f) {  // generate_beat_grid InvalidInput
        finish();
        return;
    }
    const uint32_t* os = onsets + on_off[trk];
    float* onp = n <= BEAT_LDS_ON ? s_on : ons;
    for (int k = lane; k < n; k += 64) onp[k] = (float)os[k] / (float)sr;
    __syncthreads();
    // (already ascending; the reference's sort_by(partial_cmp) is a no-op here)
    {
        // the HMM grid's frame count (hmm_track's nf) bounds its beats: LDS when it fits
        const float interval = 60.0f / bpm;
        const uint64_t nfr = sd_f2u64(__builtin_ceilf((onp[n - 1] - onp[0]) / interval)) + 1;
        if (bpm > EPS && nfr <= (uint64_t)BEAT_LDS_B) hb = s_hb;
    }
    int nh = hmm_track(bpm, onp, n, hb, cap, &overflow);
    __syncthreads();
    if (nh <= 0 || overflow) {
        if (overflow) r.ok = -1;
        finish();
        return;
    }
    const float* fin = hb;
    int nfin = nh;
    // tempo variations + Bayesian refinement (mod.rs:140-219); every lane replays the segment
    // generator identically (uniform control flow)
    SegGen g;
    if (!seg_init(g, hb, nh, bpm)) {
        finish();
        return;
    }
    bool any = false, has_var = false;
    Seg s;
    {
        SegGen g2 = g;
        bool any2 = false;
        while (seg_next(g2, &s, &any2)) has_var |= s.variable;
    }
    if (has_var) {
        float cur_bpm = bpm;
        int nr = 0;
        while (seg_next(g, &s, &any)) {
            if (s.variable) {
                const int i0 = lower_bound_f(onp, n, s.start);
                const int i1 = upper_bound_f(onp, n, s.end);
                if (i1 > i0) {
                    float ub;
                    if (!bayes_update(&cur_bpm, onp + i0, i1 - i0, &ub)) {
                        finish();  // Err propagates -> empty grid
                        return;
                    }
                    const int got = hmm_track(ub, onp + i0, i1 - i0, rb + nr, cap - nr, &overflow);
                    __syncthreads();
                    if (overflow) {
                        r.ok = -1;
                        finish();
                        return;
                    }
                    if (got > 0) nr += got;
                }
            } else {
                const int j0 = lower_bound_f(hb, nh, s.start);
                const int j1 = upper_bound_f(hb, nh, s.end);
                if (nr + (j1 - j0) > cap) {
                    r.ok = -1;
                    finish();
                    return;
                }
                for (int k = j0 + lane; k < j1; k += 64) rb[nr + (k - j0)] = hb[k];
                nr += j1 - j0;
                __syncthreads();
            }
        }
        if (nr > 0) {
            int np2 = 1;
            while (np2 < nr) np2 <<= 1;
            if (np2 <= BEAT_SORT_MAX) {
                wave_sort_stable(rb, s_rb, nr, s_kv, s_ki, np2);
                fin = s_rb;
            } else {
                if (lane == 0) merge_sort_f(rb, tmp, nr);
                __syncthreads();
                fin = rb;
            }
            nfin = nr;
        }
    }
    // time signature (time_signature.rs:90-149): lanes 0/1/2 score 4/4, 3/4, 6/8
    int bpb = 4;
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
            const float s44 = __shfl(sc, 0, 64), s34 = __shfl(sc, 1, 64), s68 = __shfl(sc, 2, 64);
            float bs = s44;
            if (!(s34 < bs)) {
                bpb = 3;
                bs = s34;
            }
            if (!(s68 < bs)) {
                bpb = 6;
                bs = s68;
            }
        }
    }
    // beats + downbeats (mod.rs:290-404)
    for (int k = lane; k < nfin; k += 64) ob[k] = fin[k];
    int nd = 0;
    if (lane == 0) {
        const float bi = 60.0f / bpm;
        const float bar = bi * (float)bpb;
        const float tolb = bar * 0.1f;
        float last = fin[0];
        od[nd++] = last;
        for (int k = 1; k < nfin; k++) {
            const float et = last + bar;
            if (sd_absf(fin[k] - et) <= tolb) od[nd++] = last = fin[k];
        }
        // stability (mod.rs:425-485)
        float stab = 0.0f;
        if (nfin >= 2) {
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
                if (mean > 1e-10f) {
                    float vs = 0.0f;
                    for (int k = 1; k < nfin; k++) {
                        const float d = fin[k] - fin[k - 1];
                        if (d > 0.0f) {
                            const float dd = d - mean;
                            vs += dd * dd;
                        }
                    }
                    const float var = vs / (float)niv;
                    const float cv = __builtin_sqrtf(var) / mean;
                    stab = 1.0f / (1.0f + cv);
                }
            }
        }
        r.n_beats = nfin;
        r.n_down = nd;
        r.stability = stab;
        r.ok = 1;
        out[trk] = r;
    }
}

void launch_beat(const int* tracks, int n_items, const uint32_t* onsets, const uint64_t* on_off, const int* on_n,
                 uint32_t sr, const float* bpm, const float* conf, float* scratch, const uint64_t* beat_off,
                 const int* beat_cap, float* beats, float* downs, BeatOut* out, hipStream_t st) {
    if (n_items == 0) return;
    hipLaunchKernelGGL(k_beat, dim3(n_items), dim3(64), 0, st, tracks, n_items, onsets, on_off, on_n, sr,
                       bpm, conf, scratch, beat_off, beat_cap, beats, downs, out);
}

// Gathers the tracks' beat and downbeat lists (capacity-strided in `beats` / `downs`) into
// dense arrays so the host downloads only what was produced: one workgroup; pfx[0..n] and
// pfx[n+1..2n+1] are the exclusive prefixes of the beat and downbeat counts (0 for failed
// tracks).  Integer sums, so the scan order is immaterial.
__global__ __launch_bounds__(1024) void k_beat_compact(int n, const BeatOut* __restrict__ out,
                                                       const uint64_t* __restrict__ beat_off,
                                                       const float* __restrict__ beats, const float* __restrict__ downs,
                                                       uint64_t* __restrict__ pfx, float* __restrict__ cb,
                                                       float* __restrict__ cd) {
    __shared__ uint64_t sb[1024], sd[1024];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int per = (n + nt - 1) / nt, i0 = tid * per, i1 = min(n, i0 + per);
    uint64_t ab = 0, ad = 0;
    for (int i = i0; i < i1; i++) {
        const BeatOut r = out[i];
        ab += r.ok > 0 ? (uint64_t)r.n_beats : 0;
        ad += r.ok > 0 ? (uint64_t)r.n_down : 0;
    }
    sb[tid] = ab;
    sd[tid] = ad;
    __syncthreads();
    for (int o = 1; o < nt; o <<= 1) {  // inclusive Hillis-Steele scan
        const uint64_t vb = tid >= o ? sb[tid - o] : 0, vd = tid >= o ? sd[tid - o] : 0;
        __syncthreads();
        sb[tid] += vb;
        sd[tid] += vd;
        __syncthreads();
    }
    uint64_t pb = sb[tid] - ab, pd = sd[tid] - ad;
    for (int i = i0; i < i1; i++) {
        const BeatOut r = out[i];
        pfx[i] = pb;
        pfx[n + 1 + i] = pd;
        pb += r.ok > 0 ? (uint64_t)r.n_beats : 0;
        pd += r.ok > 0 ? (uint64_t)r.n_down : 0;
    }
    if (tid == nt - 1) {
        pfx[n] = sb[tid];
        pfx[2 * n + 1] = sd[tid];
    }
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6, nw = nt >> 6;
    for (int i = w; i < n; i += nw) {  // one wave per track
        const BeatOut r = out[i];
        if (r.ok <= 0) continue;
        const uint64_t ob = pfx[i], od = pfx[n + 1 + i], src = beat_off[i];
        for (int k = lane; k < r.n_beats; k += 64) cb[ob + k] = beats[src + k];
        for (int k = lane; k < r.n_down; k += 64) cd[od + k] = downs[src + k];
    }
}

// The same gather with one 64-thread workgroup per track: the wave sums the counts of the tracks
// before its own (n/64 loads per lane, L2-resident) and copies its track.  A single-wave
// workgroup dispatches into any free wave slot, where the 1024-thread one above waits for 16 slots
// on one CU; on the shared chip (the key stream's STFT holds most slots) that wait stalled the
// tempo stream behind it.  Used up to COMPACT_W_MAX tracks (the prefix work is quadratic in n).
constexpr int COMPACT_W_MAX = 4096;
__global__ __launch_bounds__(64) void k_beat_compact_w(int n, const BeatOut* __restrict__ out,
                                                       const uint64_t* __restrict__ beat_off,
                                                       const float* __restrict__ beats, const float* __restrict__ downs,
                                                       uint64_t* __restrict__ pfx, float* __restrict__ cb,
                                                       float* __restrict__ cd) {
    const int i = blockIdx.x, lane = threadIdx.x;
    uint64_t ab = 0, ad = 0;
    for (int j = lane; j < i; j += 64) {
        const BeatOut r = out[j];
        ab += r.ok > 0 ? (uint64_t)r.n_beats : 0;
        ad += r.ok > 0 ? (uint64_t)r.n_down : 0;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        ab += __shfl_xor(ab, o, 64);
        ad += __shfl_xor(ad, o, 64);
    }
    const BeatOut r = out[i];
    const uint64_t nb = r.ok > 0 ? (uint64_t)r.n_beats : 0, nd = r.ok > 0 ? (uint64_t)r.n_down : 0;
    if (lane == 0) {
        pfx[i] = ab;
        pfx[n + 1 + i] = ad;
        if (i == n - 1) {
            pfx[n] = ab + nb;
            pfx[2 * n + 1] = ad + nd;
        }
    }
    if (r.ok <= 0) return;
    const uint64_t src = beat_off[i];
    for (int k = lane; k < r.n_beats; k += 64) cb[ab + k] = beats[src + k];
    for (int k = lane; k < r.n_down; k += 64) cd[ad + k] = downs[src + k];
}

void launch_beat_compact(int n, const BeatOut* out, const uint64_t* beat_off, const float* beats, const float* downs,
                         uint64_t* pfx, float* cb, float* cd, hipStream_t st) {
    if (n == 0) return;
    if (n <= COMPACT_W_MAX)
        hipLaunchKernelGGL(k_beat_compact_w, dim3(n), dim3(64), 0, st, n, out, beat_off, beats, downs, pfx, cb, cd);
    else
        hipLaunchKernelGGL(k_beat_compact, dim3(1), dim3(1024), 0, st, n, out, beat_off, beats, downs, pfx, cb, cd);
}

}  // namespace sdsp
