// k_key_timeline.hip — the key timeline's per-segment keys (include/stratum_hip.h,
// sdsp_key_timeline; reference key/key_changes.rs:103-126 -> key/detector.rs:68-313,
// key_clarity.rs:51-93): detect_key with the Krumhansl-Kessler templates over every segment
// [s H, s H + L) of a track's smoothed chroma rows (k_key_vote's chroma_s).
//
//   k_key_timeline   one lane per (segment, key), KT_SEGS segments per block
//
// The grid runs over the call's segments, all tracks' back to back (seg_pfx), so a track's
// segments spread over many blocks.  A lane folds its key's score over the segment's frames as
// k_key_vote's weighted_sum_dot does without weights (f32, the dot from 0 in pitch-class order,
// then the sum from 0 in frame order; multiply and add stay separate), with its template row in
// registers; the 24 lanes of a segment read the same chroma row.  The decision (per-mode
// normalisation, last maximum, circle-of-fifths bonus, stable descending sort, clarity) is
// key_from_raw / clarity_of restated for 24 cooperating lanes over LDS rows: a key's place in the
// stable sort is the count of strictly larger scores plus the equal scores of lower index, so no
// lane holds an indexed array.
#include "block_utils.hpp"
#include "kernels.hpp"
#include "key_timeline_plan.hpp"

namespace sdsp {

namespace {
typedef float kt_f4 __attribute__((ext_vector_type(4)));
constexpr int KT_NT = KT_SEGS * 24;
}  // namespace

__global__ __launch_bounds__(KT_NT) void k_key_timeline(const float* __restrict__ chroma_s,
                                                        const uint64_t* __restrict__ frame_pfx,
                                                        const uint64_t* __restrict__ seg_pfx, int n_tracks,
                                                        uint64_t n_segs, uint32_t L, uint32_t H,
                                                        const float* __restrict__ tmpl, KtSeg* __restrict__ out) {
    __shared__ float va[KT_SEGS][24];  // raw scores, then the bonused scores
    __shared__ float vb[KT_SEGS][24];  // normalised scores, then the sorted table
    __shared__ int vo[KT_SEGS][24];    // the sorted table's keys
    const int sl = (int)threadIdx.x / 24;  // segment slot of the block
    const int k = (int)threadIdx.x - 24 * sl;
    const uint64_t u = (uint64_t)blockIdx.x * KT_SEGS + (uint64_t)sl;
    const bool live = u < n_segs;
    // the track of segment u: the last t with seg_pfx[t] <= u
    int lo = 0, hi = n_tracks;
    while (live && hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_pfx[mid] <= u) lo = mid;
        else hi = mid;
    }
    float a = 0.0f;
    if (live) {
        const uint64_t s = u - seg_pfx[lo];
        const float* c = chroma_s + (frame_pfx[lo] + kt_start(s, H)) * 12;  // L rows, inside the track's F
        float tr[12];
#pragma unroll
        for (int i = 0; i < 12; i++) tr[i] = tmpl[k * 12 + i];
#pragma unroll 4
        for (uint32_t f = 0; f < L; f++) {
            const kt_f4* r = reinterpret_cast<const kt_f4*>(c + (size_t)f * 12);  // rows are 48 B: 16-B aligned
            const kt_f4 r0 = r[0], r1 = r[1], r2 = r[2];
            float d = 0.0f;
            d += r0.x * tr[0];
            d += r0.y * tr[1];
            d += r0.z * tr[2];
            d += r0.w * tr[3];
            d += r1.x * tr[4];
            d += r1.y * tr[5];
            d += r1.z * tr[6];
            d += r1.w * tr[7];
            d += r2.x * tr[8];
            d += r2.y * tr[9];
            d += r2.z * tr[10];
            d += r2.w * tr[11];
            a += d;
        }
    }
    va[sl][k] = a;
    __syncthreads();
    // per-mode maxima from 0 (detector.rs:135-160); every lane of the segment folds both
    float mM = 0.0f, mm = 0.0f;
#pragma unroll
    for (int j = 0; j < 12; j++) mM = sd_maxf(mM, va[sl][j]);
#pragma unroll
    for (int j = 0; j < 12; j++) mm = sd_maxf(mm, va[sl][12 + j]);
    const bool norm = mM > 1e-9f && mm > 1e-9f;
    const float sc = norm ? a / (k < 12 ? mM : mm) : a;
    vb[sl][k] = sc;
    __syncthreads();
    // the last maximum of each mode (detector.rs:162-200)
    int tM = 0, tm = 0;
    float tMs = vb[sl][0], tms = vb[sl][12];
#pragma unroll
    for (int j = 1; j < 12; j++) {
        const float v = vb[sl][j], w = vb[sl][12 + j];
        if (!(v < tMs)) tM = j, tMs = v;
        if (!(w < tms)) tm = j, tms = w;
    }
    // circle-of-fifths bonus (detector.rs:202-260): a tonic's place on the circle is 7 t mod 12
    const int ton = k < 12 ? k : k - 12;
    const int ref_t = k < 12 ? tM : tm;
    const float ref_s = k < 12 ? tMs : tms;
    float rs = sc;
    if (ref_s > 1e-9f) {
        const int tp = (7 * ton) % 12, rp = (7 * ref_t) % 12;
        const int ad = tp > rp ? tp - rp : rp - tp;
        const int dist = ad < 12 - ad ? ad : 12 - ad;
        if (dist <= 2) rs += ref_s * (0.20f * (1.0f - (float)dist * 0.5f));
    }
    __syncthreads();  // (the raw scores have been read)
    va[sl][k] = rs;
    __syncthreads();
    // stable descending sort: this key's place
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 24; j++) {
        const float v = va[sl][j];
        rank += (v > rs || (v == rs && j < k)) ? 1 : 0;
    }
    __syncthreads();  // (the normalised scores have been read)
    vb[sl][rank] = rs;
    vo[sl][rank] = k;
    __syncthreads();
    if (live && k == 0) {
        const float s0 = vb[sl][0], s1 = vb[sl][1];
        KtSeg o;
        o.key = vo[sl][0];
        o.conf = s0 > 0.0f ? sd_clampf((s0 - s1) / s0, 0.0f, 1.0f) : 0.0f;
        // compute_key_clarity over the sorted table (key_clarity.rs:51-93)
        float sum = 0.0f, mn = s0, mx = s0;
#pragma unroll
        for (int j = 0; j < 24; j++) {
            const float v = vb[sl][j];
            sum += v;
            if (j > 0) {
                if (v < mn) mn = v;
                if (!(v < mx)) mx = v;
            }
        }
        const float avg = sum / 24.0f, range = mx - mn;
        o.clarity = range > 1e-10f ? sd_clampf((s0 - avg) / range, 0.0f, 1.0f) : 0.0f;
        o.top_keys[0] = o.key;
        o.top_keys[1] = vo[sl][1];
        o.top_keys[2] = vo[sl][2];
        o.top_scores[0] = s0;
        o.top_scores[1] = s1;
        o.top_scores[2] = vb[sl][2];
        out[u] = o;
    }
}

void launch_key_timeline(const float* chroma_s, const uint64_t* frame_pfx, const uint64_t* seg_pfx, int n_tracks,
                         uint64_t n_segs, uint32_t L, uint32_t H, const float* tmpl, KtSeg* out, hipStream_t st) {
    if (n_tracks <= 0 || n_segs == 0) return;
    const uint64_t blocks = (n_segs + KT_SEGS - 1) / KT_SEGS;
    hipLaunchKernelGGL(k_key_timeline, dim3((unsigned)blocks), dim3(KT_NT), 0, st, chroma_s, frame_pfx, seg_pfx, n_tracks,
                       n_segs, L, H, tmpl, out);
}

}  // namespace sdsp
