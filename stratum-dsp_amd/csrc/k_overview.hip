// k_overview.hip — the per-track overview envelope (include/stratum_hip.h, sdsp_overview): per
// column the minimum and maximum of the normalised, trimmed signal and the maximum magnitude of
// the base tempo pass's spectrogram in three bands.  No reference counterpart: a library scanner's
// summary, computed from buffers an analysis call already holds.
//
//   k_ov_segments   min / max of raw * gain per hop segment       the sample stream, read once
//   k_ov_columns    band maxima and segment min / max per column   the spectrogram rows, read once
//   k_ov_fold       the pieces of a column longer than OV_PIECE frames
//
// A column's samples are whole hop segments: segment t of a track is [t hop, (t + 1) hop), and the
// last one, t = F - 1, runs to the track's end (overview_plan.hpp, ov_sample_range).  So the
// sample envelope is taken per segment, one value pair per spectrogram row, and k_ov_columns
// folds segments and rows over a column's frames alike; the column form does not touch the
// 31.75 MB stream.
//
// Only min, max and their cross-lane folds are taken, so no order is observable.  The sample
// extrema are folded on order-preserving integer keys of the f32 bits, a total order with
// -0 < +0: the result does not depend on which zero a hardware min would return.  Magnitudes are
// never negative; their maxima are taken as floats and folded across pieces on their bits.
#include "block_utils.hpp"
#include "kernels.hpp"
#include "overview_plan.hpp"

namespace sdsp {

namespace {
typedef float f4 __attribute__((ext_vector_type(4)));

// f32 bits -> u32 key, ascending in the float's value (-0 below +0), and back
__device__ __forceinline__ uint32_t ov_key(float v) {
    const uint32_t u = sd_bits_f(v);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float ov_unkey(uint32_t k) {
    return sd_from_bits_f((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max_nn(float v) {  // no NaN among the operands
    for (int o = 32; o > 0; o >>= 1) v = max_bnn(v, __shfl_xor(v, o, 64));
    return v;
}
}  // namespace

// ---- sample envelope per hop segment ----
// One wave per segment, OV_SEGS consecutive segments (rows of the frame prefix) per wave: the
// 16-B aligned body of the segment as float4 loads, 64 lanes side by side (whole cache lines),
// two loads per lane in flight; the < 4 unaligned samples at either end as scalars (k_peak_abs's
// split).  A segment is hop samples (2 KiB at hop 512); the last of a track up to
// frame_size + hop - 1.
constexpr int OV_SEGS = 8;
__global__ __launch_bounds__(256) void k_ov_segments(const float* __restrict__ x, const uint64_t* __restrict__ src_off,
                                                     const float* __restrict__ gain,
                                                     const uint64_t* __restrict__ n_len,
                                                     const uint64_t* __restrict__ frame_pfx, int T, uint64_t total,
                                                     int hop, uint32_t* __restrict__ seg_lo,
                                                     uint32_t* __restrict__ seg_hi) {
    const int l = threadIdx.x & 63;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t g = ((uint64_t)blockIdx.x * 4 + wv) * OV_SEGS;
    if (g >= total) return;
    const uint64_t gend = g + OV_SEGS < total ? g + OV_SEGS : total;
    int trk = find_track(frame_pfx, T, g);
    for (; g < gend; g++) {
        while (g >= frame_pfx[trk + 1]) trk++;  // g < total = frame_pfx[T]: stops at trk <= T - 1
        const uint64_t t = g - frame_pfx[trk], F = frame_pfx[trk + 1] - frame_pfx[trk];
        const uint64_t n = n_len[trk];
        const uint64_t s0 = t * (uint64_t)hop;
        const uint64_t s1 = t + 1 < F ? s0 + (uint64_t)hop : n;  // s0 < s1 <= n (frame t lies inside the track)
        const int64_t len = (int64_t)(s1 - s0);
        const float* p = x + src_off[trk] + s0;
        const float gn = gain[trk];
        const int lead = (int)(((16u - ((uintptr_t)p & 15u)) & 15u) / 4u);  // samples before 16-B alignment
        const int64_t h = lead < len ? lead : len;
        const int64_t nb = (len - h) / 4;  // aligned float4s
        const f4* q = reinterpret_cast<const f4*>(p + h);
        uint32_t lo = 0xFFFFFFFFu, hi = 0u;
        auto take = [&](float v) {
            const uint32_t k = ov_key(v * gn);
            lo = min(lo, k);
            hi = max(hi, k);
        };
        for (int64_t k = l; k < nb; k += 128) {
            // the second load clamped onto the first where it would pass the body: the same
            // samples folded twice change neither extremum
            const f4 a = q[k], b = q[k + 64 < nb ? k + 64 : k];
            take(a.x), take(a.y), take(a.z), take(a.w);
            take(b.x), take(b.y), take(b.z), take(b.w);
        }
        if (l < h) take(p[l]);
        const int64_t tl = h + 4 * nb;
        if (l < len - tl) take(p[tl + l]);
        lo = wave_min_u32(lo);
        hi = wave_max_u32(hi);
        if (l == 0) {
            seg_lo[g] = lo;
            seg_hi[g] = hi;
        }
    }
}

// ---- columns: band maxima over the rows, sample extrema over the segments ----
// One wave per unit.  A track's columns are cut into P = ceil(longest column / OV_PIECE) pieces of
// at most OV_PIECE frames each (P = 1 unless the request asks for few, long columns), unit
// r = c P + p of the track being piece p of column c, so that no wave streams more than OV_PIECE
// rows whatever the column count.  A lane owns the same 4 bins (one float4 of the row) in every
// frame of the piece: its running maxima stay in registers across the frames, their bands are
// looked at once per piece, and the cross-lane fold is paid once per unit.  With one frame per
// column that is once per frame.  Rows are 64 lanes x 16 B side by side, 256 bins a pass.
// Lanes past the row's last float4 are clamped onto it (a maximum taken twice).  P = 1 units
// write the column's five values; others write their partial keys for k_ov_fold.
__global__ __launch_bounds__(256) void k_ov_columns(const float* __restrict__ mags,
                                                    const uint64_t* __restrict__ frame_pfx,
                                                    const uint64_t* __restrict__ col_pfx,
                                                    const uint64_t* __restrict__ unit_pfx, int T, uint64_t n_units,
                                                    const uint32_t* __restrict__ seg_lo,
                                                    const uint32_t* __restrict__ seg_hi, OvParams P,
                                                    float* __restrict__ out,
                                                    uint32_t* __restrict__ part) {
    const int l = threadIdx.x & 63;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t u = (uint64_t)blockIdx.x * 4 + wv;
    if (u >= n_units) return;
    const int trk = find_track(unit_pfx, T, u);
    const uint64_t F = frame_pfx[trk + 1] - frame_pfx[trk], C = col_pfx[trk + 1] - col_pfx[trk];
    const uint64_t np = ov_pieces(F, C, P.columns, P.frames_per_column, OV_PIECE);
    const uint64_t r = u - unit_pfx[trk], c = r / np, pc = r % np;
    const uint64_t c0 = ov_f0(c, F, C, P.columns, P.frames_per_column);
    const uint64_t c1 = ov_f0(c + 1, F, C, P.columns, P.frames_per_column);
    uint64_t fa = c0 + pc * OV_PIECE, fb = fa + OV_PIECE;
    fa = fa < c1 ? fa : c1;  // (an empty piece of a shorter column: the neutral values)
    fb = fb < c1 ? fb : c1;
    const int nfr = (int)(fb - fa);
    const uint64_t row0 = frame_pfx[trk] + fa;

    float lo = 0.0f, mi = 0.0f, hi = 0.0f;
    const int nf4 = (P.B + 3) / 4, s4 = P.stride / 4;
    const f4* rows = reinterpret_cast<const f4*>(mags) + row0 * (uint64_t)s4;
    for (int k0 = 0; k0 < nf4 && nfr > 0; k0 += 64) {
        const int k = k0 + l < nf4 ? k0 + l : nf4 - 1;
        const f4* q = rows + k;
        f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
        for (int fr = 0; fr < nfr; fr++) {
            const f4 v = q[(uint64_t)fr * (uint64_t)s4];
            acc.x = max_bnn(acc.x, v.x);
            acc.y = max_bnn(acc.y, v.y);
            acc.z = max_bnn(acc.z, v.z);
            acc.w = max_bnn(acc.w, v.w);
        }
        const float a[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t b = (uint32_t)(4 * k + e);  // the row's padding (b >= B) belongs to no band
            if (b < P.b1)
                lo = max_bnn(lo, a[e]);
            else if (b < P.b2)
                mi = max_bnn(mi, a[e]);
            else if (b < (uint32_t)P.B)
                hi = max_bnn(hi, a[e]);
        }
    }
    uint32_t slo = 0xFFFFFFFFu, shi = 0u;
    if (l < nfr) {  // nfr <= OV_PIECE = 64: one segment per lane
        slo = seg_lo[row0 + (uint64_t)l];
        shi = seg_hi[row0 + (uint64_t)l];
    }
    lo = wave_max_nn(lo);
    mi = wave_max_nn(mi);
    hi = wave_max_nn(hi);
    slo = wave_min_u32(slo);
    shi = wave_max_u32(shi);
    if (l != 0) return;
    if (np == 1) {
        float* o = out + 5 * col_pfx[trk] + c;  // the track's five arrays back to back, C each
        o[0] = ov_unkey(slo);
        o[C] = ov_unkey(shi);
        o[2 * C] = lo;
        o[3 * C] = mi;
        o[4 * C] = hi;
    } else {
        part[u] = slo;
        part[n_units + u] = shi;
        part[2 * n_units + u] = sd_bits_f(lo);  // magnitudes >= +0: the bits order as the values
        part[3 * n_units + u] = sd_bits_f(mi);
        part[4 * n_units + u] = sd_bits_f(hi);
    }
}

// The columns cut into several pieces: one lane per column folds its pieces' partial keys.
__global__ __launch_bounds__(256) void k_ov_fold(const uint64_t* __restrict__ frame_pfx,
                                                 const uint64_t* __restrict__ col_pfx,
                                                 const uint64_t* __restrict__ unit_pfx, int T, uint64_t n_units,
                                                 OvParams P, uint64_t n_cols, const uint32_t* __restrict__ part,
                                                 float* __restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_cols) return;
    const int trk = find_track(col_pfx, T, g);
    const uint64_t F = frame_pfx[trk + 1] - frame_pfx[trk], C = col_pfx[trk + 1] - col_pfx[trk];
    const uint64_t np = ov_pieces(F, C, P.columns, P.frames_per_column, OV_PIECE);
    if (np == 1) return;  // k_ov_columns wrote the column
    const uint64_t u0 = unit_pfx[trk] + (g - col_pfx[trk]) * np;
    uint32_t v[5] = {0xFFFFFFFFu, 0u, 0u, 0u, 0u};
    for (uint64_t p = 0; p < np; p++) {
        v[0] = min(v[0], part[u0 + p]);
#pragma unroll
        for (int k = 1; k < 5; k++) v[k] = max(v[k], part[(uint64_t)k * n_units + u0 + p]);
    }
    float* o = out + 5 * col_pfx[trk] + (g - col_pfx[trk]);
    o[0] = ov_unkey(v[0]);
    o[C] = ov_unkey(v[1]);
#pragma unroll
    for (int k = 2; k < 5; k++) o[(uint64_t)k * C] = sd_from_bits_f(v[k]);
}

void launch_overview_segments(const float* x, const uint64_t* src_off, const float* gain, const uint64_t* n_len,
                              const uint64_t* frame_pfx, int T, uint64_t total, int hop, uint32_t* seg_lo,
                              uint32_t* seg_hi, hipStream_t st) {
    if (total == 0) return;
    const uint64_t per_wg = 4 * (uint64_t)OV_SEGS;
    hipLaunchKernelGGL(k_ov_segments, dim3((unsigned)((total + per_wg - 1) / per_wg)), dim3(256), 0, st, x, src_off,
                       gain, n_len, frame_pfx, T, total, hop, seg_lo, seg_hi);
}

void launch_overview_columns(const float* mags, const uint64_t* frame_pfx, const uint64_t* col_pfx,
                             const uint64_t* unit_pfx, int T, uint64_t n_units, uint64_t n_cols, bool pieces,
                             const uint32_t* seg_lo, const uint32_t* seg_hi, const OvParams& P, float* out,
                             uint32_t* part, hipStream_t st) {
    if (n_units == 0) return;
    hipLaunchKernelGGL(k_ov_columns, dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, st, mags, frame_pfx, col_pfx,
                       unit_pfx, T, n_units, seg_lo, seg_hi, P, out, part);
    if (pieces)
        hipLaunchKernelGGL(k_ov_fold, dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, st, frame_pfx, col_pfx,
                           unit_pfx, T, n_units, P, n_cols, part, out);
}

}  // namespace sdsp
