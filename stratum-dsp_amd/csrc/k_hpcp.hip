// k_hpcp.hip — the key path's chroma (reference src/lib.rs:961-1559):
//
//   k_hpcp       HPCP chroma + frame energies over every bin        chroma/extractor.rs:529-680, 1097-1150
//   k_hpcp_band  the same after k_mask_rp (k_mask.hip): walks the peak band only, folds the frame
//                energy from the mask's block sums and bounds its distance from the reference's
//                sequential fold (energy_delta, the input of k_key_vote's certificate)
//
// One thread per frame walks its bins in order through an LDS-staged chunk and keeps the top-K
// peaks in a register-resident sorted list (HpcpFrame).
#include "block_utils.hpp"
#include "kernels.hpp"

namespace sdsp {

constexpr int HP_CW = 16;  // bins per staged chunk (LDS row stride 17: conflict-free)
constexpr int HPB_CW = HP_CW;  // k_hpcp_band's chunk (32: 164 VGPRs, 3 waves, 15 % slower in round 5)
static_assert(HPB_CW == 16, "k_hpcp_band stages a chunk as four 16-byte groups per row");
constexpr int HP_HU = 4;  // harmonic-table entries HpcpFrame::finish loads ahead per peak

// The per-frame HPCP state of one thread (extractor.rs:529-680 for one frame): the energy fold,
// the last two magnitudes for the local-maximum test, and a register-resident top-KCAP list
// ordered (magnitude desc, bin asc).  KCAP is the compile-time list capacity (>= K); the
// insertion is branch-free straight-line code over the KCAP slots.  Slots K..KCAP-1 hold the
// runners-up and are ignored at the end (the first K slots are exactly the top-K in order).
// thr = pm[KCAP-1]: a candidate must beat it to move anything.
template <int KCAP>
struct HpcpFrame {
    float e = 0.0f, m1 = 0.0f, m2 = 0.0f;  // m1 = m[b-1], m2 = m[b-2]
    float thr = -1.0f;
    float pm[KCAP];
    int pb[KCAP];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int q = 0; q < KCAP; q++) {
            pm[q] = -1.0f;  // empty slot; every real peak is > 0
            pb[q] = 0;
        }
    }
    // bins c0 .. c0+cw-1 of this frame, row[j] = m[c0 + j], in bin order
    template <bool ENERGY = true>
    __device__ __forceinline__ void walk(const float* row, int c0, int cw, const HpcpParams& P) {
        for (int j = 0; j < cw; j++) {
            const int b = c0 + j;
            const float m = row[j];
            if (ENERGY) e += m * m;
            const int c = b - 1;  // candidate peak bin, needs m[c-1] = m2, m[c] = m1, m[c+1] = m
            if (c >= P.pk_lo && c <= P.pk_hi && !(m1 <= m2 || m1 < m) && m1 > thr) {
                // insertion into the descending list: gt[q] = m1 > pm[q] is false then true along
                // the list (an equal magnitude already listed has the lower bin and stays
                // ahead), so slot q takes m1 where gt turns true and its predecessor after that.
                // Updated from the tail in place: one compare, one median and two selects per slot.
                bool gt[KCAP];
#pragma unroll
                for (int q = 0; q < KCAP; q++) gt[q] = m1 > pm[q];
                // the magnitudes: slot q takes the median of {pm[q], m1, pm[q-1]} (pm[q-1] >= pm[q]:
                // that is pm[q] if m1 <= pm[q], m1 between the two, pm[q-1] if m1 > pm[q-1]), one
                // v_med3 instead of two selects; exact, every operand is a number (m1 > thr >= -1)
#pragma unroll
                for (int q = KCAP - 1; q >= 1; q--) {
                    const int nbv = gt[q - 1] ? pb[q - 1] : c;
                    pm[q] = __builtin_amdgcn_fmed3f(pm[q], m1, pm[q - 1]);
                    pb[q] = gt[q] ? nbv : pb[q];
                }
                pm[0] = gt[0] ? m1 : pm[0];
                pb[0] = gt[0] ? c : pb[0];
                thr = pm[KCAP - 1];
            }
            m2 = m1;
            m1 = m;
        }
    }
    // harmonic summation of the top-K peaks into 12 pitch classes (pc[q][i]: this thread's
    // column of an LDS scratch), L2 normalisation, and the frame's chroma row and energy at g
    __device__ __forceinline__ void finish(float (*pc)[HP_FRAMES], int i, const HpcpParams& P,
                                           const HarmEntry* __restrict__ harm, float* __restrict__ chroma,
                                           float* __restrict__ energy, uint64_t g) {
#pragma unroll
        for (int q = 0; q < 12; q++) pc[q][i] = 0.0f;
#pragma unroll
        for (int k = 0; k < KCAP; k++) {
            if (k >= P.K || !(pm[k] > 0.0f)) continue;
            const int bin = pb[k];
            const float xk = sd_maxf(pm[k], 0.0f);
            float w0;
            if (P.p == 0.5f) {  // the default power: the correctly rounded sqrt where it is sd_powf's value
                const float s = __builtin_sqrtf(xk);
                w0 = sd_sqrt_is_powf_half(xk, s) ? s : sd_powf_ool(xk, 0.5f);
            } else {
                w0 = sd_powf_ool(xk, P.p);
            }
            if (w0 <= 0.0f) continue;
            // the peak's first HP_HU table entries (128 contiguous bytes) are loaded together, ahead of
            // their use, instead of one dependent load per harmonic; the accumulation order is the
            // same (h ascending, the walk ends at the first state-0 entry)
            HarmEntry hv[HP_HU];
#pragma unroll
            for (int h = 0; h < HP_HU; h++)
                if (h < P.hmax) hv[h] = harm[bin * HP_HMAX + h];
            bool stop = false;
#pragma unroll
            for (int h = 0; h < HP_HU; h++) {
                if (stop || h >= P.hmax) break;
                const HarmEntry& he = hv[h];
                if (he.state == 0) {
                    stop = true;
                    break;
                }
                if (he.state == 1) continue;
                const float contrib = w0 * he.hw;
                for (int o = 0; o < 3; o++) pc[he.tc[o]][i] += contrib * he.wt[o];
            }
            for (int h = HP_HU + 1; !stop && h <= P.hmax; h++) {
                const HarmEntry he = harm[bin * HP_HMAX + (h - 1)];
                if (he.state == 0) break;
                if (he.state == 1) continue;
                const float contrib = w0 * he.hw;
                for (int o = 0; o < 3; o++) pc[he.tc[o]][i] += contrib * he.wt[o];
            }
        }
        float nsq = 0.0f;
#pragma unroll
        for (int q = 0; q < 12; q++) nsq += pc[q][i] * pc[q][i];
        const float norm = __builtin_sqrtf(nsq);
#pragma unroll
        for (int q = 0; q < 12; q++) {
            float v = pc[q][i];
            if (norm > EPS) v /= norm;
            chroma[g * 12 + q] = v;
        }
        energy[g] = e;
    }
};

// 4 waves per SIMD: round 3 measured it 8 % faster than the 3-wave build (14.6 vs 15.9 ms per
// 256-track launch, then at 128 VGPRs with a 16-byte spill); with per-wave staging and the
// pitch-class scratch in its own LDS array the HPCP kernels take 112 VGPRs, no spill: hence
// amdgpu_waves_per_eu(4) on both kernels.
// One thread per frame, HP_FRAMES frames per workgroup.  Bins are staged through LDS in
// HP_CW-column chunks (coalesced row segments) and each thread walks its frame's bins in
// order (HpcpFrame).  Each wave stages the rows of its own 64 frames, so no workgroup barrier
// holds the waves together per chunk (as k_hpcp_band).
template <int KCAP>
__global__ __launch_bounds__(HP_FRAMES) __attribute__((amdgpu_waves_per_eu(4))) void k_hpcp(const float* __restrict__ mags,
                                                    const uint64_t* __restrict__ frame_pfx,
                                                    const uint64_t* __restrict__ tile_pfx,
                                                    const int* __restrict__ tracks, int n_items, HpcpParams P,
                                                    const HarmEntry* __restrict__ harm, float* __restrict__ chroma,
                                                    float* __restrict__ energy) {
    __shared__ float tile[HP_FRAMES][HP_CW + 1];
    __shared__ float pcs[12][HP_FRAMES];  // pitch-class accumulators (a column per thread)
    const uint64_t gb = blockIdx.x;
    const int it = find_track(tile_pfx, n_items, gb);
    const int trk = tracks[it];
    const int64_t F = (int64_t)(frame_pfx[trk + 1] - frame_pfx[trk]);
    const int64_t f0 = (int64_t)(gb - tile_pfx[it]) * HP_FRAMES;
    const int i = threadIdx.x;
    const int64_t f = f0 + i;
    const bool valid = f < F;
    const int lane = i & 63, wrow = i & ~63;
    const int64_t rows = F - f0 < HP_FRAMES ? F - f0 : HP_FRAMES;
    if (wrow >= rows) return;  // the whole wave is past the track's end
    const uint64_t g0 = frame_pfx[trk];
    HpcpFrame<KCAP> hf;
    hf.init();
    constexpr int RSTEP = 64 / HP_CW;
    constexpr int NLD = 64 / RSTEP;
    const int sub = lane / HP_CW, jj = lane % HP_CW;
    // software pipeline: chunk c0+HP_CW is loaded into registers while chunk c0 is walked
    const float* rowp = mags + (g0 + (uint64_t)f0 + (uint64_t)(wrow + sub)) * (uint64_t)P.stride + jj;
    const uint64_t rstride = (uint64_t)RSTEP * (uint64_t)P.stride;
    float nx[NLD];
    auto load_chunk = [&](int c0) {
        const bool col_ok = c0 + jj < P.B;
#pragma unroll
        for (int u = 0; u < NLD; u++)
            nx[u] = (wrow + sub + u * RSTEP < rows && col_ok) ? rowp[(uint64_t)u * rstride + c0] : 0.0f;
    };
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    load_chunk(0);
    for (int c0 = 0; c0 < P.B; c0 += HP_CW) {
        wave_sync();  // the previous chunk's walk has read its rows
#pragma unroll
        for (int u = 0; u < NLD; u++) tile[wrow + sub + u * RSTEP][jj] = nx[u];
        wave_sync();
        if (c0 + HP_CW < P.B) load_chunk(c0 + HP_CW);
        if (!valid) continue;
        hf.walk(tile[i], c0, P.B - c0 < HP_CW ? P.B - c0 : HP_CW, P);
    }
    if (!valid) return;
    hf.finish(pcs, i, P, harm, chroma, energy, g0 + (uint64_t)f);
}

// A rigorous bound on |e_blk - e_ref| / e_blk for one frame ("Certification"): e_blk
// is this engine's fold of the 65 block sums Bt_b (each an f32 fold of its 64 squares
// t_k = RN(x_k^2) from 0, k_mask_rp: two sequential halves of 32, then their sum; the g63 bound
// below holds for any association of 64 non-negative terms, since no term passes through more than
// 63 roundings), e_ref the reference's one sequential f32 fold of the same
// 4,097 squares (extractor.rs:1133).  With u = 2^-24, T = sum t_k (exact), B_b the exact block sums:
//   |Bt_b - B_b| <= g63 B_b, so B_b <= Bt_b / (1 - g63) =: Bu_b;
//   |e_blk - sum Bt_b| <= u (1 + g64) sum_b (Bt_0 + .. + Bt_b)   (one rounding per block fold step);
//   |sum Bt_b - T| <= g63 sum_b Bu_b;
//   |e_ref - T| <= sum_k |d_k|, d_k the rounding of the reference's step k: |d_k| <= t_k (its
//   partial sum S_{k-1} is a float next to S_{k-1} + t_k) and |d_k| <= u (1 + u) U_b for k in block
//   b, U_b = (Bu_0 + .. + Bu_b)(1 + gN) bounding every partial sum there (the terms are >= 0), so
//   block b adds at most min(Bu_b, n_b u (1 + u) U_b).
// Evaluated in double (relative error ~1e-14, covered by a 1e-9 factor) and rounded up to f32.
// e_blk = 0 means every square is +0, so both folds are +0 (bound 0).
__device__ float energy_delta(const float* __restrict__ pp, uint64_t total, int n_blocks, int B, float e_blk) {
    if (!(e_blk > 0.0f)) return 0.0f;
    const double u = 0x1p-24, g63 = 63.0 * u / (1.0 - 63.0 * u), g64 = 64.0 * u / (1.0 - 64.0 * u);
    const double gN = (double)B * u / (1.0 - (double)B * u), iu = 1.0 / (1.0 - g63);
    double pu = 0.0, pt = 0.0, eref = 0.0, eo = 0.0;
    for (int g = 0; g < n_blocks; g++) {
        const double bt = (double)pp[(uint64_t)g * total], bu = bt * iu;
        pu += bu;
        pt += bt;
        const int nb = B - 64 * g < 64 ? B - 64 * g : 64;
        eref += __builtin_fmin(bu, (double)nb * u * (1.0 + u) * pu * (1.0 + gN));
        eo += pt;
    }
    const double D = (eref + u * (1.0 + u) * (1.0 + g64) * eo + g63 * pu) * (1.0 + 1e-9);
    const double r = D / (double)e_blk;
    if (!(r < 1.0)) return 1.0f;  // no usable bound (cannot happen for finite sums); the vote flags it
    float d = (float)r;
    if ((double)d < r) d = __uint_as_float(__float_as_uint(d) + 1u);
    return d;
}

// energy_delta's bound from its terms accumulated in f32 (round 6): every term is >= 0 and every f32
// operation rounds to nearest, so each computed sum or product is at least (1 - 2^-24)^m of its exact
// value for the m <= 300 roundings on its path (the constants' included), and the computed bound
// times (1 + 2^-14) is an upper bound of the exact one (300 * 2^-24 = 1.8e-5 < 2^-14 = 6.1e-5, the
// final division's rounding included).  Outside e in [2^-60, 2^100] (no overflow; no denormal loses
// more than 2^-141 absolute against a bound >= 2^-78) the double evaluation runs instead.
constexpr float KC_IU_F = (float)(1.0 / (1.0 - 63.0 * 0x1p-24 / (1.0 - 63.0 * 0x1p-24)));
__device__ float energy_delta_f32(float e_blk, float pu, float eref, float eo, const float* __restrict__ pp,
                                  uint64_t total, int n_blocks, int B) {
    if (!(e_blk > 0.0f)) return 0.0f;
    if (!(e_blk >= 0x1p-60f && e_blk <= 0x1p100f)) return energy_delta(pp, total, n_blocks, B, e_blk);
    const float u = 0x1p-24f;
    const float g63 = 63.0f * u / (1.0f - 63.0f * u), g64 = 64.0f * u / (1.0f - 64.0f * u);
    const float D = eref + u * (1.0f + u) * (1.0f + g64) * eo + g63 * pu;
    const float r = (D / e_blk) * (1.0f + 0x1p-14f);
    if (!(r < 1.0f)) return 1.0f;  // no usable bound; the vote flags it
    return r;
}

// k_hpcp_band: k_hpcp after k_mask_rp.  The frame energy folds the 65 block sums part[g][frame] in
// block order; the bin walk covers only the band k_mask_rp stored, [pk_lo - 1, pk_hi + 1] (the
// local-maximum test of candidate c reads bins c - 1 .. c + 1; starting the walk at pk_lo - 1 with
// the walk's zero history gives exactly k_hpcp's candidates).  Each wave stages the 64 rows of its
// own frames, so the waves run without workgroup barriers: a wave whose frames insert more peaks
// does not hold the others at a barrier per chunk (a wave's LDS operations execute in order; a
// wave-level fence keeps the staging writes and the walk's reads in program order).
template <int KCAP>
__global__ __launch_bounds__(HP_FRAMES) __attribute__((amdgpu_waves_per_eu(4))) void k_hpcp_band(const float* __restrict__ mags,
                                                         const uint64_t* __restrict__ frame_pfx,
                                                         const uint64_t* __restrict__ tile_pfx,
                                                         const int* __restrict__ tracks, int n_items, HpcpParams P,
                                                         const HarmEntry* __restrict__ harm,
                                                         const float* __restrict__ part, int n_blocks, uint64_t total,
                                                         float* __restrict__ chroma, float* __restrict__ energy,
                                                         float* __restrict__ edel) {
    __shared__ float tile[HP_FRAMES][HPB_CW + 1];
    __shared__ float pcs[12][HP_FRAMES];  // pitch-class accumulators (a column per thread)
    const uint64_t gb = blockIdx.x;
    const int it = find_track(tile_pfx, n_items, gb);
    const int trk = tracks[it];
    const int64_t F = (int64_t)(frame_pfx[trk + 1] - frame_pfx[trk]);
    const int64_t f0 = (int64_t)(gb - tile_pfx[it]) * HP_FRAMES;
    const int i = threadIdx.x;
    const int64_t f = f0 + i;
    const bool valid = f < F;
    const int lane = i & 63, wrow = i & ~63;
    const int64_t rows = F - f0 < HP_FRAMES ? F - f0 : HP_FRAMES;
    if (wrow >= rows) return;  // the whole wave is past the track's end
    const uint64_t g0 = frame_pfx[trk];
    HpcpFrame<KCAP> hf;
    hf.init();
    if (valid) {
        const float* pp = part + g0 + (uint64_t)f;
        // the frame energy (pt: the block sums folded in block order) and, in the same pass, the
        // terms of the certificate's per-frame energy bound in f32 (energy_delta_f32; k_key_vote,
        // KeyParams::near_check)
        const float u = 0x1p-24f;
        const float gN = (float)P.B * u / (1.0f - (float)P.B * u);
        const float c64 = 64.0f * u * (1.0f + u) * (1.0f + gN);
        const float clast = (float)(P.B - 64 * (n_blocks - 1)) * u * (1.0f + u) * (1.0f + gN);
        float pt = 0.0f, pu = 0.0f, eref = 0.0f, eo = 0.0f;
        for (int g = 0; g < n_blocks; g++) {
            const float bt = pp[(uint64_t)g * total];
            pt += bt;
            const float bu = bt * KC_IU_F;
            pu += bu;
            eref += __builtin_fminf(bu, (g + 1 < n_blocks ? c64 : clast) * pu);
            eo += pt;
        }
        hf.e = pt;
        if (edel) edel[g0 + (uint64_t)f] = energy_delta_f32(pt, pu, eref, eo, pp, total, n_blocks, P.B);
    }
    const int w_lo = P.pk_lo - 1 > 0 ? P.pk_lo - 1 : 0, w_hi = P.pk_hi + 1 < P.B - 1 ? P.pk_hi + 1 : P.B - 1;
    // lane (r4, q4) stages bins 4 q4 .. 4 q4 + 3 of rows wrow + r4 + 16 u (u < 4), one 16-byte load
    // per row: a wave load covers 16 rows' 64-byte segments (4 with 4-byte loads: 8.8 % slower per
    // launch, round 5)
    typedef float f4v __attribute__((ext_vector_type(4)));
    const int r4 = lane >> 2, q4 = lane & 3;
    const f4v* rowp4 = reinterpret_cast<const f4v*>(mags + (g0 + (uint64_t)f0 + (uint64_t)(wrow + r4)) * (uint64_t)P.stride + 4 * q4);
    const uint64_t rstride4 = 4 * (uint64_t)P.stride;  // 16 rows, in f4v units
    f4v n4[4];
    auto load_chunk = [&](int c0) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            // a group wholly past w_hi is not read; one that starts at a bin b <= w_hi < B ends
            // inside the row (strides are multiples of 4 floats, at least B: b + 4 <= stride)
            const int b = c0 + 4 * q4;
            f4v v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (wrow + r4 + 16 * u < rows && b <= w_hi) v = rowp4[(uint64_t)u * rstride4 + (uint64_t)(c0 >> 2)];
            n4[u] = f4v{b <= w_hi ? v.x : 0.0f, b + 1 <= w_hi ? v.y : 0.0f, b + 2 <= w_hi ? v.z : 0.0f,
                        b + 3 <= w_hi ? v.w : 0.0f};
        }
    };
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    // chunks on HPB_CW-bin boundaries, so every 64-byte row segment is one aligned sector (rows
    // are 64-byte aligned); the bins below w_lo this adds are no candidates (c < pk_lo), they only
    // pass through the walk's two-bin history.  (From w_lo itself: 2.2-2.5 % slower; the chunk after
    // next in flight too: 20-25 % slower, at 4 waves with spills or at 3; round 5.)
    const int c_start = w_lo & ~(HPB_CW - 1);
    if (w_lo <= w_hi) load_chunk(c_start);
    for (int c0 = c_start; c0 <= w_hi; c0 += HPB_CW) {
        wave_sync();  // the previous chunk's walk has read its rows
#pragma unroll
        for (int u = 0; u < 4; u++) {
            float* tr = tile[wrow + r4 + 16 * u] + 4 * q4;
            tr[0] = n4[u].x;
            tr[1] = n4[u].y;
            tr[2] = n4[u].z;
            tr[3] = n4[u].w;
        }
        wave_sync();
        if (c0 + HPB_CW <= w_hi) load_chunk(c0 + HPB_CW);
        if (!valid) continue;
        hf.template walk<false>(tile[i], c0, w_hi + 1 - c0 < HPB_CW ? w_hi + 1 - c0 : HPB_CW, P);
    }
    if (!valid) return;
    hf.finish(pcs, i, P, harm, chroma, energy, g0 + (uint64_t)f);
}

// ---- launchers ----
void launch_hpcp_band(const float* mags, const uint64_t* frame_pfx, const uint64_t* tile_pfx, const int* tracks,
                      int n_items, uint64_t n_tiles, const HpcpParams& P, const HarmEntry* harm, const float* part,
                      uint64_t total, float* chroma, float* energy, float* edel, hipStream_t st) {
    if (n_tiles == 0) return;
    const int nblk = (P.B + MASK_T - 1) / MASK_T;
    const dim3 grid((unsigned)n_tiles), block(HP_FRAMES);
#define SDSP_HB(K)                                                                                                   \
    hipLaunchKernelGGL(k_hpcp_band<K>, grid, block, 0, st, mags, frame_pfx, tile_pfx, tracks, n_items, P, harm, part, \
                       nblk, total, chroma, energy, edel)
    if (P.K <= 8)
        SDSP_HB(8);
    else if (P.K <= 16)
        SDSP_HB(16);
    else if (P.K <= 24)
        SDSP_HB(24);
    else
        SDSP_HB(HP_KMAX);
#undef SDSP_HB
}
void launch_hpcp(const float* mags, const uint64_t* frame_pfx, const uint64_t* tile_pfx, const int* tracks,
                 int n_items, uint64_t n_tiles, const HpcpParams& P, const HarmEntry* harm, float* chroma,
                 float* energy, hipStream_t st) {
    if (n_tiles == 0) return;
    const dim3 grid((unsigned)n_tiles), block(HP_FRAMES);
    if (P.K <= 8)
        hipLaunchKernelGGL(k_hpcp<8>, grid, block, 0, st, mags, frame_pfx, tile_pfx, tracks, n_items, P, harm, chroma,
                           energy);
    else if (P.K <= 16)
        hipLaunchKernelGGL(k_hpcp<16>, grid, block, 0, st, mags, frame_pfx, tile_pfx, tracks, n_items, P, harm, chroma,
                           energy);
    else if (P.K <= 24)
        hipLaunchKernelGGL(k_hpcp<24>, grid, block, 0, st, mags, frame_pfx, tile_pfx, tracks, n_items, P, harm, chroma,
                           energy);
    else
        hipLaunchKernelGGL(k_hpcp<HP_KMAX>, grid, block, 0, st, mags, frame_pfx, tile_pfx, tracks, n_items, P, harm,
                           chroma, energy);
}

}  // namespace sdsp
