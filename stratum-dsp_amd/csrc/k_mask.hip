// k_mask.hip — the key path's time masks (reference src/lib.rs:961-1559):
//
//   k_mask      harmonic_spectrogram_time_mask + smooth_spectrogram_time  chroma/extractor.rs:1246-1349
//   k_mask_r    the same for the default margin 12, power 2: rings in registers
//   k_mask_rp   k_mask_r before k_hpcp_band: stores HPCP's peak band only, folds the frame energies
//
// k_mask: one thread per (track, bin) streams the track's frames in order, carrying the
// reference's sequential per-bin f32 prefix sum (prefix[t+1] = prefix[t] + x) in a 2M+2-slot
// ring in LDS; adjacent lanes touch adjacent bins of the same frame, so every HBM access is a
// coalesced 1 KB row segment.  The mask is applied in place.  The workgroup is one wave of
// MASK_T = 64 bins (kernels.hpp): 4097 bins = 64 full waves + 1 lane.
#include "block_utils.hpp"
#include "kernels.hpp"

namespace sdsp {

constexpr int MASK_U = 16;  // frames loaded ahead per thread (independent HBM loads in flight)

// LDS: prefix ring pre[2M+2][MASK_T] and raw ring raw[M+1][MASK_T] (dynamic, sized by M).
// Ring slots advance by counters (no runtime modulo): the prefix for en = min(t+M+1, F) is
// always the last one written; st = max(t-M, 0) advances once t > M; raw[t] was written M
// frames earlier.
// PW: 2 -> power 2 (x*x, the default), 1 -> power 1, 0 -> any other power (sd_powf); keeps the
// unrolled body free of the general pow code.
template <int PW>
__device__ __forceinline__ float mask_pow(float x, float p) {
    if (PW == 2) return x * x;
    if (PW == 1) return x;
    return sd_powf(x, p);
}

template <int PW>
__global__ __launch_bounds__(MASK_T) void k_mask(float* __restrict__ mags, int stride, int B,
                                                  const uint64_t* __restrict__ frame_pfx, const int* __restrict__ tracks,
                                                  int blocks_per_track, int margin, float power, int smooth_only) {
    extern __shared__ float mask_lds[];
    const int it = blockIdx.x / blocks_per_track;
    const int trk = tracks[it];
    const int b = (blockIdx.x % blocks_per_track) * MASK_T + threadIdx.x;
    const int64_t F = (int64_t)(frame_pfx[trk + 1] - frame_pfx[trk]);
    if (b >= B || F <= 0) return;
    float* col = mags + frame_pfx[trk] * (uint64_t)stride + b;
    const int M = margin;
    const int R = 2 * M + 2, RX = M + 1;
    float* pre = mask_lds + threadIdx.x;
    float* raw = mask_lds + (size_t)R * MASK_T + threadIdx.x;
    const float p = sd_maxf(power, 1.0f);
    const float eps = 1e-12f;
    pre[0] = 0.0f;
    float prev = 0.0f;
    int w_slot = 0;   // slot of prefix[min(tin+1, F)] after this step's write (= en's slot)
    int s_slot = 0;   // slot of prefix[st]
    int xw = 0;       // raw write slot (tin % RX)
    int xr = 0;       // raw read slot (t % RX)
    for (int64_t base = 0; base < F + M; base += MASK_U) {
        float xv[MASK_U];
#pragma unroll
        for (int u = 0; u < MASK_U; u++) {
            const int64_t tin = base + u;
            xv[u] = tin < F ? col[tin * stride] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < MASK_U; u++) {
            const int64_t tin = base + u;
            if (tin >= F + M) break;
            if (tin < F) {
                prev = prev + xv[u];
                w_slot = w_slot + 1 == R ? 0 : w_slot + 1;
                pre[w_slot * MASK_T] = prev;
                raw[xw * MASK_T] = xv[u];
                xw = xw + 1 == RX ? 0 : xw + 1;
            }
            const int64_t t = tin - M;
            if (t < 0) continue;
            const int64_t st = t >= M ? t - M : 0;
            const int64_t en = t + M + 1 < F ? t + M + 1 : F;
            const float denom = (float)(en - st > 1 ? en - st : 1);
            const float x_raw = M == 0 ? xv[u] : raw[xr * MASK_T];
            // margin 0: smooth_spectrogram_time returns its input unchanged (extractor.rs:1250-1252)
            const float hm = M == 0 ? x_raw : (pre[w_slot * MASK_T] - pre[s_slot * MASK_T]) / denom;
            if (smooth_only) {  // smooth_spectrogram_time alone (src/lib.rs:1042-1055)
                col[t * stride] = hm;
                if (M > 0) xr = xr + 1 == RX ? 0 : xr + 1;
                if (t >= M) s_slot = s_slot + 1 == R ? 0 : s_slot + 1;
                continue;
            }
            const float x = max_bnn(x_raw, 0.0f);
            const float h = max_bnn(hm, 0.0f);
            const float r = max_bnn(x - h, 0.0f);
            const float hp = mask_pow<PW>(h, p);
            const float rp = mask_pow<PW>(r, p);
            const float m = hp / (hp + rp + eps);
            col[t * stride] = x * m;
            if (M > 0) xr = xr + 1 == RX ? 0 : xr + 1;
            if (t >= M) s_slot = s_slot + 1 == R ? 0 : s_slot + 1;
        }
    }
}

// Register-ring variant for a compile-time margin M (the default 12): the prefix ring
// (R = 2M+2 slots) and the raw ring (M+1 slots) live in VGPRs and the frame loop is unrolled
// by R, so every slot index is static.  Edges need no special case: frames past the end
// contribute x = 0 (prefix + 0 == prefix, so P[min(t+M+1, F)] is read as P[t+M+1]), and
// prefixes of negative index are the ring's initial zeros (== P[0]) because slot (t-M) mod R
// is not written before t >= M.  R loads are issued ahead of each unrolled block.
// One masked element: window sum a over `den` frames and the raw value xr -> xr * mask
// (extractor.rs:1281-1285 then 1320-1340).  For the full window (2M+1 frames) a/(2M+1) is one
// product and one FMA correction, == the correctly rounded quotient for every f32 a in
// {0} U [2^-90, 2^120] (tools/check_div.c: exhaustive, every odd window 3..25); otherwise the
// IEEE division.
template <int M, int PW>
__device__ __forceinline__ float mask_elem(float a, int64_t den, float xr, float p, float inv_w) {
    float hm;
    if (den == 2 * M + 1 && (a == 0.0f || (a >= 0x1p-90f && a <= 0x1p120f))) {
        const float q0 = a * inv_w;
        hm = __builtin_fmaf(__builtin_fmaf(-q0, (float)(2 * M + 1), a), inv_w, q0);
    } else {
        hm = a / (float)(den > 1 ? den : 1);
    }
    const float x = max_bnn(xr, 0.0f);
    const float h = max_bnn(hm, 0.0f);
    const float r = max_bnn(x - h, 0.0f);
    const float hp = mask_pow<PW>(h, p);
    const float rp = mask_pow<PW>(r, p);
    const float m = hp / (hp + rp + 1e-12f);
    return x * m;
}

template <int M, int PW>
__global__ __launch_bounds__(MASK_T) void k_mask_r(float* __restrict__ mags, int stride, int B,
                                                    const uint64_t* __restrict__ frame_pfx,
                                                    const int* __restrict__ tracks, int blocks_per_track,
                                                    float power) {
    constexpr int R = 2 * M + 2, RX = M + 1;
    static_assert(M >= 1 && (2 * M + 1) % 2 == 1 && 2 * M + 1 <= 25, "fast window division validated for 3..25");
    const int it = blockIdx.x / blocks_per_track;
    const int trk = tracks[it];
    const int b = (blockIdx.x % blocks_per_track) * MASK_T + threadIdx.x;
    const int64_t F = (int64_t)(frame_pfx[trk + 1] - frame_pfx[trk]);
    if (b >= B || F <= 0) return;
    float* col = mags + frame_pfx[trk] * (uint64_t)stride + b;
    const float p = sd_maxf(power, 1.0f);
    const float inv_w = 1.0f / (float)(2 * M + 1);
    float P[R], X[RX];
#pragma unroll
    for (int j = 0; j < R; j++) P[j] = 0.0f;
#pragma unroll
    for (int j = 0; j < RX; j++) X[j] = 0.0f;
    float prev = 0.0f;
    auto emit = [&](float a, int64_t den, float xr, int64_t t) {
        __builtin_nontemporal_store(mask_elem<M, PW>(a, den, xr, p, inv_w), &col[t * stride]);
    };
    for (int64_t base = 0; base < F + M; base += R) {
        float xv[R];
        if (base >= 2 * M && base + R <= F) {
            // interior block: every step has a full window; no edge conditions
#pragma unroll
            for (int u = 0; u < R; u++) xv[u] = __builtin_nontemporal_load(&col[(base + u) * stride]);
#pragma unroll
            for (int u = 0; u < R; u++) {
                prev = prev + xv[u];
                P[(u + 1) % R] = prev;
                X[u % RX] = xv[u];
                emit(P[(u + 1) % R] - P[(u + R - 2 * M) % R], 2 * M + 1, X[(u + 1) % RX], base + u - M);
            }
            continue;
        }
#pragma unroll
        for (int u = 0; u < R; u++) xv[u] = base + u < F ? __builtin_nontemporal_load(&col[(base + u) * stride]) : 0.0f;
#pragma unroll
        for (int u = 0; u < R; u++) {
            const int64_t tin = base + u;
            prev = prev + xv[u];  // == prev once tin >= F (x = 0)
            P[(u + 1) % R] = prev;
            X[u % RX] = xv[u];
            const int64_t t = tin - M;
            if (t >= 0 && t < F) {
                const int64_t st = t >= M ? t - M : 0;
                const int64_t en = t + M + 1 < F ? t + M + 1 : F;
                emit(P[(u + 1) % R] - P[(u + R - 2 * M) % R], en - st, X[(u + 1) % RX], t);
            }
        }
    }
}

// k_mask_rp: k_mask_r for the default HPCP path, which reads the masked spectrogram only on its
// peak band [st_lo, st_hi] (extractor.rs:583-671: peaks in [pk_lo, pk_hi] and their neighbours)
// and otherwise only folds the frame energy sum(x * x) over every bin (extractor.rs:1133).  The
// masked value is stored only on that band; for every frame the workgroup's 64 bins (block g) fold
// their squares into part[g][frame] (an LDS tile: lane = bin writes, then lanes u and u + 32 fold the
// two 32-bin halves of the row of frame base + u - M in bin order and the halves are added), and
// HPCP folds the 65 block sums in block order.  Only that fold's association differs from the
// reference's one sequential sum over 4,097 bins (a GPU-only re-association of the key energies,
// DESIGN.md §2); every masked value is bit-identical.
// Lanes past the last bin stay in the wave and contribute +0 (exact: the sums are >= +0).
// The block fold's two lanes per frame measured 1.8 % faster per launch than one lane folding all
// 64 squares, and than two interleaved chains of 16 per lane (profiles/r06_kernel_ab_mask_fold.txt).
template <int M, int PW>
__global__ __launch_bounds__(MASK_T) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_mask_rp(float* __restrict__ mags, int stride, int B,
                                                     const uint64_t* __restrict__ frame_pfx,
                                                     const int* __restrict__ tracks, int blocks_per_track,
                                                     float power, int st_lo, int st_hi, float* __restrict__ part,
                                                     uint64_t total, int outside) {
    constexpr int R = 2 * M + 2, RX = M + 1;
    static_assert(M >= 1 && 2 * M + 1 <= 25 && R <= MASK_T, "fast window division validated for 3..25");
    __shared__ float tile[R][MASK_T + 1];
    const int it = blockIdx.x / blocks_per_track;
    const int trk = tracks[it];
    const int gblk = blockIdx.x % blocks_per_track;
    const int lane = threadIdx.x;
    const int b = gblk * MASK_T + lane;
    const int64_t F = (int64_t)(frame_pfx[trk + 1] - frame_pfx[trk]);
    if (F <= 0) return;  // the whole workgroup
    // outside: store the bins outside [st_lo, st_hi] instead (the exact rerun's completion of a
    // spectrogram whose band already holds masked values); a block wholly inside stores nothing
    if (outside && gblk * MASK_T >= st_lo && gblk * MASK_T + MASK_T - 1 <= st_hi) return;
    const bool live = b < B;
    const bool keep = live && (outside ? (b < st_lo || b > st_hi) : (b >= st_lo && b <= st_hi));
    // Rows are addressed through buffer resources whose base is the row (wave-uniform, advanced in
    // SGPRs) and lane offsets in VGPRs: no 64-bit address arithmetic per element.  A store
    // resource spans one row (B floats) and the lanes off HPCP's band carry an offset past it, so
    // the hardware drops their stores without an exec-mask branch per element.
    float* const trk0 = mags + frame_pfx[trk] * (uint64_t)stride;
    const uint32_t lvo = (uint32_t)(live ? b : 0) * 4u;
    // lanes past the last bin load through an offset past the row resource's range: the hardware
    // returns 0 without an exec-mask branch per load
    const uint32_t lvo_z = live ? (uint32_t)b * 4u : 0x80000000u;
    const uint32_t svo = keep ? (uint32_t)b * 4u : 0x80000000u;
    const uint32_t rowb = (uint32_t)stride * 4u;
    auto row_rsrc = [&](int64_t row, uint32_t bytes) {
        return __builtin_amdgcn_make_buffer_rsrc((void*)(trk0 + row * (int64_t)stride), (short)0, (int)bytes, 0x00020000);
    };
    float* pg = part + (uint64_t)gblk * total + frame_pfx[trk];
    const float p = sd_maxf(power, 1.0f);
    const float inv_w = 1.0f / (float)(2 * M + 1);
    float P[R], X[RX];
#pragma unroll
    for (int j = 0; j < R; j++) P[j] = 0.0f;
#pragma unroll
    for (int j = 0; j < RX; j++) X[j] = 0.0f;
    float prev = 0.0f;
    auto finish = [&](float v, int64_t t, int u) {
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), row_rsrc(t, (uint32_t)B * 4u), svo, 0, 2 /* nt */);
        tile[u][lane] = v * v;  // lanes past the last bin load x = 0, so v = 0 * (0 / 1e-12) = +0
    };
    // interior element: the full window's quotient by the product + FMA correction, exact on
    // {0} U [2^-90, 2^120] (mask_elem); a wave with a lane outside that range (tiny non-zero or huge
    // window sums) redoes that lane by the IEEE division, behind a wave-uniform branch.  chk =
    // false: the block's range test (below) already holds for every lane of the wave
    auto emit_full = [&](float a, float xr, int64_t t, int u, bool chk = true) {
        const float q0 = a * inv_w;
        float hm = __builtin_fmaf(__builtin_fmaf(-q0, (float)(2 * M + 1), a), inv_w, q0);
        // outside {+-0} U [2^-90, 2^120] (negative, NaN: sign or exponent bits above the range)
        const uint32_t ab = __float_as_uint(a);
        const bool bad = ((ab << 1) != 0u) & (ab - 0x12800000u > 0x7B800000u - 0x12800000u);
        if (chk && __builtin_expect(__builtin_amdgcn_ballot_w64(bad) != 0, 0))
            if (bad) hm = a / (float)(2 * M + 1);
        // the block test (chk = false) also certifies every sample of the block and the ring finite
        // and >= +0, and then a >= +0 and its correctly rounded quotient hm >= +0: both max(., 0)
        // are the identity there
        const float x = chk ? max0_quiet(xr) : xr;
        const float h = chk ? max0_quiet(hm) : hm;
        const float r = max_bnn(x - h, 0.0f);
        const float hp = mask_pow<PW>(h, p);
        const float rp = mask_pow<PW>(r, p);
        const float den = hp + rp + 1e-12f;
        if (!chk) {  // the block's range test holds (below)
            const float y = __builtin_amdgcn_rcpf(den);
            const float y1 = __builtin_fmaf(__builtin_fmaf(-den, y, 1.0f), y, y);
            const float q0 = hp * y1;
            finish(x * __builtin_fmaf(__builtin_fmaf(-den, q0, hp), y1, q0), t, u);
            return;
        }
        finish(x * (hp / den), t, u);
    };
    // the block's partial sums: the 64 squares of frame base + u - M, folded in bin order
    auto fold = [&](int64_t base) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        {
            // two lanes per frame (u, u + 32), each folding half of the block's bins in bin order,
            // the halves added at the end
            const int fu = lane & 31, hf = lane >> 5;
            const int64_t t = base + fu - M;
            float sum = 0.0f;
            if (fu < R) {
#pragma unroll
                for (int j = 0; j < MASK_T / 2; j++) sum += tile[fu][hf * (MASK_T / 2) + j];
            }
            const float hi = __shfl_down(sum, 32);
            if (hf == 0 && fu < R && t >= 0 && t < F) pg[t] = sum + hi;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    // the next block's loads are issued as soon as the current block's values are consumed, so
    // they are in flight during the block-sum fold (its 64-step chains would otherwise stall them)
    float xv[R];
    auto load_block = [&](int64_t base) {
        const auto rs = row_rsrc(base, 0x7FFFFFFFu);
        if (base >= 2 * M && base + R <= F) {
#pragma unroll
            for (int u = 0; u < R; u++) xv[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, lvo_z, (uint32_t)u * rowb, 2));
        } else {
#pragma unroll
            for (int u = 0; u < R; u++)
                xv[u] = (live && base + u < F) ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, lvo, (uint32_t)u * rowb, 2))
                                               : 0.0f;
        }
    };
    load_block(0);
    for (int64_t base = 0; base < F + M; base += R) {
        if (base >= 2 * M && base + R <= F) {
            // interior block: every step has a full window; no edge conditions
            // the per-element range checks once per block.  P is non-decreasing and every window
            // sum a = P1 - P0 has P1 in [P[base + 1], P[base + R]]; a nonzero difference is at
            // least half an ulp of P1 (or P1 / 2), so a = 0 or a >= P[base + 1] 2^-25, and the
            // sequential prefix rounds up by at most (1 + 2^-24)^R, so a <= 2^60.01 when prev +
            // R max(x) <= 2^60.  With P[base + 1] >= 2^-21: a is 0 or in [2^-46, 2^61] (the window
            // quotient's exact range), hp = h^2 is 0 or >= 2^-103 (the mask quotient's residual is
            // exact), and with P[base + 1] >= max(x) 2^-31, hp / den >= 2^-124 (r <= x), hp, rp and
            // den stay below 2^112: the reciprocal + Newton + FMA-residual quotient is then the
            // correctly rounded one (tools/check_div_fast.hip, D1, every mantissa pair).  max(x)
            // covers the block's samples and the raw ring (the centres x of the block's first
            // elements are the previous block's).  A block and past of zeros is exact on either
            // path.  NaN and inf fail the tests.
            // max(x) over the block and the ring as unsigned bit patterns: for values with a clear
            // sign bit that is the float maximum, and a NaN, an infinity or a negative value (sign bit)
            // makes it >= 0x7F800000, so the test below also certifies every value finite and >= +0
            uint32_t mb = __float_as_uint(xv[0]);
#pragma unroll
            for (int u = 1; u < R; u++) mb = max(mb, __float_as_uint(xv[u]));
#pragma unroll
            for (int j = 0; j < RX; j++) mb = max(mb, __float_as_uint(X[j]));
            const float mx = __uint_as_float(mb);
            const float pf = prev + xv[0];
            const bool ok = mb < 0x7F800000u && (prev + mx == 0.0f || (pf >= 0x1p-21f && pf >= mx * 0x1p-31f &&
                                                                        prev + (float)R * mx <= 0x1p60f));
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) == 0, 1)) {
#pragma unroll
                for (int u = 0; u < R; u++) {
                    prev = prev + xv[u];
                    P[(u + 1) % R] = prev;
                    X[u % RX] = xv[u];
                    emit_full(P[(u + 1) % R] - P[(u + R - 2 * M) % R], X[(u + 1) % RX], base + u - M, u, false);
                }
            } else
#pragma unroll
            for (int u = 0; u < R; u++) {
                prev = prev + xv[u];
                P[(u + 1) % R] = prev;
                X[u % RX] = xv[u];
                emit_full(P[(u + 1) % R] - P[(u + R - 2 * M) % R], X[(u + 1) % RX], base + u - M, u);
            }
        } else {
#pragma unroll
            for (int u = 0; u < R; u++) {
                const int64_t tin = base + u;
                prev = prev + xv[u];  // == prev once tin >= F (x = 0)
                P[(u + 1) % R] = prev;
                X[u % RX] = xv[u];
                const int64_t t = tin - M;
                if (t >= 0 && t < F) {
                    const int64_t st = t >= M ? t - M : 0;
                    const int64_t en = t + M + 1 < F ? t + M + 1 : F;
                    finish(mask_elem<M, PW>(P[(u + 1) % R] - P[(u + R - 2 * M) % R], en - st, X[(u + 1) % RX], p, inv_w),
                           t, u);
                }
            }
        }
        if (base + R < F + M) load_block(base + R);
        fold(base);
    }
}

// ---- launchers ----
void launch_mask(float* mags, int stride, int B, const uint64_t* frame_pfx, const int* tracks, int n_items, int margin,
                 float power, hipStream_t st, bool smooth_only) {
    if (n_items == 0) return;
    const int bpt = (B + MASK_T - 1) / MASK_T;
    const size_t lds = (size_t)(2 * margin + 2 + margin + 1) * MASK_T * sizeof(float);
    const float p = sd_maxf(power, 1.0f);
    if (smooth_only) {
        if (margin == 0) return;  // smooth_spectrogram_time returns its input (extractor.rs:1250-1252)
        hipLaunchKernelGGL(k_mask<1>, dim3(n_items * bpt), dim3(MASK_T), lds, st, mags, stride, B, frame_pfx, tracks,
                           bpt, margin, power, 1);
        return;
    }
    if (margin == 12 && p == 2.0f) {
        hipLaunchKernelGGL((k_mask_r<12, 2>), dim3(n_items * bpt), dim3(MASK_T), 0, st, mags, stride, B, frame_pfx,
                           tracks, bpt, power);
        return;
    }
    if (p == 2.0f)
        hipLaunchKernelGGL(k_mask<2>, dim3(n_items * bpt), dim3(MASK_T), lds, st, mags, stride, B, frame_pfx, tracks,
                           bpt, margin, power, 0);
    else if (p == 1.0f)
        hipLaunchKernelGGL(k_mask<1>, dim3(n_items * bpt), dim3(MASK_T), lds, st, mags, stride, B, frame_pfx, tracks,
                           bpt, margin, power, 0);
    else
        hipLaunchKernelGGL(k_mask<0>, dim3(n_items * bpt), dim3(MASK_T), lds, st, mags, stride, B, frame_pfx, tracks,
                           bpt, margin, power, 0);
}
bool mask_band_ok(int margin, float power) { return margin == 12 && sd_maxf(power, 1.0f) == 2.0f; }
void launch_mask_band(float* mags, int stride, int B, const uint64_t* frame_pfx, const int* tracks, int n_items,
                      float power, int st_lo, int st_hi, float* part, uint64_t total, hipStream_t st, bool outside) {
    if (n_items == 0) return;
    const int bpt = (B + MASK_T - 1) / MASK_T;
    hipLaunchKernelGGL((k_mask_rp<12, 2>), dim3(n_items * bpt), dim3(MASK_T), 0, st, mags, stride, B, frame_pfx, tracks,
                       bpt, power, st_lo, st_hi, part, total, outside ? 1 : 0);
}

}  // namespace sdsp
