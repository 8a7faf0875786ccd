// k_levels.hip — the levels request's kernels (include/stratum_hip.h, sdsp_levels).
//
//   k_levels_fold    the per-track sequential folds of normalize()'s three methods
//                    (normalization.rs:183-259, 303, 337, 443, 464), up to four chains per track
//   k_levels_gain    the Loudness gain from the first launch's folds, for the second launch's chain
//   k_silence_map    detect_and_trim's silence regions from the trim pass's frame RMS (silence.rs:183-231)
//   k_silence_gather the kept regions of all tracks, dense
//
// The arithmetic (fold steps, gains, the keep-rule) is levels_core.hpp's, shared with the host.
#include "block_utils.hpp"
#include "kernels.hpp"
#include "levels_core.hpp"

namespace sdsp {

// ---- the folds ----
// The shape of k_loudness_gain: a workgroup owns LV_TPW tracks, loader waves stage the next
// LV_C-sample chunk of every track into the other half of a double-buffered LDS tile (half its
// chunk, see LV_C), and wave 0 folds.  Where k_loudness_gain folds on 16 of its 64 lanes, here
// lane = chain * 16 + track: the four chains of a track
//   0  sum x^2                         (RMS)
//   1  the K-weighting biquad with gated 400-ms block sums   (Loudness)
//   2  sum (x * g_peak)^2              (Peak's rms_db; g_peak from the peak kernel)
//   3  sum (x * g_lufs)^2              (Loudness' rms_db; a second launch, after k_levels_gain)
// read the same LDS addresses (broadcasts) and run beside each other.  So that they run *beside*
// each other and not one after the other under divergent exec masks, a launch with the biquad chain
// (BQ) runs one instruction stream on every lane: the biquad step on y = x * g, its output squared
// into the lane's sum.  A sum-of-squares lane carries the identity filter (b0 = 1, the other
// coefficients 0): its state stays +-0, o = 1 * y + (+-0) has y's value, so o * o is exactly y * y
// (finite samples; non-finite input is out of scope), and with g = 1 the product x * 1 is x.  Only
// the biquad lanes close blocks.  A launch without the biquad chain runs the plain square step.
constexpr int LV_TPW = 16;        // tracks per workgroup
// Samples per track per chunk.  k_loudness_gain's 1,024 make the tile 131 KB, which keeps every
// LDS-using kernel of the analysis off the workgroup's CU for as long as the folds run beside it
// (a quarter of the chip at 1,024 tracks): a step with the request cost +151 ms at 1,024, +106 ms at
// 512 (66 KB) and +96 ms at 256, the folds alone on an idle device 197 / 199 / 206 ms
// (tools/levels_bench.py, one run each of 5 repetitions; -DSDSP_LV_C builds the others).
#ifndef SDSP_LV_C
#define SDSP_LV_C 512
#endif
constexpr int LV_C = SDSP_LV_C;
static_assert(LV_C % 256 == 0, "a loader wave moves a chunk in 16-byte loads of 64 lanes");
constexpr int LV_ROW = LV_C + 4;  // LDS row stride (floats): rows start 4 banks apart
constexpr int LV_LOADERS = 8;     // loader waves
static_assert(LV_TPW * LV_CHAINS == 64, "lane = chain * LV_TPW + track fills the fold wave");

template <bool BQ>
__global__ __launch_bounds__(64 * (1 + LV_LOADERS)) void k_levels_fold(LvFoldArgs A, LvParams P) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    extern __shared__ float lv_tile[];  // [2][LV_TPW][LV_ROW]
    __shared__ uint64_t nmax_s, nmin_s;
    const float* __restrict__ x = A.x;
    const int w = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int t0 = blockIdx.x * LV_TPW;
    const int nt = A.T - t0 < LV_TPW ? A.T - t0 : LV_TPW;
    if (threadIdx.x == 0) nmax_s = 0, nmin_s = ~0ull;
    __syncthreads();
    if (w == 0 && lane < nt) {
        atomicMax((unsigned long long*)&nmax_s, (unsigned long long)A.n_raw[t0 + lane]);
        atomicMin((unsigned long long*)&nmin_s, (unsigned long long)A.n_raw[t0 + lane]);
    }
    __syncthreads();
    const uint64_t nch = (nmax_s + LV_C - 1) / LV_C;
    auto load = [&](uint64_t c, int buf) {  // loader waves: chunk c of every track (zeros past its end)
        float* base = lv_tile + (size_t)buf * LV_TPW * LV_ROW;
        const uint64_t s0 = c * LV_C;
        for (int tt = w - 1; tt < nt; tt += LV_LOADERS) {
            const uint64_t a = A.in_off[t0 + tt], n = A.n_raw[t0 + tt];
            float* row = base + tt * LV_ROW;
            if ((a & 3u) == 0 && s0 + LV_C <= n) {  // whole aligned chunk: 16-B loads
                const f4* q = reinterpret_cast<const f4*>(x + a + s0);
                f4 v[LV_C / 256];
#pragma unroll
                for (int i = 0; i < LV_C / 256; i++) v[i] = q[i * 64 + lane];
#pragma unroll
                for (int i = 0; i < LV_C / 256; i++) reinterpret_cast<f4*>(row)[i * 64 + lane] = v[i];
            } else {
                float v[LV_C / 64];
#pragma unroll
                for (int i = 0; i < LV_C / 64; i++) {
                    const uint64_t sm = s0 + (uint64_t)(i * 64 + lane);
                    v[i] = sm < n ? x[a + sm] : 0.0f;
                }
#pragma unroll
                for (int i = 0; i < LV_C / 64; i++) row[i * 64 + lane] = v[i];
            }
        }
    };
    if (w > 0 && nch > 0) load(0, 0);
    __syncthreads();

    // ---- wave 0: lane = chain * LV_TPW + track ----
    // Every track starts at sample 0, so the position inside the 400-ms block is the same on all
    // lanes: the block bookkeeping is wave-uniform, and a chunk every track fills runs without
    // per-lane tests.
    const int chain = lane / LV_TPW, tt = lane % LV_TPW;
    const bool act = w == 0 && tt < nt && ((A.chains >> chain) & 1u);
    const int t = t0 + (tt < nt ? tt : 0);
    const uint64_t n = act ? A.n_raw[t] : 0;
    const float g = act && chain >= 2 ? A.gains[(size_t)chain * A.T + t] : 1.0f;
    const bool isbq = chain == 1;
    LvBiquad q{1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (isbq) q = LvBiquad{P.b0, P.b1, P.b2, P.a1, P.a2, 0.0f, 0.0f};
    LvGated gs{0.0f, 0.0f, 0};  // bsum: the lane's running sum (the open block's on a biquad lane)
    const int64_t bs = P.block;
    int64_t cnt = 0;  // samples into the current block (uniform)
    auto step = [&](float v) {
        if (BQ) {
            const float o = lv_biquad(q, v * g);
            gs.bsum += o * o;
        } else {
            lv_square(gs.bsum, v, g);
        }
    };
    for (uint64_t c = 0; c < nch; c++) {
        const int buf = (int)(c & 1);
        if (w > 0) {
            if (c + 1 < nch) load(c + 1, buf ^ 1);
        } else {
            const float* row = lv_tile + (size_t)buf * LV_TPW * LV_ROW + tt * LV_ROW;
            const f4* row4 = reinterpret_cast<const f4*>(row);
            const uint64_t s0 = c * LV_C;
            if (s0 + LV_C <= nmin_s) {  // every track fills this chunk
                int i = 0;
                while (i < LV_C) {
                    // samples up to the next block end (or the chunk end), uniform
                    const int64_t room = BQ ? bs - cnt : (int64_t)LV_C;
                    const int e = (int64_t)(LV_C - i) < room ? LV_C : i + (int)room;
                    int k = i;
                    for (; k < e && (k & 3); k++) step(row[k]);
                    for (; k + 16 <= e; k += 16) {
                        const f4 v0 = row4[k / 4], v1 = row4[k / 4 + 1], v2 = row4[k / 4 + 2], v3 = row4[k / 4 + 3];
                        step(v0.x), step(v0.y), step(v0.z), step(v0.w);
                        step(v1.x), step(v1.y), step(v1.z), step(v1.w);
                        step(v2.x), step(v2.y), step(v2.z), step(v2.w);
                        step(v3.x), step(v3.y), step(v3.z), step(v3.w);
                    }
                    for (; k + 4 <= e; k += 4) {
                        const f4 v = row4[k / 4];
                        step(v.x), step(v.y), step(v.z), step(v.w);
                    }
                    for (; k < e; k++) step(row[k]);
                    if (BQ) {
                        cnt += e - i;
                        if (cnt == bs) {
                            if (isbq) lv_close_block(gs, bs, P.gate);
                            cnt = 0;
                        }
                    }
                    i = e;
                }
            } else {  // some track ends inside this chunk: per-lane bounds
                const int m = !act || s0 >= n ? 0 : (n - s0 < (uint64_t)LV_C ? (int)(n - s0) : LV_C);
                for (int k = 0; k < LV_C; k++) {
                    if (k < m) step(row[k]);
                    if (BQ && ++cnt == bs) {
                        if (isbq && k < m) lv_close_block(gs, bs, P.gate);
                        cnt = 0;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!act) return;
    if (isbq) {
        const int64_t rem = (int64_t)(n % (uint64_t)bs);
        if (rem > 0) lv_close_block(gs, rem, P.gate);  // this track's last, partial block
        A.sums[(size_t)A.T + t] = gs.gsum;
        A.gated_n[t] = gs.gn;
    } else {
        A.sums[(size_t)chain * A.T + t] = gs.bsum;
    }
}

// chain 3's gain: what normalize_lufs multiplies by, from the first launch's gated sums
__global__ void k_levels_gain(const unsigned int* __restrict__ peak_bits, const float* __restrict__ sums,
                              const int* __restrict__ gated_n, int T, LvParams P, float* __restrict__ gains) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    LvFolds f{};
    f.peak = sd_from_bits_f(peak_bits[t]);
    f.gsum = sums[(size_t)T + t];
    f.gn = gated_n[t];
    int st;
    gains[(size_t)3 * T + t] = lv_lufs_gain(f, P, &st);
}

void launch_levels_fold(const LvFoldArgs& A, const LvParams& P, hipStream_t st) {
    if (A.T == 0 || (A.chains & 15u) == 0) return;
    const size_t lds = 2 * LV_TPW * LV_ROW * sizeof(float);
    auto kern = (A.chains & 2u) ? k_levels_fold<true> : k_levels_fold<false>;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3((A.T + LV_TPW - 1) / LV_TPW), dim3(64 * (1 + LV_LOADERS)), lds, st, A, P);
}
void launch_levels_gain(const unsigned int* peak_bits, const float* sums, const int* gated_n, int T, const LvParams& P,
                        float* gains, hipStream_t st) {
    if (T == 0) return;
    hipLaunchKernelGGL(k_levels_gain, dim3((T + 255) / 256), dim3(256), 0, st, peak_bits, sums, gated_n, T, P, gains);
}

// ---- the silence map ----
// One workgroup per track over the frame-RMS row k_trim reads (frame f at rms[base_pfx[t] + f *
// stride]), in tiles of 256 frames.  A run of silent frames ends at a non-silent frame f whose
// predecessor is silent; its start follows the last non-silent frame before f, an inclusive max
// scan of (non-silent ? f : -1) over the tile on top of the value carried from the earlier tiles
// (so a run may span any number of tiles).  Kept runs (lv_keep_run) are written in order by an
// ordered compaction; the run that reaches the last frame is closed after the walk.  Track t's
// regions go to regions[2 * cap_pfx[t] ...] as (start, end) sample pairs, count[t] of them.
__global__ __launch_bounds__(256) void k_silence_map(const float* __restrict__ rms, const uint64_t* __restrict__ frame_pfx,
                                                     const uint64_t* __restrict__ base_pfx, int stride,
                                                     const uint64_t* __restrict__ n_raw, int hop, float thr,
                                                     uint64_t min_frames, const uint64_t* __restrict__ cap_pfx,
                                                     uint64_t* __restrict__ regions, int* __restrict__ count) {
    __shared__ long long wlast[4];
    __shared__ int red[5];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t n = n_raw[t];
    const int64_t nf = (int64_t)(frame_pfx[t + 1] - frame_pfx[t]);
    const int64_t cap = (int64_t)(cap_pfx[t + 1] - cap_pfx[t]);
    const float* r = rms + base_pfx[t];
    uint64_t* out = regions + 2 * cap_pfx[t];
    long long carry = -1;  // the last non-silent frame before the tile
    int64_t kept = 0;
    for (int64_t f0 = 0; f0 < nf; f0 += 256) {
        const int64_t f = f0 + tid;
        const bool in = f < nf;
        const bool loud = in && !(r[f * stride] <= thr);
        long long v = loud ? (long long)f : -1;
        for (int o = 1; o < 64; o <<= 1) {
            const long long u = __shfl_up(v, o, 64);
            if (lane >= o && u > v) v = u;
        }
        const long long prev = __shfl_up(v, 1, 64);  // the wave's scan up to the lane before
        if (lane == 63) wlast[w] = v;
        __syncthreads();
        long long before = carry;  // ... up to the wave before
        for (int i = 0; i < w; i++) before = wlast[i] > before ? wlast[i] : before;
        const long long last = lane == 0 ? before : (prev > before ? prev : before);  // last non-silent frame < f
        for (int i = 0; i < 4; i++) carry = wlast[i] > carry ? wlast[i] : carry;
        const bool end = loud && f > 0 && last < f - 1;  // frame f - 1 is silent: the run [last + 1, f) ends here
        const bool keep = end && lv_keep_run((uint64_t)(last + 1), (uint64_t)f, min_frames);
        int tot;
        const int slot = block_exclusive_flag(keep, red, &tot);  // (its barriers also fence wlast)
        if (keep && kept + slot < cap) {
            out[2 * (kept + slot)] = (uint64_t)(last + 1) * (uint64_t)hop;
            out[2 * (kept + slot) + 1] = (uint64_t)f * (uint64_t)hop;
        }
        kept += tot;
    }
    if (tid != 0) return;
    if (nf > 0 && carry < nf - 1 && lv_keep_run((uint64_t)(carry + 1), (uint64_t)nf, min_frames)) {  // trailing run
        if (kept < cap) {
            out[2 * kept] = (uint64_t)(carry + 1) * (uint64_t)hop;
            out[2 * kept + 1] = n;
        }
        kept++;
    }
    count[t] = (int)(kept < cap ? kept : cap);
}

// pfx[t] = regions kept by the tracks before t (pfx[T] the total); track t's pairs to dense[2 * pfx[t] ...]
__global__ __launch_bounds__(256) void k_silence_gather(int T, const int* __restrict__ count,
                                                        const uint64_t* __restrict__ cap_pfx,
                                                        const uint64_t* __restrict__ regions, uint64_t* __restrict__ pfx,
                                                        uint64_t* __restrict__ dense) {
    __shared__ int red[4];
    const int t = blockIdx.x;
    int s = 0;
    for (int i = threadIdx.x; i < t; i += blockDim.x) s += count[i];
    const uint64_t base = (uint64_t)block_sum_i(s, red);
    const int c = count[t];
    if (threadIdx.x == 0) {
        pfx[t] = base;
        if (t == T - 1) pfx[T] = base + (uint64_t)c;
    }
    const uint64_t* src = regions + 2 * cap_pfx[t];
    for (int i = threadIdx.x; i < 2 * c; i += blockDim.x) dense[2 * base + i] = src[i];
}

void launch_silence_map(const float* rms, const uint64_t* frame_pfx, const uint64_t* base_pfx, int stride, int T,
                        const uint64_t* n_raw, int hop, float thr, uint64_t min_frames, const uint64_t* cap_pfx,
                        uint64_t* regions, int* count, uint64_t* pfx, uint64_t* dense, hipStream_t st) {
    if (T == 0) return;
    hipLaunchKernelGGL(k_silence_map, dim3(T), dim3(256), 0, st, rms, frame_pfx, base_pfx ? base_pfx : frame_pfx,
                       base_pfx ? stride : 1, n_raw, hop, thr, min_frames, cap_pfx, regions, count);
    hipLaunchKernelGGL(k_silence_gather, dim3(T), dim3(256), 0, st, T, count, cap_pfx, regions, pfx, dense);
}

}  // namespace sdsp
