// k_r128.hip — the programme loudness request's kernels (include/stratum_hip.h, sdsp_r128).
//
//   k_r128_steps   z[j]: the K-weighted energy of every 100-ms step of every track, each from a
//                  filter restarted one step earlier — a throughput kernel over (track, step)
//   k_r128_peak    the sample peak and the 4x-interpolated true peak, one lane per 4 samples
//   k_r128_track   per track: the blocks, both gates, the ordered means, the two order statistics
//                  and the maxima, from z; any track length, no scratch
//
// The arithmetic (filter step, block folds, gates, ranks) is r128_core.hpp's, shared with the host.
#include "block_utils.hpp"
#include "kernels.hpp"
#include "r128_core.hpp"

namespace sdsp {

// ---- the step energies ----
// A lane owns R128_M consecutive steps of one track and walks R128_M + 1 segments of `step` samples:
// the one before its first step, then its own.  On every sample it advances two independent
// chains: A, restarted from zero at each segment's start (the warm-up of the next step), and B,
// which starts each segment from the state A left at the end of the previous one and sums its
// squared output (the step's own energy).  So a step's 2 * step-long chain is exactly the
// contract's, each sample is fetched once for both of its uses, only the lane's first segment is
// read without being measured (1 / R128_M more traffic), and the two chains give the scheduler
// independent work inside the latency-bound recurrence.
// Feeding: a workgroup is one wave; its 64 lanes read 64 streams R128_M * step samples apart, so
// the wave stages the next R128_C samples of every stream into an LDS tile with coalesced loads
// (half a row per 32 lanes) and each lane then reads its own row with 16-byte loads.  Rows are
// R128_C + 4 floats apart: 16 lanes' b128 reads cover the 64 banks once (a stride of `step` words
// would put every lane on one bank at 48 kHz).  The next chunk's loads are issued before the
// current chunk's arithmetic and written to the tile after it.
constexpr int R128_M = 8;
constexpr int R128_C = 32;
constexpr int R128_ROW = R128_C + 4;
constexpr int R128_WG_STEPS = 64 * R128_M;  // steps per workgroup
static_assert(R128_C == 32, "a staging load covers two rows of 32 samples");

__global__ __launch_bounds__(64) void k_r128_steps(R128StepArgs A, R128Params P) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float tile[64 * R128_ROW];
    const int lane = threadIdx.x;
    const int t = find_track(A.bpfx, A.T, (uint64_t)blockIdx.x);
    const uint64_t step = P.step;
    const uint64_t J = A.n_raw[t] / step;
    const uint64_t j0 = ((uint64_t)blockIdx.x - A.bpfx[t]) * R128_WG_STEPS;  // < J: the track has this block
    const float* __restrict__ x = A.x + A.in_off[t];
    float* __restrict__ z = A.z + A.zpfx[t];
    const int imax = J - j0 < (uint64_t)R128_M ? (int)(J - j0) : R128_M;  // lane 0 owns the most steps
    const int nck = (int)((step + R128_C - 1) / R128_C);
    const int total = (imax + 1) * nck;
    const int64_t s0 = (int64_t)j0 + (int64_t)lane * R128_M;  // the lane's first own step

    // chunk c of the walk: samples [k0, k0 + cnt) of segment first + i of every row
    float v[R128_C];
    auto fetch = [&](int c) {
        const int i = c / nck;
        const uint64_t k0 = (uint64_t)(c % nck) * R128_C;
        const int col = lane & 31;
        const bool in = k0 + (uint64_t)col < step;
#pragma unroll
        for (int q = 0; q < R128_C; q++) {
            const int row = 2 * q + (lane >> 5);
            const int64_t seg = (int64_t)j0 + (int64_t)row * R128_M - 1 + i;
            const bool ok = in && seg >= 0 && (uint64_t)seg < J;  // (inside the track: seg * step + k0 + col < J * step <= n)
            v[q] = ok ? x[(uint64_t)seg * step + k0 + (uint64_t)col] : 0.0f;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int q = 0; q < R128_C; q++) tile[(2 * q + (lane >> 5)) * R128_ROW + (lane & 31)] = v[q];
    };

    R128Chain a{}, b{};
    float zs = 0.0f;
    auto one = [&](float s) {
        r128_kweight(a, P.shelf, P.hp, s);
        const float o = r128_kweight(b, P.shelf, P.hp, s);
        zs += o * o;
    };
    const float* row = tile + lane * R128_ROW;
    fetch(0);
    for (int c = 0; c < total; c++) {
        __syncthreads();  // the tile's readers are done
        store();
        __syncthreads();
        if (c + 1 < total) fetch(c + 1);
        const int i = c / nck, ck = c % nck;
        const int cnt = (uint64_t)(ck + 1) * R128_C <= step ? R128_C : (int)(step - (uint64_t)ck * R128_C);
        if (cnt == R128_C) {
#pragma unroll
            for (int k = 0; k < R128_C; k += 4) {
                const f4 w = *reinterpret_cast<const f4*>(row + k);
                one(w.x), one(w.y), one(w.z), one(w.w);
            }
        } else {
            for (int k = 0; k < cnt; k++) one(row[k]);
        }
        if (ck == nck - 1) {  // the segment ends: B measured step seg (not in the lane's first segment)
            const int64_t seg = s0 - 1 + i;
            if (i >= 1 && (uint64_t)seg < J) z[seg] = zs;
            b = a;
            if (seg < 0) b = R128Chain{};  // step 0 has no warm-up
            a = R128Chain{};
            zs = 0.0f;
        }
    }
}

void launch_r128_steps(const R128StepArgs& A, uint64_t n_blocks, const R128Params& P, hipStream_t st) {
    if (A.T == 0 || n_blocks == 0) return;
    hipLaunchKernelGGL(k_r128_steps, dim3((unsigned)n_blocks), dim3(64), 0, st, A, P);
}
uint64_t r128_step_blocks(uint64_t J) { return (J + R128_WG_STEPS - 1) / R128_WG_STEPS; }

// ---- the peaks ----
// A workgroup takes R128_PK_TILE consecutive samples of one track with their 5 + 6 neighbours into
// LDS (coalesced, zeros outside the track); a lane reads 16 consecutive values with four 16-byte
// loads and forms its 4 outputs' |x| and, with TP, their 3 interpolated values each.  The maxima
// are folded as the unsigned bits of non-negative floats: a tree in the block, one atomic per block.
constexpr int R128_PK_TILE = 1024;
constexpr int R128_PK_LDS = R128_PK_TILE + 16;

template <bool TP>
__global__ __launch_bounds__(256) void k_r128_peak(const float* __restrict__ xall, const uint64_t* __restrict__ in_off,
                                                   const uint64_t* __restrict__ n_raw,
                                                   const uint64_t* __restrict__ cpfx, int T, R128Params P,
                                                   unsigned int* __restrict__ peak_bits) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float w[R128_PK_LDS];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int t = find_track(cpfx, T, (uint64_t)blockIdx.x);
    const uint64_t n = n_raw[t];
    const float* __restrict__ x = xall + in_off[t];
    const uint64_t i0 = ((uint64_t)blockIdx.x - cpfx[t]) * R128_PK_TILE;  // < n
    for (int q = tid; q < R128_PK_LDS; q += 256) {
        const int64_t at = (int64_t)i0 + q - R128_AHEAD;
        w[q] = at >= 0 && (uint64_t)at < n ? x[at] : 0.0f;
    }
    __syncthreads();
    float r[16];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const f4 u = *reinterpret_cast<const f4*>(w + 4 * tid + 4 * k);
        r[4 * k] = u.x, r[4 * k + 1] = u.y, r[4 * k + 2] = u.z, r[4 * k + 3] = u.w;
    }
    float sp = 0.0f, tp = 0.0f;
#pragma unroll
    for (int o = 0; o < 4; o++) {
        if (i0 + (uint64_t)(4 * tid + o) >= n) break;
        sp = max_bnn(sp, sd_absf(r[o + R128_AHEAD]));
        if (TP) {
#pragma unroll
            for (int p = 0; p < 3; p++) tp = max_bnn(tp, sd_absf(r128_interp(P.h[p], r + o)));
        }
    }
    sp = block_max(sp, red);
    if (TP) tp = block_max(max_bnn(tp, sp), red);
    if (tid == 0) {
        atomicMax(&peak_bits[t], sd_bits_f(sp));
        if (TP) atomicMax(&peak_bits[T + t], sd_bits_f(tp));
    }
}

uint64_t r128_peak_blocks(uint64_t n) { return (n + R128_PK_TILE - 1) / R128_PK_TILE; }
// peak_bits: 2 * T words, zeroed here; [t] the sample peak, [T + t] the true peak (0 without tp)
void launch_r128_peak(const float* x, const uint64_t* in_off, const uint64_t* n_raw, const uint64_t* cpfx, int T,
                      uint64_t n_blocks, const R128Params& P, bool tp, unsigned int* peak_bits, hipStream_t st) {
    if (T == 0) return;
    (void)hipMemsetAsync(peak_bits, 0, 2 * (size_t)T * sizeof(unsigned int), st);
    if (n_blocks == 0) return;
    auto kern = tp ? k_r128_peak<true> : k_r128_peak<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_blocks), dim3(256), 0, st, x, in_off, n_raw, cpfx, T, P, peak_bits);
}

// ---- per track ----
// One workgroup per track over its z.  The blocks are formed 256 at a time, one per thread (every
// thread folds its own 4 or 30 steps in ascending order), into LDS tiles; thread 0 then folds the
// momentary tile and thread 64 the short-term tile, sequentially in block order, carrying their sums
// from tile to tile.  Two such walks: the absolute gate's means and the maxima, then the relative
// gate's.  The order statistics need no sorted copy: a radix select over the bit patterns of the
// surviving short-term blocks (non-negative floats order as their bits), which recomputes the
// blocks on each of its 4 passes and counts with integer atomics in LDS.
// curves (or NULL): track t's momentary blocks at curves[cvpfx[t] ...], its short-term blocks behind.
namespace {
template <class F>
__device__ float r128_select(uint64_t n, uint64_t k, F value, int* hist, uint64_t* misc) {
    uint32_t prefix = 0, mask = 0;
    uint64_t kk = k;
    for (int pass = 3; pass >= 0; pass--) {
        const int shift = pass * 8;
        for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        for (uint64_t j = threadIdx.x; j < n; j += blockDim.x) {
            float s;
            if (!value(j, &s)) continue;
            const uint32_t u = sd_bits_f(s);
            if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255], 1);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t acc = 0;
            int d = 0;
            for (d = 0; d < 255; d++) {
                if (acc + (uint64_t)hist[d] > kk) break;
                acc += (uint64_t)hist[d];
            }
            misc[0] = (uint64_t)d;
            misc[1] = kk - acc;
        }
        __syncthreads();
        prefix |= (uint32_t)misc[0] << shift;
        mask |= 255u << shift;
        kk = misc[1];
        __syncthreads();
    }
    return sd_from_bits_f(prefix);
}
}  // namespace

__global__ __launch_bounds__(256) void k_r128_track(const float* __restrict__ zall, const uint64_t* __restrict__ zpfx,
                                                    const uint64_t* __restrict__ cvpfx, R128Params P,
                                                    R128Folds* __restrict__ out, float* __restrict__ curves) {
    __shared__ float tm[256], ts[256];
    __shared__ float gr_s[2];
    __shared__ uint64_t cnt_s[2];
    __shared__ int hist[256];
    __shared__ uint64_t misc[2];
    __shared__ int red[4];
    const int t = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ z = zall + zpfx[t];
    const uint64_t J = zpfx[t + 1] - zpfx[t];
    const uint64_t nm = r128_n_mom(J), ns = r128_n_short(J);
    const uint32_t step = P.step;
    const float ga = P.gate;
    float* cm = curves ? curves + cvpfx[t] : nullptr;
    float* cs = curves ? cm + nm : nullptr;
    R128Folds f{};
    // thread 0 folds the momentary blocks, thread 64 the short-term blocks
    const bool fm = tid == 0, fs = tid == 64;
    const float* tile = fm ? tm : ts;
    const uint64_t nb = fm ? nm : ns;
    for (int walk = 0; walk < 2; walk++) {
        R128Mean acc{0.0f, 0};
        float mx = 0.0f;
        float gr = 0.0f;
        if (walk == 1) {
            gr = gr_s[fm ? 0 : 1];
            if (cnt_s[0] == 0) break;  // (uniform) nothing above the absolute gate: no second mean
        }
        for (uint64_t j0 = 0; j0 < nm; j0 += 256) {
            const uint64_t j = j0 + (uint64_t)tid;
            if (j < nm) {
                const float m = r128_momentary(z, j, step);
                tm[tid] = m;
                if (walk == 0 && cm) cm[j] = m;
            }
            if (walk == 0 && j < ns) {
                const float s = r128_short_term(z, j, step);
                ts[tid] = s;
                if (cs) cs[j] = s;
            }
            __syncthreads();
            if ((fm || (fs && walk == 0)) && j0 < nb) {
                const int m = nb - j0 < 256 ? (int)(nb - j0) : 256;
                for (int k = 0; k < m; k++) {
                    const float e = tile[k];
                    r128_mean_add(acc, e, walk == 0 ? e > ga : (e > ga && e > gr));
                    mx = max_bnn(mx, e);
                }
            }
            __syncthreads();
        }
        if (walk == 0) {
            if (fm || fs) {
                cnt_s[fm ? 0 : 1] = acc.n;
                gr_s[fm ? 0 : 1] = acc.n ? r128_mean(acc) * (fm ? 0.1f : 0.01f) : 0.0f;
                if (fm) f.max_m = mx;
            }
            if (fs) ts[0] = mx;  // (to thread 0, which writes the folds)
            __syncthreads();
            if (fm) f.max_s = ts[0];
            __syncthreads();
        } else if (fm) {
            f.gated_sum = acc.sum;
            f.n_gated = acc.n;
        }
    }
    // the short-term survivors and their two order statistics
    if (cnt_s[1] > 0) {
        const float gr = gr_s[1];
        auto value = [&](uint64_t j, float* s) {
            *s = r128_short_term(z, j, step);
            return r128_short_pass(*s, ga, gr);
        };
        int c = 0;
        for (uint64_t j = tid; j < ns; j += 256) {
            float s;
            c += value(j, &s);
        }
        const uint64_t M = (uint64_t)block_sum_i(c, red);
        f.n_gated_short = M;
        if (M) {
            f.low = r128_select(ns, r128_rank_low(M), value, hist, misc);
            f.high = r128_select(ns, r128_rank_high(M), value, hist, misc);
        }
    }
    if (tid == 0) out[t] = f;
}

void launch_r128_track(const float* z, const uint64_t* zpfx, const uint64_t* cvpfx, int T, const R128Params& P,
                       R128Folds* out, float* curves, hipStream_t st) {
    if (T == 0) return;
    hipLaunchKernelGGL(k_r128_track, dim3(T), dim3(256), 0, st, z, zpfx, cvpfx, P, out, curves);
}

}  // namespace sdsp
