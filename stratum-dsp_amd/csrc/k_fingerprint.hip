// k_fingerprint.hip — the fingerprint request (include/stratum_hip.h, sdsp_fingerprint; the arithmetic
// in fingerprint_core.hpp): cell means of the smoothed chroma rows, the words, and the comparison of
// every pair of a call's tracks at every offset.
//
//   k_fp_cells   one lane per (cell, pitch class): m[c][i], the mean of C[f][i] over the cell's key frames
//   k_fp_words   one lane per word: three 12-float rows of m in, one word out, into the call's word buffer
//   k_fp_match   one block per FP_TA x FP_TB tile of (a, b) tracks: a dense (o, has, e, n) record per pair
//
// The match walks the words of its a-tracks in chunks of FP_CH positions.  Per chunk the block stages
// the a-tracks' words and, with an O-word halo on both sides, the b-tracks' into LDS (zeros outside a
// track), so a word fetched from L2 serves FP_TB (an a-word) or FP_TA (a b-word) pairs at 2 O + 1
// offsets each.  A wave owns one a-track and its FP_TB pairs; a lane owns an offset, 64 offsets per
// pass, NP passes (a template parameter: the accumulators of every pass stay in registers across
// chunks).  A[p] is one LDS address for the whole wave (a broadcast), B[p + o] is consecutive across
// lanes (no bank conflict).  The range of p and "counted" are predicates; e and n are two VGPR
// accumulators per (pair, pass), e through the popcount's add operand.  A wave-wide butterfly over
// fp_rec_before, a strict total order, picks the best offset: the record does not depend on the
// reduction's order, and nothing is appended atomically.
#include "fingerprint_core.hpp"
#include "kernels.hpp"

namespace sdsp {

namespace {
constexpr int FP_CELLS = 16;  // k_fp_cells: cells per block, 12 lanes each

// the track of item u: the last t in [0, n) with pfx[t] <= u (u < pfx[n])
__device__ __forceinline__ int fp_track_of(const uint64_t* __restrict__ pfx, int n, uint64_t u) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pfx[mid] <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}
}  // namespace

__global__ __launch_bounds__(FP_CELLS * 12) void k_fp_cells(const float* __restrict__ chroma_s,
                                                            const uint64_t* __restrict__ frame_pfx,
                                                            const uint64_t* __restrict__ cell_pfx, int n_tracks,
                                                            uint64_t n_cells, uint64_t Cs, uint64_t khop,
                                                            float* __restrict__ m) {
    const int sl = (int)threadIdx.x / 12, i = (int)threadIdx.x - 12 * sl;
    const uint64_t u = (uint64_t)blockIdx.x * FP_CELLS + (uint64_t)sl;
    if (u >= n_cells) return;
    const int t = fp_track_of(cell_pfx, n_tracks, u);
    const uint64_t c = u - cell_pfx[t];
    m[u * 12 + i] = sc_cell_mean(chroma_s + frame_pfx[t] * 12 + i, 12, sc_first(c, Cs, khop), sc_first(c + 1, Cs, khop));
}

__global__ __launch_bounds__(256) void k_fp_words(const float* __restrict__ m, const uint64_t* __restrict__ cell_pfx,
                                                  const uint64_t* __restrict__ word_pfx, const uint64_t* __restrict__ slot,
                                                  int n_tracks, uint64_t n_words, uint32_t* __restrict__ words) {
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= n_words) return;
    const int t = fp_track_of(word_pfx, n_tracks, u);
    const uint64_t w = u - word_pfx[t];  // (< the track's n_cells - 2: rows w, w + 1, w + 2 exist)
    const float* r = m + (cell_pfx[t] + w) * 12;
    words[slot[t] + w] = fp_word(r, r + 12, r + 24);
}

// The pairs (ia, jb), jb > ia, of the compared tracks [0, NC): track k's words at words + slot[k], W[k]
// of them (>= 1).  The launch covers the a-rows [row0, row0 + rows); the pair's record goes to
// rec[(ia - row0) * NC + jb].  O <= 32 NP - 1.
template <int NP>
__global__ __launch_bounds__(FP_TA * 64) void k_fp_match(const uint32_t* __restrict__ words,
                                                         const uint64_t* __restrict__ slot,
                                                         const uint32_t* __restrict__ W, int NC, int row0, int rows, int O,
                                                         uint32_t need, FpRec* __restrict__ rec) {
    constexpr int SB = FP_CH + 64 * NP;  // staged b-words per track: FP_CH + 2 O at most
    __shared__ uint32_t sA[FP_TA][FP_CH];
    __shared__ uint32_t sB[FP_TB][SB];
    const int tid = (int)threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int ia0 = row0 + (int)blockIdx.y * FP_TA, jb0 = (int)blockIdx.x * FP_TB;
    if (jb0 + FP_TB - 1 <= ia0) return;  // (the whole block: no pair with jb > ia in this tile)
    const int a_end = min(row0 + rows, NC);
    // this wave's a-track and the tile's b-tracks; a pair that does not exist gets Wb = 0
    const int ia = ia0 + wv;
    const int Wa = ia < a_end ? (int)W[ia] : 0;
    int Wb[FP_TB], Wa_max = 0;
    for (int a = 0; a < FP_TA; a++)
        if (ia0 + a < a_end) Wa_max = max(Wa_max, (int)W[ia0 + a]);
#pragma unroll
    for (int b = 0; b < FP_TB; b++) Wb[b] = (jb0 + b < NC && jb0 + b > ia && Wa > 0) ? (int)W[jb0 + b] : 0;
    // per pass this lane's offset and the range [lo, hi) of its positions; hi <= lo: none (also a lane past O)
    int lo[NP], hi[FP_TB][NP];
    uint32_t e[FP_TB][NP], n[FP_TB][NP];
#pragma unroll
    for (int ps = 0; ps < NP; ps++) {
        const int o = lane + 64 * ps - O;
        lo[ps] = (int)fp_lo(o);
#pragma unroll
        for (int b = 0; b < FP_TB; b++) {
            hi[b][ps] = (o <= O && Wb[b] > 0) ? (int)fp_hi(Wa, Wb[b], o) : 0;
            e[b][ps] = 0;
            n[b][ps] = 0;
        }
    }
    const int LB = FP_CH + 2 * O;
    for (int p0 = 0; p0 < Wa_max; p0 += FP_CH) {
        __syncthreads();  // (the previous chunk is read)
        // track by track: its length and slot are read once (block-uniform), its words by consecutive lanes
        for (int a = 0; a < FP_TA; a++) {
            const int k = ia0 + a;
            const int Wk = k < a_end ? (int)W[k] : 0;
            const uint32_t* src = words + (k < a_end ? slot[k] : 0);
            for (int q = tid; q < FP_CH; q += FP_TA * 64) sA[a][q] = p0 + q < Wk ? src[p0 + q] : 0u;
        }
        // (the columns [LB, SB) of sB are never written: only lanes past O read them, and their hi is 0)
        for (int b = 0; b < FP_TB; b++) {
            const int k = jb0 + b;
            const int Wk = k < NC ? (int)W[k] : 0;
            const uint32_t* src = words + (k < NC ? slot[k] : 0);
            for (int q = tid; q < LB; q += FP_TA * 64) {
                const int p = p0 - O + q;
                sB[b][q] = (p >= 0 && p < Wk) ? src[p] : 0u;
            }
        }
        __syncthreads();
        const int q_end = min(FP_CH, Wa - p0);
        for (int q = 0; q < q_end; q++) {
            const uint32_t a = sA[wv][q];
            const int p = p0 + q;
#pragma unroll
            for (int b = 0; b < FP_TB; b++) {
                if (Wb[b] == 0) continue;  // (wave-uniform)
#pragma unroll
                for (int ps = 0; ps < NP; ps++) {
                    const uint32_t x = sB[b][q + lane + 64 * ps];  // B[p + o]: index q + o + O
                    const bool c = fp_counted(a, x) && p >= lo[ps] && p < hi[b][ps];
                    e[b][ps] = fp_popc(c ? a ^ x : 0u) + e[b][ps];
                    n[b][ps] += c ? 1u : 0u;
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < FP_TB; b++) {
        const int jb = jb0 + b;
        if (!(ia < a_end && jb < NC && jb > ia)) continue;  // (wave-uniform)
        FpRec best{0, 0, 0, 0};
#pragma unroll
        for (int ps = 0; ps < NP; ps++) {
            const int o = lane + 64 * ps - O;
            const FpRec c{o, (o <= O && n[b][ps] >= need) ? 1u : 0u, e[b][ps], n[b][ps]};
            if (fp_rec_before(c, best)) best = c;
        }
        for (int d = 32; d >= 1; d >>= 1) {
            FpRec y;
            y.o = __shfl_xor(best.o, d, 64);
            y.has = (uint32_t)__shfl_xor((int)best.has, d, 64);
            y.e = (uint32_t)__shfl_xor((int)best.e, d, 64);
            y.n = (uint32_t)__shfl_xor((int)best.n, d, 64);
            if (fp_rec_before(y, best)) best = y;
        }
        if (lane == 0) rec[(uint64_t)(ia - row0) * (uint64_t)NC + (uint64_t)jb] = best.has ? best : FpRec{0, 0, 0, 0};
    }
}

void launch_fp_cells(const float* chroma_s, const uint64_t* frame_pfx, const uint64_t* cell_pfx, int n_tracks,
                     uint64_t n_cells, uint64_t Cs, uint64_t khop, float* m, hipStream_t st) {
    if (n_tracks <= 0 || n_cells == 0) return;
    hipLaunchKernelGGL(k_fp_cells, dim3((unsigned)((n_cells + FP_CELLS - 1) / FP_CELLS)), dim3(FP_CELLS * 12), 0, st,
                       chroma_s, frame_pfx, cell_pfx, n_tracks, n_cells, Cs, khop, m);
}

void launch_fp_words(const float* m, const uint64_t* cell_pfx, const uint64_t* word_pfx, const uint64_t* slot, int n_tracks,
                     uint64_t n_words, uint32_t* words, hipStream_t st) {
    if (n_tracks <= 0 || n_words == 0) return;
    hipLaunchKernelGGL(k_fp_words, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st, m, cell_pfx, word_pfx, slot,
                       n_tracks, n_words, words);
}

void launch_fp_match(const uint32_t* words, const uint64_t* slot, const uint32_t* W, int NC, int row0, int rows, int O,
                     uint32_t need, FpRec* rec, hipStream_t st) {
    if (NC < 2 || rows <= 0 || O < 0 || O > (int)FP_OMAX) return;
    const dim3 grid((unsigned)((NC + FP_TB - 1) / FP_TB), (unsigned)((rows + FP_TA - 1) / FP_TA)), block(FP_TA * 64);
    if (O < 32)
        hipLaunchKernelGGL(k_fp_match<1>, grid, block, 0, st, words, slot, W, NC, row0, rows, O, need, rec);
    else if (O < 64)
        hipLaunchKernelGGL(k_fp_match<2>, grid, block, 0, st, words, slot, W, NC, row0, rows, O, need, rec);
    else if (O < 128)
        hipLaunchKernelGGL(k_fp_match<4>, grid, block, 0, st, words, slot, W, NC, row0, rows, O, need, rec);
    else
        hipLaunchKernelGGL(k_fp_match<8>, grid, block, 0, st, words, slot, W, NC, row0, rows, O, need, rec);
}

}  // namespace sdsp
