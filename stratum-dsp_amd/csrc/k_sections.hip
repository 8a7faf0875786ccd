// k_sections.hip — the sections request (include/stratum_hip.h, sdsp_sections; the arithmetic in
// sections_core.hpp): cell means of the base pass's frame energies and of the smoothed chroma rows,
// the checkerboard novelty over cells, and the boundary rule.
//
//   k_section_energy    one lane per cell: g[c], the mean of E[f] over the cell's base frames
//   k_section_chroma    one lane per (cell, pitch class): m[c][i], the mean of C[f][i] over its key frames
//   k_section_novelty   one block per (track, 64-cell tile): N[c]
//   k_section_pick      one block per (track, 64-cell tile): the boundary flag of each cell
//
// Grids run over the call's cells (or tiles), all tracks' back to back (cell_pfx, tile_pfx), so a
// track of any length spreads over blocks and per-track features stay in HBM.  The novelty block
// stages its tile with a K-cell halo on each side into LDS as rows of SC_ROW floats (m, then e = g / gmax,
// gmax by a block-wide maximum over the track's g) and folds cross, wp and wf on one wave each, lane
// = cell, every fold sequential in the definition's order.  Boundaries need Nmax and up to G neighbours
// on either side, which cross tiles, so they are picked by a second launch once every N is written.
#include "block_utils.hpp"
#include "kernels.hpp"
#include "sections_core.hpp"

namespace sdsp {

namespace {
constexpr int SC_NT = 3 * SC_TILE;               // k_section_novelty: cross, wp, wf on a wave each
constexpr int SC_HALO = SC_TILE + 2 * SC_KMAX;   // staged cells at most
constexpr int SC_CH_CELLS = 16;                  // k_section_chroma: cells per block, 12 lanes each

// the track of item u: the last t in [0, n) with pfx[t] <= u (u < pfx[n])
__device__ __forceinline__ int sc_track_of(const uint64_t* __restrict__ pfx, int n, uint64_t u) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pfx[mid] <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}
}  // namespace

__global__ __launch_bounds__(256) void k_section_energy(const float* __restrict__ E, const uint64_t* __restrict__ row0,
                                                        const uint64_t* __restrict__ cell_pfx, int n_tracks,
                                                        uint64_t n_cells, uint64_t Cs, uint64_t hop,
                                                        float* __restrict__ g) {
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= n_cells) return;
    const int t = sc_track_of(cell_pfx, n_tracks, u);
    const uint64_t c = u - cell_pfx[t];
    g[u] = sc_cell_mean(E + row0[t], 1, sc_first(c, Cs, hop), sc_first(c + 1, Cs, hop));
}

__global__ __launch_bounds__(SC_CH_CELLS * 12) void k_section_chroma(const float* __restrict__ chroma_s,
                                                                    const uint64_t* __restrict__ frame_pfx,
                                                                    const uint64_t* __restrict__ cell_pfx, int n_tracks,
                                                                    uint64_t n_cells, uint64_t Cs, uint64_t khop,
                                                                    float* __restrict__ m) {
    const int sl = (int)threadIdx.x / 12, i = (int)threadIdx.x - 12 * sl;
    const uint64_t u = (uint64_t)blockIdx.x * SC_CH_CELLS + (uint64_t)sl;
    if (u >= n_cells) return;
    const int t = sc_track_of(cell_pfx, n_tracks, u);
    const uint64_t c = u - cell_pfx[t];
    m[u * 12 + i] = sc_cell_mean(chroma_s + frame_pfx[t] * 12 + i, 12, sc_first(c, Cs, khop), sc_first(c + 1, Cs, khop));
}

__global__ __launch_bounds__(SC_NT) void k_section_novelty(const float* __restrict__ m, const float* __restrict__ g,
                                                           const uint64_t* __restrict__ cell_pfx,
                                                           const uint64_t* __restrict__ tile_pfx, int n_tracks, int K,
                                                           float w, float* __restrict__ N) {
    __shared__ float rows[SC_HALO * SC_ROW];
    __shared__ float part[3][SC_TILE];
    __shared__ float red[SC_NT / 64];
    const int tid = (int)threadIdx.x;
    const int t = sc_track_of(tile_pfx, n_tracks, blockIdx.x);
    const uint64_t cell0 = cell_pfx[t];
    const int64_t n_cells = (int64_t)(cell_pfx[t + 1] - cell0);
    const int64_t c0 = (int64_t)(blockIdx.x - tile_pfx[t]) * SC_TILE;  // (< n_cells: the tile exists)
    const float* gk = g + cell0;
    const float* mk = m + cell0 * 12;
    float mx = gk[0];
    for (int64_t j = tid; j < n_cells; j += SC_NT) mx = sd_maxf(mx, gk[j]);
    const float gmax = block_max(mx, red);
    // rows[r] holds cell c0 - K + r, for the cells of [c0 - K, c0 + SC_TILE + K) inside the track
    const int64_t lo = c0 - K;
    const int n_rows = SC_TILE + 2 * K;
    for (int j = tid; j < n_rows * 12; j += SC_NT) {
        const int r = j / 12, i = j - 12 * r;
        const int64_t c = lo + r;
        if (c >= 0 && c < n_cells) rows[r * SC_ROW + i] = mk[c * 12 + i];
    }
    for (int r = tid; r < n_rows; r += SC_NT) {
        const int64_t c = lo + r;
        if (c >= 0 && c < n_cells) rows[r * SC_ROW + 12] = sc_rel_energy(gk[c], gmax);
    }
    __syncthreads();
    const int role = tid >> 6, lane = tid & 63;
    const int64_t c = c0 + lane;
    const bool scored = c < n_cells && sc_scored((uint64_t)c, (uint64_t)n_cells, (uint64_t)K);
    float v = 0.0f;
    if (scored) {  // cell c is row lane + K; its folds read rows [lane, lane + 2 K)
        const int64_t rc = lane + K;
        v = role == 0 ? sc_cross(rows, rc, K, w) : sc_within(rows, role == 1 ? rc - K : rc, K, w);
    }
    part[role][lane] = v;
    __syncthreads();
    if (role == 0 && c < n_cells)
        N[cell0 + (uint64_t)c] = scored ? sc_combine(part[0][lane], part[1][lane], part[2][lane], K) : 0.0f;
}

__global__ __launch_bounds__(SC_TILE) void k_section_pick(const float* __restrict__ N,
                                                          const uint64_t* __restrict__ cell_pfx,
                                                          const uint64_t* __restrict__ tile_pfx, int n_tracks,
                                                          uint64_t G, float min_strength, uint8_t* __restrict__ boundary) {
    __shared__ float red[1];
    const int t = sc_track_of(tile_pfx, n_tracks, blockIdx.x);
    const uint64_t cell0 = cell_pfx[t];
    const uint64_t n_cells = cell_pfx[t + 1] - cell0;
    const uint64_t c = (blockIdx.x - tile_pfx[t]) * SC_TILE + threadIdx.x;
    const float* Nk = N + cell0;
    float mx = Nk[0];
    for (uint64_t j = threadIdx.x; j < n_cells; j += SC_TILE) mx = sd_maxf(mx, Nk[j]);
    const float nmax = block_max(mx, red);
    if (c < n_cells) boundary[cell0 + c] = sc_is_boundary(Nk, n_cells, c, G, min_strength, nmax) ? 1 : 0;
}

void launch_section_energy(const float* E, const uint64_t* row0, const uint64_t* cell_pfx, int n_tracks, uint64_t n_cells,
                           uint64_t Cs, uint64_t hop, float* g, hipStream_t st) {
    if (n_tracks <= 0 || n_cells == 0) return;
    hipLaunchKernelGGL(k_section_energy, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, st, E, row0, cell_pfx,
                       n_tracks, n_cells, Cs, hop, g);
}

void launch_section_chroma(const float* chroma_s, const uint64_t* frame_pfx, const uint64_t* cell_pfx, int n_tracks,
                           uint64_t n_cells, uint64_t Cs, uint64_t khop, float* m, hipStream_t st) {
    if (n_tracks <= 0 || n_cells == 0) return;
    hipLaunchKernelGGL(k_section_chroma, dim3((unsigned)((n_cells + SC_CH_CELLS - 1) / SC_CH_CELLS)),
                       dim3(SC_CH_CELLS * 12), 0, st, chroma_s, frame_pfx, cell_pfx, n_tracks, n_cells, Cs, khop, m);
}

void launch_section_novelty(const float* m, const float* g, const uint64_t* cell_pfx, const uint64_t* tile_pfx,
                            int n_tracks, uint64_t n_tiles, int K, float w, uint64_t G, float min_strength, float* N,
                            uint8_t* boundary, hipStream_t st) {
    if (n_tracks <= 0 || n_tiles == 0) return;
    hipLaunchKernelGGL(k_section_novelty, dim3((unsigned)n_tiles), dim3(SC_NT), 0, st, m, g, cell_pfx, tile_pfx, n_tracks,
                       K, w, N);
    hipLaunchKernelGGL(k_section_pick, dim3((unsigned)n_tiles), dim3(SC_TILE), 0, st, N, cell_pfx, tile_pfx, n_tracks, G,
                       min_strength, boundary);
}

}  // namespace sdsp
