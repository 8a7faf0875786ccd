// overview_plan.hpp — the column plan of the per-track overview envelope (include/stratum_hip.h,
// sdsp_overview): request validation, frame and column counts, each column's first frame and
// sample range, the band bins.
//
// Pure functions of integers and the request's two floats, host and device (the kernels compute a
// column's frames with ov_f0 instead of reading a host-built list, which at one frame per column
// would be as long as the spectrogram has rows).  No HIP: the library and the host harness
// tests/cpp/overview_plan_test.cpp compile this header.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OV_HD __host__ __device__ inline
#else
#define OV_HD inline
#endif

namespace sdsp {

// Why a request cannot run (NULL: it can).  Exactly one of the two counts is non-zero; the band
// edges are finite, non-negative and ordered.
inline const char* overview_request_error(uint32_t columns, uint32_t frames_per_column, float low_max_hz,
                                          float mid_max_hz) {
    if (columns == 0 && frames_per_column == 0)
        return "Invalid input: overview request sets neither columns nor frames_per_column";
    if (columns != 0 && frames_per_column != 0)
        return "Invalid input: overview request sets both columns and frames_per_column";
    // (x - x is 0 for a finite x and NaN for an infinity or a NaN)
    if (!(low_max_hz - low_max_hz == 0.0f) || !(mid_max_hz - mid_max_hz == 0.0f))
        return "Invalid input: overview band edge is not finite";
    if (low_max_hz < 0.0f || mid_max_hz < 0.0f) return "Invalid input: overview band edge is negative";
    if (low_max_hz > mid_max_hz) return "Invalid input: overview band edges out of order (low_max_hz > mid_max_hz)";
    return nullptr;
}

// F: the STFT frames of n samples (the base tempo pass's rows)
OV_HD uint64_t ov_frames(uint64_t n, uint64_t frame_size, uint64_t hop) {
    if (hop == 0 || n < frame_size) return 0;
    return (n - frame_size) / hop + 1;
}

// C: columns form min(columns, F), frames form ceil(F / frames_per_column)
OV_HD uint64_t ov_columns(uint64_t F, uint32_t columns, uint32_t frames_per_column) {
    if (columns) return F < columns ? F : (uint64_t)columns;
    if (!frames_per_column) return 0;
    return F / frames_per_column + (F % frames_per_column != 0);
}

// f0(c), c in [0, C]: the column's first frame; f0(C) = F.  c * F < F^2 stays far inside u64 for
// every F a device buffer can hold.
OV_HD uint64_t ov_f0(uint64_t c, uint64_t F, uint64_t C, uint32_t columns, uint32_t frames_per_column) {
    if (c >= C) return F;
    if (columns) return c * F / C;
    const uint64_t f = c * (uint64_t)frames_per_column;
    return f < F ? f : F;
}

// The longest column of the track, in frames (the kernels size a column's pieces by it).
OV_HD uint64_t ov_max_column_frames(uint64_t F, uint64_t C, uint32_t columns, uint32_t frames_per_column) {
    if (C == 0) return 0;
    if (columns) return F / C + (F % C != 0);
    return F < frames_per_column ? F : (uint64_t)frames_per_column;
}

// Pieces a column of the track is cut into for the kernels: 1 unless its longest column has more
// than `piece` frames.
OV_HD uint64_t ov_pieces(uint64_t F, uint64_t C, uint32_t columns, uint32_t frames_per_column, uint32_t piece) {
    const uint64_t m = ov_max_column_frames(F, C, columns, frames_per_column);
    return m > piece ? (m + piece - 1) / piece : 1;
}

// Column c's samples [*s0, *s1) of the trimmed signal: from its first frame's first sample to the
// next column's; the last column takes the samples after the last hop as well.
OV_HD void ov_sample_range(uint64_t c, uint64_t F, uint64_t C, uint32_t columns, uint32_t frames_per_column,
                           uint64_t hop, uint64_t n, uint64_t* s0, uint64_t* s1) {
    *s0 = ov_f0(c, F, C, columns, frames_per_column) * hop;
    *s1 = c + 1 < C ? ov_f0(c + 1, F, C, columns, frames_per_column) * hop : n;
}

// Band edges in bins: low [0, b1), mid [b1, b2), high [b2, B), B = frame_size / 2 + 1.
inline uint32_t ov_edge_bin(float hz, uint64_t frame_size, uint32_t sample_rate, uint32_t B) {
    if (sample_rate == 0) return B;
    const double v = (double)hz * (double)frame_size / (double)sample_rate;
    if (!(v < (double)B)) return B;  // also a NaN
    return v <= 0.0 ? 0u : (uint32_t)v;  // truncation = floor for v >= 0
}
inline void ov_band_bins(float low_max_hz, float mid_max_hz, uint64_t frame_size, uint32_t sample_rate, uint32_t* b1,
                         uint32_t* b2) {
    const uint32_t B = (uint32_t)(frame_size / 2 + 1);
    *b1 = ov_edge_bin(low_max_hz, frame_size, sample_rate, B);
    const uint32_t m = ov_edge_bin(mid_max_hz, frame_size, sample_rate, B);
    *b2 = m < *b1 ? *b1 : m;
}

}  // namespace sdsp
