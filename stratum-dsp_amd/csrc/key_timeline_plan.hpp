// key_timeline_plan.hpp — the segment plan of the key timeline (include/stratum_hip.h,
// sdsp_key_timeline; reference src/features/key/key_changes.rs:70-160): request validation, the
// segment length L and hop H in key frames, the segment count, a segment's first frame and
// timestamp, and the host-side primary key and key changes over the per-segment results.
//
// Pure functions of integers and the request's floats, host and device.  No HIP: the library and
// the host harness tests/cpp/key_timeline_plan_test.cpp compile this header.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KT_HD __host__ __device__ inline
#else
#define KT_HD inline
#endif

namespace sdsp {

// frames per second of the key STFT, as key_changes.rs:92 takes it
inline float kt_fps(uint32_t sample_rate, uint32_t khop) { return (float)sample_rate / (float)khop; }

// (x - x is 0 for a finite x and NaN for an infinity or a NaN)
inline bool kt_finite(float x) { return x - x == 0.0f; }

// Why a request cannot run (NULL: it can), and its L and H.  Exactly one form: seconds
// (segment_seconds / overlap_seconds, f32 products with fps truncated, key_changes.rs:92-95) or
// frames (segment_frames / hop_frames).  A form counts as given when either of its fields is not 0.
inline const char* key_timeline_plan(float segment_seconds, float overlap_seconds, uint32_t segment_frames,
                                     uint32_t hop_frames, float min_change_confidence, uint32_t sample_rate,
                                     uint32_t khop, uint32_t* L_out, uint32_t* H_out) {
    *L_out = *H_out = 0;
    const bool sec = !(segment_seconds == 0.0f) || !(overlap_seconds == 0.0f);
    const bool frm = segment_frames != 0 || hop_frames != 0;
    if (!sec && !frm) return "Invalid input: key timeline request sets neither segment_seconds nor segment_frames";
    if (sec && frm) return "Invalid input: key timeline request sets both the seconds form and the frames form";
    if (sec && (!kt_finite(segment_seconds) || !kt_finite(overlap_seconds)))
        return "Invalid input: key timeline seconds are not finite";
    if (sec && (segment_seconds < 0.0f || overlap_seconds < 0.0f)) return "Invalid input: key timeline seconds are negative";
    if (min_change_confidence != min_change_confidence)
        return "Invalid input: key timeline min_change_confidence is NaN";
    uint64_t L, O, H;
    if (sec) {
        if (khop == 0) return "Invalid input: key timeline segment is empty (L == 0)";
        const float fps = kt_fps(sample_rate, khop);
        const float pl = segment_seconds * fps, po = overlap_seconds * fps;
        // (the products are >= 0 and not NaN here; one at or past 2^31 is refused below)
        L = pl < 4294967296.0f ? (uint64_t)pl : (uint64_t)1 << 32;
        O = po < 4294967296.0f ? (uint64_t)po : (uint64_t)1 << 32;
        if (L == 0) return "Invalid input: key timeline segment is empty (L == 0)";
        if (O >= L) return "Invalid input: key timeline overlap is not shorter than the segment (O >= L)";
        H = L - O;
    } else {
        L = segment_frames;
        H = hop_frames;
        if (L == 0) return "Invalid input: key timeline segment is empty (L == 0)";
        if (H == 0) return "Invalid input: key timeline hop is empty (H == 0)";
    }
    if (L >= ((uint64_t)1 << 31) || H >= ((uint64_t)1 << 31))
        return "Invalid input: key timeline segment or hop of 2^31 frames or more";
    *L_out = (uint32_t)L;
    *H_out = (uint32_t)H;
    return nullptr;
}

// S: the segments of F chroma rows
KT_HD uint64_t kt_segments(uint64_t F, uint64_t L, uint64_t H) {
    if (L == 0 || H == 0 || F < L) return 0;
    return (F - L) / H + 1;
}

// segment s covers frames [kt_start(s, H), kt_start(s, H) + L)
KT_HD uint64_t kt_start(uint64_t s, uint64_t H) { return s * H; }

inline float kt_timestamp(uint64_t s, uint64_t H, float fps) { return (float)kt_start(s, H) / fps; }

// The primary key over S segments: the key with the most segments, ties to the key whose first
// segment is earliest; its confidence is the f32 sum of its segments' confidences in segment
// order over (f32)count.  S == 0: key -1, confidence 0, count 0.
inline void kt_primary(const int32_t* key, const float* conf, uint64_t S, int32_t* pkey, float* pconf, uint64_t* pcount) {
    uint64_t count[24] = {}, first[24] = {};
    float sum[24] = {};
    for (uint64_t s = 0; s < S; s++) {
        const int k = key[s];
        if (k < 0 || k >= 24) continue;
        if (count[k] == 0) first[k] = s;
        count[k]++;
        sum[k] += conf[s];
    }
    int best = -1;
    for (int k = 0; k < 24; k++) {
        if (count[k] == 0) continue;
        if (best < 0 || count[k] > count[best] || (count[k] == count[best] && first[k] < first[best])) best = k;
    }
    *pkey = best;
    *pcount = best < 0 ? 0 : count[best];
    *pconf = best < 0 ? 0.0f : sum[best] / (float)count[best];
}

// Whether the boundary before segment i (i >= 1) is a reported change, and its confidence: the
// keys differ and (conf[i-1] + conf[i]) / 2 > min_change_confidence (strict; key_changes.rs:132).
inline bool kt_change(const int32_t* key, const float* conf, uint64_t i, float min_change_confidence, float* cconf) {
    *cconf = (conf[i - 1] + conf[i]) / 2.0f;
    return key[i] != key[i - 1] && *cconf > min_change_confidence;
}

}  // namespace sdsp
