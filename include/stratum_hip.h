/*
 * stratum_hip.h — C ABI of the MI355X-native analyze_audio() engine (libstratum_hip.so).
 *
 * This is the drop-in boundary for the reference crate's public API
 * (HLLMR/stratum-dsp, /root/reference):
 *
 *   pub fn analyze_audio(samples: &[f32], sample_rate: u32, config: AnalysisConfig)
 *       -> Result<AnalysisResult, AnalysisError>                      src/lib.rs:86-90
 *   impl Default for AnalysisConfig                                    src/config.rs:594-744
 *   pub struct AnalysisResult / AnalysisMetadata / BeatGrid / Key      src/analysis/result.rs:7-263
 *   pub enum AnalysisError (+ Display)                                 src/error.rs:7-34
 *
 * The Rust side binds these with `extern "C"` declarations (INTEGRATION.md shows the shim);
 * every struct here is `#[repr(C)]`-compatible: fixed-width scalars, pointer + length for
 * Vec fields, int32 for enums, int8 tri-states for Option<bool>.
 *
 * Ownership mirrors the reference: samples are borrowed (the library copies what it
 * needs, src/lib.rs:113), the config is read-only, results are owned by the library
 * until sdsp_result_free() is called.
 *
 * Threading: every entry point is reentrant.  Concurrent callers are serialised per
 * device inside the library (one HIP stream + workspace per device).
 */
#ifndef STRATUM_HIP_H
#define STRATUM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDSP_ABI_VERSION 1

/* AnalysisError variants, src/error.rs:7-22 (0 = Ok) */
enum sdsp_status {
    SDSP_OK = 0,
    SDSP_ERR_INVALID_INPUT = 1,    /* "Invalid input: {}"    */
    SDSP_ERR_DECODING = 2,         /* "Decoding error: {}"   */
    SDSP_ERR_PROCESSING = 3,       /* "Processing error: {}" */
    SDSP_ERR_NOT_IMPLEMENTED = 4,  /* "Not implemented: {}"  */
    SDSP_ERR_NUMERICAL = 5         /* "Numerical error: {}"  */
};

/* NormalizationMethod, src/preprocessing/normalization.rs:30-37 */
enum sdsp_normalization { SDSP_NORM_PEAK = 0, SDSP_NORM_RMS = 1, SDSP_NORM_LOUDNESS = 2 };
/* TemplateSet, src/features/key/templates.rs:17-22 */
enum sdsp_template_set { SDSP_TEMPLATES_KRUMHANSL_KESSLER = 0, SDSP_TEMPLATES_TEMPERLEY = 1 };

/*
 * AnalysisConfig, src/config.rs:8-592 — every pub field, same name, same meaning.
 * bool -> uint8_t, usize -> uint64_t, Option<T> -> has_x flag + value, Vec<T> -> ptr + len.
 */
typedef struct sdsp_config {
    float min_amplitude_db;
    int32_t normalization; /* enum sdsp_normalization */
    uint8_t enable_normalization;
    uint8_t enable_silence_trimming;
    uint8_t enable_onset_consensus;
    float onset_threshold_percentile;
    uint32_t onset_consensus_tolerance_ms;
    float onset_consensus_weights[4];
    uint8_t enable_hpss_onsets;
    uint64_t hpss_margin;
    uint8_t force_legacy_bpm;
    uint8_t enable_bpm_fusion;
    uint8_t enable_legacy_bpm_guardrails;
    uint8_t enable_tempogram_multi_resolution;
    uint64_t tempogram_multi_res_top_k;
    float tempogram_multi_res_w512;
    float tempogram_multi_res_w256;
    float tempogram_multi_res_w1024;
    float tempogram_multi_res_structural_discount;
    float tempogram_multi_res_double_time_512_factor;
    float tempogram_multi_res_margin_threshold;
    uint8_t tempogram_multi_res_use_human_prior;
    uint8_t enable_tempogram_percussive_fallback;
    uint8_t enable_tempogram_band_fusion;
    float tempogram_band_low_max_hz;
    float tempogram_band_mid_max_hz;
    float tempogram_band_high_max_hz;
    float tempogram_band_w_full;
    float tempogram_band_w_low;
    float tempogram_band_w_mid;
    float tempogram_band_w_high;
    uint8_t tempogram_band_seed_only;
    float tempogram_band_support_threshold;
    float tempogram_band_consensus_bonus;
    float tempogram_novelty_w_spectral;
    float tempogram_novelty_w_energy;
    float tempogram_novelty_w_hfc;
    uint64_t tempogram_novelty_local_mean_window;
    uint64_t tempogram_novelty_smooth_window;
    uint8_t has_debug_track_id;
    uint32_t debug_track_id;
    uint8_t has_debug_gt_bpm;
    float debug_gt_bpm;
    uint64_t debug_top_n;
    uint8_t enable_tempogram_mel_novelty;
    uint64_t tempogram_mel_n_mels;
    float tempogram_mel_fmin_hz;
    float tempogram_mel_fmax_hz;
    uint64_t tempogram_mel_max_filter_bins;
    float tempogram_mel_weight;
    uint64_t tempogram_superflux_max_filter_bins;
    uint8_t emit_tempogram_candidates;
    uint64_t tempogram_candidates_top_n;
    float legacy_bpm_preferred_min;
    float legacy_bpm_preferred_max;
    float legacy_bpm_soft_min;
    float legacy_bpm_soft_max;
    float legacy_bpm_conf_mul_preferred;
    float legacy_bpm_conf_mul_soft;
    float legacy_bpm_conf_mul_extreme;
    float min_bpm;
    float max_bpm;
    float bpm_resolution;
    uint64_t frame_size;
    uint64_t hop_size;
    float center_frequency;
    uint8_t soft_chroma_mapping;
    float soft_mapping_sigma;
    float chroma_sharpening_power;
    uint8_t enable_key_spectrogram_time_smoothing;
    uint64_t key_spectrogram_smooth_margin;
    uint8_t enable_key_frame_weighting;
    float key_min_tonalness;
    float key_tonalness_power;
    float key_energy_power;
    uint8_t enable_key_harmonic_mask;
    float key_harmonic_mask_power;
    uint8_t enable_key_hpss_harmonic;
    uint64_t key_hpss_frame_step;
    uint64_t key_hpss_time_margin;
    uint64_t key_hpss_freq_margin;
    float key_hpss_mask_power;
    uint8_t enable_key_stft_override;
    uint64_t key_stft_frame_size;
    uint64_t key_stft_hop_size;
    uint8_t enable_key_log_frequency;
    uint8_t enable_key_beat_synchronous;
    uint8_t enable_key_multi_scale;
    int32_t key_template_set; /* enum sdsp_template_set */
    uint8_t enable_key_ensemble;
    float key_ensemble_kk_weight;
    float key_ensemble_temperley_weight;
    uint8_t enable_key_median;
    uint64_t key_median_segment_length_frames;
    uint64_t key_median_segment_hop_frames;
    uint64_t key_median_min_segments;
    const uint64_t* key_multi_scale_lengths; /* Vec<usize> */
    uint64_t key_multi_scale_lengths_len;
    uint64_t key_multi_scale_hop;
    float key_multi_scale_min_clarity;
    const float* key_multi_scale_weights; /* Vec<f32> */
    uint64_t key_multi_scale_weights_len;
    uint8_t enable_key_tuning_compensation;
    float key_tuning_max_abs_semitones;
    uint64_t key_tuning_frame_step;
    float key_tuning_peak_rel_threshold;
    uint8_t enable_key_edge_trim;
    float key_edge_trim_fraction;
    uint8_t enable_key_segment_voting;
    uint64_t key_segment_len_frames;
    uint64_t key_segment_hop_frames;
    float key_segment_min_clarity;
    uint8_t enable_key_mode_heuristic;
    float key_mode_third_ratio_margin;
    float key_mode_flip_min_score_ratio;
    uint8_t enable_key_hpcp;
    uint64_t key_hpcp_peaks_per_frame;
    uint64_t key_hpcp_num_harmonics;
    float key_hpcp_harmonic_decay;
    float key_hpcp_mag_power;
    uint8_t enable_key_hpcp_whitening;
    uint64_t key_hpcp_whitening_smooth_bins;
    uint8_t enable_key_hpcp_bass_blend;
    float key_hpcp_bass_fmin_hz;
    float key_hpcp_bass_fmax_hz;
    float key_hpcp_bass_weight;
    uint8_t enable_key_minor_harmonic_bonus;
    float key_minor_leading_tone_bonus_weight;
    uint8_t enable_ml_refinement; /* #[cfg(feature = "ml")] */
} sdsp_config;

/* AnalysisFlag, src/analysis/result.rs:157-166 — bit i set <=> flags contains variant i */
enum sdsp_flag {
    SDSP_FLAG_MULTIMODAL_BPM = 1u << 0,
    SDSP_FLAG_WEAK_TONALITY = 1u << 1,
    SDSP_FLAG_TEMPO_VARIATION = 1u << 2,
    SDSP_FLAG_ONSET_DETECTION_AMBIGUOUS = 1u << 3
};

/* TempoCandidateDebug, src/analysis/result.rs:168-181 */
typedef struct sdsp_tempo_candidate {
    float bpm;
    float score;
    float fft_norm;
    float autocorr_norm;
    uint8_t selected;
} sdsp_tempo_candidate;

/* Key, src/analysis/result.rs:7-12 */
enum sdsp_key_mode { SDSP_KEY_MAJOR = 0, SDSP_KEY_MINOR = 1 };

/* AnalysisResult + AnalysisMetadata + BeatGrid, src/analysis/result.rs:144-263 */
typedef struct sdsp_result {
    float bpm;
    float bpm_confidence;
    int32_t key_mode;   /* enum sdsp_key_mode */
    uint32_t key_tonic; /* 0 = C .. 11 = B */
    float key_confidence;
    float key_clarity;
    /* beat_grid (library-owned arrays) */
    float* beats;
    uint64_t n_beats;
    float* downbeats;
    uint64_t n_downbeats;
    float* bars;
    uint64_t n_bars;
    float grid_stability;
    /* metadata */
    float duration_seconds;
    uint32_t sample_rate;
    float processing_time_ms;
    char algorithm_version[16];
    float onset_method_consensus;
    uint32_t methods_used; /* always energy_flux|chroma_extraction|key_detection (lib.rs:1606-1610) */
    uint32_t flags;        /* enum sdsp_flag bitmask, in reference push order */
    char** warnings;       /* confidence_warnings, in order */
    uint64_t n_warnings;
    sdsp_tempo_candidate* tempogram_candidates; /* valid iff has_tempogram_candidates */
    uint64_t n_tempogram_candidates;
    int8_t has_tempogram_candidates;
    /* Option<bool>: -1 = None, 0 = Some(false), 1 = Some(true) */
    int8_t tempogram_multi_res_triggered;
    int8_t tempogram_multi_res_used;
    int8_t tempogram_percussive_triggered;
    int8_t tempogram_percussive_used;
    /* per-track status for the batch entry points (enum sdsp_status + Display text) */
    int32_t status;
    char error_message[256];
} sdsp_result;

/* AnalysisConfig::default(), src/config.rs:594-744 */
void sdsp_config_default(sdsp_config* cfg);

/*
 * analyze_audio(samples, sample_rate, config), src/lib.rs:86.
 * Returns enum sdsp_status; on error the Display text ("Invalid input: Empty audio samples")
 * is written to err (NUL-terminated, truncated to errlen) and *out is left zeroed.
 */
int32_t sdsp_analyze_audio(const float* samples, uint64_t n_samples, uint32_t sample_rate,
                           const sdsp_config* cfg, sdsp_result* out, char* err, uint64_t errlen);

/*
 * Batch form (new): N independent analyze_audio calls, sharded over the devices in
 * device_mask (bit d = HIP device d; 0 = device 0).  outs[i].status carries each track's
 * Ok/Err.  Returns SDSP_OK unless the batch itself could not run.
 */
int32_t sdsp_analyze_batch(const float* const* tracks, const uint64_t* lens, uint64_t n_tracks,
                           uint32_t sample_rate, const sdsp_config* cfg, uint32_t device_mask,
                           sdsp_result* outs);

/*
 * Device-resident batch: tracks already in HBM on `device` (concatenated, track i starts at
 * d_samples + offsets[i] and has lens[i] samples; host arrays).  `stream` is a hipStream_t
 * (NULL = the library's own stream).  Used by the throughput benchmark.
 */
int32_t sdsp_analyze_batch_device(const float* d_samples, const uint64_t* offsets,
                                  const uint64_t* lens, uint64_t n_tracks, uint32_t sample_rate,
                                  const sdsp_config* cfg, int32_t device, void* stream,
                                  sdsp_result* outs);

/*
 * Stage selection for the device-resident batch (new; the reference has no such switch).
 * SDSP_STAGES_BPM_ONLY runs the tempo path alone -- src/lib.rs:86-910, SURVEY.md rows a1-a19:
 * normalisation, trim, onsets, tempogram, multi-resolution escalation, BPM choice.  bpm,
 * bpm_confidence, duration and the tempogram_* flags equal a full run's; the key fields keep their
 * defaults (C major, 0) and the beat grid is empty.  BASELINE config 5 is quoted in this mode.
 */
enum sdsp_stages { SDSP_STAGES_FULL = 0, SDSP_STAGES_BPM_ONLY = 1 };
int32_t sdsp_analyze_batch_device_ex(const float* d_samples, const uint64_t* offsets,
                                     const uint64_t* lens, uint64_t n_tracks, uint32_t sample_rate,
                                     const sdsp_config* cfg, int32_t device, void* stream,
                                     int32_t stages, sdsp_result* outs);

/* Frees the arrays owned by one result (beats, downbeats, bars, warnings, candidates). */
void sdsp_result_free(sdsp_result* r);

/*
 * Overview envelopes (new; the reference has none): per track a compact amplitude and band summary
 * in C columns, computed inside the analysis call from what it already holds on the device (the
 * gain and trim bounds, the samples, the base tempo pass's magnitude spectrogram), so a caller whose
 * audio exists only in HBM (sdsp_decode_audio_batch_device) neither downloads nor decodes it again.
 *
 * Per track, with n the trimmed length, first_sample the trim start in the caller's track,
 *   x[i] = raw[first_sample + i] * gain   (one f32 multiply: the normalised, trimmed signal as the
 *                                          reference stores it, whatever the normalisation method,
 *                                          and with normalisation or trimming switched off)
 *   frame_size, hop = the configuration's frame_size and hop_size, B = frame_size / 2 + 1
 *   F = n < frame_size ? 0 : (n - frame_size) / hop + 1
 *   M[t][k] = the magnitudes of the hop_size STFT of x (the base tempo pass's rows)
 * the request selects the columns by exactly one of
 *   columns > 0            C = min(columns, F),               f0(c) = floor(c * F / C)
 *   frames_per_column > 0  C = ceil(F / frames_per_column),   f0(c) = min(c * frames_per_column, F)
 * (u64 arithmetic; f0(C) = F), the bands by
 *   b1 = min(B, floor((double)low_max_hz * frame_size / sample_rate))
 *   b2 = min(B, max(b1, floor((double)mid_max_hz * frame_size / sample_rate)))
 *   low = bins [0, b1), mid = [b1, b2), high = [b2, B)
 * and column c holds
 *   smin[c], smax[c]   the minimum and maximum of x[i] over i in [f0(c) * hop, s1), with
 *                      s1 = f0(c + 1) * hop for c + 1 < C and s1 = n for the last column (which
 *                      takes the samples after the last hop); where both zeros occur, -0 < +0
 *   low[c], mid[c], high[c]   the maximum of M[t][k] over t in [f0(c), f0(c + 1)) and k in the
 *                      band; 0.0f for an empty band
 * Every value is a minimum or maximum, so it is exact: equal, bit for bit, to the same reduction
 * over the reference's normalised signal and spectrogram.  Non-finite input samples are out of
 * scope: the overview of a track that holds a NaN or an infinity is unspecified.
 *
 * F = 0 (a track shorter than one frame) gives zero columns and leaves the status alone.  A track
 * whose analysis status is not SDSP_OK gets that status, zero columns, and zero n_frames,
 * first_sample and n_samples.  frame_size, hop_size and band_bins are filled for every track.
 */
typedef struct sdsp_overview_request {
    uint32_t columns;
    uint32_t frames_per_column;
    float low_max_hz, mid_max_hz;
} sdsp_overview_request;

typedef struct sdsp_overview {
    uint64_t n_columns, n_frames;     /* C, F */
    uint64_t first_sample, n_samples; /* the trim start in the caller's track, n */
    uint32_t frame_size, hop_size;
    uint32_t band_bins[2];            /* b1, b2 */
    float *smin, *smax, *low, *mid, *high; /* library-owned, n_columns each (NULL for none) */
    int32_t status;                   /* the track's sdsp_status */
} sdsp_overview;

/*
 * sdsp_analyze_batch_device_ex, and for each track its overview in overviews[i] (n_tracks entries,
 * freed one by one with sdsp_overview_free).  With SDSP_STAGES_FULL and SDSP_STAGES_BPM_ONLY alike:
 * both run the base tempo pass.  req == NULL is sdsp_analyze_batch_device_ex itself (the same
 * launches, the same results; overviews is not touched and may be NULL).  A request with both
 * counts zero or both non-zero, or with a band edge that is not finite, is negative, or
 * low_max_hz > mid_max_hz, fails the call with SDSP_ERR_INVALID_INPUT before any device is touched:
 * every outs[i] carries the status and the reason, every overview is zeroed.
 */
int32_t sdsp_analyze_batch_device_overview(const float* d_samples, const uint64_t* offsets,
                                           const uint64_t* lens, uint64_t n_tracks, uint32_t sample_rate,
                                           const sdsp_config* cfg, int32_t device, void* stream,
                                           int32_t stages, sdsp_result* outs,
                                           const sdsp_overview_request* req, sdsp_overview* overviews);
/* Frees the arrays owned by one overview (never free() them one by one: they share one allocation). */
void sdsp_overview_free(sdsp_overview* o);

/*
 * Key timeline: per-segment keys, a primary key and the key changes of every track, the reference's
 * detect_key_changes (src/features/key/key_changes.rs:70) computed inside the analysis call from the
 * smoothed chroma rows it already holds on the device.
 *
 * Scope: a track whose key path runs (SDSP_STAGES_FULL, trimmed length n >= frame_size and n >= the
 * key STFT's frame size).  With kfs, khop the key STFT's frame and hop (the override's
 * key_stft_frame_size / key_stft_hop_size, else frame_size / hop_size):
 *   F = (n - kfs) / khop + 1 key frames
 *   C[f][0..12), f in [0, F): the chroma rows the key decision reads: after sharpening (if
 *       configured), after the 5-frame median smoothing (when F > 5), before the edge trim and
 *       without frame weights (enable_key_edge_trim and the frame weighting do not reach the timeline)
 *   fps = (f32)sample_rate / (f32)khop
 * The request gives exactly one of two forms (a form is given when either of its fields is not 0):
 *   seconds  L = (u64)(segment_seconds * fps), O = (u64)(overlap_seconds * fps), H = L - O
 *            (f32 products, truncated: key_changes.rs:92-95)
 *   frames   L = segment_frames, H = hop_frames
 *   S = F < L ? 0 : (F - L) / H + 1 segments; segment s covers frames [s H, s H + L),
 *   start_frame = s H, timestamp = (f32)(s H) / fps seconds after first_sample.
 * Per segment, detect_key (key/detector.rs:68-313) with the Krumhansl-Kessler templates T:
 *   raw[k] = the f32 sum from 0, over the segment's frames in ascending order, of the f32 dot
 *            product from 0 over i ascending of C[f][i] * T[k][i]   (detector.rs:984-1001)
 *   then per-mode normalisation when both maxima > 1e-9, the last maximum of each mode, the
 *   0.20 / 0.10 circle-of-fifths bonus, and a stable descending sort (detector.rs:135-293)
 *   key         the first key of the sorted table (mode * 12 + tonic: 0-11 major, 12-23 minor)
 *   confidence  sorted[0] > 0 ? clamp((sorted[0] - sorted[1]) / sorted[0], 0, 1) : 0
 *   clarity     compute_key_clarity over the sorted table (key_clarity.rs:51-93)
 *   top_keys, top_scores   the first three entries of the sorted table
 * Primary key: the key with the most segments; among keys with equally many, the one whose first
 * segment is earliest (the reference takes max_by_key over a HashMap, so it returns any of them,
 * differing from run to run; this is one of its outcomes).  primary_confidence is the f32 sum of
 * that key's segment confidences in segment order over (f32)primary_count.  S = 0: primary_key -1,
 * primary_confidence 0, primary_count 0.
 * Changes: for i in [1, S) with key[i] != key[i-1]: confidence = (confidence[i-1] + confidence[i]) / 2.0f,
 * timestamp = timestamp[i], segment = i; reported iff confidence > min_change_confidence.  The
 * reference's fixed threshold is 0.2; a negative value reports every change.
 *
 * What these numbers are, as measured on tonal and noise tracks alike:
 *   - The templates are always Krumhansl-Kessler (KeyTemplates::new()), whatever key_template_set
 *     and enable_key_ensemble say.  Following the configured set is left for later.
 *   - Whenever both modes score (> 1e-9), both within-mode maxima normalise to exactly 1.0 and each
 *     takes its own full bonus, so the top major and the top minor key tie at exactly 1.2: the
 *     stable sort puts the major key first, and confidence is exactly 0.  The reference's threshold
 *     0.2 therefore reports no change on such input; min_change_confidence < 0 is the setting that
 *     reports where the key moves.
 *   - clarity is reported as the reference computes it; it does not separate tonal input from noise
 *     (about 0.65 on cadences, about 0.75 on white noise) and is not a tonality measure.
 * Non-finite input samples are out of scope.
 *
 * Per track: an analysis status other than SDSP_OK gives that status, zero segments and zero fields;
 * a track whose key path is skipped (too short) gives n_frames 0, zero segments, primary_key -1 and
 * leaves the status alone.  segment_frames (L), hop_frames (H), frame_size (kfs) and hop_size (khop)
 * are filled for every track.  first_sample is the trim start in the caller's track, as in
 * sdsp_overview: sample first_sample + start_frame * hop_size begins a segment.
 */
typedef struct sdsp_key_timeline_request {
    float segment_seconds, overlap_seconds; /* the seconds form */
    uint32_t segment_frames, hop_frames;    /* the frames form */
    float min_change_confidence;
} sdsp_key_timeline_request;

typedef struct sdsp_key_segment {
    uint64_t start_frame;
    float timestamp;
    int32_t key;
    float confidence, clarity;
    int32_t top_keys[3];
    float top_scores[3];
} sdsp_key_segment;

typedef struct sdsp_key_change {
    uint64_t segment; /* i: the change lies between segments i - 1 and i */
    float timestamp;
    int32_t from_key, to_key;
    float confidence;
} sdsp_key_change;

typedef struct sdsp_key_timeline {
    uint64_t n_segments, n_changes, n_frames; /* S, reported changes, F */
    uint64_t first_sample;
    uint32_t segment_frames, hop_frames; /* L, H */
    uint32_t frame_size, hop_size;       /* kfs, khop */
    int32_t primary_key;
    float primary_confidence;
    uint64_t primary_count;
    sdsp_key_segment* segments; /* library-owned, n_segments (NULL for none) */
    sdsp_key_change* changes;   /* library-owned, n_changes (NULL for none) */
    int32_t status;             /* the track's sdsp_status */
} sdsp_key_timeline;

/*
 * sdsp_analyze_batch_device_ex with both optional requests, so a caller who wants overviews and
 * key timelines pays for one analysis: ov_req / overviews as in sdsp_analyze_batch_device_overview,
 * kt_req / timelines (n_tracks entries, freed one by one with sdsp_key_timeline_free) as above.
 * Both requests NULL is sdsp_analyze_batch_device_ex itself (the same launches, the same results).
 * A request never changes an sdsp_result.  Checked before any device is touched, failing the whole
 * call (every outs[i] carries the status and the reason, every requested overview and timeline is
 * zeroed but for its status):
 *   SDSP_ERR_INVALID_INPUT    an overview request sdsp_analyze_batch_device_overview refuses; both
 *                             timeline forms given, or neither; seconds that are not finite or are
 *                             negative; a NaN min_change_confidence; L == 0, O >= L or H == 0; L or
 *                             H >= 2^31; a timeline request with SDSP_STAGES_BPM_ONLY (no key path);
 *                             a request without its output array
 *   SDSP_ERR_NOT_IMPLEMENTED  a timeline request with enable_key_beat_synchronous and not
 *                             enable_key_log_frequency (the chroma rows are beats, not frames)
 */
int32_t sdsp_analyze_batch_device_requests(const float* d_samples, const uint64_t* offsets,
                                           const uint64_t* lens, uint64_t n_tracks, uint32_t sample_rate,
                                           const sdsp_config* cfg, int32_t device, void* stream,
                                           int32_t stages, sdsp_result* outs,
                                           const sdsp_overview_request* ov_req, sdsp_overview* overviews,
                                           const sdsp_key_timeline_request* kt_req,
                                           sdsp_key_timeline* timelines);
/* Frees the arrays owned by one timeline (they share one allocation: never free() them one by one). */
void sdsp_key_timeline_free(sdsp_key_timeline* t);

/*
 * Levels: the loudness metadata of the reference's normalize() and the silence map of its
 * detect_and_trim(), both of which analyze_audio computes and drops
 * (src/preprocessing/normalization.rs:64-73, 262-547; src/preprocessing/silence.rs:102-279),
 * computed inside the analysis call from the samples on the device.
 *
 * method[m], for each method bit m of the request (bit m = NormalizationMethod m), is what
 *   normalize(copy of the caller's raw track, {method m, -14 LUFS, 1 dB}, sample_rate)
 * returns, whatever cfg.normalization and cfg.enable_normalization say.  With peak = max |x|,
 * target = 10^(-1/20), dB(v) = 20 log10(v), every sum the sequential f32 fold from 0 in sample order,
 * every log10 / pow include/sdsp_libm.h's, the K-weighting coefficients as the engine's own
 * normalisation computes them:
 *   Peak      peak <= 1e-10: peak_db = rms_db = -inf, gain_db = 0, gain = 1.  Else peak_db = dB(peak),
 *             gain_db = dB(target / peak) while the applied gain = min(target / peak, 1 / peak)
 *             (normalization.rs:291-295: the metadata is that of the unlimited gain), and rms_db is
 *             the RMS of the *normalised* samples, sqrt(sum (x * gain)^2 / n) (:303), -inf at or
 *             below 1e-10.
 *   RMS       rms = sqrt(sum x^2 / n) of the raw samples; rms <= 1e-10 as the quiet Peak case.  Else
 *             rms_db = dB(rms) (raw), peak_db = dB(peak), gain = 10^((-14 + 3 - 1) / 20) / rms, or
 *             1 / peak when peak * gain > 1; gain_db = dB(applied gain).
 *   Loudness  measured_lufs = -0.691 + 10 log10(mean of the 400-ms blocks' mean squares of the
 *             K-weighted signal that exceed 10^((-70 + 0.691) / 10)); gain = 10^((-14 - lufs) / 20), or
 *             target / peak when peak * gain > target (gain_db then dB(target / peak), else -14 - lufs);
 *             rms_db the RMS of the normalised samples (:443, :464).  With every block under the gate
 *             the reference falls back to normalize_peak: the Peak metadata, has_lufs 0.  This is the
 *             reference's measure: one shelving stage, no relative gate (BS.1770 has a second stage
 *             and a relative gate; the reference has neither).  The NumericalError branch of
 *             calculate_lufs cannot be reached: a gated mean exceeds the gate, about 1.17e-7, and the
 *             branch tests mean <= 1e-10.
 * A method the request does not ask for has measured 0 and zeroed fields.  -inf is reported as -inf;
 * measured_lufs is -inf wherever has_lufs is 0 (the reference's None).
 *
 * The silence map (SDSP_LEVELS_SILENCE_MAP) is detect_and_trim's second return value on the signal
 * raw * applied_gain, with the detector {cfg.min_amplitude_db, 500 ms, cfg.frame_size}: frames of
 * frame_size every frame_size / 2, silent when their RMS <= 10^(threshold_db / 20), runs of silent
 * frames as regions [start_sample, end_sample) in the caller's track, ascending.
 *   - the run starting at frame 0 is kept whatever its length; an interior run is kept from
 *     min_duration_frames = ceil((u64)(0.5f * sample_rate) / (frame_size / 2)) frames on;
 *   - a trailing run (ending with the last frame, end_sample = n) shorter than that is dropped: the
 *     reference's in-loop test `silence_end_frame == num_frames` can never be true, a run found in the
 *     loop ends at a frame index < num_frames;
 *   - duration_seconds = (f32)(end_sample - start_sample) / (f32)sample_rate.
 * The map is computed when requested even with enable_silence_trimming off (it is a pure function
 * of the signal; trim_start / trim_end are then 0 / n).
 *
 * Per track: every track with n > 0, sample_rate > 0 and a supported configuration has status
 * SDSP_OK, including one whose analysis fails with "entirely silent after trimming".  Any other track
 * carries the analysis status and zeroed fields.  If the configured normalisation itself fails,
 * method[m].status carries the error, applied_gain is 1 and the map is empty.  Non-finite samples
 * are out of scope.  True peak, loudness range and per-channel levels are not computed.
 */
enum sdsp_levels_what { /* bits of sdsp_levels_request.what */
    SDSP_LEVELS_PEAK = 1, SDSP_LEVELS_RMS = 2, SDSP_LEVELS_LOUDNESS = 4, /* bit m = NormalizationMethod m */
    SDSP_LEVELS_SILENCE_MAP = 8
};
typedef struct sdsp_levels_request { uint32_t what; } sdsp_levels_request;

typedef struct sdsp_loudness { /* LoudnessMetadata of one method, normalization.rs:64-73 */
    int32_t status;            /* SDSP_OK, or the error normalize() returns for this method */
    int8_t measured;           /* 1 iff the request asked for this method */
    int8_t has_lufs;           /* measured_lufs is Some */
    float measured_lufs, peak_db, rms_db, gain_db;
    float gain; /* the f32 the reference multiplies the samples by (1.0f where it applies none) */
} sdsp_loudness;

typedef struct sdsp_silence_region { uint64_t start_sample, end_sample; float duration_seconds; } sdsp_silence_region;

typedef struct sdsp_levels {
    sdsp_loudness method[3];       /* index = enum sdsp_normalization */
    float applied_gain;            /* what this analysis multiplied by (1.0f with normalisation off) */
    uint64_t n_samples;            /* the caller's track length */
    uint64_t trim_start, trim_end; /* the bounds the analysis used, in the caller's track */
    uint32_t frame_size;           /* the detector's: cfg.frame_size */
    float threshold_db;            /* ... and cfg.min_amplitude_db */
    uint64_t n_regions;
    sdsp_silence_region* regions;  /* library-owned, NULL for none */
    int32_t status;
} sdsp_levels;

/*
 * Tempo map: what the beat stage computes on the way to the beat list and drops, as the reference's
 * analyze_audio does: the consensus onsets, the tempo segments of detect_tempo_variations over the
 * whole-track HMM beats with what the Bayesian refinement did in each (beat_tracking/mod.rs:140-219,
 * tempo_variation.rs:95-227, bayesian.rs:104-178), and the time signature that chose the downbeats
 * (time_signature.rs:90-199).  Everything is a function of (onsets, nominal_bpm): with the onsets
 * returned a caller can recompute every field.  Times are seconds on the time axis of the result's
 * beats (0 = first_sample of the caller's track).
 *
 * Segments: exactly detect_tempo_variations(HMM beats, nominal_bpm); start_time, end_time, bpm and
 * confidence are the reference's f32 values.  With b the HMM beats (hmm_beats of them):
 *   - fewer than 4 beats: one segment [b first, b last], nominal_bpm, confidence 0.5, not variable;
 *     a span under 2 s, or no window that qualified: the same with confidence 0.8;
 *   - else windows of seg_dur = clamp(span / 4, 4, 8) s starting at cur, from cur = b first while
 *     cur < b last, where cur is the sequential f32 accumulation cur += seg_dur - seg_dur / 2 (not
 *     b first + s * step); a window ends at min(cur + seg_dur, b last);
 *   - a window with fewer than 3 beats in [start, end], or without a positive interval, emits nothing;
 *   - bpm = 60 / mean positive interval, cv = sd / mean (population variance, both folded in beat
 *     order), is_variable = cv > 0.15, confidence = max(1 - min(cv / 0.3, 1), 0).
 * Refinement (filled only when has_variation; else updated = 0 and the four fields are 0): a tracker
 * starts at nominal_bpm and walks the segments in order, its tempo carrying from one variable segment
 * to the next.  In a variable segment with onsets in [start_time, end_time] (n_onsets of them) it
 * scores the candidates max(t - 5, 60), +0.5, ... <= min(t + 5, 180) around its tempo t; updated_bpm
 * is the first candidate that reaches the maximum likelihood (t itself when none is positive),
 * updated_confidence = min(likelihood * penalty, 1) with penalty 1 / 0.8 / 0.5 for a change below 1 /
 * below 3 / otherwise, and n_beats the beat count of the HMM re-run over those onsets at updated_bpm
 * (0 if it failed).  A variable segment without onsets is skipped (updated 0, n_beats 0).  A constant
 * segment passes the HMM beats in [start_time, end_time] on: n_beats of them.  The refined list is the
 * concatenation, stably sorted: `refined` (it was not empty, and is what the result publishes)
 * implies sum of n_beats == the result's n_beats, and because the windows overlap by half, beats
 * of overlapping segments are in that list twice.
 *
 * Time signature: detect_time_signature(the published beats, nominal_bpm).  time_signature_scores are
 * the scores of 4/4, 3/4 and 6/8, 0.7 x the mean similarity of the positive intervals at lag 4, 3, 6
 * + 0.3 / (1 + cv); the LAST maximum wins and time_signature_confidence is its score clamped to
 * [0, 1].  With fewer than 8 beats or no positive interval nothing is scored: beats_per_bar 4,
 * confidence 0.5, time_signature_scored 0.  What these numbers are: a perfectly regular grid ties all
 * three scores and is therefore reported as 6 beats per bar; an exact click track comes out as 6, a
 * four-bar 120 BPM loop as 3.  The value explains which of the published beats became downbeats; it
 * is not a meter estimate.
 *
 * onsets: the consensus onset list the beat stage and the legacy estimator ran on, as sample
 * positions after first_sample, ascending.  SDSP_TEMPO_MAP_SEGMENTS asks for the segment list,
 * SDSP_TEMPO_MAP_ONSETS for the onset list (n_* = 0 and NULL when not asked for); the scalar fields
 * are always filled.
 *
 * Per track: an analysis status other than SDSP_OK gives that status and zeroed fields.  A track
 * without a grid (tempo <= 0 or above 300, fewer than 2 onsets, an HMM or tracker error) has has_grid 0,
 * no segments, zero counts, beats_per_bar 0, and still its nominal tempo and its onsets.
 */
enum sdsp_tempo_map_what { SDSP_TEMPO_MAP_SEGMENTS = 1, SDSP_TEMPO_MAP_ONSETS = 2 }; /* bits of sdsp_tempo_map_request.what */
typedef struct sdsp_tempo_map_request { uint32_t what; } sdsp_tempo_map_request;

typedef struct sdsp_tempo_segment { /* TempoSegment, tempo_variation.rs:56-71, and what mod.rs:167-208 did with it */
    float start_time, end_time;     /* seconds, on the time axis of the result's beats */
    float bpm, confidence;
    uint8_t is_variable;
    uint8_t updated;                /* the Bayesian tracker was updated with this segment's onsets */
    uint32_t n_onsets;              /* onsets in [start_time, end_time] handed to it (0 unless updated) */
    float updated_bpm, updated_confidence; /* update_with_onsets' return (0 unless updated) */
    uint32_t n_beats;               /* beats this segment put into the refined list (0 without variation) */
} sdsp_tempo_segment;

typedef struct sdsp_tempo_map {
    int32_t status;                 /* the track's sdsp_status */
    int8_t has_grid;                /* generate_beat_grid returned Ok: the result has beats */
    int8_t has_variation, refined;  /* has_tempo_variation(); the published beats are the refined list */
    int8_t time_signature_scored;   /* 0: fewer than 8 beats or no positive interval -> (4, 0.5), scores 0 */
    float nominal_bpm, nominal_confidence; /* what the beat stage ran with */
    uint32_t hmm_beats;             /* the whole-track HMM's beat count */
    uint32_t beats_per_bar;         /* 4, 3 or 6 */
    float time_signature_confidence;
    float time_signature_scores[3]; /* 4/4, 3/4, 6/8 */
    uint64_t first_sample;          /* trim start in the caller's track, as in sdsp_overview */
    uint64_t n_segments;
    sdsp_tempo_segment* segments;   /* library-owned, one allocation with onsets */
    uint64_t n_onsets;
    uint32_t* onsets;
} sdsp_tempo_map;

/*
 * Sections: structural boundaries of a track and the energy of each part, a self-distance novelty
 * (Foote's checkerboard) over short cells of the smoothed chroma rows and the base tempo pass's
 * frame energies, both resident during the analysis call.  The reference has no counterpart; this
 * definition is the contract.
 *
 * What the numbers are: a novelty of chroma change and energy change at cell resolution.  It is not
 * a phrase or bar estimate, and energy_weight is the caller's trade between the two kinds of change
 * (0: chroma alone).  Non-finite input samples are out of scope.
 *
 * Scope: a track whose key path runs (SDSP_STAGES_FULL, trimmed length n >= frame_size and n >= the
 * key STFT's frame size).  Inputs:
 *   kfs, khop  the key STFT's frame and hop; F = (n - kfs) / khop + 1 key frames with the rows
 *              C[f][0..12) exactly as sdsp_key_timeline defines them
 *   frame_size, hop_size  the base tempo pass; Fb = (n - frame_size) / hop_size + 1 frames with the
 *              energies E[f] = the f32 sum over bins ascending of mag * mag (novelty.rs:511-515)
 * Every sum below is f32, starts from 0 and runs in ascending index order; multiply and add are
 * separate operations; division is IEEE f32.
 * Cells: Cs = cell_samples, or (u64)(cell_seconds * (f32)sample_rate); exactly one of the two is
 *   given (a form is given when its field is not 0).  Cs >= max(khop, hop_size).
 *   n_cells = min(F * khop, Fb * hop_size) / Cs (integer division).  Cell c owns the key frames whose
 *   start f * khop lies in [c Cs, (c + 1) Cs), and likewise the base frames by f * hop_size: integer
 *   arithmetic only, and every cell owns at least one frame of each kind.
 * Cell features:
 *   m[c][i] = (sum over the cell's key frames of C[f][i]) / (f32)count
 *   g[c]    = (sum over the cell's base frames of E[f]) / (f32)count
 *   gmax = max over c of g[c];  e[c] = gmax > 0 ? g[c] / gmax : 0
 * Distance: D(a, b) = sum over i = 0..11 of (m[a][i] - m[b][i])^2, then + energy_weight * (e[a] - e[b])^2
 * Novelty, with K = kernel_cells (1 <= K <= 64), for c in [K, n_cells - K]:
 *   cross = sum over a = c-K..c-1 (outer), b = c..c+K-1 (inner) of D(a, b)
 *   wp    = sum over a = c-K..c-1, b = a+1..c-1 of D(a, b);  wf the same over [c, c + K)
 *   N[c]  = cross / (f32)(K K) - (K > 1 ? (wp + wf) / (f32)(K (K - 1)) : 0);  N[c] = 0 for every other c
 * Boundaries, with G = min_gap_cells and Nmax = max over c of N[c]: cell c is a boundary when
 *   N[c] > 0, N[c] >= min_strength * Nmax, N[c] > N[j] for every valid j in [c - G, c) and
 *   N[c] >= N[j] for every valid j in (c, c + G]: the first of two equal peaks wins.
 * Sections: the runs of cells between boundaries, n_boundaries + 1 of them covering [0, n_cells)
 *   (none when n_cells is 0).  start_time = (f32)(start_cell * Cs) / (f32)sample_rate on the time axis of
 *   the result's beats (0 = first_sample), end_time alike; strength = N at start_cell (0 for the
 *   first section); mean_energy = (sum of g[c] over its cells) / (f32)count; relative_energy =
 *   mean_energy / the largest section mean_energy (0 when that is 0).  downbeat is the index of the
 *   result's downbeat nearest to start_time (|downbeats[j] - start_time| in f32, the first on a tie)
 *   if that distance is <= snap_seconds, and snapped_time that downbeat; otherwise downbeat = -1 and
 *   snapped_time = start_time.
 * SDSP_SECTIONS_LIST asks for the sections, SDSP_SECTIONS_CURVE for N[c] and g[c] per cell (n_* = 0 and
 * NULL when not asked for).  n_cells, cell_samples, first_sample, gmax, nmax and status are always filled.
 *
 * Per track: an analysis status other than SDSP_OK gives that status and zeroed fields (cell_samples
 * aside); a track whose key path is skipped gives n_cells 0 and leaves the status alone;
 * n_cells < 2 K gives one section and no boundary.
 */
enum sdsp_sections_what { SDSP_SECTIONS_LIST = 1, SDSP_SECTIONS_CURVE = 2 }; /* bits of sdsp_sections_request.what */
typedef struct sdsp_sections_request {
    uint32_t what;
    float cell_seconds;     /* the seconds form of Cs */
    uint64_t cell_samples;  /* the samples form of Cs */
    uint32_t kernel_cells;  /* K */
    uint32_t min_gap_cells; /* G */
    float energy_weight, min_strength, snap_seconds;
} sdsp_sections_request;

typedef struct sdsp_section {
    uint64_t start_cell, end_cell; /* cells [start_cell, end_cell) */
    float start_time, end_time;
    float strength, mean_energy, relative_energy;
    float snapped_time;
    int32_t downbeat;              /* index into the result's downbeats, or -1 */
} sdsp_section;

typedef struct sdsp_sections {
    int32_t status;         /* the track's sdsp_status */
    uint64_t n_cells, cell_samples;
    uint64_t first_sample;  /* trim start in the caller's track, as in sdsp_overview */
    float gmax, nmax;
    uint64_t n_sections;
    sdsp_section* sections; /* library-owned, one allocation with the curves */
    uint64_t n_curve;       /* n_cells with SDSP_SECTIONS_CURVE, else 0 */
    float* novelty;         /* N[c] */
    float* energy;          /* g[c] */
} sdsp_sections;

/*
 * The optional requests of one analysis call, by name: a later request is a new pair of fields at
 * the end, and a caller built against an older header (a smaller struct_size) keeps working.
 */
typedef struct sdsp_request_set {
    uint32_t struct_size; /* sizeof(sdsp_request_set) of the caller; fields past it read as NULL */
    const sdsp_overview_request* ov_req;     sdsp_overview* overviews;
    const sdsp_key_timeline_request* kt_req; sdsp_key_timeline* timelines;
    const sdsp_levels_request* lv_req;       sdsp_levels* levels;
    const sdsp_tempo_map_request* tm_req;    sdsp_tempo_map* tempo_maps;
} sdsp_request_set;

/*
 * The request set with the pairs added after the tempo map.  sdsp_request_set itself stays at its
 * four pairs (its size and last pair are pinned by the layout checks of callers built against it);
 * this struct begins with it, so in memory the fifth pair lies right at its end, and a later request
 * is a new pair at the end of this one.  Pass &ext.base with ext.base.struct_size = sizeof(ext): the
 * library reads sc_req / sections only when struct_size covers them, so a caller that passes a plain
 * sdsp_request_set (a smaller struct_size) keeps working.
 */
typedef struct sdsp_request_set_ext {
    sdsp_request_set base;
    const sdsp_sections_request* sc_req;     sdsp_sections* sections;
} sdsp_request_set_ext;

/*
 * ---- Programme loudness (ITU-R BS.1770-4 / EBU R 128) of every track of an analysis call ----
 *
 * Integrated loudness in LUFS with the absolute and the relative gate, the loudness range (EBU Tech
 * 3342), the maximum momentary and short-term loudness, the sample peak and a 4x-oversampled true
 * peak, from the samples the call already holds on the device.  (The levels request's "LUFS" is the
 * reference crate's own measure, one shelving stage and no relative gate; it is unchanged.)
 *
 * The definition.  All arithmetic is f32, every sum starts from 0 and runs in ascending index order,
 * multiply and add are separate operations, log10 is sdsp_libm.h's.  x[0..n) is the caller's raw
 * track (before normalisation and trim, as for levels), sr the call's sample rate, step = sr / 10,
 * J = n / step (integer divisions).
 *   Coefficients, computed in double and rounded to f32 (returned in shelf[] / highpass[] as
 *   b0 b1 b2 a1 a2).  Shelf: K = tan(pi * 1681.974450955533 / sr), Vh = 10^(3.999843853973347 / 20),
 *   Vb = Vh^0.4996667741545416, Q = 0.7071752369554196, a0 = 1 + K/Q + K*K,
 *   b = {(Vh + Vb*K/Q + K*K)/a0, 2(K*K - Vh)/a0, (Vh - Vb*K/Q + K*K)/a0}, a = {2(K*K - 1)/a0,
 *   (1 - K/Q + K*K)/a0}.  High-pass: K = tan(pi * 38.13547087602444 / sr), Q = 0.5003270373238773,
 *   b = {1, -2, 1}, a as above.  At 48 kHz these are the standard's table to its printed digits.
 *   Step energies.  For step j both filters start from zero state at sample max(j - 1, 0) * step and
 *   run, Direct Form II transposed (o = b0*s + x1; x1 = (b1*s + x2) - a1*o; x2 = b2*s - a2*o), the
 *   shelf feeding the high-pass, through sample (j + 1) * step - 1.  z[j] is the sum of o*o of the
 *   high-pass output over step j's own samples.  Samples past J * step are not measured.
 *   Blocks.  Momentary m[j] = (((z[j] + z[j+1]) + z[j+2]) + z[j+3]) / (f32)(4 * step), j in [0, J - 3);
 *   short-term s[j] = (the ascending sum of z[j .. j+30)) / (f32)(30 * step), j in [0, J - 29).
 *   L(e) = -0.691f + 10 log10(e).
 *   Integrated.  Ga = 10^((-70 + 0.691) / 10) (the levels request's gate constant).  A = the blocks
 *   with m > Ga, Gr = mean(A) * 0.1f; integrated_lufs = L(mean of the m with m > Ga and m > Gr), both
 *   means in block order; n_gated_momentary is the second mean's count.
 *   Range.  Of the s > Ga, the mean times 0.01f is the relative gate; the s above both gates, sorted
 *   ascending, are e[0..M): range_low = L(e[((M-1)*10 + 50) / 100]), range_high = L(e[((M-1)*95 + 50)
 *   / 100]), range_lu = range_high - range_low; has_range = 0 and the three fields 0 when M == 0.
 *   n_gated_short_term = M.
 *   Maxima.  L of the largest m and of the largest s, ungated; -inf without a block.
 *   Peaks.  sample_peak = max |x[i]|.  true_peak = the larger of sample_peak and the maximum over
 *   i in [0, n), p in {1, 2, 3} of |sum over k = 0..11 of h[p][k] * x[i + k - 5]|, x = 0 outside the
 *   track, h[p][k] = sinc(t) * (0.5 + 0.5 cos(pi t / 6)), t = (k - 5) - p/4, in double rounded to f32:
 *   4x oversampling with a 48-tap Hann-windowed sinc, the size of BS.1770 Annex 2's filter but not its
 *   table.  dB values are 20 log10; the dB of 0 is -inf.
 *
 * What these numbers are.  The engine holds the mono mix: this is BS.1770 with one channel of weight
 * 1, and a centre-panned stereo file reads 3.01 LU below its stereo programme loudness.  The filter
 * is restarted one step before each step instead of running through the track; its slowest pole
 * (the 38 Hz high-pass) has decayed below f32 rounding by then, and on noise, a DC-offset track and
 * a two-level track the integrated, momentary and short-term values lie within 0.00006 LU of an
 * unbroken f64 filter's at 48 kHz (tests/test_r128_ref.py; the bound asserted there is 0.01 LU).  The 4x grid
 * under-reads peaks of tones near Nyquist by up to 0.44 dB (cos 18 degrees), as the standard notes.
 * Non-finite samples are out of scope.
 *
 * SDSP_R128_CURVES needs SDSP_R128_LOUDNESS.  Without SDSP_R128_LOUDNESS only the peak fields (and
 * n_samples, step_samples, the coefficients) are filled; without SDSP_R128_TRUE_PEAK true_peak is 0
 * and true_peak_dbtp -inf.  A track with n > 0 under a supported configuration has SDSP_OK whatever its
 * analysis status (as for levels); another has the analysis status and zeroed fields.
 */
enum sdsp_r128_what { SDSP_R128_LOUDNESS = 1, SDSP_R128_TRUE_PEAK = 2, SDSP_R128_CURVES = 4 }; /* bits of sdsp_r128_request.what */
typedef struct sdsp_r128_request { uint32_t what; } sdsp_r128_request;

typedef struct sdsp_r128 {
    int32_t status;
    int8_t has_integrated, has_range;      /* 0: no block passed the gates */
    float integrated_lufs;                 /* -inf when has_integrated is 0 */
    float range_lu, range_low_lufs, range_high_lufs;
    float max_momentary_lufs, max_short_term_lufs;  /* -inf without a block */
    float sample_peak, true_peak;          /* linear; true_peak 0 without SDSP_R128_TRUE_PEAK */
    float sample_peak_db, true_peak_dbtp;
    uint64_t n_samples;                    /* the caller's track length */
    uint32_t step_samples;                 /* sample_rate / 10 */
    uint64_t n_steps, n_momentary, n_short_term, n_gated_momentary, n_gated_short_term;
    float shelf[5], highpass[5];           /* b0 b1 b2 a1 a2 as f32: a caller can recompute every field */
    float *momentary, *short_term;         /* mean squares per block, library-owned, one allocation; CURVES only */
} sdsp_r128;

/*
 * The request set with the pair added after sections: it begins with sdsp_request_set_ext (whose
 * last pair callers' layout checks pin), as that one begins with sdsp_request_set.  Pass
 * &ext2.base.base with ext2.base.base.struct_size = sizeof(ext2); the library reads r128_req / r128
 * only when struct_size covers them, so callers that pass either older struct keep working.
 */
typedef struct sdsp_request_set_ext2 {
    sdsp_request_set_ext base;
    const sdsp_r128_request* r128_req;       sdsp_r128* r128;
} sdsp_request_set_ext2;

/*
 * ---- Fingerprints: a chroma fingerprint per track and the duplicate pairs of an analysis call ----
 *
 * The one request that relates the tracks of a call to each other: the same recording twice (another
 * encoding, a re-download, a rip with a different lead-in).  A gain-invariant binary fingerprint from
 * short cells of the smoothed chroma rows, and every pair of the call's tracks compared on the device
 * at every alignment within max_offset_words.  The reference has no counterpart; this definition is
 * the contract.  Every output is an integer or one f32 quotient of two integers.
 *
 * What the numbers are: on synthetic material (24 s of non-repeating random triads, default
 * configuration, Cs = 5512, max_offset_words = 16, min_overlap_words = 32; CPU numbers of
 * tests/fingerprint_ref.py over the oracle's rows, tests/test_fingerprint_ref.py) copies of a track
 * with another gain, white noise 30 and 20 dB below its level or up to half a second cut from its
 * start read a bit error rate of at most 0.194 at the right offset (the noise 20 dB below), unrelated
 * tracks at least 0.460 at their best; at Cs = 11025 at most 0.171 and at least 0.442.  These are the
 * values that test measures.  That is no claim about real music; max_ber is the caller's decision.
 *
 * Scope: a track whose key path runs (SDSP_STAGES_FULL, trimmed length n >= frame_size and n >= the
 * key STFT's frame size).  kfs, khop, F and the rows C[f][0..12) are exactly as sdsp_key_timeline
 * defines them.  All float arithmetic is f32, sums start from 0 in ascending order, multiply and add
 * are separate operations.
 * Cells: Cs = cell_samples, or (u64)(cell_seconds * (f32)sample_rate); exactly one of the two is given
 *   (a form is given when its field is not 0).  khop <= Cs < 2^31.  n_cells = (F * khop) / Cs (integer
 *   division).  Cell c owns the key frames whose start f * khop lies in [c Cs, (c + 1) Cs), and
 *   m[c][i] = (sum over the cell's frames of C[f][i]) / (f32)count: the sections request's cell rule
 *   and fold over the key frames alone.
 * Words: W = n_cells >= 3 ? n_cells - 2 : 0.  For w in [0, W), i in [0, 12), j = (i + 1) % 12, with
 *   d(c) = m[c][i] - m[c][j]: bit i of word[w] is (d(w + 1) - d(w)) > 0, bit 12 + i is
 *   (d(w + 2) - d(w)) > 0, bits 24 to 31 are 0.  The twelve cyclic differences of a lag sum to zero, so
 *   a word is 0 exactly where the cell means did not move: silence, or a held constant (whose means
 *   are equal when the cells own equally many frames or their sums are exact; cells of 43 and of 44
 *   frames may round the mean of one value apart by an ulp and set bits).
 * Pairs: tracks a < b of the call, both with analysis status SDSP_OK and W >= 1; O = max_offset_words
 *   (0 to 255).  For o in [-O, O] the positions p run over [max(0, -o), min(W_a, W_b - o)); p is
 *   counted when (A[p] | B[p + o]) != 0; n(o) is the number of counted positions, e(o) the sum of
 *   popcount(A[p] ^ B[p + o]) over them.  o is eligible when n(o) >= max(min_overlap_words, 1).  The
 *   best offset minimises e / n (e1 * n2 < e2 * n1 in u64); on equality the smaller |o|, then the
 *   negative one.  A pair without an eligible offset has no best offset.  ber = (f32)e / (f32)(24 * n);
 *   the pair is a match when it has a best offset and ber <= max_ber.
 * Outputs: per track an sdsp_fingerprint (words with SDSP_FP_WORDS, else NULL; n_matches the matches
 *   the track takes part in, 0 without SDSP_FP_MATCH); per call, with SDSP_FP_MATCH, one
 *   sdsp_fingerprint_matches: n_compared the tracks with status SDSP_OK and W >= 1, n_pairs =
 *   n_compared (n_compared - 1) / 2, and the matches sorted by (a, b).  offset_samples =
 *   (first_sample_b + o * Cs) - first_sample_a: sample s of a's caller buffer meets sample
 *   s + offset_samples of b's.  bits_compared = 24 n.
 * Per track: an analysis status other than SDSP_OK gives that status and zeroed fields (cell_samples
 * aside) and the track is not compared; a track whose key path is skipped gives n_cells 0.  A track of
 * 2^27 words or more fails the call.
 */
enum sdsp_fingerprint_what { SDSP_FP_WORDS = 1, SDSP_FP_MATCH = 2 }; /* bits of sdsp_fingerprint_request.what */
typedef struct sdsp_fingerprint_request {
    uint32_t what;
    float cell_seconds;         /* the seconds form of Cs */
    uint64_t cell_samples;      /* the samples form of Cs */
    uint32_t max_offset_words;  /* O */
    uint32_t min_overlap_words;
    float max_ber;
} sdsp_fingerprint_request;

typedef struct sdsp_fingerprint {
    int32_t status;             /* the track's sdsp_status */
    uint64_t n_cells, n_words, cell_samples;
    uint64_t first_sample;      /* trim start in the caller's track, as in sdsp_overview */
    uint64_t n_matches;
    uint32_t* words;            /* library-owned; NULL without SDSP_FP_WORDS */
} sdsp_fingerprint;

typedef struct sdsp_fingerprint_match {
    uint64_t a, b;              /* track indices in the call, a < b */
    int32_t offset_words;
    int64_t offset_samples;
    uint64_t bit_errors, bits_compared;
    float ber;
} sdsp_fingerprint_match;

typedef struct sdsp_fingerprint_matches {
    uint64_t n_compared, n_pairs, n_matches;
    sdsp_fingerprint_match* matches; /* library-owned, sorted by (a, b) */
} sdsp_fingerprint_matches;

/*
 * The request set with the fields added after programme loudness: it begins with
 * sdsp_request_set_ext2, as that one begins with sdsp_request_set_ext.  Pass &ext3.base.base.base with
 * its struct_size = sizeof(ext3); the library reads fp_req / fingerprints / fp_matches only when
 * struct_size covers them, so callers that pass any of the three older structs keep working.
 */
typedef struct sdsp_request_set_ext3 {
    sdsp_request_set_ext2 base;
    const sdsp_fingerprint_request* fp_req;  sdsp_fingerprint* fingerprints;
    sdsp_fingerprint_matches* fp_matches;    /* one struct per call; needed with SDSP_FP_MATCH */
} sdsp_request_set_ext3;

/*
 * sdsp_analyze_batch_device_ex with any of the optional requests from one analysis: overviews and
 * key timelines as in sdsp_analyze_batch_device_requests (which forwards here), levels (n_tracks
 * entries, freed one by one with sdsp_levels_free) as above, with SDSP_STAGES_FULL and
 * SDSP_STAGES_BPM_ONLY alike.  set == NULL, or a set with every request NULL, is
 * sdsp_analyze_batch_device_ex itself (the same launches, the same results).  A request never
 * changes an sdsp_result.  Refused with SDSP_ERR_INVALID_INPUT before any device is touched, beside
 * what sdsp_analyze_batch_device_requests refuses: a levels request with what == 0 or with unknown
 * bits, a request without its output array, a struct_size smaller than the first request pair.
 * Tempo maps (n_tracks entries, freed one by one with sdsp_tempo_map_free) as above; also refused:
 * a tempo map request with what == 0 or unknown bits, or with SDSP_STAGES_BPM_ONLY, which has no
 * beat stage.  The nested exact key reruns never see a request.
 * Sections (sdsp_request_set_ext: n_tracks entries, freed one by one with sdsp_sections_free) as above.  Also refused with
 * SDSP_ERR_INVALID_INPUT: both cell forms or neither; a float that is not finite or is negative;
 * what == 0 or unknown bits; K == 0 or K > 64; G >= 2^31; Cs < max(khop, hop_size) or Cs >= 2^31; no
 * output array; SDSP_STAGES_BPM_ONLY.  With SDSP_ERR_NOT_IMPLEMENTED: force_legacy_bpm (no feature
 * pass, so no E), and enable_key_beat_synchronous without enable_key_log_frequency (the rows are
 * beats, as for the key timeline).
 * Programme loudness (sdsp_request_set_ext2: n_tracks entries, freed one by one with sdsp_r128_free)
 * as above, with SDSP_STAGES_FULL and SDSP_STAGES_BPM_ONLY alike.  Also refused with
 * SDSP_ERR_INVALID_INPUT: what == 0 or unknown bits; SDSP_R128_CURVES without SDSP_R128_LOUDNESS; no
 * output array; a sample rate under 8000 Hz.
 * Fingerprints (sdsp_request_set_ext3: n_tracks entries, freed one by one with sdsp_fingerprint_free,
 * and one sdsp_fingerprint_matches, freed with sdsp_fingerprint_matches_free) as above.  Also refused
 * with SDSP_ERR_INVALID_INPUT: what == 0 or unknown bits; both cell forms or neither; a float that is
 * not finite or is negative; max_ber > 1; Cs < khop or Cs >= 2^31; max_offset_words > 255;
 * SDSP_FP_MATCH without the matches struct; no output array; SDSP_STAGES_BPM_ONLY.  With
 * SDSP_ERR_NOT_IMPLEMENTED: enable_key_beat_synchronous without enable_key_log_frequency.
 * force_legacy_bpm is accepted: no frame energies are used.
 */
int32_t sdsp_analyze_batch_device_with(const float* d_samples, const uint64_t* offsets, const uint64_t* lens,
                                       uint64_t n_tracks, uint32_t sample_rate, const sdsp_config* cfg,
                                       int32_t device, void* stream, int32_t stages, sdsp_result* outs,
                                       const sdsp_request_set* set);
/* Frees the regions owned by one sdsp_levels. */
void sdsp_levels_free(sdsp_levels* l);
/* Frees the arrays owned by one tempo map (they share one allocation: never free() them one by one). */
void sdsp_tempo_map_free(sdsp_tempo_map* m);
/* Frees the arrays owned by one sdsp_sections (they share one allocation: never free() them one by one). */
void sdsp_sections_free(sdsp_sections* s);
/* Frees the curves owned by one sdsp_r128 (they share one allocation: never free() them one by one). */
void sdsp_r128_free(sdsp_r128* r);
/* Frees the words owned by one sdsp_fingerprint, and the list owned by one sdsp_fingerprint_matches. */
void sdsp_fingerprint_free(sdsp_fingerprint* f);
void sdsp_fingerprint_matches_free(sdsp_fingerprint_matches* m);

/*
 * Synthetic track generator on device: writes n_tracks tracks of `len`
 * samples each, track i at d_out + i*len, seeds seed0 + i.  bpm_out/key_out (host, may be
 * NULL) receive the generated tempo and key (key = mode*12 + tonic).  bpm_mode 0 = uniform
 * [70,180] on a 0.5 grid; 1 = thirds in [55,80], [170,200], [80,170] (config 5).
 */
int32_t sdsp_generate_synthetic(float* d_out, uint64_t n_tracks, uint64_t len, uint32_t sample_rate,
                                uint64_t seed0, int32_t bpm_mode, int32_t device, void* stream,
                                float* bpm_out, int32_t* key_out);

/*
 * Device-memory plumbing for harnesses that hold tracks in HBM (benchmarks, tests).  The engine
 * links the system ROCm HIP runtime; callers that use these need no second GPU runtime.
 */
int32_t sdsp_device_count(void);
int32_t sdsp_device_malloc(int32_t device, uint64_t bytes, void** ptr);
int32_t sdsp_device_free(int32_t device, void* ptr);
int32_t sdsp_memcpy_h2d(int32_t device, void* dst, const void* src, uint64_t bytes);
int32_t sdsp_memcpy_d2h(int32_t device, void* dst, const void* src, uint64_t bytes);
int32_t sdsp_device_synchronize(int32_t device);

/*
 * compute_confidence (src/analysis/confidence.rs:121-297): host-side scores of one result.
 * flag_list holds AnalysisFlag indices (0 MultimodalBpm, 1 WeakTonality, 2 TempoVariation,
 * 3 OnsetDetectionAmbiguous) in the reference's push order, duplicates kept (the result's own
 * flags first, then MultimodalBpm / WeakTonality / TempoVariation as their thresholds fire).
 */
typedef struct sdsp_confidence {
    float bpm_confidence;
    float key_confidence;
    float grid_stability;
    float overall_confidence;
    uint32_t n_flags;
    int32_t flag_list[8];
} sdsp_confidence;
int32_t sdsp_compute_confidence(const sdsp_result* result, sdsp_confidence* out);

/* Key::name (src/analysis/result.rs:31-39): "C", "F#", "Am", "C#m"; returns the length. */
int32_t sdsp_key_name(int32_t key_mode, uint32_t key_tonic, char* buf, uint64_t buflen);

/*
 * Audio decode front-end (examples/analyze_file.rs:25-180, analyze_batch.rs:30-177), by magic
 * number: RIFF/WAVE (PCM u8 / s16 / s24 / s32, IEEE float f32 / f64, G.711, IMA and Microsoft
 * ADPCM, WAVE_FORMAT_EXTENSIBLE with those sub-formats), AIFF / AIFF-C, CAF (lpcm, G.711, ALAC),
 * FLAC (native or in Ogg; 8-32 bits, 1-8 channels; symphonia's S32 buffers, sample << (32 -
 * bps)), ALAC in ISO MP4 / M4A, Ogg Vorbis, and Matroska / WebM carrying PCM, FLAC, ALAC or
 * Vorbis -- decoded to mono f32 as the reference's
 * symphonia path converts its buffers (s16 / 32768, s24 / 8388608, s32 / 2147483648, (u8 - 128) /
 * 128, f64 -> f32, f32 as is; channels summed in order and divided by the channel count).  A
 * packet that fails to decode (a FLAC frame failing its CRC, a damaged ALAC packet, an Ogg page
 * failing its CRC) is skipped, as the examples skip such a packet.  *samples is malloc'ed (free
 * with sdsp_free_samples).  Returns 0, or SDSP_ERR_DECODING with the reason in err (MP3 / MP2 /
 * MP1, AAC and Opus are named as unsupported codecs).
 */
int32_t sdsp_decode_audio_file(const char* path, float** samples, uint64_t* n_samples, uint32_t* sample_rate,
                               char* err, uint64_t errlen);
void sdsp_free_samples(float* samples);

/*
 * Batched FLAC decode on the device (new; the reference decodes on the host): n_files native FLAC
 * files held in memory ("fLaC", or an ID3v2 tag then "fLaC") are decoded by HIP kernels on `device`
 * into one device buffer of concatenated mono f32 tracks, bit-identical to sdsp_decode_audio_file
 * on the same bytes.  Track i is (*d_samples)[offsets[i] .. offsets[i] + lens[i]) at
 * sample_rates[i]: the arguments of sdsp_analyze_batch_device, per sample rate.  *d_samples is
 * owned by the caller (sdsp_device_free).  `stream` is a hipStream_t (NULL = the library's own);
 * the call returns after the buffer is complete.
 *
 * status[i] and errs + 256 * i (NUL-terminated) are what sdsp_decode_audio_file returns for the
 * same bytes in a file; a failed file has lens[i] = 0 and the others still decode.  A file the
 * device path does not take (not native FLAC, 2 GiB or more, more frame-header candidates than one
 * per 8 bytes, or past the HBM budget of the call) is decoded by the host decoder, uploaded and
 * counted in host_fallback_files.  Returns SDSP_OK unless the call itself could not run (no HIP
 * device: SDSP_ERR_PROCESSING and "Processing error: no HIP device" in every errs slot).
 */
typedef struct sdsp_flac_decode_stats {
    uint64_t files, device_files, host_fallback_files, error_files;
    uint64_t candidates, frames_accepted, frames_rejected;
    uint64_t bytes_in, samples_out;
    double scan_ms, frames_ms, chain_ms, gather_ms, total_ms;
} sdsp_flac_decode_stats;

int32_t sdsp_decode_flac_batch_device(const uint8_t* const* files, const uint64_t* sizes, uint64_t n_files,
                                      int32_t device, void* stream,
                                      float** d_samples, /* out: free with sdsp_device_free */
                                      uint64_t* offsets, uint64_t* lens, uint32_t* sample_rates,
                                      int32_t* status, char* errs /* n_files x 256 */);
/* Counters and phase times (HIP events; total_ms is the call's wall time) of the last call on `device`. */
int32_t sdsp_last_flac_decode_stats(int32_t device, sdsp_flac_decode_stats* out);

/*
 * Batched lossless decode on the device: one entry for every lossless family the front-end reads.
 * Arguments, ownership and per-file results are those of sdsp_decode_flac_batch_device: n_files
 * files held in memory are decoded into one caller-owned device buffer of concatenated mono f32
 * tracks (sdsp_device_free), track i bit-identical to sdsp_decode_audio_file on the same bytes,
 * status[i] and errs + 256 * i the host's; a failed file has lens[i] = 0 and the others still
 * decode; the call returns after the buffer is complete.  Each file is dispatched by content, as
 * the front-end probes it:
 *   native FLAC                          the FLAC kernels (scan, frames, chain, gather)
 *   ALAC in ISO MP4 / M4A and in CAF     the ALAC kernels: one lane per packet (the container's
 *                                        sample table gives every packet), offsets, gather
 *   RIFF/WAVE and AIFF / AIFF-C with     the PCM kernel: conversion and channel mix
 *   linear PCM (u8 / s16 / s24 / s32 / f32 / f64, either byte order, up to 8 channels)
 * Everything else is decoded by the host decoder, uploaded into the same buffer and counted in
 * host_fallback_files: G.711, ADPCM, CAF lpcm, Ogg, Matroska, every unsupported codec (which gets
 * the host's error text), an ALAC frame length above 16384, PCM wider than 8 channels, a file of
 * 2 GiB or more, files past the call's HBM budget.  A container the host plan refuses (a missing
 * cookie or sample table, AAC in MP4, a packet outside the file) is that file's error, not a
 * fallback.  With no HIP device: SDSP_ERR_PROCESSING and "Processing error: no HIP device" in every
 * errs slot.
 */
typedef struct sdsp_decode_stats {
    uint64_t files, device_files, host_fallback_files, error_files;
    uint64_t flac_files, alac_files, pcm_files; /* device files per family */
    uint64_t alac_packets, alac_packets_decoded, alac_packets_skipped;
    uint64_t bytes_in, samples_out;
    double upload_ms, flac_ms, alac_ms, pcm_ms, gather_ms; /* HIP events */
    double total_ms;                                       /* the call's wall time */
} sdsp_decode_stats;

int32_t sdsp_decode_batch_device(const uint8_t* const* files, const uint64_t* sizes, uint64_t n_files,
                                 int32_t device, void* stream,
                                 float** d_samples, /* out: free with sdsp_device_free */
                                 uint64_t* offsets, uint64_t* lens, uint32_t* sample_rates,
                                 int32_t* status, char* errs /* n_files x 256 */);
/* Counters and phase times of the last sdsp_decode_batch_device call on `device`
 * (sdsp_last_flac_decode_stats keeps reporting calls made through the FLAC entry). */
int32_t sdsp_last_decode_stats(int32_t device, sdsp_decode_stats* out);

/*
 * Batched decode on the device of everything the front-end reads: sdsp_decode_batch_device with
 * Ogg Vorbis on the device as well.  Arguments, ownership, per-file status and error texts are
 * those of sdsp_decode_batch_device, and every file that entry dispatches is dispatched the same
 * way here; in addition
 *   Ogg Vorbis (the first logical stream)  the Vorbis kernels: one lane per packet decodes floors,
 *                                          residues and coupling into spectra, the inverse MDCT and
 *                                          window per (packet, channel), the overlap-add and mono
 *                                          mix per output sample
 * bit-identical to sdsp_decode_audio_file on the same bytes.  The host plan reads the Ogg pages,
 * the headers and each audio packet's first bits, so a header the host decoder refuses is that
 * file's error with the host's text, not a fallback.  Decoded by the host decoder, uploaded and
 * counted in host_fallback_files: G.711, ADPCM, CAF lpcm, Ogg FLAC, Opus and every other
 * unsupported codec (which gets the host's error text), Matroska (Vorbis in Matroska included), an
 * ALAC frame length above 16384, PCM wider than 8 channels, a Vorbis setup whose flattened tables
 * exceed 64 MiB, a file of 2 GiB or more, files past the call's HBM budget.  sdsp_decode_batch_device
 * keeps its contract: there an Ogg file is a host fallback.
 */
typedef struct sdsp_audio_decode_stats {
    uint64_t files, device_files, host_fallback_files, error_files;
    uint64_t flac_files, alac_files, pcm_files, vorbis_files; /* device files per family */
    uint64_t alac_packets, alac_packets_decoded, alac_packets_skipped;
    uint64_t vorbis_packets;        /* kept audio packets of the device Vorbis files */
    uint64_t vorbis_packets_zeroed; /* of those: a floor decode failed, the block is silent */
    uint64_t bytes_in, samples_out;
    double upload_ms, flac_ms, alac_ms, pcm_ms, gather_ms, vorbis_ms; /* HIP events */
    double total_ms;                                                  /* the call's wall time */
} sdsp_audio_decode_stats;

int32_t sdsp_decode_audio_batch_device(const uint8_t* const* files, const uint64_t* sizes, uint64_t n_files,
                                       int32_t device, void* stream,
                                       float** d_samples, /* out: free with sdsp_device_free */
                                       uint64_t* offsets, uint64_t* lens, uint32_t* sample_rates,
                                       int32_t* status, char* errs /* n_files x 256 */);
/* Counters and phase times of the last sdsp_decode_audio_batch_device call on `device`. */
int32_t sdsp_last_audio_decode_stats(int32_t device, sdsp_audio_decode_stats* out);

/* Library identification: "stratum-hip <abi> gfx950" */
const char* sdsp_version(void);

/* Per-kernel timing of the last batch on `device` (bench/roofline), milliseconds. */
typedef struct sdsp_stage_times {
    double stft2048_ms;     /* k_stft_mag<2048> launches, summed */
    double stft8192_ms;     /* k_stft_mag<8192> launches, summed */
    double features_ms;     /* frame features + novelty */
    double tempogram_ms;    /* FFT + autocorrelation tempograms + candidate scoring */
    double key_ms;          /* mask + HPCP + key voting */
    double beat_ms;         /* onset consensus + beat grid */
    double total_ms;        /* whole batch, device time */
    uint64_t stft2048_launches;
    uint64_t stft8192_launches;
    double stft2048_bytes;  /* algorithmic bytes: 4*N_in + 4*F*(nfft/2+1) per STFT */
    double stft8192_bytes;
    uint64_t stft2048_frames; /* frames the STFT launches computed (the VALU census is per frame) */
    uint64_t stft8192_frames;
    uint64_t key_reruns;      /* tracks analysed again with the sequential key-energy fold (near a
                                 key decision under the block-folded energies) */
    double rerun_ms;          /* wall time of that rerun (included in total_ms) */
} sdsp_stage_times;
int32_t sdsp_last_stage_times(int32_t device, sdsp_stage_times* out);

#ifdef __cplusplus
}
#endif

#endif /* STRATUM_HIP_H */
