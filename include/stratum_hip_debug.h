/*
 * stratum_hip_debug.h -- test and probe entry points of libstratum_hip.so.
 *
 * Not part of the drop-in boundary (include/stratum_hip.h): no reference interface corresponds to
 * these.  They exist for the parity tests (stage probes compared against the oracle), the
 * benchmark's isolated kernel timing and the failure-path tests.  The library reads no test switch
 * from the environment; the hooks below are set only through sdsp_debug_set_test_hooks.
 */
#ifndef STRATUM_HIP_DEBUG_H
#define STRATUM_HIP_DEBUG_H

#include <stdint.h>

#include "stratum_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Test hooks, process-wide: fail_chunk >= 0 makes sdsp_analyze_batch's chunk of that index throw
 * (the per-chunk failure path); devices[0..n_devices) replaces the device mask's worker list
 * (repeats allowed: two workers on device 0 run the multi-device chunk path on one GPU);
 * stft_frame_parallel != 0 forces the frame-parallel STFT kernel for every hop.  Reset with
 * (-1, NULL, 0, 0).
 */
int32_t sdsp_debug_set_test_hooks(int64_t fail_chunk, const int32_t* devices, uint32_t n_devices,
                                  int32_t stft_frame_parallel);

/*
 * Schedule knobs, process-wide (0 = the product's schedule): serial_streams != 0 runs the key path
 * on the main stream (per-kernel profiling); no_key_defer != 0 joins each sub-batch's key stream at
 * its own end instead of one sub-batch late; no_row_reuse != 0 recomputes the escalation passes'
 * hop-512 rows instead of reading the base pass's; host_trace != 0 prints per-stage host times on
 * stderr; batch_chunk_tracks > 0 sets sdsp_analyze_batch's chunk size (default 512 tracks);
 * hbm_budget_gb > 0 sets the sub-batch HBM budget (default: 80 % of free HBM / 1.125).  Every
 * setting gives the same results; the tests use them to reach the other schedules and the tools
 * to profile.  The Python layer maps SDSP_SERIAL_STREAMS, SDSP_NO_KEY_DEFER, SDSP_NO_ROW_REUSE,
 * SDSP_HOST_TRACE, SDSP_BATCH_CHUNK_TRACKS and SDSP_HBM_BUDGET_GB onto this call; the library
 * itself reads no environment variable.
 */
int32_t sdsp_debug_set_schedule(int32_t serial_streams, int32_t no_key_defer, int32_t no_row_reuse, int32_t host_trace,
                                uint64_t batch_chunk_tracks, double hbm_budget_gb);

/*
 * 1 when `cfg` at `sample_rate` takes the default key path's band-limited mask with HPCP frame
 * energies folded in 64-bin blocks (k_mask_rp / k_hpcp_band: key_confidence and key_clarity are
 * then a re-associated sum of the reference's), 0 when it keeps the reference's
 * single sequential energy fold, -1 on a NULL config or a zero rate.  No device is touched.
 */
int32_t sdsp_debug_key_energy_blocked(const sdsp_config* cfg, uint32_t sample_rate);

/*
 * Per track of the last analysis call on `device` (n entries): non-zero where the block-folded
 * key energies left a key decision within its margin, so the track's key path ran again with the
 * sequential energy fold (sdsp_stage_times.key_reruns counts them), else 0.  Bits: 1 a segment's
 * (or the slice's) within-mode argmax, 2 a segment clarity gate, 4 the final key gap, 8 the
 * weight-sum fallback, 16 a weight, energy or mode top outside the certificate's range (underflow,
 * no usable bound, near the 1e-9 normalisation guard).
 */
int32_t sdsp_debug_last_key_near(int32_t device, uint8_t* out, uint64_t n);

/*
 * The key vote's near-decision certificate on the default key path: 0 (default) the
 * rigorous bounds (per-frame energy bounds carried through the weights, raw scores, clarities and
 * the vote, with the fixed margins as floors); non-zero the fixed round-5 margins alone (A/B of the
 * flagged sets).  Process-wide; applies to the next analysis calls.
 */
int32_t sdsp_debug_set_key_cert(int32_t fixed_margins);

/* Free and total HBM bytes of `device` (the benchmark sizes its kernel probe by them). */
int32_t sdsp_debug_mem_info(int32_t device, uint64_t* free_bytes, uint64_t* total_bytes);

/* PCI bus id of HIP device `device` ("dddd:bb:dd.f", NUL-terminated; len >= 13). */
int32_t sdsp_debug_device_pci_bus_id(int32_t device, char* out, uint32_t len);

/* Device allocations the engine has made so far (count, bytes): "a repeated call allocates nothing". */
int32_t sdsp_debug_alloc_stats(uint64_t* n_allocs, uint64_t* bytes);

/*
 * STFT magnitudes of one host buffer (x * gain framed at hop), frames x (nfft/2 + 1) into host_out;
 * frame maxima into host_frame_max (NULL allowed; not for nfft 8192).
 */
int32_t sdsp_debug_stft(const float* host_x, uint64_t n, uint64_t nfft, uint64_t hop, float gain, float* host_out,
                        float* host_frame_max, int32_t device);

/*
 * Frame RMS of n_tracks host tracks (track t = host_x[offs[t] .. offs[t] + lens[t])), frames of fs
 * samples every hop, the silence-trimming framing; per_frame = 1 forces the per-frame kernel.
 */
int32_t sdsp_debug_frame_rms(const float* host_x, uint64_t n_total, const uint64_t* offs, const uint64_t* lens,
                             const float* gains, uint64_t n_tracks, uint64_t fs, uint64_t hop, int32_t per_frame,
                             float* host_out, int32_t device);

/*
 * Tracks of the last analysis call on `device` whose key path was rerun in place over the last
 * sub-batch's band-path buffers (the sequential energy fold without a second STFT);
 * the other reruns counted in sdsp_stage_times.key_reruns ran the nested key-only pipeline.
 */
int32_t sdsp_debug_last_tail_reruns(int32_t device, uint64_t* n_tracks);

/*
 * The overview kernels of the last sdsp_analyze_batch_device_overview call with a request on
 * `device`, summed over its sub-batches: HIP event times of the sample-envelope kernel
 * (k_ov_segments) and of the band-envelope kernels (k_ov_columns, and k_ov_fold where a column is
 * cut into pieces), the bytes each reads by the definition (4 n per track; 4 F (frame_size / 2 + 1)
 * per track), and the columns produced.  All zero after a call without a request.
 */
typedef struct sdsp_debug_overview_times {
    double sample_ms, band_ms;
    double sample_bytes, band_bytes;
    uint64_t columns, sub_batches;
} sdsp_debug_overview_times;
int32_t sdsp_debug_last_overview_times(int32_t device, sdsp_debug_overview_times* out);

/*
 * The levels folds of the last sdsp_analyze_batch_device_with call with a levels request on
 * `device`: HIP event times of the first launch (the peak kernels and k_levels_fold with every
 * chain but Loudness' rms_db) and of the second (k_levels_gain and that chain), and the tracks
 * folded.  The events lie on the fold stream, so beside a running analysis they include what the
 * folds waited for.  All zero after a call without a request.
 */
typedef struct sdsp_debug_levels_times {
    double fold_ms, fold2_ms;
    uint64_t tracks;
} sdsp_debug_levels_times;
int32_t sdsp_debug_last_levels_times(int32_t device, sdsp_debug_levels_times* out);

/*
 * Stage probe of the key timeline (include/stratum_hip.h, sdsp_key_timeline): the timeline kernel
 * and the host's primary-key and change logic over uploaded chroma rows, taken as the smoothed rows
 * C of the definition.  host_chroma: the tracks' rows back to back, frames[t] rows of 12 floats for
 * track t (0 allowed).  out[t] (n_tracks entries, sdsp_key_timeline_free) is filled as an analysis
 * call fills it, with first_sample 0 and status SDSP_OK.  SDSP_ERR_INVALID_INPUT for a request
 * sdsp_analyze_batch_device_requests refuses.
 */
int32_t sdsp_debug_key_timeline(const float* host_chroma, const uint64_t* frames, uint64_t n_tracks,
                                uint32_t sample_rate, const sdsp_config* cfg,
                                const sdsp_key_timeline_request* req, sdsp_key_timeline* out, int32_t device);

/*
 * Stage probe of the tempo path: the pipeline's own tempo pass (features, novelty, both tempograms;
 * the same parameter set-up and launches as an analysis call) over host magnitude spectrograms
 * instead of an STFT.  host_mags holds the tracks' rows back to back, frame_size / 2 + 1 values per
 * row (cfg->frame_size), frames[t] >= 1 rows for track t; total = the sum of frames.  The caller
 * allocates every array of `out`; the probe fills them in the kernels' own layout:
 *   E, H, SFX      4 x total, variant-major (full, low, mid, high); SFX and SFO of the frame pair
 *                  (f, f + 1) at f, so the last frame of a track is not written
 *   SFO            total
 *   MEL            mel_cap x total, mel-major; n_mels rows written
 *   nov            5 x total (full, low, mid, high, mel), frames - 1 values per track and present
 *                  variant; nov_sum 5 x n_tracks, variant-major
 *   acf, fft       per (track, variant) slot t * 5 + v: acf_cap (fft_cap) pairs (bpm, value) in the
 *                  order the kernels wrote them; acf_n / fft_n (n_tracks x 5) the entries written
 *                  (0 for an absent variant or a track of one frame)
 * and the band edges [bs, be), band_on[4], present[5], n_mels and the ACF grid size NB it used.
 * Fails with SDSP_ERR_INVALID_INPUT when a capacity is too small.  Allocates only buffers of its
 * own, released before it returns.
 */
typedef struct sdsp_debug_tempo_out {
    float *E, *H, *SFX, *SFO, *MEL, *nov, *nov_sum, *acf, *fft;
    int32_t *acf_n, *fft_n;
    uint32_t mel_cap, acf_cap, fft_cap;
    int32_t n_mels, NB;
    int32_t bs[4], be[4], band_on[4], present[5];
} sdsp_debug_tempo_out;
int32_t sdsp_debug_tempo_stages(const float* host_mags, const uint64_t* frames, uint64_t n_tracks, uint32_t sample_rate,
                                uint32_t hop, const sdsp_config* cfg, sdsp_debug_tempo_out* out, int32_t device);

/*
 * Stage probe of the key path: the pipeline's own key conditioning and chroma launches over host
 * key spectrograms (rows of key-FFT / 2 + 1 values, 4097 by default; frames[t] >= 1 rows per track).
 *   mode 0  the path the configuration selects (default: k_mask_rp on [pk_lo - 1, pk_hi + 1], then
 *           k_hpcp_band with block-folded energies and the per-frame bound edel)
 *   mode 1  the in-place rerun's sequence: mode 0's band mask, the mask outside the band, k_hpcp
 *   mode 2  the nested rerun's sequence: one full-width band-kernel mask, k_hpcp
 * Modes 1 and 2 need a configuration with sdsp_debug_key_energy_blocked() == 1.  Returns the
 * spectrogram after conditioning (total x bins), chroma (total x 12), energy (total) and, where the
 * band path ran (mode 0), edel (total; untouched otherwise).  info = {st_lo, st_hi, band path ran,
 * bins}; st_lo > st_hi when no band-limited mask ran.
 */
int32_t sdsp_debug_key_stages(const float* host_mags, const uint64_t* frames, uint64_t n_tracks, uint32_t sample_rate,
                              const sdsp_config* cfg, int32_t mode, float* masked, float* chroma, float* energy,
                              float* edel, int32_t info[4], int32_t device);

/*
 * Stage probe of the key vote: the pipeline's own vote launch (k_key_vote through its launcher, with
 * the parameters, templates and segment scratch sizing of an analysis call) over uploaded chroma rows
 * and frame energies instead of a spectrogram.  host_chroma holds the tracks' raw rows back to back,
 * frames[t] >= 1 rows of 12 floats for track t (total = their sum); host_energy one value per row;
 * host_edel (NULL allowed) the per-frame relative energy bound of the band path.  With host_edel the
 * launch is the band path's (near_check = 1, edel and wdel passed: the near-decision certificate
 * runs, rigorous unless cert_fixed != 0); without it the exact path's (near_check = 0, no bounds).
 * sel / n_sel: NULL / 0 votes on every track in order; otherwise the listed track indices (a subset,
 * in any order, no repeats), launched as the in-place rerun launches its selection: the item list
 * is `sel`, the segment scratch offsets are compact by item and the frame prefix stays by track.
 * threads: 0 the launcher's own choice from the item count and `alone` (the flag an analysis call
 * sets for a launch with nothing beside it); 256, 512 or 1024 force that instantiation.
 * The caller allocates every array of `out`:
 *   key        n_tracks records as the kernel wrote them; the probe uploads the caller's contents
 *              first, so the records of tracks outside `sel` come back untouched
 *   chroma_s   total x 12, the sharpened and smoothed rows (zero for tracks outside `sel`)
 *   weights    total, the frame weights over the voted slice (zero elsewhere)
 *   wdel       total, the certificate's per-frame weight bounds; written only with host_edel
 *   seg_rows   the segment scratch, 128 floats per row (24 sorted scores, 24 key indices, clarity at
 *              [48], gate decision at [49], clarity x scale weight at [50], the certificate's columns
 *              from [64]); item i's rows start at row seg_row_pfx[i] (n_items + 1 entries written),
 *              sized as the pipeline sizes them; seg_rows_cap rows must hold seg_row_pfx[n_items]
 *   dbg        n_items records: the final sorted table, its key indices, the chosen key, the
 *              weighted pitch-class summary, slice frames and used frames
 * n_items = n_sel, or n_tracks without a selection.  SDSP_ERR_INVALID_INPUT for a bad selection or
 * a capacity too small.  Allocates only buffers of its own, released before it returns.
 */
typedef struct sdsp_debug_key_out {
    int32_t mode, tonic;
    float conf, clarity;
    int32_t ok, used_segments, weights_used, near;
} sdsp_debug_key_out;
typedef struct sdsp_debug_key_dbg {
    float tab[24];
    int32_t order[24];
    int32_t key;
    float agg[12];
    int32_t frames, used;
} sdsp_debug_key_dbg;
typedef struct sdsp_debug_key_vote_out {
    sdsp_debug_key_out* key;
    float *chroma_s, *weights, *wdel, *seg_rows;
    uint64_t* seg_row_pfx;
    uint64_t seg_rows_cap;
    sdsp_debug_key_dbg* dbg;
} sdsp_debug_key_vote_out;
int32_t sdsp_debug_key_vote(const float* host_chroma, const float* host_energy, const float* host_edel,
                            const uint64_t* frames, uint64_t n_tracks, const int32_t* sel, uint64_t n_sel,
                            uint32_t sample_rate, const sdsp_config* cfg, int32_t threads, int32_t alone,
                            int32_t cert_fixed, sdsp_debug_key_vote_out* out, int32_t device);

/*
 * Stage probe of the onset detectors and their consensus: the pipeline's own buffer set-up and
 * launches (k_energy_onsets, k_flux_onsets, k_consensus, as an analysis call makes them after its
 * frame RMS) over uploaded per-frame curves instead of samples and a spectrogram.  Every curve
 * holds the tracks' frames back to back, frames[t] >= 1 values for track t (total = their sum):
 *   rms   the frame RMS of the trimmed signal (the energy-flux detector's input)
 *   hfc   the full-band HFC per frame (E/H/SFX variant 0 of sdsp_debug_tempo_stages)
 *   sfo   the spectral-flux onset curve, the pair (f, f + 1) at f; a track's last value is not read
 *   hpe   the frame energy of the percussive spectrogram; NULL allowed (then, with
 *         enable_hpss_onsets, the HPSS lists are empty, as for a pass without frames)
 * n_trim[t] is the trimmed length in samples (an onset at frame f is kept when f * hop < n_trim);
 * hop >= 1 with frames[t] * hop < 2^32.  cfg supplies onset_threshold_percentile, the consensus
 * switch, tolerance and weights and enable_hpss_onsets.  The caller allocates `out`: energy,
 * spectral, hfc and hpss hold `total` sample positions each, track t's list at its frame prefix;
 * chosen holds 4 x total, track t's at 4 x its frame prefix; n_* (n_tracks each) the entries
 * written.  hpss counts are 0 without HPSS onsets.  Allocates only buffers of its own, released
 * before it returns.
 */
typedef struct sdsp_debug_onset_out {
    uint32_t *energy, *spectral, *hfc, *hpss, *chosen;
    int32_t *n_energy, *n_spectral, *n_hfc, *n_hpss, *n_chosen;
} sdsp_debug_onset_out;
int32_t sdsp_debug_onset_stages(const float* rms, const float* hfc, const float* sfo, const float* hpe,
                                const uint64_t* frames, const uint64_t* n_trim, uint64_t n_tracks, uint32_t sample_rate,
                                uint32_t hop, const sdsp_config* cfg, sdsp_debug_onset_out* out, int32_t device);

/*
 * Stage probe of the beat grid: the pipeline's own beat stage (k_beat with its capacity formula,
 * then the compaction kernel its track count selects, and the download) over uploaded consensus
 * onsets and tempo estimates instead of an analysis.  onsets holds the tracks' ascending sample
 * positions back to back, n_onsets[t] of them for track t; frames[t] >= 1 and n_trim[t] are the
 * track's base-pass frame count and trimmed length, from which the pipeline sizes its lists: the
 * consensus list holds lists x frames[t] entries (lists = 4 with HPSS onsets, else 3) and the beat
 * lists cap[t] = max(12 (n_trim[t] / sample_rate + 1) + 64, 3 frames[t] + 8).  An onset list longer
 * than either is refused with SDSP_ERR_INVALID_INPUT (the analysis call cannot produce one).  bpm[t], conf[t]:
 * the final tempo estimate.  The caller allocates `out`: ok (1 a grid, 0 none, -1 a list outgrew
 * cap[t]), n_beats, n_down and stability per track as k_beat wrote them, and the beats and
 * downbeats of the tracks with ok = 1 back to back in track order (the sum of cap[t] entries
 * suffices).  Allocates only buffers of its own, released before it returns.
 */
typedef struct sdsp_debug_beat_out {
    int32_t *ok, *n_beats, *n_down;
    float *stability, *beats, *downs;
} sdsp_debug_beat_out;
int32_t sdsp_debug_beat_grid(const uint32_t* onsets, const uint64_t* n_onsets, const uint64_t* frames,
                             const uint64_t* n_trim, const float* bpm, const float* conf, uint64_t n_tracks,
                             uint32_t sample_rate, const sdsp_config* cfg, sdsp_debug_beat_out* out, int32_t device);

/*
 * Stage probe of the tempo map (include/stratum_hip.h, sdsp_tempo_map): sdsp_debug_beat_grid's
 * arguments, set-up and launches with the pipeline's own tempo map step queued behind k_beat and
 * read back with the beat lists, as an analysis call with a tempo map request does.  what: the
 * request's bits.  maps receives n_tracks maps (free each with sdsp_tempo_map_free): status SDSP_OK,
 * or SDSP_ERR_PROCESSING with zeroed fields for a track whose lists outgrew their capacity; the onset
 * list is the uploaded one, first_sample 0.  beats (NULL allowed) receives what sdsp_debug_beat_grid
 * returns, from the same launch.  Allocates only buffers of its own, released before it returns.
 */
int32_t sdsp_debug_tempo_map(const uint32_t* onsets, const uint64_t* n_onsets, const uint64_t* frames,
                             const uint64_t* n_trim, const float* bpm, const float* conf, uint64_t n_tracks,
                             uint32_t sample_rate, const sdsp_config* cfg, uint32_t what, sdsp_tempo_map* maps,
                             sdsp_debug_beat_out* beats, int32_t device);

/*
 * The tempo map step of the last sdsp_analyze_batch_device_with call with a tempo map request on
 * `device`, summed over its sub-batches: HIP event times of k_tempo_map (from k_beat's end to its
 * own) and of k_beat (the call's beat_ms), and the tracks mapped.  The events lie on the main
 * stream beside the key stream's work.  All zero after a call without a request.
 */
typedef struct sdsp_debug_tempo_map_times {
    double map_ms, beat_ms;
    uint64_t tracks;
} sdsp_debug_tempo_map_times;
int32_t sdsp_debug_last_tempo_map_times(int32_t device, sdsp_debug_tempo_map_times* out);

/*
 * Stage probe of the sections request (include/stratum_hip.h, sdsp_sections): the four kernels of
 * k_sections.hip over uploaded rows and energies, taken as the rows C and the energies E of the
 * definition.  host_chroma: the tracks' rows back to back, frames[t] rows of 12 floats for track t,
 * khop samples apart; host_energy: base_frames[t] energies for track t, hop samples apart (0 frames
 * allowed for either).  req is checked as an analysis call checks it against khop and hop.  Track t
 * has n_cells[t] = min(frames[t] khop, base_frames[t] hop) / Cs cells; with P the prefix of n_cells,
 * out->m receives m[c][0..12) at 12 (P[t] + c), out->g, out->novelty and out->boundary their values at
 * P[t] + c.  The caller sizes the arrays from the same plan; cell_capacity is their length in cells,
 * and a call that needs more is refused.  SDSP_ERR_INVALID_INPUT for a refused request.
 */
typedef struct sdsp_debug_sections_out {
    uint64_t cell_capacity;
    uint64_t* n_cells; /* n_tracks */
    float* m;          /* 12 x cell_capacity */
    float* g;
    float* novelty;
    uint8_t* boundary;
} sdsp_debug_sections_out;
int32_t sdsp_debug_sections(const float* host_chroma, const uint64_t* frames, const float* host_energy,
                            const uint64_t* base_frames, uint64_t n_tracks, uint32_t sample_rate, uint32_t khop,
                            uint32_t hop, const sdsp_sections_request* req, sdsp_debug_sections_out* out, int32_t device);

/*
 * The sections step of the last sdsp_analyze_batch_device_with call with a sections request on
 * `device`, summed over its sub-batches: HIP event times of k_section_energy (main stream),
 * k_section_chroma and k_section_novelty with k_section_pick (vote stream), and the cells folded.
 * All zero after a call without a request.
 */
typedef struct sdsp_debug_sections_times {
    double energy_ms, chroma_ms, novelty_ms;
    uint64_t cells;
} sdsp_debug_sections_times;
int32_t sdsp_debug_last_sections_times(int32_t device, sdsp_debug_sections_times* out);

/*
 * The programme loudness kernels of the last sdsp_analyze_batch_device_with call with an r128 request
 * on `device`: HIP event times of k_r128_steps, k_r128_peak and k_r128_track (0 for one that did not
 * run), the tracks and the steps measured.  The events lie on the vote stream, so beside a running
 * analysis they include what the kernels shared the device with.  All zero after a call without a
 * request.
 */
typedef struct sdsp_debug_r128_times {
    double steps_ms, peak_ms, track_ms;
    uint64_t tracks, steps;
} sdsp_debug_r128_times;
int32_t sdsp_debug_last_r128_times(int32_t device, sdsp_debug_r128_times* out);

/*
 * Stage probes of the fingerprint request (include/stratum_hip.h, sdsp_fingerprint).
 *
 * sdsp_debug_fingerprint: k_fp_cells and k_fp_words over uploaded rows, taken as the rows C of the
 * definition.  host_chroma: the tracks' rows back to back, frames[t] rows of 12 floats for track t,
 * khop samples apart (0 frames allowed).  req is checked as an analysis call checks it against khop
 * (its `what` and match fields are not used).  Track t has n_cells[t] = frames[t] khop / Cs cells and
 * n_words[t] words; out->m receives m[c][0..12) at 12 (P[t] + c) with P the prefix of n_cells,
 * out->words word w at Q[t] + w with Q the prefix of n_words.  The caller sizes the arrays from the
 * same plan; a call that needs more than the capacities is refused.
 *
 * sdsp_debug_fingerprint_match: k_fp_match over uploaded word arrays, every track compared: track t's
 * n_words[t] words (>= 1 each) back to back in host_words.  rec receives n_tracks * n_tracks records,
 * the pair (a, b), a < b, at a * n_tracks + b, the others zero; eligible == 0 (and the rest 0) for a
 * pair without an eligible offset.  Only max_offset_words and min_overlap_words of the request are
 * used: the records are before the max_ber filter.
 */
typedef struct sdsp_debug_fingerprint_out {
    uint64_t cell_capacity, word_capacity;
    uint64_t* n_cells; /* n_tracks */
    uint64_t* n_words; /* n_tracks */
    float* m;          /* 12 x cell_capacity */
    uint32_t* words;   /* word_capacity */
} sdsp_debug_fingerprint_out;
int32_t sdsp_debug_fingerprint(const float* host_chroma, const uint64_t* frames, uint64_t n_tracks, uint32_t sample_rate,
                               uint32_t khop, const sdsp_fingerprint_request* req, sdsp_debug_fingerprint_out* out,
                               int32_t device);
typedef struct sdsp_debug_fingerprint_pair {
    int32_t offset_words;
    uint32_t eligible, bit_errors, positions; /* has, e, n */
} sdsp_debug_fingerprint_pair;
int32_t sdsp_debug_fingerprint_match(const uint32_t* host_words, const uint64_t* n_words, uint64_t n_tracks,
                                     const sdsp_fingerprint_request* req, sdsp_debug_fingerprint_pair* rec, int32_t device);

/*
 * The fingerprint kernels of the last sdsp_analyze_batch_device_with call with a fingerprint request
 * on `device`: HIP event times of k_fp_cells and k_fp_words summed over the sub-batches (vote
 * stream, so beside a running analysis they include what the kernels shared the device with) and of
 * k_fp_match summed over its row bands (main stream, after the last join), the words written, the
 * tracks compared and the pairs.  All zero after a call without a request.
 */
typedef struct sdsp_debug_fingerprint_times {
    double cells_ms, words_ms, match_ms;
    uint64_t words, compared, pairs;
} sdsp_debug_fingerprint_times;
int32_t sdsp_debug_last_fingerprint_times(int32_t device, sdsp_debug_fingerprint_times* out);

/*
 * Stage probe of the candidate selection: the pipeline's own select launch (k_tempo_select with the
 * parameters an analysis call derives from cfg: Pipeline::pass_select from its offset tables on) over
 * uploaded tempogram lists instead of a novelty curve.  Per track t and variant v (full, low, mid,
 * high, mel) a list of (bpm, value) pairs in the order the tempogram kernels write them (value
 * descending):
 *   fft   track t's five lists back to back, fft_n[t] pairs each (one count per track, as in the
 *         pipeline; 0 allowed, at most 1024): list (t, v) starts at pair 5 (fft_n[0] + ... +
 *         fft_n[t - 1]) + v fft_n[t]
 *   acf   NB pairs per list (one NB for the call, at most 512): list (t, v) at pair (5 t + v) NB
 * present[v] selects the variants (the lists of the others are not read; present[0] must be set),
 * active[t] = 0 marks a track without a novelty curve (its record comes back zero), top_n, cand_cap
 * (1 ... 1024) and gate are the pass's: the candidates kept, the rows of the candidate table, and
 * whether the ambiguity gate of the base pass is evaluated.  est receives n_tracks records as the
 * kernel wrote them; cand n_tracks x cand_cap x 4 floats (bpm, score, fft_norm, autocorr_norm), of
 * which the first est[t].n_cands rows of track t are written.  SDSP_ERR_INVALID_INPUT for a count or
 * capacity outside these ranges.  Allocates only buffers of its own, released before it returns.
 */
typedef struct sdsp_debug_tempo_est {
    float bpm, conf;
    int32_t agree, ok, n_cands, ambiguous, trap_low, trap_high;
} sdsp_debug_tempo_est;
int32_t sdsp_debug_tempo_select(const float* fft, const int32_t* fft_n, const float* acf, uint32_t NB,
                                const int32_t present[5], const int32_t* active, uint64_t n_tracks, int32_t top_n,
                                int32_t cand_cap, int32_t gate, uint32_t sample_rate, const sdsp_config* cfg,
                                sdsp_debug_tempo_est* est, float* cand, int32_t device);

/*
 * Stage probe of the multi-resolution fusion: the pipeline's own fusion launch (k_multires with
 * the parameters, count tables and list stride of an analysis call: the tail of Pipeline::escalate)
 * over uploaded candidate lists and hop-512 novelty curves instead of three tempo passes.  The call
 * has n_tracks tracks, of which the n_items listed in `items` (ascending track indices) are fused.
 *   c256, c1024  n_items x cap_aux x 4 floats (bpm, score, fft_norm, autocorr_norm per candidate),
 *                n256 / n1024 [n_items] the candidates of each list, -1 where that hop's tempogram
 *                failed
 *   c512, n512   the hop-512 lists: with own512 = 0 the base pass's, one per track (n_tracks rows of
 *                cap_base candidates); with own512 = 1 the escalation's own, one per item (n_items
 *                rows of max(cfg->tempogram_multi_res_top_k, 1) candidates); -1 as above
 *   nov512       the hop-512 novelty curves back to back, nov_n[r] values for row r, indexed like
 *                the hop-512 lists (by track or by item)
 *   base         the base pass's estimate of every track (the acceptance reads bpm, conf, agree,
 *                trap_low, trap_high)
 * out->mr and out->dbg receive one record per item: the multi-resolution estimate (ok = 0: a hop
 * failed or no hypothesis; its other fields and the item's dbg record are then zero) and what the
 * kernel decided (fold-down, fold-up and triplet-family switches with their values, the acceptance).
 * out->used, final_bpm, final_conf hold n_tracks values: the probe uploads the caller's contents
 * first and the kernel overwrites used for every item and the estimate of the accepted ones, so the
 * other tracks come back untouched.  SDSP_ERR_INVALID_INPUT for an item list that is not ascending
 * within [0, n_tracks), a capacity outside 1 ... 1024 (with own512, a top_k above 1024), a count above
 * its list's capacity, or a novelty row of 2^24 values or more.
 * Allocates only buffers of its own, released before it returns.
 */
typedef struct sdsp_debug_mr_dbg {
    int32_t fd, fu, tf;
    float fd_from, fd_to, fd_ratio;
    int32_t fd_a0, fd_a1;
    float fu_from, fu_to, fu_ratio;
    int32_t fu_a0, fu_a1;
    float tf_from, tf_to, tf_sup0, tf_sup1, tf_al0, tf_al1;
    int32_t tf_label;
    float rel;
    int32_t fam, forbid, better;
} sdsp_debug_mr_dbg;
typedef struct sdsp_debug_multires_in {
    const float *c256, *c512, *c1024;
    const int32_t *n256, *n512, *n1024;
    uint32_t cap_aux, cap_base;
    const float* nov512;
    const uint64_t* nov_n;
    const sdsp_debug_tempo_est* base;
    const int32_t* items;
    uint64_t n_items, n_tracks;
    int32_t own512;
} sdsp_debug_multires_in;
typedef struct sdsp_debug_multires_out {
    sdsp_debug_tempo_est* mr;
    sdsp_debug_mr_dbg* dbg;
    int32_t* used;
    float *final_bpm, *final_conf;
} sdsp_debug_multires_out;
int32_t sdsp_debug_multires(const sdsp_debug_multires_in* in, uint32_t sample_rate, const sdsp_config* cfg,
                            sdsp_debug_multires_out* out, int32_t device);

/*
 * Isolated STFT kernel timing: `reps` launches over n_tracks device-resident noise tracks of len
 * samples; mean launch time (HIP events on the launch stream) and algorithmic bytes per launch
 * (4 N_in + 4 F (nfft/2 + 1) per track).  stride 0 = the pipeline's row stride.
 */
int32_t sdsp_probe_stft(int32_t device, uint64_t nfft, uint64_t hop, uint64_t n_tracks, uint64_t len, int32_t reps,
                        int32_t stride, double* ms_per_launch, double* bytes_per_launch);

/*
 * The device FLAC decoder's four phases on the CPU, through the same frame-level code
 * (csrc/flac_core.hpp): frame_header at every byte offset of the frame region, a frame decode of
 * every candidate into its own scratch slot, the chain over the sorted candidates, the gather of the
 * accepted slots.  Status, text and samples equal sdsp_decode_audio_file's for the same bytes in a
 * file; *samples is malloc'ed (sdsp_free_samples).  counts (NULL allowed) receives candidates,
 * accepted and rejected frames.  No device is touched.
 */
int32_t sdsp_debug_flac_decode_phased(const uint8_t* data, uint64_t n, float** samples, uint64_t* n_samples,
                                      uint32_t* sample_rate, uint64_t counts[3], char* err, uint64_t errlen);

/*
 * The device ALAC decoder's phases on the CPU, through the same packet-level code
 * (csrc/alac_core.hpp): the host plan (cookie and packet table of the CAF or ISO MP4 container), a
 * decode of every packet into its own slot with its sample count, the walk of the counts into
 * offsets, the gather of the decoded slots.  Status, text and samples equal
 * sdsp_decode_audio_file's for the same bytes in a file; *samples is malloc'ed
 * (sdsp_free_samples).  counts (NULL allowed) receives packets, decoded and skipped packets.
 * SDSP_ERR_NOT_IMPLEMENTED ("not planned: ...") for bytes that are no ALAC container.  No device
 * is touched.
 */
int32_t sdsp_debug_alac_decode_phased(const uint8_t* data, uint64_t n, float** samples, uint64_t* n_samples,
                                      uint32_t* sample_rate, uint64_t counts[3], char* err, uint64_t errlen);

/*
 * The device Vorbis decoder's phases on the CPU, through the code the kernels run
 * (csrc/vorbis_core.hpp) and with their buffer layouts (csrc/vorbis_phased.hpp): the host plan (Ogg
 * pages, the identification and setup headers, every audio packet's first bits), every kept
 * packet's spectra, every (packet, channel) windowed block, every output sample from its packet
 * pair.  Status, text and samples equal sdsp_decode_audio_file's for the same bytes in a file;
 * *samples is malloc'ed (sdsp_free_samples).  info (NULL allowed) receives the kept packets and
 * those a failed floor decode silenced.  SDSP_ERR_NOT_IMPLEMENTED ("not planned: ...") for bytes
 * that are no Ogg Vorbis stream.  No device is touched.
 */
int32_t sdsp_debug_vorbis_decode_phased(const uint8_t* data, uint64_t n, float** samples, uint64_t* n_samples,
                                        uint32_t* sample_rate, uint64_t info[2], char* err, uint64_t errlen);

/*
 * The device PCM path's steps on the CPU: the host plan of a RIFF/WAVE or AIFF / AIFF-C file, then
 * csrc/pcm_core.hpp over the planned frames.  info (NULL allowed) receives the plan: sample kind
 * (0 u8, 1 s16, 2 s24, 3 s32, 4 f32, 5 f64) | big-endian << 8, channels, data offset, frames.
 * SDSP_ERR_NOT_IMPLEMENTED ("not planned: ...") for a file that is not linear PCM (G.711, ADPCM,
 * another container: the batch decoder's host fallback); SDSP_ERR_DECODING with the host decoder's
 * text for a file it refuses.  No device is touched.
 */
int32_t sdsp_debug_pcm_decode_planned(const uint8_t* data, uint64_t n, float** samples, uint64_t* n_samples,
                                      uint32_t* sample_rate, uint64_t info[4], char* err, uint64_t errlen);

#ifdef __cplusplus
}
#endif

#endif /* STRATUM_HIP_DEBUG_H */
