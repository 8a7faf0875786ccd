// oracle_internal.hpp — CPU restatement of stratum-dsp's default analyze_audio() path.
//
// TEST INFRASTRUCTURE ONLY.  This code is the parity checker for the HIP engine in
// stratum-dsp_amd/ and the "port" CPU baseline in bench.py.  Nothing in the product links
// or calls it; only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg do.
//
// Every function follows the reference file:line it cites (paths under /root/reference).
// Arithmetic is f32 in the reference's order (sequential folds, no FMA: -ffp-contract=off);
// transcendentals go through include/sdsp_libm.h and FFTs through include/sdsp_fft_spec.h.
// Parity pinning: see oracle/README.md (integration-test ranges + known-answer tests of the
// reference's own test-suite; the FFT/libm layers are pinned to numpy / correctly rounded
// double references because the reference's rustfft/libm rounding is itself unpinned).
#pragma once

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../include/sdsp_fft_spec.h"
#include "../include/sdsp_libm.h"
#include "../include/stratum_hip.h"

namespace orc {

constexpr float EPS = 1e-10f;  // `const EPSILON: f32 = 1e-10` (every module)

// AnalysisError propagated with `?`  (src/error.rs:7-22)
struct AErr {
    int code;
    std::string msg;
};
[[noreturn]] inline void fail(int code, const std::string& m) { throw AErr{code, m}; }

struct Cx {
    float re, im;
};

// Vec<Vec<f32>> spectrogram, flat row-major [frame][bin]
struct Spec {
    size_t frames = 0, bins = 0;
    std::vector<float> d;
    float* row(size_t t) { return d.data() + t * bins; }
    const float* row(size_t t) const { return d.data() + t * bins; }
    bool empty() const { return frames == 0; }
};

// ---------- FFT (sdsp_fft_spec.h) ----------
void fft_complex(std::vector<Cx>& x);                          // in place, forward
void rfft(const float* x, size_t n, std::vector<Cx>& out);    // out: n/2+1 bins
Spec compute_stft(const float* s, size_t n, size_t frame_size, size_t hop);  // extractor.rs:301

// ---------- BPM estimate types (src/features/period/mod.rs) ----------
struct BpmCandidate {
    float bpm, confidence;
};
struct BpmEstimate {
    float bpm, confidence;
    uint32_t method_agreement;
};
struct TempoCand {  // TempogramCandidateDebug, tempogram.rs:47-54
    float bpm, score, fft_norm, autocorr_norm;
    bool selected;
};

// ---------- preprocessing + onsets ----------
void normalize_peak(std::vector<float>& x, float headroom_db);
void normalize_rms(std::vector<float>& x, float target_lufs, float headroom_db);
void normalize_lufs(std::vector<float>& x, uint32_t sr, float target_lufs, float headroom_db);
void detect_and_trim(const std::vector<float>& x, uint32_t sr, float threshold_db, uint32_t min_ms,
                     size_t frame_size, size_t* trim_start, size_t* trim_end,
                     std::vector<std::pair<size_t, size_t>>* silence_map = nullptr);
std::vector<size_t> energy_flux_onsets(const float* s, size_t n, size_t frame, size_t hop, float thr_db);
// its tail over the frame RMS, and detect_hpss_onsets' over the percussive frame energies
std::vector<size_t> energy_onsets_from_rms(const std::vector<float>& e, size_t hop, size_t n, float thr_db);
std::vector<size_t> hpss_onsets_from_energy(const std::vector<float>& e, float pct);
std::vector<float> spectral_flux_curve(const Spec& m);  // the flux spectral_flux_onsets thresholds (frames >= 2)
std::vector<size_t> spectral_flux_onsets(const Spec& m, float pct);
std::vector<size_t> hfc_onsets(const Spec& m, uint32_t sr, float pct);
struct OnsetCand {
    size_t time_samples;
    float time_seconds, confidence;
    uint32_t voted_by;
};
void hpss_decompose(const Spec& m, size_t margin, Spec* H, Spec* P);  // hpss.rs:71-172
std::vector<size_t> hpss_onsets(const Spec& p, float pct);            // hpss.rs:290-372
std::vector<OnsetCand> vote_onsets(const std::vector<size_t> lists[4], const float w[4], uint32_t tol_ms,
                                   uint32_t sr);

// ---------- legacy BPM (period/mod.rs, autocorrelation.rs, comb_filter.rs, candidate_filter.rs) ----------
struct Guardrails {
    float preferred_min, preferred_max, soft_min, soft_max, mul_preferred, mul_soft, mul_extreme;
};
bool estimate_bpm_legacy(const std::vector<size_t>& onsets, uint32_t sr, size_t hop, float min_bpm,
                         float max_bpm, float res, const Guardrails* g, BpmEstimate* out);

// ---------- tempogram (novelty.rs, tempogram*.rs, multi_resolution.rs) ----------
struct BandCfg {
    bool enabled;
    float low_max_hz, mid_max_hz, high_max_hz, w_full, w_low, w_mid, w_high;
    bool seed_only;
    float support_threshold, consensus_bonus;
    bool enable_mel;
    size_t mel_n_mels;
    float mel_fmin_hz, mel_fmax_hz;
    size_t mel_max_filter_bins;
    float w_mel, nw_spectral, nw_energy, nw_hfc;
    size_t local_mean_window, smooth_window, superflux_k;
};
std::vector<float> combined_full_novelty(const Spec& m, uint32_t sr, const BandCfg& c);
// AnalysisConfig -> the BandCfg analyze passes (src/lib.rs:337-377), and whether it passes one
BandCfg band_cfg_of(const sdsp_config& c);
bool band_cfg_used(const sdsp_config& c);
// Stage export (test probes): what tempogram_impl computed one seeded variant from.  Bands: bins
// [s, e); mel: e = n_mels, melf = the mel log-magnitudes (frames x n_mels), the curve in nov.
struct StageVariant {
    std::string name;
    size_t s = 0, e = 0;
    std::vector<float> energy, hfc, sfx_raw, sf, nov, melf;
    std::vector<std::pair<float, float>> fft, ac;
};
void tempogram_impl(const Spec& m, uint32_t sr, uint32_t hop, float min_bpm, float max_bpm, float res,
                    const BandCfg* band, BpmEstimate* est, std::vector<TempoCand>* cands,
                    std::vector<StageVariant>* dump = nullptr);
// tempogram_impl from its seeded variants on (tempogram.rs:501-775): candidate seeding and dedupe,
// weighted lookup scoring, the consensus bonus, the octave fold.  seeds[0] is the full variant.
using Tg = std::vector<std::pair<float, float>>;  // (bpm, value), sorted by value desc
struct SelVariant {
    std::string name;
    float w;
    Tg fft, ac;
};
struct SelBranch {  // what tempo_select did (test probes)
    int n_in = 0, n_out = 0;        // seed images inside / outside [min_bpm, max_bpm]
    int n_dup = 0, n_uniq = 0;      // images dropped by the 0.75 dedupe; candidates scored
    int n_pen_hi = 0, n_pen_lo = 0; // candidates above 180 / below 60
    int sb_hist[5] = {0, 0, 0, 0, 0};  // candidates by supporting variants (the last bin: 4 or more)
    int fold = 0;  // 0 best <= 180, 1 folded value out of range, 2 no candidate at it, 3 kept out by both ratios, 4 taken
    float fft_pb = 0.0f, ac_pb = 0.0f;
    // scoring lookups that passed over an equidistant entry of another value (the first wins), and
    // whose entry lies exactly at the tolerance; FFT lists, then autocorrelation lists
    int n_tie = 0, n_at_tol = 0, n_tie_ac = 0, n_at_tol_ac = 0;
};
void tempo_select(const std::vector<SelVariant>& seeds, float min_bpm, float max_bpm, float res, const BandCfg* band,
                  BpmEstimate* est, std::vector<TempoCand>* cands, SelBranch* br = nullptr);
// the ambiguity gate over the base estimate and its truncated candidates (src/lib.rs:412-459)
struct GateFlags {
    bool trap_low, trap_high, family, fold_into_trap, weak, ambiguous;
    float s_base, s_2x, s_half;
};
GateFlags ambiguity_gate(const BpmEstimate& base, const std::vector<TempoCand>& base_c, float res);
void multi_resolution(const std::vector<float>& samples, uint32_t sr, size_t frame_size, float min_bpm,
                      float max_bpm, float res, size_t top_k, float w512, float w256, float w1024,
                      float structural_discount, float dt512, float margin_threshold, bool human_prior,
                      const BandCfg* band, BpmEstimate* est, std::vector<TempoCand>* c512);
// multi_resolution from its hypothesis loop on (multi_resolution.rs:272-901) over the three hops'
// truncated candidate lists; nov512: the hop-512 novelty of the fold gates, null without a BandCfg.
// Marks c512's `selected`.
struct MrBranch {  // what multires_fuse did (test probes; the fields k_multires' MrDbg mirrors, and counters)
    int fd = 0, fu = 0, tf = 0;
    float fd_from = 0, fd_to = 0, fd_ratio = 0;
    int fd_a0 = 0, fd_a1 = 0;
    float fu_from = 0, fu_to = 0, fu_ratio = 0;
    int fu_a0 = 0, fu_a1 = 0;
    float tf_from = 0, tf_to = 0, tf_sup0 = 0, tf_sup1 = 0, tf_al0 = 0, tf_al1 = 0;
    int tf_label = 0;
    // fold gates evaluated: 0 not reached, else 1 + 4 (agreement ok) + 2 (supports > 0) + 1 (ratio ok)
    int fd_eval = 0, fu_eval = 0;
    float fd_eval_ratio = 0, fu_eval_ratio = 0;
    int fd_eval_a1 = 0, fu_eval_a1 = 0;
    int n_hyps = 0, n_uniq = 0, n_dup = 0;  // hypotheses before the dedupe, kept, dropped as duplicates
    int n_h102 = 0, n_2t102 = 0, n_r2_110 = 0, n_r2_100 = 0, n_rh_110 = 0, n_rh_100 = 0;  // structural discounts taken
    int n_pen210 = 0, n_pen180 = 0, n_pen60 = 0;  // band penalties taken
    int n_reset = 0, n_prior = 0, n_margin_lo = 0;  // margin below the threshold; the anchor reset; the human prior
    int n_fam = 0;  // family members considered
    float fam_bpm[5] = {0}, fam_sup[5] = {0}, fam_align[5] = {0};
    int fam_eval = 0;  // max_alt >= 0.45: a member was chosen
    float max_alt = 0, cur_align = 0;
    int chosen = -1;   // index of the chosen member
    int cur_phase = -1, fam_phase[5] = {-1, -1, -1, -1, -1};  // the first phase that gives each alignment
};
struct MrFuseCfg {
    float min_bpm, max_bpm, res;
    size_t top_k;
    float w512, w256, w1024, dt, margin_thr;
    bool human_prior;
};
void multires_fuse(const std::vector<TempoCand>& c256, std::vector<TempoCand>& c512, const std::vector<TempoCand>& c1024,
                   const std::vector<float>* nov512, uint32_t sr, const MrFuseCfg& f, BpmEstimate* est,
                   MrBranch* br = nullptr);
// the acceptance of the multi-resolution estimate (src/lib.rs:515-545)
struct MrAccept {
    float rel;
    bool fam, forbid, better;
    int clause;  // bits: 1 confidence, 2 agreement, 4 trap-zone family
};
MrAccept mr_accept(const BpmEstimate& base, bool trap_low, bool trap_high, const BpmEstimate& mr);

// ---------- beat grid (beat_tracking/) ----------
struct BeatDiag {            // which branches generate_beat_grid took (test probes)
    bool variable = false;   // detect_tempo_variations flagged a variable segment (mod.rs:152-154)
    bool refined = false;    // the Bayesian / per-segment HMM beats replaced the HMM beats (:205-219)
    uint32_t beats_per_bar = 4;
    uint32_t hmm_beats = 0;  // beats of the whole-track HMM (before any refinement)
};
bool generate_beat_grid(float bpm, float conf, const std::vector<float>& onsets_s, uint32_t sr,
                        std::vector<float>* beats, std::vector<float>* downbeats, float* stability,
                        BeatDiag* diag = nullptr);

// ---------- key (chroma/, key/) ----------
void harmonic_mask_inplace(Spec& s, size_t margin, float power);
// the key spectrogram conditioning analyze applies (src/lib.rs:1011-1060)
void key_condition_inplace(Spec& ks, const sdsp_config& c, uint32_t sr, size_t kfft);
void hpcp_frames(const Spec& s, uint32_t sr, size_t fft_size, float sigma, size_t peaks, size_t harmonics,
                 float decay, float mag_power, std::vector<float>* chroma12, std::vector<float>* energies);
void smooth_chroma_inplace(std::vector<float>& ch, size_t frames, size_t window);
// opt-in chroma front-ends (o_chroma.cpp)
struct HpcpCfg {
    float sigma = 0.5f, tuning = 0.0f;
    size_t peaks = 24, harmonics = 4;
    float decay = 0.6f, mag_power = 0.5f;
    bool whitening = false;
    size_t whitening_bins = 31;
    bool bass_blend = false;
    float bass_fmin = 55.0f, bass_fmax = 300.0f, bass_weight = 0.35f;
};
float estimate_tuning(const Spec& s, uint32_t sr, size_t fft_size, float fmin_hz, float fmax_hz, size_t frame_step,
                      float peak_rel_threshold);
void chroma_frames(const Spec& s, uint32_t sr, size_t fft_size, bool soft, float sigma, float tuning,
                   std::vector<float>* chroma12, std::vector<float>* energies);
void hpcp_frames_x(const Spec& s, uint32_t sr, size_t fft_size, const HpcpCfg& c, std::vector<float>* chroma12,
                   std::vector<float>* energies);
bool log_freq_chroma(const Spec& s, uint32_t sr, size_t fft_size, std::vector<float>* chroma12,
                     std::vector<float>* energies);
void beat_sync_chroma(const Spec& s, uint32_t sr, size_t fft_size, size_t hop, const std::vector<float>& beats,
                      bool soft, float sigma, float tuning, std::vector<float>* chroma12, std::vector<float>* energies);
void smooth_time_inplace(Spec& s, size_t margin);
void key_hpss_mask_inplace(Spec& s, uint32_t sr, size_t fft_size, float fmin_hz, float fmax_hz, size_t frame_step,
                           size_t time_margin, size_t freq_margin, float mask_power);

struct KeyResult {
    int mode;
    uint32_t tonic;
    float confidence;
    float scores[24];
    int order[24];  // key index (mode*12+tonic) of scores[i]
};
void key_templates(float major[12][12], float minor[12][12], int template_set = 0);
KeyResult detect_key_weighted(const float* chroma, size_t frames, const float* weights,
                              const float maj[12][12], const float min[12][12]);
KeyResult key_from_raw(const float raw[24]);  // detect_key_weighted after its 24 weighted template sums
float key_clarity(const float* sorted_scores, int n);
void sharpen_chroma_inplace(float* ch12, float power);
struct ModeHeuristic {
    bool on = false;  // enable_key_mode_heuristic || enable_key_minor_harmonic_bonus
    float third_margin = 0.0f, flip_ratio = 0.0f, bonus_w = 0.0f;
    bool bonus = false;
};
KeyResult detect_key_weighted_mode_heuristic(const float* chroma, size_t frames, const float* weights,
                                             const float maj[12][12], const float min[12][12],
                                             const ModeHeuristic& mh);
KeyResult detect_key_ensemble(const float* chroma, size_t frames, const float* weights, float kk_weight,
                              float temperley_weight);
// detect_key_multi_scale; returns false when no segment qualified (the caller falls back)
bool detect_key_multi_scale(const float* chroma, size_t frames, const float* weights, const float maj[12][12],
                            const float min[12][12], const std::vector<size_t>& lengths, size_t hop, float min_clarity,
                            const std::vector<float>* scale_weights, const ModeHeuristic& mh, KeyResult* out,
                            int* used_segments, int* n_segments = nullptr);  // n_segments: those evaluated

// The key decision analyze makes from its chroma front-end's output (src/lib.rs:1200-1470): chroma
// sharpening, median smoothing, edge trim, frame weights, then the ensemble / multi-scale /
// segment-voting / full-slice branch the configuration selects.  chroma: raw rows (frames x 12),
// energies: one per frame.  err: the reference's Err path (all-zero key fields).
struct KeyVote {
    bool err = false;
    int mode = 0;
    uint32_t tonic = 0;
    float conf = 0.0f, clarity = 0.0f;
    int used_segments = 0;
    int n_segments = 0;  // segments evaluated (multi-scale or segment voting)
    bool weights_used = false;
    size_t t0 = 0, frames = 0;   // the voted slice [t0, t0 + frames) of the rows (the edge trim's)
    std::vector<float> chroma;   // sharpened and smoothed, every row
    std::vector<float> weights;  // over the slice; empty without frame weighting
    float scores[24] = {0};      // the final table, descending ...
    int order[24] = {0};         // ... and the key index of each entry
};
void key_vote(std::vector<float> chroma, std::vector<float> energies, const sdsp_config& c, KeyVote* out);

// ---------- unit probes (o_*.cpp "unit probes" sections; tests/test_oracle_units_*.py) ----------
// Entry points at the granularity of the reference's own unit tests.  A probe returns a count /
// 0 on success or -(AnalysisError code) on error, with the message kept for
// sdsp_oracle_probe_error().
extern std::string g_probe_err;
// Study switches (tools/key_near_study.py; never set by the parity tests): g_block_energy folds
// each HPCP frame energy in 64-bin blocks the way the GPU's default key path does (k_mask_rp /
// k_hpcp_band) instead of the reference's one sequential sum; g_key_trace, when
// non-null, receives per detect_key_weighted call its 24 raw scores and, in segment voting and
// multi-scale detection, the segment's clarity after them (sdsp_oracle_key_vote returns it too).
extern int g_block_energy;
extern std::vector<float>* g_key_trace;
template <class F>
int64_t probe_call(F f) {
    try {
        return f();
    } catch (const AErr& e) {
        g_probe_err = e.msg;
        return -(int64_t)e.code;
    }
}
// Vec<Vec<f32>> from a flat row-major buffer; row_lens (nullable) lets a test pass a ragged
// spectrogram: the reference's validate loops reject frame lengths that differ from frame 0's
void spec_from_rows(const float* d, size_t frames, size_t bins, const uint64_t* row_lens, Spec* out);
std::vector<float> superflux_novelty(const Spec& m, size_t k);                    // novelty.rs:336-393
std::vector<float> energy_flux_novelty(const Spec& m);                            // novelty.rs:477-545
std::vector<float> hfc_novelty(const Spec& m, uint32_t sr);                       // novelty.rs:687-772
std::vector<float> spectral_flux_novelty(const Spec& m);                          // novelty.rs:222-334
std::vector<float> combined_novelty_params(const std::vector<float>& s, const std::vector<float>& e,
                                           const std::vector<float>& h, float ws, float we, float wh,
                                           size_t lmw, size_t smw);              // novelty.rs:874-932

// ---------- trace (test probes) ----------
struct Trace {
    size_t trim_start = 0, trim_end = 0;
    std::vector<size_t> energy_onsets, spectral_onsets, hfc_onsets, chosen_onsets;
    bool has_legacy = false;
    BpmEstimate legacy{0, 0, 0};
    bool has_tempogram = false;
    BpmEstimate base{0, 0, 0}, mr{0, 0, 0};
    bool ambiguous = false, used_mr = false, ran_mr = false;
    std::vector<TempoCand> base_cands;
    std::vector<float> novelty_full;
    std::vector<float> chroma;    // smoothed, frames*12
    std::vector<float> energies;  // per key frame
    std::vector<float> weights;
    bool weights_used = false;
    float tuning = 0.0f;
    int used_segments = 0;
    BeatDiag beat;
};

}  // namespace orc
