// pipeline_params.hip — configuration -> host tables and launch parameters for the pipeline's
// stages (pipeline.hpp declares them).  Pure functions of the configuration, the sample rate and
// plan integers: none takes a Pipeline, a device context or a stream.
#include "pipeline.hpp"

namespace sdsp {
namespace detail {

constexpr int SUPPORT_HMAX = 8;


// MelFilterbank::new, novelty.rs:83-165
MelTable mel_table(uint32_t sr, int n_bins, int n_mels_in, float fmin_hz, float fmax_hz, std::string* err) {
    MelTable t;
    const int n_mels = std::max(n_mels_in, 4);
    t.n_mels = n_mels;
    const float nyq = (float)sr * 0.5f;
    const float fmin = sd_minf(sd_maxf(fmin_hz, 0.0f), sd_maxf(nyq, 1.0f));
    float fmax = fmax_hz;
    if (!(sd_isfinite_f(fmax) && fmax > 0.0f)) fmax = nyq;
    fmax = sd_clampf(fmax, fmin + 1.0f, nyq);
    const int fft_size = (n_bins - 1) * 2;
    const float fres = (float)sr / (float)fft_size;
    auto mel = [](float f) { return 2595.0f * sd_log10f(1.0f + (f / 700.0f)); };
    auto inv_mel = [](float v) { return 700.0f * (sd_powf(10.0f, v / 2595.0f) - 1.0f); };
    const float mmin = mel(fmin), mmax = mel(fmax);
    const float step = (mmax - mmin) / (float)(n_mels + 1);
    std::vector<int> bp((size_t)n_mels + 2);
    for (int i = 0; i < n_mels + 2; i++) {
        const float hz = inv_mel(mmin + step * (float)i);
        int64_t b = sd_f2i64(sd_roundf(hz / fres));
        b = std::max<int64_t>(0, std::min<int64_t>(b, n_bins - 1));
        bp[(size_t)i] = (int)b;
    }
    for (size_t i = 1; i < bp.size(); i++)
        if (bp[i] <= bp[i - 1]) bp[i] = std::min(bp[i - 1] + 1, n_bins - 1);
    t.m.assign((size_t)n_bins * 2, -1);
    t.w.assign((size_t)n_bins * 2, 0.0f);
    std::vector<int> cnt((size_t)n_bins, 0);
    auto push = [&](int b, int m, float w) {
        if (cnt[(size_t)b] >= 2) {
            *err = "mel filterbank: more than two contributions for one bin";
            return;
        }
        t.m[(size_t)b * 2 + cnt[(size_t)b]] = m;
        t.w[(size_t)b * 2 + cnt[(size_t)b]] = w;
        cnt[(size_t)b]++;
    };
    for (int mm = 0; mm < n_mels; mm++) {
        const int l = bp[(size_t)mm], c = bp[(size_t)mm + 1], r = bp[(size_t)mm + 2];
        if (!(l < c && c < r)) continue;
        for (int b = l; b <= c; b++) {
            const float w = b == l ? 0.0f : ((float)b - (float)l) / ((float)c - (float)l);
            if (w > 0.0f) push(b, mm, w);
        }
        for (int b = c; b <= r; b++) {
            const float w = b == r ? 0.0f : ((float)r - (float)b) / ((float)r - (float)c);
            if (w > 0.0f) push(b, mm, w);
        }
    }
    return t;
}

// Register-pair schedule for the mel sums (see k_features.hip): mels are flushed in index
// order; every contribution of a bin must land on the two live accumulators mA, mA+1.
std::vector<MelPlan> mel_plan(const MelTable& t, int n_bins, std::string* err) {
    std::vector<MelPlan> p((size_t)n_bins, MelPlan{0, 0, 0, 0.0f, 0.0f});
    int mA = 0;
    for (int b = 0; b < n_bins; b++) {
        int mx = -1;
        for (int s = 0; s < 2; s++) mx = std::max(mx, t.m[(size_t)b * 2 + s]);
        if (mx < 0) continue;
        const int nf = std::max(0, mx - (mA + 1));
        MelPlan& q = p[(size_t)b];
        q.nflush = nf;
        mA += nf;
        for (int s = 0; s < 2; s++) {
            const int m = t.m[(size_t)b * 2 + s];
            if (m < 0) continue;
            if (m != mA && m != mA + 1) *err = "mel filterbank: contributions not on adjacent mels";
            (s == 0 ? q.s0 : q.s1) = m - mA;
            (s == 0 ? q.w0 : q.w1) = t.w[(size_t)b * 2 + s];
        }
    }
    return p;
}

// hz_to_bin, tempogram.rs:279-289
int hz_to_bin(float f, float fres, int n_bins) {
    if (!sd_isfinite_f(f) || f <= 0.0f || !sd_isfinite_f(fres) || fres <= 0.0f) return 0;
    int64_t b = sd_f2i64(sd_roundf(f / fres));
    return (int)std::max<int64_t>(0, std::min<int64_t>(b, (int64_t)n_bins - 1));
}

// compiler-rt __powisf2 (Rust f32::powi)
float powi_f(float a, int b) {
    const bool recip = b < 0;
    float r = 1.0f;
    while (true) {
        if (b & 1) r *= a;
        b /= 2;
        if (b == 0) break;
        a *= a;
    }
    return recip ? 1.0f / r : r;
}

// per-(bin, harmonic) HPCP decisions, extractor.rs:636-668 (tuning 0)
std::vector<HarmEntry> harm_table(int B, uint32_t sr, int fft_size, float sigma_in, int hmax, float decay_in) {
    std::vector<HarmEntry> t((size_t)B * HP_HMAX);
    const float fres = (float)sr / (float)fft_size;
    const float fmin = sd_maxf(100.0f, 20.0f), fmax = sd_minf(5000.0f, (float)sr / 2.0f);
    const float sigma = sd_maxf(sigma_in, 1e-6f);
    const float decay = sd_clampf(decay_in, 0.0f, 1.0f);
    for (int bin = 0; bin < B; bin++) {
        const float f0 = (float)bin * fres;
        for (int h = 1; h <= HP_HMAX; h++) {
            HarmEntry& e = t[(size_t)bin * HP_HMAX + (size_t)(h - 1)];
            e = HarmEntry{};
            const float fh = f0 * (float)h;
            if (h > hmax || fh > fmax) {
                e.state = 0;
                continue;
            }
            if (fh < fmin) {
                e.state = 1;
                continue;
            }
            e.state = 2;
            const float semitone = 12.0f * sd_log2f(fh / 440.0f) + 57.0f - 0.0f;
            const float spc = sd_rem_euclid_f(semitone, 12.0f);
            const float ppc = sd_rem_euclid_f(sd_roundf(spc), 12.0f);
            const int primary = sd_f2i32(ppc);
            e.hw = powi_f(decay, h - 1) / (float)h;
            for (int o = -1; o <= 1; o++) {
                const int tc = (((primary + o) % 12) + 12) % 12;
                float dist = sd_absf(spc - (float)tc);
                dist = sd_minf(dist, 12.0f - dist);
                e.tc[o + 1] = tc;
                e.wt[o + 1] = sd_expf(-dist * dist / (2.0f * sigma * sigma));
            }
        }
    }
    return t;
}

// Contiguous candidate bins of a band, as the reference's peak loops visit them:
// `for bin in 1..len-1 { if f < fmin continue; if f > fmax break; ... }` (extractor.rs:599-617).
// Leaves *lo > *hi when the band is empty.
void band_bins(int B, float fres, float fmin, float fmax, int* lo, int* hi) {
    *lo = 1;
    *hi = 0;
    if (!(fmax > fmin)) return;
    int l = -1, h = -1;
    for (int b = 1; b + 1 < B; b++) {
        const float f = (float)b * fres;
        if (f < fmin) continue;
        if (f > fmax) break;
        if (l < 0) l = b;
        h = b;
    }
    if (l >= 0) *lo = l, *hi = h;
}

// HPCP's peak band of the key spectrogram (bins pk_lo .. pk_hi; empty when lo > hi), and whether a
// configuration takes the default key path's band-limited mask with block-folded frame energies
// (k_mask_rp / k_hpcp_band): the harmonic mask at margin 12 and power 2, plain HPCP,
// nothing else reading the masked spectrogram.  SDSP_KEY_EXACT_ENERGY builds never take it.
void key_peak_band(const sdsp_config& c, uint32_t sr, int* lo, int* hi) {
    const int kfs = (int)std::min<uint64_t>(key_fft(c), STFT_GEN_MAX);
    band_bins(kfs / 2 + 1, (float)sr / (float)kfs, sd_maxf(100.0f, 20.0f), sd_minf(5000.0f, (float)sr / 2.0f), lo, hi);
}
bool key_energy_blocked(const sdsp_config& c, uint32_t sr) {
#ifdef SDSP_KEY_EXACT_ENERGY
    return false;
#else
    const bool use_log = c.enable_key_log_frequency;
    const bool tuned = c.enable_key_tuning_compensation && !use_log;
    const bool whiten = c.enable_key_hpcp_whitening && c.key_hpcp_whitening_smooth_bins >= 3;
    const bool plain_hpcp = !use_log && c.enable_key_hpcp && !tuned && !whiten && !c.enable_key_hpcp_bass_blend;
    int lo = 1, hi = 0;
    key_peak_band(c, sr, &lo, &hi);
    // the scoring whose energy-dependent decisions k_key_vote certifies (KeyParams::near_check):
    // segment voting or the full slice, without the mode heuristic, ensemble or multi-scale voting
    const bool plain_scoring = !c.enable_key_mode_heuristic && !c.enable_key_minor_harmonic_bonus &&
                               !c.enable_key_ensemble && !(c.enable_key_multi_scale && c.key_multi_scale_lengths_len > 0);
    return plain_hpcp && plain_scoring && !c.enable_key_hpss_harmonic && c.enable_key_harmonic_mask &&
           mask_band_ok((int)c.key_spectrogram_smooth_margin, c.key_harmonic_mask_power) &&
           !(c.enable_key_beat_synchronous && !c.enable_key_log_frequency) && lo <= hi;
#endif
}

// estimate_tuning_offset_semitones_from_spectrogram over [80, 2000] Hz (src/lib.rs:1101-1109,
// extractor.rs:98-140): the band is every bin with fmin <= f <= fmax
TuningParams tuning_params(const sdsp_config& c, uint32_t sr, int B, float fres, int stride) {
    TuningParams t{};
    t.stride = stride;
    const float fmin = sd_maxf(80.0f, 20.0f);
    const float fmax = sd_clampf(2000.0f, fmin + 1.0f, (float)sr / 2.0f);
    t.lo = 1;
    t.hi = 0;
    for (int b = 0; b < B; b++) {
        const float f = (float)b * fres;
        if (f < fmin) continue;
        if (f > fmax) break;
        if (t.lo > t.hi) t.lo = b;
        t.hi = b;
    }
    t.step = (int)std::min<uint64_t>(std::max<uint64_t>(c.key_tuning_frame_step, 1), INT32_MAX);
    const int tb = t.hi - t.lo + 1;
    t.chf = tb > 0 ? std::max(1, std::min(8, 4096 / tb)) : 1;
    t.fres = fres;
    t.thr = sd_clampf(c.key_tuning_peak_rel_threshold, 0.0f, 1.0f);
    t.lim = sd_absf(c.key_tuning_max_abs_semitones);
    return t;
}

// k_chroma parameters: mode 0 frame_to_chroma_tuned (extractor.rs:393-481), mode 1 the
// log-frequency conversion (extractor.rs:701-828, fmin 100, fmax 5000 from src/lib.rs:1068-1073)
ChromaParams chroma_params(const sdsp_config& c, uint32_t sr, int mode, int B, float fres, int stride) {
    ChromaParams p{};
    p.B = B;
    p.stride = stride;
    p.fres = fres;
    p.soft = c.soft_chroma_mapping ? 1 : 0;
    p.sigma = c.soft_mapping_sigma;
    p.gate_small = 1;
    p.lo = 1;
    p.hi = 0;
    const float nyq = (float)sr / 2.0f;
    if (mode == 0) {
        const float top = sd_minf(5000.0f, nyq);
        for (int b = 0; b < B; b++) {
            const float f = (float)b * fres;
            if (f < 100.0f) continue;
            if (f > top || f >= nyq) break;
            if (p.lo > p.hi) p.lo = b;
            p.hi = b;
        }
    } else {
        const float fmin = sd_maxf(100.0f, 20.0f), fmax = sd_minf(5000.0f, nyq - 1.0f);
        const float smin = 12.0f * sd_log2f(fmin / 440.0f) + 57.0f;
        const float smax = 12.0f * sd_log2f(fmax / 440.0f) + 57.0f;
        p.bmin = sd_f2i32(__builtin_floorf(smin));
        p.n_log = sd_f2i32(__builtin_ceilf(smax)) - p.bmin + 1;
        p.log_off = sd_f2i32(__builtin_floorf(12.0f * sd_log2f(100.0f / 440.0f) + 57.0f));
        for (int b = 0; b < B; b++) {
            const float f = (float)b * fres;
            if (f < fmin || f >= fmax || f >= nyq) continue;
            if (p.lo > p.hi) p.lo = b;
            p.hi = b;
        }
    }
    return p;
}

// k_hpcp_x parameters (extractor.rs:529-680 with whitening, :1154-1244 bass blend)
HpcpXParams hpcp_x_params(const sdsp_config& c, uint32_t sr, int B, float fres, bool whiten, int stride) {
    HpcpXParams h{};
    h.B = B;
    h.stride = stride;
    h.fres = fres;
    h.fmin = sd_maxf(100.0f, 20.0f);
    h.fmax = sd_minf(5000.0f, (float)sr / 2.0f);
    h.main_ok = h.fmax > h.fmin;
    band_bins(B, fres, h.fmin, h.fmax, &h.pk_lo, &h.pk_hi);
    h.K = (int)std::max<uint64_t>(c.key_hpcp_peaks_per_frame, 1);
    h.hmax = (int)std::max<uint64_t>(c.key_hpcp_num_harmonics, 1);
    h.p = sd_clampf(c.key_hpcp_mag_power, 0.05f, 1.0f);
    h.decay = sd_clampf(c.key_hpcp_harmonic_decay, 0.0f, 1.0f);
    h.sigma = c.soft_mapping_sigma;
    h.bass = c.enable_key_hpcp_bass_blend ? 1 : 0;
    h.bk_lo = 1;
    h.bk_hi = 0;
    if (h.bass) {
        h.bfmin = sd_maxf(c.key_hpcp_bass_fmin_hz, 20.0f);
        h.bfmax = sd_minf(c.key_hpcp_bass_fmax_hz, (float)sr / 2.0f);
        h.bass_ok = h.bfmax > h.bfmin;
        band_bins(B, fres, h.bfmin, h.bfmax, &h.bk_lo, &h.bk_hi);
        h.KB = (int)std::min<uint64_t>(std::max<uint64_t>(c.key_hpcp_peaks_per_frame, 1), 12);
        h.bw = sd_clampf(c.key_hpcp_bass_weight, 0.0f, 1.0f);
    }
    if (whiten) {
        const int win = (int)(std::max<uint64_t>(c.key_hpcp_whitening_smooth_bins, 3) | 1);
        h.half = win / 2;
        int rp = 1, rx = 1;
        while (rp < 2 * h.half + 2) rp <<= 1;
        while (rx < h.half + 1) rx <<= 1;
        h.rp = rp, h.rp_mask = rp - 1, h.rx = rx, h.rx_mask = rx - 1;
    }
    return h;
}

// harmonic_spectrogram_hpss_median_mask's band and windows (extractor.rs:1400-1420, with
// fmin 100 / fmax 5000 from src/lib.rs:1014-1024); nb = 0 when the band is empty
KeyHpssParams key_hpss_params(const sdsp_config& c, uint32_t sr, int B, float fres, int stride) {
    KeyHpssParams k{};
    k.B = B;
    k.stride = stride;
    const float fmin = sd_maxf(100.0f, 20.0f);
    const float fmax = sd_clampf(5000.0f, fmin + 1.0f, (float)sr / 2.0f);
    int64_t bs = sd_f2i64(__builtin_floorf(fmin / fres)), be = sd_f2i64(__builtin_ceilf(fmax / fres));
    bs = std::min<int64_t>(std::max<int64_t>(bs, 0), B);
    be = std::min<int64_t>(std::max<int64_t>(be, 0), B);
    k.bin0 = (int)bs;
    k.nb = be > bs ? (int)(be - bs) : 0;
    k.step = (int)std::min<uint64_t>(std::max<uint64_t>(c.key_hpss_frame_step, 1), INT32_MAX);
    k.tm = (int)std::min<uint64_t>(c.key_hpss_time_margin, 1u << 20);
    k.fm = (int)std::min<uint64_t>(c.key_hpss_freq_margin, 1u << 20);
    k.p = sd_maxf(c.key_hpss_mask_power, 1.0f);
    return k;
}

// Configuration support that depends on the sample rate.
std::string unsupported_sr(const sdsp_config& c, uint32_t sr) {
    if (sr == 0) return "";
    const int kfs = (int)std::min<uint64_t>(key_fft(c), STFT_GEN_MAX);
    const int B8 = kfs / 2 + 1, ks = base_stride(kfs);
    const float fres = (float)sr / (float)kfs;
    if (c.enable_key_log_frequency) {
        const ChromaParams p = chroma_params(c, sr, 1, B8, fres, ks);
        if (p.n_log <= 0) return "degenerate key log-frequency range (sample rate too low)";
        if ((size_t)(p.hi - p.lo + 1) * sizeof(ChromaBin) > 65536) return "log-frequency chroma band > 3276 bins";
    } else if (c.enable_key_tuning_compensation) {
        const TuningParams t = tuning_params(c, sr, B8, fres, ks);
        if (t.hi - t.lo + 1 > 4096) return "tuning band > 4096 bins";
    }
    if (!c.enable_key_log_frequency && !c.enable_key_hpcp) {
        const ChromaParams p = chroma_params(c, sr, 0, B8, fres, ks);
        if ((size_t)(p.hi - p.lo + 1) * sizeof(ChromaBin) > 65536) return "chroma band > 3276 bins (sample rate too low)";
    }
    return "";
}

// templates.rs:64-145 (Krumhansl-Kessler) and :147-235 (Temperley): rows 0-23 K-K major/minor
// keys, rows 24-47 Temperley; each profile rotated to the key, then L2-normalised.
void key_templates(float* out /*48x12*/) {
    const float kM[12] = {6.35f, 2.23f, 3.48f, 2.33f, 4.38f, 4.09f, 2.52f, 5.19f, 2.39f, 3.66f, 2.29f, 2.88f};
    const float km[12] = {6.33f, 2.68f, 3.52f, 5.38f, 2.60f, 3.53f, 2.54f, 4.75f, 3.98f, 2.69f, 3.34f, 3.17f};
    const float tM[12] = {5.0f, 2.0f, 3.5f, 2.0f, 4.5f, 4.0f, 2.0f, 4.5f, 2.0f, 3.5f, 1.5f, 4.0f};
    const float tm[12] = {5.0f, 2.0f, 3.5f, 5.0f, 2.0f, 3.5f, 2.0f, 4.5f, 3.5f, 2.0f, 4.0f, 3.5f};
    for (int k = 0; k < 48; k++) {
        float* v = out + k * 12;
        const float* base = k < 24 ? (k < 12 ? kM : km) : (k < 36 ? tM : tm);
        const int key = k % 12;
        for (int s = 0; s < 12; s++) v[s] = base[(s + 12 - key) % 12];
        float sq = 0.0f;
        for (int i = 0; i < 12; i++) sq += v[i] * v[i];
        const float n = __builtin_sqrtf(sq);
        if (n > 1e-12f)
            for (int i = 0; i < 12; i++) v[i] /= n;
    }
}

// RMS / LUFS constants (normalization.rs:119-158, 183-259, 325-470; lib.rs:118-122 fixes
// target_loudness_lufs = -14 and max_headroom_db = 1).  The K-weighting coefficients use the C
// library's sinf/cosf, the functions f32::sin/cos lower to.
LoudnessParams loudness_params(int method, uint32_t sr) {
    LoudnessParams p{};
    p.method = method == SDSP_NORM_RMS ? 1 : 2;
    const float target_lufs = -14.0f, headroom = 1.0f;
    p.target_lufs = target_lufs;
    p.target_rms = sd_powf(10.0f, ((target_lufs + 3.0f) - headroom) / 20.0f);
    p.target_peak = sd_powf(10.0f, (0.0f - headroom) / 20.0f);
    p.gate = sd_powf(10.0f, (-70.0f + 0.691f) / 10.0f);
    const float fsr = (float)sr;
    p.block = (int64_t)sd_f2u64(fsr * 400.0f / 1000.0f);
    const float w0 = 2.0f * 3.14159274f * 1681.9745f / fsr;
    const float cw = cosf(w0), sw = sinf(w0);
    const float alpha = sw / 2.0f * sqrtf(1.0f / 0.707f);
    const float b0 = (1.0f + cw) / 2.0f, b1 = -(1.0f + cw), b2 = (1.0f + cw) / 2.0f;
    const float a0 = 1.0f + alpha, a1 = -2.0f * cw, a2 = 1.0f - alpha;
    p.b0 = b0 / a0;
    p.b1 = b1 / a0;
    p.b2 = b2 / a0;
    p.a1 = a1 / a0;
    p.a2 = a2 / a0;
    return p;
}

// autocorrelation_tempogram's BPM grid and lags for one hop (tempogram_autocorr.rs:128-140)
void acf_grid(uint32_t sr, int hop, float min_bpm, float max_bpm, float res, std::vector<float>* bpms,
              std::vector<int>* lags) {
    const float frame_rate = (float)sr / (float)hop;
    for (float bpm = min_bpm; bpm <= max_bpm; bpm += res) {
        const float bps = bpm / 60.0f;
        const float fpb = frame_rate / bps;
        bpms->push_back(bpm);
        lags->push_back((int)std::min<uint64_t>(sd_f2u64(fpb), (uint64_t)INT32_MAX));
    }
}

// in-range FFT-tempogram bins for size P (tempogram_fft.rs:158-175)
void fft_bins(uint32_t sr, int hop, uint64_t P, float min_bpm, float max_bpm, int* b_lo, int* K, float* fres_out) {
    const float frame_rate = (float)sr / (float)hop;
    const float fres = frame_rate / (float)P;
    *fres_out = fres;
    int lo = -1, hi = -2;
    for (uint64_t b = 0; b <= P / 2; b++) {
        const float bpm = (float)b * fres * 60.0f;
        if (bpm >= min_bpm && bpm <= max_bpm) {
            if (lo < 0) lo = (int)b;
            hi = (int)b;
        }
    }
    *b_lo = lo < 0 ? 0 : lo;
    *K = lo < 0 ? 0 : hi - lo + 1;
}

// Configuration support (everything the default path and its numeric knobs need).
std::string unsupported(const sdsp_config& c, uint32_t sr) {
    if (c.enable_normalization && c.normalization != SDSP_NORM_PEAK && c.normalization != SDSP_NORM_RMS &&
        c.normalization != SDSP_NORM_LOUDNESS)
        return "unknown normalization method";
    if (c.frame_size > (uint64_t)STFT_GEN_MAX || !stft_size_ok((int)c.frame_size))
        return "frame_size not a power of two in [64, 16384]";
    if (c.hop_size == 0 || c.hop_size > 8192) return "hop_size outside 1..8192";
    if ((c.enable_hpss_onsets || c.enable_tempogram_percussive_fallback) && c.hpss_margin > 16) return "hpss_margin > 16";
    if (!(c.min_bpm > 0.0f && c.max_bpm > c.min_bpm && c.bpm_resolution > 0.0f)) return "BPM range/resolution";
    if (c.force_legacy_bpm || c.enable_bpm_fusion) {  // k_legacy's fixed LDS lists
        int nc = 0;
        for (float b = c.min_bpm; b <= c.max_bpm + EPS && nc <= LG_COMB_MAX; b += c.bpm_resolution) nc++;
        if (nc > LG_COMB_MAX) return "legacy BPM: more than 2048 comb-filter candidates";
        const uint64_t hop = c.hop_size ? c.hop_size : 1;
        const float lmin = std::ceil((60.0f * (float)sr) / (c.max_bpm * (float)hop));
        const float lmax = std::floor((60.0f * (float)sr) / (c.min_bpm * (float)hop));
        if (lmax - lmin > (float)(2 * LG_AC_MAX - 4)) return "legacy BPM: autocorrelation lag range above 1020";
        if ((60.0f * (float)sr) / c.max_bpm < 1.0f) return "legacy BPM: period below one sample";
    }
    if (c.tempogram_superflux_max_filter_bins > (uint64_t)FT_KMAX) return "superflux_max_filter_bins > 8";
    if (c.enable_tempogram_mel_novelty && std::max<uint64_t>(c.tempogram_mel_n_mels, 4) > (uint64_t)FT_MELMAX)
        return "tempogram_mel_n_mels > 48";
    if (c.tempogram_mel_max_filter_bins > 16) return "tempogram_mel_max_filter_bins > 16";
    if (key_fft(c) > (uint64_t)STFT_GEN_MAX || !stft_size_ok((int)key_fft(c)))
        return "key STFT frame size not a power of two in [256, 16384]";
    if (c.enable_key_stft_override && c.key_stft_hop_size == 0) return "key_stft_hop_size 0";
    if (c.enable_key_hpss_harmonic && (c.key_hpss_time_margin > 16 || c.key_hpss_freq_margin > 16))
        return "key_hpss_time_margin / key_hpss_freq_margin > 16";
    if (c.key_spectrogram_smooth_margin > 31) return "key_spectrogram_smooth_margin > 31";
    if (c.enable_key_hpcp_whitening && c.key_hpcp_whitening_smooth_bins > 63) return "key_hpcp_whitening_smooth_bins > 63";
    if (c.key_hpcp_peaks_per_frame > (uint64_t)HP_KMAX) return "key_hpcp_peaks_per_frame > 32";
    if (c.key_hpcp_num_harmonics > (uint64_t)SUPPORT_HMAX) return "key_hpcp_num_harmonics > 8";
    if (c.enable_key_multi_scale && c.key_multi_scale_lengths_len > 8) return "more than 8 multi-scale key lengths";
    if (c.enable_ml_refinement) return "ML refinement";
    return "";
}
std::string check_supported(const sdsp_config& c, uint32_t sr) {
    const std::string why = unsupported(c, sr);
    return why.empty() ? unsupported_sr(c, sr) : why;
}

bool band_configured(const sdsp_config& c) {
    return c.enable_tempogram_band_fusion || c.enable_tempogram_mel_novelty || c.tempogram_band_consensus_bonus > 0.0f;
}

// k_features' bands (full, low, mid, high) and mel count for B bins; chunk_flags / mel_chunks are
// device tables the caller uploads (feat_chunk_tables)
FeatParams feat_params(const sdsp_config& c, uint32_t sr, int B, int stride) {
    FeatParams fp{};
    fp.B = B;
    fp.stride = stride;
    fp.K = (int)std::max<uint64_t>(c.tempogram_superflux_max_filter_bins, 1);
    const float fres = (float)sr / (float)((B - 1) * 2);
    const int b0 = std::min(1, B - 1);
    const int bl = std::max(hz_to_bin(c.tempogram_band_low_max_hz, fres, B), b0);
    const int bm = std::max(hz_to_bin(c.tempogram_band_mid_max_hz, fres, B), bl + 1);
    int bh = c.tempogram_band_high_max_hz > 0.0f ? std::max(hz_to_bin(c.tempogram_band_high_max_hz, fres, B), bm + 1) : B;
    bh = std::min(bh, B);
    const float wb[4] = {c.tempogram_band_w_full, c.tempogram_band_w_low, c.tempogram_band_w_mid, c.tempogram_band_w_high};
    const int bs_[4] = {0, b0, bl, bm}, be_[4] = {B, bl, bm, bh};
    const bool configured = band_configured(c);
    for (int v = 0; v < 4; v++) {
        fp.bs[v] = std::min(bs_[v], B);
        fp.be[v] = std::min(be_[v], B);
        if (v == 0)
            fp.band_on[v] = 1;
        else
            fp.band_on[v] = configured && c.enable_tempogram_band_fusion && sd_isfinite_f(wb[v]) && wb[v] > 0.0f &&
                            be_[v] > bs_[v] + 1 && fp.be[v] > fp.bs[v] + 1;
    }
    // MelFilterbank::new's count (mel_table)
    fp.n_mels = configured && c.enable_tempogram_mel_novelty ? std::max((int)c.tempogram_mel_n_mels, 4) : 0;
    return fp;
}

// k_features' per-chunk flags and mel schedule (8-bin chunks of the <8, 16, 4> walk; see FeatParams)
void feat_chunk_tables(const FeatParams& fp, const std::vector<MelPlan>& mplan, std::vector<int>* flags,
                       std::vector<MelChunk>* mel_chunks) {
    const int B = fp.B;
    auto band_of = [&](int b) {
        int v = 0;
        for (int q = 3; q >= 1; q--)
            if (fp.band_on[q] && b >= fp.bs[q] && b < fp.be[q]) v = q;
        return v;
    };
    std::vector<int>& cf = *flags;
    std::vector<MelChunk>& mc = *mel_chunks;
    cf.assign((size_t)(B + 7) / 8 + 1, 0);
    mc.assign((size_t)(B + 7) / 8 + 1, MelChunk{});
    for (int c0 = 0; c0 < B; c0 += 8) {
        const int v0 = band_of(c0);
        bool fast = fp.K == 4 && c0 + 8 <= B, mel = false, mel_ok = true, mel_reg = true;
        MelChunk& m = mc[(size_t)c0 / 8];
        for (int j = 0; j < 8; j++) m.bf[j] = (float)(c0 + j);
        for (int b = c0; fast && b < c0 + 8; b++) {
            const int v = band_of(b);
            if (v != v0) fast = false;
            if (v) {
                const int lo = b - fp.K < 0 ? 0 : b - fp.K, hi = b + fp.K + 1 < B ? b + fp.K + 1 : B;
                if (lo < fp.bs[v] || hi > fp.be[v]) fast = false;
            }
            if (fp.n_mels > 0) {
                const MelPlan& q = mplan[(size_t)b];
                if (q.nflush != 0 || q.w0 != 0.0f || q.w1 != 0.0f) mel = true;
                if (q.nflush < 0 || q.nflush > 3 || (q.s0 & ~1) || (q.s1 & ~1)) mel_ok = false;
                if ((q.w0 != 0.0f && q.s0 != 0) || (q.w1 != 0.0f && q.s1 != 1)) mel_reg = false;
                const int j = b - c0;
                m.bits |= (uint32_t)(q.nflush & 3) << (4 * j) | (uint32_t)(q.s0 & 1) << (4 * j + 2) |
                          (uint32_t)(q.s1 & 1) << (4 * j + 3);
                m.w0[j] = q.w0;
                m.w1[j] = q.w1;
            }
        }
        cf[(size_t)c0 / 8] = v0 | (fast && !mel ? FT_CHUNK_FAST : 0) | (fast && mel && mel_ok ? FT_CHUNK_MEL : 0) |
                             (fast && mel && mel_ok && mel_reg ? FT_CHUNK_MELREG : 0);
    }
}

// the combined novelty's weights and windows: the configured ones, or combined_novelty's defaults
// (novelty.rs:868-871)
NovParams nov_params(const sdsp_config& c, bool configured) {
    NovParams np{};
    np.ws = configured ? sd_maxf(c.tempogram_novelty_w_spectral, 0.0f) : 0.5f;
    np.we = configured ? sd_maxf(c.tempogram_novelty_w_energy, 0.0f) : 0.3f;
    np.wh = configured ? sd_maxf(c.tempogram_novelty_w_hfc, 0.0f) : 0.2f;
    np.lmw = configured ? (int)c.tempogram_novelty_local_mean_window : 16;
    np.smw = configured ? (int)c.tempogram_novelty_smooth_window : 5;
    np.wsum = sd_maxf(np.ws + np.we + np.wh, EPS);
    return np;
}

SelParams sel_params(const sdsp_config& c, const int present[NVAR], int NB, int top_n, int gate) {
    const bool configured = band_configured(c);
    SelParams sp{};
    sp.min_bpm = c.min_bpm;
    sp.max_bpm = c.max_bpm;
    sp.ac_tol = sd_maxf(c.bpm_resolution, 0.5f);
    for (int v = 0; v < NVAR; v++) sp.present[v] = present[v];
    sp.w[0] = configured ? c.tempogram_band_w_full : 1.0f;
    sp.w[1] = c.tempogram_band_w_low;
    sp.w[2] = c.tempogram_band_w_mid;
    sp.w[3] = c.tempogram_band_w_high;
    sp.w[4] = c.tempogram_mel_weight;
    sp.seed_only = configured ? c.tempogram_band_seed_only : 1;
    sp.support_thr = sd_clampf(configured ? c.tempogram_band_support_threshold : 0.25f, 0.0f, 1.0f);
    sp.bonus = sd_maxf(configured ? c.tempogram_band_consensus_bonus : 0.0f, 0.0f);
    sp.bonus_on = sp.bonus > 0.0f && configured && (c.enable_tempogram_band_fusion || c.enable_tempogram_mel_novelty);
    sp.top_n = top_n;
    sp.NB = NB;
    sp.gate = gate;
    sp.gate_top_n = (int)std::max<uint64_t>(std::max<uint64_t>(c.tempogram_candidates_top_n, c.tempogram_multi_res_top_k), 10);
    sp.gate_tol = sd_maxf(2.0f, c.bpm_resolution);
    return sp;
}

MrParams mr_params(const sdsp_config& c, uint32_t sr, int top_k, bool own512) {
    MrParams mp{};
    mp.min_bpm = c.min_bpm;
    mp.max_bpm = c.max_bpm;
    mp.tol = sd_maxf(2.0f, c.bpm_resolution);
    mp.w512 = c.tempogram_multi_res_w512;
    mp.w256 = c.tempogram_multi_res_w256;
    mp.w1024 = c.tempogram_multi_res_w1024;
    mp.dt = c.tempogram_multi_res_double_time_512_factor;
    mp.margin_thr = c.tempogram_multi_res_margin_threshold;
    mp.human_prior = c.tempogram_multi_res_use_human_prior;
    mp.top_k = top_k;
    mp.band = 1;  // src/lib.rs:509 always passes Some(band_cfg)
    mp.sr = (int)sr;
    mp.hop512 = 512;
    mp.own512 = own512 ? 1 : 0;
    return mp;
}

LegacyParams legacy_params(const sdsp_config& c, uint32_t sr, int hop) {
    LegacyParams P{};
    P.sr = (int)sr;
    P.hop = hop;
    P.min_bpm = c.min_bpm;
    P.max_bpm = c.max_bpm;
    P.res = c.bpm_resolution;
    P.guard = c.enable_legacy_bpm_guardrails ? 1 : 0;
    // LegacyBpmGuardrails::clamp_sane (period/mod.rs:88-121)
    const float pmn = c.legacy_bpm_preferred_min, pmx = c.legacy_bpm_preferred_max;
    const float smn = c.legacy_bpm_soft_min, smx = c.legacy_bpm_soft_max;
    P.g[0] = sd_minf(pmn, pmx);
    P.g[1] = sd_maxf(pmn, pmx);
    P.g[2] = sd_minf(sd_minf(smn, smx), P.g[0]);
    P.g[3] = sd_maxf(sd_maxf(smn, smx), P.g[1]);
    const float mul[3] = {c.legacy_bpm_conf_mul_preferred, c.legacy_bpm_conf_mul_soft, c.legacy_bpm_conf_mul_extreme};
    for (int k = 0; k < 3; k++) P.g[4 + k] = sd_isfinite_f(mul[k]) ? sd_maxf(mul[k], 0.0f) : 0.0f;
    return P;
}

// k_key_vote's parameters; band: the block-folded energies, whose decisions the vote certifies
KeyParams key_vote_params(const sdsp_config& c, bool band) {
    const int seg_len = (int)std::min<uint64_t>(c.key_segment_len_frames, INT32_MAX);
    const bool ms_on = c.enable_key_multi_scale && c.key_multi_scale_lengths_len > 0;
    KeyParams kp{};
    kp.near_check = band ? 1 : 0;
    kp.weighting = c.enable_key_frame_weighting;
    kp.min_tonal = c.key_min_tonalness;
    kp.tonal_pow = c.key_tonalness_power;
    kp.energy_pow = c.key_energy_power;
    kp.seg_voting = c.enable_key_segment_voting && c.key_segment_len_frames >= 120 && c.key_segment_hop_frames >= 1;
    kp.seg_len = std::max(seg_len, 1);
    kp.seg_hop = (int)std::max<uint64_t>(std::min<uint64_t>(c.key_segment_hop_frames, (uint64_t)seg_len), 1);
    kp.min_clarity = sd_clampf(c.key_segment_min_clarity, 0.0f, 1.0f);
    kp.sharpen = c.chroma_sharpening_power;
    kp.edge_trim = c.enable_key_edge_trim;
    kp.edge_frac = c.key_edge_trim_fraction;
    kp.ensemble = c.enable_key_ensemble;
    kp.kk_w = c.key_ensemble_kk_weight;
    kp.tp_w = c.key_ensemble_temperley_weight;
    kp.tset = c.key_template_set == SDSP_TEMPLATES_TEMPERLEY ? 1 : 0;
    kp.mh_on = c.enable_key_mode_heuristic || c.enable_key_minor_harmonic_bonus;
    kp.mh_bonus = c.enable_key_minor_harmonic_bonus;
    kp.mh_margin = c.key_mode_third_ratio_margin;
    kp.mh_flip = c.enable_key_mode_heuristic ? c.key_mode_flip_min_score_ratio : 0.0f;
    kp.mh_bonus_w = c.key_minor_leading_tone_bonus_weight;
    kp.ms_on = ms_on;
    kp.ms_n = ms_on ? (int)c.key_multi_scale_lengths_len : 0;
    kp.ms_hop = (int)std::max<uint64_t>(std::min<uint64_t>(c.key_multi_scale_hop, INT32_MAX), 1);
    kp.ms_nw = (int)std::min<uint64_t>(c.key_multi_scale_weights_len, 8);
    kp.ms_min_cl = sd_clampf(c.key_multi_scale_min_clarity, 0.0f, 1.0f);
    for (int j = 0; j < kp.ms_n; j++) kp.ms_len[j] = (int)std::min<uint64_t>(c.key_multi_scale_lengths[j], INT32_MAX);
    for (int j = 0; j < kp.ms_nw; j++) kp.ms_w[j] = c.key_multi_scale_weights[j];
    return kp;
}

// segment scratch rows of a chroma slice of F rows under vote parameters kp (an upper bound: edge
// trim only shortens it; with segment voting seg_len is the configured length, >= 120)
uint64_t seg_rows(const KeyParams& kp, uint64_t F) {
    uint64_t ns = (kp.seg_voting && F >= (uint64_t)kp.seg_len) ? (F - (uint64_t)kp.seg_len) / (uint64_t)kp.seg_hop + 1 : 0;
    uint64_t nm = 0;
    for (int j = 0; j < kp.ms_n; j++) {
        const uint64_t len = (uint64_t)kp.ms_len[j];
        if (len != 0 && len <= F) nm += (F - len) / (uint64_t)kp.ms_hop + 1;
    }
    return std::max(ns, nm);
}

// The percussive fallback's acceptance rule (src/lib.rs:640-668): the percussive estimate p against
// the current bpm / confidence / agreement and the base estimate
bool perc_better(const TempoEst& p, float cb, float cc, int ca, const TempoEst& b) {
    const float rel = cb > 1e-6f ? sd_maxf(p.bpm / cb, cb / p.bpm) : 1.0f;
    const bool fam = sd_absf(rel - 2.0f) < 0.05f || sd_absf(rel - 1.5f) < 0.05f ||
                     sd_absf(rel - (4.0f / 3.0f)) < 0.05f || sd_absf(rel - (3.0f / 2.0f)) < 0.05f ||
                     sd_absf(rel - (2.0f / 3.0f)) < 0.05f || sd_absf(rel - (3.0f / 4.0f)) < 0.05f;
    const bool forbid = cb <= 180.0f && p.bpm > 180.0f;
    const bool base_low_trap = b.trap_low || b.bpm < 95.0f;
    const bool in_common = p.bpm >= 70.0f && p.bpm <= 180.0f;
    return !forbid && fam && in_common &&
           (p.conf >= cc + 0.04f || (base_low_trap && p.conf >= cc * 0.85f) || (p.agree > ca && p.conf >= cc * 0.92f));
}

}  // namespace detail
}  // namespace sdsp
