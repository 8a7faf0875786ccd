// pipeline_debug.hip — the debug_track_id dumps (src/lib.rs:461-487, 547-573, 1471-1538;
// multi_resolution.rs:304-403, 707-745, 845-857): the reference's eprintln! diagnostics, printed
// per analysed track in batch order from what the kernels computed (candidate lists, estimates,
// MrDbg / KeyDbg records), and the stage probes of include/stratum_hip_debug.h.
#include "pipeline.hpp"

namespace sdsp {
namespace detail {
const char* tf_str(bool b) { return b ? "true" : "false"; }
// cand_support (src/lib.rs:420-431) and lookup_nearest (multi_resolution.rs:281-292)
float cand_support(const std::vector<Cand4>& c, float bpm, float tol) {
    float b = 0.0f;
    for (const Cand4& x : c)
        if (sd_absf(x.bpm - bpm) <= tol) b = sd_maxf(b, x.score);
    return b;
}
float lookup_nearest_h(const std::vector<Cand4>& c, float bpm, float tol) {
    float bd = SD_INF_F, bs = 0.0f;
    for (const Cand4& x : c) {
        const float d = sd_absf(x.bpm - bpm);
        if (d <= tol && d < bd) {
            bd = d;
            bs = x.score;
        }
    }
    return bs;
}
std::string key_str(int key) {  // Key::name
    char b[8];
    sdsp_key_name(key < 12 ? 0 : 1, (uint32_t)(key % 12), b, sizeof b);
    return b;
}
void print_debug(const sdsp_config& c, const TrackDbg& d) {
    const unsigned id = c.debug_track_id;
    auto gt = [&]() {
        if (c.has_debug_gt_bpm) std::fprintf(stderr, "GT bpm: %.3f\n", (double)c.debug_gt_bpm);
    };
    const float tol = sd_maxf(2.0f, c.bpm_resolution);
    if (d.base) {
        const TempoEst& b = d.est;
        const float s_base = cand_support(d.base_c, b.bpm, tol), s_2x = cand_support(d.base_c, b.bpm * 2.0f, tol),
                    s_half = cand_support(d.base_c, b.bpm * 0.5f, tol);
        const bool fam = (s_2x > 0.0f && s_2x >= s_base * 0.90f) || (s_half > 0.0f && s_half >= s_base * 0.90f);
        const bool fold = b.bpm * 2.0f >= 170.0f && b.bpm * 2.0f <= 200.0f;
        const bool weak = b.agree == 0 || b.conf < 0.06f;
        std::fprintf(stderr, "\n=== DEBUG base tempogram (track_id=%u) ===\n", id);
        gt();
        std::fprintf(stderr, "base_est: bpm=%.2f conf=%.4f agree=%d (trap_low=%s trap_high=%s ambiguous=%s)\n",
                     (double)b.bpm, (double)b.conf, b.agree, tf_str(b.trap_low), tf_str(b.trap_high), tf_str(b.ambiguous));
        std::fprintf(stderr,
                     "ambiguity signals: family_competes=%s (s_base=%.4f s_2x=%.4f s_half=%.4f) weak_base=%s "
                     "fold_into_trap=%s\n",
                     tf_str(fam), (double)s_base, (double)s_2x, (double)s_half, tf_str(weak), tf_str(fold));
        if (!b.ambiguous) std::fprintf(stderr, "NOTE: multi-res not run (outside trap zones).\n");
    }
    if (d.mr) {
        const size_t top_n = std::max<uint64_t>(c.debug_top_n, 1);
        std::fprintf(stderr, "\n=== DEBUG multi-res (track_id=%u) ===\n", id);
        gt();
        auto top = [&](const char* label, const std::vector<Cand4>& v) {
            std::fprintf(stderr, "%s top-%zu:\n", label, top_n);
            for (size_t k = 0; k < v.size() && k < top_n; k++)
                std::fprintf(stderr, "  bpm=%7.2f score=%.4f\n", (double)v[k].bpm, (double)v[k].score);
        };
        top("hop=256", d.c256);
        top("hop=512", d.c512);
        top("hop=1024", d.c1024);
        if (c.has_debug_gt_bpm) {
            const float g = c.debug_gt_bpm;
            const float t512 = lookup_nearest_h(d.c512, g, tol), t256 = lookup_nearest_h(d.c256, g, tol),
                        t1024 = lookup_nearest_h(d.c1024, g, tol);
            const float d512 = lookup_nearest_h(d.c512, g * 2.0f, tol), d256 = lookup_nearest_h(d.c256, g * 2.0f, tol),
                        d1024 = lookup_nearest_h(d.c1024, g * 2.0f, tol);
            const float h512 = lookup_nearest_h(d.c512, g * 0.5f, tol), h256 = lookup_nearest_h(d.c256, g * 0.5f, tol),
                        h1024 = lookup_nearest_h(d.c1024, g * 0.5f, tol);
            std::fprintf(stderr, "Support near GT / family (lookup tol=%.2f):\n", (double)tol);
            std::fprintf(stderr, "  T     @512=%.4f @256=%.4f @1024=%.4f\n", (double)t512, (double)t256, (double)t1024);
            std::fprintf(stderr, "  2T    @512=%.4f @256=%.4f @1024=%.4f\n", (double)d512, (double)d256, (double)d1024);
            std::fprintf(stderr, "  T/2   @512=%.4f @256=%.4f @1024=%.4f\n", (double)h512, (double)h256, (double)h1024);
            const float w512 = c.tempogram_multi_res_w512, w256 = c.tempogram_multi_res_w256,
                        w1024 = c.tempogram_multi_res_w1024, dt = c.tempogram_multi_res_double_time_512_factor;
            const float h_t = w512 * t512 + w256 * t256 + w1024 * (t1024 + c.tempogram_multi_res_structural_discount * d1024);
            float h_2t = w512 * (dt * t512 + (1.0f - dt) * d512) + w256 * d256 + w1024 * d1024;
            float h_h = w512 * (dt * t512 + (1.0f - dt) * h512) + w256 * h256 + w1024 * h1024;
            const float eps = 1e-6f;
            const float r2 = (d256 + eps) / (t256 + eps), rh = (h1024 + eps) / (t1024 + eps);
            if (r2 < 1.10f) h_2t *= 0.75f;
            if (r2 < 1.00f) h_2t *= 0.75f;
            if (rh < 1.10f) h_h *= 0.75f;
            if (rh < 1.00f) h_h *= 0.75f;
            struct L {
                float bpm, s;
                const char* tag;
            };
            std::vector<L> loc = {{g, h_t, "T"}, {g * 2.0f, h_2t, "2T"}, {g * 0.5f, h_h, "T/2"}};
            std::vector<L> keep;
            for (const L& l : loc)
                if (l.bpm >= c.min_bpm && l.bpm <= c.max_bpm) keep.push_back(l);
            for (L& l : keep) {
                if (l.bpm > 210.0f) l.s *= 0.80f;
                else if (l.bpm > 180.0f) l.s *= 0.90f;
                else if (l.bpm < 60.0f) l.s *= 0.92f;
            }
            std::stable_sort(keep.begin(), keep.end(), [](const L& a, const L& b) { return a.s > b.s; });
            std::fprintf(stderr, "Fusion scores (T anchored at GT, after guardrails+prior):\n");
            for (const L& l : keep) std::fprintf(stderr, "  %3s bpm=%7.2f score=%.4f\n", l.tag, (double)l.bpm, (double)l.s);
            if (keep.size() >= 2)
                std::fprintf(stderr, "  margin(best-second)=%.4f (threshold=%.4f)\n", (double)(keep[0].s - keep[1].s),
                             (double)c.tempogram_multi_res_margin_threshold);
            std::fprintf(stderr, "  ratio_2T_256=%.3f ratio_half_1024=%.3f (guardrails)\n", (double)r2, (double)rh);
        }
        const MrDbg& m = d.md;
        if (m.fd)
            std::fprintf(stderr, "DEBUG fold-down (track_id=%u): %.2f -> %.2f (support ratio %.3f, agree %d->%d).\n", id,
                         (double)m.fd_from, (double)m.fd_to, (double)m.fd_ratio, m.fd_a0, m.fd_a1);
        if (m.fu)
            std::fprintf(stderr, "DEBUG fold-up (track_id=%u): %.2f -> %.2f (support ratio %.3f, agree %d->%d).\n", id,
                         (double)m.fu_from, (double)m.fu_to, (double)m.fu_ratio, m.fu_a0, m.fu_a1);
        if (m.tf) {
            static const char* lab[5] = {"T", "3/2", "2/3", "4/3", "3/4"};
            std::fprintf(stderr,
                         "DEBUG triplet-family (track_id=%u): %.2f -> %.2f (%s, support %.3f->%.3f, align %.3f->%.3f)\n",
                         id, (double)m.tf_from, (double)m.tf_to, lab[m.tf_label < 0 || m.tf_label > 4 ? 0 : m.tf_label],
                         (double)m.tf_sup0, (double)m.tf_sup1, (double)m.tf_al0, (double)m.tf_al1);
        }
        std::fprintf(stderr, "\n=== DEBUG multi-res decision (track_id=%u) ===\n", id);
        gt();
        std::fprintf(stderr, "base_est: bpm=%.2f conf=%.4f agree=%d\n", (double)d.est.bpm, (double)d.est.conf, d.est.agree);
        std::fprintf(stderr, "mr_est:   bpm=%.2f conf=%.4f agree=%d\n", (double)d.mr_est.bpm, (double)d.mr_est.conf,
                     d.mr_est.agree);
        std::fprintf(stderr, "ambiguous(trap_low||trap_high)=%s\n", tf_str(d.est.ambiguous));
        std::fprintf(stderr, "rel=%.3f family_related=%s forbid_promote_high=%s\n", (double)m.rel, tf_str(m.fam),
                     tf_str(m.forbid));
        std::fprintf(stderr, "mr_better=%s used_mr=%s\n", tf_str(m.better), tf_str(m.better));
    }
    if (d.key) {
        const KeyDbg& k = d.kd;
        std::fprintf(stderr, "\n=== DEBUG key (track_id=%u) ===\n", id);
        std::fprintf(stderr,
                     "key=%s conf=%.4f clarity=%.4f frames=%d used_frames=%d soft_mapping=%s sigma=%.3f harmonic_mask=%s "
                     "mask_p=%.2f tuning=%.4f time_smooth=%s margin=%llu edge_trim=%s trim_frac=%.2f\n",
                     key_str(d.ko.mode * 12 + d.ko.tonic).c_str(), (double)d.ko.conf, (double)d.ko.clarity, k.frames, k.used,
                     tf_str(c.soft_chroma_mapping), (double)c.soft_mapping_sigma, tf_str(c.enable_key_harmonic_mask),
                     (double)c.key_harmonic_mask_power, (double)d.tuning, tf_str(c.enable_key_spectrogram_time_smoothing),
                     (unsigned long long)c.key_spectrogram_smooth_margin, tf_str(c.enable_key_edge_trim),
                     (double)c.key_edge_trim_fraction);
        // top_keys: the first three of the final table; the chosen key replaces the third when it is
        // not among them (detector.rs:506-510)
        std::vector<std::pair<int, float>> tk;
        for (int q = 0; q < 3; q++) tk.push_back({k.order[q], k.tab[q]});
        bool in = false;
        for (const auto& e : tk) in |= e.first == k.key;
        if (!in)
            for (int q = 3; q < 24; q++)
                if (k.order[q] == k.key) tk.back() = {k.key, k.tab[q]};
        std::string line;
        for (size_t q = 0; q < tk.size(); q++) {
            char b[64];
            std::snprintf(b, sizeof b, "%s%s:%.4f", q ? ", " : "", key_str(tk[q].first).c_str(), (double)tk[q].second);
            line += b;
        }
        std::fprintf(stderr, "top_keys: %s\n", line.c_str());
        static const char* notes[12] = {"C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"};
        std::vector<int> pcs(12);
        for (int q = 0; q < 12; q++) pcs[q] = q;
        std::stable_sort(pcs.begin(), pcs.end(), [&](int a, int b) { return k.agg[a] > k.agg[b]; });
        line.clear();
        for (int q = 0; q < 6; q++) {
            char b[64];
            std::snprintf(b, sizeof b, "%s%s:%.3f", q ? ", " : "", notes[pcs[q]], (double)k.agg[pcs[q]]);
            line += b;
        }
        std::fprintf(stderr, "top_pitch_classes(weighted): %s\n", line.c_str());
    }
}
}  // namespace detail

static std::vector<Cand4> cand_list(const std::vector<float>& h, size_t row, int cap, int n) {
    std::vector<Cand4> v;
    for (int c = 0; c < n; c++) {
        const float* q = h.data() + (row * (size_t)cap + (size_t)c) * 4;
        v.push_back({q[0], q[1], q[2], q[3]});
    }
    return v;
}

// src/lib.rs:461-487: the base estimate and its candidate list
void Pipeline::debug_base(const TempoPassIn& bin, const TempoPassOut& bo, const std::vector<TempoEst>& best,
                          std::vector<TrackDbg>& tdbg) {
    const std::vector<float> bc = c_.down(bo.cand, best.size() * (size_t)bin.cand_cap * 4);
    for (size_t i = 0; i < best.size(); i++) {
        if (!best[i].ok) continue;
        TrackDbg& t = tdbg[i];
        t.base = true;
        t.est = best[i];
        t.base_c = cand_list(bc, i, bin.cand_cap, std::min(best[i].n_cands, bin.cand_cap));
    }
}

// multi_resolution.rs:304-403, 707-860 and src/lib.rs:547-573: the three hops' candidate lists (the
// hop-512 one has rows512 rows of cap512, in E order when it is the escalation's own), the
// multi-resolution estimates and k_multires' decision records
void Pipeline::debug_multires(const std::vector<int>& E, bool own512, int cap512, int cap_aux, size_t rows512,
                              const TempoPassOut& o256, const TempoPassOut& b512, const TempoPassOut& o1024,
                              const std::vector<int>& n256, const std::vector<int>& n512, const std::vector<int>& n1024,
                              const TempoEst* d_mr, const MrDbg* d_mdbg, std::vector<TrackDbg>& tdbg) {
    const size_t NE = E.size();
    const std::vector<float> h256 = c_.down(o256.cand, NE * (size_t)cap_aux * 4);
    const std::vector<float> h1024 = c_.down(o1024.cand, NE * (size_t)cap_aux * 4);
    const std::vector<float> h512 = c_.down(b512.cand, rows512 * (size_t)cap512 * 4);
    const std::vector<TempoEst> hmr = c_.down(d_mr, NE);
    const std::vector<MrDbg> hmd = c_.down(d_mdbg, NE);
    for (size_t k = 0; k < NE; k++) {
        const size_t i = (size_t)E[k];
        TrackDbg& t = tdbg[i];
        const size_t j512 = own512 ? k : i;
        if (!hmr[k].ok || n256[k] < 0 || n1024[k] < 0 || n512[j512] < 0) continue;
        t.mr = true;
        t.c256 = cand_list(h256, k, cap_aux, n256[k]);
        t.c512 = cand_list(h512, j512, cap512, n512[j512]);
        t.c1024 = cand_list(h1024, k, cap_aux, n1024[k]);
        t.mr_est = hmr[k];
        t.md = hmd[k];
    }
}

// src/lib.rs:1471-1538 (the beat-synchronous re-vote keeps the frame-level record)
void Pipeline::debug_key(const KeyLaunch& kl, const std::vector<KeyOut>& kout, std::vector<TrackDbg>& tdbg) {
    const size_t NK = kl.K.size();
    if (NK == 0) return;
    const std::vector<KeyDbg> kd = c_.down(kl.d_kdbg, NK);
    const std::vector<float> tu = kl.d_tune ? c_.down(kl.d_tune, NK) : std::vector<float>(NK, 0.0f);
    for (size_t k = 0; k < NK; k++) {
        if (!kout[k].ok) continue;
        TrackDbg& t = tdbg[(size_t)kl.K[k]];
        t.key = true;
        t.ko = kout[k];
        t.kd = kd[k];
        t.tuning = tu[k];
    }
}

// sdsp_debug_tempo_stages: tempo_pass through its mags_in / fmax_in path (the percussive
// fallback's), then the stage buffers and the tempogram lists back to the host.
void Pipeline::debug_tempo_stages(const float* host_mags, const uint64_t* frames, uint64_t n_tracks, int hop,
                                  sdsp_debug_tempo_out* out) {
    if (const std::string why = check_supported(cfg_, sr_); !why.empty()) throw HipError(why);
    TempoPassIn in;
    in.hop = hop;
    in.samples = nullptr;
    uint64_t total = 0;
    for (uint64_t t = 0; t < n_tracks; t++) {
        in.src_off.push_back(0);
        in.gain_h.push_back(1.0f);
        in.n_trim.push_back((uint64_t)fs_ + (frames[t] - 1) * (uint64_t)hop);  // frames[t] frames exactly
        total += frames[t];
    }
    in.top_n = 10;
    in.cand_cap = 10;
    in.gate = 0;
    std::vector<float> fmax((size_t)total);
    for (uint64_t r = 0; r < total; r++) {  // the exact row maximum
        float m = 0.0f;
        for (int b = 0; b < nb_; b++) m = std::max(m, host_mags[r * (uint64_t)nb_ + (uint64_t)b]);
        fmax[(size_t)r] = m;
    }
    float* d_mags = c_.dev<float>("P.in", total * (uint64_t)s2_);
    SDSP_HIP_CHECK(hipMemsetAsync(d_mags, 0, total * (uint64_t)s2_ * sizeof(float), d_.stream));
    SDSP_HIP_CHECK(hipMemcpy2DAsync(d_mags, (size_t)s2_ * sizeof(float), host_mags, (size_t)nb_ * sizeof(float),
                                    (size_t)nb_ * sizeof(float), total, hipMemcpyHostToDevice, d_.stream));
    in.mags_in = d_mags;
    in.fmax_in = c_.up("P.inmax", fmax);
    TempoStageDbg g;
    in.dbg = &g;
    TempoPassOut po;
    tempo_pass("B.", in, po);
    const PassTg& tg = g.tg;
    out->n_mels = g.fp.n_mels;
    out->NB = tg.NB;
    for (int v = 0; v < 4; v++) {
        out->bs[v] = g.fp.bs[v];
        out->be[v] = g.fp.be[v];
        out->band_on[v] = g.fp.band_on[v];
    }
    for (int v = 0; v < NVAR; v++) out->present[v] = tg.present[v];
    if ((uint32_t)g.fp.n_mels > out->mel_cap || (uint32_t)tg.NB > out->acf_cap) throw std::invalid_argument("capacity");
    for (int k : tg.fft_k)
        if ((uint32_t)k > out->fft_cap) throw std::invalid_argument("capacity");
    auto get = [&](const float* d, float* h, size_t n) {
        if (n) SDSP_HIP_CHECK(hipMemcpyAsync(h, d, n * sizeof(float), hipMemcpyDeviceToHost, d_.stream));
    };
    get(po.E, out->E, 4 * (size_t)total);
    get(po.H, out->H, 4 * (size_t)total);
    get(po.SFX, out->SFX, 4 * (size_t)total);
    get(po.SFO, out->SFO, (size_t)total);
    get(po.MEL, out->MEL, (size_t)g.fp.n_mels * (size_t)total);
    get(po.nov, out->nov, NVAR * (size_t)total);
    get(po.nov_sum, out->nov_sum, NVAR * (size_t)n_tracks);
    const size_t n_it = tg.items.size();
    uint64_t n_fft = 0;
    for (size_t i = 0; i < n_it; i++) n_fft = std::max(n_fft, tg.fft_off[i] + (uint64_t)tg.fft_k[i]);
    const std::vector<float> ab = c_.down(tg.acf_bpm, n_it * (size_t)tg.NB), as = c_.down(tg.acf_str, n_it * (size_t)tg.NB);
    const std::vector<float> fb = c_.down(tg.fft_bpm, (size_t)n_fft), fw = c_.down(tg.fft_pow, (size_t)n_fft);
    for (uint64_t k = 0; k < n_tracks * NVAR; k++) out->acf_n[k] = out->fft_n[k] = 0;
    for (size_t i = 0; i < n_it; i++) {
        const size_t slot = (size_t)tg.items[i];
        float* a = out->acf + slot * out->acf_cap * 2;
        float* f = out->fft + slot * out->fft_cap * 2;
        for (int j = 0; j < tg.NB; j++) {
            a[2 * j] = ab[i * (size_t)tg.NB + (size_t)j];
            a[2 * j + 1] = as[i * (size_t)tg.NB + (size_t)j];
        }
        for (int j = 0; j < tg.fft_k[i]; j++) {
            f[2 * j] = fb[(size_t)tg.fft_off[i] + (size_t)j];
            f[2 * j + 1] = fw[(size_t)tg.fft_off[i] + (size_t)j];
        }
        out->acf_n[slot] = tg.NB;
        out->fft_n[slot] = tg.fft_k[i];
    }
}

// sdsp_debug_tempo_select: select_lists (pass_select from its offset tables on) over uploaded
// tempogram lists, packed as pass_tempograms leaves them: the present variants of the active tracks
// back to back, offset 0 for every other slot.
void Pipeline::debug_tempo_select(const float* fft, const int32_t* fft_n, const float* acf, int NB, const int32_t present[5],
                                  const int32_t* active, uint64_t n_tracks, int top_n, int cand_cap, int gate,
                                  sdsp_debug_tempo_est* est, float* cand) {
    static_assert(sizeof(sdsp_debug_tempo_est) == sizeof(TempoEst), "the probe's record mirrors the kernel's");
    if (const std::string why = check_supported(cfg_, sr_); !why.empty()) throw HipError(why);
    const int T = (int)n_tracks;
    SelLists sl;
    sl.NB = NB;
    for (int v = 0; v < NVAR; v++) sl.present[v] = present[v] != 0;
    sl.fo.assign((size_t)T * NVAR, 0);
    sl.ao.assign((size_t)T * NVAR, 0);
    sl.fft_k.assign((size_t)T, 0);
    std::vector<float> fb, fw, ab, as;
    uint64_t pair0 = 0;  // first pair of the track's five lists
    for (int t = 0; t < T; t++) {
        const uint64_t K = (uint64_t)fft_n[t];
        sl.fft_k[(size_t)t] = (int)K;
        for (int v = 0; v < NVAR && active[t]; v++) {
            if (!sl.present[v]) continue;
            sl.fo[(size_t)t * NVAR + (size_t)v] = fb.size();
            sl.ao[(size_t)t * NVAR + (size_t)v] = ab.size();
            const float* f = fft + 2 * (pair0 + (uint64_t)v * K);
            const float* a = acf + 2 * ((uint64_t)t * NVAR + (uint64_t)v) * (uint64_t)NB;
            for (uint64_t j = 0; j < K; j++) fb.push_back(f[2 * j]), fw.push_back(f[2 * j + 1]);
            for (int j = 0; j < NB; j++) ab.push_back(a[2 * j]), as.push_back(a[2 * j + 1]);
        }
        pair0 += NVAR * K;
    }
    sl.fft_bpm = c_.up("S.fftb", fb);
    sl.fft_pow = c_.up("S.fftp", fw);
    sl.acf_bpm = c_.up("S.acfb", ab);
    sl.acf_str = c_.up("S.acfs", as);
    TempoPassOut o;
    o.active = c_.up("S.active", std::vector<int>(active, active + T));
    select_lists("S.", T, sl, top_n, gate, cand_cap, o);
    const std::vector<TempoEst> e = c_.down(o.est, (size_t)T);
    const std::vector<float> c = c_.down(o.cand, (size_t)T * (size_t)cand_cap * 4);
    std::memcpy(est, e.data(), (size_t)T * sizeof(TempoEst));
    std::fill(cand, cand + (size_t)T * (size_t)cand_cap * 4, 0.0f);
    for (int t = 0; t < T; t++)  // the rows the kernel wrote
        std::copy_n(c.begin() + (ptrdiff_t)((size_t)t * (size_t)cand_cap * 4), (size_t)e[(size_t)t].n_cands * 4,
                    cand + (size_t)t * (size_t)cand_cap * 4);
}

// sdsp_debug_multires: fuse_multires (escalate's tail) over uploaded candidate lists, base estimates
// and hop-512 novelty rows; the rows lie at a frame prefix of nov_n + 1 frames each, as a tempo pass
// leaves a novelty curve.
void Pipeline::debug_multires_fuse(const sdsp_debug_multires_in* in, sdsp_debug_multires_out* out) {
    static_assert(sizeof(sdsp_debug_tempo_est) == sizeof(TempoEst) && sizeof(sdsp_debug_mr_dbg) == sizeof(MrDbg),
                  "the probe's records mirror the kernel's");
    if (const std::string why = check_supported(cfg_, sr_); !why.empty()) throw HipError(why);
    const size_t NR = (size_t)in->n_tracks, NE = (size_t)in->n_items;
    const int top_k = (int)std::max<uint64_t>(cfg_.tempogram_multi_res_top_k, 1);
    const bool own512 = in->own512 != 0;
    const size_t rows = own512 ? NE : NR;
    const int cap512 = own512 ? top_k : (int)in->cap_base, cap_aux = (int)in->cap_aux;
    std::vector<int> E(in->items, in->items + NE);
    for (size_t k = 0; k < NE; k++)
        if (E[k] < 0 || (size_t)E[k] >= NR || (k > 0 && E[k] <= E[k - 1])) throw std::invalid_argument("item list");
    MrFuse m;
    m.n256.assign(in->n256, in->n256 + NE);
    m.n1024.assign(in->n1024, in->n1024 + NE);
    m.n512.assign(in->n512, in->n512 + rows);
    for (size_t k = 0; k < NE; k++)
        if (m.n256[k] > cap_aux || m.n1024[k] > cap_aux) throw std::invalid_argument("capacity");
    std::vector<uint64_t> fpfx(1, 0);
    for (size_t r = 0; r < rows; r++) {
        if (m.n512[r] > cap512) throw std::invalid_argument("capacity");
        if (in->nov_n[r] >= (1u << 24)) throw std::invalid_argument("novelty row");
        fpfx.push_back(fpfx.back() + in->nov_n[r] + 1);
    }
    std::vector<float> nov((size_t)fpfx.back(), 0.0f);
    for (size_t r = 0, at = 0; r < rows; at += (size_t)in->nov_n[r], r++)
        std::copy_n(in->nov512 + at, (size_t)in->nov_n[r], nov.begin() + (ptrdiff_t)fpfx[r]);
    m.c256 = c_.up("M.c256", std::vector<float>(in->c256, in->c256 + NE * (size_t)cap_aux * 4));
    m.c1024 = c_.up("M.c1024", std::vector<float>(in->c1024, in->c1024 + NE * (size_t)cap_aux * 4));
    m.c512 = c_.up("M.c512", std::vector<float>(in->c512, in->c512 + rows * (size_t)cap512 * 4));
    m.cap_aux = cap_aux;
    m.cap_base = (int)in->cap_base;
    m.own512 = own512;
    const TempoEst* base = reinterpret_cast<const TempoEst*>(in->base);
    m.base_est = c_.up("M.base", std::vector<TempoEst>(base, base + NR));
    m.nov512 = c_.up("M.nov", nov);
    m.fpfx512 = c_.up("M.fpfx", fpfx);
    m.want_dbg = true;
    Tempo tp;
    tp.d_fbpm = c_.up("B.fbpm", std::vector<float>(out->final_bpm, out->final_bpm + NR));
    tp.d_fconf = c_.up("B.fconf", std::vector<float>(out->final_conf, out->final_conf + NR));
    tp.d_used = c_.up("B.used", std::vector<int>(out->used, out->used + NR));
    fuse_multires(E, (int)NR, m, tp);
    tempo_down((int)NR, tp);
    std::vector<TempoEst> mr = c_.down(tp.d_mr_all, NE);
    std::vector<MrDbg> md = c_.down(m.d_mdbg, NE);
    for (size_t k = 0; k < NE; k++)  // the kernel writes only `ok` of an item it leaves early
        if (!mr[k].ok) mr[k] = TempoEst{}, md[k] = MrDbg{};
    std::memcpy(out->mr, mr.data(), NE * sizeof(TempoEst));
    std::memcpy(out->dbg, md.data(), NE * sizeof(MrDbg));
    std::copy(tp.used.begin(), tp.used.end(), out->used);
    std::copy(tp.fbpm_h.begin(), tp.fbpm_h.end(), out->final_bpm);
    std::copy(tp.fconf_h.begin(), tp.fconf_h.end(), out->final_conf);
}

// sdsp_debug_key_stages: key_condition (and, for mode 1, tail_exact) over uploaded key spectrograms.
// exact_energy_ selects mode 2's sequence, as it does for the nested rerun.
void Pipeline::debug_key_stages(const float* host_mags, const uint64_t* frames, uint64_t n_tracks, int mode,
                                float* masked, float* chroma, float* energy, float* edel, int32_t info[4]) {
    if (const std::string why = check_supported(cfg_, sr_); !why.empty()) throw HipError(why);
    if ((mode == 2) != exact_energy_) throw HipError("debug_key_stages: mode 2 runs on an exact-energy pipeline");
    if (mode != 0 && !key_energy_blocked(cfg_, sr_)) throw std::invalid_argument("modes 1 and 2 need the band path");
    const int NK = (int)n_tracks, B8 = kfs_ / 2 + 1;
    std::vector<uint64_t> kpfx(1, 0), ktile(1, 0);
    std::vector<int> kid((size_t)NK);
    for (int k = 0; k < NK; k++) {
        kpfx.push_back(kpfx.back() + frames[k]);
        ktile.push_back(ktile.back() + (frames[k] + HP_FRAMES - 1) / HP_FRAMES);
        kid[(size_t)k] = k;
    }
    const uint64_t total8 = kpfx.back();
    const std::string EP = "E0.";
    hipStream_t st = d_.stream;
    uint64_t* d_kpfx = c_.up(EP + "kpfx", kpfx);
    uint64_t* d_ktile = c_.up(EP + "ktile", ktile);
    int* d_kid = c_.up(EP + "kid", kid);
    float* mags8 = c_.dev<float>("E.mags8", total8 * (uint64_t)ks_);
    SDSP_HIP_CHECK(hipMemsetAsync(mags8, 0, total8 * (uint64_t)ks_ * sizeof(float), st));
    SDSP_HIP_CHECK(hipMemcpy2DAsync(mags8, (size_t)ks_ * sizeof(float), host_mags, (size_t)B8 * sizeof(float),
                                    (size_t)B8 * sizeof(float), total8, hipMemcpyHostToDevice, st));
    Timers kt;
    kt.init(d_);
    const KeyCond kc = key_condition(EP, mags8, kpfx, ktile, d_kpfx, d_ktile, d_kid, st, kt);
    if (mode == 1) {
        if (!kc.band || !kc.d_ht) throw HipError("debug_key_stages: mode 1 without the band path");
        KeyTail t;
        tail_buffers(t, kc, mags8, d_kpfx, total8);
        tail_exact(t, d_kid, NK, d_ktile, ktile.back(), st);
    }
    info[0] = kc.st_lo;
    info[1] = kc.st_hi;
    info[2] = kc.band ? 1 : 0;
    info[3] = B8;
    SDSP_HIP_CHECK(hipMemcpy2DAsync(masked, (size_t)B8 * sizeof(float), mags8, (size_t)ks_ * sizeof(float),
                                    (size_t)B8 * sizeof(float), total8, hipMemcpyDeviceToHost, st));
    SDSP_HIP_CHECK(hipMemcpyAsync(chroma, kc.d_chroma, total8 * 12 * sizeof(float), hipMemcpyDeviceToHost, st));
    SDSP_HIP_CHECK(hipMemcpyAsync(energy, kc.d_energy, total8 * sizeof(float), hipMemcpyDeviceToHost, st));
    if (edel && kc.d_edel && mode == 0)
        SDSP_HIP_CHECK(hipMemcpyAsync(edel, kc.d_edel, total8 * sizeof(float), hipMemcpyDeviceToHost, st));
    c_.sync();
}

// sdsp_debug_key_vote: the vote launch of launch_key (all tracks) or rerun_tail (a selection) over
// uploaded chroma rows and energies, then every buffer the kernel wrote back to the host.
void Pipeline::debug_key_vote(const float* host_chroma, const float* host_energy, const float* host_edel,
                              const uint64_t* frames, uint64_t n_tracks, const int32_t* sel, uint64_t n_sel, int threads,
                              bool alone, bool cert_fixed, sdsp_debug_key_vote_out* out) {
    static_assert(sizeof(sdsp_debug_key_out) == sizeof(KeyOut) && sizeof(sdsp_debug_key_dbg) == sizeof(KeyDbg),
                  "the probe's records mirror the kernel's");
    if (const std::string why = check_supported(cfg_, sr_); !why.empty()) throw HipError(why);
    KeyParams kp = key_vote_params(cfg_, host_edel != nullptr);
    kp.cert_fixed = cert_fixed ? 1 : 0;
    std::vector<uint64_t> kpfx(1, 0);
    for (uint64_t t = 0; t < n_tracks; t++) kpfx.push_back(kpfx.back() + frames[t]);
    const uint64_t total = kpfx.back();
    std::vector<int> items;
    if (sel) {
        std::vector<char> seen((size_t)n_tracks, 0);
        for (uint64_t j = 0; j < n_sel; j++) {
            if (sel[j] < 0 || (uint64_t)sel[j] >= n_tracks || seen[(size_t)sel[j]]) throw std::invalid_argument("selection");
            seen[(size_t)sel[j]] = 1;
            items.push_back(sel[j]);
        }
    } else {
        for (uint64_t t = 0; t < n_tracks; t++) items.push_back((int)t);
    }
    const int n_items = (int)items.size();
    // the segment scratch as launch_key sizes it, compact by item as rerun_tail's
    std::vector<uint64_t> kseg(1, 0);
    for (int k : items) kseg.push_back(kseg.back() + (uint64_t)KV_ROW * seg_rows(kp, frames[(size_t)k]));
    if (kseg.back() / KV_ROW > out->seg_rows_cap) throw std::invalid_argument("capacity");
    for (size_t i = 0; i < kseg.size(); i++) out->seg_row_pfx[i] = kseg[i] / KV_ROW;
    if (n_items == 0) return;
    hipStream_t st = d_.stream;
    // the kernel sharpens the raw rows in place: a copy of the caller's
    float* d_cr = c_.up("V.chroma", std::vector<float>(host_chroma, host_chroma + total * 12));
    float* d_en = c_.up("V.energy", std::vector<float>(host_energy, host_energy + total));
    float* d_edel = host_edel ? c_.up("V.edel", std::vector<float>(host_edel, host_edel + total)) : nullptr;
    uint64_t* d_kpfx = c_.up("V.kpfx", kpfx);
    uint64_t* d_kseg = c_.up("V.kseg", kseg);
    int* d_items = c_.up("V.items", items);
    std::vector<float> tpl(576);
    key_templates(tpl.data());
    float* d_tpl = c_.up("V.tpl", tpl);
    const KeyOut* in_ko = reinterpret_cast<const KeyOut*>(out->key);
    KeyOut* d_ko = c_.up("V.kout", std::vector<KeyOut>(in_ko, in_ko + n_tracks));
    const size_t n_scr = (size_t)std::max<uint64_t>(kseg.back(), 1);
    float* d_cs = c_.dev<float>("V.chroma_s", total * 12);
    float* d_w = c_.dev<float>("V.weights", total);
    float* d_wdel = host_edel ? c_.dev<float>("V.wdel", total) : nullptr;
    float* d_scr = c_.dev<float>("V.segscr", n_scr);
    KeyDbg* d_dbg = c_.dev<KeyDbg>("V.kdbg", (size_t)n_items);
    SDSP_HIP_CHECK(hipMemsetAsync(d_cs, 0, total * 12 * sizeof(float), st));
    SDSP_HIP_CHECK(hipMemsetAsync(d_w, 0, total * sizeof(float), st));
    if (d_wdel) SDSP_HIP_CHECK(hipMemsetAsync(d_wdel, 0, total * sizeof(float), st));
    SDSP_HIP_CHECK(hipMemsetAsync(d_scr, 0, n_scr * sizeof(float), st));
    SDSP_HIP_CHECK(hipMemsetAsync(d_dbg, 0, (size_t)n_items * sizeof(KeyDbg), st));
    launch_key_vote(d_items, n_items, d_kpfx, d_cr, d_en, d_cs, d_w, d_scr, d_kseg, d_tpl, kp, d_ko, st, d_dbg, d_edel,
                    d_wdel, alone, threads);
    SDSP_HIP_CHECK(hipGetLastError());
    auto get = [&](const void* d, void* h, size_t bytes) {
        if (bytes) SDSP_HIP_CHECK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st));
    };
    get(d_ko, out->key, (size_t)n_tracks * sizeof(KeyOut));
    get(d_cs, out->chroma_s, (size_t)total * 12 * sizeof(float));
    get(d_w, out->weights, (size_t)total * sizeof(float));
    if (d_wdel && out->wdel) get(d_wdel, out->wdel, (size_t)total * sizeof(float));
    get(d_scr, out->seg_rows, (size_t)kseg.back() * sizeof(float));
    get(d_dbg, out->dbg, (size_t)n_items * sizeof(KeyDbg));
    c_.sync();
}

// sdsp_debug_onset_stages: onset_lists over uploaded curves, then every list back to the host.
void Pipeline::debug_onset_stages(const float* rms, const float* hfc, const float* sfo, const float* hpe,
                                  const uint64_t* frames, const uint64_t* n_trim, uint64_t n_tracks, int hop,
                                  sdsp_debug_onset_out* out) {
    if (const std::string why = check_supported(cfg_, sr_); !why.empty()) throw HipError(why);
    TempoPassOut bo;
    bo.fpfx.assign(1, 0);
    for (uint64_t t = 0; t < n_tracks; t++) bo.fpfx.push_back(bo.fpfx.back() + frames[t]);
    const uint64_t total = bo.total = bo.fpfx.back();
    bo.d_fpfx = c_.up("O.fpfx", bo.fpfx);
    auto curve = [&](const char* name, const float* h) { return c_.up(name, std::vector<float>(h, h + total)); };
    float* d_erms = curve("O.rms", rms);
    bo.H = curve("O.hfc", hfc);
    bo.SFO = curve("O.sfo", sfo);
    Hpss hp;
    if (hpe) hp.d_hpe = curve("O.hpe", hpe);
    const uint64_t* d_nt = c_.up("B.ntrim", std::vector<uint64_t>(n_trim, n_trim + n_tracks));
    const Onsets on = onset_lists(d_erms, d_nt, hop, bo, hp);
    const size_t T = (size_t)n_tracks;
    const int kinds = on.lists - 1;
    const std::vector<uint32_t> eon = c_.down(on.d_eon, (size_t)total), fon = c_.down(on.d_fon, (size_t)(kinds * total)),
                                ch = c_.down(on.d_chosen, (size_t)on.lists * (size_t)total);
    const std::vector<int> fn = c_.down(on.d_fn, (size_t)kinds * T), cn = c_.down(on.d_cn, T);
    uint32_t* const lists[3] = {out->spectral, out->hfc, out->hpss};
    int32_t* const counts[3] = {out->n_spectral, out->n_hfc, out->n_hpss};
    for (size_t t = 0; t < T; t++) {
        const size_t f0 = (size_t)bo.fpfx[t];
        out->n_energy[t] = on.en_h[t];
        std::copy_n(eon.begin() + (ptrdiff_t)f0, on.en_h[t], out->energy + f0);
        for (int k = 0; k < 3; k++) {
            counts[k][t] = k < kinds ? fn[(size_t)k * T + t] : 0;
            std::copy_n(fon.begin() + (ptrdiff_t)((size_t)k * (size_t)total + f0), counts[k][t], lists[k] + f0);
        }
        out->n_chosen[t] = cn[t];
        std::copy_n(ch.begin() + (ptrdiff_t)((size_t)on.lists * f0), cn[t], out->chosen + 4 * f0);
    }
}

// sdsp_debug_beat_grid: beat_grid and download_results over uploaded consensus onsets and tempo
// estimates, laid out as Pipeline::onset_lists and seed_tempo leave them.
void Pipeline::debug_beat_grid(const uint32_t* onsets, const uint64_t* n_onsets, const uint64_t* frames,
                               const uint64_t* n_trim, const float* bpm, const float* conf, uint64_t n_tracks,
                               sdsp_debug_beat_out* out) {
    debug_tempo_map(onsets, n_onsets, frames, n_trim, bpm, conf, n_tracks, 0, nullptr, out);
}

// sdsp_debug_tempo_map: the same set-up and launches with Pipeline::tempo_map queued behind k_beat
// and read by download_results, as the analysis call does with a tempo map request.  maps == nullptr:
// sdsp_debug_beat_grid (no request); out == nullptr: the beat lists are not copied out.
void Pipeline::debug_tempo_map(const uint32_t* onsets, const uint64_t* n_onsets, const uint64_t* frames,
                               const uint64_t* n_trim, const float* bpm, const float* conf, uint64_t n_tracks,
                               uint32_t what, std::vector<TrackTm>* maps, sdsp_debug_beat_out* out) {
    if (const std::string why = check_supported(cfg_, sr_); !why.empty()) throw HipError(why);
    const size_t T = (size_t)n_tracks;
    const uint64_t lists = hpss_on() ? 4 : 3;
    TempoPassIn bin;
    bin.n_trim.assign(n_trim, n_trim + T);
    TempoPassOut bo;
    bo.fpfx.assign(1, 0);
    std::vector<uint64_t> coff(T);
    std::vector<int> cn(T);
    for (size_t t = 0; t < T; t++) {
        const uint64_t cap = std::max<uint64_t>(12 * (n_trim[t] / std::max<uint32_t>(sr_, 1) + 1) + 64, 3 * frames[t] + 8);
        if (n_onsets[t] > lists * frames[t] || n_onsets[t] > cap) throw std::invalid_argument("onset list too long");
        coff[t] = lists * bo.fpfx.back();
        cn[t] = (int)n_onsets[t];
        bo.fpfx.push_back(bo.fpfx.back() + frames[t]);
    }
    bo.total = bo.fpfx.back();
    std::vector<uint32_t> chosen((size_t)(lists * bo.total), 0);
    for (size_t t = 0, at = 0; t < T; at += (size_t)n_onsets[t], t++)
        std::copy_n(onsets + at, (size_t)n_onsets[t], chosen.begin() + (ptrdiff_t)coff[t]);
    Onsets on;
    on.d_chosen = c_.up("B.chosen", chosen);
    on.d_coff = c_.up("B.coff", coff);
    on.d_cn = c_.up("B.cn", cn);
    Tempo tp;
    tp.d_fbpm = c_.up("C.fbpm", std::vector<float>(bpm, bpm + T));
    tp.d_fconf = c_.up("C.fconf", std::vector<float>(conf, conf + T));
    if (maps) set_tempo_map(what, maps);
    const Beats bt = beat_grid(bin, bo, on, tp);
    const TempoMapQ tq = tempo_map(bin, on, tp, bt);
    const ResultsHost rh = download_results(bt, bin, bo, tq);
    if (maps) {
        maps->clear();
        for (size_t t = 0; t < T; t++) maps->push_back(track_tempo_map(rh, t, bpm[t], conf[t], 0));
    }
    if (!out) return;
    for (size_t t = 0; t < T; t++) {
        out->ok[t] = rh.bout[t].ok;
        out->n_beats[t] = rh.bout[t].n_beats;
        out->n_down[t] = rh.bout[t].n_down;
        out->stability[t] = rh.bout[t].stability;
    }
    std::copy(rh.beats_h.begin(), rh.beats_h.end(), out->beats);
    std::copy(rh.downs_h.begin(), rh.downs_h.end(), out->downs);
}

}  // namespace sdsp
