// pipeline_tempo.hip — the tempo path of a sub-batch (stages B and C of pipeline.hip's overview):
// tempo_pass and its stages (frame plan + STFT, features, novelty, tempograms, select), the final
// tempo's seed, the multi-resolution escalation, the percussive fallback and the legacy select.
#include "pipeline.hpp"

namespace sdsp {

namespace detail {
TempoPassIn subset(const TempoPassIn& base, const std::vector<int>& which) {
    TempoPassIn s;
    s.hop = base.hop;
    s.samples = base.samples;
    for (int i : which) {
        s.src_off.push_back(base.src_off[(size_t)i]);
        s.gain_h.push_back(base.gain_h[(size_t)i]);
        s.n_trim.push_back(base.n_trim[(size_t)i]);
    }
    return s;
}
}  // namespace detail

static uint64_t next_pow2(uint64_t n) {
    uint64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

void Pipeline::add_pass_times(const TempoPassOut& o) {
    times_.stft2048_ms += o.stft_ms;
    times_.stft2048_launches += o.stft_launch;
    times_.stft2048_frames += o.stft_frames;
    times_.stft2048_bytes += o.stft_bytes;
    times_.features_ms += o.feat_ms;
    times_.tempogram_ms += o.tempo_ms;
}

void Pipeline::tempo_pass(const std::string& tag, const TempoPassIn& in, TempoPassOut& o) {
    Timers tm;
    tm.init(d_);
    const PassPlan pl = pass_stft(tag, in, o, tm);
    tm.mark(1);
    const PassFeat pf = pass_features(tag, in, pl, o);
    pass_novelty(tag, in, pl, pf, o);
    tm.mark(2);
    const PassTg tg = pass_tempograms(tag, in, pl, pf, o);
    pass_select(tag, in, pl, tg, o);
    tm.mark(3);
    if (in.dbg) {
        in.dbg->fp = pf.fp;
        in.dbg->tg = tg;
    }
    c_.sync();
    o.stft_ms = tm.ms(0, 1);
    o.feat_ms = tm.ms(1, 2);
    o.tempo_ms = tm.ms(2, 3);
}

// Frames per pass-track, the plan uploads, and the spectrogram the features read: the pass's own
// STFT, a precomputed one (mags_in), or rows shared with the hop-512 pass (reuse).
PassPlan Pipeline::pass_stft(const std::string& tag, const TempoPassIn& in, TempoPassOut& o, Timers& tm) {
    PassPlan pl;
    const int P_T = pl.P_T = (int)in.src_off.size();
    const int FS = fs_, hop = in.hop;
    // frames per feature tile: the walk's, or the gather's 256 when the pass has no walk of its own
    const uint64_t tstep = in.sfx_in ? 256 : in.sfx4_out ? FT_STEP_X4 : FT_STEP;
    o.fpfx.assign((size_t)P_T + 1, 0);
    pl.tpfx.assign((size_t)P_T + 1, 0);
    o.active_h.assign((size_t)P_T, 0);
    for (int t = 0; t < P_T; t++) {
        const uint64_t n = in.n_trim[(size_t)t];
        const uint64_t F = n >= (uint64_t)FS ? (n - FS) / (uint64_t)hop + 1 : 0;
        o.fpfx[(size_t)t + 1] = o.fpfx[(size_t)t] + F;
        pl.tpfx[(size_t)t + 1] = pl.tpfx[(size_t)t] + (F + tstep - 1) / tstep;
        o.active_h[(size_t)t] = F >= 2;
    }
    const uint64_t total = o.total = o.fpfx[(size_t)P_T];
    o.d_fpfx = c_.up(tag + "fpfx", o.fpfx);
    pl.d_tpfx = c_.up(tag + "tpfx", pl.tpfx);
    uint64_t* d_src = c_.up(tag + "src", in.src_off);
    float* d_gain = c_.up(tag + "gain", in.gain_h);
    o.active = c_.up(tag + "active", o.active_h);
    FftTables& tb = d_.tables(FS, true);
    tm.mark(0);
    uint64_t stft_frames = 0;
    if (in.mags_in) {
        o.mags = const_cast<float*>(in.mags_in);
        o.fmax = const_cast<float*>(in.fmax_in);
    } else if (in.reuse == 1) {  // hop 1024: nothing to compute
        o.mags = nullptr;
        o.fmax = nullptr;
        pl.rm = RowMap{in.base_mags, in.base_mags, in.base_fmax, in.base_fmax, c_.up(tag + "brow", in.base_row0), nullptr,
                       2, 4, 4};
    } else if (in.reuse == 2) {  // hop 256: the odd frames, as a hop-512 STFT from sample 256
        std::vector<uint64_t> opfx((size_t)P_T + 1, 0), osrc((size_t)P_T);
        for (int t = 0; t < P_T; t++) {
            opfx[(size_t)t + 1] = opfx[(size_t)t] + (o.fpfx[(size_t)t + 1] - o.fpfx[(size_t)t]) / 2;
            osrc[(size_t)t] = in.src_off[(size_t)t] + (uint64_t)hop;
        }
        stft_frames = opfx[(size_t)P_T];
        o.mags = c_.dev<float>(tag + "mags", std::max<uint64_t>(stft_frames, 1) * s2_);
        // no frame maxima without the spectral flux, unless they also select the kernel (at a frame
        // size of 8192 the tempo path's STFT is the general kernel only with them)
        const bool fm = !in.no_flux || stft_general(FS, true) != stft_general(FS, false);
        o.fmax = fm ? c_.dev<float>(tag + "fmax", std::max<uint64_t>(stft_frames, 1)) : nullptr;
        uint64_t* d_opfx = c_.up(tag + "opfx", opfx);
        const std::vector<uint64_t> ostr = stft_strips(opfx);
        launch_stft(FS, fm, in.samples, d_opfx, P_T, stft_frames, c_.up(tag + "osrc", osrc), d_gain, 2 * hop,
                    tb.window.as<float>(), stft_twp(tb, FS, fm), stft_rtp(tb, FS, fm), o.mags, d_opfx, s2_, o.fmax,
                    d_.stream, c_.up(tag + "ostrip", ostr), ostr.back(), c_.dev<uint32_t>(tag + "redo", stft_frames + 1));
        SDSP_HIP_CHECK(hipGetLastError());
        pl.rm = RowMap{in.base_mags, o.mags, in.base_fmax, o.fmax, c_.up(tag + "brow", in.base_row0), d_opfx, 0, 1, 1};
    } else {
        o.mags = c_.dev<float>(tag + "mags", total * s2_);
        o.fmax = c_.dev<float>(tag + "fmax", total);
        const std::vector<uint64_t> str = stft_strips(o.fpfx);
        launch_stft(FS, true, in.samples, o.d_fpfx, P_T, total, d_src, d_gain, hop, tb.window.as<float>(),
                    stft_twp(tb, FS, true), stft_rtp(tb, FS, true), o.mags, o.d_fpfx, s2_, o.fmax, d_.stream,
                    c_.up(tag + "strip", str), str.back(), c_.dev<uint32_t>(tag + "redo", total + 1));
        SDSP_HIP_CHECK(hipGetLastError());
        stft_frames = total;
    }
    if (in.mags_in || in.reuse == 0) pl.rm = RowMap{o.mags, o.mags, o.fmax, o.fmax, o.d_fpfx, nullptr, 1, 2, 2};
    o.stft_launch = stft_frames ? 1 : 0;
    o.stft_frames = stft_frames;
    if (stft_frames) {
        double inb = 0;
        for (int t = 0; t < P_T; t++) inb += 4.0 * (double)in.n_trim[(size_t)t];
        o.stft_bytes = inb + 4.0 * (double)stft_frames * (double)nb_;
    }
    return pl;
}

PassFeat Pipeline::pass_features(const std::string& tag, const TempoPassIn& in, const PassPlan& pl, TempoPassOut& o) {
    PassFeat pf;
    const int B = nb_;
    const uint64_t total = o.total;
    pf.configured = band_configured(cfg_);
    pf.mel_on = pf.configured && cfg_.enable_tempogram_mel_novelty;
    FeatParams& fp = pf.fp = feat_params(cfg_, sr_, B, s2_);
    if (in.sfx_in) {  // escalation hop 1024: nothing to walk (TempoPassIn)
        const TempoPassOut& b = *in.feat512;
        o.E = c_.dev<float>(tag + "E", 4 * total);
        o.H = c_.dev<float>(tag + "H", 4 * total);
        o.SFX = in.sfx_in;
        o.MEL = c_.dev<float>(tag + "MEL", std::max<uint64_t>(total * (uint64_t)std::max(fp.n_mels, 1), 1));
        launch_features_gather2(o.d_fpfx, pl.rm.rowA0, pl.P_T, pl.d_tpfx, pl.tpfx[(size_t)pl.P_T], fp.n_mels, b.E, b.H, b.MEL,
                                b.total, o.E, o.H, o.MEL, total, d_.stream);
        SDSP_HIP_CHECK(hipGetLastError());
        return pf;
    }
    std::string merr;
    MelTable mt = mel_table(sr_, B, (int)cfg_.tempogram_mel_n_mels, cfg_.tempogram_mel_fmin_hz, cfg_.tempogram_mel_fmax_hz,
                            &merr);
    if (!merr.empty()) throw HipError(merr);
    std::vector<MelPlan> mplan = mel_plan(mt, B, &merr);
    if (!merr.empty()) throw HipError(merr);
    MelPlan* d_mplan = c_.up(tag + "melplan", mplan);
    std::vector<int> cf;
    std::vector<MelChunk> mc;
    feat_chunk_tables(fp, mplan, &cf, &mc);
    fp.chunk_flags = c_.up(tag + "ftchunk", cf);
    fp.mel_chunks = c_.up(tag + "ftmelchunk", mc);
    o.E = c_.dev<float>(tag + "E", 4 * total);
    o.H = c_.dev<float>(tag + "H", 4 * total);
    o.SFX = c_.dev<float>(tag + "SFX", 4 * total);
    o.MEL = c_.dev<float>(tag + "MEL", std::max<uint64_t>(total * (uint64_t)std::max(fp.n_mels, 1), 1));
    if (in.no_flux) {
        launch_features_esc(pl.rm, o.d_fpfx, pl.d_tpfx, pl.P_T, pl.tpfx[(size_t)pl.P_T], fp, d_mplan, o.E, o.H, o.SFX, o.MEL,
                            total, in.sfx4_fpfx, in.sfx4_out, in.sfx4_total, d_.stream);
        SDSP_HIP_CHECK(hipGetLastError());
        return pf;
    }
    o.SFO = c_.dev<float>(tag + "SFO", total);
    launch_features(pl.rm, o.d_fpfx, pl.d_tpfx, pl.P_T, pl.tpfx[(size_t)pl.P_T], fp, d_mplan, o.E, o.H, o.SFX, o.SFO,
                    o.MEL, total, d_.stream);
    SDSP_HIP_CHECK(hipGetLastError());
    return pf;
}

void Pipeline::pass_novelty(const std::string& tag, const TempoPassIn& in, const PassPlan& pl, const PassFeat& pf,
                            TempoPassOut& o) {
    const int P_T = pl.P_T;
    const uint64_t total = o.total;
    NovParams np = nov_params(cfg_, pf.configured);
    for (int v = 0; v < 4; v++) np.band_on[v] = pf.fp.band_on[v];
    float* scratch = c_.dev<float>(tag + "novscr", 8 * std::max<uint64_t>(total, 1));
    o.nov = c_.dev<float>(tag + "nov", NVAR * std::max<uint64_t>(total, 1));
    o.nov_sum = c_.dev<float>(tag + "novsum", NVAR * (size_t)std::max(P_T, 1));
    launch_novelty(o.E, o.H, o.SFX, o.d_fpfx, P_T, total, np, scratch, o.nov, o.nov_sum, o.MEL, pf.fp.n_mels,
                   (int)std::max<uint64_t>(cfg_.tempogram_mel_max_filter_bins, 1), pf.mel_on,
                   c_.dev<unsigned int>(tag + "melmax", (size_t)std::max(P_T, 1)), d_.stream);
    SDSP_HIP_CHECK(hipGetLastError());
    o.nov_mr = o.nov;
    if (in.mr_nov && !pf.configured) {
        // without the auxiliary variants the tempogram's novelty uses combined_novelty's defaults,
        // but multi-resolution's hop-512 novelty still takes the configured weights
        // (multi_resolution.rs:680-694): the full-band variant again, with those
        NovParams nm = nov_params(cfg_, true);
        nm.band_on[0] = np.band_on[0];
        o.nov_mr = c_.dev<float>(tag + "novmr", NVAR * std::max<uint64_t>(total, 1));
        launch_novelty(o.E, o.H, o.SFX, o.d_fpfx, P_T, total, nm, scratch, o.nov_mr,
                       c_.dev<float>(tag + "novmrsum", NVAR * (size_t)std::max(P_T, 1)), o.MEL, 0, 1, false,
                       c_.dev<unsigned int>(tag + "melmax", (size_t)std::max(P_T, 1)), d_.stream);
        SDSP_HIP_CHECK(hipGetLastError());
    }
}

// ACF and FFT tempograms of the items (track, variant) of the active tracks; the FFT ones grouped
// by size P
PassTg Pipeline::pass_tempograms(const std::string& tag, const TempoPassIn& in, const PassPlan& pl, const PassFeat& pf,
                                 const TempoPassOut& o) {
    PassTg tg;
    const int P_T = pl.P_T, hop = in.hop;
    const uint64_t total = o.total;
    for (int v = 0; v < 4; v++) tg.present[v] = pf.fp.band_on[v];
    tg.present[4] = pf.mel_on;
    std::vector<int>& items = tg.items;
    for (int t = 0; t < P_T; t++)
        if (o.active_h[(size_t)t])
            for (int v = 0; v < NVAR; v++)
                if (tg.present[v]) items.push_back(t * NVAR + v);
    // ACF
    std::vector<float> gb;
    std::vector<int> gl;
    acf_grid(sr_, hop, cfg_.min_bpm, cfg_.max_bpm, cfg_.bpm_resolution, &gb, &gl);
    const int NB = tg.NB = (int)gb.size();
    if (NB > 512) throw HipError("autocorrelation grid larger than 512 BPMs");
    float* d_gb = c_.up(tag + "acfgb", gb);
    int* d_gl = c_.up(tag + "acfgl", gl);
    int* d_items = c_.up(tag + "items", items);
    const size_t n_it = items.size();
    tg.acf_bpm = c_.dev<float>(tag + "acfb", std::max<size_t>(n_it, 1) * (size_t)NB);
    tg.acf_str = c_.dev<float>(tag + "acfs", std::max<size_t>(n_it, 1) * (size_t)NB);
    launch_acf_tempogram(d_items, (int)n_it, o.nov, o.d_fpfx, total, d_gb, d_gl, NB, tg.acf_bpm, tg.acf_str, d_.stream);
    SDSP_HIP_CHECK(hipGetLastError());
    // FFT tempograms grouped by P
    tg.fft_off.assign(n_it, 0);
    tg.fft_k.assign(n_it, 0);
    tg.fft_k_track.assign((size_t)P_T, 0);
    std::map<uint64_t, std::vector<int>> byP;  // P -> item positions
    for (size_t i = 0; i < n_it; i++) {
        const int t = items[i] / NVAR;
        const uint64_t L = o.fpfx[(size_t)t + 1] - o.fpfx[(size_t)t] - 1;
        byP[next_pow2(L)].push_back((int)i);
    }
    uint64_t fcur = 0;
    std::map<uint64_t, FftTgParams> prm;
    for (auto& kv : byP) {
        FftTgParams& p = prm[kv.first];
        p.P = (int)kv.first;
        fft_bins(sr_, hop, kv.first, cfg_.min_bpm, cfg_.max_bpm, &p.b_lo, &p.K, &p.fres);
        // k_fft_tempogram's in-place LDS FFT up to P = 8192 (32 KB of LDS); larger P (3-min tracks
        // at hop 512 have P = 16384) through L2-resident global scratch.  A 64 KB LDS workgroup
        // waits for a CU that no key-stream STFT workgroup occupies, which the concurrent pipeline
        // seldom offers: its launches stretched from 0.3 ms to 19 ms (round 4)
#ifndef SDSP_FFT_TG_LDS_MAX
#define SDSP_FFT_TG_LDS_MAX 8192
#endif
        p.lds = kv.first <= SDSP_FFT_TG_LDS_MAX ? 1 : 0;
        uint64_t K2 = 1;
        while (K2 < (uint64_t)p.K) K2 <<= 1;
        if (p.K > 0 && K2 > kv.first / 2) throw HipError("FFT tempogram: too many in-range bins for the key buffer");
        for (int i : kv.second) {
            tg.fft_off[(size_t)i] = fcur;
            fcur += (uint64_t)p.K;
            tg.fft_k[(size_t)i] = p.K;
            tg.fft_k_track[(size_t)(items[(size_t)i] / NVAR)] = p.K;
        }
    }
    tg.fft_bpm = c_.dev<float>(tag + "fftb", std::max<uint64_t>(fcur, 1));
    tg.fft_pow = c_.dev<float>(tag + "fftp", std::max<uint64_t>(fcur, 1));
    for (auto& kv : byP) {
        const FftTgParams& p = prm[kv.first];
        if (p.K == 0) continue;
        std::vector<int> sub;
        std::vector<uint64_t> offs;
        for (int i : kv.second) {
            sub.push_back(items[(size_t)i]);
            offs.push_back(tg.fft_off[(size_t)i]);
        }
        int* d_sub = c_.up(tag + "fsub" + std::to_string(kv.first), sub);
        uint64_t* d_offs = c_.up(tag + "foff" + std::to_string(kv.first), offs);
        FftTables& ft = d_.tables((int)kv.first, false);
        cx* gscr = nullptr;
        if (!p.lds) gscr = c_.dev<cx>(tag + "fgscr", sub.size() * (size_t)kv.first);
        launch_fft_tempogram(d_sub, (int)sub.size(), P_T, o.nov, o.nov_sum, o.d_fpfx, total, p, ft.tw.as<cx>(),
                             ft.rt.as<cx>(), gscr, d_offs, tg.fft_bpm, tg.fft_pow, d_.stream);
        SDSP_HIP_CHECK(hipGetLastError());
    }
    return tg;
}

void Pipeline::pass_select(const std::string& tag, const TempoPassIn& in, const PassPlan& pl, const PassTg& tg,
                           TempoPassOut& o) {
    const int P_T = pl.P_T;
    // per (track, variant) offsets for the selector
    SelLists sl;
    sl.fo.assign((size_t)P_T * NVAR, 0);
    sl.ao.assign((size_t)P_T * NVAR, 0);
    for (size_t i = 0; i < tg.items.size(); i++) {
        sl.fo[(size_t)tg.items[i]] = tg.fft_off[i];
        sl.ao[(size_t)tg.items[i]] = (uint64_t)i * (uint64_t)tg.NB;
    }
    sl.fft_k = tg.fft_k_track;
    sl.fft_bpm = tg.fft_bpm;
    sl.fft_pow = tg.fft_pow;
    sl.acf_bpm = tg.acf_bpm;
    sl.acf_str = tg.acf_str;
    for (int v = 0; v < NVAR; v++) sl.present[v] = tg.present[v];
    sl.NB = tg.NB;
    select_lists(tag, P_T, sl, in.top_n, in.gate, in.cand_cap, o);
}

// pass_select from its offset tables on (o.active is the pass's); sdsp_debug_tempo_select enters here
void Pipeline::select_lists(const std::string& tag, int P_T, const SelLists& sl, int top_n, int gate, int cand_cap,
                            TempoPassOut& o) {
    uint64_t* d_fo = c_.up(tag + "selfo", sl.fo);
    uint64_t* d_ao = c_.up(tag + "selao", sl.ao);
    int* d_fk = c_.up(tag + "selfk", sl.fft_k);
    const SelParams sp = sel_params(cfg_, sl.present, sl.NB, top_n, gate);
    o.est = c_.dev<TempoEst>(tag + "est", (size_t)std::max(P_T, 1));
    o.cand = c_.dev<float>(tag + "cand", (size_t)std::max(P_T, 1) * (size_t)cand_cap * 4);
    launch_tempo_select(P_T, o.active, sl.fft_bpm, sl.fft_pow, d_fo, d_fk, sl.acf_bpm, sl.acf_str, d_ao, sp, o.est,
                        o.cand, cand_cap, d_.stream);
    SDSP_HIP_CHECK(hipGetLastError());
}

// Final tempo per track (tempogram -> legacy -> 0; legacy is never consulted on the default path,
// see DESIGN.md "legacy estimator"): the base pass's estimates, and the tracks to escalate.
Tempo Pipeline::seed_tempo(const Front& f, const std::vector<TempoEst>& best, const Onsets& on,
                           std::vector<TrackRes>& res) {
    const int NR = (int)f.R.size();
    Tempo tp;
    tp.fbpm_h.assign((size_t)NR, 0.0f);
    tp.fconf_h.assign((size_t)NR, 0.0f);
    tp.used.assign((size_t)NR, 0);
    tp.perc_cands.assign((size_t)NR, {});
    tp.perc_took.assign((size_t)NR, 0);
    for (int i = 0; i < NR; i++) {
        TrackRes& r = res[f.slot[(size_t)i]];
        const TempoEst& e = best[(size_t)i];
        r.onset_consensus = on.en_h[(size_t)i] > 0 ? 1.0f : 0.0f;
        if (!e.ok || !tg_on()) continue;
        tp.fbpm_h[(size_t)i] = e.bpm;
        tp.fconf_h[(size_t)i] = e.conf;
        if (mr_on()) {
            r.mr_trig = (int8_t)(e.ambiguous != 0);
            r.mr_used = 0;
            r.perc_trig = (int8_t)(e.ambiguous && e.trap_low);
            if (e.ambiguous) tp.E.push_back(i);
        }
    }
    return tp;
}

// C: escalation (multi_resolution.rs:205-901) of the ambiguous tracks tp.E, then the estimates as
// they stand back on the host.
void Pipeline::escalate(const Front& f, const TempoPassIn& bin, const TempoPassOut& bo, const std::vector<TempoEst>& best,
                        Tempo& tp, std::vector<TrackDbg>& tdbg, std::vector<TrackRes>& res) {
    const int NR = (int)f.R.size();
    const std::vector<int>& E = tp.E;
    tp.d_fbpm = c_.up("B.fbpm", tp.fbpm_h);
    tp.d_fconf = c_.up("B.fconf", tp.fconf_h);
    tp.d_used = c_.up("B.used", tp.used);
    if (mr_on() && !E.empty()) {
        const int NE = (int)E.size();
        const int top_k = (int)std::max<uint64_t>(cfg_.tempogram_multi_res_top_k, 1);
        const int aux_k = std::min(std::max(top_k * 4, 25), 200);
        TempoPassIn ein = subset(bin, E);
        // multi_resolution.rs:237-239 recomputes the STFT at hops 256, 512 and 1024 of the trimmed
        // samples.  At hop_size 512 the base pass is the hop-512 one; otherwise the escalated
        // tracks get their own hop-512 pass (top_k candidates, :273) first.  The hop-256 and
        // hop-1024 passes read the hop-512 rows they share with it (SDSP_NO_ROW_REUSE: control).
        const bool own512 = bin.hop != 512;
        TempoPassOut o256, o512, o1024;
        if (own512) {
            ein.hop = 512;
            ein.top_n = top_k;
            ein.cand_cap = top_k;
            ein.mr_nov = true;
            tempo_pass("C512.", ein, o512);
            ein.mr_nov = false;
        }
        const TempoPassOut& b512 = own512 ? o512 : bo;
        ein.base_mags = b512.mags;
        ein.base_fmax = b512.fmax;
        for (int k = 0; k < NE; k++) ein.base_row0.push_back(b512.fpfx[own512 ? (size_t)k : (size_t)E[(size_t)k]]);
        ein.top_n = aux_k;
        ein.cand_cap = aux_k;
        const bool reuse_on = test_hooks().no_row_reuse.load() == 0;  // the tests' control (sdsp_debug_set_schedule)
        // With the shared rows, the hop-256 feature walk also folds the hop-1024 SuperFlux (its
        // frame j is hop-256 frame 4 j) and the hop-1024 pass takes E / H / MEL from the hop-512
        // pass (frame 2 j), so it launches no features; neither computes the spectral flux, which
        // only the base pass's onsets read.  The complete passes stay as the control, for the
        // debug dumps, and for a SuperFlux width the fused walk is not built for.
        const bool fused = reuse_on && !dbg_on() && feat_params(cfg_, sr_, nb_, s2_).K == 4;
        ein.hop = 256;
        ein.reuse = reuse_on ? 2 : 0;
        if (fused) {
            std::vector<uint64_t> fpfx4((size_t)NE + 1, 0);
            for (int k = 0; k < NE; k++) {
                const uint64_t n = ein.n_trim[(size_t)k];
                fpfx4[(size_t)k + 1] = fpfx4[(size_t)k] + (n >= (uint64_t)fs_ ? (n - (uint64_t)fs_) / 1024 + 1 : 0);
            }
            ein.no_flux = true;
            ein.sfx4_total = fpfx4[(size_t)NE];
            ein.sfx4_fpfx = c_.up("C256.fpfx4", fpfx4);
            ein.sfx4_out = c_.dev<float>("C1024.SFX", 4 * ein.sfx4_total);
        }
        tempo_pass("C256.", ein, o256);
        ein.hop = 1024;
        ein.reuse = reuse_on ? 1 : 0;
        if (fused) {
            ein.sfx_in = ein.sfx4_out;
            ein.sfx4_out = nullptr;
            ein.feat512 = &b512;
        }
        tempo_pass("C1024.", ein, o1024);
        add_pass_times(o256);
        add_pass_times(o1024);
        if (own512) add_pass_times(o512);
        std::vector<TempoEst> e256 = c_.down(o256.est, (size_t)NE), e1024 = c_.down(o1024.est, (size_t)NE);
        MrFuse mf;
        mf.n256.assign((size_t)NE, 0);
        mf.n1024.assign((size_t)NE, 0);
        mf.n512.assign((size_t)NR, 0);
        std::vector<int> &n256 = mf.n256, &n1024 = mf.n1024, &n512 = mf.n512;  // the fusion's count tables
        for (int k = 0; k < NE; k++) {
            n256[(size_t)k] = e256[(size_t)k].ok ? e256[(size_t)k].n_cands : -1;
            n1024[(size_t)k] = e1024[(size_t)k].ok ? e1024[(size_t)k].n_cands : -1;
        }
        if (own512) {  // E order; -1: the hop-512 tempogram failed (multi_resolution returns Err)
            const std::vector<TempoEst> e512 = c_.down(o512.est, (size_t)NE);
            n512.assign((size_t)NE, 0);
            for (int k = 0; k < NE; k++)
                n512[(size_t)k] = e512[(size_t)k].ok ? std::min(e512[(size_t)k].n_cands, top_k) : -1;
            if (cfg_.emit_tempogram_candidates) {
                tp.c512_h = c_.down(o512.cand, (size_t)NE * (size_t)top_k * 4);
                tp.n512_own = n512;
                tp.c512_cap = top_k;
            }
        } else {
            for (int i = 0; i < NR; i++) n512[(size_t)i] = std::min(best[(size_t)i].n_cands, top_k);
        }
        mf.c256 = o256.cand;
        mf.c512 = b512.cand;
        mf.c1024 = o1024.cand;
        mf.cap_aux = ein.cand_cap;
        mf.cap_base = bin.cand_cap;
        mf.own512 = own512;
        mf.base_est = bo.est;
        mf.nov512 = b512.nov_mr;
        mf.fpfx512 = b512.d_fpfx;
        mf.want_dbg = dbg_on();
        fuse_multires(E, NR, mf, tp);
        if (dbg_on())
            debug_multires(E, own512, mf.cap512, ein.cand_cap, (size_t)(own512 ? NE : NR), o256, b512, o1024, n256, n512,
                           n1024, tp.d_mr_all, mf.d_mdbg, tdbg);
        for (int i : E)
            if (tp.used[(size_t)i]) res[f.slot[(size_t)i]].mr_used = 1;
    }
    tp.epos.assign((size_t)NR, -1);
    for (size_t k = 0; k < E.size(); k++) tp.epos[(size_t)E[k]] = (int)k;
    tempo_down(NR, tp);
}

// escalate's tail (sdsp_debug_multires enters here): the count tables and the item list up,
// k_multires over the three hops' lists, and which tracks took the multi-resolution estimate back.
// tp.d_used / d_fbpm / d_fconf hold the base pass's values; the kernel overwrites the accepted tracks'.
void Pipeline::fuse_multires(const std::vector<int>& E, int NR, MrFuse& m, Tempo& tp) {
    const int NE = (int)E.size();
    const int top_k = (int)std::max<uint64_t>(cfg_.tempogram_multi_res_top_k, 1);
    int* d_n256 = c_.up("C.n256", m.n256);
    int* d_n1024 = c_.up("C.n1024", m.n1024);
    int* d_n512 = c_.up("C.n512", m.n512);
    int* d_E = c_.up("C.E", E);
    const int cap512 = m.cap512 = m.own512 ? top_k : m.cap_base;
    for (int n : m.n512)  // k_tempo_select writes at most SEL_MAXC = MR_HYP_MAX
        if (std::min(top_k, n) > MR_HYP_MAX) throw HipError("multi-resolution fusion: more than 1024 hop-512 candidates");
    TempoEst* d_mr = tp.d_mr_all = c_.dev<TempoEst>("C.mr", (size_t)NE);
    MrDbg* d_mdbg = m.d_mdbg = m.want_dbg ? c_.dev<MrDbg>("C.mrdbg", (size_t)NE) : nullptr;
    launch_multires(d_E, NE, m.c256, d_n256, m.c512, d_n512, m.c1024, d_n1024, m.cap_aux, cap512, m.cap_aux, m.base_est,
                    m.nov512, m.fpfx512, mr_params(cfg_, sr_, top_k, m.own512), d_mr, tp.d_used, tp.d_fbpm, tp.d_fconf,
                    d_.stream, d_mdbg);
    SDSP_HIP_CHECK(hipGetLastError());
    tp.used = c_.down(tp.d_used, (size_t)NR);
}

// the estimates as they stand back on the host
void Pipeline::tempo_down(int NR, Tempo& tp) {
    tp.fbpm_h = c_.down(tp.d_fbpm, (size_t)NR);
    tp.fconf_h = c_.down(tp.d_fconf, (size_t)NR);
}

// C': percussive tempogram fallback (src/lib.rs:582-683) for the tracks in the low trap zone: the
// tempo pass over HPSS's percussive spectrogram, taken where perc_better accepts it.
void Pipeline::perc_fallback(const Front& f, const TempoPassIn& bin, const TempoPassOut& bo,
                             const std::vector<TempoEst>& best, const Hpss& hp, Tempo& tp, std::vector<TrackRes>& res) {
    const int NR = (int)f.R.size();
    hipStream_t st = d_.stream;
    std::vector<int> Q;  // positions in R
    for (int i = 0; i < NR; i++) {
        const TempoEst& e = best[(size_t)i];
        if (!e.ok) continue;
        res[f.slot[(size_t)i]].perc_used = 0;
        if (e.ambiguous && e.trap_low) Q.push_back(i);
    }
    const int NQ = (int)Q.size();
    if (NQ == 0 || !hp.d_P0) return;
    TempoPassIn pin = subset(bin, Q);
    std::vector<uint64_t> qpfx(1, 0);
    for (int i : Q) qpfx.push_back(qpfx.back() + (bo.fpfx[(size_t)i + 1] - bo.fpfx[(size_t)i]));
    pin.top_n = bin.top_n;
    pin.cand_cap = bin.cand_cap;
    if (hpss_on()) {  // HPSS ran on every track: gather Q's rows (its items are Q otherwise)
        float* pq = c_.dev<float>("P.in", std::max<uint64_t>(qpfx.back(), 1) * s2_);
        float* pm = c_.dev<float>("P.inmax", std::max<uint64_t>(qpfx.back(), 1));
        for (int k = 0; k < NQ; k++) {
            const uint64_t F = qpfx[(size_t)k + 1] - qpfx[(size_t)k], r0 = bo.fpfx[(size_t)Q[(size_t)k]];
            if (F == 0) continue;
            SDSP_HIP_CHECK(hipMemcpyAsync(pq + qpfx[(size_t)k] * s2_, hp.d_P0 + r0 * s2_, F * s2_ * sizeof(float),
                                          hipMemcpyDeviceToDevice, st));
            SDSP_HIP_CHECK(hipMemcpyAsync(pm + qpfx[(size_t)k], hp.d_hfmax + r0, F * sizeof(float),
                                          hipMemcpyDeviceToDevice, st));
        }
        pin.mags_in = pq;
        pin.fmax_in = pm;
    } else {
        pin.mags_in = hp.d_P0;
        pin.fmax_in = hp.d_hfmax;
    }
    TempoPassOut po;
    tempo_pass("P.", pin, po);
    times_.features_ms += po.feat_ms;
    times_.tempogram_ms += po.tempo_ms;
    std::vector<TempoEst> pe = c_.down(po.est, (size_t)NQ);
    std::vector<TempoEst> mr_h;
    if (tp.d_mr_all) mr_h = c_.down(tp.d_mr_all, tp.E.size());
    std::vector<float> pc_h;
    if (cfg_.emit_tempogram_candidates) pc_h = c_.down(po.cand, (size_t)NQ * (size_t)pin.cand_cap * 4);
    bool changed = false;
    for (int k = 0; k < NQ; k++) {
        const int i = Q[(size_t)k];
        const TempoEst& p = pe[(size_t)k];
        if (!p.ok) continue;  // "Percussive tempogram fallback failed" -> not used
        const TempoEst& b = best[(size_t)i];
        const int ca = (tp.used[(size_t)i] && tp.epos[(size_t)i] >= 0) ? mr_h[(size_t)tp.epos[(size_t)i]].agree : b.agree;
        if (!perc_better(p, tp.fbpm_h[(size_t)i], tp.fconf_h[(size_t)i], ca, b)) continue;
        tp.fbpm_h[(size_t)i] = p.bpm;
        tp.fconf_h[(size_t)i] = p.conf;
        res[f.slot[(size_t)i]].perc_used = 1;
        tp.perc_took[(size_t)i] = 1;
        changed = true;
        if (cfg_.emit_tempogram_candidates)
            tp.perc_cands[(size_t)i].assign(pc_h.begin() + (long)((size_t)k * (size_t)pin.cand_cap * 4),
                                            pc_h.begin() + (long)((size_t)k * (size_t)pin.cand_cap * 4 +
                                                                  (size_t)p.n_cands * 4));
    }
    if (changed) {
        SDSP_HIP_CHECK(hipMemcpyAsync(tp.d_fbpm, c_.keep_bytes(tp.fbpm_h), (size_t)NR * sizeof(float),
                                      hipMemcpyHostToDevice, st));
        SDSP_HIP_CHECK(hipMemcpyAsync(tp.d_fconf, c_.keep_bytes(tp.fconf_h), (size_t)NR * sizeof(float),
                                      hipMemcpyHostToDevice, st));
    }
}

// C'': the legacy estimate of every track from its beat-tracking onsets (on_legacy == on_beat,
// src/lib.rs:176-329), then force_legacy_bpm / enable_bpm_fusion's choice (src/lib.rs:814-892).
// ACF scratch: M = next_pow2(2L) complex per buffer, L <= (n_trim - 1) / hop + 1.
void Pipeline::legacy_select(const Front& f, const TempoPassIn& bin, const Onsets& on, Tempo& tp,
                             std::vector<TrackRes>& res) {
    hipStream_t st = d_.stream;
    const int NR = (int)f.R.size();
    const uint64_t hop = (uint64_t)bin.hop;
    std::vector<uint64_t> soff((size_t)NR), scap((size_t)NR);
    uint64_t tot = 0, mmax = 4;
    for (int i = 0; i < NR; i++) {
        const uint64_t n = bin.n_trim[(size_t)i];
        const uint64_t M = next_pow2(2 * ((n ? n - 1 : 0) / hop + 1));
        scap[(size_t)i] = M;
        soff[(size_t)i] = tot;
        tot += 2 * M;
        mmax = std::max(mmax, M);
    }
    FftTables& tb = d_.tables((int)(2 * mmax), false);
    cx* scr = c_.dev<cx>("G.acf", tot);
    LegacyOut* d_lo = c_.dev<LegacyOut>("G.out", (size_t)NR);
    launch_legacy(on.d_chosen, on.d_coff, on.d_cn, NR, c_.up("G.soff", soff), c_.up("G.scap", scap), scr, tb.tw.as<cx>(),
                  (int)mmax, legacy_params(cfg_, sr_, (int)hop), d_lo, st);
    SDSP_HIP_CHECK(hipGetLastError());
    const std::vector<LegacyOut> lo = c_.down(d_lo, (size_t)NR);
    for (int i = 0; i < NR; i++) {
        TrackRes& r = res[f.slot[(size_t)i]];
        const LegacyOut& l = lo[(size_t)i];
        if (l.ok < 0) {  // estimate_bpm_with_guardrails(...)? propagates (src/lib.rs:315, 324)
            r.status = SDSP_ERR_PROCESSING;
            r.err = l.ok == -1 ? "Processing error: Signal too short for autocorrelation"
                               : "Processing error: legacy BPM scratch too small";
            continue;
        }
        const bool has = l.ok > 0;
        float& bpm = tp.fbpm_h[(size_t)i];
        float& conf = tp.fconf_h[(size_t)i];
        if (cfg_.force_legacy_bpm || bpm <= 0.0f) {  // fusion without a tempogram BPM: legacy's
            bpm = has ? l.bpm : 0.0f;
            conf = has ? l.conf : 0.0f;
            continue;
        }
        // fusion: the tempogram BPM is kept; legacy only moves its confidence
        const float t_bpm = bpm;
        const float l_bpm = has ? l.bpm : 0.0f;
        const float l_conf = sd_clampf(has ? l.conf : 0.0f, 0.0f, 1.0f);
        float c = sd_clampf(conf, 0.0f, 1.0f);
        bool agree = false;
        if (l_bpm > 0.0f) {
            const float d[5] = {sd_absf(l_bpm - t_bpm), sd_absf(l_bpm - (t_bpm * 0.5f)), sd_absf(l_bpm - (t_bpm * 2.0f)),
                                sd_absf(l_bpm - (t_bpm * (2.0f / 3.0f))), sd_absf(l_bpm - (t_bpm * (3.0f / 2.0f)))};
            for (float v : d) agree |= v <= 2.0f;
        }
        if (agree)
            c = sd_clampf(c + 0.12f * l_conf, 0.0f, 1.0f);
        else if (l_bpm > 0.0f)
            c = sd_clampf(c * 0.90f, 0.0f, 1.0f);
        conf = c;
    }
    SDSP_HIP_CHECK(hipMemcpyAsync(tp.d_fbpm, c_.keep_bytes(tp.fbpm_h), (size_t)NR * sizeof(float), hipMemcpyHostToDevice, st));
    SDSP_HIP_CHECK(hipMemcpyAsync(tp.d_fconf, c_.keep_bytes(tp.fconf_h), (size_t)NR * sizeof(float), hipMemcpyHostToDevice, st));
}

}  // namespace sdsp
