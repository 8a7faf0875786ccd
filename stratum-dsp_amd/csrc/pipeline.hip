// pipeline.hip — analyze_audio() for a batch of tracks on one MI355X (reference src/lib.rs:86-1635).
//
// Per sub-batch (sized to an HBM budget; Pipeline::run), the host plans ragged per-track frame
// ranges and Pipeline::sub_batch launches, one method per stage:
//   A  front: peak/gain, silence RMS, trim                -> host reads trim bounds (sync 1)
//   E  launch_key (pipeline_key.hip), forked onto the key stream: STFT 8192/512 (key_stft_frame_size
//      / hop; the tempo path's frame_size / hop_size without the override) -> harmonic mask (in
//      place) -> HPCP -> key vote (runs under B-D)
//   B  tempo_pass (pipeline_tempo.hip): STFT 2048/512 (frame_size / hop_size); frame features;
//      novelty (5 variants); FFT + ACF tempograms; candidate scoring + gate
//                                                        -> host reads estimates (sync 2)
//      (with a sections request: section_novelty, pipeline_key.hip, the cell energies behind the
//      pass and the novelty on the vote stream behind them)
//      hpss, onsets: energy RMS + energy-flux onsets; spectral/HFC (/HPSS) onsets; consensus
//   C  seed_tempo, escalate for ambiguous tracks: STFT 2048/256 and 2048/1024 of those tracks, the
//      same feature/novelty/tempogram/scoring kernels, then multi-resolution fusion;
//      perc_fallback, legacy_select (pipeline_tempo.hip)
//   D  beat_grid (with a tempo map request: tempo_map behind it); join_key (pipeline_key.hip): the
//      previous sub-batch's key results, and this one's now or one sub-batch late; download_results,
//      beat_sync_revote, fill_results
//                                                        -> host reads results (sync 3)
// Each stage returns a plain struct with what later stages read (pipeline.hpp).
// pipeline_params.hip maps the configuration to launch parameters, pipeline_debug.hip has the
// debug_track_id dumps and the stage probes, pipeline_abi.hip the C ABI entry points.
// No stage falls back to the CPU; host code only plans offsets and formats the result.
#include "overview_plan.hpp"
#include "pipeline.hpp"

namespace sdsp {

namespace detail {
// Spectrogram row strides (floats; multiples of 4 for 16-B rows).  The key spectrogram's rows
// are 16 KiB + 256 B apart: at 16 KiB + 16 B the mask's column streams (one 256-B row segment
// per wave per frame) run 1.5x slower (profiles/README.md, stride sweep of round 2).
constexpr int STRIDE2 = 1028;  // 1025 bins
constexpr int STRIDE8 = 4160;  // 4097 bins
// row stride of the tempo path's spectrogram for AnalysisConfig::frame_size (nb = fs/2 + 1 bins)
int base_stride(int fs) {
    if (fs == 2048) return STRIDE2;
    if (fs == 8192) return STRIDE8;
    return (fs / 2 + 1 + 3) & ~3;
}
}  // namespace detail

Pipeline::Pipeline(DeviceCtx& d, const sdsp_config& cfg, uint32_t sr, int stages, bool exact_energy, bool key_only,
                   bool nested, bool probe)
    : c_(d),
      d_(d),
      cfg_(cfg),
      sr_(sr),
      bpm_only_(stages == SDSP_STAGES_BPM_ONLY),
      exact_energy_(exact_energy),
      key_only_(key_only),
      nested_(nested || probe),
      fs_((int)std::min<uint64_t>(cfg.frame_size, STFT_GEN_MAX)),
      nb_(fs_ / 2 + 1),
      s2_(base_stride(fs_)),
      kfs_((int)std::min<uint64_t>(key_fft(cfg), STFT_GEN_MAX)),
      khop_((int)std::min<uint64_t>(std::max<uint64_t>(key_hop(cfg), 1), INT32_MAX)),
      ks_(base_stride(kfs_)) {
    if (nested_) c_.pre = probe ? "D." : "X.";
}

void Pipeline::run(const float* d_samples, const std::vector<uint64_t>& in_off, const std::vector<uint64_t>& n_raw,
                   std::vector<TrackRes>& res) {
    const size_t T = n_raw.size();
    res.assign(T, TrackRes{});
    if (ov_out_) ov_out_->assign(T, TrackOv{});
    if (kt_out_) kt_out_->assign(T, TrackKt{});
    if (lv_out_) lv_out_->assign(T, TrackLv{});
    if (tm_out_) tm_out_->assign(T, TrackTm{});
    if (sc_out_) sc_out_->assign(T, TrackSc{});
    if (r128_out_) r128_out_->assign(T, TrackR128{});
    const std::string why = check_supported(cfg_, sr_);
    for (size_t i = 0; i < T; i++) {
        if (n_raw[i] == 0) {
            res[i].status = SDSP_ERR_INVALID_INPUT;
            res[i].err = "Invalid input: Empty audio samples";
        } else if (sr_ == 0) {
            res[i].status = SDSP_ERR_INVALID_INPUT;
            res[i].err = "Invalid input: Invalid sample rate";
        } else if (!why.empty()) {
            res[i].status = SDSP_ERR_NOT_IMPLEMENTED;
            res[i].err = "Not implemented: " + why;
        }
    }
    // Sub-batches under an HBM budget (bytes per track estimated from its raw length): what is
    // free now plus what this context already holds (its buffers are reused), less headroom
    // for the grow-only buffers' 1/8 slack.  SDSP_HBM_BUDGET_GB overrides.
    double budget = 64e9;
    {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
            double held = 0;  // (a nested rerun's "X." buffers are not this pipeline's to reuse)
            for (auto& kv : d_.bufs)
                if (kv.first.compare(0, c_.pre.size(), c_.pre) == 0 && (!c_.pre.empty() || kv.first.compare(0, 2, "X.") != 0))
                    held += (double)kv.second->bytes;
            budget = std::max(4e9, ((double)fr + held) * 0.80 / 1.125);
        }
        // schedule knob (sdsp_debug_set_schedule): the tests' several-sub-batch paths
        if (const double gb = test_hooks().hbm_budget_gb.load(); gb > 0.0) budget = std::max(1.0, gb) * 1e9;
    }
    const uint64_t hop = cfg_.hop_size, khop = (uint64_t)khop_;
    std::vector<int> cur;
    double acc = 0;
    auto flush = [&]() {
        if (!cur.empty()) sub_batch(d_samples, in_off, n_raw, cur, res);
        cur.clear();
        acc = 0;
    };
    times_ = sdsp_stage_times{};
    last_sub_ = false;
    auto t0 = std::chrono::steady_clock::now();
    // with a levels request its folds also give the configured RMS / LUFS gain (one fold, not two)
    if (lv_out_ && why.empty())
        levels_prepass(d_samples, in_off, n_raw, res);
    else if (cfg_.enable_normalization && cfg_.normalization != SDSP_NORM_PEAK && why.empty())
        loudness_prepass(d_samples, in_off, n_raw, res);
    // the programme loudness kernels, on the vote stream beside the first sub-batch (nothing without a request)
    if (r128_out_ && why.empty()) r128_prepass(d_samples, in_off, n_raw, res);
    // the fingerprint request's word buffer of the call, a slot per track (nothing without a request)
    if (fp_out_) fingerprint_plan(n_raw);
    // equal shares: the fewest sub-batches that fit the budget, each near total / count (a
    // short last sub-batch runs at a fraction of the chip)
    std::vector<double> need(T, 0.0);
    double total_need = 0;
    for (size_t i = 0; i < T; i++) {
        if (res[i].status != SDSP_OK) continue;
        const double n = (double)n_raw[i];
        need[i] = n / hop * (s2_ * 4.0 * 1.3 + 4 * 70.0) + (bpm_only_ ? 0.0 : n / khop * ks_ * 4.0) +
                  (n / 256 + n / 1024) * s2_ * 4.0 + 1e6;
        if (cfg_.enable_hpss_onsets || cfg_.enable_tempogram_percussive_fallback)  // H, P ping-pong + a copy
            need[i] += n / hop * s2_ * 4.0 * 5.0;
        if (cfg_.enable_key_hpss_harmonic && !bpm_only_) need[i] += n / khop * 1024.0 * 4.0;
        if (kt_out_ && !bpm_only_) need[i] += (n / khop / kt_H_ + 1.0) * 2.0 * sizeof(KtSeg);  // both parities' segments
        if (cfg_.enable_tempogram_multi_resolution && hop != 512) need[i] += n / 512 * s2_ * 4.0 * 1.3;
        if (lv_out_) {  // the folds' words; the map's frame RMS (not there with trimming off), scratch and dense regions
            const double F = n / (fs_ / 2) + 1.0;
            need[i] += 64.0 + (map_on() ? F * 4.0 + (F / (double)(lv_min_frames(sr_, (uint64_t)fs_) + 1) + 2.0) * 2.0 * 16.0 : 0.0);
        }
        if (tm_out_ && !bpm_only_)  // the segment lists and the gathered onsets (a few per second)
            need[i] += (double)tm_segment_capacity((uint64_t)n, sr_) * sizeof(TmSeg) + n / std::max<uint32_t>(sr_, 1) * 16.0 * 4.0;
        if (sc_out_ && !bpm_only_)  // both parities' cell means, novelty and flags
            need[i] += (n / (double)sc_Cs_ + 1.0) * 2.0 * (12.0 * 4.0 + 4.0 + 4.0 + 1.0);
        if (r128_out_) need[i] += n / (double)std::max<uint32_t>(sr_ / 10, 1) * 12.0 + 64.0;  // z and both curves
        if (fp_out_ && !bpm_only_) need[i] += (n / (double)fp_Cs_ + 1.0) * (4.0 + 12.0 * 4.0);  // its words and cell means
        total_need += need[i];
    }
    const double parts = std::max(1.0, std::ceil(total_need / budget));
    const double share = total_need / parts;
    double cum = 0;
    int part = 0;
    for (size_t i = 0; i < T; i++) {
        if (res[i].status != SDSP_OK) continue;
        // a track belongs to the share its midpoint falls in
        const int p = (int)std::min(parts - 1.0, std::floor((cum + 0.5 * need[i]) / share));
        if (!cur.empty() && (p != part || acc + need[i] > budget)) flush();
        part = p;
        cur.push_back((int)i);
        acc += need[i];
        cum += need[i];
    }
    last_sub_ = true;
    flush();
    last_sub_ = false;
    // the last sub-batch's near tracks: rerun in place when its band-path buffers are intact,
    // otherwise by run_locked
    rerun_tail(finish_key(res, true), res);
    levels_join();  // the one join of the levels folds (nothing without a request)
    r128_join();    // ... and of the programme loudness kernels
    if (fp_out_) fingerprint_finish(res);  // every join is done: the call's words are complete
    times_.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    times_.key_reruns = reruns_;  // in-flight reruns (rerun_near), their time inside total_ms
    times_.rerun_ms = rerun_ms_;
    d_.last = times_;
    if (!exact_energy_ && !nested_) d_.last_tail_reruns = tail_reruns_;
}

void Pipeline::loudness_prepass(const float* d_samples, const std::vector<uint64_t>& in_off,
                                const std::vector<uint64_t>& n_raw, std::vector<TrackRes>& res) {
    const size_t T = n_raw.size();
    loud_gain_.assign(T, 1.0f);
    loud_stat_.assign(T, 0);
    const LoudnessParams lp = loudness_params(cfg_.normalization, sr_);
    std::vector<uint64_t> off, nr, cpfx(1, 0);
    std::vector<size_t> at;
    for (size_t i = 0; i < T; i++) {
        if (res[i].status != SDSP_OK) continue;
        if (lp.method == 2 && lp.block == 0) {  // calculate_lufs :199-204
            res[i].status = SDSP_ERR_INVALID_INPUT;
            res[i].err = "Invalid input: Sample rate too low for LUFS calculation";
            continue;
        }
        at.push_back(i);
        off.push_back(in_off[i]);
        nr.push_back(n_raw[i]);
        cpfx.push_back(cpfx.back() + (n_raw[i] + PK_CH - 1) / PK_CH);
    }
    const int L = (int)at.size();
    if (L == 0) return;
    uint64_t* d_off = c_.up("L.off", off);
    uint64_t* d_nr = c_.up("L.nr", nr);
    uint64_t* d_cpfx = c_.up("L.cpfx", cpfx);
    unsigned int* d_peak = c_.dev<unsigned int>("L.peak", (size_t)L);
    float* d_gain = c_.dev<float>("L.gain", (size_t)L);
    int* d_stat = c_.dev<int>("L.stat", (size_t)L);
    launch_loudness_gain(d_samples, d_off, d_nr, d_cpfx, L, cpfx.back(),
                         c_.dev<unsigned int>("L.peakchunk", std::max<uint64_t>(cpfx.back(), 1)), d_peak, lp, d_gain,
                         d_stat, d_.stream);
    SDSP_HIP_CHECK(hipGetLastError());
    const std::vector<float> g = c_.down(d_gain, (size_t)L);
    const std::vector<int> st = c_.down(d_stat, (size_t)L);
    for (int k = 0; k < L; k++) {
        loud_gain_[at[(size_t)k]] = g[(size_t)k];
        loud_stat_[at[(size_t)k]] = st[(size_t)k];
    }
}

void Pipeline::sub_batch(const float* d_samples, const std::vector<uint64_t>& in_off, const std::vector<uint64_t>& n_raw,
                         const std::vector<int>& idx, std::vector<TrackRes>& res) {
    HostTrace htr;
    Timers tm;
    tm.init(d_);
    tm.mark(0);
    // A: peak/gain, silence, trim; the surviving tracks
    const Front f = front(d_samples, in_off, n_raw, idx, res);
    htr("A");
    tm.mark(1);
    const int NR = (int)f.R.size();
    if (NR == 0) return;
    std::vector<TrackDbg> tdbg(dbg_on() ? (size_t)NR : 0);
    const TempoPassIn bin = base_pass_in(d_samples, f);
    // E: key, on the key stream under B-D
    KeyLaunch kl = launch_key(d_samples, bin, f);
    if (key_only_) {
        join_key_only(kl, f, res);
        htr("E key only");
        return;
    }
    // B: base tempo pass (hop = config hop), HPSS, onsets
    TempoPassOut bo;
    tempo_pass("B.", bin, bo);
    add_pass_times(bo);
    section_novelty(kl, bo);  // (nothing without a request)
    tm.mark(2);
    const Overview ov = overview(d_samples, bin, bo, tm);  // (nothing without a request)
    const std::vector<TempoEst> best = c_.down(bo.est, (size_t)NR);
    const Hpss hp = hpss(bo, best, htr);
    const Onsets on = onsets(d_samples, f, bin, bo, hp);
    htr("B");
    tm.mark(3);
    // C: the final tempo, refined in turn by the escalation, the percussive fallback, the legacy estimator
    Tempo tp = seed_tempo(f, best, on, res);
    if (dbg_on() && mr_on()) debug_base(bin, bo, best, tdbg);
    escalate(f, bin, bo, best, tp, tdbg, res);
    htr("C");
    if (perc_on()) {
        perc_fallback(f, bin, bo, best, hp, tp, res);
        htr("C perc");
    }
    if (cfg_.force_legacy_bpm || cfg_.enable_bpm_fusion) legacy_select(f, bin, on, tp, res);
    tm.mark(4);
    if (bpm_only_) {
        for (int i = 0; i < NR; i++) {
            TrackRes& r = res[f.slot[(size_t)i]];
            if (r.status != SDSP_OK) continue;
            r.bpm = tp.fbpm_h[(size_t)i];
            r.bpm_conf = tp.fconf_h[(size_t)i];
        }
        overview_results(ov, f, bin, bo, tm);
        htr("results (bpm only)");
        return;
    }
    // D: beat grid, key joins, results
    const Beats bt = beat_grid(bin, bo, on, tp);
    tm.mark(5);
    const TempoMapQ tq = tempo_map(bin, on, tp, bt);  // (nothing without a request)
    if (tq.on) tm.mark(9);
    std::vector<KeyOut> kout = join_key(d_samples, in_off, n_raw, f, kl, htr, res);  // empty: joined one sub-batch late
    const ResultsHost rh = download_results(bt, bin, bo, tq);
    if (tq.on) {
        tempo_map_results(rh, f, tp);
        d_.last_tm.map_ms += tm.ms(5, 9);
        d_.last_tm.beat_ms += tm.ms(4, 5);
        d_.last_tm.tracks += (uint64_t)NR;
    }
    overview_results(ov, f, bin, bo, tm);
    htr("D down");
    if (cfg_.enable_key_beat_synchronous && !cfg_.enable_key_log_frequency && !kl.K.empty()) {
        beat_sync_revote(kl, rh, kout);
        htr("E beat-sync");
    }
    times_.beat_ms += tm.ms(4, 5);
    fill_results(f, bin, best, tp, rh, res);
    for (size_t k = 0; k < kout.size(); k++) {
        TrackRes& r = res[f.slot[(size_t)kl.K[k]]];
        if (!kout[k].ok) continue;
        set_key_fields(r, kout[k]);
        r.key_near = kout[k].near;
    }
    if (dbg_on()) {
        debug_key(kl, kout, tdbg);
        for (const TrackDbg& t : tdbg) print_debug(cfg_, t);
    }
    htr("results");
}

// A: peak/gain, silence RMS, trim (sync 1), and the tracks that are non-empty after trimming.
Front Pipeline::front(const float* d_samples, const std::vector<uint64_t>& in_off, const std::vector<uint64_t>& n_raw,
                      const std::vector<int>& idx, std::vector<TrackRes>& res) {
    Front f;
    const int T = (int)idx.size();
    const int FS = fs_;
    const int HOP = (int)cfg_.hop_size;
    hipStream_t st = d_.stream;
    std::vector<uint64_t> nr((size_t)T), cpfx((size_t)T + 1, 0), spfx((size_t)T + 1, 0);
    f.off.resize((size_t)T);
    for (int t = 0; t < T; t++) {
        f.off[(size_t)t] = in_off[(size_t)idx[(size_t)t]];
        nr[(size_t)t] = n_raw[(size_t)idx[(size_t)t]];
        cpfx[(size_t)t + 1] = cpfx[(size_t)t] + (nr[(size_t)t] + PK_CH - 1) / PK_CH;
        const uint64_t fs = nr[(size_t)t] >= (uint64_t)FS ? (nr[(size_t)t] - FS) / (FS / 2) + 1 : 1;
        spfx[(size_t)t + 1] = spfx[(size_t)t] + (cfg_.enable_silence_trimming || map_on() ? fs : 0);
    }
    uint64_t* d_off = c_.up("A.off", f.off);
    uint64_t* d_nr = c_.up("A.nr", nr);
    uint64_t* d_cpfx = c_.up("A.cpfx", cpfx);
    uint64_t* d_spfx = c_.up("A.spfx", spfx);
    unsigned int* d_peak = c_.dev<unsigned int>("A.peak", (size_t)T);
    float* d_gain = c_.dev<float>("A.gain", (size_t)T);
    const float target = sd_powf(10.0f, (0.0f - 1.0f) / 20.0f);  // lib.rs:121 max_headroom_db = 1.0
    const bool loud = cfg_.enable_normalization && cfg_.normalization != SDSP_NORM_PEAK;
    std::vector<int> nstat((size_t)T, 0);
    if (loud) {  // gains from the batch-wide pre-pass (loudness_prepass)
        std::vector<float> g((size_t)T);
        for (int t = 0; t < T; t++) {
            g[(size_t)t] = loud_gain_[(size_t)idx[(size_t)t]];
            nstat[(size_t)t] = loud_stat_[(size_t)idx[(size_t)t]];
        }
        d_gain = c_.up("A.gain", g);
    } else {
        launch_peak_gain(d_samples, d_off, d_nr, d_cpfx, T, cpfx[(size_t)T],
                         c_.dev<unsigned int>("A.peakchunk", std::max<uint64_t>(cpfx[(size_t)T], 1)), d_peak, target,
                         cfg_.enable_normalization, d_gain, st);
    }
    // One read of the samples for both frame-RMS passes: with trimming on and the trim hop (fs / 2)
    // a multiple of the energy hop, the trim pass runs on the raw signal at the energy hop (trim
    // frame f = raw frame f * (fs / 2) / hop), and the energy pass takes its whole frames from it
    // (launch_frame_rms_from_raw)
    const int G_e = HOP > 0 && FS % HOP == 0 ? FS / HOP : 0;
    const bool rms_shared = f.rms_shared = cfg_.enable_silence_trimming && HOP > 0 && HOP % 32 == 0 &&
                                           (FS / 2) % HOP == 0 && (G_e == 1 || G_e == 2 || G_e == 4 || G_e == 8);
    std::vector<uint64_t>& rpfx = f.rpfx;
    rpfx.assign((size_t)T + 1, 0);
    for (int t = 0; t < T; t++)
        rpfx[(size_t)t + 1] = rpfx[(size_t)t] + (rms_shared ? (nr[(size_t)t] >= (uint64_t)FS ? (nr[(size_t)t] - FS) / HOP + 1 : 1) : 0);
    uint64_t* d_rpfx = nullptr;
    if (rms_shared) {
        d_rpfx = c_.up("A.rpfx", rpfx);
        f.d_srms = c_.dev<float>("A.rrms", std::max<uint64_t>(rpfx[(size_t)T], 1));
        launch_frame_rms(d_samples, d_off, d_gain, d_nr, d_rpfx, T, rpfx[(size_t)T], FS, HOP, f.d_srms, st);
    } else {
        f.d_srms = c_.dev<float>("A.srms", spfx[(size_t)T]);
        launch_frame_rms(d_samples, d_off, d_gain, d_nr, d_spfx, T, spfx[(size_t)T], FS, FS / 2, f.d_srms, st);
    }
    const float thr = sd_powf(10.0f, cfg_.min_amplitude_db / 20.0f);
    const uint64_t min_samples = sd_f2u64((float)500u / 1000.0f * (float)sr_);
    const uint64_t min_frames = (min_samples + (FS / 2) - 1) / (FS / 2);
    uint64_t* d_ts = c_.dev<uint64_t>("A.ts", (size_t)T);
    uint64_t* d_te = c_.dev<uint64_t>("A.te", (size_t)T);
    launch_trim(f.d_srms, d_spfx, T, d_nr, FS / 2, thr, min_frames, cfg_.enable_silence_trimming, d_ts, d_te, st,
                rms_shared ? d_rpfx : nullptr, rms_shared ? (FS / 2) / HOP : 1);
    // the silence map (levels request) from the same rows, trimming on or off
    uint64_t *d_mpfx = nullptr, *d_mdense = nullptr;
    if (map_on()) {
        std::vector<uint64_t> mcap((size_t)T + 1, 0);
        for (int t = 0; t < T; t++)
            mcap[(size_t)t + 1] = mcap[(size_t)t] + lv_map_capacity(spfx[(size_t)t + 1] - spfx[(size_t)t], min_frames);
        d_mpfx = c_.dev<uint64_t>("A.mpfx", (size_t)T + 1);
        d_mdense = c_.dev<uint64_t>("A.mdense", 2 * mcap[(size_t)T]);
        launch_silence_map(f.d_srms, d_spfx, rms_shared ? d_rpfx : nullptr, rms_shared ? (FS / 2) / HOP : 1, T, d_nr,
                           FS / 2, thr, min_frames, c_.up("A.mcap", mcap), c_.dev<uint64_t>("A.mreg", 2 * mcap[(size_t)T]),
                           c_.dev<int>("A.mcnt", (size_t)T), d_mpfx, d_mdense, st);
    }
    SDSP_HIP_CHECK(hipGetLastError());
    f.gain_h = c_.down(d_gain, (size_t)T);
    f.ts = c_.down(d_ts, (size_t)T);
    f.te = c_.down(d_te, (size_t)T);
    if (lv_out_) {
        std::vector<uint64_t> mpfx((size_t)T + 1, 0), dense;
        if (map_on()) {
            mpfx = c_.down(d_mpfx, (size_t)T + 1);
            dense = c_.down(d_mdense, 2 * (size_t)mpfx[(size_t)T]);
        }
        for (int t = 0; t < T; t++) {
            TrackLv& l = (*lv_out_)[(size_t)idx[(size_t)t]];
            if (nstat[(size_t)t] != 0) continue;  // the configured normalisation failed: gain 1, no map
            l.applied_gain = f.gain_h[(size_t)t];
            l.ts = f.ts[(size_t)t];
            l.te = f.te[(size_t)t];
            l.regions.assign(dense.begin() + (long)(2 * mpfx[(size_t)t]), dense.begin() + (long)(2 * mpfx[(size_t)t + 1]));
        }
    }
    for (int t = 0; t < T; t++) {
        TrackRes& r = res[(size_t)idx[(size_t)t]];
        const uint64_t n = f.te[(size_t)t] - f.ts[(size_t)t];
        if (nstat[(size_t)t] != 0) {
            r.status = SDSP_ERR_NUMERICAL;
            r.err = "Numerical error: Mean square too small for LUFS calculation";
            continue;
        }
        if (n == 0) {
            r.status = SDSP_ERR_PROCESSING;
            r.err = "Processing error: Audio is entirely silent after trimming";
            continue;
        }
        r.duration = (float)n / (float)sr_;
        f.R.push_back(t);
        f.slot.push_back((size_t)idx[(size_t)t]);
    }
    return f;
}

// The base tempo pass's input: the surviving tracks' trimmed samples at the configured hop.
TempoPassIn Pipeline::base_pass_in(const float* d_samples, const Front& f) const {
    const int base_top_n =
        (int)std::max<uint64_t>(std::max<uint64_t>(cfg_.tempogram_candidates_top_n, cfg_.tempogram_multi_res_top_k), 10);
    TempoPassIn bin;
    bin.hop = (int)cfg_.hop_size;
    bin.samples = d_samples;
    for (int t : f.R) {
        bin.src_off.push_back(f.off[(size_t)t] + f.ts[(size_t)t]);
        bin.gain_h.push_back(f.gain_h[(size_t)t]);
        bin.n_trim.push_back(f.te[(size_t)t] - f.ts[(size_t)t]);
    }
    bin.top_n = mr_on() ? base_top_n : (cfg_.emit_tempogram_candidates ? (int)cfg_.tempogram_candidates_top_n : 1);
    bin.cand_cap = std::max(bin.top_n, 1);
    bin.gate = mr_on();
    bin.mr_nov = mr_on() && bin.hop == 512;  // at another hop the escalation runs its own hop-512 pass
    return bin;
}

// HPSS (hpss.rs:71-172) of the base spectrogram: for the HPSS onsets every track
// (src/lib.rs:222-236), for the percussive tempogram fallback only the tracks in the low
// trap zone (src/lib.rs:587-598); both read the same decomposition.
Hpss Pipeline::hpss(const TempoPassOut& bo, const std::vector<TempoEst>& best, HostTrace& htr) {
    Hpss hp;
    if (!hpss_on() && !perc_on()) return hp;
    hipStream_t st = d_.stream;
    std::vector<int> S;                // HPSS items (positions in R)
    std::vector<uint64_t> hpfx(1, 0);  // frame prefix over S
    for (size_t i = 0; i < best.size(); i++) {
        const TempoEst& e = best[i];
        if (hpss_on() || (e.ok && e.ambiguous && e.trap_low)) {
            S.push_back((int)i);
            hpfx.push_back(hpfx.back() + (bo.fpfx[i + 1] - bo.fpfx[i]));
        }
    }
    const int NS = (int)S.size();
    const uint64_t totS = hpfx.back();
    if (NS == 0 || totS == 0) return hp;
    std::vector<uint64_t> orow, vt(1, 0), rt(1, 0);
    const uint64_t ncb = (nb_ + HPSS_COLS - 1) / HPSS_COLS;
    for (int k = 0; k < NS; k++) {
        const uint64_t F = hpfx[(size_t)k + 1] - hpfx[(size_t)k];
        orow.push_back(bo.fpfx[(size_t)S[(size_t)k]]);
        vt.push_back(vt.back() + (F + HPSS_VM_FRAMES - 1) / HPSS_VM_FRAMES * ncb);
        rt.push_back(rt.back() + (F + HPSS_ROW_FRAMES - 1) / HPSS_ROW_FRAMES);
    }
    HpssLaunch L{};
    L.P.B = nb_;
    L.P.stride = s2_;
    L.P.m = (int)cfg_.hpss_margin;
    L.orig = bo.mags;
    L.orig_row0 = c_.up("H.orow", orow);
    for (int q = 0; q < 2; q++) {
        L.h[q] = c_.dev<float>("H.h" + std::to_string(q), totS * s2_);
        L.p[q] = c_.dev<float>("H.p" + std::to_string(q), totS * s2_);
    }
    uint64_t* d_hpfx = c_.up("H.hpfx", hpfx);
    L.row0 = d_hpfx;
    L.fpfx = d_hpfx;
    L.vtile_pfx = c_.up("H.vt", vt);
    L.n_vtiles = vt.back();
    L.last_it = c_.up("H.last", std::vector<int>((size_t)NS, 9));
    L.change = c_.dev<unsigned int>("H.chg", (size_t)NS);
    L.n_items = NS;
    launch_hpss(L, st);
    SDSP_HIP_CHECK(hipGetLastError());
    hp.d_P0 = L.p[0];
    hp.d_hpe = c_.dev<float>("H.e", totS);
    hp.d_hfmax = c_.dev<float>("H.fmax", totS);
    launch_hpss_rows(hp.d_P0, d_hpfx, d_hpfx, c_.up("H.rt", rt), rt.back(), NS, s2_, nb_, hp.d_hpe, hp.d_hfmax, st);
    SDSP_HIP_CHECK(hipGetLastError());
    htr("HPSS");
    return hp;
}

// onsets: energy flux (frame FS, hop HOP; same framing as the STFT), spectral flux, HFC, HPSS, consensus
Onsets Pipeline::onsets(const float* d_samples, const Front& f, const TempoPassIn& bin, const TempoPassOut& bo,
                        const Hpss& hp) {
    const int NR = (int)f.R.size(), FS = fs_, HOP = bin.hop;
    hipStream_t st = d_.stream;
    uint64_t* d_src = c_.up("B.src2", bin.src_off);
    float* d_g = c_.up("B.gain2", bin.gain_h);
    uint64_t* d_nt = c_.up("B.ntrim", bin.n_trim);
    float* d_erms = c_.dev<float>("B.erms", std::max<uint64_t>(bo.total, 1));
    bool from_raw = f.rms_shared;
    std::vector<uint64_t> rbase;
    for (int t : f.R) {
        from_raw = from_raw && f.ts[(size_t)t] % (uint64_t)HOP == 0;
        rbase.push_back(f.rpfx[(size_t)t] + f.ts[(size_t)t] / (uint64_t)HOP);
    }
    if (from_raw)
        launch_frame_rms_from_raw(f.d_srms, c_.up("B.rbase", rbase), d_samples, d_src, d_g, d_nt, bo.d_fpfx, NR, bo.total,
                                  FS, HOP, d_erms, st);
    else
        launch_frame_rms(d_samples, d_src, d_g, d_nt, bo.d_fpfx, NR, bo.total, FS, HOP, d_erms, st);
    return onset_lists(d_erms, d_nt, HOP, bo, hp);
}

// The onset lists and their consensus from the device curves of a pass's tracks: the frame RMS
// d_erms, bo.SFO, bo.H (its full-band quarter) and, with HPSS onsets, hp.d_hpe, at bo's frame
// prefix.  The analysis call (Pipeline::onsets) and the stage probe (debug_onset_stages) both
// launch from here.
Onsets Pipeline::onset_lists(const float* d_erms, const uint64_t* d_nt, int HOP, const TempoPassOut& bo,
                             const Hpss& hp) {
    Onsets on;
    const int NR = (int)bo.fpfx.size() - 1;
    hipStream_t st = d_.stream;
    const bool hpss_on = cfg_.enable_hpss_onsets && cfg_.enable_onset_consensus;
    uint32_t* d_eon = c_.dev<uint32_t>("B.eon", std::max<uint64_t>(bo.total, 1));
    int* d_en = c_.dev<int>("B.en", (size_t)NR);
    launch_energy_onsets(d_erms, bo.d_fpfx, d_nt, HOP, sd_powf(10.0f, -20.0f / 20.0f), d_eon, bo.d_fpfx, d_en, NR, st);
    const int kinds = hpss_on ? 3 : 2;  // spectral flux, HFC (+ HPSS)
    uint32_t* d_fon = c_.dev<uint32_t>("B.fon", kinds * std::max<uint64_t>(bo.total, 1));
    int* d_fn = c_.dev<int>("B.fn", kinds * (size_t)NR);
    float* d_fscr = c_.dev<float>("B.fscr", kinds * std::max<uint64_t>(bo.total, 1));
    const float pct = cfg_.onset_threshold_percentile;
    if (pct >= 0.0f && pct <= 1.0f)
        launch_flux_onsets(bo.SFO, bo.H, hpss_on ? hp.d_hpe : nullptr, d_fscr, bo.d_fpfx, d_nt, HOP, pct, d_fon, bo.d_fpfx,
                           d_fn, NR, st);
    else  // detect_*_onsets return Err -> warn + empty lists (src/lib.rs:196-236)
        SDSP_HIP_CHECK(hipMemsetAsync(d_fn, 0, kinds * (size_t)NR * sizeof(int), st));
    if (hpss_on && !hp.d_hpe)  // no frames at all: empty HPSS lists
        SDSP_HIP_CHECK(hipMemsetAsync(d_fn + 2 * NR, 0, (size_t)NR * sizeof(int), st));
    const uint64_t lists = hpss_on ? 4 : 3;
    std::vector<int> has_mags((size_t)NR);
    std::vector<uint64_t> coff((size_t)NR);
    for (int i = 0; i < NR; i++) {
        has_mags[(size_t)i] = bo.fpfx[(size_t)i + 1] > bo.fpfx[(size_t)i];
        coff[(size_t)i] = lists * bo.fpfx[(size_t)i];
    }
    int* d_hm = c_.up("B.hasm", has_mags);
    on.d_coff = c_.up("B.coff", coff);
    on.d_chosen = c_.dev<uint32_t>("B.chosen", lists * std::max<uint64_t>(bo.total, 1));
    on.d_cn = c_.dev<int>("B.cn", (size_t)NR);
    bool cons_ok = cfg_.enable_onset_consensus && cfg_.onset_consensus_tolerance_ms > 0;
    for (int k = 0; k < 4; k++) cons_ok = cons_ok && !(cfg_.onset_consensus_weights[k] < 0.0f);
    const uint32_t tol = (uint32_t)sd_f2u64((float)cfg_.onset_consensus_tolerance_ms / 1000.0f * (float)sr_);
    uint32_t* d_cscr = c_.dev<uint32_t>("B.cscr", 5 * lists * std::max<uint64_t>(bo.total, 1));
    launch_consensus(d_eon, bo.d_fpfx, d_en, d_fon, bo.d_fpfx, d_fn, bo.total, NR, tol, cons_ok, d_hm, on.d_chosen,
                     on.d_coff, on.d_cn, d_cscr, st, hpss_on ? 1 : 0);
    SDSP_HIP_CHECK(hipGetLastError());
    on.d_eon = d_eon;
    on.d_en = d_en;
    on.d_fon = d_fon;
    on.d_fn = d_fn;
    on.lists = (int)lists;
    on.en_h = c_.down(d_en, (size_t)NR);
    return on;
}

// D: beat grid from the consensus onsets and the final tempo
Beats Pipeline::beat_grid(const TempoPassIn& bin, const TempoPassOut& bo, const Onsets& on, const Tempo& tp) {
    Beats bt;
    const int NR = (int)bin.n_trim.size();
    std::vector<int> ident((size_t)NR);
    std::vector<uint64_t>& boff = bt.boff;
    boff.assign((size_t)NR + 1, 0);
    std::vector<int> bcap((size_t)NR);
    for (int i = 0; i < NR; i++) {
        ident[(size_t)i] = i;
        const uint64_t n = bin.n_trim[(size_t)i];
        const uint64_t dur_s = n / std::max<uint32_t>(sr_, 1) + 1;
        const uint64_t F = bo.fpfx[(size_t)i + 1] - bo.fpfx[(size_t)i];
        const uint64_t cap = std::max<uint64_t>(12 * dur_s + 64, 3 * F + 8);
        bcap[(size_t)i] = (int)cap;
        boff[(size_t)i + 1] = boff[(size_t)i] + cap;
    }
    int* d_ident = c_.up("D.ident", ident);
    bt.d_boff = c_.up("D.boff", boff);
    int* d_bcap = c_.up("D.bcap", bcap);
    float* d_bscr = c_.dev<float>("D.bscr", 4 * boff[(size_t)NR]);
    bt.d_beats = c_.dev<float>("D.beats", boff[(size_t)NR]);
    bt.d_downs = c_.dev<float>("D.downs", boff[(size_t)NR]);
    bt.d_bout = c_.dev<BeatOut>("D.bout", (size_t)NR);
    bt.d_bscr = d_bscr;
    bt.d_bcap = d_bcap;
    launch_beat(d_ident, NR, on.d_chosen, on.d_coff, on.d_cn, sr_, tp.d_fbpm, tp.d_fconf, d_bscr, bt.d_boff, d_bcap,
                bt.d_beats, bt.d_downs, bt.d_bout, d_.stream);
    SDSP_HIP_CHECK(hipGetLastError());
    return bt;
}

// The tempo maps (include/stratum_hip.h, sdsp_tempo_map) of the surviving tracks, queued on the
// main stream right behind k_beat: one wave per track over the same onsets, tempo and published
// beats (k_tempo_map.hip).  Segment capacity per track: tm_segment_capacity.
TempoMapQ Pipeline::tempo_map(const TempoPassIn& bin, const Onsets& on, const Tempo& tp, const Beats& bt) {
    TempoMapQ tq;
    if (!tm_out_) return tq;
    tq.on = true;
    const int NR = (int)bin.n_trim.size();
    tq.soff.assign((size_t)NR + 1, 0);
    for (int i = 0; i < NR; i++)
        tq.soff[(size_t)i + 1] = tq.soff[(size_t)i] + tm_segment_capacity(bin.n_trim[(size_t)i], sr_);
    uint64_t* d_soff = c_.up("D.tmsoff", tq.soff);
    tq.d_segs = c_.dev<TmSeg>("D.tmsegs", tq.soff[(size_t)NR]);
    tq.d_out = c_.dev<TmOut>("D.tmout", (size_t)NR);
    tq.d_chosen = on.d_chosen;
    tq.d_coff = on.d_coff;
    tq.d_cn = on.d_cn;
    launch_tempo_map(NR, on.d_chosen, on.d_coff, on.d_cn, sr_, tp.d_fbpm, bt.d_bscr, bt.d_boff, bt.d_bcap, bt.d_beats,
                     bt.d_bout, d_soff, tq.d_segs, tq.d_out, d_.stream);
    SDSP_HIP_CHECK(hipGetLastError());
    return tq;
}

// The sub-batch's tempo maps into the call's per-track entries.
void Pipeline::tempo_map_results(const ResultsHost& rh, const Front& f, const Tempo& tp) {
    const size_t NR = f.R.size();
    for (size_t i = 0; i < NR; i++)
        (*tm_out_)[f.slot[i]] = track_tempo_map(rh, i, tp.fbpm_h[i], tp.fconf_h[i], f.ts[(size_t)f.R[i]]);
}

// Track i of a sub-batch's downloaded tempo maps.
TrackTm Pipeline::track_tempo_map(const ResultsHost& rh, size_t i, float bpm, float conf, uint64_t first) const {
    TrackTm m;
    m.on = true;
    m.o = rh.tm_out[i];
    m.bpm = bpm;
    m.conf = conf;
    m.first = first;
    if (m.o.ok > 0 && (tm_what_ & SDSP_TEMPO_MAP_SEGMENTS))
        m.segs.assign(rh.tm_segs.begin() + (long)rh.tm_soff[i], rh.tm_segs.begin() + (long)(rh.tm_soff[i] + (uint64_t)m.o.n_seg));
    if (!rh.tm_opfx.empty())
        m.onsets.assign(rh.tm_onsets.begin() + (long)rh.tm_opfx[i], rh.tm_onsets.begin() + (long)rh.tm_opfx[i + 1]);
    return m;
}

// The beat lists compacted on the device and read back (sync 3), with the base pass's candidates
// and, with a tempo map request, the maps, their segments and the onset lists.
ResultsHost Pipeline::download_results(const Beats& bt, const TempoPassIn& bin, const TempoPassOut& bo,
                                       const TempoMapQ& tq) {
    ResultsHost rh;
    const size_t NR = bin.n_trim.size();
    uint64_t* d_bpfx = c_.dev<uint64_t>("D.bpfx", 2 * (NR + 1));
    rh.d_cbeats = c_.dev<float>("D.cbeats", bt.boff[NR]);
    float* d_cdowns = c_.dev<float>("D.cdowns", bt.boff[NR]);
    launch_beat_compact((int)NR, bt.d_bout, bt.d_boff, bt.d_beats, bt.d_downs, d_bpfx, rh.d_cbeats, d_cdowns, d_.stream);
    SDSP_HIP_CHECK(hipGetLastError());
    rh.bout = c_.down(bt.d_bout, NR);
    rh.bpfx = c_.down(d_bpfx, 2 * (NR + 1));
    rh.beats_h = c_.down(rh.d_cbeats, rh.bpfx[NR]);
    rh.downs_h = c_.down(d_cdowns, rh.bpfx[2 * NR + 1]);
    if (cfg_.emit_tempogram_candidates) rh.cand_h = c_.down(bo.cand, NR * (size_t)bin.cand_cap * 4);
    if (tq.on) {
        rh.tm_out = c_.down(tq.d_out, NR);
        rh.tm_soff = tq.soff;
        if (tm_what_ & SDSP_TEMPO_MAP_SEGMENTS) rh.tm_segs = c_.down(tq.d_segs, tq.soff[NR]);
        if (tm_what_ & SDSP_TEMPO_MAP_ONSETS) {  // the lists gathered densely, by the counts just read
            const std::vector<int> cn = c_.down(tq.d_cn, NR);
            rh.tm_opfx.assign(NR + 1, 0);
            for (size_t i = 0; i < NR; i++) rh.tm_opfx[i + 1] = rh.tm_opfx[i] + (uint64_t)std::max(cn[i], 0);
            uint32_t* d_dense = c_.dev<uint32_t>("D.tmons", std::max<uint64_t>(rh.tm_opfx[NR], 1));
            launch_onset_gather((int)NR, tq.d_chosen, tq.d_coff, tq.d_cn, c_.up("D.tmopfx", rh.tm_opfx), d_dense, d_.stream);
            SDSP_HIP_CHECK(hipGetLastError());
            rh.tm_onsets = c_.down(d_dense, rh.tm_opfx[NR]);
        }
    }
    return rh;
}

// The overview envelopes (include/stratum_hip.h, sdsp_overview) of the surviving tracks, queued on
// the main stream behind the base pass: the sample extrema per hop segment from the samples, then
// per column those and the band maxima from the pass's rows (k_overview.hip).  The column plan is
// overview_plan.hpp's; the kernels compute a column's frames from the same functions.
Overview Pipeline::overview(const float* d_samples, const TempoPassIn& bin, const TempoPassOut& bo, Timers& tm) {
    Overview ov;
    if (!ov_out_) return ov;
    ov.on = true;
    const int NR = (int)bin.n_trim.size();
    OvParams P{};
    P.B = nb_;
    P.stride = s2_;
    P.columns = ov_req_.columns;
    P.frames_per_column = ov_req_.frames_per_column;
    ov_band_bins(ov_req_.low_max_hz, ov_req_.mid_max_hz, (uint64_t)fs_, sr_, &P.b1, &P.b2);
    std::vector<uint64_t> upfx((size_t)NR + 1, 0);
    ov.cpfx.assign((size_t)NR + 1, 0);
    bool pieces = false;
    for (int i = 0; i < NR; i++) {
        const uint64_t F = bo.fpfx[(size_t)i + 1] - bo.fpfx[(size_t)i];
        const uint64_t C = ov_columns(F, P.columns, P.frames_per_column);
        const uint64_t np = ov_pieces(F, C, P.columns, P.frames_per_column, OV_PIECE);
        pieces = pieces || np > 1;
        ov.cpfx[(size_t)i + 1] = ov.cpfx[(size_t)i] + C;
        upfx[(size_t)i + 1] = upfx[(size_t)i] + C * np;
        ov.seg_bytes += 4.0 * (double)bin.n_trim[(size_t)i];
        ov.col_bytes += 4.0 * (double)F * (double)nb_;
    }
    const uint64_t n_cols = ov.n_cols = ov.cpfx[(size_t)NR], n_units = upfx[(size_t)NR];
    if (n_units / 4 >= 0x7FFFFFFFull) throw HipError("overview: too many columns for one launch");
    if (n_cols == 0) return ov;  // no track has a frame
    uint64_t* d_src = c_.up("O.src", bin.src_off);
    float* d_gain = c_.up("O.gain", bin.gain_h);
    uint64_t* d_n = c_.up("O.n", bin.n_trim);
    uint64_t* d_cpfx = c_.up("O.cpfx", ov.cpfx);
    uint64_t* d_upfx = c_.up("O.upfx", upfx);
    uint32_t* d_lo = c_.dev<uint32_t>("O.seglo", bo.total);
    uint32_t* d_hi = c_.dev<uint32_t>("O.seghi", bo.total);
    ov.d_out = c_.dev<float>("O.out", 5 * n_cols);
    uint32_t* d_part = c_.dev<uint32_t>("O.part", pieces ? 5 * n_units : 1);
    tm.mark(6);
    launch_overview_segments(d_samples, d_src, d_gain, d_n, bo.d_fpfx, NR, bo.total, bin.hop, d_lo, d_hi, d_.stream);
    tm.mark(7);
    launch_overview_columns(bo.mags, bo.d_fpfx, d_cpfx, d_upfx, NR, n_units, n_cols, pieces, d_lo, d_hi, P, ov.d_out,
                            d_part, d_.stream);
    tm.mark(8);
    SDSP_HIP_CHECK(hipGetLastError());
    return ov;
}

// The sub-batch's overviews read back with its results, into the call's per-track entries.
void Pipeline::overview_results(const Overview& ov, const Front& f, const TempoPassIn& bin, const TempoPassOut& bo,
                                Timers& tm) {
    if (!ov.on) return;
    const size_t NR = f.R.size();
    // one download (not value-initialised: at one frame per column it is as long as the samples / 100)
    std::shared_ptr<float[]> h;
    if (ov.n_cols) {
        h.reset(new float[5 * (size_t)ov.n_cols]);
        SDSP_HIP_CHECK(hipMemcpyAsync(h.get(), ov.d_out, 5 * (size_t)ov.n_cols * sizeof(float), hipMemcpyDeviceToHost,
                                      d_.stream));
    }
    c_.sync();
    for (size_t i = 0; i < NR; i++) {
        TrackOv& o = (*ov_out_)[f.slot[i]];
        o.F = bo.fpfx[i + 1] - bo.fpfx[i];
        o.C = ov.cpfx[i + 1] - ov.cpfx[i];
        o.first = f.ts[(size_t)f.R[i]];
        o.n = bin.n_trim[i];
        o.blk = h;
        o.at = 5 * (size_t)ov.cpfx[i];
    }
    sdsp_debug_overview_times& t = d_.last_ov;
    if (ov.n_cols) {
        t.sample_ms += tm.ms(6, 7);
        t.band_ms += tm.ms(7, 8);
    }
    t.sample_bytes += ov.seg_bytes;
    t.band_bytes += ov.col_bytes;
    t.columns += ov.n_cols;
    t.sub_batches++;
}

// Tempo, beat lists and candidate lists into the surviving tracks' results.
void Pipeline::fill_results(const Front& f, const TempoPassIn& bin, const std::vector<TempoEst>& best, const Tempo& tp,
                            const ResultsHost& rh, std::vector<TrackRes>& res) {
    const size_t NR = f.R.size();
    auto add_cands = [](TrackRes& r, const float* c, int n) {
        r.has_cands = true;
        for (int k = 0; k < n; k++, c += 4)
            r.cands.push_back(sdsp_tempo_candidate{c[0], c[1], c[2], c[3], (uint8_t)(sd_absf(c[0] - r.bpm) < 0.75f)});
    };
    for (size_t i = 0; i < NR; i++) {
        TrackRes& r = res[f.slot[i]];
        if (r.status != SDSP_OK) continue;  // a legacy-estimator error propagated
        r.bpm = tp.fbpm_h[i];
        r.bpm_conf = tp.fconf_h[i];
        const BeatOut& b = rh.bout[i];
        if (b.ok < 0) {
            r.status = SDSP_ERR_PROCESSING;
            r.err = "Processing error: beat buffer capacity exceeded";
            continue;
        }
        if (b.ok > 0) {
            const uint64_t ob = rh.bpfx[i], od = rh.bpfx[NR + 1 + i];
            r.beats.assign(rh.beats_h.begin() + (long)ob, rh.beats_h.begin() + (long)(ob + b.n_beats));
            r.downs.assign(rh.downs_h.begin() + (long)od, rh.downs_h.begin() + (long)(od + b.n_down));
            r.stability = b.stability;
        }
        if (!cfg_.emit_tempogram_candidates) continue;
        if (tp.perc_took[i]) {  // chosen_cands = p_cands (:661-664)
            add_cands(r, tp.perc_cands[i].data(), (int)(tp.perc_cands[i].size() / 4));
        } else if (r.mr_used == 1 && !tp.n512_own.empty() && tp.epos[i] >= 0) {
            const size_t k = (size_t)tp.epos[i];  // the escalation's own hop-512 list (hop_size != 512)
            add_cands(r, tp.c512_h.data() + k * (size_t)tp.c512_cap * 4, tp.n512_own[k]);
        } else if (best[i].ok && tg_on()) {
            int n = best[i].n_cands;
            if (mr_on() && r.mr_used == 1) n = std::min(n, (int)std::max<uint64_t>(cfg_.tempogram_multi_res_top_k, 1));
            add_cands(r, rh.cand_h.data() + i * (size_t)bin.cand_cap * 4, n);
        }
    }
}

}  // namespace sdsp
