// pipeline_levels.hip — the levels request's folds (include/stratum_hip.h, sdsp_levels): queued
// once per call before the sub-batches, where loudness_prepass runs, and joined once at the call's
// end.  The folds are a per-track sequential latency, not a throughput, so they go to the key
// vote's low-priority stream, which is idle until the first sub-batch's chroma is ready, and run
// beside the first sub-batch.  The silence map is computed per sub-batch (Pipeline::front), from the
// frame RMS the trim reads.
#include "pipeline.hpp"

namespace sdsp {

namespace {
LvParams lv_params(uint32_t sr) {
    const LoudnessParams lp = loudness_params(SDSP_NORM_LOUDNESS, sr);  // (the targets are every method's)
    LvParams P{};
    P.target_peak = lp.target_peak;
    P.target_rms = lp.target_rms;
    P.target_lufs = lp.target_lufs;
    P.gate = lp.gate;
    P.block = lp.block;
    P.b0 = lp.b0, P.b1 = lp.b1, P.b2 = lp.b2, P.a1 = lp.a1, P.a2 = lp.a2;
    return P;
}
}  // namespace

// Chains of k_levels_fold for the requested methods, and for the configured RMS / LUFS
// normalisation, whose gain comes from the same folds (k_loudness_gain is not run as well).
void Pipeline::levels_prepass(const float* d_samples, const std::vector<uint64_t>& in_off,
                              const std::vector<uint64_t>& n_raw, std::vector<TrackRes>& res) {
    const size_t T = n_raw.size();
    LevelsPending& lp = lv_pending_;
    lp = LevelsPending{};
    const bool loud = cfg_.enable_normalization && cfg_.normalization != SDSP_NORM_PEAK;
    const LvParams P = lp.P = lv_params(sr_);
    uint32_t chains = 0;
    if (lv_what_ & SDSP_LEVELS_RMS) chains |= 1u;
    if (lv_what_ & SDSP_LEVELS_PEAK) chains |= 4u;
    if (lv_what_ & SDSP_LEVELS_LOUDNESS) chains |= 2u | 4u | 8u;  // 4: the all-gated fallback is the Peak metadata
    if (loud) chains |= cfg_.normalization == SDSP_NORM_RMS ? 1u : 2u;
    if (P.block == 0) chains &= ~(2u | 8u);  // calculate_lufs :199-204 (lv_finish_loudness reports it)
    if (loud) {
        loud_gain_.assign(T, 1.0f);
        loud_stat_.assign(T, 0);
    }
    std::vector<uint64_t> off, nr, cpfx(1, 0);
    for (size_t i = 0; i < T; i++) {
        if (res[i].status != SDSP_OK) continue;
        TrackLv& l = (*lv_out_)[i];
        l.on = true;
        l.n = n_raw[i];
        l.te = n_raw[i];
        if (loud && cfg_.normalization == SDSP_NORM_LOUDNESS && P.block == 0) {
            res[i].status = SDSP_ERR_INVALID_INPUT;
            res[i].err = "Invalid input: Sample rate too low for LUFS calculation";
        }
        lp.at.push_back(i);
        off.push_back(in_off[i]);
        nr.push_back(n_raw[i]);
        cpfx.push_back(cpfx.back() + (n_raw[i] + PK_CH - 1) / PK_CH);
    }
    const int L = (int)lp.at.size();
    if (L == 0 || chains == 0) return;  // (a silence map alone needs no fold)
    lp.on = true;
    lp.chains = chains;
    uint64_t* d_off = c_.up("V.off", off);
    uint64_t* d_nr = c_.up("V.nr", nr);
    uint64_t* d_cpfx = c_.up("V.cpfx", cpfx);
    lp.d_peak = c_.dev<unsigned int>("V.peak", (size_t)L);
    float* d_g = c_.dev<float>("V.gain", (size_t)LV_CHAINS * L);
    lp.d_sums = c_.dev<float>("V.sums", (size_t)LV_CHAINS * L);
    lp.d_gn = c_.dev<int>("V.gn", (size_t)L);
    unsigned int* d_pchunk = c_.dev<unsigned int>("V.peakchunk", std::max<uint64_t>(cpfx.back(), 1));
    // the fold stream starts behind the main stream: the uploads above, and whatever the caller's
    // samples wait for
    hipStream_t s = d_.stream3;
    hipEvent_t ev;
    SDSP_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    SDSP_HIP_CHECK(hipEventRecord(ev, d_.stream));
    SDSP_HIP_CHECK(hipStreamWaitEvent(s, ev, 0));
    SDSP_HIP_CHECK(hipEventDestroy(ev));
    lp.tm.reset(new Timers());
    lp.tm->init(d_);
    lp.tm->mark(0, s);
    // the peak, and chain 2's gain (k_gain's min(target / peak, 1 / peak), 1 for a quiet track)
    launch_peak_gain(d_samples, d_off, d_nr, d_cpfx, L, cpfx.back(), d_pchunk, lp.d_peak, P.target_peak, 1, d_g + 2 * (size_t)L,
                     s);
    LvFoldArgs A{};
    A.x = d_samples;
    A.in_off = d_off;
    A.n_raw = d_nr;
    A.T = L;
    A.gains = d_g;
    A.sums = lp.d_sums;
    A.gated_n = lp.d_gn;
    A.chains = chains & 7u;
    launch_levels_fold(A, P, s);
    lp.tm->mark(1, s);
    SDSP_HIP_CHECK(hipGetLastError());
    if (chains & 8u) {  // Loudness' rms_db: the fold under the gain its own first launch gives
        launch_levels_gain(lp.d_peak, lp.d_sums, lp.d_gn, L, P, d_g, s);
        A.chains = 8u;
        launch_levels_fold(A, P, s);
        SDSP_HIP_CHECK(hipGetLastError());
    }
    lp.tm->mark(2, s);
    if (!loud) return;
    // the configured gain is needed before the first sub-batch: wait for the first launch only
    std::vector<unsigned int> pk((size_t)L);
    std::vector<float> sums((size_t)LV_CHAINS * L);
    std::vector<int> gn((size_t)L);
    SDSP_HIP_CHECK(hipEventSynchronize(lp.tm->ev[1]));
    SDSP_HIP_CHECK(hipMemcpy(pk.data(), lp.d_peak, pk.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
    SDSP_HIP_CHECK(hipMemcpy(sums.data(), lp.d_sums, sums.size() * sizeof(float), hipMemcpyDeviceToHost));
    SDSP_HIP_CHECK(hipMemcpy(gn.data(), lp.d_gn, gn.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int k = 0; k < L; k++) {
        const size_t i = lp.at[(size_t)k];
        if (res[i].status != SDSP_OK) continue;
        LvFolds f{};
        f.peak = sd_from_bits_f(pk[(size_t)k]);
        f.ss_raw = sums[(size_t)k];
        f.gsum = sums[(size_t)L + k];
        f.gn = gn[(size_t)k];
        if (cfg_.normalization == SDSP_NORM_RMS) {
            loud_gain_[i] = lv_finish_rms(f, n_raw[i], P).gain;
        } else {
            int st;
            loud_gain_[i] = lv_lufs_gain(f, P, &st);
            loud_stat_[i] = st < 0;
        }
    }
}

// The join: the folds read back and finished on the host (levels_core.hpp), into the call's levels.
void Pipeline::levels_join() {
    LevelsPending& lp = lv_pending_;
    if (!lv_out_ || !lp.on) return;
    const size_t L = lp.at.size();
    hipStream_t s = d_.stream3;
    std::vector<unsigned int> pk(L);
    std::vector<float> sums((size_t)LV_CHAINS * L);
    std::vector<int> gn(L);
    SDSP_HIP_CHECK(hipMemcpyAsync(pk.data(), lp.d_peak, L * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    SDSP_HIP_CHECK(hipMemcpyAsync(sums.data(), lp.d_sums, sums.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    SDSP_HIP_CHECK(hipMemcpyAsync(gn.data(), lp.d_gn, L * sizeof(int), hipMemcpyDeviceToHost, s));
    SDSP_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t k = 0; k < L; k++) {
        TrackLv& l = (*lv_out_)[lp.at[k]];
        LvFolds f{};
        f.peak = sd_from_bits_f(pk[k]);
        f.ss_raw = sums[k];
        f.gsum = sums[L + k];
        f.gn = gn[k];
        f.ss_peak = sums[2 * L + k];
        f.ss_lufs = sums[3 * L + k];
        if (lv_what_ & SDSP_LEVELS_PEAK) l.method[SDSP_NORM_PEAK] = lv_finish_peak(f, l.n, lp.P);
        if (lv_what_ & SDSP_LEVELS_RMS) l.method[SDSP_NORM_RMS] = lv_finish_rms(f, l.n, lp.P);
        if (lv_what_ & SDSP_LEVELS_LOUDNESS) l.method[SDSP_NORM_LOUDNESS] = lv_finish_loudness(f, l.n, lp.P);
    }
    sdsp_debug_levels_times& t = d_.last_lv;
    t.fold_ms = lp.tm->ms(0, 1);
    t.fold2_ms = lp.tm->ms(1, 2);
    t.tracks = L;
    lp = LevelsPending{};
}

}  // namespace sdsp
