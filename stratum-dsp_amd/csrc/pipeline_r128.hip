// pipeline_r128.hip — the programme loudness request (include/stratum_hip.h, sdsp_r128): its three
// kernels queued once per call before the sub-batches and joined once at the call's end, as the
// levels folds are.  They read the caller's raw samples only, so they go to the key vote's
// low-priority stream, which is idle until the first sub-batch's chroma is ready, and run beside the
// first sub-batch.  The nested exact reruns never see the request.
#include "pipeline.hpp"

namespace sdsp {

void Pipeline::r128_prepass(const float* d_samples, const std::vector<uint64_t>& in_off,
                            const std::vector<uint64_t>& n_raw, const std::vector<TrackRes>& res) {
    R128Pending& rp = r128_pending_;
    rp = R128Pending{};
    const R128Params P = rp.P = r128_params(sr_);
    const bool loud = r128_what_ & SDSP_R128_LOUDNESS, curves = r128_what_ & SDSP_R128_CURVES;
    std::vector<uint64_t> off, bpfx(1, 0), zpfx(1, 0), cpfx(1, 0);
    rp.cvpfx.assign(1, 0);
    for (size_t i = 0; i < n_raw.size(); i++) {
        if (res[i].status != SDSP_OK) continue;  // (before run(): n == 0, or an unsupported configuration)
        (*r128_out_)[i].on = true;
        rp.at.push_back(i);
        rp.n.push_back(n_raw[i]);
        off.push_back(in_off[i]);
        const uint64_t J = n_raw[i] / P.step;
        bpfx.push_back(bpfx.back() + r128_step_blocks(J));
        zpfx.push_back(zpfx.back() + J);
        cpfx.push_back(cpfx.back() + r128_peak_blocks(n_raw[i]));
        rp.cvpfx.push_back(rp.cvpfx.back() + r128_n_mom(J) + r128_n_short(J));
    }
    const int L = (int)rp.at.size();
    if (L == 0) return;
    if (bpfx.back() >= (1ull << 31) || cpfx.back() >= (1ull << 31)) throw HipError("r128: batch too large for one launch");
    rp.on = true;
    rp.steps = zpfx.back();
    uint64_t* d_off = c_.up("R.off", off);
    uint64_t* d_n = c_.up("R.n", rp.n);
    uint64_t* d_bpfx = c_.up("R.bpfx", bpfx);
    uint64_t* d_zpfx = c_.up("R.zpfx", zpfx);
    uint64_t* d_cpfx = c_.up("R.cpfx", cpfx);
    uint64_t* d_cvpfx = c_.up("R.cvpfx", rp.cvpfx);
    float* d_z = c_.dev<float>("R.z", (size_t)zpfx.back());
    rp.d_peak = c_.dev<unsigned int>("R.peak", 2 * (size_t)L);
    rp.d_folds = c_.dev<R128Folds>("R.folds", (size_t)L);
    rp.d_curves = curves ? c_.dev<float>("R.curves", (size_t)rp.cvpfx.back()) : nullptr;
    // the stream starts behind the main stream: the uploads above, and whatever the caller's samples
    // wait for
    hipStream_t s = d_.stream3;
    hipEvent_t ev;
    SDSP_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    SDSP_HIP_CHECK(hipEventRecord(ev, d_.stream));
    SDSP_HIP_CHECK(hipStreamWaitEvent(s, ev, 0));
    SDSP_HIP_CHECK(hipEventDestroy(ev));
    rp.tm.reset(new Timers());
    rp.tm->init(d_);
    rp.tm->mark(0, s);
    if (loud) {
        R128StepArgs A{};
        A.x = d_samples;
        A.in_off = d_off;
        A.n_raw = d_n;
        A.bpfx = d_bpfx;
        A.zpfx = d_zpfx;
        A.z = d_z;
        A.T = L;
        launch_r128_steps(A, bpfx.back(), P, s);
    }
    rp.tm->mark(1, s);
    if (loud) launch_r128_track(d_z, d_zpfx, d_cvpfx, L, P, rp.d_folds, rp.d_curves, s);
    rp.tm->mark(2, s);
    launch_r128_peak(d_samples, d_off, d_n, d_cpfx, L, cpfx.back(), P, (r128_what_ & SDSP_R128_TRUE_PEAK) != 0, rp.d_peak, s);
    rp.tm->mark(3, s);
    SDSP_HIP_CHECK(hipGetLastError());
}

// The join: folds, peaks and curves read back and finished on the host (r128_core.hpp).
void Pipeline::r128_join() {
    R128Pending& rp = r128_pending_;
    if (!r128_out_ || !rp.on) return;
    const size_t L = rp.at.size();
    const bool loud = r128_what_ & SDSP_R128_LOUDNESS;
    hipStream_t s = d_.stream3;
    std::vector<unsigned int> pk(2 * L);
    std::vector<R128Folds> folds(L, R128Folds{});
    std::vector<float> cv(rp.d_curves ? (size_t)rp.cvpfx.back() : 0);
    SDSP_HIP_CHECK(hipMemcpyAsync(pk.data(), rp.d_peak, pk.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    if (loud) SDSP_HIP_CHECK(hipMemcpyAsync(folds.data(), rp.d_folds, L * sizeof(R128Folds), hipMemcpyDeviceToHost, s));
    if (!cv.empty()) SDSP_HIP_CHECK(hipMemcpyAsync(cv.data(), rp.d_curves, cv.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    SDSP_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t k = 0; k < L; k++) {
        TrackR128& o = (*r128_out_)[rp.at[k]];
        r128_finish(folds[k], sd_from_bits_f(pk[k]), sd_from_bits_f(pk[L + k]), rp.n[k], r128_what_, rp.P, &o.r);
        if (rp.d_curves) o.curves.assign(cv.begin() + (size_t)rp.cvpfx[k], cv.begin() + (size_t)rp.cvpfx[k + 1]);
    }
    sdsp_debug_r128_times& t = d_.last_r128;
    t.steps_ms = loud ? rp.tm->ms(0, 1) : 0.0;
    t.track_ms = loud ? rp.tm->ms(1, 2) : 0.0;
    t.peak_ms = rp.tm->ms(2, 3);
    t.tracks = L;
    t.steps = loud ? rp.steps : 0;
    rp = R128Pending{};
}

}  // namespace sdsp
