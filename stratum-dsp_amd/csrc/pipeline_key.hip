// pipeline_key.hip — the key path of a sub-batch (stage E of pipeline.hip's overview): its launch
// on the key and vote streams, the spectrogram conditioning and chroma, the join (late by default),
// the exact reruns of near-decision tracks and the beat-synchronous re-vote.
#include "key_timeline_plan.hpp"
#include "pipeline.hpp"

namespace sdsp {

// E: key (second stream; overlaps B-D).  The key path depends only on the trimmed signal, so it is
// forked onto the context's key stream right after trimming and joined before the results are
// read back: its bandwidth-bound STFT/mask/HPCP kernels run under the latency-bound tempo and beat
// kernels of the main stream.  bin: the base pass's tracks (the surviving ones).
KeyLaunch Pipeline::launch_key(const float* d_samples, const TempoPassIn& bin, const Front& f) {
    KeyLaunch kl;
    KeyTail& t = kl.tail;
    t.kp = key_vote_params(cfg_, false);  // near_check: set once the conditioning's path is known
    hipStream_t st = d_.stream;
    const int KFS = kfs_, KHOP = khop_;
    std::vector<uint64_t> ksrc;
    std::vector<float> kgain;
    double key_in_bytes = 0;
    for (size_t i = 0; i < bin.n_trim.size(); i++) {
        const uint64_t n = bin.n_trim[i];
        if (bpm_only_) break;  // SDSP_STAGES_BPM_ONLY: stages a1-a19 only, no key path
        if (n < (uint64_t)fs_ || n < (uint64_t)KFS) continue;  // key skipped or empty key spectrogram -> default key
        const uint64_t F8 = (n - KFS) / (uint64_t)KHOP + 1;
        kl.K.push_back((int)i);
        t.kpfx.push_back(t.kpfx.back() + F8);
        kl.ktile.push_back(kl.ktile.back() + (F8 + HP_FRAMES - 1) / HP_FRAMES);
        t.kseg.push_back(t.kseg.back() + (uint64_t)KV_ROW * seg_rows(t.kp, F8));
        ksrc.push_back(bin.src_off[i]);
        kgain.push_back(bin.gain_h[i]);
        key_in_bytes += 4.0 * (double)n;
    }
    const int NK = (int)kl.K.size();
    kl.kt.reset(new Timers());
    Timers& kt = *kl.kt;
    kt.init(d_);
    // what the main stream uploads for the key stream (read by it before the sub-batch's join)
    sb_parity_ ^= 1;
    const std::string EP = sb_parity_ ? "E1." : "E0.";
    // schedule knob (sdsp_debug_set_schedule): the key path on the main stream (per-kernel profiling)
    kl.serial_streams = nested_ || test_hooks().serial_streams.load() != 0;
    hipStream_t st2 = kl.serial_streams ? st : d_.stream2;
    hipStream_t st3 = kl.serial_streams ? st : d_.stream3;  // the key vote
    if (NK == 0) return kl;
    const int B8 = KFS / 2 + 1;
    const uint64_t total8 = t.kpfx.back();
    t.d_kpfx = c_.up(EP + "kpfx", t.kpfx);
    kl.d_ktile = c_.up(EP + "ktile", kl.ktile);
    uint64_t* d_kseg = c_.up(EP + "kseg", t.kseg);
    const std::vector<uint64_t> kstr = stft_strips(t.kpfx);
    uint64_t* d_kstr = c_.up(EP + "kstrip", kstr);
    uint64_t* d_ksrc = c_.up(EP + "ksrc", ksrc);
    float* d_kgain = c_.up(EP + "kgain", kgain);
    std::vector<int> kid((size_t)NK);
    for (int k = 0; k < NK; k++) kid[(size_t)k] = k;
    kl.d_kid = c_.up(EP + "kid", kid);
    FftTables& t8 = d_.tables(KFS, true);
    t.mags8 = c_.dev<float>("E.mags8", total8 * ks_);
    // uploads above were queued on the main stream: order the key stream after them
    kt.mark(7);
    SDSP_HIP_CHECK(hipStreamWaitEvent(st2, kt.ev[7], 0));
    kt.mark(0, st2);
    launch_stft(KFS, false, d_samples, t.d_kpfx, NK, total8, d_ksrc, d_kgain, KHOP, t8.window.as<float>(),
                stft_twp(t8, KFS, false), stft_rtp(t8, KFS, false), t.mags8, t.d_kpfx, ks_, nullptr, st2, d_kstr,
                kstr.back(), c_.dev<uint32_t>("E.redo", total8 + 1));
    SDSP_HIP_CHECK(hipGetLastError());
    kt.mark(1, st2);
    const KeyCond kc = key_condition(EP, t.mags8, t.kpfx, kl.ktile, t.d_kpfx, kl.d_ktile, kl.d_kid, st2, kt);
    kl.d_tune = kc.d_tune;
    std::vector<float> tpl(576);
    key_templates(tpl.data());
    t.d_tpl = c_.up(EP + "tpl", tpl);
    t.kp.near_check = kc.band ? 1 : 0;
    t.kp.cert_fixed = test_hooks().key_cert_fixed.load();  // sdsp_debug_set_key_cert
    float* d_cs = c_.dev<float>("E.chroma_s", total8 * 12);
    float* d_w = c_.dev<float>("E.weights", total8);
    float* d_sscr = c_.dev<float>("E.segscr", std::max<uint64_t>(t.kseg.back(), 1));
    kl.d_kout = c_.dev<KeyOut>(EP + "kout", (size_t)NK);
    if (kc.band && kc.d_ht) {
        t.ok = true;
        tail_buffers(t, kc, t.mags8, t.d_kpfx, total8);
        t.d_cs = d_cs;
        t.d_w = d_w;
        t.d_sscr = d_sscr;
    }
    // the key timeline's segment prefix (a request only): uploaded on the main stream like the templates
    uint64_t* d_kspfx = nullptr;
    if (kt_out_) {
        KeyTimelineOut& o = kl.ktl;
        for (int k = 0; k < NK; k++) {
            o.frames.push_back(t.kpfx[(size_t)k + 1] - t.kpfx[(size_t)k]);
            o.spfx.push_back(o.spfx.back() + kt_segments(o.frames.back(), kt_L_, kt_H_));
        }
        if (o.spfx.back() / KT_SEGS >= 0x7FFFFFFFull) throw HipError("key timeline: too many segments for one launch");
        d_kspfx = c_.up(EP + "kt_spfx", o.spfx);
        o.d_out = c_.dev<KtSeg>(EP + "kt_out", (size_t)std::max<uint64_t>(o.spfx.back(), 1));
    }
    // the sections request's cell plan (a request only): uploaded on the main stream alike
    if (sc_out_) {
        SectionsOut& o = kl.sc;
        for (int k = 0; k < NK; k++) {
            const uint64_t n = bin.n_trim[(size_t)kl.K[(size_t)k]];
            const uint64_t Fb = (n - (uint64_t)fs_) / (uint64_t)bin.hop + 1;  // (n >= fs_: a key track)
            const uint64_t nc = sc_cells(t.kpfx[(size_t)k + 1] - t.kpfx[(size_t)k], (uint64_t)KHOP, Fb, (uint64_t)bin.hop, sc_Cs_);
            o.cpfx.push_back(o.cpfx.back() + nc);
            o.tpfx.push_back(o.tpfx.back() + (nc + SC_TILE - 1) / SC_TILE);
        }
        if (o.cpfx.back() / 16 >= 0x7FFFFFFFull) throw HipError("sections: too many cells for one launch");
        const size_t cells = (size_t)std::max<uint64_t>(o.cpfx.back(), 1);
        o.d_cpfx = c_.up(EP + "sc_cpfx", o.cpfx);
        o.d_tpfx = c_.up(EP + "sc_tpfx", o.tpfx);
        o.d_m = c_.dev<float>(EP + "sc_m", 12 * cells);
        o.d_g = c_.dev<float>(EP + "sc_g", cells);
        o.d_N = c_.dev<float>(EP + "sc_N", cells);
        o.d_b = c_.dev<uint8_t>(EP + "sc_b", cells);
    }
    // the fingerprint request's cell and word plan (a request only), uploaded on the main stream alike;
    // the cell means are scratch of the sub-batch on the vote stream, the words go to the call's buffer
    uint64_t *d_fcpfx = nullptr, *d_fwpfx = nullptr, *d_fslot = nullptr;
    float* d_fm = nullptr;
    if (fp_out_) {
        FingerprintOut& o = kl.fp;
        std::vector<uint64_t> slot;
        for (int k = 0; k < NK; k++) {
            const int i = kl.K[(size_t)k];
            TrackFp& tf = fp_out_->tracks[f.slot[(size_t)i]];
            tf.on = true;
            tf.first = f.ts[(size_t)f.R[(size_t)i]];
            tf.n_cells = fp_cells(t.kpfx[(size_t)k + 1] - t.kpfx[(size_t)k], (uint64_t)KHOP, fp_Cs_);
            tf.W = fp_words(tf.n_cells);  // (<= the slot's lens / Cs - 2: the trimmed track is no longer than the raw one)
            o.cpfx.push_back(o.cpfx.back() + tf.n_cells);
            o.wpfx.push_back(o.wpfx.back() + tf.W);
            slot.push_back(fp_out_->slot[f.slot[(size_t)i]]);
        }
        if (o.cpfx.back() / 16 >= 0x7FFFFFFFull) throw HipError("fingerprint: too many cells for one launch");
        d_fcpfx = c_.up(EP + "fp_cpfx", o.cpfx);
        d_fwpfx = c_.up(EP + "fp_wpfx", o.wpfx);
        d_fslot = c_.up(EP + "fp_slot", slot);
        d_fm = c_.dev<float>("F.m", 12 * (size_t)std::max<uint64_t>(o.cpfx.back(), 1));
    }
    // the template upload above is on the main stream too; the vote follows the chroma on st2
    kt.mark(8);
    kt.mark(11, st2);
    SDSP_HIP_CHECK(hipStreamWaitEvent(st3, kt.ev[8], 0));
    SDSP_HIP_CHECK(hipStreamWaitEvent(st3, kt.ev[11], 0));
    kl.d_kdbg = dbg_on() ? c_.dev<KeyDbg>(EP + "kdbg", (size_t)NK) : nullptr;
    float* d_wdel = kc.d_edel ? c_.dev<float>("E.wdel", total8) : nullptr;
    // the call's last sub-batch votes with nothing beside it on the chip (its tail)
    launch_key_vote(kl.d_kid, NK, t.d_kpfx, kc.d_chroma, kc.d_energy, d_cs, d_w, d_sscr, d_kseg, t.d_tpl, t.kp,
                    kl.d_kout, st3, kl.d_kdbg, kc.d_edel, d_wdel, last_sub_ || nested_ || key_only_);
    SDSP_HIP_CHECK(hipGetLastError());
    // The key timeline (include/stratum_hip.h) reads the rows the vote just smoothed, behind it on the
    // vote stream and before ev[2], so both joins wait for it; the next sub-batch's vote, which
    // rewrites E.chroma_s, follows in stream order.  rerun_tail does not touch it: the chroma rows are
    // exact on the band path (only the frame energies are not), and the timeline uses no energies.
    if (d_kspfx) {
        launch_key_timeline(d_cs, t.d_kpfx, d_kspfx, NK, kl.ktl.spfx.back(), kt_L_, kt_H_, t.d_tpl, kl.ktl.d_out, st3);
        SDSP_HIP_CHECK(hipGetLastError());
    }
    // The sections request's chroma cell means read the same rows, under the same ordering.
    if (sc_out_ && kl.sc.cpfx.back() > 0) {
        kt.mark(3, st3);
        launch_section_chroma(d_cs, t.d_kpfx, kl.sc.d_cpfx, NK, kl.sc.cpfx.back(), sc_Cs_, (uint64_t)KHOP, kl.sc.d_m, st3);
        SDSP_HIP_CHECK(hipGetLastError());
        kt.mark(4, st3);
    }
    // The fingerprint request's cell means and words read the same rows, under the same ordering; the
    // words land in the call's buffer (fp_words_), which only the match after the last join reads.
    if (fp_out_ && kl.fp.wpfx.back() > 0) {
        fp_tm_.emplace_back(new Timers());
        Timers& ft = *fp_tm_.back();
        ft.init(d_);
        ft.mark(0, st3);
        launch_fp_cells(d_cs, t.d_kpfx, d_fcpfx, NK, kl.fp.cpfx.back(), fp_Cs_, (uint64_t)KHOP, d_fm, st3);
        ft.mark(1, st3);
        launch_fp_words(d_fm, d_fcpfx, d_fwpfx, d_fslot, NK, kl.fp.wpfx.back(), fp_words_, st3);
        SDSP_HIP_CHECK(hipGetLastError());
        ft.mark(2, st3);
    }
    kt.mark(2, st3);
    if (!nested_) SDSP_HIP_CHECK(hipEventRecord(d_.vote_done, st3));
    times_.stft8192_launches += 1;
    times_.stft8192_frames += total8;
    times_.stft8192_bytes += key_in_bytes + 4.0 * (double)total8 * (double)B8;
    return kl;
}

// Key spectrogram conditioning and chroma (src/lib.rs:1011-1197) of the key tracks whose frame
// prefix is kpfx, in place over mags8 on st2: the branch the configuration selects, with the
// parameters every launch takes.  sub_batch's key path and the key stage probe both run this.
KeyCond Pipeline::key_condition(const std::string& EP, float* mags8, const std::vector<uint64_t>& kpfx,
                                const std::vector<uint64_t>& ktile, uint64_t* d_kpfx, uint64_t* d_ktile, int* d_kid,
                                hipStream_t st2, Timers& kt) {
    const int NK = (int)kpfx.size() - 1;
    const int KFS = kfs_;
    const int B8 = KFS / 2 + 1;
    const float fres8 = (float)sr_ / (float)KFS;
    const uint64_t total8 = kpfx.back();
    float* d_tune = nullptr;  // per key track tuning offset (tuning compensation)
    // key spectrogram conditioning (src/lib.rs:1011-1060): the mask runs in place over HBM
    // (k_mask_r), then HPCP reads the masked spectrogram (DESIGN.md §4 on the fused variant)
    const bool use_log = cfg_.enable_key_log_frequency;  // :1062-1095
    const bool tuned = cfg_.enable_key_tuning_compensation && !use_log;
    const bool whiten = cfg_.enable_key_hpcp_whitening && cfg_.key_hpcp_whitening_smooth_bins >= 3;
    // the default key path (harmonic mask, plain HPCP, nothing else reading the masked
    // spectrogram): the mask stores only HPCP's peak band and folds the frame energies in
    // 64-bin blocks (k_mask_rp / k_hpcp_band); SDSP_KEY_EXACT_ENERGY builds
    // keep the reference's one sequential energy sum (k_mask_r / k_hpcp)
    KeyCond kc;
    HpcpParams& hp = kc.hp;
    hp.B = B8;
    hp.stride = ks_;
    key_peak_band(cfg_, sr_, &hp.pk_lo, &hp.pk_hi);
    hp.K = (int)std::max<uint64_t>(cfg_.key_hpcp_peaks_per_frame, 1);
    hp.hmax = (int)std::max<uint64_t>(cfg_.key_hpcp_num_harmonics, 1);
    hp.p = sd_clampf(cfg_.key_hpcp_mag_power, 0.05f, 1.0f);
    // sdsp_debug_key_energy_blocked answers the same; exact_energy_: the rerun of near-decision tracks
    // exact_energy_ on the same configurations (the rerun): the band path's mask storing every
    // bin (its masked values are k_mask_r's, bit for bit, at less cost), then k_hpcp's one
    // sequential energy sum; the block sums it also writes go unused
    const bool blocked = key_energy_blocked(cfg_, sr_);
    const bool band = kc.band = blocked && !exact_energy_;
    float* d_part = kc.d_part = blocked ? c_.dev<float>("E.kpart", total8 * (uint64_t)((B8 + 63) / 64)) : nullptr;
    if (blocked) {
        kc.st_lo = band ? hp.pk_lo - 1 : 0;
        kc.st_hi = band ? hp.pk_hi + 1 : B8 - 1;
        launch_mask_band(mags8, ks_, B8, d_kpfx, d_kid, NK, cfg_.key_harmonic_mask_power, kc.st_lo, kc.st_hi, d_part,
                         total8, st2);
    } else if (cfg_.enable_key_hpss_harmonic) {
        const KeyHpssParams kh = key_hpss_params(cfg_, sr_, B8, fres8, ks_);
        if (kh.nb > 0) {  // an empty band returns the spectrogram unchanged (extractor.rs:1408-1410)
            std::vector<uint64_t> moff(1, 0), mt(1, 0), at(1, 0);
            for (int k = 0; k < NK; k++) {
                const uint64_t F8 = kpfx[(size_t)k + 1] - kpfx[(size_t)k];
                const uint64_t nds = (F8 + (uint64_t)kh.step - 1) / (uint64_t)kh.step;
                moff.push_back(moff.back() + nds * (uint64_t)kh.nb);
                mt.push_back(mt.back() + ((nds + KH_TILE_FRAMES - 1) / KH_TILE_FRAMES) *
                                             (((uint64_t)kh.nb + KH_TILE_BINS - 1) / KH_TILE_BINS));
                at.push_back(at.back() + (F8 + KH_APPLY_FRAMES - 1) / KH_APPLY_FRAMES);
            }
            uint64_t* d_moff = c_.up(EP + "kh_off", moff);
            uint64_t* d_mt = c_.up(EP + "kh_mt", mt);
            uint64_t* d_at = c_.up(EP + "kh_at", at);
            float* d_kmask = c_.dev<float>("E.kh_mask", std::max<uint64_t>(moff.back(), 1));
            // the uploads are on the main stream
            kt.mark(9);
            SDSP_HIP_CHECK(hipStreamWaitEvent(st2, kt.ev[9], 0));
            launch_key_hpss(mags8, d_kpfx, d_mt, mt.back(), d_at, at.back(), d_moff, d_kid, NK, kh, d_kmask, st2);
        }
    } else if (cfg_.enable_key_harmonic_mask)
        launch_mask(mags8, ks_, B8, d_kpfx, d_kid, NK, (int)cfg_.key_spectrogram_smooth_margin,
                    cfg_.key_harmonic_mask_power, st2);
    else if (cfg_.enable_key_spectrogram_time_smoothing)
        launch_mask(mags8, ks_, B8, d_kpfx, d_kid, NK, (int)cfg_.key_spectrogram_smooth_margin,
                    cfg_.key_harmonic_mask_power, st2, true);
    // tuning offset per track (:1097-1119)
    if (tuned) {
        TuningParams tp = tuning_params(cfg_, sr_, B8, fres8, ks_);
        d_tune = kc.d_tune = c_.dev<float>("E.tune", (size_t)NK);
        launch_tuning(mags8, d_kpfx, d_kid, NK, tp, d_tune, st2);
        SDSP_HIP_CHECK(hipGetLastError());
    }
    float* d_chroma = kc.d_chroma = c_.dev<float>("E.chroma", total8 * 12);
    float* d_energy = kc.d_energy = c_.dev<float>("E.energy", total8);
    float* d_edel = nullptr;  // the band path's per-frame energy bounds (the vote's certificate)
    // the previous sub-batch's key vote (stream3) reads E.chroma / E.energy: the producers
    // below wait for it (an event never recorded counts as complete)
    // (a nested rerun has its own "X." buffers and runs in order on the main stream)
    if (!nested_) SDSP_HIP_CHECK(hipStreamWaitEvent(st2, d_.vote_done, 0));
    if (use_log) {  // :1120-1131
        const ChromaParams cp = chroma_params(cfg_, sr_, 1, B8, fres8, ks_);
        launch_chroma(1, mags8, d_kpfx, d_ktile, d_kid, NK, ktile.back(), cp, nullptr, d_chroma, d_energy, st2);
    } else if (cfg_.enable_key_hpcp && (d_tune || whiten || cfg_.enable_key_hpcp_bass_blend)) {  // :1133-1168
        const HpcpXParams hx = hpcp_x_params(cfg_, sr_, B8, fres8, whiten, ks_);
        launch_hpcp_x(mags8, d_kpfx, d_ktile, d_kid, NK, ktile.back(), hx, d_tune, d_chroma, d_energy, st2);
    } else if (cfg_.enable_key_hpcp) {
        std::vector<HarmEntry> ht =
            harm_table(B8, sr_, KFS, cfg_.soft_mapping_sigma, hp.hmax, cfg_.key_hpcp_harmonic_decay);
        HarmEntry* d_ht = c_.up(EP + "harm", ht);
        kc.d_ht = d_ht;
        // the table upload is queued on the main stream: order the key stream after it
        kt.mark(10);
        SDSP_HIP_CHECK(hipStreamWaitEvent(st2, kt.ev[10], 0));
        if (band) {
            d_edel = kc.d_edel = c_.dev<float>("E.edel", total8);
            launch_hpcp_band(mags8, d_kpfx, d_ktile, d_kid, NK, ktile.back(), hp, d_ht, d_part, total8, d_chroma,
                             d_energy, d_edel, st2);
        }
        else
            launch_hpcp(mags8, d_kpfx, d_ktile, d_kid, NK, ktile.back(), hp, d_ht, d_chroma, d_energy, st2);
    } else {  // :1169-1197 (the tuned variant only when |offset| > 1e-6)
        const ChromaParams cp = chroma_params(cfg_, sr_, 0, B8, fres8, ks_);
        launch_chroma(0, mags8, d_kpfx, d_ktile, d_kid, NK, ktile.back(), cp, d_tune, d_chroma, d_energy, st2);
    }
    SDSP_HIP_CHECK(hipGetLastError());
    return kc;
}

// run_locked's exact key rerun (key_only_): the key fields only, the tempo path is not run
void Pipeline::join_key_only(KeyLaunch& kl, const Front& f, std::vector<TrackRes>& res) {
    if (kl.K.empty()) return;
    SDSP_HIP_CHECK(hipStreamWaitEvent(d_.stream, kl.kt->ev[2], 0));
    const std::vector<KeyOut> ko = c_.down(kl.d_kout, kl.K.size());
    for (size_t k = 0; k < kl.K.size(); k++)
        if (ko[k].ok) set_key_fields(res[f.slot[(size_t)kl.K[k]]], ko[k]);
}

// The joins at the end of a sub-batch's main-stream work.  First the previous sub-batch's key
// results (its key work ran ahead of this one's on the key stream) and the exact rerun of its
// near-decision tracks on the main stream.  Then this sub-batch's: handed to key_pending_ for the
// next sub-batch (or run()) to read, or joined here; returns its key results, empty when deferred.
// Late join by default (+2 % in alternating bench runs on one box, 2,350 vs 2,301 tracks/s: the
// main stream otherwise idles ~45 ms per sub-batch waiting for the key tail); no_key_defer
// (sdsp_debug_set_schedule) joins at the end of each sub-batch (the tests' control).
std::vector<KeyOut> Pipeline::join_key(const float* d_samples, const std::vector<uint64_t>& in_off,
                                       const std::vector<uint64_t>& n_raw, const Front& f, KeyLaunch& kl,
                                       HostTrace& htr, std::vector<TrackRes>& res) {
    rerun_near(d_samples, in_off, n_raw, finish_key(res), res);
    std::vector<KeyOut> kout;
    const size_t NK = kl.K.size();
    const bool beat_sync = cfg_.enable_key_beat_synchronous && !cfg_.enable_key_log_frequency;
    const bool defer_key =
        NK > 0 && !beat_sync && !kl.serial_streams && !dbg_on() && test_hooks().no_key_defer.load() == 0;
    if (defer_key) {
        key_pending_.reset(new KeyPending());
        key_pending_->kt = std::move(kl.kt);
        key_pending_->d_kout = kl.d_kout;
        for (int i : kl.K) key_pending_->at.push_back(f.slot[(size_t)i]);
        for (int i : kl.K) key_pending_->first.push_back(f.ts[(size_t)f.R[(size_t)i]]);
        key_pending_->ktl = std::move(kl.ktl);
        key_pending_->sc = std::move(kl.sc);
        key_pending_->tail = std::move(kl.tail);
    } else if (NK > 0) {  // join the key stream
        SDSP_HIP_CHECK(hipStreamWaitEvent(d_.stream, kl.kt->ev[kl.sc.queued ? 13 : 2], 0));
        kout = c_.down(kl.d_kout, NK);
        if (kt_out_ || sc_out_) {
            std::vector<size_t> at;
            std::vector<uint64_t> first;
            for (int i : kl.K) at.push_back(f.slot[(size_t)i]), first.push_back(f.ts[(size_t)f.R[(size_t)i]]);
            key_timeline_results(kl.ktl, at, first);
            sections_results(kl.sc, *kl.kt, at, first);
        }
        htr("E join");
        times_.stft8192_ms += kl.kt->ms(0, 1);
        times_.key_ms += kl.kt->ms(1, 2);
    }
    return kout;
}

// A joined sub-batch's key timeline segments (downloaded with its key results) into the call's
// per-track entries: `at` the result slot and `first` the trim start of each key track.
void Pipeline::key_timeline_results(const KeyTimelineOut& ktl, const std::vector<size_t>& at,
                                    const std::vector<uint64_t>& first) {
    if (!kt_out_ || ktl.frames.empty()) return;
    const std::vector<KtSeg> seg = c_.down(ktl.d_out, (size_t)ktl.spfx.back());
    for (size_t k = 0; k < at.size(); k++) {
        TrackKt& o = (*kt_out_)[at[k]];
        o.on = true;
        o.F = ktl.frames[k];
        o.first = first[k];
        o.seg.assign(seg.begin() + (ptrdiff_t)ktl.spfx[k], seg.begin() + (ptrdiff_t)ktl.spfx[k + 1]);
    }
}

// The sections request behind the base pass (sub_batch calls it right after tempo_pass, whose E is
// only valid until the next pass with the same tag): k_section_energy on the main stream over the
// key tracks' base frames, then, on the vote stream behind an event wait on it and behind the chroma
// cell means queued by launch_key, the novelty and the boundary flags.  ev[13] follows ev[2] on the
// vote stream, so a join that waits for it has waited for the vote too; the next sub-batch's vote
// follows in stream order.
void Pipeline::section_novelty(KeyLaunch& kl, const TempoPassOut& bo) {
    SectionsOut& o = kl.sc;
    if (!sc_out_ || kl.K.empty() || o.cpfx.back() == 0) return;
    Timers& kt = *kl.kt;
    const std::string EP = sb_parity_ ? "E1." : "E0.";
    hipStream_t st3 = kl.serial_streams ? d_.stream : d_.stream3;
    std::vector<uint64_t> row0;
    for (int i : kl.K) row0.push_back(bo.fpfx[(size_t)i]);
    uint64_t* d_row0 = c_.up(EP + "sc_row0", row0);
    kt.mark(5);
    launch_section_energy(bo.E, d_row0, o.d_cpfx, (int)kl.K.size(), o.cpfx.back(), sc_Cs_, (uint64_t)cfg_.hop_size, o.d_g,
                          d_.stream);
    SDSP_HIP_CHECK(hipGetLastError());
    kt.mark(6);
    SDSP_HIP_CHECK(hipStreamWaitEvent(st3, kt.ev[6], 0));
    kt.mark(12, st3);
    launch_section_novelty(o.d_m, o.d_g, o.d_cpfx, o.d_tpfx, (int)kl.K.size(), o.tpfx.back(), (int)sc_req_.kernel_cells,
                           sc_req_.energy_weight, (uint64_t)sc_req_.min_gap_cells, sc_req_.min_strength, o.d_N, o.d_b, st3);
    SDSP_HIP_CHECK(hipGetLastError());
    kt.mark(13, st3);
    o.queued = true;
}

// A joined sub-batch's cell energies, novelty and boundary flags into the call's per-track entries.
void Pipeline::sections_results(const SectionsOut& sc, Timers& kt, const std::vector<size_t>& at,
                                const std::vector<uint64_t>& first) {
    if (!sc_out_ || sc.cpfx.size() != at.size() + 1) return;
    const size_t cells = (size_t)sc.cpfx.back();
    std::vector<float> g, N;
    std::vector<uint8_t> b;
    if (sc.queued) {
        g = c_.down(sc.d_g, cells);
        N = c_.down(sc.d_N, cells);
        b = c_.down(sc.d_b, cells);
        d_.last_sc.energy_ms += kt.ms(5, 6);
        d_.last_sc.chroma_ms += kt.ms(3, 4);
        d_.last_sc.novelty_ms += kt.ms(12, 13);
        d_.last_sc.cells += cells;
    }
    for (size_t k = 0; k < at.size(); k++) {
        TrackSc& o = (*sc_out_)[at[k]];
        o.on = true;
        o.first = first[k];
        if (!sc.queued) continue;
        const ptrdiff_t a = (ptrdiff_t)sc.cpfx[k], e = (ptrdiff_t)sc.cpfx[k + 1];
        o.g.assign(g.begin() + a, g.begin() + e);
        o.N.assign(N.begin() + a, N.begin() + e);
        o.b.assign(b.begin() + a, b.begin() + e);
    }
}

// The fingerprint request before the first sub-batch: the call's word buffer with a slot per track at
// a prefix of lens[t] / Cs, an upper bound of its words known now, so no sub-batch waits for another.
void Pipeline::fingerprint_plan(const std::vector<uint64_t>& n_raw) {
    FpOut& o = *fp_out_;
    const size_t T = n_raw.size();
    o = FpOut{};
    o.tracks.assign(T, TrackFp{});
    o.slot.assign(T + 1, 0);
    for (size_t i = 0; i < T; i++) {
        const uint64_t cap = n_raw[i] / fp_Cs_;
        if (cap >= FP_WMAX) throw HipError("fingerprint: a track of 2^27 words or more");
        o.slot[i + 1] = o.slot[i] + cap;
    }
    fp_words_ = c_.dev<uint32_t>("F.words", (size_t)std::max<uint64_t>(o.slot[T], 1));
    fp_tm_.clear();
}

namespace detail {
double fp_match_bands(Ctx& c, const std::string& tag, const uint32_t* d_words, const uint64_t* d_slot, const uint32_t* d_W,
                      int NC, uint32_t O, uint32_t min_overlap_words,
                      const std::function<void(int, int, const FpRec*)>& band) {
    if (NC < 2) return 0.0;
    // at most 64 MB of records per launch, whole tiles of rows
    const uint64_t per_row = (uint64_t)NC * sizeof(FpRec);
    const int rows_max = (int)std::max<uint64_t>(FP_TA, ((uint64_t)64 << 20) / per_row / FP_TA * FP_TA);
    const int rows_band = std::min(rows_max, (NC - 1 + FP_TA - 1) / FP_TA * FP_TA);  // (the last track has no pair of its own)
    FpRec* d_rec = c.dev<FpRec>(tag + "fp_rec", (size_t)rows_band * (size_t)NC);
    Timers tm;
    tm.init(c.d);
    double ms = 0.0;
    for (int r0 = 0; r0 < NC - 1; r0 += rows_band) {
        const int rows = std::min(rows_band, NC - 1 - r0);
        SDSP_HIP_CHECK(hipMemsetAsync(d_rec, 0, (size_t)rows * per_row, c.d.stream));
        tm.mark(0);
        launch_fp_match(d_words, d_slot, d_W, NC, r0, rows, (int)O, fp_min_overlap(min_overlap_words), d_rec, c.d.stream);
        SDSP_HIP_CHECK(hipGetLastError());
        tm.mark(1);
        const std::vector<FpRec> rec = c.down(d_rec, (size_t)rows * (size_t)NC);
        ms += tm.ms(0, 1);
        band(r0, r0 + rows, rec.data());
    }
    return ms;
}
}  // namespace detail

// The fingerprint request after the last join: every sub-batch's words are in the call's buffer (the
// main stream has waited for the vote stream's last event).  Downloads the words when asked for, and
// with SDSP_FP_MATCH compares every pair of the tracks with a word and status SDSP_OK on the device
// and keeps the pairs within max_ber.
void Pipeline::fingerprint_finish(const std::vector<TrackRes>& res) {
    FpOut& o = *fp_out_;
    const size_t T = o.tracks.size();
    sdsp_debug_fingerprint_times& lt = d_.last_fp;
    for (auto& ft : fp_tm_) lt.cells_ms += ft->ms(0, 1), lt.words_ms += ft->ms(1, 2);
    fp_tm_.clear();
    for (size_t i = 0; i < T; i++) lt.words += o.tracks[i].W;
    if (fp_req_.what & SDSP_FP_WORDS) o.words = c_.down(fp_words_, (size_t)o.slot[T]);
    if (!(fp_req_.what & SDSP_FP_MATCH)) return;
    std::vector<uint64_t> who, slot, first(T, 0);
    std::vector<uint32_t> W;
    for (size_t i = 0; i < T; i++) {
        first[i] = o.tracks[i].first;
        if (res[i].status != SDSP_OK || !o.tracks[i].on || o.tracks[i].W == 0) continue;
        who.push_back(i);
        slot.push_back(o.slot[i]);
        W.push_back((uint32_t)o.tracks[i].W);
    }
    const int NC = (int)who.size();
    lt.compared = (uint64_t)NC;
    lt.pairs = (uint64_t)NC * (uint64_t)(NC > 0 ? NC - 1 : 0) / 2;
    if (NC < 2) return;
    uint64_t* d_slot = c_.up("F.slot", slot);
    uint32_t* d_W = c_.up("F.W", W);
    lt.match_ms += fp_match_bands(c_, "F.", fp_words_, d_slot, d_W, NC, fp_req_.max_offset_words, fp_req_.min_overlap_words,
                                  [&](int r0, int r1, const FpRec* rec) {
                                      fp_assemble(rec, who, (size_t)r0, (size_t)r1, first.data(), fp_Cs_, fp_req_.max_ber,
                                                  &o.matches);
                                  });
}

// The pending key results (the previous sub-batch's, or at the end of run() the last one's) into
// their result slots; returns the tracks whose vote was near a decision.
std::vector<size_t> Pipeline::finish_key(std::vector<TrackRes>& res, bool keep_tail) {
    std::vector<size_t> near;
    if (!key_pending_) return near;
    std::unique_ptr<KeyPending> kp = std::move(key_pending_);
    SDSP_HIP_CHECK(hipStreamWaitEvent(d_.stream, kp->kt->ev[kp->sc.queued ? 13 : 2], 0));
    const std::vector<KeyOut> kout = c_.down(kp->d_kout, kp->at.size());
    key_timeline_results(kp->ktl, kp->at, kp->first);
    sections_results(kp->sc, *kp->kt, kp->at, kp->first);
    for (size_t k = 0; k < kp->at.size(); k++) {
        TrackRes& r = res[kp->at[k]];
        const KeyOut& ko = kout[k];
        if (!ko.ok) continue;
        set_key_fields(r, ko);
        r.key_near = ko.near;
        if (ko.near) near.push_back(kp->at[k]);
    }
    times_.stft8192_ms += kp->kt->ms(0, 1);
    times_.key_ms += kp->kt->ms(1, 2);
    if (keep_tail && kp->tail.ok) tail_ = std::move(kp);
    return near;
}

// The exact key rerun of the call's last sub-batch's near-decision tracks, in place:
// the reference's sequential frame-energy fold needs every masked bin, and the band path stored only
// HPCP's band.  The bins outside it still hold the STFT's magnitudes, so k_mask_rp completes the
// masked spectrogram there (the same masked values the nested rerun's full-bin mask stores), k_hpcp
// folds each frame's energy in bin order (and rewrites the same chroma), and the vote runs on the
// exact energies: the nested rerun's results without its front end and 8192-point STFT.
void Pipeline::rerun_tail(const std::vector<size_t>& near_all, std::vector<TrackRes>& res) {
    std::unique_ptr<KeyPending> kp = std::move(tail_);
    if (near_all.empty() || !kp || exact_energy_ || nested_) return;
    const KeyTail& t = kp->tail;
    const auto t0 = std::chrono::steady_clock::now();
    // a track that already failed keeps its error: its key fields are not reported, nothing to certify
    std::vector<size_t> near;
    for (size_t i : near_all)
        if (res[i].status == SDSP_OK) near.push_back(i);
    if (near.empty()) return;
    std::vector<int> sel;
    for (size_t i : near)
        for (size_t k = 0; k < kp->at.size(); k++)
            if (kp->at[k] == i) sel.push_back((int)k);
    if (sel.size() != near.size()) throw HipError("rerun_tail: a near track is not in the last sub-batch");
    const int n = (int)sel.size();
    std::vector<uint64_t> tp(1, 0), sp(1, 0);
    for (int k : sel) {
        const uint64_t F = t.kpfx[(size_t)k + 1] - t.kpfx[(size_t)k];
        tp.push_back(tp.back() + (F + HP_FRAMES - 1) / HP_FRAMES);
        sp.push_back(sp.back() + (t.kseg[(size_t)k + 1] - t.kseg[(size_t)k]));
    }
    hipStream_t st = d_.stream;
    int* d_sel = c_.up("E.tail_sel", sel);
    uint64_t* d_tp = c_.up("E.tail_tile", tp);
    uint64_t* d_sp = c_.up("E.tail_seg", sp);
    tail_exact(t, d_sel, n, d_tp, tp.back(), st);
    KeyParams kx = t.kp;
    kx.near_check = 0;  // the exact energies: nothing left to certify
    // (the vote writes out[track], so the selected tracks' entries of the sub-batch's KeyOut array)
    launch_key_vote(d_sel, n, t.d_kpfx, t.d_chroma, t.d_energy, t.d_cs, t.d_w, t.d_sscr, d_sp, t.d_tpl, kx, kp->d_kout,
                    st, nullptr, nullptr, nullptr, true);
    SDSP_HIP_CHECK(hipGetLastError());
    const std::vector<KeyOut> ko = c_.down(kp->d_kout, kp->at.size());
    for (int j = 0; j < n; j++) {
        TrackRes& r = res[near[(size_t)j]];
        const KeyOut& o = ko[(size_t)sel[(size_t)j]];
        if (!o.ok) {
            r.status = SDSP_ERR_PROCESSING;
            r.err = "Processing error: key certification rerun failed (no key from the exact energies)";
            r.key_rerun = true;  // the rerun ran: run_locked does not run it again
            continue;
        }
        set_key_fields(r, o);
        r.key_rerun = true;
    }
    reruns_ += (uint64_t)n;
    tail_reruns_ += (uint64_t)n;
    rerun_ms_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The in-place rerun's kernels over the band path's buffers: the mask on the bins outside the
// stored band, then the sequential-energy HPCP, for the selected key tracks.
void Pipeline::tail_exact(const KeyTail& t, const int* d_sel, int n, const uint64_t* d_tiles, uint64_t n_tiles,
                          hipStream_t st) {
    launch_mask_band(t.mags8, ks_, t.B8, t.d_kpfx, d_sel, n, cfg_.key_harmonic_mask_power, t.st_lo, t.st_hi, t.d_part,
                     t.total8, st, true);
    SDSP_HIP_CHECK(hipGetLastError());
    launch_hpcp(t.mags8, t.d_kpfx, d_tiles, d_sel, n, n_tiles, t.hp, t.d_ht, t.d_chroma, t.d_energy, st);
    SDSP_HIP_CHECK(hipGetLastError());
}

// The exact key rerun of near-decision tracks for a finished sub-batch, from inside
// the main pass: a nested key-only pipeline with the sequential energy fold, its buffers prefixed
// ("X.") and its key path on the main stream, whose queue then runs it in the slack the tempo path
// leaves beside the key stream.  The tracks of the last sub-batch are rerun by run_locked.
void Pipeline::rerun_near(const float* d_samples, const std::vector<uint64_t>& in_off, const std::vector<uint64_t>& n_raw,
                          const std::vector<size_t>& near, std::vector<TrackRes>& res) {
    if (near.empty() || exact_energy_ || nested_) return;
    std::vector<uint64_t> o2, l2;
    for (size_t i : near) o2.push_back(in_off[i]), l2.push_back(n_raw[i]);
    std::vector<TrackRes> r2;
    Pipeline px(d_, cfg_, sr_, SDSP_STAGES_FULL, true, true, true);
    px.run(d_samples, o2, l2, r2);
    for (size_t j = 0; j < near.size(); j++) {
        TrackRes& r = res[near[j]];
        if (r2[j].status != SDSP_OK) {  // the key fields are not certified: the track fails
            r.status = SDSP_ERR_PROCESSING;
            r.err = "Processing error: key certification rerun failed (" + r2[j].err + ")";
            continue;
        }
        set_key_fields(r, r2[j]);
        r.key_rerun = true;
    }
    reruns_ += near.size();
    rerun_ms_ += d_.last.total_ms;  // px.run's
}

void Pipeline::tail_buffers(KeyTail& t, const KeyCond& kc, float* mags8, uint64_t* d_kpfx, uint64_t total8) const {
    t.mags8 = mags8;
    t.d_kpfx = d_kpfx;
    t.d_part = kc.d_part;
    t.total8 = total8;
    t.st_lo = kc.st_lo;
    t.st_hi = kc.st_hi;
    t.B8 = kc.hp.B;
    t.hp = kc.hp;
    t.d_ht = kc.d_ht;
    t.d_chroma = kc.d_chroma;
    t.d_energy = kc.d_energy;
}

// Beat-synchronous chroma (src/lib.rs:1121-1133): for key tracks with a non-empty beat grid the
// chroma rows are the beat intervals' mean frame chroma; the key vote is re-run on them and
// replaces those tracks' entries of kout.
void Pipeline::beat_sync_revote(const KeyLaunch& kl, const ResultsHost& rh, std::vector<KeyOut>& kout) {
    hipStream_t st = d_.stream;
    const int NK = (int)kl.K.size();
    std::vector<int> sel, sel_id;
    std::vector<uint64_t> sb_off, rpfx(1, 0), sseg(1, 0);
    for (int k = 0; k < NK; k++) {
        const int i = kl.K[(size_t)k];
        const int nb = rh.bout[(size_t)i].ok > 0 ? rh.bout[(size_t)i].n_beats : 0;
        if (nb < 1) continue;
        sel.push_back(k);
        sel_id.push_back((int)sel_id.size());
        sb_off.push_back(rh.bpfx[(size_t)i]);
        const uint64_t rows = (uint64_t)nb - 1;
        rpfx.push_back(rpfx.back() + rows);
        sseg.push_back(sseg.back() + (uint64_t)KV_ROW * seg_rows(kl.tail.kp, rows));
    }
    const int NS = (int)sel.size();
    if (NS == 0) return;
    const uint64_t total8 = kl.tail.kpfx.back();
    ChromaParams cp = chroma_params(cfg_, sr_, 0, kfs_ / 2 + 1, (float)sr_ / (float)kfs_, ks_);
    cp.gate_small = 0;  // extract_beat_synchronous_chroma takes the offset as is
    float* fc = c_.dev<float>("E.bs_fc", total8 * 12);
    float* fe = c_.dev<float>("E.bs_fe", total8);
    launch_chroma(0, kl.tail.mags8, kl.tail.d_kpfx, kl.d_ktile, kl.d_kid, NK, kl.ktile.back(), cp, kl.d_tune, fc, fe, st);
    int* d_sel = c_.up("E.bs_sel", sel);
    int* d_sid = c_.up("E.bs_id", sel_id);
    uint64_t* d_sboff = c_.up("E.bs_boff", sb_off);
    uint64_t* d_rpfx = c_.up("E.bs_rpfx", rpfx);
    uint64_t* d_sseg = c_.up("E.bs_seg", sseg);
    const uint64_t rows = std::max<uint64_t>(rpfx.back(), 1);
    float* bc = c_.dev<float>("E.bs_chroma", rows * 12);
    float* be = c_.dev<float>("E.bs_energy", rows);
    const float fd = (float)khop_ / (float)sr_;
    launch_beat_sync(d_sel, NS, kl.tail.d_kpfx, fc, fe, rh.d_cbeats, d_sboff, d_rpfx, fd, bc, be, st);
    float* bcs = c_.dev<float>("E.bs_chroma_s", rows * 12);
    float* bw = c_.dev<float>("E.bs_weights", rows);
    float* bscr = c_.dev<float>("E.bs_segscr", std::max<uint64_t>(sseg.back(), 1));
    KeyOut* d_bko = c_.dev<KeyOut>("E.bs_kout", (size_t)NS);
    launch_key_vote(d_sid, NS, d_rpfx, bc, be, bcs, bw, bscr, d_sseg, kl.tail.d_tpl, kl.tail.kp, d_bko, st);
    SDSP_HIP_CHECK(hipGetLastError());
    std::vector<KeyOut> bko = c_.down(d_bko, (size_t)NS);
    for (int j = 0; j < NS; j++) kout[(size_t)sel[(size_t)j]] = bko[(size_t)j];
}

}  // namespace sdsp
