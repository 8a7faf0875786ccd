// pipeline_abi.hip — the C ABI entry points over the pipeline (sdsp_analyze_audio / _batch /
// _batch_device, the stage probes, synthetic tracks): result assembly, the certified key rerun of
// the last sub-batch's near-decision tracks, the per-device staging pool of sdsp_analyze_batch.
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "batch_sched.hpp"
#include "key_timeline_plan.hpp"
#include "overview_plan.hpp"
#include "pipeline.hpp"
#include "sections_core.hpp"

namespace sdsp {
namespace {

std::string fmt2(float v) {
    char b[64];
    std::snprintf(b, sizeof b, "%.2f", (double)v);
    return b;
}

char* dup_str(const std::string& s) {
    char* p = (char*)std::malloc(s.size() + 1);
    std::memcpy(p, s.c_str(), s.size() + 1);
    return p;
}
float* dup_f(const std::vector<float>& v) {
    if (v.empty()) return nullptr;
    float* p = (float*)std::malloc(v.size() * sizeof(float));
    std::memcpy(p, v.data(), v.size() * sizeof(float));
    return p;
}

// result assembly + warnings (src/lib.rs:1561-1619)
void fill_result(const TrackRes& r, uint32_t sr, float ms, sdsp_result* o) {
    std::memset(o, 0, sizeof(*o));
    o->status = r.status;
    o->tempogram_multi_res_triggered = o->tempogram_multi_res_used = -1;
    o->tempogram_percussive_triggered = o->tempogram_percussive_used = -1;
    if (r.status != SDSP_OK) {
        std::snprintf(o->error_message, sizeof o->error_message, "%s", r.err.c_str());
        return;
    }
    o->bpm = r.bpm;
    o->bpm_confidence = r.bpm_conf;
    o->key_mode = r.key_mode;
    o->key_tonic = (uint32_t)r.key_tonic;
    o->key_confidence = r.key_conf;
    o->key_clarity = r.key_clarity;
    o->beats = dup_f(r.beats);
    o->n_beats = r.beats.size();
    o->downbeats = dup_f(r.downs);
    o->n_downbeats = r.downs.size();
    o->bars = dup_f(r.downs);
    o->n_bars = r.downs.size();
    o->grid_stability = r.stability;
    o->duration_seconds = r.duration;
    o->sample_rate = sr;
    o->processing_time_ms = ms;
    std::snprintf(o->algorithm_version, sizeof o->algorithm_version, "0.1.0-alpha");
    o->onset_method_consensus = r.onset_consensus;
    o->methods_used = 7;
    std::vector<std::string> w;
    if (r.bpm == 0.0f) w.push_back("BPM detection failed: insufficient onsets or estimation error");
    if (r.stability < 0.5f) w.push_back("Low beat grid stability: " + fmt2(r.stability) + " (may indicate tempo variation)");
    if (r.key_conf < 0.3f)
        w.push_back("Low key detection confidence: " + fmt2(r.key_conf) + " (may indicate ambiguous or atonal music)");
    if (r.key_clarity < 0.2f) {
        w.push_back("Low key clarity: " + fmt2(r.key_clarity) + " (track may be atonal or have weak tonality)");
        o->flags |= SDSP_FLAG_WEAK_TONALITY;
    }
    o->n_warnings = w.size();
    if (!w.empty()) {
        o->warnings = (char**)std::malloc(w.size() * sizeof(char*));
        for (size_t i = 0; i < w.size(); i++) o->warnings[i] = dup_str(w[i]);
    }
    o->has_tempogram_candidates = r.has_cands;
    if (r.has_cands && !r.cands.empty()) {
        o->n_tempogram_candidates = r.cands.size();
        o->tempogram_candidates = (sdsp_tempo_candidate*)std::malloc(r.cands.size() * sizeof(sdsp_tempo_candidate));
        std::memcpy(o->tempogram_candidates, r.cands.data(), r.cands.size() * sizeof(sdsp_tempo_candidate));
    }
    o->tempogram_multi_res_triggered = r.mr_trig;
    o->tempogram_multi_res_used = r.mr_used;
    o->tempogram_percussive_triggered = r.perc_trig;
    o->tempogram_percussive_used = r.perc_used;
}

// one track's overview: the arrays for a track that is OK, the config-wide fields for every track
void fill_overview(const TrackOv& t, int status, const sdsp_config& cfg, uint32_t sr, const sdsp_overview_request& req,
                   sdsp_overview* o) {
    std::memset(o, 0, sizeof(*o));
    o->status = status;
    o->frame_size = (uint32_t)cfg.frame_size;
    o->hop_size = (uint32_t)cfg.hop_size;
    ov_band_bins(req.low_max_hz, req.mid_max_hz, cfg.frame_size, sr, &o->band_bins[0], &o->band_bins[1]);
    if (status != SDSP_OK) return;
    o->n_columns = t.C;
    o->n_frames = t.F;
    o->first_sample = t.first;
    o->n_samples = t.n;
    if (t.C == 0) return;
    // one block for the five arrays (sdsp_overview_free frees it through smin)
    float* p = (float*)std::malloc(5 * (size_t)t.C * sizeof(float));
    std::memcpy(p, t.blk.get() + t.at, 5 * (size_t)t.C * sizeof(float));
    o->smin = p;
    o->smax = p + t.C;
    o->low = p + 2 * t.C;
    o->mid = p + 3 * t.C;
    o->high = p + 4 * t.C;
}

// A checked key timeline request: L and H of key_timeline_plan, and where the timelines go.
struct KtCall {
    uint32_t L = 0, H = 0;
    float min_conf = 0.0f;
    sdsp_key_timeline* out = nullptr;
};
uint32_t kt_khop(const sdsp_config& c) {
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(key_hop(c), 1), INT32_MAX);
}

// One track's timeline from its segments as the kernel wrote them: starts, timestamps, the primary
// key and the changes (key_timeline_plan.hpp) on the host; the call-wide fields for every track.
void fill_key_timeline(const TrackKt& t, int status, const sdsp_config& cfg, uint32_t sr, const KtCall& kc,
                       sdsp_key_timeline* o) {
    std::memset(o, 0, sizeof(*o));
    o->status = status;
    o->segment_frames = kc.L;
    o->hop_frames = kc.H;
    o->frame_size = (uint32_t)std::min<uint64_t>(key_fft(cfg), STFT_GEN_MAX);
    o->hop_size = kt_khop(cfg);
    if (status != SDSP_OK) return;
    o->primary_key = -1;
    if (!t.on) return;  // the key path did not run (a short track)
    o->n_frames = t.F;
    o->first_sample = t.first;
    const uint64_t S = t.seg.size();
    if (S == 0) return;
    const float fps = kt_fps(sr, o->hop_size);
    std::vector<int32_t> key((size_t)S);
    std::vector<float> conf((size_t)S);
    for (uint64_t s = 0; s < S; s++) key[(size_t)s] = t.seg[(size_t)s].key, conf[(size_t)s] = t.seg[(size_t)s].conf;
    kt_primary(key.data(), conf.data(), S, &o->primary_key, &o->primary_confidence, &o->primary_count);
    std::vector<sdsp_key_change> ch;
    for (uint64_t i = 1; i < S; i++) {
        float cc;
        if (!kt_change(key.data(), conf.data(), i, kc.min_conf, &cc)) continue;
        sdsp_key_change c{};
        c.segment = i;
        c.timestamp = kt_timestamp(i, kc.H, fps);
        c.from_key = key[(size_t)i - 1];
        c.to_key = key[(size_t)i];
        c.confidence = cc;
        ch.push_back(c);
    }
    // one block for both arrays (sdsp_key_timeline_free frees it through segments)
    static_assert(sizeof(sdsp_key_segment) % alignof(sdsp_key_change) == 0, "changes follow the segments");
    char* p = (char*)std::malloc((size_t)S * sizeof(sdsp_key_segment) + ch.size() * sizeof(sdsp_key_change));
    o->segments = (sdsp_key_segment*)p;
    for (uint64_t s = 0; s < S; s++) {
        const KtSeg& g = t.seg[(size_t)s];
        sdsp_key_segment& e = o->segments[s];
        std::memset(&e, 0, sizeof e);
        e.start_frame = kt_start(s, kc.H);
        e.timestamp = kt_timestamp(s, kc.H, fps);
        e.key = g.key;
        e.confidence = g.conf;
        e.clarity = g.clarity;
        for (int j = 0; j < 3; j++) e.top_keys[j] = g.top_keys[j], e.top_scores[j] = g.top_scores[j];
    }
    o->n_segments = S;
    if (!ch.empty()) {
        o->changes = (sdsp_key_change*)(p + (size_t)S * sizeof(sdsp_key_segment));
        std::memcpy(o->changes, ch.data(), ch.size() * sizeof(sdsp_key_change));
        o->n_changes = ch.size();
    }
}

// A checked levels request and where the levels go.
struct LvCall {
    uint32_t what = 0;
    sdsp_levels* out = nullptr;
};
// One track's levels: every field for a track that gets levels (TrackLv::on: status SDSP_OK whatever
// the analysis status), else the analysis status and zeroed fields.
void fill_levels(const TrackLv& t, int status, const sdsp_config& cfg, uint32_t sr, sdsp_levels* o) {
    std::memset(o, 0, sizeof(*o));
    o->status = t.on ? (int32_t)SDSP_OK : status;
    if (!t.on) return;
    for (int m = 0; m < 3; m++) o->method[m] = t.method[m];
    o->applied_gain = t.applied_gain;
    o->n_samples = t.n;
    o->trim_start = t.ts;
    o->trim_end = t.te;
    o->frame_size = (uint32_t)cfg.frame_size;
    o->threshold_db = cfg.min_amplitude_db;
    const size_t R = t.regions.size() / 2;
    if (R == 0) return;
    o->regions = (sdsp_silence_region*)std::malloc(R * sizeof(sdsp_silence_region));
    for (size_t r = 0; r < R; r++) {
        sdsp_silence_region& e = o->regions[r];
        std::memset(&e, 0, sizeof e);
        e.start_sample = t.regions[2 * r];
        e.end_sample = t.regions[2 * r + 1];
        e.duration_seconds = (float)(e.end_sample - e.start_sample) / (float)sr;
    }
    o->n_regions = R;
}

// A checked tempo map request and where the maps go.
struct TmCall {
    uint32_t what = 0;
    sdsp_tempo_map* out = nullptr;
};
// One track's tempo map: the analysis status and zeroed fields unless the track is SDSP_OK;
// SDSP_ERR_PROCESSING for a map whose segments outgrew their capacity.  Both lists share one block.
void fill_tempo_map(const TrackTm& t, int status, sdsp_tempo_map* o) {
    std::memset(o, 0, sizeof(*o));
    o->status = status;
    if (status != SDSP_OK || !t.on) return;
    if (t.o.ok < 0) {
        o->status = SDSP_ERR_PROCESSING;
        return;
    }
    o->nominal_bpm = t.bpm;
    o->nominal_confidence = t.conf;
    o->first_sample = t.first;
    if (t.o.ok > 0) {
        o->has_grid = 1;
        o->has_variation = (int8_t)t.o.has_var;
        o->refined = (int8_t)t.o.refined;
        o->time_signature_scored = (int8_t)t.o.ts_scored;
        o->hmm_beats = (uint32_t)t.o.hmm_beats;
        o->beats_per_bar = (uint32_t)t.o.bpb;
        o->time_signature_confidence = t.o.ts_conf;
        for (int k = 0; k < 3; k++) o->time_signature_scores[k] = t.o.score[k];
    }
    const size_t S = t.segs.size(), N = t.onsets.size();
    if (S + N == 0) return;
    char* blk = (char*)std::malloc(S * sizeof(sdsp_tempo_segment) + N * sizeof(uint32_t));
    if (!blk) throw std::bad_alloc();
    if (S) {
        o->segments = (sdsp_tempo_segment*)blk;
        for (size_t k = 0; k < S; k++) {
            sdsp_tempo_segment& e = o->segments[k];
            const TmSeg& g = t.segs[k];
            std::memset(&e, 0, sizeof e);
            e.start_time = g.start;
            e.end_time = g.end;
            e.bpm = g.bpm;
            e.confidence = g.conf;
            e.is_variable = (uint8_t)(g.variable != 0);
            e.updated = (uint8_t)(g.updated != 0);
            e.n_onsets = g.n_onsets;
            e.updated_bpm = g.ubpm;
            e.updated_confidence = g.uconf;
            e.n_beats = g.n_beats;
        }
        o->n_segments = S;
    }
    if (N) {
        o->onsets = (uint32_t*)(blk + S * sizeof(sdsp_tempo_segment));
        std::memcpy(o->onsets, t.onsets.data(), N * sizeof(uint32_t));
        o->n_onsets = N;
    }
}

// A checked sections request: its cell Cs, and where the sections go.
struct ScCall {
    sdsp_sections_request req{};
    uint64_t Cs = 0;
    sdsp_sections* out = nullptr;
};
// One track's sections from its cell energies, novelty and boundary flags as the kernels wrote
// them: gmax and nmax (order-free maxima), the section list with its energies, and the snap to the
// result's downbeats (sections_core.hpp) on the host.  The list and the curves share one block.
void fill_sections(const TrackSc& t, const TrackRes& r, uint32_t sr, const ScCall& sc, sdsp_sections* o) {
    std::memset(o, 0, sizeof(*o));
    o->status = r.status;
    o->cell_samples = sc.Cs;
    if (r.status != SDSP_OK || !t.on) return;  // (not on: the key path did not run, n_cells 0)
    o->first_sample = t.first;
    const uint64_t nc = t.g.size();
    o->n_cells = nc;
    if (nc == 0) return;
    float gmax = t.g[0], nmax = t.N[0];
    for (uint64_t c = 1; c < nc; c++) gmax = sd_maxf(gmax, t.g[(size_t)c]), nmax = sd_maxf(nmax, t.N[(size_t)c]);
    o->gmax = gmax;
    o->nmax = nmax;
    std::vector<sdsp_section> secs;
    if (sc.req.what & SDSP_SECTIONS_LIST)
        secs = sc_assemble(t.g.data(), t.N.data(), t.b.data(), nc, sc.Cs, sr, r.downs.data(), r.downs.size(),
                           sc.req.snap_seconds);
    const size_t S = secs.size(), NC = (sc.req.what & SDSP_SECTIONS_CURVE) ? (size_t)nc : 0;
    if (S + NC == 0) return;
    static_assert(sizeof(sdsp_section) % alignof(float) == 0, "the curves follow the sections");
    char* blk = (char*)std::malloc(S * sizeof(sdsp_section) + 2 * NC * sizeof(float));
    if (!blk) throw std::bad_alloc();
    if (S) {
        o->sections = (sdsp_section*)blk;
        std::memcpy(o->sections, secs.data(), S * sizeof(sdsp_section));
        o->n_sections = S;
    }
    if (NC) {
        o->novelty = (float*)(blk + S * sizeof(sdsp_section));
        o->energy = o->novelty + NC;
        std::memcpy(o->novelty, t.N.data(), NC * sizeof(float));
        std::memcpy(o->energy, t.g.data(), NC * sizeof(float));
        o->n_curve = NC;
    }
}

// A checked programme loudness request and where the results go.
struct R128Call {
    uint32_t what = 0;
    sdsp_r128* out = nullptr;
};
// One track's programme loudness: every field for a measured track (TrackR128::on: status SDSP_OK
// whatever the analysis status), else the analysis status and zeroed fields.  Both curves share one
// block, the momentary curve first.
void fill_r128(const TrackR128& t, int status, sdsp_r128* o) {
    std::memset(o, 0, sizeof(*o));
    o->status = t.on ? (int32_t)SDSP_OK : status;
    if (!t.on) return;
    *o = t.r;
    o->momentary = o->short_term = nullptr;
    if (t.curves.empty()) return;
    float* blk = (float*)std::malloc(t.curves.size() * sizeof(float));
    if (!blk) throw std::bad_alloc();
    std::memcpy(blk, t.curves.data(), t.curves.size() * sizeof(float));
    o->momentary = blk;
    o->short_term = blk + o->n_momentary;
}

// A checked fingerprint request: its cell Cs, and where the fingerprints and the match list go.
struct FpCall {
    sdsp_fingerprint_request req{};
    uint64_t Cs = 0;
    sdsp_fingerprint* out = nullptr;
    sdsp_fingerprint_matches* matches = nullptr;
};
// The call's fingerprints and match list from the pipeline's FpOut and the final statuses: a track
// that failed (also after the match ran: a certification rerun) is not compared and takes its
// matches with it.
void fill_fingerprints(const FpOut& f, const std::vector<TrackRes>& res, const FpCall& fc) {
    const size_t T = res.size();
    const bool match = (fc.req.what & SDSP_FP_MATCH) != 0;
    std::vector<sdsp_fingerprint_match> ms;
    uint64_t compared = 0;
    for (size_t i = 0; i < T; i++) {
        sdsp_fingerprint* o = &fc.out[i];
        std::memset(o, 0, sizeof(*o));
        o->status = res[i].status;
        o->cell_samples = fc.Cs;
        const TrackFp& t = f.tracks[i];
        if (res[i].status != SDSP_OK || !t.on) continue;  // (not on: the key path did not run, n_cells 0)
        o->first_sample = t.first;
        o->n_cells = t.n_cells;
        o->n_words = t.W;
        if (t.W > 0) compared++;
    }
    if (match)
        for (const sdsp_fingerprint_match& m : f.matches)
            if (res[(size_t)m.a].status == SDSP_OK && res[(size_t)m.b].status == SDSP_OK) {
                ms.push_back(m);
                fc.out[m.a].n_matches++;
                fc.out[m.b].n_matches++;
            }
    // allocate last, so a failed allocation leaves nothing behind to free
    sdsp_fingerprint_match* list = nullptr;
    if (!ms.empty()) {
        list = (sdsp_fingerprint_match*)std::malloc(ms.size() * sizeof(sdsp_fingerprint_match));
        if (!list) throw std::bad_alloc();
        std::memcpy(list, ms.data(), ms.size() * sizeof(sdsp_fingerprint_match));
    }
    if (fc.req.what & SDSP_FP_WORDS)
        for (size_t i = 0; i < T; i++) {
            sdsp_fingerprint* o = &fc.out[i];
            if (o->n_words == 0) continue;
            o->words = (uint32_t*)std::malloc((size_t)o->n_words * sizeof(uint32_t));
            if (!o->words) {
                for (size_t j = 0; j < i; j++) sdsp_fingerprint_free(&fc.out[j]);
                std::free(list);
                throw std::bad_alloc();
            }
            std::memcpy(o->words, f.words.data() + f.slot[i], (size_t)o->n_words * sizeof(uint32_t));
        }
    if (fc.matches) {
        std::memset(fc.matches, 0, sizeof(*fc.matches));
        if (match) {
            fc.matches->n_compared = compared;
            fc.matches->n_pairs = compared * (compared > 0 ? compared - 1 : 0) / 2;
            fc.matches->n_matches = ms.size();
            fc.matches->matches = list;
        }
    }
}

// One device-resident batch on `device`.  The engine's main stream first waits for `user_stream`
// (everything queued on it so far) and for `wait_ev` (a copy's completion), whichever are given.
// The batch on a context whose mutex the caller holds (run_device, and sdsp_analyze_audio's
// direct path, which stages its one track into a context buffer under the same lock).
int32_t run_locked(DeviceCtx& d, const float* d_samples, const uint64_t* offsets, const uint64_t* lens, uint64_t n,
                   uint32_t sr, const sdsp_config* cfg, void* user_stream, sdsp_result* outs, int stages,
                   hipEvent_t wait_ev, const sdsp_overview_request* req = nullptr, sdsp_overview* ovs = nullptr,
                   const KtCall* ktc = nullptr, const LvCall* lvc = nullptr, const TmCall* tmc = nullptr,
                   const ScCall* scc = nullptr, const R128Call* rc = nullptr, const FpCall* fc = nullptr) {
    if (stages != SDSP_STAGES_FULL && stages != SDSP_STAGES_BPM_ONLY) throw HipError("unknown stage mask");
    if (user_stream) {
        hipEvent_t ev;
        SDSP_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        SDSP_HIP_CHECK(hipEventRecord(ev, (hipStream_t)user_stream));
        SDSP_HIP_CHECK(hipStreamWaitEvent(d.stream, ev, 0));
        SDSP_HIP_CHECK(hipEventDestroy(ev));
    }
    if (wait_ev) SDSP_HIP_CHECK(hipStreamWaitEvent(d.stream, wait_ev, 0));
    auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> off(offsets, offsets + n), ln(lens, lens + n);
    std::vector<TrackRes> res;
    std::vector<TrackOv> ov;
    Pipeline p(d, *cfg, sr, stages);
    d.last_ov = sdsp_debug_overview_times{};
    if (req) p.set_overview(*req, &ov);
    std::vector<TrackKt> ktl;
    if (ktc) p.set_key_timeline(ktc->L, ktc->H, &ktl);
    std::vector<TrackLv> lvl;
    d.last_lv = sdsp_debug_levels_times{};
    if (lvc) p.set_levels(lvc->what, &lvl);
    std::vector<TrackTm> tml;
    d.last_tm = sdsp_debug_tempo_map_times{};
    if (tmc) p.set_tempo_map(tmc->what, &tml);
    std::vector<TrackSc> scl;
    d.last_sc = sdsp_debug_sections_times{};
    if (scc) p.set_sections(scc->req, scc->Cs, &scl);
    std::vector<TrackR128> r128l;
    d.last_r128 = sdsp_debug_r128_times{};
    if (rc) p.set_r128(rc->what, &r128l);
    FpOut fpo;
    d.last_fp = sdsp_debug_fingerprint_times{};
    if (fc) p.set_fingerprint(fc->req, fc->Cs, &fpo);
    try {
        p.run(d_samples, off, ln, res);
        // Certified block energies: a track whose key vote had an energy-dependent
        // decision within its margin (KeyOut::near) has its key path run again with the reference's
        // sequential frame-energy fold, and those key fields replace its own (everything else is
        // independent of the key energies).
        std::vector<size_t> near;
        d.last_near.assign(res.size(), 0);
        for (size_t i = 0; i < res.size(); i++) {
            if (res[i].key_near) d.last_near[i] = (uint8_t)res[i].key_near;
            if (res[i].key_near && !res[i].key_rerun) near.push_back(i);  // the last sub-batch's
        }
        if (!near.empty()) {
            const sdsp_stage_times first = d.last;
            std::vector<uint64_t> o2, l2;
            for (size_t i : near) o2.push_back(off[i]), l2.push_back(ln[i]);
            std::vector<TrackRes> r2;
            Pipeline px(d, *cfg, sr, stages, true, true);
            px.run(d_samples, o2, l2, r2);
            for (size_t j = 0; j < near.size(); j++) {
                TrackRes& r = res[near[j]];
                if (r2[j].status != SDSP_OK) {  // (the same front end as the main pass) uncertified: fail
                    r.status = SDSP_ERR_PROCESSING;
                    r.err = "Processing error: key certification rerun failed (" + r2[j].err + ")";
                    continue;
                }
                set_key_fields(r, r2[j]);
            }
            // the call's stage times stay the main pass's; the rerun is reported beside them
            const double rerun_ms = d.last.total_ms;
            d.last = first;
            d.last.key_reruns += near.size();
            d.last.rerun_ms += rerun_ms;
            d.last.total_ms += rerun_ms;
        }
    } catch (...) {
        // a sub-batch may have queued key-stream work (the late join) before a later one threw:
        // nothing of this call may still run on the engine's streams once the context lock is
        // released, or the next call's uploads into the same context buffers would race it
        for (hipStream_t s : d.own) (void)hipStreamSynchronize(s);
        throw;
    }
    const float ms = (float)(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() /
                             (double)std::max<uint64_t>(n, 1));
    for (uint64_t i = 0; i < n; i++) fill_result(res[(size_t)i], sr, ms, &outs[i]);
    if (req)
        for (uint64_t i = 0; i < n; i++) fill_overview(ov[(size_t)i], res[(size_t)i].status, *cfg, sr, *req, &ovs[i]);
    if (ktc)
        for (uint64_t i = 0; i < n; i++)
            fill_key_timeline(ktl[(size_t)i], res[(size_t)i].status, *cfg, sr, *ktc, &ktc->out[i]);
    if (lvc)
        for (uint64_t i = 0; i < n; i++) fill_levels(lvl[(size_t)i], res[(size_t)i].status, *cfg, sr, &lvc->out[i]);
    if (tmc)
        for (uint64_t i = 0; i < n; i++) fill_tempo_map(tml[(size_t)i], res[(size_t)i].status, &tmc->out[i]);
    if (scc)
        for (uint64_t i = 0; i < n; i++) fill_sections(scl[(size_t)i], res[(size_t)i], sr, *scc, &scc->out[i]);
    if (rc)
        for (uint64_t i = 0; i < n; i++) fill_r128(r128l[(size_t)i], res[(size_t)i].status, &rc->out[i]);
    if (fc) fill_fingerprints(fpo, res, *fc);
    return SDSP_OK;
}

int32_t run_device(int device, const float* d_samples, const uint64_t* offsets, const uint64_t* lens, uint64_t n,
                   uint32_t sr, const sdsp_config* cfg, void* user_stream, sdsp_result* outs,
                   int stages = SDSP_STAGES_FULL, hipEvent_t wait_ev = nullptr,
                   const sdsp_overview_request* req = nullptr, sdsp_overview* ovs = nullptr,
                   const KtCall* ktc = nullptr, const LvCall* lvc = nullptr, const TmCall* tmc = nullptr,
                   const ScCall* scc = nullptr, const R128Call* rc = nullptr, const FpCall* fc = nullptr) {
    DeviceCtx& d = device_ctx(device);
    std::lock_guard<std::mutex> lk(d.mu);
    SDSP_HIP_CHECK(hipSetDevice(device));
    return run_locked(d, d_samples, offsets, lens, n, sr, cfg, user_stream, outs, stages, wait_ev, req, ovs, ktc, lvc,
                      tmc, scc, rc, fc);
}

}  // namespace
}  // namespace sdsp

using namespace sdsp;

namespace sdsp {
namespace {
struct Slot {
    float* d = nullptr;
    uint64_t cap = 0;  // floats
    hipEvent_t ready = nullptr;
};
// A device's staging area: its copy stream and two HBM slots.  Areas are pooled per device and
// reused by later calls (grow-only slots, like the engine's own buffers), so a repeated call
// creates no stream, event or allocation; concurrent callers on one device take separate areas.
struct DeviceStage {
    int dev = 0;
    hipStream_t copy = nullptr;
    Slot slot[2];
};
std::mutex g_stage_mu;
std::map<int, std::vector<DeviceStage*>>* g_stage_free = new std::map<int, std::vector<DeviceStage*>>();  // never freed:
// the areas outlive the call and are released with the process (no HIP calls at static teardown)
DeviceStage* stage_acquire(int dev) {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    auto& v = (*g_stage_free)[dev];
    if (!v.empty()) {
        DeviceStage* ds = v.back();
        v.pop_back();
        return ds;
    }
    DeviceStage* ds = new DeviceStage();
    ds->dev = dev;
    return ds;
}
void stage_release(DeviceStage* ds) {
    if (ds->copy) {  // nothing may still be copying into the slots the next caller receives
        (void)hipSetDevice(ds->dev);
        (void)hipStreamSynchronize(ds->copy);
    }
    std::lock_guard<std::mutex> lk(g_stage_mu);
    (*g_stage_free)[ds->dev].push_back(ds);
}
// test hook (sdsp_debug_set_test_hooks): the worker devices of sdsp_analyze_batch, repeats
// allowed (two workers on device 0 exercise the multi-device chunk path on a one-GPU box)
// (compiled only into the test build, -DSDSP_TEST_HOOKS: the shipping library cannot be re-routed)
std::vector<int> device_list_override(int ndev) {
    std::vector<int> devs;
#ifdef SDSP_TEST_HOOKS
    for (int v : test_hooks_devices())
        if (v >= 0 && v < ndev) devs.push_back(v);
#endif
    return devs;
}
}  // namespace
}  // namespace sdsp

// Stage probes (include/stratum_hip_debug.h): a probe pipeline on the device context, whose "D."
// buffers are released again, so an analysis call finds the context as it left it.
namespace sdsp {
namespace {
template <class F>
int32_t run_stage_probe(const char* name, int32_t device, F f) {
    try {
        DeviceCtx& d = device_ctx(device);
        std::lock_guard<std::mutex> lk(d.mu);
        SDSP_HIP_CHECK(hipSetDevice(device));
        int32_t rc = SDSP_OK;
        try {
            f(d);
        } catch (const std::invalid_argument& e) {
            std::fprintf(stderr, "%s: %s\n", name, e.what());
            rc = SDSP_ERR_INVALID_INPUT;
        } catch (const std::exception& e) {
            std::fprintf(stderr, "%s: %s\n", name, e.what());
            rc = SDSP_ERR_PROCESSING;
        }
        for (hipStream_t s : d.own) (void)hipStreamSynchronize(s);
        for (auto it = d.bufs.begin(); it != d.bufs.end();)
            it = it->first.compare(0, 2, "D.") == 0 ? d.bufs.erase(it) : std::next(it);
        return rc;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s: %s\n", name, e.what());
        return SDSP_ERR_PROCESSING;
    }
}
}  // namespace
}  // namespace sdsp


extern "C" {

int32_t sdsp_analyze_batch_device(const float* d_samples, const uint64_t* offsets, const uint64_t* lens,
                                  uint64_t n_tracks, uint32_t sample_rate, const sdsp_config* cfg, int32_t device,
                                  void* stream, sdsp_result* outs) {
    return sdsp_analyze_batch_device_ex(d_samples, offsets, lens, n_tracks, sample_rate, cfg, device, stream,
                                        SDSP_STAGES_FULL, outs);
}

int32_t sdsp_analyze_batch_device_ex(const float* d_samples, const uint64_t* offsets, const uint64_t* lens,
                                     uint64_t n_tracks, uint32_t sample_rate, const sdsp_config* cfg, int32_t device,
                                     void* stream, int32_t stages, sdsp_result* outs) {
    try {
        return run_device(device, d_samples, offsets, lens, n_tracks, sample_rate, cfg, stream, outs, stages);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "sdsp_analyze_batch_device: %s\n", e.what());
        for (uint64_t i = 0; i < n_tracks; i++) {
            std::memset(&outs[i], 0, sizeof(outs[i]));
            outs[i].status = SDSP_ERR_PROCESSING;
            std::snprintf(outs[i].error_message, sizeof outs[i].error_message, "Processing error: %s", e.what());
        }
        return SDSP_ERR_PROCESSING;
    }
}

// The device batch with per-track overview envelopes (include/stratum_hip.h).  The request is
// checked before anything else; without one the call is sdsp_analyze_batch_device_ex.
int32_t sdsp_analyze_batch_device_overview(const float* d_samples, const uint64_t* offsets, const uint64_t* lens,
                                           uint64_t n_tracks, uint32_t sample_rate, const sdsp_config* cfg,
                                           int32_t device, void* stream, int32_t stages, sdsp_result* outs,
                                           const sdsp_overview_request* req, sdsp_overview* overviews) {
    if (!req)
        return sdsp_analyze_batch_device_ex(d_samples, offsets, lens, n_tracks, sample_rate, cfg, device, stream, stages,
                                            outs);
    auto fail_all = [&](int32_t status, const char* text) {
        for (uint64_t i = 0; i < n_tracks; i++) {
            std::memset(&outs[i], 0, sizeof(outs[i]));
            outs[i].status = status;
            std::snprintf(outs[i].error_message, sizeof outs[i].error_message, "%s", text);
            if (overviews) {
                std::memset(&overviews[i], 0, sizeof(overviews[i]));
                overviews[i].status = status;
            }
        }
        return status;
    };
    if (const char* why = overview_request_error(req->columns, req->frames_per_column, req->low_max_hz, req->mid_max_hz))
        return fail_all(SDSP_ERR_INVALID_INPUT, why);
    if (!overviews) return fail_all(SDSP_ERR_INVALID_INPUT, "Invalid input: overview request without an overviews array");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail_all(SDSP_ERR_PROCESSING, "Processing error: no HIP device");
    try {
        return run_device(device, d_samples, offsets, lens, n_tracks, sample_rate, cfg, stream, outs, stages, nullptr, req,
                          overviews);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "sdsp_analyze_batch_device_overview: %s\n", e.what());
        char text[256];
        std::snprintf(text, sizeof text, "Processing error: %s", e.what());
        return fail_all(SDSP_ERR_PROCESSING, text);
    }
}

// The device batch with both optional requests (include/stratum_hip.h): the overview envelopes
// and the key timelines from one analysis.  Both are checked before any device is touched.
int32_t sdsp_analyze_batch_device_requests(const float* d_samples, const uint64_t* offsets, const uint64_t* lens,
                                           uint64_t n_tracks, uint32_t sample_rate, const sdsp_config* cfg,
                                           int32_t device, void* stream, int32_t stages, sdsp_result* outs,
                                           const sdsp_overview_request* ov_req, sdsp_overview* overviews,
                                           const sdsp_key_timeline_request* kt_req, sdsp_key_timeline* timelines) {
    sdsp_request_set set{};
    set.struct_size = (uint32_t)sizeof(set);
    set.ov_req = ov_req;
    set.overviews = overviews;
    set.kt_req = kt_req;
    set.timelines = timelines;
    return sdsp_analyze_batch_device_with(d_samples, offsets, lens, n_tracks, sample_rate, cfg, device, stream, stages, outs,
                                          &set);
}

// The device batch with any of the optional requests (include/stratum_hip.h): the overview
// envelopes, the key timelines and the levels from one analysis.  Every request is checked before
// any device is touched.
int32_t sdsp_analyze_batch_device_with(const float* d_samples, const uint64_t* offsets, const uint64_t* lens,
                                       uint64_t n_tracks, uint32_t sample_rate, const sdsp_config* cfg, int32_t device,
                                       void* stream, int32_t stages, sdsp_result* outs, const sdsp_request_set* caller_set) {
    sdsp_request_set set;
    const char* set_err = request_set_read(caller_set, &set);
    const sdsp_overview_request* ov_req = set.ov_req;
    sdsp_overview* overviews = set.overviews;
    const sdsp_key_timeline_request* kt_req = set.kt_req;
    sdsp_key_timeline* timelines = set.timelines;
    const sdsp_levels_request* lv_req = set.lv_req;
    sdsp_levels* levels = set.levels;
    const sdsp_tempo_map_request* tm_req = set.tm_req;
    sdsp_tempo_map* tempo_maps = set.tempo_maps;
    const sdsp_sections_request* sc_req = nullptr;  // (sdsp_request_set_ext's pair, when struct_size covers it)
    sdsp_sections* sections = nullptr;
    if (!set_err) request_set_ext_read(caller_set, &sc_req, &sections);
    const sdsp_r128_request* r128_req = nullptr;  // (sdsp_request_set_ext2's pair, likewise)
    sdsp_r128* r128 = nullptr;
    if (!set_err) request_set_ext2_read(caller_set, &r128_req, &r128);
    const sdsp_fingerprint_request* fp_req = nullptr;  // (sdsp_request_set_ext3's fields, likewise)
    sdsp_fingerprint* fingerprints = nullptr;
    sdsp_fingerprint_matches* fp_matches = nullptr;
    if (!set_err) request_set_ext3_read(caller_set, &fp_req, &fingerprints, &fp_matches);
    if (!set_err && !ov_req && !kt_req && !lv_req && !tm_req && !sc_req && !r128_req && !fp_req)
        return sdsp_analyze_batch_device_ex(d_samples, offsets, lens, n_tracks, sample_rate, cfg, device, stream, stages,
                                            outs);
    auto fail_all = [&](int32_t status, const char* text) {
        for (uint64_t i = 0; i < n_tracks; i++) {
            std::memset(&outs[i], 0, sizeof(outs[i]));
            outs[i].status = status;
            std::snprintf(outs[i].error_message, sizeof outs[i].error_message, "%s", text);
            if (ov_req && overviews) {
                std::memset(&overviews[i], 0, sizeof(overviews[i]));
                overviews[i].status = status;
            }
            if (kt_req && timelines) {
                std::memset(&timelines[i], 0, sizeof(timelines[i]));
                timelines[i].status = status;
            }
            if (lv_req && levels) {
                std::memset(&levels[i], 0, sizeof(levels[i]));
                levels[i].status = status;
            }
            if (tm_req && tempo_maps) {
                std::memset(&tempo_maps[i], 0, sizeof(tempo_maps[i]));
                tempo_maps[i].status = status;
            }
            if (sc_req && sections) {
                std::memset(&sections[i], 0, sizeof(sections[i]));
                sections[i].status = status;
            }
            if (r128_req && r128) {
                std::memset(&r128[i], 0, sizeof(r128[i]));
                r128[i].status = status;
            }
            if (fp_req && fingerprints) {
                std::memset(&fingerprints[i], 0, sizeof(fingerprints[i]));
                fingerprints[i].status = status;
            }
        }
        if (fp_req && fp_matches) std::memset(fp_matches, 0, sizeof(*fp_matches));
        return status;
    };
    if (set_err) return fail_all(SDSP_ERR_INVALID_INPUT, set_err);
    if (!cfg) return fail_all(SDSP_ERR_INVALID_INPUT, "Invalid input: no configuration");
    LvCall lc;
    if (lv_req) {
        if (const char* why = levels_request_error(lv_req->what)) return fail_all(SDSP_ERR_INVALID_INPUT, why);
        if (!levels) return fail_all(SDSP_ERR_INVALID_INPUT, "Invalid input: levels request without a levels array");
        lc.what = lv_req->what;
        lc.out = levels;
    }
    TmCall tc;
    if (tm_req) {
        if (const char* why = tempo_map_request_error(tm_req->what, tempo_maps != nullptr, stages))
            return fail_all(SDSP_ERR_INVALID_INPUT, why);
        tc.what = tm_req->what;
        tc.out = tempo_maps;
    }
    if (ov_req) {
        if (const char* why = overview_request_error(ov_req->columns, ov_req->frames_per_column, ov_req->low_max_hz,
                                                     ov_req->mid_max_hz))
            return fail_all(SDSP_ERR_INVALID_INPUT, why);
        if (!overviews) return fail_all(SDSP_ERR_INVALID_INPUT, "Invalid input: overview request without an overviews array");
    }
    KtCall kc;
    if (kt_req) {
        if (const char* why = key_timeline_plan(kt_req->segment_seconds, kt_req->overlap_seconds, kt_req->segment_frames,
                                                kt_req->hop_frames, kt_req->min_change_confidence, sample_rate,
                                                kt_khop(*cfg), &kc.L, &kc.H))
            return fail_all(SDSP_ERR_INVALID_INPUT, why);
        if (!timelines)
            return fail_all(SDSP_ERR_INVALID_INPUT, "Invalid input: key timeline request without a timelines array");
        if (stages == SDSP_STAGES_BPM_ONLY)
            return fail_all(SDSP_ERR_INVALID_INPUT, "Invalid input: key timeline request with SDSP_STAGES_BPM_ONLY (no key path)");
        if (cfg->enable_key_beat_synchronous && !cfg->enable_key_log_frequency)
            return fail_all(SDSP_ERR_NOT_IMPLEMENTED,
                            "Not implemented: key timeline with beat-synchronous chroma (the rows are beats, not frames)");
        kc.min_conf = kt_req->min_change_confidence;
        kc.out = timelines;
    }
    ScCall sc;
    if (sc_req) {
        int32_t why_status = SDSP_OK;
        if (const char* why = sections_request_error(
                *sc_req, sections != nullptr, stages, sample_rate, kt_khop(*cfg), cfg->hop_size, cfg->force_legacy_bpm != 0,
                cfg->enable_key_beat_synchronous && !cfg->enable_key_log_frequency, &sc.Cs, &why_status))
            return fail_all(why_status, why);
        sc.req = *sc_req;
        sc.out = sections;
    }
    R128Call rc;
    if (r128_req) {
        if (const char* why = r128_request_error(r128_req->what, r128 != nullptr, sample_rate))
            return fail_all(SDSP_ERR_INVALID_INPUT, why);
        rc.what = r128_req->what;
        rc.out = r128;
    }
    FpCall fpc;
    if (fp_req) {
        int32_t why_status = SDSP_OK;
        if (const char* why = fingerprint_request_error(
                *fp_req, fingerprints != nullptr, fp_matches != nullptr, stages, sample_rate, kt_khop(*cfg),
                cfg->enable_key_beat_synchronous && !cfg->enable_key_log_frequency, &fpc.Cs, &why_status))
            return fail_all(why_status, why);
        fpc.req = *fp_req;
        fpc.out = fingerprints;
        fpc.matches = fp_matches;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail_all(SDSP_ERR_PROCESSING, "Processing error: no HIP device");
    try {
        return run_device(device, d_samples, offsets, lens, n_tracks, sample_rate, cfg, stream, outs, stages, nullptr,
                          ov_req, overviews, kt_req ? &kc : nullptr, lv_req ? &lc : nullptr, tm_req ? &tc : nullptr,
                          sc_req ? &sc : nullptr, r128_req ? &rc : nullptr, fp_req ? &fpc : nullptr);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "sdsp_analyze_batch_device_with: %s\n", e.what());
        char text[256];
        std::snprintf(text, sizeof text, "Processing error: %s", e.what());
        return fail_all(SDSP_ERR_PROCESSING, text);
    }
}

void sdsp_sections_free(sdsp_sections* s) {
    if (!s) return;
    std::free(s->sections ? (void*)s->sections : (void*)s->novelty);  // one block (fill_sections), sections first
    s->sections = nullptr;
    s->novelty = s->energy = nullptr;
    s->n_sections = s->n_curve = 0;
}

void sdsp_fingerprint_free(sdsp_fingerprint* f) {
    if (!f) return;
    std::free(f->words);
    f->words = nullptr;
}

void sdsp_fingerprint_matches_free(sdsp_fingerprint_matches* m) {
    if (!m) return;
    std::free(m->matches);
    m->matches = nullptr;
    m->n_matches = 0;
}

int32_t sdsp_debug_last_fingerprint_times(int32_t device, sdsp_debug_fingerprint_times* out) {
    try {
        if (!out) return SDSP_ERR_INVALID_INPUT;
        DeviceCtx& d = device_ctx(device);
        std::lock_guard<std::mutex> lk(d.mu);
        *out = d.last_fp;
        return SDSP_OK;
    } catch (const std::exception&) {
        return SDSP_ERR_PROCESSING;
    }
}

// k_fp_cells and k_fp_words over uploaded chroma rows (include/stratum_hip_debug.h).
int32_t sdsp_debug_fingerprint(const float* host_chroma, const uint64_t* frames, uint64_t n_tracks, uint32_t sample_rate,
                               uint32_t khop, const sdsp_fingerprint_request* req, sdsp_debug_fingerprint_out* out,
                               int32_t device) {
    if (!frames || !req || !out || !out->n_cells || !out->n_words || n_tracks == 0 || n_tracks > (1u << 20) || khop == 0)
        return SDSP_ERR_INVALID_INPUT;
    uint64_t Cs = 0;
    int32_t why_status = SDSP_OK;
    if (fingerprint_request_error(*req, true, true, SDSP_STAGES_FULL, sample_rate, khop, false, &Cs, &why_status))
        return SDSP_ERR_INVALID_INPUT;
    std::vector<uint64_t> kpfx(1, 0), cpfx(1, 0), wpfx(1, 0);
    for (uint64_t t = 0; t < n_tracks; t++) {
        if (frames[t] > (1u << 24)) return SDSP_ERR_INVALID_INPUT;
        kpfx.push_back(kpfx.back() + frames[t]);
        const uint64_t nc = fp_cells(frames[t], khop, Cs);
        cpfx.push_back(cpfx.back() + nc);
        wpfx.push_back(wpfx.back() + fp_words(nc));
    }
    if (kpfx.back() > 0 && !host_chroma) return SDSP_ERR_INVALID_INPUT;
    const uint64_t cells = cpfx.back(), words = wpfx.back();
    if (cells > out->cell_capacity || words > out->word_capacity || cells / 16 >= 0x7FFFFFFFull) return SDSP_ERR_INVALID_INPUT;
    if ((cells > 0 && !out->m) || (words > 0 && !out->words)) return SDSP_ERR_INVALID_INPUT;
    for (uint64_t t = 0; t < n_tracks; t++) {
        out->n_cells[t] = cpfx[(size_t)t + 1] - cpfx[(size_t)t];
        out->n_words[t] = wpfx[(size_t)t + 1] - wpfx[(size_t)t];
    }
    if (cells == 0) return SDSP_OK;
    return run_stage_probe("sdsp_debug_fingerprint", device, [&](DeviceCtx& d) {
        Ctx c(d);
        c.pre = "D.";
        const std::vector<float> rows(host_chroma, host_chroma + kpfx.back() * 12);
        float* d_cs = c.up("fp_chroma", rows);
        uint64_t* d_kpfx = c.up("fp_kpfx", kpfx);
        uint64_t* d_cpfx = c.up("fp_cpfx", cpfx);
        uint64_t* d_wpfx = c.up("fp_wpfx", wpfx);  // (also the slots: the words back to back)
        float* d_m = c.dev<float>("fp_m", 12 * (size_t)cells);
        uint32_t* d_w = c.dev<uint32_t>("fp_words", (size_t)std::max<uint64_t>(words, 1));
        launch_fp_cells(d_cs, d_kpfx, d_cpfx, (int)n_tracks, cells, Cs, khop, d_m, d.stream);
        launch_fp_words(d_m, d_cpfx, d_wpfx, d_wpfx, (int)n_tracks, words, d_w, d.stream);
        SDSP_HIP_CHECK(hipGetLastError());
        const std::vector<float> m = c.down(d_m, 12 * (size_t)cells);
        const std::vector<uint32_t> w = c.down(d_w, (size_t)words);
        std::memcpy(out->m, m.data(), m.size() * sizeof(float));
        if (words) std::memcpy(out->words, w.data(), w.size() * sizeof(uint32_t));
    });
}

// k_fp_match over uploaded word arrays (include/stratum_hip_debug.h).
int32_t sdsp_debug_fingerprint_match(const uint32_t* host_words, const uint64_t* n_words, uint64_t n_tracks,
                                     const sdsp_fingerprint_request* req, sdsp_debug_fingerprint_pair* rec, int32_t device) {
    static_assert(sizeof(sdsp_debug_fingerprint_pair) == sizeof(FpRec) && offsetof(sdsp_debug_fingerprint_pair, positions) == offsetof(FpRec, n),
                  "the probe hands the kernel's records out as they are");
    if (!host_words || !n_words || !req || !rec || n_tracks == 0 || n_tracks > 4096 || req->max_offset_words > FP_OMAX)
        return SDSP_ERR_INVALID_INPUT;
    std::vector<uint64_t> slot(1, 0);
    std::vector<uint32_t> W;
    for (uint64_t t = 0; t < n_tracks; t++) {
        if (n_words[t] == 0 || n_words[t] > (1u << 24)) return SDSP_ERR_INVALID_INPUT;
        slot.push_back(slot.back() + n_words[t]);
        W.push_back((uint32_t)n_words[t]);
    }
    std::memset(rec, 0, (size_t)(n_tracks * n_tracks) * sizeof(*rec));
    if (n_tracks < 2) return SDSP_OK;
    return run_stage_probe("sdsp_debug_fingerprint_match", device, [&](DeviceCtx& d) {
        Ctx c(d);
        c.pre = "D.";
        const std::vector<uint32_t> words(host_words, host_words + slot.back());
        uint32_t* d_words = c.up("fp_mwords", words);
        uint64_t* d_slot = c.up("fp_mslot", slot);
        uint32_t* d_W = c.up("fp_mW", W);
        const size_t NC = (size_t)n_tracks;
        fp_match_bands(c, "", d_words, d_slot, d_W, (int)NC, req->max_offset_words, req->min_overlap_words,
                       [&](int r0, int r1, const FpRec* band) {
                           std::memcpy(rec + (size_t)r0 * NC, band, (size_t)(r1 - r0) * NC * sizeof(FpRec));
                       });
    });
}

void sdsp_r128_free(sdsp_r128* r) {
    if (!r) return;
    std::free(r->momentary);  // one block (fill_r128), the momentary curve first
    r->momentary = r->short_term = nullptr;
}

int32_t sdsp_debug_last_r128_times(int32_t device, sdsp_debug_r128_times* out) {
    try {
        if (!out) return SDSP_ERR_INVALID_INPUT;
        DeviceCtx& d = device_ctx(device);
        std::lock_guard<std::mutex> lk(d.mu);
        *out = d.last_r128;
        return SDSP_OK;
    } catch (const std::exception&) {
        return SDSP_ERR_PROCESSING;
    }
}

int32_t sdsp_debug_last_sections_times(int32_t device, sdsp_debug_sections_times* out) {
    try {
        if (!out) return SDSP_ERR_INVALID_INPUT;
        DeviceCtx& d = device_ctx(device);
        std::lock_guard<std::mutex> lk(d.mu);
        *out = d.last_sc;
        return SDSP_OK;
    } catch (const std::exception&) {
        return SDSP_ERR_PROCESSING;
    }
}

// The sections kernels over uploaded chroma rows and frame energies (include/stratum_hip_debug.h).
int32_t sdsp_debug_sections(const float* host_chroma, const uint64_t* frames, const float* host_energy,
                            const uint64_t* base_frames, uint64_t n_tracks, uint32_t sample_rate, uint32_t khop,
                            uint32_t hop, const sdsp_sections_request* req, sdsp_debug_sections_out* out, int32_t device) {
    if (!frames || !base_frames || !req || !out || !out->n_cells || n_tracks == 0 || n_tracks > (1u << 20) || khop == 0 ||
        hop == 0)
        return SDSP_ERR_INVALID_INPUT;
    uint64_t Cs = 0;
    int32_t why_status = SDSP_OK;
    if (sections_request_error(*req, true, SDSP_STAGES_FULL, sample_rate, khop, hop, false, false, &Cs, &why_status))
        return SDSP_ERR_INVALID_INPUT;
    std::vector<uint64_t> kpfx(1, 0), bpfx(1, 0), cpfx(1, 0), tpfx(1, 0);
    for (uint64_t t = 0; t < n_tracks; t++) {
        if (frames[t] > (1u << 24) || base_frames[t] > (1u << 24)) return SDSP_ERR_INVALID_INPUT;
        kpfx.push_back(kpfx.back() + frames[t]);
        bpfx.push_back(bpfx.back() + base_frames[t]);
        const uint64_t nc = sc_cells(frames[t], khop, base_frames[t], hop, Cs);
        cpfx.push_back(cpfx.back() + nc);
        tpfx.push_back(tpfx.back() + (nc + SC_TILE - 1) / SC_TILE);
    }
    if ((kpfx.back() > 0 && !host_chroma) || (bpfx.back() > 0 && !host_energy)) return SDSP_ERR_INVALID_INPUT;
    const uint64_t cells = cpfx.back();
    if (cells > out->cell_capacity || cells / 16 >= 0x7FFFFFFFull) return SDSP_ERR_INVALID_INPUT;
    if (cells > 0 && (!out->m || !out->g || !out->novelty || !out->boundary)) return SDSP_ERR_INVALID_INPUT;
    for (uint64_t t = 0; t < n_tracks; t++) out->n_cells[t] = cpfx[(size_t)t + 1] - cpfx[(size_t)t];
    if (cells == 0) return SDSP_OK;
    return run_stage_probe("sdsp_debug_sections", device, [&](DeviceCtx& d) {
        Ctx c(d);
        c.pre = "D.";
        const std::vector<float> rows(host_chroma, host_chroma + kpfx.back() * 12);
        const std::vector<float> en(host_energy, host_energy + bpfx.back());
        bpfx.pop_back();  // row0 of each track
        float* d_cs = c.up("sc_chroma", rows);
        float* d_E = c.up("sc_E", en);
        uint64_t* d_kpfx = c.up("sc_kpfx", kpfx);
        uint64_t* d_row0 = c.up("sc_row0", bpfx);
        uint64_t* d_cpfx = c.up("sc_cpfx", cpfx);
        uint64_t* d_tpfx = c.up("sc_tpfx", tpfx);
        float* d_m = c.dev<float>("sc_m", 12 * (size_t)cells);
        float* d_g = c.dev<float>("sc_g", (size_t)cells);
        float* d_N = c.dev<float>("sc_N", (size_t)cells);
        uint8_t* d_b = c.dev<uint8_t>("sc_b", (size_t)cells);
        launch_section_energy(d_E, d_row0, d_cpfx, (int)n_tracks, cells, Cs, hop, d_g, d.stream);
        launch_section_chroma(d_cs, d_kpfx, d_cpfx, (int)n_tracks, cells, Cs, khop, d_m, d.stream);
        launch_section_novelty(d_m, d_g, d_cpfx, d_tpfx, (int)n_tracks, tpfx.back(), (int)req->kernel_cells,
                               req->energy_weight, req->min_gap_cells, req->min_strength, d_N, d_b, d.stream);
        SDSP_HIP_CHECK(hipGetLastError());
        const std::vector<float> m = c.down(d_m, 12 * (size_t)cells), g = c.down(d_g, (size_t)cells),
                                 N = c.down(d_N, (size_t)cells);
        const std::vector<uint8_t> b = c.down(d_b, (size_t)cells);
        std::memcpy(out->m, m.data(), m.size() * sizeof(float));
        std::memcpy(out->g, g.data(), g.size() * sizeof(float));
        std::memcpy(out->novelty, N.data(), N.size() * sizeof(float));
        std::memcpy(out->boundary, b.data(), b.size());
    });
}

void sdsp_tempo_map_free(sdsp_tempo_map* m) {
    if (!m) return;
    std::free(m->segments ? (void*)m->segments : (void*)m->onsets);  // one block (fill_tempo_map), segments first
    m->segments = nullptr;
    m->onsets = nullptr;
    m->n_segments = m->n_onsets = 0;
}

int32_t sdsp_debug_last_tempo_map_times(int32_t device, sdsp_debug_tempo_map_times* out) {
    try {
        if (!out) return SDSP_ERR_INVALID_INPUT;
        DeviceCtx& d = device_ctx(device);
        std::lock_guard<std::mutex> lk(d.mu);
        *out = d.last_tm;
        return SDSP_OK;
    } catch (const std::exception&) {
        return SDSP_ERR_PROCESSING;
    }
}

void sdsp_levels_free(sdsp_levels* l) {
    if (!l) return;
    std::free(l->regions);
    l->regions = nullptr;
    l->n_regions = 0;
}

int32_t sdsp_debug_last_levels_times(int32_t device, sdsp_debug_levels_times* out) {
    try {
        if (!out) return SDSP_ERR_INVALID_INPUT;
        DeviceCtx& d = device_ctx(device);
        std::lock_guard<std::mutex> lk(d.mu);
        *out = d.last_lv;
        return SDSP_OK;
    } catch (const std::exception&) {
        return SDSP_ERR_PROCESSING;
    }
}

void sdsp_key_timeline_free(sdsp_key_timeline* t) {
    if (!t) return;
    std::free(t->segments);  // both arrays are one block (fill_key_timeline)
    t->segments = nullptr;
    t->changes = nullptr;
    t->n_segments = t->n_changes = 0;
}

// The key timeline kernel and host logic over uploaded chroma rows (include/stratum_hip_debug.h).
int32_t sdsp_debug_key_timeline(const float* host_chroma, const uint64_t* frames, uint64_t n_tracks,
                                uint32_t sample_rate, const sdsp_config* cfg, const sdsp_key_timeline_request* req,
                                sdsp_key_timeline* out, int32_t device) {
    if (!frames || !cfg || !req || !out || n_tracks == 0 || n_tracks > (1u << 20)) return SDSP_ERR_INVALID_INPUT;
    KtCall kc;
    if (key_timeline_plan(req->segment_seconds, req->overlap_seconds, req->segment_frames, req->hop_frames,
                          req->min_change_confidence, sample_rate, kt_khop(*cfg), &kc.L, &kc.H))
        return SDSP_ERR_INVALID_INPUT;
    kc.min_conf = req->min_change_confidence;
    kc.out = out;
    std::vector<uint64_t> kpfx(1, 0), spfx(1, 0);
    for (uint64_t t = 0; t < n_tracks; t++) {
        if (frames[t] > (1u << 24)) return SDSP_ERR_INVALID_INPUT;
        kpfx.push_back(kpfx.back() + frames[t]);
        spfx.push_back(spfx.back() + kt_segments(frames[t], kc.L, kc.H));
    }
    if (kpfx.back() > 0 && !host_chroma) return SDSP_ERR_INVALID_INPUT;
    if (spfx.back() / KT_SEGS >= 0x7FFFFFFFull) return SDSP_ERR_INVALID_INPUT;
    return run_stage_probe("sdsp_debug_key_timeline", device, [&](DeviceCtx& d) {
        Ctx c(d);
        c.pre = "D.";
        const std::vector<float> rows(host_chroma, host_chroma + kpfx.back() * 12);
        std::vector<float> tpl(576);
        key_templates(tpl.data());
        float* d_cs = c.up("kt_chroma", rows);
        uint64_t* d_kpfx = c.up("kt_kpfx", kpfx);
        uint64_t* d_spfx = c.up("kt_spfx", spfx);
        float* d_tpl = c.up("kt_tpl", tpl);
        KtSeg* d_out = c.dev<KtSeg>("kt_out", (size_t)std::max<uint64_t>(spfx.back(), 1));
        launch_key_timeline(d_cs, d_kpfx, d_spfx, (int)n_tracks, spfx.back(), kc.L, kc.H, d_tpl, d_out, d.stream);
        SDSP_HIP_CHECK(hipGetLastError());
        const std::vector<KtSeg> seg = c.down(d_out, (size_t)spfx.back());
        for (uint64_t t = 0; t < n_tracks; t++) {
            TrackKt k;
            k.on = true;
            k.F = frames[t];
            k.seg.assign(seg.begin() + (ptrdiff_t)spfx[(size_t)t], seg.begin() + (ptrdiff_t)spfx[(size_t)t + 1]);
            fill_key_timeline(k, SDSP_OK, *cfg, sample_rate, kc, &out[t]);
        }
    });
}

void sdsp_overview_free(sdsp_overview* o) {
    if (!o) return;
    std::free(o->smin);  // the five arrays are one block (fill_overview)
    o->smin = o->smax = o->low = o->mid = o->high = nullptr;
    o->n_columns = 0;
}

int32_t sdsp_debug_last_overview_times(int32_t device, sdsp_debug_overview_times* out) {
    try {
        if (!out) return SDSP_ERR_INVALID_INPUT;
        DeviceCtx& d = device_ctx(device);
        std::lock_guard<std::mutex> lk(d.mu);
        *out = d.last_ov;
        return SDSP_OK;
    } catch (const std::exception&) {
        return SDSP_ERR_PROCESSING;
    }
}

// Whether `cfg` at `sample_rate` takes the default key path's block-folded HPCP frame energies
// (include/stratum_hip_debug.h): the parity tests then compare key_confidence / key_clarity with
// the oracle within the north star's tolerance, and every other configuration bit for bit.
int32_t sdsp_debug_key_energy_blocked(const sdsp_config* cfg, uint32_t sample_rate) {
    if (!cfg || sample_rate == 0) return -1;
    return key_energy_blocked(*cfg, sample_rate) ? 1 : 0;
}

// Per track of the last sdsp_analyze_batch_device / sdsp_analyze_audio call on `device`: 1 where
// its key vote was near an energy-dependent decision and the track was analysed again exactly.
int32_t sdsp_debug_last_key_near(int32_t device, uint8_t* out, uint64_t n) {
    try {
        DeviceCtx& d = device_ctx(device);
        std::lock_guard<std::mutex> lk(d.mu);
        for (uint64_t i = 0; i < n; i++) out[i] = i < d.last_near.size() ? d.last_near[(size_t)i] : 0;
        return SDSP_OK;
    } catch (const std::exception&) {
        return SDSP_ERR_PROCESSING;
    }
}

// Tracks the last call on `device` reran in place (Pipeline::rerun_tail).
int32_t sdsp_debug_last_tail_reruns(int32_t device, uint64_t* n_tracks) {
    try {
        if (!n_tracks) return SDSP_ERR_INVALID_INPUT;
        DeviceCtx& d = device_ctx(device);
        std::lock_guard<std::mutex> lk(d.mu);
        *n_tracks = d.last_tail_reruns;
        return SDSP_OK;
    } catch (const std::exception&) {
        return SDSP_ERR_PROCESSING;
    }
}

int32_t sdsp_debug_tempo_stages(const float* host_mags, const uint64_t* frames, uint64_t n_tracks, uint32_t sample_rate,
                                uint32_t hop, const sdsp_config* cfg, sdsp_debug_tempo_out* out, int32_t device) {
    if (!host_mags || !frames || !cfg || !out || n_tracks == 0 || n_tracks > (1u << 20) || sample_rate == 0 || hop == 0 ||
        hop > 8192)
        return SDSP_ERR_INVALID_INPUT;
    for (uint64_t t = 0; t < n_tracks; t++)
        if (frames[t] == 0 || frames[t] > (1u << 24)) return SDSP_ERR_INVALID_INPUT;
    return run_stage_probe("sdsp_debug_tempo_stages", device, [&](DeviceCtx& d) {
        Pipeline p(d, *cfg, sample_rate, SDSP_STAGES_FULL, false, false, false, true);
        p.debug_tempo_stages(host_mags, frames, n_tracks, (int)hop, out);
    });
}

int32_t sdsp_debug_key_stages(const float* host_mags, const uint64_t* frames, uint64_t n_tracks, uint32_t sample_rate,
                              const sdsp_config* cfg, int32_t mode, float* masked, float* chroma, float* energy,
                              float* edel, int32_t info[4], int32_t device) {
    if (!host_mags || !frames || !cfg || !masked || !chroma || !energy || !info || n_tracks == 0 ||
        n_tracks > (1u << 20) || sample_rate == 0 || mode < 0 || mode > 2)
        return SDSP_ERR_INVALID_INPUT;
    for (uint64_t t = 0; t < n_tracks; t++)
        if (frames[t] == 0 || frames[t] > (1u << 24)) return SDSP_ERR_INVALID_INPUT;
    return run_stage_probe("sdsp_debug_key_stages", device, [&](DeviceCtx& d) {
        Pipeline p(d, *cfg, sample_rate, SDSP_STAGES_FULL, mode == 2, false, false, true);
        p.debug_key_stages(host_mags, frames, n_tracks, mode, masked, chroma, energy, edel, info);
    });
}

int32_t sdsp_debug_key_vote(const float* host_chroma, const float* host_energy, const float* host_edel,
                            const uint64_t* frames, uint64_t n_tracks, const int32_t* sel, uint64_t n_sel,
                            uint32_t sample_rate, const sdsp_config* cfg, int32_t threads, int32_t alone,
                            int32_t cert_fixed, sdsp_debug_key_vote_out* out, int32_t device) {
    if (!host_chroma || !host_energy || !frames || !cfg || !out || n_tracks == 0 || n_tracks > (1u << 20) ||
        sample_rate == 0 || (threads != 0 && threads != 256 && threads != 512 && threads != 1024) ||
        (sel == nullptr) != (n_sel == 0) || n_sel > n_tracks)
        return SDSP_ERR_INVALID_INPUT;
    if (!out->key || !out->chroma_s || !out->weights || !out->seg_rows || !out->seg_row_pfx || !out->dbg ||
        (host_edel && !out->wdel))
        return SDSP_ERR_INVALID_INPUT;
    for (uint64_t t = 0; t < n_tracks; t++)
        if (frames[t] == 0 || frames[t] > (1u << 24)) return SDSP_ERR_INVALID_INPUT;
    return run_stage_probe("sdsp_debug_key_vote", device, [&](DeviceCtx& d) {
        Pipeline p(d, *cfg, sample_rate, SDSP_STAGES_FULL, false, false, false, true);
        p.debug_key_vote(host_chroma, host_energy, host_edel, frames, n_tracks, sel, n_sel, threads, alone != 0,
                         cert_fixed != 0, out);
    });
}

int32_t sdsp_debug_onset_stages(const float* rms, const float* hfc, const float* sfo, const float* hpe,
                                const uint64_t* frames, const uint64_t* n_trim, uint64_t n_tracks, uint32_t sample_rate,
                                uint32_t hop, const sdsp_config* cfg, sdsp_debug_onset_out* out, int32_t device) {
    if (!rms || !hfc || !sfo || !frames || !n_trim || !cfg || !out || n_tracks == 0 || n_tracks > (1u << 20) ||
        sample_rate == 0 || hop == 0 || hop > (1u << 24))
        return SDSP_ERR_INVALID_INPUT;
    if (!out->energy || !out->spectral || !out->hfc || !out->hpss || !out->chosen || !out->n_energy ||
        !out->n_spectral || !out->n_hfc || !out->n_hpss || !out->n_chosen)
        return SDSP_ERR_INVALID_INPUT;
    for (uint64_t t = 0; t < n_tracks; t++)
        if (frames[t] == 0 || frames[t] > (1u << 24) || frames[t] * (uint64_t)hop >= (1ull << 32))
            return SDSP_ERR_INVALID_INPUT;
    return run_stage_probe("sdsp_debug_onset_stages", device, [&](DeviceCtx& d) {
        Pipeline p(d, *cfg, sample_rate, SDSP_STAGES_FULL, false, false, false, true);
        p.debug_onset_stages(rms, hfc, sfo, hpe, frames, n_trim, n_tracks, (int)hop, out);
    });
}

int32_t sdsp_debug_beat_grid(const uint32_t* onsets, const uint64_t* n_onsets, const uint64_t* frames,
                             const uint64_t* n_trim, const float* bpm, const float* conf, uint64_t n_tracks,
                             uint32_t sample_rate, const sdsp_config* cfg, sdsp_debug_beat_out* out, int32_t device) {
    if (!onsets || !n_onsets || !frames || !n_trim || !bpm || !conf || !cfg || !out || n_tracks == 0 ||
        n_tracks > (1u << 20) || sample_rate == 0)
        return SDSP_ERR_INVALID_INPUT;
    if (!out->ok || !out->n_beats || !out->n_down || !out->stability || !out->beats || !out->downs)
        return SDSP_ERR_INVALID_INPUT;
    for (uint64_t t = 0; t < n_tracks; t++) {
        if (frames[t] == 0 || frames[t] > (1u << 24) || n_trim[t] > (1ull << 40)) return SDSP_ERR_INVALID_INPUT;
    }
    for (uint64_t t = 0, at = 0; t < n_tracks; at += n_onsets[t], t++) {
        if (n_onsets[t] > (1u << 26)) return SDSP_ERR_INVALID_INPUT;
        for (uint64_t k = 1; k < n_onsets[t]; k++)
            if (onsets[at + k] < onsets[at + k - 1]) return SDSP_ERR_INVALID_INPUT;  // ascending, as the consensus leaves them
    }
    return run_stage_probe("sdsp_debug_beat_grid", device, [&](DeviceCtx& d) {
        Pipeline p(d, *cfg, sample_rate, SDSP_STAGES_FULL, false, false, false, true);
        p.debug_beat_grid(onsets, n_onsets, frames, n_trim, bpm, conf, n_tracks, out);
    });
}

int32_t sdsp_debug_tempo_map(const uint32_t* onsets, const uint64_t* n_onsets, const uint64_t* frames,
                             const uint64_t* n_trim, const float* bpm, const float* conf, uint64_t n_tracks,
                             uint32_t sample_rate, const sdsp_config* cfg, uint32_t what, sdsp_tempo_map* maps,
                             sdsp_debug_beat_out* beats, int32_t device) {
    if (!onsets || !n_onsets || !frames || !n_trim || !bpm || !conf || !cfg || !maps || n_tracks == 0 ||
        n_tracks > (1u << 20) || sample_rate == 0 || tempo_map_request_error(what, true, SDSP_STAGES_FULL))
        return SDSP_ERR_INVALID_INPUT;
    if (beats && (!beats->ok || !beats->n_beats || !beats->n_down || !beats->stability || !beats->beats || !beats->downs))
        return SDSP_ERR_INVALID_INPUT;
    for (uint64_t t = 0; t < n_tracks; t++) {
        if (frames[t] == 0 || frames[t] > (1u << 24) || n_trim[t] > (1ull << 40)) return SDSP_ERR_INVALID_INPUT;
    }
    for (uint64_t t = 0, at = 0; t < n_tracks; at += n_onsets[t], t++) {
        if (n_onsets[t] > (1u << 26)) return SDSP_ERR_INVALID_INPUT;
        for (uint64_t k = 1; k < n_onsets[t]; k++)
            if (onsets[at + k] < onsets[at + k - 1]) return SDSP_ERR_INVALID_INPUT;  // ascending, as the consensus leaves them
    }
    for (uint64_t t = 0; t < n_tracks; t++) std::memset(&maps[t], 0, sizeof(maps[t]));
    return run_stage_probe("sdsp_debug_tempo_map", device, [&](DeviceCtx& d) {
        Pipeline p(d, *cfg, sample_rate, SDSP_STAGES_FULL, false, false, false, true);
        std::vector<TrackTm> tml;
        p.debug_tempo_map(onsets, n_onsets, frames, n_trim, bpm, conf, n_tracks, what, &tml, beats);
        for (uint64_t t = 0; t < n_tracks; t++) fill_tempo_map(tml[(size_t)t], SDSP_OK, &maps[t]);
    });
}

int32_t sdsp_debug_tempo_select(const float* fft, const int32_t* fft_n, const float* acf, uint32_t NB,
                                const int32_t present[5], const int32_t* active, uint64_t n_tracks, int32_t top_n,
                                int32_t cand_cap, int32_t gate, uint32_t sample_rate, const sdsp_config* cfg,
                                sdsp_debug_tempo_est* est, float* cand, int32_t device) {
    if (!fft || !fft_n || !acf || !present || !active || !cfg || !est || !cand || n_tracks == 0 ||
        n_tracks > (1u << 16) || sample_rate == 0 || NB > 512 || top_n < 0 || cand_cap < 1 || cand_cap > 1024 ||
        !present[0])
        return SDSP_ERR_INVALID_INPUT;
    for (uint64_t t = 0; t < n_tracks; t++)
        if (fft_n[t] < 0 || fft_n[t] > 1024) return SDSP_ERR_INVALID_INPUT;
    return run_stage_probe("sdsp_debug_tempo_select", device, [&](DeviceCtx& d) {
        Pipeline p(d, *cfg, sample_rate, SDSP_STAGES_FULL, false, false, false, true);
        p.debug_tempo_select(fft, fft_n, acf, (int)NB, present, active, n_tracks, top_n, cand_cap, gate != 0, est, cand);
    });
}

int32_t sdsp_debug_multires(const sdsp_debug_multires_in* in, uint32_t sample_rate, const sdsp_config* cfg,
                            sdsp_debug_multires_out* out, int32_t device) {
    if (!in || !cfg || !out || sample_rate == 0 || in->n_tracks == 0 || in->n_tracks > (1u << 16) ||
        in->n_items > in->n_tracks || in->cap_aux == 0 || in->cap_aux > 1024 || in->cap_base == 0 || in->cap_base > 1024)
        return SDSP_ERR_INVALID_INPUT;
    if (!in->c256 || !in->c512 || !in->c1024 || !in->n256 || !in->n512 || !in->n1024 || !in->nov512 || !in->nov_n ||
        !in->base || !in->items || !out->mr || !out->dbg || !out->used || !out->final_bpm || !out->final_conf)
        return SDSP_ERR_INVALID_INPUT;
    if (in->own512 && cfg->tempogram_multi_res_top_k > 1024) return SDSP_ERR_INVALID_INPUT;
    return run_stage_probe("sdsp_debug_multires", device, [&](DeviceCtx& d) {
        Pipeline p(d, *cfg, sample_rate, SDSP_STAGES_FULL, false, false, false, true);
        p.debug_multires_fuse(in, out);
    });
}

// Host buffers: chunks of whole tracks (up to SDSP_BATCH_CHUNK_TRACKS tracks, default
// 512, and about 8 GB) pulled from a shared counter by one worker per device; per device a copier
// thread stages the next chunk into the second of two HBM slots (its own stream, completion
// signalled by an event the engine's stream waits on) while the device analyses the current one.
// The queue itself is batch_sched.hpp (host-only, tested with fake devices).
int32_t sdsp_analyze_batch(const float* const* tracks, const uint64_t* lens, uint64_t n_tracks, uint32_t sample_rate,
                           const sdsp_config* cfg, uint32_t device_mask, sdsp_result* outs) {
    std::vector<int> devs;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        for (uint64_t i = 0; i < n_tracks; i++) {
            std::memset(&outs[i], 0, sizeof(outs[i]));
            outs[i].status = SDSP_ERR_PROCESSING;
            std::snprintf(outs[i].error_message, sizeof outs[i].error_message, "Processing error: no HIP device");
        }
        return SDSP_ERR_PROCESSING;
    }
    devs = device_list_override(ndev);
    if (devs.empty())
        for (int d = 0; d < ndev && d < 32; d++)
            if (device_mask == 0 ? d == 0 : ((device_mask >> d) & 1u)) devs.push_back(d);
    if (devs.empty()) devs.push_back(0);
    uint64_t max_tracks = 512;
    if (const uint64_t t = test_hooks().batch_chunk_tracks.load()) max_tracks = t;  // sdsp_debug_set_schedule
    const std::vector<uint64_t> cb = plan_chunks(lens, n_tracks, max_tracks, (uint64_t)2 << 30 /* 8 GB of f32 */);
    // test hook (sdsp_debug_set_test_hooks): the chunk whose analysis throws (the per-chunk failure path)
#ifdef SDSP_TEST_HOOKS
    const long fail_chunk = test_hooks().fail_chunk.load();
#endif
    const size_t n_chunks = cb.size() - 1;
    // every result starts as an error; run_device overwrites the tracks it analyses
    auto mark_failed = [&](size_t c, const std::string& what) {
        for (uint64_t i = cb[c]; i < cb[c + 1]; i++) {
            std::memset(&outs[i], 0, sizeof(outs[i]));
            outs[i].status = SDSP_ERR_PROCESSING;
            std::snprintf(outs[i].error_message, sizeof outs[i].error_message, "Processing error: %s", what.c_str());
        }
    };
    for (size_t c = 0; c < n_chunks; c++) mark_failed(c, "track not analysed");
    std::vector<DeviceStage*> stg;
    std::vector<ChunkDevice> cds;
    for (int dev : devs) {
        stg.push_back(stage_acquire(dev));
        DeviceStage* ds = stg.back();
        ChunkDevice cd;
        cd.stage = [ds, &cb, tracks, lens](int s, size_t c) {
            SDSP_HIP_CHECK(hipSetDevice(ds->dev));
            if (!ds->copy) SDSP_HIP_CHECK(hipStreamCreateWithFlags(&ds->copy, hipStreamNonBlocking));
            Slot& sl = ds->slot[s];
            if (!sl.ready) SDSP_HIP_CHECK(hipEventCreateWithFlags(&sl.ready, hipEventDisableTiming));
            uint64_t tot = 0;
            for (uint64_t i = cb[c]; i < cb[c + 1]; i++) tot += lens[i];
            if (sl.cap < tot) {
                if (sl.d) SDSP_HIP_CHECK(hipFree(sl.d));
                sl.d = nullptr;
                sl.cap = 0;
                const uint64_t want = std::max<uint64_t>(tot + tot / 8, 1);  // grow-only, with slack
                SDSP_HIP_CHECK(hipMalloc(&sl.d, want * sizeof(float)));
                note_alloc(want * sizeof(float));
                sl.cap = want;
            }
            uint64_t o = 0;
            for (uint64_t i = cb[c]; i < cb[c + 1]; i++) {
                if (lens[i])
                    SDSP_HIP_CHECK(hipMemcpyAsync(sl.d + o, tracks[i], lens[i] * sizeof(float), hipMemcpyHostToDevice,
                                                  ds->copy));
                o += lens[i];
            }
            SDSP_HIP_CHECK(hipEventRecord(sl.ready, ds->copy));
        };
#ifdef SDSP_TEST_HOOKS
        cd.analyze = [ds, &cb, lens, sample_rate, cfg, outs, fail_chunk](int s, size_t c) {
            if ((long)c == fail_chunk) throw HipError("injected chunk failure (test hook)");
#else
        cd.analyze = [ds, &cb, lens, sample_rate, cfg, outs](int s, size_t c) {  // (no failure injection)
#endif
            const uint64_t a = cb[c], b = cb[c + 1];
            std::vector<uint64_t> off(b - a), ln(b - a);
            uint64_t tot = 0;
            for (uint64_t i = a; i < b; i++) {
                off[i - a] = tot;
                ln[i - a] = lens[i];
                tot += lens[i];
            }
            run_device(ds->dev, ds->slot[s].d, off.data(), ln.data(), b - a, sample_rate, cfg, nullptr, outs + a,
                       SDSP_STAGES_FULL, ds->slot[s].ready);
        };
        cd.drain = [ds]() {  // after a failed chunk: nothing may still read the slot it reuses
            // the engine's own streams and this stage's copy stream, never the caller's streams
            SDSP_HIP_CHECK(hipSetDevice(ds->dev));
            DeviceCtx& c = device_ctx(ds->dev);
            {
                std::lock_guard<std::mutex> lk(c.mu);
                for (hipStream_t s : c.own) SDSP_HIP_CHECK(hipStreamSynchronize(s));
            }
            if (ds->copy) SDSP_HIP_CHECK(hipStreamSynchronize(ds->copy));
        };
        cds.push_back(cd);
    }
    const size_t failed = run_chunked(n_chunks, cds, [&](size_t c, const std::string& what) {
        std::fprintf(stderr, "sdsp_analyze_batch: %s\n", what.c_str());
        mark_failed(c, what);
    });
    for (DeviceStage* ds : stg) stage_release(ds);
    return failed ? SDSP_ERR_PROCESSING : SDSP_OK;
}

int32_t sdsp_analyze_audio(const float* samples, uint64_t n_samples, uint32_t sample_rate, const sdsp_config* cfg,
                           sdsp_result* out, char* err, uint64_t errlen) {
    std::memset(out, 0, sizeof(*out));
    if (n_samples == 0 || sample_rate == 0) {
        const char* m = n_samples == 0 ? "Invalid input: Empty audio samples" : "Invalid input: Invalid sample rate";
        if (err && errlen) std::snprintf(err, (size_t)errlen, "%s", m);
        out->status = SDSP_ERR_INVALID_INPUT;
        return SDSP_ERR_INVALID_INPUT;
    }
    // one track: staged into a context buffer on the engine's stream under the context lock (no
    // copy stream, copier thread or staging allocation per call); device 0, as the batch's
    // default mask
    int32_t rc = SDSP_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        out->status = SDSP_ERR_PROCESSING;
        std::snprintf(out->error_message, sizeof out->error_message, "Processing error: no HIP device");
    } else {
        try {
            DeviceCtx& d = device_ctx(0);
            std::lock_guard<std::mutex> lk(d.mu);
            SDSP_HIP_CHECK(hipSetDevice(0));
            DevBuf& in = d.buf("api.track");
            in.ensure(n_samples * sizeof(float));
            SDSP_HIP_CHECK(hipMemcpyAsync(in.p, samples, n_samples * sizeof(float), hipMemcpyHostToDevice, d.stream));
            const uint64_t off = 0;
            rc = run_locked(d, in.as<float>(), &off, &n_samples, 1, sample_rate, cfg, nullptr, out, SDSP_STAGES_FULL,
                            nullptr);
        } catch (const std::exception& e) {
            std::memset(out, 0, sizeof(*out));
            out->status = SDSP_ERR_PROCESSING;
            std::snprintf(out->error_message, sizeof out->error_message, "Processing error: %s", e.what());
        }
    }
    if (rc != SDSP_OK && out->status == SDSP_OK) out->status = rc;
    if (out->status != SDSP_OK) {
        if (err && errlen) std::snprintf(err, (size_t)errlen, "%s", out->error_message);
        const int32_t s = out->status;
        sdsp_result_free(out);
        std::memset(out, 0, sizeof(*out));
        out->status = s;
        return s;
    }
    return SDSP_OK;
}

int32_t sdsp_generate_synthetic(float* d_out, uint64_t n_tracks, uint64_t len, uint32_t sample_rate, uint64_t seed0,
                                int32_t bpm_mode, int32_t device, void* stream, float* bpm_out, int32_t* key_out) {
    try {
        DeviceCtx& d = device_ctx(device);
        std::lock_guard<std::mutex> lk(d.mu);
        SDSP_HIP_CHECK(hipSetDevice(device));
        std::vector<float> bpm((size_t)n_tracks);
        std::vector<int> key((size_t)n_tracks);
        for (uint64_t i = 0; i < n_tracks; i++) {
            uint64_t x = 0x5EED0000ull + seed0 + i;
            auto next = [&]() {  // splitmix64
                x += 0x9E3779B97F4A7C15ull;
                uint64_t z = x;
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                return z ^ (z >> 31);
            };
            float b;
            if (bpm_mode == 1) {  // config 5: thirds in [55,80], [170,200], [80,170]
                const int third = (int)(i % 3);
                const uint64_t r = next();
                if (third == 0)
                    b = 55.0f + 0.5f * (float)(r % 51);
                else if (third == 1)
                    b = 170.0f + 0.5f * (float)(r % 61);
                else
                    b = 80.0f + 0.5f * (float)(r % 181);
            } else {
                b = 70.0f + 0.5f * (float)(next() % 221);
            }
            bpm[(size_t)i] = b;
            key[(size_t)i] = (int)(next() % 24);
        }
        if (bpm_out) std::memcpy(bpm_out, bpm.data(), bpm.size() * sizeof(float));
        if (key_out) std::memcpy(key_out, key.data(), key.size() * sizeof(int));
        hipStream_t st = stream ? (hipStream_t)stream : d.stream;
        DevBuf& db = d.buf("synth.bpm");
        db.ensure(bpm.size() * 4 + 16);
        DevBuf& dk = d.buf("synth.key");
        dk.ensure(key.size() * 4 + 16);
        DevBuf& dp = d.buf("synth.peak");
        dp.ensure(key.size() * 4 + 16);
        SDSP_HIP_CHECK(hipMemcpyAsync(db.p, bpm.data(), bpm.size() * 4, hipMemcpyHostToDevice, st));
        SDSP_HIP_CHECK(hipMemcpyAsync(dk.p, key.data(), key.size() * 4, hipMemcpyHostToDevice, st));
        launch_synth(d_out, n_tracks, len, sample_rate, db.as<float>(), dk.as<int>(), seed0, st);
        launch_synth_normalize(d_out, n_tracks, len, dp.as<unsigned int>(), st);
        SDSP_HIP_CHECK(hipGetLastError());
        SDSP_HIP_CHECK(hipStreamSynchronize(st));
        return SDSP_OK;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "sdsp_generate_synthetic: %s\n", e.what());
        return SDSP_ERR_PROCESSING;
    }
}

}  // extern "C"
