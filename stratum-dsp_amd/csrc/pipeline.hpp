// pipeline.hpp — what the host pipeline's files share (pipeline.hip has the overview): the upload /
// download context, the per-track result, the tempo pass's input and output, the structs one
// stage of a sub-batch hands to the later ones, class Pipeline, and the configuration -> launch
// parameter functions of pipeline_params.hip.
//
// A stage struct is filled once by the stage that returns it and read-only afterwards (host
// vectors and device pointers, no behaviour); later stages take it by const reference.  Tempo is
// the exception, see there.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/sdsp_fft_spec.h"
#include "../../include/stratum_hip_debug.h"
#include "fingerprint_core.hpp"
#include "kernels.hpp"
#include "levels_core.hpp"
#include "r128_core.hpp"
#include "sections_core.hpp"
#include "tempo_map_core.hpp"
#include "sdsp_runtime.hpp"

namespace sdsp {
namespace detail {

// ---- pipeline.hip: spectrogram row strides ----
int base_stride(int fs);
// the key spectrogram's frame size and hop (src/lib.rs:985-1009): the override's, else the tempo
// path's frame_size / hop_size (whose spectrogram the reference reuses; the engine recomputes it
// on the key stream, bit-identical by the STFT spec)
inline uint64_t key_fft(const sdsp_config& c) {
    return c.enable_key_stft_override ? std::max<uint64_t>(c.key_stft_frame_size, 256) : c.frame_size;
}
inline uint64_t key_hop(const sdsp_config& c) {
    return c.enable_key_stft_override ? std::max<uint64_t>(c.key_stft_hop_size, 1) : c.hop_size;
}

// ---- pipeline_params.hip: configuration -> tables and launch parameters (no Pipeline, no stream) ----
struct MelTable {
    std::vector<int> m;    // 2 per bin, -1 = none
    std::vector<float> w;  // 2 per bin
    int n_mels = 0;
};
MelTable mel_table(uint32_t sr, int n_bins, int n_mels_in, float fmin_hz, float fmax_hz, std::string* err);
std::vector<MelPlan> mel_plan(const MelTable& t, int n_bins, std::string* err);
std::vector<HarmEntry> harm_table(int B, uint32_t sr, int fft_size, float sigma_in, int hmax, float decay_in);
void key_peak_band(const sdsp_config& c, uint32_t sr, int* lo, int* hi);
bool key_energy_blocked(const sdsp_config& c, uint32_t sr);
TuningParams tuning_params(const sdsp_config& c, uint32_t sr, int B, float fres, int stride);
ChromaParams chroma_params(const sdsp_config& c, uint32_t sr, int mode, int B, float fres, int stride);
HpcpXParams hpcp_x_params(const sdsp_config& c, uint32_t sr, int B, float fres, bool whiten, int stride);
KeyHpssParams key_hpss_params(const sdsp_config& c, uint32_t sr, int B, float fres, int stride);
std::string check_supported(const sdsp_config& c, uint32_t sr);  // "" or why the configuration cannot run
void key_templates(float* out /*48x12*/);
LoudnessParams loudness_params(int method, uint32_t sr);
void acf_grid(uint32_t sr, int hop, float min_bpm, float max_bpm, float res, std::vector<float>* bpms,
              std::vector<int>* lags);
void fft_bins(uint32_t sr, int hop, uint64_t P, float min_bpm, float max_bpm, int* b_lo, int* K, float* fres_out);
bool band_configured(const sdsp_config& c);  // use_aux_variants (src/lib.rs:375-377)
FeatParams feat_params(const sdsp_config& c, uint32_t sr, int B, int stride);  // without the chunk tables
void feat_chunk_tables(const FeatParams& fp, const std::vector<MelPlan>& mplan, std::vector<int>* flags,
                       std::vector<MelChunk>* mel);
NovParams nov_params(const sdsp_config& c, bool configured);  // band_on: the caller's
SelParams sel_params(const sdsp_config& c, const int present[NVAR], int NB, int top_n, int gate);
MrParams mr_params(const sdsp_config& c, uint32_t sr, int top_k, bool own512);
LegacyParams legacy_params(const sdsp_config& c, uint32_t sr, int hop);
uint64_t seg_rows(const KeyParams& kp, uint64_t F);  // segment scratch row bound of an F-row chroma slice
KeyParams key_vote_params(const sdsp_config& c, bool band);  // cert_fixed: the caller's (a test hook)
bool perc_better(const TempoEst& p, float cur_bpm, float cur_conf, int cur_agree, const TempoEst& base);

// ---------------------------------------------------------------------------------------
struct Ctx {
    DeviceCtx& d;
    std::deque<std::vector<uint8_t>> keep;  // host staging kept alive until the next sync
    std::string pre;  // buffer-name prefix: a nested pipeline's buffers are its own
    explicit Ctx(DeviceCtx& dc) : d(dc) {}
    template <class T>
    T* up(const std::string& name, const std::vector<T>& v) {
        DevBuf& b = d.buf(pre + name);
        const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
        b.ensure(bytes);
        if (!v.empty())
            SDSP_HIP_CHECK(hipMemcpyAsync(b.p, keep_bytes(v), v.size() * sizeof(T), hipMemcpyHostToDevice, d.stream));
        return b.as<T>();
    }
    // a host copy that lives until the context's queued work is done (async H2D source)
    template <class T>
    const void* keep_bytes(const std::vector<T>& v) {
        keep.emplace_back(reinterpret_cast<const uint8_t*>(v.data()),
                          reinterpret_cast<const uint8_t*>(v.data()) + v.size() * sizeof(T));
        return keep.back().data();
    }
    template <class T>
    T* dev(const std::string& name, size_t n) {
        DevBuf& b = d.buf(pre + name);
        b.ensure(std::max<size_t>(n * sizeof(T), 16));
        return b.as<T>();
    }
    template <class T>
    std::vector<T> down(const T* p, size_t n) {
        std::vector<T> v(n);
        if (n) SDSP_HIP_CHECK(hipMemcpyAsync(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost, d.stream));
        SDSP_HIP_CHECK(hipStreamSynchronize(d.stream));
        keep.clear();
        return v;
    }
    void sync() {
        SDSP_HIP_CHECK(hipStreamSynchronize(d.stream));
        keep.clear();
    }
};

struct Timers {
    hipEvent_t ev[16];
    int n = 0;
    DeviceCtx* d = nullptr;
    void init(DeviceCtx& dc) {
        d = &dc;
        for (auto& e : ev) SDSP_HIP_CHECK(hipEventCreate(&e));
    }
    void mark(int i, hipStream_t s = nullptr) { SDSP_HIP_CHECK(hipEventRecord(ev[i], s ? s : d->stream)); }
    double ms(int a, int b) {
        float t = 0.0f;
        if (hipEventElapsedTime(&t, ev[a], ev[b]) != hipSuccess) return 0.0;
        return t;
    }
    ~Timers() {
        if (d)
            for (auto& e : ev) (void)hipEventDestroy(e);
    }
};

// SDSP_HOST_TRACE=1: host wall time between the sub-batch's synchronisation points (stderr)
struct HostTrace {
    bool on = test_hooks().host_trace.load() != 0;  // sdsp_debug_set_schedule
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), tp = t0;
    void operator()(const char* tag) {
        if (!on) return;
        const auto t = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[sdsp host] %-12s +%8.3f ms  (%8.3f)\n", tag,
                     std::chrono::duration<double, std::milli>(t - tp).count(),
                     std::chrono::duration<double, std::milli>(t - t0).count());
        tp = t;
    }
};

struct TrackRes {
    int status = SDSP_OK;
    std::string err;
    float bpm = 0, bpm_conf = 0;
    int key_mode = 0, key_tonic = 0;
    float key_conf = 0, key_clarity = 0, stability = 0, duration = 0;
    float onset_consensus = 0;
    std::vector<float> beats, downs;
    int8_t mr_trig = -1, mr_used = -1, perc_trig = -1, perc_used = -1;
    bool has_cands = false;
    std::vector<sdsp_tempo_candidate> cands;
    int key_near = 0;  // block-folded key energies near a decision (KV_NEAR_* bits): rerun with the sequential fold
    bool key_rerun = false;  // that rerun has replaced the key fields
};
// a key vote's mode, tonic, confidence and clarity; key_near / key_rerun stay with the caller
inline void set_key_fields(TrackRes& r, const KeyOut& ko) {
    r.key_mode = ko.mode;
    r.key_tonic = ko.tonic;
    r.key_conf = ko.conf;
    r.key_clarity = ko.clarity;
}
inline void set_key_fields(TrackRes& r, const TrackRes& rerun) {  // from a rerun pipeline's result
    r.key_mode = rerun.key_mode;
    r.key_tonic = rerun.key_tonic;
    r.key_conf = rerun.key_conf;
    r.key_clarity = rerun.key_clarity;
}

// A tempo pass's tempograms: the items launched and their ACF / FFT lists.  Device pointers stay
// valid until the next pass with the same tag.
struct PassTg {
    int present[NVAR] = {0, 0, 0, 0, 0};
    int NB = 0;
    std::vector<int> items;         // (track, variant) = track * NVAR + variant, active tracks, in launch order
    std::vector<uint64_t> fft_off;  // per item: first entry of its FFT list
    std::vector<int> fft_k;         // per item: entries of its FFT list
    std::vector<int> fft_k_track;   // per pass-track
    float *acf_bpm = nullptr, *acf_str = nullptr;  // item i at [i * NB, (i + 1) * NB)
    float *fft_bpm = nullptr, *fft_pow = nullptr;
};
// What a tempo pass launched with, kept for the stage probe (sdsp_debug_tempo_stages).
struct TempoStageDbg {
    FeatParams fp{};
    PassTg tg;
};

// One "tempo pass": STFT (2048, hop) -> features -> novelty -> tempograms -> candidate scoring,
// for a dense list of tracks.  Used for hop 512 (all tracks) and the escalation hops.
struct TempoPassOut;
struct TempoPassIn {
    int hop = 0;
    const float* samples = nullptr;
    std::vector<uint64_t> src_off;  // per pass-track
    std::vector<float> gain_h;
    std::vector<uint64_t> n_trim;
    int top_n = 0, gate = 0, cand_cap = 0;
    // a precomputed frame_size-point spectrogram (rows at the pass's frame prefix, stride s2_) and
    // its frame maxima: the STFT is skipped (the percussive tempogram fallback runs on the HPSS output)
    const float* mags_in = nullptr;
    const float* fmax_in = nullptr;
    // escalation hops over the hop-512 spectrogram (rows base_row0[t] + frame): 1 = hop 1024, every
    // frame is a hop-512 row (2v); 2 = hop 256, even frames are hop-512 rows, odd ones are computed
    int reuse = 0;
    const float* base_mags = nullptr;
    const float* base_fmax = nullptr;
    std::vector<uint64_t> base_row0;
    // also the hop-512 novelty multi_resolution.rs:680-694 gates its folds with (the combined
    // novelty with the configured weights, whatever the band-fusion setting; out.nov_mr)
    bool mr_nov = false;
    // What the escalation's hop-256 and hop-1024 passes share (Pipeline::escalate; the defaults are
    // a complete pass).  no_flux: features without the spectral flux (out.SFO stays null; only the
    // base pass's is read) and the hop-256 odd-frame STFT without frame maxima.
    bool no_flux = false;
    // hop 256: its feature walk also stores the hop-1024 pass's SFX of the same tracks (that pass's
    // frame prefix on the device and its frame total)
    float* sfx4_out = nullptr;
    const uint64_t* sfx4_fpfx = nullptr;
    uint64_t sfx4_total = 0;
    // hop 1024: no feature launch; SFX as the hop-256 walk stored it, and E / H / MEL copied from the
    // hop-512 pass feat512 (frame j from its frame base_row0[t] + 2 j)
    float* sfx_in = nullptr;
    const TempoPassOut* feat512 = nullptr;
    TempoStageDbg* dbg = nullptr;  // the stage probe's record (never set by an analysis call)
};
// the pass input of a subset of another pass's tracks (its hop and samples; no gate)
TempoPassIn subset(const TempoPassIn& base, const std::vector<int>& which);
struct TempoPassOut {
    std::vector<uint64_t> fpfx;  // frame prefix over the pass's tracks
    uint64_t total = 0;
    // device pointers (valid until the next pass with the same tag)
    float *mags = nullptr, *fmax = nullptr, *E = nullptr, *H = nullptr, *SFX = nullptr, *SFO = nullptr, *MEL = nullptr,
          *nov = nullptr, *nov_sum = nullptr, *cand = nullptr, *nov_mr = nullptr;
    uint64_t* d_fpfx = nullptr;
    TempoEst* est = nullptr;
    int* active = nullptr;
    std::vector<int> active_h;
    double stft_ms = 0, feat_ms = 0, tempo_ms = 0;
    uint64_t stft_launch = 0;
    uint64_t stft_frames = 0;
    double stft_bytes = 0;
};
// tempo_pass's other stages: frame plan + STFT, features (novelty and select return nothing)
struct PassPlan {
    int P_T = 0;
    std::vector<uint64_t> tpfx;  // feature-tile prefix over the pass's tracks
    uint64_t* d_tpfx = nullptr;
    RowMap rm{};  // where the features read each frame's row
};
struct PassFeat {
    FeatParams fp{};
    bool configured = false, mel_on = false;  // band_configured(); the mel variant
};

// pass_select from its offset tables on: the tempogram lists on the device and, per (track, variant)
// slot t * NVAR + v, where each list starts (0 for an absent variant); fft_k per track.
struct SelLists {
    const float *fft_bpm = nullptr, *fft_pow = nullptr, *acf_bpm = nullptr, *acf_str = nullptr;
    std::vector<uint64_t> fo, ao;
    std::vector<int> fft_k;
    int present[NVAR] = {0, 0, 0, 0, 0};
    int NB = 0;
};
// escalate's tail: the three hops' candidate lists on the device with their counts (-1: that hop's
// tempogram failed; n256 / n1024 per item, n512 per item with own512, else per track), the base
// estimates and the hop-512 novelty with its frame prefix (by item or by track like n512).
struct MrFuse {
    const float *c256 = nullptr, *c512 = nullptr, *c1024 = nullptr;
    std::vector<int> n256, n512, n1024;
    int cap_aux = 0, cap_base = 0;  // rows of the aux lists; of the base pass's list (the hop-512 one without own512)
    bool own512 = false;
    const TempoEst* base_est = nullptr;
    const float* nov512 = nullptr;
    const uint64_t* fpfx512 = nullptr;
    bool want_dbg = false;
    // set by fuse_multires
    int cap512 = 0;
    MrDbg* d_mdbg = nullptr;
};

// ---- debug_track_id dumps (pipeline_debug.hip) ----
struct Cand4 {
    float bpm, score, fft, acf;
};
struct TrackDbg {
    bool base = false;  // base tempogram estimate available (multi-resolution path)
    TempoEst est{};
    std::vector<Cand4> base_c;
    bool mr = false;  // escalated and every hop's tempogram succeeded
    std::vector<Cand4> c256, c512, c1024;
    TempoEst mr_est{};
    MrDbg md{};
    bool key = false;
    KeyOut ko{};
    KeyDbg kd{};
    float tuning = 0.0f;
};
void print_debug(const sdsp_config& c, const TrackDbg& d);

// ---- the key stream's records (pipeline_key.hip) ----
// The band path's state of a sub-batch for the exact rerun in place (rerun_tail): its key
// spectrogram (band masked in place, every other bin the STFT's), its chroma and vote buffers.
// Valid for the call's last sub-batch only (the next sub-batch's key stream reuses them).
struct KeyTail {
    bool ok = false;
    float* mags8 = nullptr;
    uint64_t* d_kpfx = nullptr;
    std::vector<uint64_t> kpfx{0}, kseg{0};  // frame and segment-scratch prefixes over the key tracks
    float* d_part = nullptr;
    uint64_t total8 = 0;
    int st_lo = 0, st_hi = -1, B8 = 0;
    HpcpParams hp{};
    const HarmEntry* d_ht = nullptr;
    float *d_chroma = nullptr, *d_energy = nullptr, *d_cs = nullptr, *d_w = nullptr, *d_sscr = nullptr;
    const float* d_tpl = nullptr;
    KeyParams kp{};
};
// The key timeline's segments of a sub-batch's key tracks as queued behind the vote
// (Pipeline::launch_key); nothing is queued without a request.  The output and
// the segment prefix are per-parity buffers like the vote's output: the late join reads them after
// the next sub-batch has launched.
struct KeyTimelineOut {
    std::vector<uint64_t> spfx{0};  // segment prefix over the key tracks
    std::vector<uint64_t> frames;   // F of each key track
    KtSeg* d_out = nullptr;
};
// The sections request's buffers of a sub-batch's key tracks: the cell means queued behind the vote
// (Pipeline::launch_key) and behind the base pass's features, the novelty and the boundary flags
// behind both (Pipeline::section_novelty); nothing is queued without a request.  All per-parity
// buffers, like the key timeline's: the late join reads them after the next sub-batch has launched.
struct SectionsOut {
    std::vector<uint64_t> cpfx{0}, tpfx{0};  // cell and 64-cell tile prefix over the key tracks
    uint64_t *d_cpfx = nullptr, *d_tpfx = nullptr;
    float *d_m = nullptr, *d_g = nullptr, *d_N = nullptr;
    uint8_t* d_b = nullptr;
    bool queued = false;  // the novelty is queued: the joins wait for ev[13], not ev[2]
};
// The fingerprint request's plan of a sub-batch's key tracks (Pipeline::launch_key): the cell means
// and the words queued behind the vote; nothing is queued without a request.  The words go to the
// call's word buffer, which the match reads after the last join, so no join reads anything here.
struct FingerprintOut {
    std::vector<uint64_t> cpfx{0}, wpfx{0};  // cell and word prefix over the key tracks
};
// Late key join: a sub-batch's key results are read after the next sub-batch's tempo path is
// queued, so the key stream's tail (mask, HPCP, vote) runs beside that tempo path instead of
// holding the main stream back.  Uploads read by the key stream and the key output live in
// per-parity buffers (E0.*, E1.*); the key stream itself is in order, so its big buffers are
// shared.
struct KeyPending {
    std::unique_ptr<Timers> kt;
    KeyOut* d_kout = nullptr;
    KeyTimelineOut ktl;
    SectionsOut sc;
    std::vector<size_t> at;  // result slot of each key track
    std::vector<uint64_t> first;  // its trim start in the caller's track (the key timeline's first_sample)
    KeyTail tail;
};
// what key_condition launched with
struct KeyCond {
    HpcpParams hp{};
    bool band = false;  // the band path: k_mask_rp on [pk_lo - 1, pk_hi + 1], k_hpcp_band
    int st_lo = 0, st_hi = -1;  // the bins launch_mask_band stored (blocked configurations)
    float *d_part = nullptr, *d_chroma = nullptr, *d_energy = nullptr, *d_edel = nullptr, *d_tune = nullptr;
    const HarmEntry* d_ht = nullptr;
};

// ---- what a sub-batch's stages hand on (positions: t in the sub-batch, i in R, k in K / E) ----
// A (Pipeline::front): the tracks that survive trimming.
struct Front {
    std::vector<uint64_t> off, ts, te;  // per sub-batch track: first sample, trim bounds
    std::vector<float> gain_h;
    std::vector<int> R;                 // surviving tracks (positions in the sub-batch)
    std::vector<size_t> slot;           // result slot of each surviving track
    std::vector<uint64_t> rpfx;         // raw-signal frame prefix over the sub-batch (rms_shared)
    float* d_srms = nullptr;            // the trim pass's frame RMS
    bool rms_shared = false;            // ... taken at the energy hop: the onsets reuse its frames
};
// E (Pipeline::launch_key): the key path as queued on the key and vote streams.
struct KeyLaunch {
    std::vector<int> K;  // key tracks (positions in R)
    std::vector<uint64_t> ktile{0};  // HPCP-tile prefix over K
    bool serial_streams = false;
    float* d_tune = nullptr;
    uint64_t* d_ktile = nullptr;
    int* d_kid = nullptr;
    KeyOut* d_kout = nullptr;
    KeyDbg* d_kdbg = nullptr;
    KeyTimelineOut ktl;
    SectionsOut sc;
    FingerprintOut fp;
    // the key spectrogram, frame prefix, templates and vote parameters; with tail.ok the band
    // path's state for rerun_tail
    KeyTail tail;
    std::unique_ptr<Timers> kt;   // events 0-2 time the key stream; 7-11 order it
};
// HPSS of the base spectrogram: the percussive part, its frame energies and frame maxima.
struct Hpss {
    float *d_P0 = nullptr, *d_hpe = nullptr, *d_hfmax = nullptr;
};
struct Onsets {
    uint32_t* d_chosen = nullptr;  // consensus onsets, track i at d_coff[i], d_cn[i] of them
    uint64_t* d_coff = nullptr;
    int* d_cn = nullptr;
    std::vector<int> en_h;  // energy-flux onset counts
    // the lists the consensus merged (read by the stage probe only): energy onsets at the frame
    // prefix with counts d_en; flux onsets in kind-major parts (spectral, HFC, HPSS) of the pass's
    // frame total each, counts d_fn kind-major; `lists` of them in all (3, or 4 with HPSS onsets)
    uint32_t *d_eon = nullptr, *d_fon = nullptr;
    int *d_en = nullptr, *d_fn = nullptr;
    int lists = 0;
};
// The tempo estimates of the surviving tracks.  The one hand-off that is not read-only: seeded from
// the base pass (seed_tempo), then refined in turn by the escalation, the percussive fallback and
// the legacy select, each through this one struct (host vectors and their device mirrors).
struct Tempo {
    std::vector<float> fbpm_h, fconf_h;
    std::vector<int> used, E;  // took the multi-res estimate; escalated tracks (positions in R)
    float *d_fbpm = nullptr, *d_fconf = nullptr;
    int* d_used = nullptr;
    TempoEst* d_mr_all = nullptr;  // multi-res estimates of the escalated tracks (E order)
    // position in E of each track (-1: not escalated), built once after the escalation; read by the
    // percussive fallback (the multi-res estimate's agreement) and the result fill (the own-512 list)
    std::vector<int> epos;
    // hop_size != 512: the escalation's own hop-512 candidate lists (E order; emitted for the
    // tracks that take the multi-res estimate, src/lib.rs:546,686)
    std::vector<float> c512_h;
    std::vector<int> n512_own;
    int c512_cap = 0;
    std::vector<std::vector<float>> perc_cands;  // emitted candidates of tracks that took the fallback
    std::vector<uint8_t> perc_took;
};
// D (Pipeline::beat_grid), and its compacted lists on the host (Pipeline::download_results).
struct Beats {
    std::vector<uint64_t> boff;
    uint64_t* d_boff = nullptr;
    float *d_beats = nullptr, *d_downs = nullptr;
    BeatOut* d_bout = nullptr;
    float* d_bscr = nullptr;  // k_beat's scratch and capacities (read again by Pipeline::tempo_map)
    int* d_bcap = nullptr;
};
// The tempo maps of the surviving tracks as queued behind k_beat (Pipeline::tempo_map); nothing is
// queued without a request.
struct TempoMapQ {
    bool on = false;
    std::vector<uint64_t> soff{0};  // segment capacity prefix over the surviving tracks
    TmSeg* d_segs = nullptr;
    TmOut* d_out = nullptr;
    const uint32_t* d_chosen = nullptr;  // the stage's consensus onsets (Onsets)
    const uint64_t* d_coff = nullptr;
    const int* d_cn = nullptr;
};
struct ResultsHost {
    std::vector<BeatOut> bout;
    std::vector<uint64_t> bpfx;
    std::vector<float> beats_h, downs_h, cand_h;
    float* d_cbeats = nullptr;
    // with a tempo map request: the maps, their segments (track i's at tm_soff[i]) and the onsets
    // (track i's at tm_opfx[i]; empty unless asked for)
    std::vector<TmOut> tm_out;
    std::vector<TmSeg> tm_segs;
    std::vector<uint64_t> tm_soff, tm_opfx;
    std::vector<uint32_t> tm_onsets;
};
// The overview envelopes of the surviving tracks as queued after the base pass (Pipeline::overview);
// nothing is queued without a request.
struct Overview {
    bool on = false;
    std::vector<uint64_t> cpfx{0};  // column prefix over the surviving tracks
    uint64_t n_cols = 0;
    float* d_out = nullptr;  // track i's smin, smax, low, mid, high back to back at 5 cpfx[i]
    double seg_bytes = 0, col_bytes = 0;  // algorithmic bytes of the two kernels
};
// One track's key timeline on the host (sdsp_key_timeline without the call-wide fields): its
// segments as the kernel wrote them; `on` marks a track whose key path ran.
struct TrackKt {
    bool on = false;
    uint64_t F = 0, first = 0;
    std::vector<KtSeg> seg;
};
// One track's overview on the host (sdsp_overview without the config-wide fields): its five arrays
// (smin, smax, low, mid, high, C each) back to back at blk + at, in its sub-batch's download.
struct TrackOv {
    uint64_t C = 0, F = 0, first = 0, n = 0;
    std::shared_ptr<float[]> blk;
    size_t at = 0;
};

// One track's levels on the host (sdsp_levels without the config-wide fields).  `on`: the track
// gets levels (n > 0, a sample rate, a supported configuration), whatever its analysis status.
struct TrackLv {
    bool on = false;
    sdsp_loudness method[3]{};
    float applied_gain = 1.0f;
    uint64_t n = 0, ts = 0, te = 0;
    std::vector<uint64_t> regions;  // (start, end) sample pairs, ascending
};
// One track's sections on the host: the cell energies, the novelty and the boundary flags as the
// kernels wrote them; `on` marks a track whose key path ran.
struct TrackSc {
    bool on = false;
    uint64_t first = 0;
    std::vector<float> g, N;
    std::vector<uint8_t> b;
};
// One track's fingerprint plan on the host; `on` marks a track whose key path ran.
struct TrackFp {
    bool on = false;
    uint64_t first = 0, n_cells = 0, W = 0;
};
// The fingerprints of a call (Pipeline::set_fingerprint): every track's plan and its slot in the
// call's word buffer, the words on the host (SDSP_FP_WORDS) and, with SDSP_FP_MATCH, the matches among
// the tracks whose status was SDSP_OK when the match ran (run_locked drops a track that fails later).
struct FpOut {
    std::vector<TrackFp> tracks;
    std::vector<uint64_t> slot;  // track t's words at words[slot[t]], tracks[t].W of them
    std::vector<uint32_t> words;
    std::vector<sdsp_fingerprint_match> matches;
};
// The pairs among NC compared tracks (launch_fp_match's arguments on the device) in row bands whose
// records stay under a fixed bound: band(r0, r1, rec) receives the rows [r0, r1) on the host, the pair
// (i, j), i < j, at rec[(i - r0) * NC + j].  Returns the kernel's HIP event time in ms.
double fp_match_bands(Ctx& c, const std::string& tag, const uint32_t* d_words, const uint64_t* d_slot, const uint32_t* d_W,
                      int NC, uint32_t O, uint32_t min_overlap_words,
                      const std::function<void(int, int, const FpRec*)>& band);
// One track's tempo map on the host (sdsp_tempo_map without its status).  `on`: the track reached
// the beat stage.
struct TrackTm {
    bool on = false;
    TmOut o{};
    float bpm = 0.0f, conf = 0.0f;
    uint64_t first = 0;
    std::vector<TmSeg> segs;
    std::vector<uint32_t> onsets;
};
// The levels folds as queued before the sub-batches (Pipeline::levels_prepass) and read at the
// call's end (Pipeline::levels_join); nothing is queued without a request.
struct LevelsPending {
    bool on = false;
    std::vector<size_t> at;  // result slot of each folded track
    uint32_t chains = 0;
    LvParams P{};
    unsigned int* d_peak = nullptr;
    float* d_sums = nullptr;
    int* d_gn = nullptr;
    std::unique_ptr<Timers> tm;  // events 0-1: the first launch (peak and folds), 1-2: the second
};

// One track's programme loudness on the host (sdsp_r128 with its curves still in vectors).  `on`:
// the track was measured (n > 0, a supported configuration), whatever its analysis status.
struct TrackR128 {
    bool on = false;
    sdsp_r128 r{};
    std::vector<float> curves;  // momentary blocks, then short-term blocks (SDSP_R128_CURVES)
};
// The programme loudness kernels as queued before the sub-batches (Pipeline::r128_prepass) and read
// at the call's end (Pipeline::r128_join); nothing is queued without a request.
struct R128Pending {
    bool on = false;
    std::vector<size_t> at;  // result slot of each measured track
    std::vector<uint64_t> n, cvpfx;
    R128Params P{};
    unsigned int* d_peak = nullptr;
    R128Folds* d_folds = nullptr;
    float* d_curves = nullptr;
    uint64_t steps = 0;
    std::unique_ptr<Timers> tm;  // events 0-1: the steps, 1-2: the per-track kernel, 2-3: the peaks
};

}  // namespace detail
using namespace detail;

// ---------------------------------------------------------------------------------------
class Pipeline {
   public:
    Pipeline(DeviceCtx& d, const sdsp_config& cfg, uint32_t sr, int stages = SDSP_STAGES_FULL, bool exact_energy = false,
             bool key_only = false, bool nested = false, bool probe = false);
    // Stage probes (include/stratum_hip_debug.h), on a pipeline built with probe = true: its buffers
    // carry the prefix "D." and everything runs in order on the main stream, like a nested rerun.
    void debug_tempo_stages(const float* host_mags, const uint64_t* frames, uint64_t n_tracks, int hop,
                            sdsp_debug_tempo_out* out);
    void debug_key_stages(const float* host_mags, const uint64_t* frames, uint64_t n_tracks, int mode, float* masked,
                          float* chroma, float* energy, float* edel, int32_t info[4]);
    void debug_key_vote(const float* host_chroma, const float* host_energy, const float* host_edel,
                        const uint64_t* frames, uint64_t n_tracks, const int32_t* sel, uint64_t n_sel, int threads,
                        bool alone, bool cert_fixed, sdsp_debug_key_vote_out* out);
    void debug_onset_stages(const float* rms, const float* hfc, const float* sfo, const float* hpe,
                            const uint64_t* frames, const uint64_t* n_trim, uint64_t n_tracks, int hop,
                            sdsp_debug_onset_out* out);
    void debug_beat_grid(const uint32_t* onsets, const uint64_t* n_onsets, const uint64_t* frames,
                         const uint64_t* n_trim, const float* bpm, const float* conf, uint64_t n_tracks,
                         sdsp_debug_beat_out* out);
    void debug_tempo_map(const uint32_t* onsets, const uint64_t* n_onsets, const uint64_t* frames,
                         const uint64_t* n_trim, const float* bpm, const float* conf, uint64_t n_tracks, uint32_t what,
                         std::vector<TrackTm>* maps, sdsp_debug_beat_out* beats);
    void debug_tempo_select(const float* fft, const int32_t* fft_n, const float* acf, int NB, const int32_t present[5],
                            const int32_t* active, uint64_t n_tracks, int top_n, int cand_cap, int gate,
                            sdsp_debug_tempo_est* est, float* cand);
    void debug_multires_fuse(const sdsp_debug_multires_in* in, sdsp_debug_multires_out* out);

    void run(const float* d_samples, const std::vector<uint64_t>& in_off, const std::vector<uint64_t>& n_raw,
             std::vector<TrackRes>& res);
    // Before run(): also compute every track's overview envelope (include/stratum_hip.h) into
    // *out, one entry per track of the call.  A pipeline without a request queues nothing for it.
    void set_overview(const sdsp_overview_request& req, std::vector<TrackOv>* out) {
        ov_req_ = req;
        ov_out_ = out;
    }
    // Before run(): also compute every track's key timeline (include/stratum_hip.h) with segments
    // of L key frames every H (key_timeline_plan.hpp) into *out, one entry per track of the call.
    // A pipeline without a request queues nothing for it; nested pipelines get none.
    void set_key_timeline(uint32_t L, uint32_t H, std::vector<TrackKt>* out) {
        kt_L_ = L;
        kt_H_ = H;
        kt_out_ = out;
    }
    // Before run(): also compute every track's levels (include/stratum_hip.h, sdsp_levels; `what`
    // checked by levels_request_error) into *out, one entry per track of the call.  A pipeline
    // without a request queues nothing for it; nested pipelines get none.
    void set_levels(uint32_t what, std::vector<TrackLv>* out) {
        lv_what_ = what;
        lv_out_ = out;
    }
    // Before run(): also compute every track's tempo map (include/stratum_hip.h, sdsp_tempo_map;
    // `what` checked by tempo_map_request_error) into *out, one entry per track of the call.  A
    // pipeline without a request queues nothing for it; nested pipelines get none.
    void set_tempo_map(uint32_t what, std::vector<TrackTm>* out) {
        tm_what_ = what;
        tm_out_ = out;
    }

    // Before run(): also compute every track's sections (include/stratum_hip.h, sdsp_sections; the
    // request checked by sections_request_error, Cs its cell) into *out, one entry per track of the
    // call.  A pipeline without a request queues nothing for it; nested pipelines get none.
    void set_sections(const sdsp_sections_request& req, uint64_t Cs, std::vector<TrackSc>* out) {
        sc_req_ = req;
        sc_Cs_ = Cs;
        sc_out_ = out;
    }

    // Before run(): also measure every track's programme loudness (include/stratum_hip.h, sdsp_r128;
    // `what` checked by r128_request_error) into *out, one entry per track of the call.  A pipeline
    // without a request queues nothing for it; nested pipelines get none.
    void set_r128(uint32_t what, std::vector<TrackR128>* out) {
        r128_what_ = what;
        r128_out_ = out;
    }

    // Before run(): also compute every track's fingerprint and, with SDSP_FP_MATCH, compare every pair
    // of the call's tracks (include/stratum_hip.h, sdsp_fingerprint; the request checked by
    // fingerprint_request_error, Cs its cell) into *out.  A pipeline without a request queues nothing
    // for it; nested pipelines get none.
    void set_fingerprint(const sdsp_fingerprint_request& req, uint64_t Cs, FpOut* out) {
        fp_req_ = req;
        fp_Cs_ = Cs;
        fp_out_ = out;
    }

   private:
    Ctx c_;
    DeviceCtx& d_;
    const sdsp_config& cfg_;
    uint32_t sr_;
    // SDSP_STAGES_BPM_ONLY: the tempo path alone (src/lib.rs:86-910); the key
    // stream and the beat grid are not run, their result fields keep their defaults
    bool bpm_only_ = false;
    // the key path with the reference's sequential frame-energy fold (k_mask_r / k_hpcp) even where
    // the band-limited mask applies: run_locked's rerun of tracks whose key vote was near a decision
    bool exact_energy_ = false;
    // the key path alone (with exact_energy_: the rerun): front end, key stream, key fields only
    bool key_only_ = false;
    // a rerun started from inside the main pass (rerun_near): its buffers carry the prefix "X."
    // and its key path runs on the main stream, in that stream's slack beside the key stream
    bool nested_ = false;
    // the sub-batch being run is the call's last (its key vote runs alone at the tail)
    bool last_sub_ = false;
    uint64_t reruns_ = 0;
    uint64_t tail_reruns_ = 0;  // of those, the tracks rerun_tail reran in place (sdsp_debug_last_tail_reruns)
    double rerun_ms_ = 0.0;
    // the tempo path's STFT: frame size (AnalysisConfig::frame_size), bins, row stride
    const int fs_, nb_, s2_;
    // the key path's STFT: frame size, hop, row stride (key_fft / key_hop)
    const int kfs_, khop_, ks_;
    sdsp_stage_times times_{};
    // RMS / LUFS: gains (and LUFS status) of every track, folded once for the whole batch
    // before the sub-batches (the fold is a per-track sequential latency, not a throughput)
    std::vector<float> loud_gain_;
    std::vector<int> loud_stat_;
    std::unique_ptr<KeyPending> key_pending_;
    std::unique_ptr<KeyPending> tail_;  // the last sub-batch's pending join, kept for rerun_tail
    int sb_parity_ = 0;
    sdsp_overview_request ov_req_{};
    std::vector<TrackOv>* ov_out_ = nullptr;  // the call's overviews (set_overview), else nullptr
    uint32_t kt_L_ = 0, kt_H_ = 0;
    std::vector<TrackKt>* kt_out_ = nullptr;  // the call's key timelines (set_key_timeline), else nullptr
    uint32_t lv_what_ = 0;
    std::vector<TrackLv>* lv_out_ = nullptr;  // the call's levels (set_levels), else nullptr
    LevelsPending lv_pending_;
    uint32_t tm_what_ = 0;
    std::vector<TrackTm>* tm_out_ = nullptr;  // the call's tempo maps (set_tempo_map), else nullptr
    sdsp_sections_request sc_req_{};
    uint64_t sc_Cs_ = 0;
    std::vector<TrackSc>* sc_out_ = nullptr;  // the call's sections (set_sections), else nullptr
    uint32_t r128_what_ = 0;
    std::vector<TrackR128>* r128_out_ = nullptr;  // the call's programme loudness (set_r128), else nullptr
    R128Pending r128_pending_;
    sdsp_fingerprint_request fp_req_{};
    uint64_t fp_Cs_ = 0;
    FpOut* fp_out_ = nullptr;  // the call's fingerprints (set_fingerprint), else nullptr
    uint32_t* fp_words_ = nullptr;  // the call's word buffer on the device
    std::vector<std::unique_ptr<Timers>> fp_tm_;  // per sub-batch, on the vote stream: events 0-1 k_fp_cells, 1-2 k_fp_words
    bool map_on() const { return lv_out_ && (lv_what_ & SDSP_LEVELS_SILENCE_MAP); }

    // force_legacy_bpm skips the tempogram estimate (src/lib.rs:337): no escalation, no
    // candidates, the flags stay None; the hop-512 pass still feeds the onset detectors
    bool tg_on() const { return !cfg_.force_legacy_bpm; }
    bool mr_on() const { return cfg_.enable_tempogram_multi_resolution && tg_on(); }
    bool hpss_on() const { return cfg_.enable_hpss_onsets && cfg_.enable_onset_consensus; }
    bool perc_on() const { return mr_on() && cfg_.enable_tempogram_percussive_fallback; }
    bool dbg_on() const { return cfg_.has_debug_track_id != 0; }  // debug_track_id dumps (print_debug)
    void add_pass_times(const TempoPassOut& o);

    // pipeline.hip
    void loudness_prepass(const float* d_samples, const std::vector<uint64_t>& in_off,
                          const std::vector<uint64_t>& n_raw, std::vector<TrackRes>& res);
    void levels_prepass(const float* d_samples, const std::vector<uint64_t>& in_off, const std::vector<uint64_t>& n_raw,
                        std::vector<TrackRes>& res);
    void levels_join();
    // pipeline_r128.hip
    void r128_prepass(const float* d_samples, const std::vector<uint64_t>& in_off, const std::vector<uint64_t>& n_raw,
                      const std::vector<TrackRes>& res);
    void r128_join();
    void sub_batch(const float* d_samples, const std::vector<uint64_t>& in_off, const std::vector<uint64_t>& n_raw,
                   const std::vector<int>& idx, std::vector<TrackRes>& res);
    Front front(const float* d_samples, const std::vector<uint64_t>& in_off, const std::vector<uint64_t>& n_raw,
                const std::vector<int>& idx, std::vector<TrackRes>& res);
    TempoPassIn base_pass_in(const float* d_samples, const Front& f) const;
    Hpss hpss(const TempoPassOut& bo, const std::vector<TempoEst>& best, HostTrace& htr);
    Onsets onsets(const float* d_samples, const Front& f, const TempoPassIn& bin, const TempoPassOut& bo, const Hpss& hp);
    Onsets onset_lists(const float* d_erms, const uint64_t* d_nt, int HOP, const TempoPassOut& bo, const Hpss& hp);
    Beats beat_grid(const TempoPassIn& bin, const TempoPassOut& bo, const Onsets& on, const Tempo& tp);
    TempoMapQ tempo_map(const TempoPassIn& bin, const Onsets& on, const Tempo& tp, const Beats& bt);
    ResultsHost download_results(const Beats& bt, const TempoPassIn& bin, const TempoPassOut& bo,
                                 const TempoMapQ& tq = TempoMapQ{});
    void tempo_map_results(const ResultsHost& rh, const Front& f, const Tempo& tp);
    TrackTm track_tempo_map(const ResultsHost& rh, size_t i, float bpm, float conf, uint64_t first) const;
    Overview overview(const float* d_samples, const TempoPassIn& bin, const TempoPassOut& bo, Timers& tm);
    void overview_results(const Overview& ov, const Front& f, const TempoPassIn& bin, const TempoPassOut& bo, Timers& tm);
    void fill_results(const Front& f, const TempoPassIn& bin, const std::vector<TempoEst>& best, const Tempo& tp,
                      const ResultsHost& rh, std::vector<TrackRes>& res);

    // pipeline_tempo.hip
    void tempo_pass(const std::string& tag, const TempoPassIn& in, TempoPassOut& out);
    PassPlan pass_stft(const std::string& tag, const TempoPassIn& in, TempoPassOut& o, Timers& tm);
    PassFeat pass_features(const std::string& tag, const TempoPassIn& in, const PassPlan& pl, TempoPassOut& o);
    void pass_novelty(const std::string& tag, const TempoPassIn& in, const PassPlan& pl, const PassFeat& pf,
                      TempoPassOut& o);
    PassTg pass_tempograms(const std::string& tag, const TempoPassIn& in, const PassPlan& pl, const PassFeat& pf,
                           const TempoPassOut& o);
    void pass_select(const std::string& tag, const TempoPassIn& in, const PassPlan& pl, const PassTg& tg,
                     TempoPassOut& o);
    void select_lists(const std::string& tag, int P_T, const SelLists& sl, int top_n, int gate, int cand_cap,
                      TempoPassOut& o);
    void fuse_multires(const std::vector<int>& E, int NR, MrFuse& m, Tempo& tp);
    void tempo_down(int NR, Tempo& tp);
    Tempo seed_tempo(const Front& f, const std::vector<TempoEst>& best, const Onsets& on, std::vector<TrackRes>& res);
    void escalate(const Front& f, const TempoPassIn& bin, const TempoPassOut& bo, const std::vector<TempoEst>& best,
                  Tempo& tp, std::vector<TrackDbg>& tdbg, std::vector<TrackRes>& res);
    void perc_fallback(const Front& f, const TempoPassIn& bin, const TempoPassOut& bo, const std::vector<TempoEst>& best,
                       const Hpss& hp, Tempo& tp, std::vector<TrackRes>& res);
    void legacy_select(const Front& f, const TempoPassIn& bin, const Onsets& on, Tempo& tp, std::vector<TrackRes>& res);

    // pipeline_key.hip
    KeyLaunch launch_key(const float* d_samples, const TempoPassIn& bin, const Front& f);
    void fingerprint_plan(const std::vector<uint64_t>& n_raw);
    void fingerprint_finish(const std::vector<TrackRes>& res);
    KeyCond key_condition(const std::string& EP, float* mags8, const std::vector<uint64_t>& kpfx,
                          const std::vector<uint64_t>& ktile, uint64_t* d_kpfx, uint64_t* d_ktile, int* d_kid,
                          hipStream_t st2, Timers& kt);
    void section_novelty(KeyLaunch& kl, const TempoPassOut& bo);
    void sections_results(const SectionsOut& sc, Timers& kt, const std::vector<size_t>& at,
                          const std::vector<uint64_t>& first);
    void key_timeline_results(const KeyTimelineOut& ktl, const std::vector<size_t>& at, const std::vector<uint64_t>& first);
    void join_key_only(KeyLaunch& kl, const Front& f, std::vector<TrackRes>& res);
    std::vector<KeyOut> join_key(const float* d_samples, const std::vector<uint64_t>& in_off,
                                 const std::vector<uint64_t>& n_raw, const Front& f, KeyLaunch& kl, HostTrace& htr,
                                 std::vector<TrackRes>& res);
    std::vector<size_t> finish_key(std::vector<TrackRes>& res, bool keep_tail = false);
    void rerun_near(const float* d_samples, const std::vector<uint64_t>& in_off, const std::vector<uint64_t>& n_raw,
                    const std::vector<size_t>& near, std::vector<TrackRes>& res);
    void rerun_tail(const std::vector<size_t>& near, std::vector<TrackRes>& res);
    // the band path's spectrogram, block sums, HPCP parameters and chroma / energy buffers, as
    // tail_exact reads them
    void tail_buffers(KeyTail& t, const KeyCond& kc, float* mags8, uint64_t* d_kpfx, uint64_t total8) const;
    void tail_exact(const KeyTail& t, const int* d_sel, int n, const uint64_t* d_tiles, uint64_t n_tiles, hipStream_t st);
    void beat_sync_revote(const KeyLaunch& kl, const ResultsHost& rh, std::vector<KeyOut>& kout);

    // pipeline_debug.hip
    void debug_base(const TempoPassIn& bin, const TempoPassOut& bo, const std::vector<TempoEst>& best,
                    std::vector<TrackDbg>& tdbg);
    void debug_multires(const std::vector<int>& E, bool own512, int cap512, int cap_aux, size_t rows512,
                        const TempoPassOut& o256, const TempoPassOut& b512, const TempoPassOut& o1024,
                        const std::vector<int>& n256, const std::vector<int>& n512, const std::vector<int>& n1024,
                        const TempoEst* d_mr, const MrDbg* d_mdbg, std::vector<TrackDbg>& tdbg);
    void debug_key(const KeyLaunch& kl, const std::vector<KeyOut>& kout, std::vector<TrackDbg>& tdbg);
};

}  // namespace sdsp
