"""Unit-level bindings of the CPU restatement (the "unit probes" sections of oracle/o_*.cpp).

TEST INFRASTRUCTURE: imported only by tests/ (tests/test_oracle_units_*.py restate the
reference's own #[test] functions against these).  Each function is named after the reference
function it exposes and raises AnalysisError(code, message) where the reference returns Err.
"""
import ctypes as C

import numpy as np

import oracle

fp = C.POINTER(C.c_float)
u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
i32p = C.POINTER(C.c_int32)

ERRORS = {1: "InvalidInput", 2: "DecodingError", 3: "ProcessingError", 4: "NotImplemented", 5: "NumericalError"}


class AnalysisError(Exception):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code
        self.kind = ERRORS.get(code, str(code))


_L = None


def lib():
    global _L
    if _L is None:
        L = oracle.lib()
        L.sdsp_oracle_probe_error.restype = C.c_char_p
        L.sdsp_oracle_energy_flux_onsets.argtypes = [fp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_float, u64p, C.c_uint64]
        L.sdsp_oracle_energy_flux_onsets.restype = C.c_int64
        L.sdsp_oracle_spectral_flux_onsets.argtypes = [fp, C.c_uint64, C.c_uint64, u64p, C.c_float, u64p, C.c_uint64]
        L.sdsp_oracle_spectral_flux_onsets.restype = C.c_int64
        L.sdsp_oracle_hfc_onsets.argtypes = [fp, C.c_uint64, C.c_uint64, u64p, C.c_uint32, C.c_float, u64p, C.c_uint64]
        L.sdsp_oracle_hfc_onsets.restype = C.c_int64
        L.sdsp_oracle_detect_and_trim.argtypes = [fp, C.c_uint64, C.c_uint32, C.c_float, C.c_uint32, C.c_uint64, u64p,
                                                  u64p, C.c_uint64]
        L.sdsp_oracle_detect_and_trim.restype = C.c_int64
        L.sdsp_oracle_novelty.argtypes = [C.c_int32, fp, C.c_uint64, C.c_uint64, u64p, C.c_uint32, C.c_uint64, fp]
        L.sdsp_oracle_novelty.restype = C.c_int64
        L.sdsp_oracle_combined_novelty.argtypes = [fp, C.c_uint64, fp, C.c_uint64, fp, C.c_uint64, C.c_float, C.c_float,
                                                   C.c_float, C.c_uint64, C.c_uint64, fp]
        L.sdsp_oracle_combined_novelty.restype = C.c_int64
        L.sdsp_oracle_tempogram.argtypes = [C.c_int32, fp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_float, C.c_float,
                                            C.c_float, fp, fp, C.c_uint64]
        L.sdsp_oracle_tempogram.restype = C.c_int64
        L.sdsp_oracle_tempogram_estimate.argtypes = [fp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_float,
                                                     C.c_float, C.c_float, fp]
        L.sdsp_oracle_tempogram_estimate.restype = C.c_int32
        L.sdsp_oracle_multi_resolution_analysis.argtypes = [fp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_float, C.c_float,
                                                            C.c_float, fp]
        L.sdsp_oracle_multi_resolution_analysis.restype = C.c_int32
        L.sdsp_oracle_beat_grid.argtypes = [C.c_float, C.c_float, fp, C.c_uint64, C.c_uint32, fp, fp, C.c_uint64, u64p, fp]
        L.sdsp_oracle_beat_grid.restype = C.c_int32
        L.sdsp_oracle_beat_grid_diag.argtypes = L.sdsp_oracle_beat_grid.argtypes + [i32p]
        L.sdsp_oracle_beat_grid_diag.restype = C.c_int32
        L.sdsp_oracle_downbeats.argtypes = [fp, C.c_uint64, C.c_float, C.c_uint32, fp]
        L.sdsp_oracle_downbeats.restype = C.c_int64
        L.sdsp_oracle_grid_stability.argtypes = [fp, C.c_uint64, C.c_float, fp]
        L.sdsp_oracle_grid_stability.restype = C.c_int32
        L.sdsp_oracle_tempo_variations.argtypes = [fp, C.c_uint64, C.c_float, fp, C.c_uint64]
        L.sdsp_oracle_tempo_variations.restype = C.c_int64
        L.sdsp_oracle_bayes.argtypes = [C.c_int32, C.c_float, C.c_float, fp, C.c_uint64, C.c_float, fp, C.c_uint64]
        L.sdsp_oracle_bayes.restype = C.c_int64
        L.sdsp_oracle_time_signature.argtypes = [fp, C.c_uint64, C.c_float, u32p, fp]
        L.sdsp_oracle_time_signature.restype = C.c_int32
        L.sdsp_oracle_detect_key.argtypes = [fp, C.c_uint64, C.c_uint64, fp, C.c_uint64, i32p, fp, fp, i32p]
        L.sdsp_oracle_detect_key.restype = C.c_int32
        L.sdsp_oracle_smooth_chroma.argtypes = [fp, C.c_uint64, C.c_uint64, C.c_int32, fp]
        L.sdsp_oracle_dot.argtypes = [fp, fp, C.c_uint64]
        L.sdsp_oracle_dot.restype = C.c_float
        _L = L
    return _L


def _check(rc):
    if rc < 0:
        raise AnalysisError(-rc, lib().sdsp_oracle_probe_error().decode())
    return rc


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _p(a):
    return a.ctypes.data_as(fp) if a.size else C.cast(C.c_void_p(0), fp)


def _spec(spec):
    """A list of frames (possibly ragged, as the reference's Vec<Vec<f32>>) -> flat, frames,
    bins, row lengths.  Ragged rows are zero-padded; the probe rejects them like the reference."""
    rows = [np.asarray(r, dtype=np.float32) for r in spec]
    frames = len(rows)
    lens = np.array([len(r) for r in rows], dtype=np.uint64)
    bins = int(lens.max()) if frames else 0
    flat = np.zeros((frames, bins), dtype=np.float32)
    for i, r in enumerate(rows):
        flat[i, :len(r)] = r
    return np.ascontiguousarray(flat.ravel()), frames, bins, lens


def _u64(a):
    return a.ctypes.data_as(u64p) if a.size else C.cast(C.c_void_p(0), u64p)


def _list_call(fn, *args, cap=1 << 16):
    out = np.zeros(cap, dtype=np.uint64)
    n = _check(fn(*args, _u64(out), cap))
    return [int(v) for v in out[:n]]


# ---- onsets / preprocessing ----
def detect_energy_flux_onsets(samples, frame_size, hop_size, threshold_db):
    x = _f32(samples)
    return _list_call(lib().sdsp_oracle_energy_flux_onsets, _p(x), x.size, frame_size, hop_size, threshold_db)


def detect_spectral_flux_onsets(spec, percentile):
    flat, fr, b, lens = _spec(spec)
    return _list_call(lib().sdsp_oracle_spectral_flux_onsets, _p(flat), fr, b, _u64(lens), percentile)


def detect_hfc_onsets(spec, sample_rate, percentile):
    flat, fr, b, lens = _spec(spec)
    return _list_call(lib().sdsp_oracle_hfc_onsets, _p(flat), fr, b, _u64(lens), sample_rate, percentile)


def detect_and_trim(samples, sample_rate, threshold_db=-40.0, min_duration_ms=500, frame_size=2048):
    """SilenceDetector::default() = (-40 dB, 500 ms, 2048).  Returns (trimmed samples, silence map)."""
    x = _f32(samples)
    trim = np.zeros(2, dtype=np.uint64)
    cap = 4096
    reg = np.zeros(2 * cap, dtype=np.uint64)
    n = _check(lib().sdsp_oracle_detect_and_trim(_p(x), x.size, sample_rate, threshold_db, min_duration_ms, frame_size,
                                                 _u64(trim), _u64(reg), cap))
    return x[int(trim[0]):int(trim[1])], [(int(reg[2 * i]), int(reg[2 * i + 1])) for i in range(n)]


# ---- novelty / tempograms ----
def _novelty(kind, spec, sample_rate=44100, k=4):
    flat, fr, b, lens = _spec(spec)
    out = np.zeros(max(fr, 1), dtype=np.float32)
    n = _check(lib().sdsp_oracle_novelty(kind, _p(flat), fr, b, _u64(lens), sample_rate, k, _p(out)))
    return out[:n]


def spectral_flux_novelty(spec):
    return _novelty(0, spec)


def energy_flux_novelty(spec):
    return _novelty(1, spec)


def hfc_novelty(spec, sample_rate):
    return _novelty(2, spec, sample_rate)


def superflux_novelty(spec, max_filter_bins):
    return _novelty(3, spec, k=max_filter_bins)


def combined_novelty(spectral, energy, hfc, params=(0.5, 0.3, 0.2, 16, 5)):
    s, e, h = _f32(spectral), _f32(energy), _f32(hfc)
    out = np.zeros(max(s.size, e.size, h.size, 1), dtype=np.float32)
    n = _check(lib().sdsp_oracle_combined_novelty(_p(s), s.size, _p(e), e.size, _p(h), h.size, *params, _p(out)))
    return out[:n]


def _tempogram(kind, novelty, sr, hop, lo, hi, res):
    x = _f32(novelty)
    cap = 1 << 16
    b, v = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    n = _check(lib().sdsp_oracle_tempogram(kind, _p(x), x.size, sr, hop, lo, hi, res, _p(b), _p(v), cap))
    return list(zip(b[:n].tolist(), v[:n].tolist()))


def fft_tempogram(novelty, sample_rate, hop_size, min_bpm, max_bpm):
    return _tempogram(0, novelty, sample_rate, hop_size, min_bpm, max_bpm, 1.0)


def autocorrelation_tempogram(novelty, sample_rate, hop_size, min_bpm, max_bpm, bpm_resolution):
    return _tempogram(1, novelty, sample_rate, hop_size, min_bpm, max_bpm, bpm_resolution)


def find_best_bpm(tempogram):
    """find_best_bpm_fft / find_best_bpm_autocorr: (bpm, value, confidence) or None."""
    if not tempogram:
        return None
    return oracle.find_best(tempogram)


def estimate_bpm_tempogram(spec, sample_rate, hop_size, min_bpm, max_bpm, bpm_resolution):
    flat, fr, b, _ = _spec(spec)
    out = np.zeros(3, np.float32)
    _check(lib().sdsp_oracle_tempogram_estimate(_p(flat), fr, b, sample_rate, hop_size, min_bpm, max_bpm,
                                                bpm_resolution, _p(out)))
    return float(out[0]), float(out[1]), int(out[2])


def multi_resolution_analysis(spec, sample_rate, base_hop_size, min_bpm, max_bpm, bpm_resolution):
    flat, fr, b, _ = _spec(spec)
    out = np.zeros(3, np.float32)
    _check(lib().sdsp_oracle_multi_resolution_analysis(_p(flat), fr, b, sample_rate, min_bpm, max_bpm, bpm_resolution,
                                                       _p(out)))
    return float(out[0]), float(out[1]), int(out[2])


# ---- beat tracking ----
def generate_beat_grid(bpm, bpm_confidence, onsets_s, sample_rate):
    """(beats, downbeats, bars, stability); AnalysisError where the reference returns Err."""
    on = _f32(onsets_s)
    cap = 1 << 16
    b, d = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    counts = np.zeros(2, np.uint64)
    st = C.c_float(0)
    rc = lib().sdsp_oracle_beat_grid(bpm, bpm_confidence, _p(on), on.size, sample_rate, _p(b), _p(d), cap, _u64(counts),
                                     C.byref(st))
    if rc != 0:
        raise AnalysisError(1, "generate_beat_grid failed")
    beats, downs = b[:int(counts[0])].tolist(), d[:int(counts[1])].tolist()
    return beats, downs, list(downs), st.value


def beat_grid_diag(bpm, bpm_confidence, onsets_s, sample_rate):
    """generate_beat_grid with its branch record: None where the reference returns Err, else a dict of
    beats, downbeats (float32 arrays), stability (float32) and BeatDiag's variable, refined,
    beats_per_bar and hmm_beats (the whole-track HMM's beat count)."""
    on = _f32(onsets_s)
    cap = 8 * on.size + 64
    b, d = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    counts = np.zeros(2, np.uint64)
    st = C.c_float(0)
    diag = np.zeros(4, np.int32)
    rc = lib().sdsp_oracle_beat_grid_diag(bpm, bpm_confidence, _p(on), on.size, sample_rate, _p(b), _p(d), cap,
                                          _u64(counts), C.byref(st), diag.ctypes.data_as(i32p))
    if rc != 0:
        return None
    assert int(counts[0]) <= cap
    return dict(beats=b[:int(counts[0])].copy(), downbeats=d[:int(counts[1])].copy(), stability=np.float32(st.value),
                variable=bool(diag[0]), refined=bool(diag[1]), beats_per_bar=int(diag[2]), hmm_beats=int(diag[3]))


# ---- the onset detectors' tails over their curves (tests/test_gpu_onset_stages.py) ----
def energy_onsets_from_rms(rms, hop, n, threshold_db=-20.0):
    """detect_energy_flux_onsets after its frame RMS: onset sample positions of an n-sample signal."""
    L = lib()
    L.sdsp_oracle_energy_onsets_rms.argtypes = [fp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_float, u64p, C.c_uint64]
    L.sdsp_oracle_energy_onsets_rms.restype = C.c_int64
    e = _f32(rms)
    return _list_call(L.sdsp_oracle_energy_onsets_rms, _p(e), e.size, hop, n, threshold_db, cap=e.size + 1)


def peaks_over_percentile(flux, percentile):
    """The shared tail of the spectral-flux, HFC and HPSS detectors: onset frame indices (i + 1 for a
    peak at flux index i); AnalysisError for a percentile outside [0, 1], as its callers raise."""
    L = lib()
    L.sdsp_oracle_peaks_over_percentile.argtypes = [fp, C.c_uint64, C.c_float, u64p, C.c_uint64]
    L.sdsp_oracle_peaks_over_percentile.restype = C.c_int64
    f = _f32(flux)
    return _list_call(L.sdsp_oracle_peaks_over_percentile, _p(f), f.size, percentile, cap=f.size + 1)


def hpss_onsets_from_energy(energy, percentile):
    """detect_hpss_onsets after its percussive frame energies: onset frame indices."""
    L = lib()
    L.sdsp_oracle_hpss_energy_onsets.argtypes = [fp, C.c_uint64, C.c_float, u64p, C.c_uint64]
    L.sdsp_oracle_hpss_energy_onsets.restype = C.c_int64
    e = _f32(energy)
    return _list_call(L.sdsp_oracle_hpss_energy_onsets, _p(e), e.size, percentile, cap=e.size + 1)


def consensus_select(lists, weights, tol_ms, sample_rate):
    """The onsets the analysis hands to the legacy estimator and the beat tracker (src/lib.rs:258-291):
    vote_onsets over the four lists, then the centres of the clusters at least two methods voted for,
    or every centre when there is none, sorted and deduplicated; the energy list (lists[0]) when the
    vote fails (zero tolerance, a negative weight) or nothing clustered."""
    cands = oracle.vote_onsets(lists, weights, tol_ms, sample_rate)
    if isinstance(cands, int):  # Err
        return [int(v) for v in lists[0]]
    strong = sorted({t for t, voted, _ in cands if voted >= 2})
    chosen = strong if strong else sorted({t for t, _, _ in cands})
    return chosen if chosen else [int(v) for v in lists[0]]


def detect_downbeats(beats, bpm, beats_per_bar=4):
    x = _f32(beats)
    out = np.zeros(max(x.size, 1), np.float32)
    n = _check(lib().sdsp_oracle_downbeats(_p(x), x.size, bpm, beats_per_bar, _p(out)))
    return out[:n].tolist()


def calculate_grid_stability(times, bpm):
    x = _f32(times)
    v = C.c_float(0)
    _check(lib().sdsp_oracle_grid_stability(_p(x), x.size, bpm, C.byref(v)))
    return v.value


def detect_tempo_variations(beats, nominal_bpm):
    """[(start, end, bpm, confidence, is_variable)]"""
    x = _f32(beats)
    cap = 4096
    out = np.zeros(5 * cap, np.float32)
    n = _check(lib().sdsp_oracle_tempo_variations(_p(x), x.size, nominal_bpm, _p(out), cap))
    return [(float(out[5 * i]), float(out[5 * i + 1]), float(out[5 * i + 2]), float(out[5 * i + 3]),
             bool(out[5 * i + 4])) for i in range(n)]


def has_tempo_variation(segments):
    return any(s[4] for s in segments)  # tempo_variation.rs:225-227


class BayesianBeatTracker:
    """bayesian.rs:77-272; every call rebuilds the tracker from (bpm, confidence) like new()."""

    def __init__(self, initial_bpm, initial_confidence):
        self.bpm0, self.conf0 = float(initial_bpm), float(initial_confidence)
        out = np.zeros(64, np.float32)
        n = _check(lib().sdsp_oracle_bayes(3, self.bpm0, self.conf0, _p(np.zeros(0, np.float32)), 0, 0.0, _p(out), 64))
        self.current_bpm, self.current_confidence = float(out[0]), float(out[1])
        self.history = out[2:2 + n].tolist()

    def _op(self, op, onsets=(), x=0.0, cap=4096):
        on = _f32(onsets)
        out = np.zeros(cap, np.float32)
        n = _check(lib().sdsp_oracle_bayes(op, self.bpm0, self.conf0, _p(on), on.size, x, _p(out), cap))
        return n, out

    def generate_bpm_candidates(self):
        n, out = self._op(0)
        return out[:n].tolist()

    def compute_likelihood(self, onsets, bpm):
        return float(self._op(1, onsets, bpm)[1][0])

    def compute_prior(self, bpm):
        return float(self._op(2, (), bpm)[1][0])

    def update_with_onsets(self, onsets, sample_rate=44100):
        n, out = self._op(4, onsets)
        self.current_bpm, self.current_confidence = float(out[0]), float(out[1])
        self.history = out[2:2 + n].tolist()
        return self.current_bpm, self.current_confidence


def detect_time_signature(beats, bpm):
    x = _f32(beats)
    bpb, conf = C.c_uint32(0), C.c_float(0)
    _check(lib().sdsp_oracle_time_signature(_p(x), x.size, bpm, C.byref(bpb), C.byref(conf)))
    return bpb.value, conf.value


# ---- key ----
def detect_key_weighted(chroma_vectors, weights=None):
    """(key index mode*12+tonic, confidence, all_scores [(key, score)] sorted, top_keys)"""
    rows = [list(r) for r in chroma_vectors]
    dims = len(rows[0]) if rows else 12
    if any(len(r) != dims for r in rows):
        dims = -1  # ragged: rejected like the reference's per-vector check
    flat = _f32([v for r in rows for v in r]) if dims == 12 else np.zeros(0, np.float32)
    w = _f32(weights) if weights is not None else None
    key, conf = C.c_int32(0), C.c_float(0)
    sc, ks = np.zeros(24, np.float32), np.zeros(24, np.int32)
    _check(lib().sdsp_oracle_detect_key(_p(flat), len(rows), dims if dims > 0 else 0, _p(w) if w is not None else None,
                                        w.size if w is not None else 0, C.byref(key), C.byref(conf), _p(sc),
                                        ks.ctypes.data_as(i32p)))
    all_scores = list(zip(ks.tolist(), sc.tolist()))
    return key.value, conf.value, all_scores, all_scores[:3]


def detect_key(chroma_vectors):
    return detect_key_weighted(chroma_vectors, None)


def smooth_chroma(chroma_vectors, window_size, average=False):
    x = _f32(chroma_vectors).reshape(-1)
    frames = x.size // 12
    out = np.zeros(x.size, np.float32)
    lib().sdsp_oracle_smooth_chroma(_p(x), frames, window_size, 1 if average else 0, _p(out))
    return out.reshape(frames, 12)


def smooth_chroma_average(chroma_vectors, window_size):
    return smooth_chroma(chroma_vectors, window_size, average=True)


def dot_product(a, b):
    x, y = _f32(a), _f32(b)
    return lib().sdsp_oracle_dot(_p(x), _p(y), min(x.size, y.size))


def compute_key_clarity(scores):
    return oracle.key_clarity([s for _, s in scores]) if scores else 0.0


# ---- stage exports (tests/test_oracle_stage_exports.py, tests/test_gpu_tempo_stages.py, test_gpu_key_stages.py) ----
_STAGE_WHAT = {"energy": 0, "hfc": 1, "sfx_raw": 2, "sf": 3, "nov": 4, "fft_bpm": 5, "fft_val": 6, "acf_bpm": 7,
               "acf_val": 8, "melf": 9}


def tempo_stages(spec, sample_rate=44100, hop=512, config=None):
    """tempogram_impl's seeded variants under the configuration's BandCfg, in order: {name: dict} with
    s, e (band bins; mel: e = n_mels), energy, hfc (raw per frame), sfx_raw, sf (superflux before /
    after normalisation), nov, fft / acf ((n, 2) arrays of (bpm, value), sorted as the tempogram
    returns them) and, for mel, melf (frames, n_mels)."""
    L = lib()
    L.sdsp_oracle_tempo_stages.argtypes = [fp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                           C.POINTER(oracle.SdspConfig)]
    L.sdsp_oracle_tempo_stages.restype = C.c_int64
    L.sdsp_oracle_tempo_stage_get.argtypes = [C.c_uint64, C.c_int32, fp, C.c_uint64, C.c_char_p, u64p]
    L.sdsp_oracle_tempo_stage_get.restype = C.c_int64
    cfg = config if config is not None else oracle.default_config()
    m = np.ascontiguousarray(spec, dtype=np.float32)
    n = L.sdsp_oracle_tempo_stages(_p(m), m.shape[0], m.shape[1], sample_rate, hop, C.byref(cfg))
    out = {}
    for i in range(n):
        name = C.create_string_buffer(8)
        info = np.zeros(2, np.uint64)

        def get(what):
            k = L.sdsp_oracle_tempo_stage_get(i, _STAGE_WHAT[what], None, 0, name, _u64(info))
            a = np.zeros(max(k, 1), np.float32)
            L.sdsp_oracle_tempo_stage_get(i, _STAGE_WHAT[what], _p(a), a.size, name, _u64(info))
            return a[:k]

        d = {k: get(k) for k in ("energy", "hfc", "sfx_raw", "sf", "nov")}
        d["fft"] = np.stack([get("fft_bpm"), get("fft_val")], axis=1)
        d["acf"] = np.stack([get("acf_bpm"), get("acf_val")], axis=1)
        d["s"], d["e"] = int(info[0]), int(info[1])
        if name.value == b"mel":
            d["melf"] = get("melf").reshape(m.shape[0], d["e"])
        out[name.value.decode()] = d
    return out


def tempo_stages_estimate():
    """(bpm, confidence, method agreement) of the tempogram_impl call the last tempo_stages() made."""
    out = np.zeros(3, np.float32)
    lib().sdsp_oracle_tempo_stages_estimate.argtypes = [fp]
    lib().sdsp_oracle_tempo_stages_estimate(_p(out))
    return float(out[0]), float(out[1]), int(out[2])


VARIANT_KINDS = {"full": 0, "low": 1, "mid": 2, "high": 3, "mel": 4}
SEL_REC_I = ("n_in", "n_out", "n_dup", "n_uniq", "n_pen_hi", "n_pen_lo", "sb0", "sb1", "sb2", "sb3", "sb4", "fold",
             "trap_low", "trap_high", "family", "fold_into_trap", "weak", "ambiguous", "n_tie", "n_at_tol", "n_tie_ac",
             "n_at_tol_ac")
SEL_REC_F = ("fft_pb", "ac_pb", "s_base", "s_2x", "s_half")


def _pairs(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 2))


def tempo_select(variants, min_bpm, max_bpm, res, config=None):
    """tempogram_impl from its seeded variants on, over variants = [(name, weight, fft list, acf
    list)] with "full" first and (n, 2) lists of (bpm, value) in the tempograms' order, under the
    BandCfg analyze passes for the configuration; then the ambiguity gate over the candidates
    truncated to the base pass's top_n.  Returns None where the reference returns Err, else a dict:
    bpm, conf (float32), agree, cands (n, 4: bpm, score, fft_norm, autocorr_norm; the full scored
    list) and the branch record (SEL_REC_I / SEL_REC_F: the gate's flags and supports among them;
    fold: 0 best <= 180, 1 folded value out of range, 2 no candidate there, 3 kept out by both
    ratios, 4 taken; n_tie / n_at_tol (_ac: the autocorrelation lists): scoring lookups that passed
    over an equidistant entry of another value, and whose entry lies exactly at the tolerance)."""
    L = lib()
    L.sdsp_oracle_tempo_select.argtypes = [i32p, fp, C.c_int32, fp, i32p, fp, i32p, C.c_float, C.c_float, C.c_float,
                                           C.POINTER(oracle.SdspConfig), fp, fp, C.c_uint64, i32p, fp]
    L.sdsp_oracle_tempo_select.restype = C.c_int64
    cfg = config if config is not None else oracle.default_config()
    kind = np.array([VARIANT_KINDS[v[0]] for v in variants], np.int32)
    w = np.array([v[1] for v in variants], np.float32)
    ffts, acfs = [_pairs(v[2]) for v in variants], [_pairs(v[3]) for v in variants]
    fn, an = np.array([len(a) for a in ffts], np.int32), np.array([len(a) for a in acfs], np.int32)
    fft = np.ascontiguousarray(np.concatenate(ffts + [np.zeros((1, 2), np.float32)]))
    acf = np.ascontiguousarray(np.concatenate(acfs + [np.zeros((1, 2), np.float32)]))
    cap = 1024
    est, cands = np.zeros(3, np.float32), np.zeros((cap, 4), np.float32)
    ri, rf = np.zeros(len(SEL_REC_I), np.int32), np.zeros(len(SEL_REC_F), np.float32)
    n = L.sdsp_oracle_tempo_select(kind.ctypes.data_as(i32p), _p(w), len(variants), _p(fft), fn.ctypes.data_as(i32p),
                                   _p(acf), an.ctypes.data_as(i32p), min_bpm, max_bpm, res, C.byref(cfg), _p(est),
                                   _p(cands), cap, ri.ctypes.data_as(i32p), _p(rf))
    if n < 0:
        return None
    assert n <= cap
    d = dict(bpm=est[0], conf=est[1], agree=int(est[2]), cands=cands[:n].copy())
    d.update({k: int(v) for k, v in zip(SEL_REC_I, ri)})
    d.update({k: np.float32(v) for k, v in zip(SEL_REC_F, rf)})
    return d


MR_REC_I = ("fd", "fu", "tf", "fd_a0", "fd_a1", "fu_a0", "fu_a1", "tf_label", "fam", "forbid", "better", "clause",
            "fd_eval", "fu_eval", "fd_eval_a1", "fu_eval_a1", "n_hyps", "n_uniq", "n_dup", "n_h102", "n_2t102",
            "n_r2_110", "n_r2_100", "n_rh_110", "n_rh_100", "n_pen210", "n_pen180", "n_pen60", "n_margin_lo", "n_reset",
            "n_prior", "n_fam", "fam_eval", "chosen", "cur_phase", "fam_ph0", "fam_ph1", "fam_ph2", "fam_ph3", "fam_ph4")
MR_REC_F = ("fd_from", "fd_to", "fd_ratio", "fu_from", "fu_to", "fu_ratio", "tf_from", "tf_to", "tf_sup0", "tf_sup1",
            "tf_al0", "tf_al1", "rel", "fd_eval_ratio", "fu_eval_ratio", "max_alt", "cur_align")


def multires_fuse(c256, c512, c1024, nov512, sr, base, config=None):
    """multi_resolution from its hypothesis loop on over the three hops' candidate lists ((n, 4)
    arrays, or None for a hop whose tempogram failed) and the hop-512 novelty, then the acceptance
    against base = (bpm, conf, agree, trap_low, trap_high).  Returns a dict: ok (False where
    multi_resolution returns Err; everything else is then zero), bpm, conf (float32), agree, used and
    the branch record (MR_REC_I / MR_REC_F, fam_bpm / fam_sup / fam_align of the n_fam family members
    considered; fd_eval / fu_eval: 0 the fold gate was not reached, else 1 + 4 (agreement ok) +
    2 (supports > 0) + 1 (ratio ok); clause: bits of the acceptance's three clauses; cur_phase /
    fam_phase: the first beat phase that gives the current best's / each member's alignment)."""
    L = lib()
    L.sdsp_oracle_multires_fuse.argtypes = [fp, C.c_int32, fp, C.c_int32, fp, C.c_int32, fp, C.c_uint64, C.c_uint32, fp,
                                            C.POINTER(oracle.SdspConfig), fp, i32p, fp]
    L.sdsp_oracle_multires_fuse.restype = C.c_int32
    cfg = config if config is not None else oracle.default_config()
    ls = [None if c is None else np.ascontiguousarray(np.asarray(c, np.float32).reshape(-1, 4)) for c in (c256, c512, c1024)]
    ns = [-1 if a is None else len(a) for a in ls]
    held = [np.zeros(4, np.float32) if a is None or not len(a) else a for a in ls]  # kept alive over the call
    ps = [_p(a) for a in held]
    nov = _f32(nov512)
    b5 = np.array([base[0], base[1], base[2], base[3], base[4]], np.float32)
    est = np.zeros(3, np.float32)
    ri, rf = np.zeros(len(MR_REC_I), np.int32), np.zeros(32, np.float32)
    ok = L.sdsp_oracle_multires_fuse(ps[0], ns[0], ps[1], ns[1], ps[2], ns[2], _p(nov), nov.size, sr, _p(b5), C.byref(cfg),
                                     _p(est), ri.ctypes.data_as(i32p), _p(rf))
    d = dict(ok=bool(ok), bpm=est[0], conf=est[1], agree=int(est[2]))
    d.update({k: int(v) for k, v in zip(MR_REC_I, ri)})
    d.update({k: np.float32(v) for k, v in zip(MR_REC_F, rf)})
    d["used"] = d["better"]
    d["fam_phase"] = [d[f"fam_ph{k}"] for k in range(d["n_fam"])]
    d["fam_bpm"], d["fam_sup"], d["fam_align"] = (rf[17 + 5 * j:17 + 5 * j + d["n_fam"]].copy() for j in range(3))
    return d


def spectral_flux_curve(spec):
    """The flux detect_spectral_flux_onsets thresholds: frames - 1 values."""
    L = lib()
    L.sdsp_oracle_spectral_flux_curve.argtypes = [fp, C.c_uint64, C.c_uint64, fp]
    L.sdsp_oracle_spectral_flux_curve.restype = C.c_int64
    m = np.ascontiguousarray(spec, dtype=np.float32)
    out = np.zeros(max(m.shape[0], 1), np.float32)
    n = _check(L.sdsp_oracle_spectral_flux_curve(_p(m), m.shape[0], m.shape[1], _p(out)))
    return out[:n]


def key_stages(spec, sample_rate=44100, config=None):
    """The configuration's key spectrogram conditioning, then hpcp_frames with its peaks, harmonics,
    decay and mag_power: (conditioned spectrogram, chroma (frames, 12), frame energies)."""
    L = lib()
    L.sdsp_oracle_key_stages.argtypes = [fp, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(oracle.SdspConfig), fp, fp]
    L.sdsp_oracle_key_stages.restype = C.c_int32
    cfg = config if config is not None else oracle.default_config()
    m = np.array(spec, dtype=np.float32, order="C")
    ch, en = np.zeros((m.shape[0], 12), np.float32), np.zeros(m.shape[0], np.float32)
    if L.sdsp_oracle_key_stages(_p(m), m.shape[0], m.shape[1], sample_rate, C.byref(cfg), _p(ch), _p(en)) != 0:
        raise AnalysisError(1, "key_stages: empty spectrogram")
    return m, ch, en


def key_from_raw(raw):
    """detect_key_weighted from its 24 raw scores on: (sorted refined scores, their key indices)."""
    L = lib()
    L.sdsp_oracle_key_from_raw.argtypes = [fp, fp, i32p]
    L.sdsp_oracle_key_from_raw.restype = None
    r = _f32(raw)
    sc, ks = np.zeros(24, np.float32), np.zeros(24, np.int32)
    L.sdsp_oracle_key_from_raw(_p(r), _p(sc), ks.ctypes.data_as(i32p))
    return sc, ks


def key_vote(chroma, energies, config=None):
    """analyze's key decision over raw chroma rows (F, 12) and frame energies (F,): a dict with key
    (mode * 12 + tonic), mode, tonic, confidence, clarity, used_segments, weights_used, err (the
    reference's Err path: all-zero key fields), chroma_s (F, 12) sharpened and smoothed, t0 / frames
    (the voted slice), weights (over the slice; empty without frame weighting), tab / order (the
    final sorted table), seg_raw (n, 24) / seg_clarity (n,) per voted-on segment in order and
    full_raw (m, 24): the raw scores of every other detect_key_weighted call (the full slice's, the
    ensemble's two)."""
    L = lib()
    L.sdsp_oracle_key_vote.argtypes = [fp, fp, C.c_uint64, C.POINTER(oracle.SdspConfig), i32p, fp, fp, fp, fp, i32p]
    L.sdsp_oracle_key_vote.restype = C.c_int32
    L.sdsp_oracle_study_key_trace_get.restype = C.c_uint64
    L.sdsp_oracle_study_key_trace_get.argtypes = [fp, C.c_uint64]
    cfg = config if config is not None else oracle.default_config()
    ch = np.ascontiguousarray(chroma, dtype=np.float32).reshape(-1, 12)
    en = np.ascontiguousarray(energies, dtype=np.float32).reshape(-1)
    if ch.shape[0] != en.size:
        raise ValueError("key_vote: one energy per chroma row")
    F = en.size
    info, cc = np.zeros(9, np.int32), np.zeros(2, np.float32)
    cs, w = np.zeros((max(F, 1), 12), np.float32), np.zeros(max(F, 1), np.float32)
    tab, order = np.zeros(24, np.float32), np.zeros(24, np.int32)
    L.sdsp_oracle_study_key_trace(1)
    try:
        rc = L.sdsp_oracle_key_vote(_p(ch), _p(en), F, C.byref(cfg), info.ctypes.data_as(i32p), _p(cc), _p(cs), _p(w),
                                    _p(tab), order.ctypes.data_as(i32p))
        n = int(L.sdsp_oracle_study_key_trace_get(None, 0))
        tr = np.zeros(max(n, 1), np.float32)
        L.sdsp_oracle_study_key_trace_get(_p(tr), n)
    finally:
        L.sdsp_oracle_study_key_trace(0)
    if rc != 0:
        raise AnalysisError(1, "key_vote: bad arguments")
    tr = tr[:n]
    nseg = int(info[8])  # segments come first, 24 raw scores and a clarity each; whole-slice calls (24 each) follow
    seg = tr[:nseg * 25].reshape(nseg, 25)
    return {"err": bool(info[0]), "mode": int(info[1]), "tonic": int(info[2]), "key": int(info[1]) * 12 + int(info[2]),
            "confidence": cc[0], "clarity": cc[1], "used_segments": int(info[3]), "weights_used": bool(info[4]),
            "t0": int(info[5]), "frames": int(info[6]), "chroma_s": cs[:F], "weights": w[:int(info[7])].copy(),
            "tab": tab, "order": order, "seg_raw": seg[:, :24].copy(), "seg_clarity": seg[:, 24].copy(),
            "full_raw": tr[nseg * 25:].reshape(-1, 24).copy()}
