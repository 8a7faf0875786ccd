"""Onset lists for the beat-grid stage tests (tests/test_gpu_beat_stages.py, test_oracle_stage_wrappers.py).

A case is an onset list on a grid of `nb` slots at `bpm`, each slot kept with a seeded probability and
optionally jittered, plus the tempo estimate the beat stage runs with and the condition that makes
the case reach the branch of k_beat it is named for.  Every condition is stated on what the oracle
alone computes (units.beat_grid_diag, oracle.hmm_track), so it is checked without a GPU; the seeds
below were chosen on the CPU so that it holds.
"""
import numpy as np

import oracle
import units

SR = 44100
FS, HOP = 2048, 512  # the default configuration's framing, from which a track's capacities follow
f32 = np.float32


def grid_onsets(bpm, nb, keep=1.0, seed=0, jitter_s=0.0, sr=SR, first=0):
    """Ascending, distinct uint32 sample positions: slot k of nb at first + k * 60 / bpm seconds, kept
    with probability `keep`, moved by a uniform jitter of at most jitter_s seconds."""
    rng = np.random.default_rng(seed)
    pos = first + np.arange(nb, dtype=np.float64) * (60.0 / bpm) * sr
    kept = rng.random(nb) < keep
    jit = rng.uniform(-jitter_s, jitter_s, nb) * sr
    p = np.rint(pos + jit)[kept]
    return np.unique(np.clip(p, 0, 2**32 - 1).astype(np.uint32))


def track(onsets, bpm, conf=0.8, seconds=None, sr=SR):
    """The probe's input for a track whose trimmed signal ends one frame after its last onset (or
    lasts `seconds`): frames and n_trim as the base pass would have them."""
    on = np.asarray(onsets, dtype=np.uint32)
    n_trim = int(seconds * sr) if seconds is not None else (int(on[-1]) if on.size else 0) + FS
    n_trim = max(n_trim, FS)
    return dict(onsets=on, bpm=f32(bpm), conf=f32(conf), n_trim=n_trim, frames=(n_trim - FS) // HOP + 1)


def onsets_s(trk, sr=SR):
    """The onset times as k_beat and the reference form them: f32(sample) / f32(rate)."""
    return trk["onsets"].astype(f32) / f32(sr)


def hmm_frames(trk, sr=SR):
    """hmm_track's frame count (hmm.rs:139-147) in f32: ceil((last - first) / interval) + 1."""
    on = onsets_s(trk, sr)
    interval = f32(60.0) / f32(trk["bpm"])
    return int(np.ceil(f32(f32(on[-1] - on[0]) / interval))) + 1


def reference(trk, sr=SR):
    """What the analysis computes from these onsets (src/lib.rs:913-957): None where it leaves the
    grid empty (fewer than two onsets, a tempo that is not positive, generate_beat_grid's Err), else
    units.beat_grid_diag's record."""
    if not (trk["bpm"] > 0 and trk["onsets"].size >= 2):
        return None
    return units.beat_grid_diag(float(trk["bpm"]), float(trk["conf"]), onsets_s(trk, sr), sr)


def hmm_beats(trk, sr=SR):
    return oracle.hmm_track(float(trk["bpm"]), onsets_s(trk, sr))


def positive_intervals(beats):
    return int(np.count_nonzero(np.diff(np.asarray(beats, f32)) > 0))


def _span(trk):
    hb = hmm_beats(trk)
    return float(hb[-1] - hb[0])


def _g(bpm, nb, keep=1.0, seed=0, jitter_s=0.0, est=None, conf=0.8, seconds=None):
    return track(grid_onsets(bpm, nb, keep, seed, jitter_s), bpm if est is None else est, conf, seconds)


def _refined_in(lo, hi):
    return lambda t, r: r is not None and r["variable"] and r["refined"] and lo <= len(r["beats"]) <= hi


def _var_ref(t, r):
    return r is not None and r["variable"] and r["refined"]


def _frames(n):
    return lambda t, r: r is not None and hmm_frames(t) == n


def _every_frame(bpm, keep, seed):
    """An onset on every base-pass frame of a 60 s track."""
    F = (60 * SR - FS) // HOP + 1
    rng = np.random.default_rng(seed)
    on = (np.arange(1, F, dtype=np.uint32) * HOP)[rng.random(F - 1) < keep]
    return track(on, bpm, seconds=60)


# name -> (track, condition(track, reference) that must hold for the case to reach its branch)
def build_cases():
    c = {}
    nan = float("nan")
    reg = grid_onsets(120, 40)
    # gates (src/lib.rs:913; generate_beat_grid's InvalidInput above 300 BPM)
    for name, bpm in (("bpm_0", 0.0), ("bpm_neg", -1.0), ("bpm_nan", nan), ("bpm_300_5", 300.5)):
        c["gate_" + name] = (track(reg, bpm), lambda t, r: r is None)
    c["gate_bpm_300"] = (_g(300, 40), lambda t, r: r is not None and len(r["beats"]) == 40)
    for n in (0, 1, 2):
        c[f"gate_n_{n}"] = (track(reg[:n], 120, seconds=10), (lambda n: lambda t, r: (r is None) == (n < 2))(n))
    # hmm_track's ballot compaction and the LDS / scratch choice of its output
    for nf in (63, 64, 65, 128, 129):
        c[f"hmm_frames_{nf}"] = (_g(120, nf), _frames(nf))
    for nf in (2048, 2049):
        c[f"hmm_frames_{nf}"] = (_g(300, nf), _frames(nf))
    for n in (4096, 4097):
        c[f"onsets_{n}"] = (_g(300, n), (lambda n: lambda t, r: r is not None and t["onsets"].size == n)(n))
    # seg_init
    c["seg_lt4_hmm_beats"] = (_g(120, 3), lambda t, r: r is not None and r["hmm_beats"] < 4)
    c["seg_span_lt_2s"] = (_g(240, 7), lambda t, r: r is not None and r["hmm_beats"] >= 4 and _span(t) < 2.0)
    for name, bpm, nb, seed, lo, hi in SPANS:
        c["seg_span_" + name] = (_g(bpm, nb, 0.8, seed),
                                 (lambda lo, hi: lambda t, r: r is not None and r["hmm_beats"] >= 4 and r["variable"] and
                                  lo < _span(t) < hi)(lo, hi))
    # tempo variation and the Bayesian update's candidate counts (0 below 55 and above 185 BPM)
    for bpm, seed in VARIATION:
        c[f"var_bpm_{bpm}"] = (_g(bpm, 40, 0.6, seed), _var_ref)
    bpm, nb, keep, seed, jit = WORST_LIKELIHOOD
    c["bayes_worst_likelihood"] = (_g(bpm, nb, keep, seed, jit), _var_ref)
    # the refined-beat sort: bitonic in LDS up to 2048 slots, else the single-lane merge sort
    for name, bpm, nb, keep, seed, jit, lo, hi in SORTS:
        c["sort_" + name] = (_g(bpm, nb, keep, seed, jit), _refined_in(lo, hi))
    # time signature
    c["ts_lt8_beats"] = (_g(120, 6), lambda t, r: r is not None and 1 <= len(r["beats"]) < 8)
    c["ts_regular_6_8"] = (_g(120, 40), lambda t, r: r is not None and not r["variable"] and r["beats_per_bar"] == 6)
    bpm, nb, keep, seed = FEW_INTERVALS
    c["ts_few_positive_intervals"] = (_g(bpm, nb, keep, seed),
                                      lambda t, r: _var_ref(t, r) and len(r["beats"]) >= 8 and
                                      positive_intervals(r["beats"]) < 6)
    # capacity: max(12 dur + 64, 3 F + 8) must hold what an onset on every frame produces
    c["cap_every_frame_300"] = (_every_frame(300, 1.0, 0), lambda t, r: r is not None and t["onsets"].size == t["frames"] - 1)
    c["cap_every_frame_180"] = (_every_frame(180, 0.7, CAP_SEED), lambda t, r: r is not None)
    return c


# (name, bpm, slots, seed, span window in seconds) at keep = 0.8: seg_dur = clamp(span / 4, 4, 8)
SPANS = (("15_9", 200, 54, 0, 15.8, 16.0), ("16_1", 200, 55, 0, 16.0, 16.3), ("31_9", 200, 107, 0, 31.7, 32.0),
         ("32_1", 200, 108, 1, 32.0, 32.3))
VARIATION = ((50, 0), (54.9, 0), (58, 0), (120, 0), (178, 0), (185.5, 0), (200, 0), (300, 0))
# (name, bpm, slots, keep, seed, jitter, refined-count range)
SORTS = (("1_8", 60, 6, 0.6, 1, 0.0, 1, 8), ("le_64", 120, 40, 0.6, 1, 0.0, 49, 64), ("gt_64", 120, 50, 0.6, 8, 0.0, 65, 80),
         ("2000_2048", 180, 1450, 0.7, 1, 0.010, 2000, 2048), ("2049_2400", 180, 1700, 0.7, 0, 0.010, 2049, 2400))
FEW_INTERVALS = (120, 12, 0.6, 7)
CAP_SEED = 0
# Onsets up to a quarter of a second off a 120 BPM grid: the smallest likelihoods the Bayesian update
# can see.  An onset lies at most half a candidate interval (0.5 s at 60 BPM) from the candidate's
# grid, so the mean log-likelihood is at least -0.25 / 0.005 = -50 and exp(-50) = 1.9e-22 is a
# normal f32: no onset list makes every likelihood underflow to 0.  The tracker keeps its tempo only
# where it has no candidate (below 55 and above 185 BPM: var_bpm_50, 54.9, 185.5, 200, 300).
WORST_LIKELIHOOD = (120, 60, 0.9, 3, 0.25)

_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
    return _CASES
