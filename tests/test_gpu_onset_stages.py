"""Stage-level parity of the onset kernels: k_energy_onsets, k_flux_onsets (spectral flux, HFC, HPSS;
block_select_kth and the ordered compaction) and k_consensus against the oracle's detectors' tails
and its consensus selection, as integer lists compared with ==.

No result field shows an onset list: the beat tracker keeps an HMM frame when an onset lies within
about 54 ms of it, so an onset a hop off, a peak dropped at a 256-thread chunk seam, a percentile
threshold one rank off or a cluster centre off by a few samples leave every result unchanged.  Here
the pipeline's own onset stage (sdsp_debug_onset_stages: the buffer layout and launches of an
analysis call after its frame RMS, fed per-frame curves) returns the energy, spectral, HFC, HPSS and
chosen lists of every track.  The reference runs the same curves through units.energy_onsets_from_rms,
units.peaks_over_percentile, units.hpss_onsets_from_energy and units.consensus_select, each pinned
to the whole detectors and the whole-track oracle in test_oracle_stage_wrappers.py; the last test
here feeds the probe the curves of two whole tracks and compares with the oracle's trace.

A curve here is usually given as its flux (the half-wave difference the detector thresholds): the
spectral-flux curve is the flux itself, the RMS, HFC and percussive-energy curves are built so that
their rectified differences are that flux exactly (small integers).  With hop 1 an onset of a peak
at flux index i is the sample i + 1, which places list entries at chosen samples for the consensus
cases.
"""
import numpy as np
import pytest

import oracle
import sdsp
import synth
import units

pytestmark = pytest.mark.gpu

f32 = np.float32
KINDS = ("energy", "spectral", "hfc", "hpss", "chosen")
FACTOR = oracle.libm("pow", [10.0], [-1.0])[0]  # the energy detector's 10^(-20/20) as the kernels form it


def _cfgs(**opts):
    c = sdsp.default_config()
    for k, v in opts.items():
        if k == "onset_consensus_weights":
            for i, w in enumerate(v):
                c.onset_consensus_weights[i] = w
        else:
            setattr(c, k, v)
    return c


def from_flux(flux):
    """A per-frame curve (len(flux) + 1 values) whose rectified differences are `flux` (non-negative
    integers below 2^20, so every value and difference is exact in f32): rises by the flux, falls by 1
    where the flux is 0."""
    fl = np.asarray(flux, np.int64)
    steps = np.where(fl > 0, fl, -1)
    c = np.concatenate([[0], np.cumsum(steps)])
    c = c - c.min() + 1
    assert c.max() < 2**23
    return c.astype(f32)


def flux_track(flux, n_trim=None, hop=512, hpss=True):
    """A track whose four detectors all see `flux` (an integer array)."""
    fl = np.asarray(flux, f32)
    c = from_flux(flux)
    F = c.size
    t = dict(rms=c, hfc=c, sfo=np.concatenate([fl, [0]]).astype(f32), n_trim=F * hop + 1 if n_trim is None else n_trim)
    if hpss:
        t["hpe"] = c
    return t


def raw_track(curve, n_trim=None, hop=512, hpss=True):
    """A track whose every curve is `curve` itself (the spectral detector thresholds it directly, the
    others its rectified differences)."""
    c = np.asarray(curve, f32)
    t = dict(rms=c, hfc=c, sfo=c, n_trim=c.size * hop + 1 if n_trim is None else n_trim)
    if hpss:
        t["hpe"] = c
    return t


def list_track(lists, hop=1, frames=None, n_trim=None):
    """A track whose energy, spectral, HFC and HPSS detectors (threshold percentile 0) give exactly
    `lists`: ascending sample positions, multiples of hop, at least two hops apart within a list."""
    top = max([int(l[-1]) // hop for l in lists if len(l)] + [2])
    F = (top + 2) if frames is None else frames
    fl = np.zeros((4, F - 1), np.int64)
    for k, l in enumerate(lists):
        idx = np.asarray(l, np.int64) // hop - 1
        assert np.all(np.asarray(l, np.int64) % hop == 0) and np.all(idx >= 0) and np.all(np.diff(idx) >= 2)
        fl[k, idx] = 1
    t = dict(rms=from_flux(fl[0]), sfo=np.concatenate([fl[1], [0]]).astype(f32), hfc=from_flux(fl[2]),
             hpe=from_flux(fl[3]), n_trim=F * hop + 1 if n_trim is None else n_trim)
    return t


def reference(trk, cfg, sr=44100, hop=512):
    """The five lists the analysis computes from these curves (src/lib.rs:152-291)."""
    rms, n = np.asarray(trk["rms"], f32), int(trk["n_trim"])
    F = rms.size
    pct = float(cfg.onset_threshold_percentile)
    energy = units.energy_onsets_from_rms(rms, hop, n)

    def samples(fn, *a):
        try:  # detect_*_onsets' Err (a percentile outside [0, 1]) is a warning and an empty list
            fr = fn(*a, pct)
        except units.AnalysisError:
            return []
        return sorted({f * hop for f in fr if f * hop < n})

    sfo = np.asarray(trk["sfo"], f32)[:F - 1]
    h = np.asarray(trk["hfc"], f32)
    spectral = samples(units.peaks_over_percentile, sfo)
    hfc = samples(units.peaks_over_percentile, np.maximum(h[1:] - h[:-1], f32(0)).astype(f32))
    hpss = []
    if cfg.enable_hpss_onsets and cfg.enable_onset_consensus and trk.get("hpe") is not None:
        hpss = samples(units.hpss_onsets_from_energy, np.asarray(trk["hpe"], f32))
    chosen = energy
    if cfg.enable_onset_consensus:
        chosen = units.consensus_select([energy, spectral, hfc, hpss], list(cfg.onset_consensus_weights),
                                        int(cfg.onset_consensus_tolerance_ms), sr)
    return dict(energy=energy, spectral=spectral, hfc=hfc, hpss=hpss, chosen=chosen)


def run(tracks, cfg=None, sr=44100, hop=512, names=None):
    """Probe and reference over `tracks`; every list of every track must be equal.  Returns both."""
    cfg = cfg if cfg is not None else _cfgs(enable_hpss_onsets=1)
    got = sdsp.debug_onset_stages(tracks, sr, hop, cfg)
    refs = [reference(t, cfg, sr, hop) for t in tracks]
    for i, (g, r) in enumerate(zip(got, refs)):
        for k in KINDS:
            assert g[k].tolist() == r[k], (names[i] if names else i, k, _first_diff(g[k].tolist(), r[k]))
    return got, refs


def _first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"lengths {len(a)} / {len(b)}, first difference at {i}: {x} vs {y}"
    return f"lengths {len(a)} / {len(b)}, equal up to the shorter"


def _random_flux(seed, L):
    """Integers with runs of equal values (plateaus) and about a third zeros."""
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 50, L)
    v[rng.random(L) < 0.35] = 0
    return np.repeat(v, rng.integers(1, 4, L))[:L]


# ---- curve lengths -------------------------------------------------------------------------------
LENGTHS = [1, 2, 3, 255, 256, 257, 511, 512, 513, 1025]


def test_curve_lengths_ragged_and_single():
    """L = F - 1 around k_energy_onsets' / k_flux_onsets' 256-thread chunks, in one ragged call and one
    track per call; L = 1 gives no onset (the reference's L > 1)."""
    tracks = [flux_track(_random_flux(L, L)) for L in LENGTHS]
    got, refs = run(tracks, names=LENGTHS)
    assert all(len(refs[0][k]) == 0 for k in KINDS)
    assert all(len(r["spectral"]) > 0 and len(r["energy"]) > 0 for r in refs[3:])
    for i, t in enumerate(tracks):
        one, _ = run([t], names=[LENGTHS[i]])
        for k in KINDS:
            assert one[0][k].tolist() == got[i][k].tolist(), (LENGTHS[i], k)


def test_single_frame_track():
    """F = 1: no flux at all; between other tracks its slots stay empty."""
    tracks = [flux_track(_random_flux(7, 40)), raw_track([3.0]), flux_track(_random_flux(8, 40))]
    _, refs = run(tracks)
    assert all(refs[1][k] == [] for k in KINDS)


# ---- peak rules ----------------------------------------------------------------------------------
def _pad(flux, L, at=0):
    out = np.zeros(L, np.int64)
    out[at:at + len(flux)] = flux
    return out


def test_peak_rules():
    """Plateaus keep their first index only; index 0 may equal its successor; index L - 1 must exceed
    its predecessor; a value equal to the percentile threshold is no peak; peaks on either side of the
    chunk seams at 256 and 512."""
    c0 = _cfgs(enable_hpss_onsets=1, onset_threshold_percentile=0.0)
    cases = {
        "plateau2": [0, 1, 3, 3, 1, 0, 2, 0],
        "plateau3": [0, 2, 2, 2, 0, 1, 0],
        "first_equals_second": [5, 5, 1, 0, 2, 0],
        "first_below_second": [4, 5, 1, 0, 2, 0],
        "last_equals_predecessor": [0, 2, 0, 1, 4, 4],
        "last_above_predecessor": [0, 2, 0, 1, 4, 5],
        "two_values": [3, 3],
        "two_values_rising": [0, 3],
    }
    for at in (254, 255, 256, 510, 511, 512):
        cases[f"peak_at_{at}"] = _pad([0, 7, 0], 600, at - 1)
        cases[f"plateau_from_{at}"] = _pad([0, 7, 7, 0], 600, at - 1)
    names = list(cases)
    _, refs = run([flux_track(cases[k]) for k in names], c0, names=names)
    r = dict(zip(names, refs))
    for k in ("energy", "spectral", "hfc", "hpss"):
        assert r["plateau2"][k] == [3 * 512, 7 * 512] and r["plateau3"][k] == [2 * 512, 6 * 512], k
        assert r["first_equals_second"][k][0] == 512 and r["first_below_second"][k][0] == 2 * 512, k
        assert r["last_equals_predecessor"][k][-1] == 5 * 512 and r["last_above_predecessor"][k][-1] == 6 * 512, k
        # two equal values: above the energy threshold (a tenth of the maximum), not above their own minimum
        assert r["two_values"][k] == ([512] if k == "energy" else []) and r["two_values_rising"][k] == [2 * 512], k
        for at in (254, 255, 256, 510, 511, 512):
            assert r[f"peak_at_{at}"][k] == [(at + 1) * 512] and r[f"plateau_from_{at}"][k] == [(at + 1) * 512], (k, at)


def test_peak_equal_to_percentile_threshold():
    """Of ten values the one of rank 8 (percentile 0.8) is the threshold: peaks of that value are
    dropped, larger ones kept."""
    flux = [0, 6, 0, 6, 0, 9, 0, 0, 0, 0]  # sorted: seven 0, 6, 6, 9 -> threshold 6
    _, refs = run([flux_track(flux)], _cfgs(enable_hpss_onsets=1))
    for k in ("spectral", "hfc", "hpss"):
        assert refs[0][k] == [6 * 512], k


def test_trim_removes_last_peaks():
    """An onset at sample s is kept only below n_trim: n_trim = s drops it, n_trim = s + 1 keeps it."""
    flux = _pad([0, 5, 0, 4, 0, 6, 0], 300, 290)  # peaks at 291, 293, 295 -> samples 292, 294, 296 hops
    s = 296 * 512
    tracks = [flux_track(flux, n_trim=n) for n in (s + 1, s, s - 1, 294 * 512 + 1, 294 * 512, 512, 1, 0)]
    _, refs = run(tracks, _cfgs(enable_hpss_onsets=1, onset_threshold_percentile=0.0))
    assert [len(r["spectral"]) for r in refs] == [3, 2, 2, 2, 1, 0, 0, 0]
    assert [len(r["energy"]) for r in refs] == [3, 2, 2, 2, 1, 0, 0, 0]


# ---- energy --------------------------------------------------------------------------------------
def test_energy_threshold():
    """All-equal RMS has no flux above EPS and no onset; a flux exactly at max * 10^(-20/20) is not
    above the threshold, the next larger one is."""
    thr = f32(1000) * FACTOR
    assert thr == f32(100)
    flat = raw_track(np.full(300, 0.25, f32))
    tiny = raw_track(np.tile(np.array([0, 1e-12], f32), 150))  # max flux <= EPS
    at = flux_track([0, 1000, 0, 100, 0, 101, 0, 99, 0])
    _, refs = run([flat, tiny, at])
    assert refs[0]["energy"] == [] and refs[1]["energy"] == []
    assert refs[2]["energy"] == [2 * 512, 6 * 512]


# ---- radix select --------------------------------------------------------------------------------
def _select_curves():
    rng = np.random.default_rng(5)
    half = rng.random(700, dtype=f32)
    half[rng.random(700) < 0.5] = 0
    den = (rng.integers(1, 1 << 22, 600).astype(np.uint32)).view(f32)  # denormals
    den_mix = den.copy()
    den_mix[::3] = 0
    top24 = (np.uint32(0x3F800000) + rng.integers(0, 256, 900).astype(np.uint32)).view(f32)
    both = np.concatenate([top24[:300], den[:300], half[:300]])
    return {
        "zeros": np.zeros(400, f32),
        "half_zeros": half,
        "denormals": den,
        "denormals_and_zeros": den_mix,
        "top_24_bits_equal": top24,
        "copies_1000": np.full(1000, 0.37, f32),
        "copies_and_one_peak": np.concatenate([np.full(500, 0.37, f32), [0.5], np.full(499, 0.37, f32)]).astype(f32),
        "mixed_magnitudes": both,
        "random_1025": rng.random(1026, dtype=f32) ** 8,
    }


@pytest.mark.parametrize("pct", [0.0, 0.3, 0.8, 1.0, 1.5, float("nan")], ids=lambda p: f"pct_{p}")
def test_percentile_select(pct):
    """block_select_kth's threshold at rank min(trunc(L * p), L - 1) over curves whose radix digits
    collide, and the out-of-range percentiles (empty flux lists, still a consensus of the energy
    onsets)."""
    curves = _select_curves()
    names = list(curves)
    cfg = _cfgs(enable_hpss_onsets=1, onset_threshold_percentile=pct)
    _, refs = run([raw_track(curves[k]) for k in names], cfg, names=names)
    r = dict(zip(names, refs))
    if not 0.0 <= pct <= 1.0:  # also NaN
        for k in names:
            assert r[k]["spectral"] == r[k]["hfc"] == r[k]["hpss"] == [], k
        assert len(r["random_1025"]["energy"]) > 0 and len(r["random_1025"]["chosen"]) > 0
    elif pct < 1.0:
        assert len(r["random_1025"]["spectral"]) > 0 and len(r["denormals"]["spectral"]) > 0
        assert len(r["copies_and_one_peak"]["spectral"]) == (1 if pct < 0.999 else 0)


# ---- consensus -----------------------------------------------------------------------------------
TOL = 2205  # 50 ms at 44.1 kHz


def _cons_cfg(**o):
    return _cfgs(onset_threshold_percentile=0.0, **{"enable_hpss_onsets": 1, **o})


def test_consensus_clusters():
    e = []
    p = np.arange(300) * 46 + 20  # 300 entries, 46 samples apart
    cases = {
        "all_empty": [e, e, e, e],
        "sizes_0_1_300": [e, [5000], p, e],
        "sizes_300_0_1": [p, e, [40], [41 + 46]],
        "same_sample_in_all_four": [[100, 9000], [100, 9000], [100, 9000], [100, 9000]],
        "gap_exactly_tol": [[1000], [1000 + TOL], e, e],
        "gap_tol_plus_1": [[1000], [1000 + TOL + 1], e, e],
        "chain_of_tol_gaps": [[1000, 1000 + 4 * TOL], [1000 + TOL, 1000 + 5 * TOL], [1000 + 2 * TOL, 1000 + 6 * TOL],
                              [1000 + 3 * TOL, 1000 + 7 * TOL]],
        "only_single_method_clusters": [[100], [5000], [10000], [15000]],
        "single_then_strong": [[100, 9000], [9010], [20000], e],
        "adjacent_strong_clusters": [[3000, 3000 + TOL + 1], [3000, 3000 + TOL + 1], e, e],
        "uneven_mean": [[700], [701], [703, 20000], [20003]],  # centres by integer division
    }
    names = list(cases)
    tracks = [list_track(cases[k], frames=21000) for k in names]
    _, refs = run(tracks, _cons_cfg(), hop=1, names=names)
    r = dict(zip(names, refs))
    for k in names:  # the detectors return the lists the case is built from
        assert [r[k][d] for d in KINDS[:4]] == [list(map(int, l)) for l in cases[k]], k
    assert r["all_empty"]["chosen"] == []
    assert r["same_sample_in_all_four"]["chosen"] == [100, 9000]
    assert r["gap_exactly_tol"]["chosen"] == [1000 + TOL // 2]
    assert r["gap_tol_plus_1"]["chosen"] == [1000, 1000 + TOL + 1]  # no strong cluster: every centre
    assert len(r["chain_of_tol_gaps"]["chosen"]) == 1
    assert r["only_single_method_clusters"]["chosen"] == [100, 5000, 10000, 15000]
    assert r["single_then_strong"]["chosen"] == [9005]
    assert r["adjacent_strong_clusters"]["chosen"] == [3000, 3000 + TOL + 1]
    assert r["uneven_mean"]["chosen"] == [701, 20001]
    assert len(r["sizes_0_1_300"]["chosen"]) >= 1 and len(r["sizes_300_0_1"]["chosen"]) >= 1


def test_consensus_centre_above_2_pow_24():
    """A centre that f32 cannot hold: two onsets above 2^24 whose mean is odd."""
    hop, sr = 4097, 96000
    a, b = 4101 * hop, 4105 * hop
    assert a > 1 << 24 and (a + b) // 2 % 2 == 1 and int(f32((a + b) // 2)) != (a + b) // 2
    cfg = _cons_cfg(onset_consensus_tolerance_ms=200)
    assert b - a <= int(f32(200) / f32(1000) * f32(sr))
    _, refs = run([list_track([[a], [b], [], []], hop=hop, frames=4200)], cfg, sr=sr, hop=hop)
    assert refs[0]["chosen"] == [(a + b) // 2]


def _random_lists(seed, n=60, span=12000, spread=0):
    """Four lists around shared positions, each shifted by up to `spread` samples, with some entries
    dropped and some private ones added."""
    rng = np.random.default_rng(seed)
    base = np.sort(rng.choice(np.arange(10, span, 4), n, replace=False))
    out = []
    for k in range(4):
        p = base[rng.random(n) < 0.7]
        p = p + rng.integers(-spread, spread + 1, p.size)
        extra = rng.integers(10, span, 10)
        p = np.unique(np.clip(np.concatenate([p, extra]), 2, span))
        out.append(p[np.concatenate([[True], np.diff(p) >= 2])])
    return out


@pytest.mark.parametrize("sr", [22050, 44100, 96000])
@pytest.mark.parametrize("tol_ms", [1, 50])
def test_consensus_tolerances(sr, tol_ms):
    """tol = trunc(f32(ms) / 1000 * f32(rate)) samples over random lists whose spread straddles it."""
    tol = int(f32(tol_ms) / f32(1000) * f32(sr))
    n, span = (60, 12000) if tol_ms == 1 else (16, 30 * tol)  # mean gaps of a few tolerances
    tracks = [list_track(_random_lists(s, n, span, sp), frames=span + 100)
              for s, sp in ((1, tol // 2), (2, tol), (3, 2 * tol + 3))]
    _, refs = run(tracks, _cons_cfg(onset_consensus_tolerance_ms=tol_ms), sr=sr, hop=1)
    assert all(len(r["chosen"]) >= 3 for r in refs)


@pytest.mark.parametrize("opts", [
    dict(enable_hpss_onsets=0),
    dict(enable_hpss_onsets=1),
    dict(enable_onset_consensus=0),
    dict(enable_onset_consensus=0, enable_hpss_onsets=0),
    dict(onset_consensus_tolerance_ms=0),
    dict(onset_consensus_weights=(0.25, -1.0, 0.25, 0.25)),
    dict(onset_consensus_weights=(0.0, 0.0, 0.0, 0.0)),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_consensus_options(opts):
    """Three lists or four; consensus off, a zero tolerance and a negative weight keep the energy list."""
    cfg = _cons_cfg(**{"onset_consensus_tolerance_ms": 1, **opts})
    tracks = [list_track(_random_lists(s, spread=30), frames=12100) for s in (4, 5)]
    _, refs = run(tracks, cfg, hop=1)
    keeps_energy = (not opts.get("enable_onset_consensus", 1) or opts.get("onset_consensus_tolerance_ms", 1) == 0 or
                    min(opts.get("onset_consensus_weights", (0.25,))) < 0)
    for r in refs:
        assert (r["chosen"] == r["energy"]) == keeps_energy
        assert (len(r["hpss"]) > 0) == bool(cfg.enable_hpss_onsets and cfg.enable_onset_consensus)


def test_hpss_enabled_without_percussive_energy():
    """enable_hpss_onsets with no percussive energy (a pass without frames for HPSS): the HPSS lists
    are empty and the consensus runs over the other three."""
    t = list_track(_random_lists(6, spread=30), frames=12100)
    del t["hpe"]
    _, refs = run([t, t], _cons_cfg(onset_consensus_tolerance_ms=1), hop=1)
    assert refs[0]["hpss"] == [] and len(refs[0]["chosen"]) > 5


# ---- end to end ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 4])
def test_whole_track_curves_give_the_trace_lists(seed):
    """The probe over the frame RMS (sdsp_debug_frame_rms) and the SFO and full-band H of
    sdsp_debug_tempo_stages, taken over the oracle's STFT of the trimmed signal, gives the oracle
    trace's lists: the probe's index conventions are the whole-track pipeline's."""
    x, *_ = synth.make_track(seed, seconds=10.0)
    st, res, tr = oracle.analyze(x, 44100, trace=True)
    assert st == 0, res
    _, xn = oracle.normalize(x, 0, 44100)
    xt = np.ascontiguousarray(xn[tr["trim_start"]:tr["trim_end"]])
    mags = oracle.stft(xt, 2048, 512)
    rms = sdsp.debug_frame_rms([xt], [1.0], 2048, 512)
    assert rms.size == mags.shape[0]
    _, stages = sdsp.debug_tempo_stages([mags])
    trk = dict(rms=rms, hfc=stages[0]["H"][0], sfo=stages[0]["SFO"], n_trim=xt.size)
    got = sdsp.debug_onset_stages([trk], 44100, 512, sdsp.default_config())[0]
    for k in ("energy", "spectral", "hfc", "chosen"):
        assert len(tr[k + "_onsets"]) > 3, k
        assert got[k].tolist() == list(tr[k + "_onsets"]), (k, _first_diff(got[k].tolist(), list(tr[k + "_onsets"])))
    assert got["hpss"].size == 0
