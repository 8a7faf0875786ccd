"""The oracle exports the onset and beat stage tests compare the kernels with (oracle/units.py:
energy_onsets_from_rms, peaks_over_percentile, hpss_onsets_from_energy, consensus_select,
beat_grid_diag), pinned to the whole functions and to the whole-track oracle.  CPU only.

The detectors' tails are compared with the detectors themselves on inputs whose curve is exact in
f32 (frames of one sample: RMS = |x|; two bins: HFC = the second bin squared; one bin: percussive
energy = its square).  consensus_select and beat_grid_diag are run on the trace lists of two short
synthetic tracks and must give the trace's chosen onsets and the result's beat grid.  Every case of
tests/beat_cases.py must meet its branch condition on the oracle alone.
"""
import numpy as np
import pytest

import beat_cases as B
import oracle
import synth
import units

f32 = np.float32
_cache = {}


def _track(seed):
    if seed not in _cache:
        x, *_ = synth.make_track(seed, seconds=10.0)
        st, r, tr = oracle.analyze(x, 44100, trace=True)
        assert st == 0, r
        _cache[seed] = (r, tr)
    return _cache[seed]


def _curve(seed, n):
    rng = np.random.default_rng(seed)
    c = rng.random(n, dtype=f32)
    c[rng.random(n) < 0.3] = 0  # runs of equal values: plateaus and zero flux
    return np.repeat(c, rng.integers(1, 3, n))[:n].astype(f32)


@pytest.mark.parametrize("n", [2, 3, 4, 17, 300])
def test_energy_tail_is_the_detector(n):
    x = _curve(n, n)
    assert units.energy_onsets_from_rms(np.abs(x), 1, n) == units.detect_energy_flux_onsets(x, 1, 1, -20.0)
    assert units.energy_onsets_from_rms(np.abs(x), 1, n // 2) == [o for o in units.energy_onsets_from_rms(np.abs(x), 1, n)
                                                                    if o < n // 2]


@pytest.mark.parametrize("pct", [0.0, 0.3, 0.8, 1.0])
@pytest.mark.parametrize("n", [2, 3, 17, 300])
def test_percentile_tails_are_the_detectors(n, pct):
    h = _curve(100 + n, n)
    flux = np.maximum(np.diff(h * h), 0).astype(f32)
    spec = np.stack([np.ones(n, f32), h], axis=1)
    assert units.peaks_over_percentile(flux, pct) == units.detect_hfc_onsets(spec, 44100, pct)
    assert units.hpss_onsets_from_energy(h * h, pct) == oracle.hpss_onsets(h.reshape(n, 1), pct)


def test_percentile_out_of_range_is_err():
    for pct in (1.5, -0.1, float("nan")):
        with pytest.raises(units.AnalysisError):
            units.peaks_over_percentile([0, 1, 0], pct)
        with pytest.raises(units.AnalysisError):
            units.hpss_onsets_from_energy([0, 1, 0], pct)
    assert units.peaks_over_percentile([], 0.5) == [] and units.hpss_onsets_from_energy([1.0], 0.5) == []


def test_peak_rules():
    # plateaus keep their first index; the first value may equal its successor, the last must exceed
    # its predecessor; a value equal to the threshold is no peak
    assert units.peaks_over_percentile([0, 2, 2, 0, 3, 3, 3, 0], 0.0) == [2, 5]
    assert units.peaks_over_percentile([2, 2, 0, 1, 1], 0.0) == [1, 4]
    assert units.peaks_over_percentile([0, 1, 0, 2, 0], 0.9) == []  # threshold = the maximum
    assert units.peaks_over_percentile([5], 0.0) == []  # L > 1


@pytest.mark.parametrize("seed", [3, 4])
def test_consensus_select_on_trace_lists(seed):
    r, tr = _track(seed)
    c = oracle.default_config()
    lists = [tr["energy_onsets"], tr["spectral_onsets"], tr["hfc_onsets"], []]
    assert len(lists[0]) and len(lists[1]) and len(lists[2])
    got = units.consensus_select(lists, list(c.onset_consensus_weights), int(c.onset_consensus_tolerance_ms), 44100)
    assert got == list(tr["chosen_onsets"])
    # the fallbacks: a zero tolerance and a negative weight keep the energy list
    assert units.consensus_select(lists, list(c.onset_consensus_weights), 0, 44100) == list(lists[0])
    assert units.consensus_select(lists, [0.25, -1.0, 0.25, 0.25], 50, 44100) == list(lists[0])
    assert units.consensus_select([[], [], [], []], [0.25] * 4, 50, 44100) == []


@pytest.mark.parametrize("seed", [3, 4])
def test_beat_grid_diag_on_trace_lists(seed):
    r, tr = _track(seed)
    on = np.asarray(tr["chosen_onsets"], np.uint32).astype(f32) / f32(44100)
    g = units.beat_grid_diag(r["bpm"], r["bpm_confidence"], on, 44100)
    assert g is not None and g["hmm_beats"] > 0
    assert np.array_equal(g["beats"], np.asarray(r["beat_grid"]["beats"], f32))
    assert np.array_equal(g["downbeats"], np.asarray(r["beat_grid"]["downbeats"], f32))
    assert g["stability"] == f32(r["grid_stability"])
    assert (g["variable"], g["refined"], g["beats_per_bar"]) == (bool(tr["beat_variable"]), bool(tr["beat_refined"]),
                                                                tr["beats_per_bar"])
    if not g["refined"]:
        assert g["hmm_beats"] == len(g["beats"])
    assert units.beat_grid_diag(300.5, 0.8, on, 44100) is None


@pytest.mark.parametrize("name", list(B.cases()))
def test_beat_case_reaches_its_branch(name):
    trk, cond = B.cases()[name]
    assert cond(trk, B.reference(trk)), name
