"""tests/tempo_map_ref.py against the oracle's whole beat grid (CPU only).

The reference of the tempo map request is composed from the oracle's units; here its reconstructed
beat list and branch record are pinned to units.beat_grid_diag (generate_beat_grid as a whole) on
every case of tests/beat_cases.py, its restated signature scores to units.detect_time_signature, and
the case set is shown, from the reference alone, to reach every branch the request reports.
"""
import numpy as np
import pytest

import beat_cases as B
import tempo_map_ref as R
import units

NAMES = list(B.cases())
_REFS = {}


def ref(name):
    if name not in _REFS:
        t = B.cases()[name][0]
        _REFS[name] = R.reference(t["onsets"], t["bpm"], t["conf"], B.SR)
    return _REFS[name]


@pytest.mark.parametrize("name", NAMES)
def test_reference_reconstructs_the_grid(name):
    t = B.cases()[name][0]
    diag, m = B.reference(t), ref(name)
    if diag is None:
        assert m["has_grid"] == 0 and m["n_segments"] == 0 and m["beats"].size == 0
        return
    assert m["has_grid"] == 1
    assert np.array_equal(R.bits(m["beats"]), R.bits(diag["beats"]))
    assert (m["refined"], m["has_variation"], m["beats_per_bar"], m["hmm_beats"]) == (
        int(diag["refined"]), int(diag["variable"]), diag["beats_per_bar"], diag["hmm_beats"])
    nb = m["segments"]["n_beats"]
    if m["refined"]:
        assert int(nb.sum()) == m["beats"].size
    if not m["has_variation"]:
        assert not nb.any() and not m["segments"]["updated"].any()
    # the restated scores give the oracle's pair by the last-maximum rule
    bpb, conf = units.detect_time_signature(m["beats"], float(t["bpm"]))
    assert (m["beats_per_bar"], R.bits(m["time_signature_confidence"])) == (bpb, R.bits(conf))
    if m["time_signature_scored"]:
        assert R.bits(m["time_signature_confidence"]) == R.bits(min(max(m["time_signature_scores"].max(), 0), 1))


def test_case_set_reaches_every_branch():
    n = dict(change=0, keep=0, conf_lt1=0, const_in_var=0, skipped=0, dup=0, bpb3=0, bpb4=0, bpb6=0, fallback=0,
             single05=0, single08=0, grids=0, var_refined=0, var_no_onsets=0)
    for name in NAMES:
        m = ref(name)
        if not m["has_grid"]:
            continue
        n["grids"] += 1
        s = m["segments"]
        carried = m["nominal_bpm"]
        for k in range(m["n_segments"]):
            if s["updated"][k]:
                n["change" if R.bits(s["updated_bpm"][k]) != R.bits(carried) else "keep"] += 1
                n["conf_lt1"] += bool(s["updated_confidence"][k] < 1)
                carried = s["updated_bpm"][k]
            elif m["has_variation"] and s["is_variable"][k]:
                n["var_no_onsets"] += 1
            elif m["has_variation"]:
                n["const_in_var"] += 1
        starts = R.window_starts(m["hmm"])
        if starts is not None and len(starts) > m["n_segments"]:
            n["skipped"] += 1
        n["var_refined"] += bool(m["has_variation"] and m["refined"])
        n["dup"] += bool(m["refined"] and np.any(np.diff(m["beats"]) == 0))
        if m["time_signature_scored"]:
            n["bpb%d" % m["beats_per_bar"]] += 1
        else:
            n["fallback"] += 1
        if m["n_segments"] == 1 and not s["is_variable"][0] and R.bits(s["bpm"][0]) == R.bits(m["nominal_bpm"]):
            c = float(s["confidence"][0])
            n["single05"] += c == 0.5
            n["single08"] += c == np.float32(0.8)
    print(n)
    for k in ("change", "keep", "conf_lt1", "const_in_var", "skipped", "dup", "bpb3", "bpb4", "bpb6", "fallback",
              "single05", "single08", "var_refined"):
        assert n[k] > 0, (k, n)
    assert n["grids"] >= 30
    # (no case reaches a variable segment without onsets, n["var_no_onsets"]: a variable window holds
    # three HMM beats, each within the emission tolerance of an onset)
