"""Stage-level parity of the beat kernels: k_beat, k_beat_compact_w and k_beat_compact against the
oracle's generate_beat_grid, bit for bit, on onset lists that reach the branches the whole-track
tests cannot.

The pipeline's own beat stage (sdsp_debug_beat_grid: Pipeline::beat_grid and download_results with
their capacity formula, fed consensus onsets and a tempo estimate instead of an analysis) returns
every track's ok, beats, downbeats and stability; beats, downbeats and stability are compared on
their uint32 views with units.beat_grid_diag over f32(onset) / f32(rate).  Each case of
tests/beat_cases.py names the branch it is for and carries the condition, stated on the oracle's
own record, under which it reaches it (onsets or HMM beats past the LDS capacities, the ballot
compaction at 63 / 64 / 65 frames, seg_init's clamps, 0 / few / 21 Bayesian candidates, the bitonic
and the merge sort, the time-signature edges, the capacity formula); the condition is asserted
beside the comparison, so a case cannot pass without reaching its branch.  An ok of -1 (a list
outgrew its capacity) fails everywhere in this file.

One case of the plan cannot be built: an onset list whose every Bayesian likelihood underflows to 0.
An onset lies at most half a candidate interval (0.5 s at 60 BPM) from the candidate's grid, so the
likelihood is at least exp(-50) = 1.9e-22, a normal f32.  bayes_worst_likelihood takes the onsets as
far off the grid as they go instead, and the tracker keeping its tempo is reached where it has no
candidate (var_bpm_50, 54.9, 185.5, 200, 300).  The largest list is the 60 s capacity case's 5,163
onsets (one per frame).
"""
import numpy as np
import pytest

import beat_cases as B
import sdsp

pytestmark = pytest.mark.gpu

NAMES = list(B.cases())
_RAGGED = None


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ragged():
    """Every named case in one call (shared by the tests below)."""
    global _RAGGED
    if _RAGGED is None:
        _RAGGED = sdsp.debug_beat_grid([B.cases()[k][0] for k in NAMES], B.SR)
    return _RAGGED


def check(got, ref, what):
    """One track's probe output against the reference record (None: the grid stays empty)."""
    assert got["ok"] >= 0, (what, "a list outgrew its capacity")
    if ref is None:
        assert got["ok"] == 0 and got["beats"].size == 0 and got["downbeats"].size == 0, what
        assert _bits(got["stability"]) == 0, what
        return
    assert got["ok"] == 1, what
    for k in ("beats", "downbeats"):
        a, b = got[k], ref[k]
        assert a.size == b.size, (what, k, a.size, b.size)
        d = np.flatnonzero(_bits(a) != _bits(b))
        assert d.size == 0, (what, k, f"{d.size} of {a.size} differ, first at {d[0]}: {a[d[0]]!r} vs {b[d[0]]!r}")
    assert _bits(got["stability"]) == _bits(ref["stability"]), (what, got["stability"], ref["stability"])


def _same(a, b):
    return (a["ok"] == b["ok"] and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("beats", "downbeats")) and
            _bits(a["stability"]) == _bits(b["stability"]))


@pytest.mark.parametrize("name", NAMES)
def test_case_against_oracle(name):
    trk, cond = B.cases()[name]
    ref = B.reference(trk)
    assert cond(trk, ref), (name, "the oracle does not reach the branch this case is for")
    check(ragged()[NAMES.index(name)], ref, name)


def test_gates():
    """bpm in {0, -1, NaN, 300.5} and fewer than two onsets leave the grid empty with ok = 0
    (src/lib.rs:913 and generate_beat_grid's Err); bpm = 300 gives a grid."""
    got = dict(zip(NAMES, ragged()))
    for k in ("gate_bpm_0", "gate_bpm_neg", "gate_bpm_nan", "gate_bpm_300_5", "gate_n_0", "gate_n_1"):
        assert got[k]["ok"] == 0 and got[k]["beats"].size == 0, k
    assert got["gate_bpm_300"]["ok"] == 1 and got["gate_bpm_300"]["beats"].size == 40
    assert got["gate_n_2"]["ok"] == 1


def test_ragged_against_single():
    """The named cases in one call and each alone are bit-equal (on_off, beat_off and the scratch
    layout per track; the compaction prefix)."""
    for k, name in enumerate(NAMES):
        one = sdsp.debug_beat_grid([B.cases()[name][0]], B.SR)[0]
        assert _same(one, ragged()[k]), name


def test_capacity():
    """An onset on every frame of a 60 s track fits max(12 dur + 64, 3 F + 8)."""
    got = dict(zip(NAMES, ragged()))
    for k in ("cap_every_frame_300", "cap_every_frame_180"):
        trk = B.cases()[k][0]
        assert trk["onsets"].size > 3000
        assert got[k]["ok"] == 1, k
        check(got[k], B.reference(trk), k)


def test_refuses_list_longer_than_capacity():
    """More onsets than the consensus list of the track's frames can hold: SDSP_ERR_INVALID_INPUT."""
    trk = dict(B._g(300, 40))
    trk["frames"], trk["n_trim"] = 13, B.FS + 12 * B.HOP  # 3 x 13 = 39 slots
    with pytest.raises(sdsp.AnalysisError) as e:
        sdsp.debug_beat_grid([trk], B.SR)
    assert e.value.code == 1
    trk["onsets"] = trk["onsets"][:39]
    assert sdsp.debug_beat_grid([trk], B.SR)[0]["ok"] >= 0


def _cycle():
    """Eight short lists, some empty and some with fewer than two onsets."""
    c = B.cases()
    empty = B.track(np.zeros(0, np.uint32), 120, seconds=5)
    one = B.track(np.array([4410], np.uint32), 120, seconds=5)
    return [c["ts_regular_6_8"][0], empty, c["var_bpm_120"][0], one, c["sort_1_8"][0], c["gate_bpm_300_5"][0],
            c["ts_lt8_beats"][0], c["hmm_frames_65"][0]]


def test_compaction_kernels():
    """4,097 tracks in one call run k_beat_compact (one 1024-thread workgroup); the first 4,096 of
    them run k_beat_compact_w (one wave per track).  Per track both equal the oracle."""
    cyc = _cycle()
    refs = [B.reference(t) for t in cyc]
    assert sum(r is None for r in refs) == 3 and sum(r is not None and r["refined"] for r in refs) == 2
    tracks = [cyc[i % 8] for i in range(4097)]
    big = sdsp.debug_beat_grid(tracks, B.SR)
    small = sdsp.debug_beat_grid(tracks[:4096], B.SR)
    assert len(big) == 4097 and len(small) == 4096
    for i in range(8):  # every track against the oracle through its list's first occurrence
        check(big[i], refs[i], ("k_beat_compact", i))
        check(small[i], refs[i], ("k_beat_compact_w", i))
    for i in range(4097):
        assert _same(big[i], big[i % 8]), ("k_beat_compact", i)
    for i in range(4096):
        assert _same(small[i], big[i]), ("k_beat_compact_w", i)
