"""tests/sections_ref.py on the CPU: the cell plan against a brute-force count of the frames per
cell, the degenerate inputs of the definition (a constant track, equal peaks, too few cells), the
request checks, and the behavioural case: three cadence parts of 16 s (C major loud, F sharp major
quiet, C major loud) must give exactly two boundaries, each within one cell of 16 s and 32 s, from
the oracle's own chroma rows and spectrogram."""
import numpy as np
import pytest

import key_timeline_ref as K
import oracle
import sections_ref as S

f32 = np.float32
SR = 44100


@pytest.mark.parametrize("Cs,khop,hop", [(512, 512, 512), (1024, 512, 512), (22050, 512, 512), (22050, 256, 512),
                                         (700, 256, 512), (513, 512, 512), (44100, 512, 1024)])
def test_plan_against_brute_force(Cs, khop, hop):
    for F, Fb in ((0, 0), (1, 1), (43, 44), (300, 151), (1000, 1000), (5171, 2580)):
        n = S.n_cells(F, khop, Fb, hop, Cs)
        assert n == min(F * khop, Fb * hop) // Cs
        for h, frames in ((khop, F), (hop, Fb)):
            owner = [f * h // Cs for f in range(frames)]  # the cell whose span holds the frame's start
            for c in range(n):
                f0, f1 = S.first_frame(c, Cs, h), S.first_frame(c + 1, Cs, h)
                want = [f for f in range(frames) if owner[f] == c]
                assert want and want == list(range(f0, f1)), (F, Fb, c, f0, f1, want[:3])
    assert S.plan(dict(cell_samples=Cs), SR, khop, hop) == Cs


def test_uneven_cells_of_43_and_44_frames():
    counts = {S.first_frame(c + 1, 22050, 512) - S.first_frame(c, 22050, 512) for c in range(200)}
    assert counts == {43, 44}


def test_request_checks():
    ok = dict(cell_seconds=0.5)
    assert S.plan(ok, SR, 512, 512) == 22050
    bad = [dict(), dict(cell_seconds=0.5, cell_samples=22050), dict(cell_seconds=float("nan")), dict(cell_seconds=-0.5),
           dict(ok, energy_weight=float("inf")), dict(ok, min_strength=-1.0), dict(ok, snap_seconds=float("nan")),
           dict(ok, what=0), dict(ok, what=4), dict(ok, kernel_cells=0), dict(ok, kernel_cells=65),
           dict(ok, min_gap_cells=2 ** 31), dict(cell_samples=511), dict(cell_samples=2 ** 31), dict(cell_seconds=1e9)]
    for r in bad:
        assert S.plan(r, SR, 512, 512)[0] == 1, r
    assert S.plan(dict(cell_samples=600), SR, 256, 1024)[0] == 1  # shorter than the base hop
    assert S.plan(ok, SR, 512, 512, stages_full=False)[0] == 1
    assert S.plan(ok, SR, 512, 512, legacy=True)[0] == 4 and S.plan(ok, SR, 512, 512, beat_rows=True)[0] == 4
    assert S.plan(dict(ok, min_gap_cells=2 ** 31 - 1, kernel_cells=64), SR, 512, 512) == 22050


def test_constant_track_has_no_novelty_and_one_section():
    rows = np.tile((np.arange(12, dtype=f32) / 7).astype(f32), (400, 1))
    E = np.full(400, 3.25, f32)
    for K_ in (1, 2, 16):
        r = S.sections(rows, E, dict(cell_samples=1024, kernel_cells=K_, min_gap_cells=2), SR, 512, 512)
        assert r["n_cells"] == 200 and not r["novelty"].any() and r["nmax"] == 0
        assert r["n_sections"] == 1 and r["sections"]["end_cell"].tolist() == [200]
        assert r["sections"]["relative_energy"].tolist() == [1.0] and r["sections"]["strength"].tolist() == [0.0]


def test_too_few_cells_and_no_cells():
    rng = np.random.default_rng(1)
    rows, E = rng.random((31, 12), dtype=f32), rng.random(31, dtype=f32)
    r = S.sections(rows, E, dict(cell_samples=512, kernel_cells=16), SR, 512, 512)
    assert r["n_cells"] == 31 and not r["novelty"].any() and r["n_sections"] == 1
    r = S.sections(rows[:0], E[:0], dict(cell_samples=512, kernel_cells=16), SR, 512, 512)
    assert r["n_cells"] == 0 and r["n_sections"] == 0 and r["gmax"] == 0 and r["nmax"] == 0
    r = S.sections(rows, E * 0, dict(cell_samples=512, kernel_cells=2), SR, 512, 512)  # gmax 0: e is 0, no division
    assert r["gmax"] == 0 and np.isfinite(r["novelty"]).all() and r["novelty"].any()
    assert not r["sections"]["relative_energy"].any()


def test_first_of_two_equal_peaks_wins():
    # zero rows and energies 0, 1, 0, 1, ...: at K = 1 every N[c] = D(c - 1, c) = 1, a plateau
    rows, E = np.zeros((40, 12), f32), (np.arange(40) % 2).astype(f32)
    c = S.cells_ref(rows, E, dict(cell_samples=512, kernel_cells=1, min_gap_cells=8), SR, 512, 512)
    assert c["novelty"].tolist() == [0.0] + [1.0] * 39
    # (the rule compares with neighbours, not with chosen boundaries: every later cell has an equal one before it)
    assert np.flatnonzero(c["boundary"]).tolist() == [1]
    c = S.cells_ref(rows, E, dict(cell_samples=512, kernel_cells=1, min_gap_cells=0), SR, 512, 512)
    assert np.flatnonzero(c["boundary"]).tolist() == list(range(1, 40))
    # two equal isolated peaks 3 cells apart, G = 8: only the first
    N = np.zeros(30, f32)
    N[[10, 13]] = 2.0
    assert np.flatnonzero(S.boundaries(N, 8, 0.5)).tolist() == [10]
    assert np.flatnonzero(S.boundaries(N, 2, 0.5)).tolist() == [10, 13]
    N[20] = 0.9  # below min_strength * Nmax
    assert np.flatnonzero(S.boundaries(N, 2, 0.5)).tolist() == [10, 13]
    assert np.flatnonzero(S.boundaries(N, 2, 0.25)).tolist() == [10, 13, 20]


def test_snap_takes_the_nearest_downbeat_the_first_on_a_tie():
    downs = np.array([0.5, 2.0, 4.0, 6.0], f32)
    assert S.snap(downs, f32(3.0), 1.5) == (1, f32(2.0))
    assert S.snap(downs, f32(3.0), 0.5) == (-1, f32(3.0))
    assert S.snap(downs, f32(5.9), 0.25) == (3, f32(6.0))
    assert S.snap(np.zeros(0, f32), f32(1.0), 9.0) == (-1, f32(1.0))


def behavioural_track():
    return np.concatenate([K.cadence(0, 16.0, SR, level=0.2), K.cadence(6, 16.0, SR, level=0.05),
                           K.cadence(0, 16.0, SR, level=0.2)])


BEHAVIOURAL_REQUEST = dict(cell_seconds=0.5, kernel_cells=8, min_gap_cells=8, energy_weight=1.0, min_strength=0.5)


def test_behavioural_case_two_boundaries_at_16_and_32_seconds():
    cfg = oracle.default_config()
    x = behavioural_track()
    chain = S.track_inputs(x, SR, cfg)
    assert chain[0] == 0
    r = S.sections_ref(x, SR, cfg, BEHAVIOURAL_REQUEST, chain=chain)
    first, Cs = r["first_sample"], r["cell_samples"]
    assert Cs == 22050 and r["n_sections"] == 3, (r["n_sections"], r["sections"]["start_cell"])
    starts = r["sections"]["start_cell"].tolist()
    for got, sec in zip(starts[1:], (16.0, 32.0)):
        want = (sec * SR - first) / Cs  # the part's start in cells after the trim start
        assert abs(got - want) <= 1.0, (starts, first, want)
    rel = r["sections"]["relative_energy"]
    assert rel[1] < 0.25 * min(rel[0], rel[2]) and rel.max() == 1.0  # a quarter of the level: a sixteenth of the energy
    assert (r["sections"]["strength"][1:] >= f32(0.5) * r["nmax"]).all()
