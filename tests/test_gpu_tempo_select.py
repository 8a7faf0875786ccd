"""Stage-level parity of k_tempo_select: candidate seeding and dedupe, weighted lookup scoring, the
consensus bonus, the octave fold, the bitonic sorts under equal keys and the ambiguity gate, against
the oracle's export of the same stage (units.tempo_select: tempogram_impl from its seeded variants on,
and analyze's gate), bit for bit.

The pipeline's own select launch (sdsp_debug_tempo_select: Pipeline::pass_select from its offset
tables on, with sel_params) runs over tempogram lists built directly (tests/tempo_select_cases.py).
Every float is compared on its uint32 view and every integer with ==; there is no tolerance.  That
each case reaches the branch or boundary it names is proved on the CPU, by the oracle's branch
record, in tests/test_tempo_decision_cases.py.
"""
import ctypes as C

import numpy as np
import pytest

import sdsp
import tempo_select_cases as S
import units

pytestmark = pytest.mark.gpu


def gpu_cfg(ocfg):
    """The binding's config with the oracle config's bytes (both mirror sdsp_config)."""
    c = sdsp.default_config()
    assert C.sizeof(c) == C.sizeof(ocfg)
    C.memmove(C.byref(c), C.byref(ocfg), C.sizeof(c))
    return c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(got, ref, g, trk, where):
    """One track's record and candidate table against the oracle's."""
    if not trk["active"] or ref is None:  # no novelty curve; "No BPM candidates could be scored"
        assert (got["ok"], got["n_cands"], got["agree"], got["ambiguous"], got["trap_low"], got["trap_high"]) == (0,) * 6, where
        assert _bits([got["bpm"], got["conf"]]).tolist() == [0, 0] and got["cands"].size == 0, where
        return
    assert got["ok"] == 1, where
    assert _bits([got["bpm"], got["conf"]]).tolist() == _bits([ref["bpm"], ref["conf"]]).tolist(), (where, got, ref["bpm"], ref["conf"])
    assert got["agree"] == ref["agree"], where
    n = min(len(ref["cands"]), g["top_n"], g["cand_cap"])
    assert got["n_cands"] == n, (where, got["n_cands"], n)
    assert np.array_equal(_bits(got["cands"]), _bits(ref["cands"][:n])), (where, got["cands"][:4], ref["cands"][:4])
    flags = (ref["ambiguous"], ref["trap_low"], ref["trap_high"]) if g["gate"] else (0, 0, 0)
    assert (got["ambiguous"], got["trap_low"], got["trap_high"]) == flags, (where, flags)


@pytest.fixture(scope="module")
def table():
    return S.build()


def _oracle(g, trk):
    cfg = g["cfg"]
    return units.tempo_select(S.variants(cfg, g["present"], trk), cfg.min_bpm, cfg.max_bpm, cfg.bpm_resolution, cfg)


def _call(g, tracks):
    return sdsp.debug_tempo_select(tracks, present=g["present"], top_n=g["top_n"], cand_cap=g["cand_cap"], gate=g["gate"],
                                   config=gpu_cfg(g["cfg"]))


def test_every_case_ragged_and_alone(table):
    """One ragged call per group of cases (a configuration and the pass's parameters), and every case
    in a call of its own: both equal the oracle, so they equal each other."""
    for gname, g in table.items():
        tracks = [t for _, t, _ in g["cases"]]
        refs = [_oracle(g, t) for t in tracks]
        got = _call(g, tracks)
        for (name, trk, _), r, o in zip(g["cases"], got, refs):
            check(r, o, g, trk, (gname, name, "ragged"))
        if len(tracks) > 1:
            for (name, trk, _), o in zip(g["cases"], refs):
                check(_call(g, [trk])[0], o, g, trk, (gname, name, "alone"))


def test_gate_off_leaves_the_flags_zero(table):
    g = dict(table["default"], gate=False)
    tracks = [t for _, t, _ in g["cases"]]
    for (name, trk, _), r in zip(g["cases"], _call(g, tracks)):
        check(r, _oracle(g, trk), g, trk, ("gate off", name))


def test_bad_capacity_is_refused(table):
    g = table["default"]
    trk = g["cases"][0][1]
    for kw in (dict(cand_cap=0), dict(cand_cap=1025)):
        with pytest.raises(sdsp.AnalysisError):
            sdsp.debug_tempo_select([trk], present=g["present"], top_n=10, config=gpu_cfg(g["cfg"]), **kw)
    with pytest.raises(sdsp.AnalysisError):  # the full variant is always present
        sdsp.debug_tempo_select([trk], present=(0, 1, 1, 1, 1), config=gpu_cfg(g["cfg"]))


def _spec(seed, frames, bins=1025):
    rng = np.random.default_rng(seed)
    return (rng.random((frames, bins), dtype=np.float32) ** 4 * np.float32(50)).astype(np.float32)


@pytest.mark.parametrize("seed,frames", [(3, 200), (4, 331)])
def test_chain_from_the_tempo_stage_probe(seed, frames):
    """The lists out of sdsp_debug_tempo_stages, fed to sdsp_debug_tempo_select, give the estimate
    tempogram_impl makes of the same spectrogram."""
    import oracle

    m = _spec(seed, frames)
    ocfg = oracle.default_config()
    meta, (st,) = sdsp.debug_tempo_stages([m], 44100, 512, gpu_cfg(ocfg))
    units.tempo_stages(m, 44100, 512, ocfg)
    est = units.tempo_stages_estimate()
    trk = dict(fft=st["fft"], acf=st["acf"])
    got = sdsp.debug_tempo_select([trk], present=meta["present"], top_n=25, cand_cap=25, gate=True, config=gpu_cfg(ocfg))[0]
    assert got["ok"] == 1 and est[0] > 0
    assert _bits([got["bpm"], got["conf"]]).tolist() == _bits(est[:2]).tolist() and got["agree"] == est[2]
