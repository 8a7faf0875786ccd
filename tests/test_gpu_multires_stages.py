"""Stage-level parity of k_multires: the hypothesis loop with its structural discounts, band
penalties, margin and prior, the dedupe, fold-down, fold-up and the triplet family with the wave-wide
beat contrast staged through LDS in segments, and the acceptance, against the oracle's export of the
same stage (units.multires_fuse: multi_resolution from its hypothesis loop on, and analyze's
acceptance), bit for bit.

The pipeline's own fusion launch (sdsp_debug_multires: the tail of Pipeline::escalate, with
mr_params, the count tables and the hop-512 list stride of an analysis call) runs over candidate
lists, novelty curves and base estimates built directly (tests/multires_cases.py).  Every float is
compared on its uint32 view and every integer with ==, the MrDbg record included; there is no
tolerance.  That each case reaches the branch or boundary it names is proved on the CPU, by the
oracle's branch record, in tests/test_tempo_decision_cases.py.
"""
import numpy as np
import pytest

import multires_cases as M
import sdsp
import units
from test_gpu_tempo_select import _bits, _spec, gpu_cfg

pytestmark = pytest.mark.gpu

DBG_I = ("fd", "fu", "tf", "fd_a0", "fd_a1", "fu_a0", "fu_a1", "tf_label", "fam", "forbid", "better")
DBG_F = ("fd_from", "fd_to", "fd_ratio", "fu_from", "fu_to", "fu_ratio", "tf_from", "tf_to", "tf_sup0", "tf_sup1", "tf_al0",
         "tf_al1", "rel")
SENT = dict(used=9, bpm=np.float32(-7.0), conf=np.float32(-0.5))  # uploaded first; the kernel writes none of these


def _ref(c):
    return units.multires_fuse(c["c256"], c["c512"], c["c1024"], c["nov"], c["sr"], c["base"], c["cfg"])


def check_item(got, ref, where):
    assert got["ok"] == int(ref["ok"]), where
    assert _bits([got["bpm"], got["conf"]]).tolist() == _bits([ref["bpm"], ref["conf"]]).tolist(), (where, got, ref)
    assert got["agree"] == ref["agree"], where
    d = got["dbg"]
    assert [d[k] for k in DBG_I] == [ref[k] for k in DBG_I], (where, d, {k: ref[k] for k in DBG_I})
    assert _bits([d[k] for k in DBG_F]).tolist() == _bits([ref[k] for k in DBG_F]).tolist(), (where, d, {k: ref[k] for k in DBG_F})


def check_track(t, used, fb, fc, ref, where):
    """used / final_bpm / final_conf of track t: the estimate where it was accepted, untouched otherwise."""
    if ref is None:
        want = (SENT["used"], SENT["bpm"], SENT["conf"])
    elif ref["used"]:
        want = (1, ref["bpm"], ref["conf"])
    else:
        want = (0, SENT["bpm"], SENT["conf"])
    assert (int(used[t]), *_bits([fb[t], fc[t]]).tolist()) == (want[0], *_bits(want[1:]).tolist()), (where, t)


def run_group(cases, own512, spare=True):
    """The cases as the items of one call; with `spare`, tracks that are not items before and between
    them, so an item's index and its track's differ."""
    c0 = cases[0]
    slots = []  # a case, or None for a track outside the item list
    for k, c in enumerate(cases):
        if spare and k in (0, 2):
            slots.append(None)
        slots.append(c)
    NR = len(slots)
    filler = dict(c512=M.cl((97, 0.3)), nov=M.noise(99, 40))
    base = [c["base"] if c else M.BASE for c in slots]
    items, tracks = [], []
    for t, c in enumerate(slots):
        if c is None:
            tracks.append(filler)
            continue
        it = dict(track=t, c256=c["c256"], c1024=c["c1024"])
        if own512:
            it.update(c512=c["c512"], nov=c["nov"])
        items.append(it)
        tracks.append(dict(c512=c["c512"], nov=c["nov"]))
    got, used, fb, fc = sdsp.debug_multires(
        items, None if own512 else tracks, base, own512=own512, config=gpu_cfg(c0["cfg"]), sample_rate=c0["sr"],
        used=[SENT["used"]] * NR, final_bpm=[SENT["bpm"]] * NR, final_conf=[SENT["conf"]] * NR)
    refs = [_ref(c) if c else None for c in slots]
    k = 0
    for t, c in enumerate(slots):
        if c is not None:
            check_item(got[k], refs[t], (c["name"], "own512" if own512 else "base512", NR))
            k += 1
        check_track(t, used, fb, fc, refs[t], (c["name"] if c else "spare", own512))


@pytest.fixture(scope="module")
def groups():
    out = {}
    for c in M.build():
        out.setdefault((c["cfg_key"], c["sr"]), []).append(c)
    return out


def test_every_case_in_ragged_calls(groups):
    """One call per configuration and sample rate over all its cases, the hop-512 lists by track
    (the base pass's) with tracks outside the item list between the items."""
    for cases in groups.values():
        run_group(cases, own512=False)


def test_every_case_with_its_own_hop512_lists(groups):
    """The same with the hop-512 lists and novelty by item (the escalation's own pass), for the
    cases whose list fits that pass's top_k rows."""
    for cases in groups.values():
        top_k = max(int(cases[0]["cfg"].tempogram_multi_res_top_k), 1)
        fit = [c for c in cases if c["c512"] is None or len(c["c512"]) <= top_k]
        if fit:
            run_group(fit, own512=True)


def test_every_case_alone(groups):
    for cases in groups.values():
        for c in cases:
            run_group([c], own512=False, spare=False)


def test_bad_arguments_are_refused(groups):
    c = groups[("default", 44100)][4]
    it = dict(track=0, c256=c["c256"], c1024=c["c1024"])
    trk = dict(c512=c["c512"], nov=c["nov"])
    cfg = gpu_cfg(c["cfg"])
    with pytest.raises(sdsp.AnalysisError):  # a list longer than its capacity
        sdsp.debug_multires([dict(it, c256=M.cl((100, 0.5), (120, 0.4)))], [trk], [M.BASE], cap_aux=1, config=cfg)
    with pytest.raises(sdsp.AnalysisError):  # an item outside the tracks
        sdsp.debug_multires([dict(it, track=1)], [trk], [M.BASE], config=cfg)
    with pytest.raises(sdsp.AnalysisError):  # items not ascending
        sdsp.debug_multires([dict(it, track=1), dict(it, track=0)], [trk, trk], [M.BASE, M.BASE], config=cfg)


@pytest.mark.parametrize("seed,frames", [(3, 200), (4, 331)])
def test_chain_from_the_stage_probes(seed, frames):
    """A spectrogram read at hops 256, 512 and 1024: the lists out of sdsp_debug_tempo_stages through
    sdsp_debug_tempo_select into sdsp_debug_multires give what the oracle's exports give in the same
    chain (tempo_stages, tempo_select, multires_fuse)."""
    import oracle
    import tempo_select_cases as S

    m = _spec(seed, frames)
    ocfg = oracle.default_config()
    cfg = gpu_cfg(ocfg)
    top_k = int(ocfg.tempogram_multi_res_top_k)
    aux_k = min(max(4 * top_k, 25), 200)
    glist, olist, nov = {}, {}, {}
    for hop, k in ((256, aux_k), (512, top_k), (1024, aux_k)):
        meta, (st,) = sdsp.debug_tempo_stages([m], 44100, hop, cfg)
        sel = sdsp.debug_tempo_select([dict(fft=st["fft"], acf=st["acf"])], present=meta["present"], top_n=k, cand_cap=k,
                                      gate=hop == 512, config=cfg)[0]
        assert sel["ok"] == 1
        glist[hop], nov[hop] = sel["cands"], st["nov"]["full"]
        ost = units.tempo_stages(m, 44100, hop, ocfg)
        osel = units.tempo_select(S.variants(ocfg, meta["present"], dict(fft={n: v["fft"] for n, v in ost.items()},
                                                                         acf={n: v["acf"] for n, v in ost.items()})),
                                  ocfg.min_bpm, ocfg.max_bpm, ocfg.bpm_resolution, ocfg)
        olist[hop] = osel["cands"][:k]
        assert np.array_equal(_bits(glist[hop]), _bits(olist[hop])), hop
        if hop == 512:
            base = (osel["bpm"], osel["conf"], osel["agree"], osel["trap_low"], osel["trap_high"])
            onov = ost["full"]["nov"]
    ref = units.multires_fuse(olist[256], olist[512], olist[1024], onov, 44100, base, ocfg)
    got, used, fb, fc = sdsp.debug_multires([dict(track=0, c256=glist[256], c1024=glist[1024])],
                                            [dict(c512=glist[512], nov=nov[512])], [base], config=cfg)
    check_item(got[0], ref, ("chain", seed))
    assert int(used[0]) == ref["used"]
    if ref["used"]:
        assert _bits([fb[0], fc[0]]).tolist() == _bits([ref["bpm"], ref["conf"]]).tolist()
