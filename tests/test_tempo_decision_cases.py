"""The case tables of the tempo decision kernels' stage tests (tests/tempo_select_cases.py,
tests/multires_cases.py) checked against the oracle alone: every case reaches the branch or boundary
it names, by the oracle's branch record, and each table as a whole reaches both sides of every
comparison listed here.  The GPU tests (test_gpu_tempo_select.py, test_gpu_multires_stages.py)
compare the kernels with the oracle on exactly these cases, none skipped, so what this file proves
reachable is what they pin.
"""
import re

import numpy as np
import pytest

import multires_cases as M
import tempo_select_cases as S
import units

F = np.float32


def _lists_ok(a):
    a = np.asarray(a, F).reshape(-1, 2)
    return bool(np.isfinite(a).all() and (a >= 0).all() and (np.diff(a[:, 1]) <= 0).all())


@pytest.fixture(scope="module")
def sel():
    out = {}
    for gname, g in S.build().items():
        for name, trk, check in g["cases"]:
            cfg = g["cfg"]
            r = units.tempo_select(S.variants(cfg, g["present"], trk), cfg.min_bpm, cfg.max_bpm, cfg.bpm_resolution, cfg)
            out[(gname, name)] = (g, trk, check, r)
    return out


def test_selection_lists_are_tempogram_lists(sel):
    """Finite, non-negative, sorted by value descending; one FFT length per track, one grid per group."""
    for (gname, name), (g, trk, _, _) in sel.items():
        for n in S.VARIANTS:
            assert _lists_ok(trk["fft"][n]) and _lists_ok(trk["acf"][n]), (gname, name, n)
            assert len(trk["fft"][n]) <= 1024 and len(trk["acf"][n]) <= 512
    for gname, g in S.GROUPS.items():
        assert len({len(t["acf"]["full"]) for _, t, _ in g["cases"]}) == 1, gname


def test_selection_cases_reach_what_they_name(sel):
    for key, (g, trk, check, r) in sel.items():
        assert check is not None or not trk["active"], key  # every case carries its check
        if trk["active"]:
            assert check(r), (key, None if r is None else {k: v for k, v in r.items() if k != "cands"})


def test_selection_table_reaches_both_sides(sel):
    recs = {k: v[3] for k, v in sel.items() if v[3] is not None and v[1]["active"]}
    R = list(recs.values())

    def some(f):
        return any(f(r) for r in R)

    assert some(lambda r: r is None) or any(v[3] is None for v in sel.values())  # Err: no candidate
    fft_ns = {len(v[1]["fft"]["full"]) for v in sel.values()}
    assert {0, 1, 7, 8, 9, 1024} <= fft_ns
    assert some(lambda r: r["n_out"] > 0) and some(lambda r: r["n_in"] > 0)
    assert some(lambda r: r["n_dup"] > 0) and some(lambda r: r["n_uniq"] > 1)  # an image dropped; one kept beside another
    assert some(lambda r: r["n_pen_hi"] > 0) and some(lambda r: r["n_pen_lo"] > 0)
    assert some(lambda r: r["n_uniq"] > r["n_pen_hi"] + r["n_pen_lo"])
    for k in (0, 1, 2, 4):  # the consensus bonus with 0, 1, 2 and 4 supporting variants
        assert some(lambda r: r[f"sb{k}"] > 0), k
    for k in range(5):  # the octave fold: not tried, half out of range, no candidate, kept out, taken
        assert some(lambda r: r["fold"] == k), k
    assert some(lambda r: r["n_uniq"] == 1 and r["conf"] == 1)
    assert some(lambda r: r["conf"] == 0)
    for a in (0, 1, 2):
        assert some(lambda r: r["agree"] == a), a
    for flag in ("trap_low", "trap_high", "family", "fold_into_trap", "weak", "ambiguous"):
        assert some(lambda r: r[flag] == 1) and some(lambda r: r[flag] == 0), flag
    # weak by agreement alone and by confidence alone, each with and without fold_into_trap
    for fold in (0, 1):
        assert some(lambda r: r["agree"] == 0 and r["conf"] >= F(0.06) and r["fold_into_trap"] == fold), fold
        assert some(lambda r: r["agree"] > 0 and r["conf"] < F(0.06) and r["fold_into_trap"] == fold), fold
    # the trap zones' ends from both sides
    for b in (55, 80, 170, 200):
        for x in (F(b), S.up(b), S.dn(b)):
            assert some(lambda r: r["bpm"] == x and r["n_uniq"] == 1), x
    # family support exactly at 0.90 of the base's and one step under
    assert some(lambda r: r["s_2x"] > 0 and r["s_2x"] == F(r["s_base"] * F(0.9)) and r["family"])
    assert some(lambda r: 0 < r["s_2x"] < F(r["s_base"] * F(0.9)) and r["s_half"] == 0 and not r["family"])
    # equal scores at the top of a scored list and straddling top_n
    assert some(lambda r: len(r["cands"]) > 1 and r["cands"][0, 1] == r["cands"][1, 1] > 0)
    assert any(v[3] is not None and len(v[3]["cands"]) > v[0]["top_n"] and
               v[3]["cands"][v[0]["top_n"] - 1, 1] == v[3]["cands"][v[0]["top_n"], 1] > 0 for v in sel.values())
    # the nearest lookup: an equidistant entry of another value passed over; an entry exactly at the
    # FFT tolerance taken (an autocorrelation entry at its tolerance can never be the nearest: the
    # grid covers the range at a spacing of at most the tolerance)
    assert some(lambda r: r["n_tie"] > 0) and some(lambda r: r["n_at_tol"] > 0)
    assert not some(lambda r: r["n_at_tol_ac"] > 0)
    # top_n / cand_cap above and below the number of candidates
    assert any(v[0]["top_n"] > v[3]["n_uniq"] for v in sel.values() if v[3] is not None)
    assert any(v[0]["top_n"] < v[3]["n_uniq"] for v in sel.values() if v[3] is not None)
    assert any(v[0]["cand_cap"] < min(v[0]["top_n"], v[3]["n_uniq"]) for v in sel.values() if v[3] is not None)
    presents = {v[0]["present"] for v in sel.values()}
    assert len([p for p in presents if p[0] == 1]) >= 16


# ---- the multi-resolution fusion ----
@pytest.fixture(scope="module")
def mr():
    return [(c, units.multires_fuse(c["c256"], c["c512"], c["c1024"], c["nov"], c["sr"], c["base"], c["cfg"]))
            for c in M.build()]


def test_fusion_lists_are_selection_lists(mr):
    """Sorted by score descending, finite, non-negative; novelty finite and non-negative."""
    for c, _ in mr:
        for k in ("c256", "c512", "c1024"):
            a = c[k]
            assert a is None or (np.isfinite(a).all() and (a >= 0).all() and (np.diff(a[:, 1]) <= 0).all()), (c["name"], k)
        assert np.isfinite(c["nov"]).all() and (c["nov"] >= 0).all() and c["nov"].size <= 15000, c["name"]


def test_fusion_cases_reach_what_they_name(mr):
    for c, r in mr:
        assert c["check"] is not None and c["check"](r), (c["name"], {k: v for k, v in r.items() if np.any(v != 0)})
        if "cut" in c:  # the hypotheses past the cut decide: the list cut there gives another estimate
            t = units.multires_fuse(c["c256"], c["c512"][:c["cut"]], c["c1024"], c["nov"], c["sr"], c["base"], c["cfg"])
            assert (t["bpm"], t["conf"]) != (r["bpm"], r["conf"]), c["name"]


def test_fusion_table_reaches_both_sides(mr):
    R = [r for _, r in mr if r["ok"]]

    def some(f):
        return any(f(r) for r in R)

    assert sum(not r["ok"] for _, r in mr) >= 4  # a failed hop in each position, and no hypotheses
    # every structural discount and band penalty taken by some hypothesis and left by another
    for k in ("n_h102", "n_2t102", "n_r2_110", "n_r2_100", "n_rh_110", "n_rh_100", "n_pen210", "n_pen180", "n_pen60",
              "n_margin_lo", "n_reset", "n_prior", "n_dup"):
        assert some(lambda r: r[k] > 0) and some(lambda r: r[k] < r["n_hyps"]), k
    assert some(lambda r: r["n_reset"] == 0 and r["n_margin_lo"] == 1)  # |cb - t| at 1e-3: not reset
    assert some(lambda r: r["n_uniq"] == 8 and r["n_hyps"] > 8)
    # the fold gates: each condition true and false where the gate is evaluated
    for g in ("fd", "fu"):
        for bit in (4, 2, 1):
            assert some(lambda r: r[g + "_eval"] and (r[g + "_eval"] - 1) & bit), (g, bit)
            assert some(lambda r: r[g + "_eval"] and not (r[g + "_eval"] - 1) & bit), (g, bit)
        assert some(lambda r: r[g] == 1) and some(lambda r: r[g + "_eval"] and not r[g])
    assert some(lambda r: r["fd_eval_a1"] == 2) and some(lambda r: r["fd_eval_a1"] == 3)
    assert some(lambda r: r["fu_eval_a1"] == 1) and some(lambda r: r["fu_eval_a1"] == 2)
    assert some(lambda r: r["fd_eval_ratio"] == F(0.45) and r["fd"]) and some(lambda r: r["fd_eval_ratio"] == M.dn(0.45))
    assert some(lambda r: r["fu_eval_ratio"] == F(0.55) and r["fu"]) and some(lambda r: r["fu_eval_ratio"] == M.dn(0.55))
    for n in (0, 1, 2, 5):
        assert some(lambda r: r["n_fam"] == n), n
    assert some(lambda r: r["max_alt"] == F(0.45) and r["fam_eval"]) and some(lambda r: r["max_alt"] == M.dn(0.45))
    assert some(lambda r: r["tf"] == 1) and some(lambda r: r["fam_eval"] and not r["tf"])
    assert some(lambda r: r["fam_eval"] and r["chosen"] == 0)
    # the chosen member's alignment exactly at the current one + 0.40 (taken) and under it (not taken)
    assert some(lambda r: r["tf"] and r["tf_al1"] == F(r["tf_al0"] + F(0.40)))
    assert some(lambda r: r["fam_eval"] and not r["tf"] and r["chosen"] > 0 and
                F(0.3999) < r["fam_align"][r["chosen"]] < F(r["cur_align"] + F(0.40)))
    # the acceptance: each clause alone, forbid, fam and better both ways
    for cl in (1, 2, 4):
        assert some(lambda r: r["clause"] == cl and r["used"]), cl
    for k in ("fam", "forbid", "better"):
        assert some(lambda r: r[k] == 1) and some(lambda r: r[k] == 0), k
    assert some(lambda r: r["rel"] == 1 and r["used"])
    # top_k values, the candidate counts around the 64-entry array and past 256
    assert {1, 25, 64, 65, 100, 257} <= {r["n_hyps"] for r in R}
    # novelty lengths: under 16, one segment +- 1, multi-segment; periods under 6, 6-8, >= 9, > 64, > 512
    ns = {c["nov"].size for c, _ in mr}
    for P in (M.period(44100, 80), M.period(44100, 180)):
        seg = 4096 - P
        assert {15, 16, seg - 1, seg, seg + 1, 2 * seg + 1, int(3.5 * seg)} <= ns
    ps = {M.period(c["sr"], b) for c, r in mr if r["ok"] for b in r["fam_bpm"]}
    assert any(p < 6 for p in ps) and any(6 <= p <= 8 for p in ps) and any(p > 64 for p in ps)
    assert any(p > 512 for p in ps) and any(448 < p <= 512 for p in ps)


def _beat_contrast_model(nov, P, zero_halo):
    """beat_contrast in f32 as the kernel walks it, in staging segments of 4096 - P frames; with
    zero_halo, a half- or third-beat lookup past its beat's segment end reads 0 (a lost halo)."""
    n, seg = len(nov), 4096 - P
    w = np.array([nov[max(i - 2, 0):min(i + 3, n)].max() for i in range(n)], F)
    mean = max(F(np.cumsum(nov, dtype=F)[-1] / F(n)), F(1e-6))  # cumsum folds in order, one rounding per step
    best = F(-1e9)
    for ph in range(P):
        bs = hs = ts = F(0)
        bn = hn = tn = 0
        for i in range(ph, n, P):
            s1 = (i // seg + 1) * seg
            bs, bn = F(bs + w[i]), bn + 1
            for j, third in ((i + P // 2, False), (i + P // 3, True), (i + (2 * P) // 3, True)):
                if j < n:
                    v = F(0) if zero_halo and j >= s1 else w[j]
                    if third:
                        ts, tn = F(ts + v), tn + 1
                    else:
                        hs, hn = F(hs + v), hn + 1
        c = F(F(F(bs / F(bn)) - F(F(0.6) * F(hs / F(hn)))) - F(F(0.4) * F(ts / F(tn))))
        best = max(best, min(max(F(c / mean), F(-10)), F(10)))
    return best


def test_a_lost_halo_changes_the_compared_alignments(mr):
    """On the two-segment cases, a model of the staged walk reproduces the oracle's alignments bit
    for bit, and with the halo zeroed both alignments the GPU test compares (tf_al0, tf_al1) change:
    a kernel that lost or misplaced its halo would fail those cases."""
    hit = 0
    for c, r in mr:
        m = re.search(r"\(segments of (\d+)\)", c["name"])
        if not m or c["nov"].size != 2 * int(m.group(1)) + 1:
            continue
        hit += 1
        for bpm, al in ((r["tf_from"], r["tf_al0"]), (r["tf_to"], r["tf_al1"])):
            P = M.period(44100, float(bpm))
            assert P >= 9 and _beat_contrast_model(c["nov"], P, False) == al, (c["name"], bpm)
            assert _beat_contrast_model(c["nov"], P, True) != al, (c["name"], bpm)
    assert hit == 4
