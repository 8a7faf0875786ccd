"""Stage probe of the key vote (sdsp_debug_key_vote) against the oracle's exported vote
(units.key_vote): k_key_vote's every output, bit for bit, over synthetic chroma rows and energies
that reach each branch and boundary on purpose (key_vote_cases.py); every instantiation the launcher
can pick (<256>, <512>, <1024>); and the near-decision certificate against its own claim (DESIGN.md
§2): for any reference energies within the per-frame bound, an unflagged track makes the reference's
discrete decisions.
"""
import numpy as np
import pytest

import key_vote_cases as kv
import oracle
import sdsp
import units

pytestmark = pytest.mark.gpu

NEAR_RANGE = 16


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


_CACHE = {}


def case(name):
    """(cfg, opts, tracks, oracle votes) of a configuration, computed once."""
    if name not in _CACHE:
        opts, frames = kv.CONFIGS[name]
        keep = []
        cfg = kv.config(opts, keep)
        tracks = kv.ragged_tracks(frames, seed=1000 + 97 * sorted(kv.CONFIGS).index(name))
        _CACHE[name] = (cfg, opts, tracks, [units.key_vote(c, e, cfg) for c, e in tracks], keep)
    return _CACHE[name][:4]


def segments(cfg, F):
    """The segments the vote evaluates on an F-frame slice, in its order: (start, length, weight, gate)."""
    out = []
    if cfg.enable_key_ensemble:
        return out
    if cfg.enable_key_multi_scale and cfg.key_multi_scale_lengths_len > 0:
        lens = [int(cfg.key_multi_scale_lengths[j]) for j in range(cfg.key_multi_scale_lengths_len)]
        if F >= min(lens):
            gate = np.float32(min(max(cfg.key_multi_scale_min_clarity, 0.0), 1.0))
            hop = max(int(cfg.key_multi_scale_hop), 1)
            for j, L in enumerate(lens):
                w = np.float32(cfg.key_multi_scale_weights[j]) if j < cfg.key_multi_scale_weights_len else np.float32(1)
                if L == 0 or L > F or w <= 0:
                    continue
                out += [(st, L, w, gate) for st in range(0, F - L + 1, hop)]
            return out
    L = int(cfg.key_segment_len_frames)
    if cfg.enable_key_segment_voting and L >= 120 and cfg.key_segment_hop_frames >= 1 and F >= L:
        hop = max(min(int(cfg.key_segment_hop_frames), L), 1)
        gate = np.float32(min(max(cfg.key_segment_min_clarity, 0.0), 1.0))
        out = [(st, L, np.float32(1), gate) for st in range(0, F - L + 1, hop)]
    return out


def check_track(got, ref, cfg, tag, near=0):
    """One track of a probe call against its oracle vote: every output on the uint32 view."""
    assert not ref["err"], tag
    assert (got["ok"], got["mode"], got["tonic"]) == (1, ref["mode"], ref["tonic"]), tag
    assert _same([got["conf"], got["clarity"]], [ref["confidence"], ref["clarity"]]), (tag, got["conf"], got["clarity"])
    assert (got["used_segments"], got["weights_used"]) == (ref["used_segments"], int(ref["weights_used"])), tag
    if near is not None:
        assert got["near"] == near, tag
    assert _same(got["chroma_s"], ref["chroma_s"]), tag
    t0, F = ref["t0"], ref["frames"]
    w = np.zeros(got["weights"].size, np.float32)
    w[t0:t0 + ref["weights"].size] = ref["weights"]
    assert _same(got["weights"], w), tag
    g = got["dbg"]
    assert _same(g["tab"], ref["tab"]) and np.array_equal(g["order"], ref["order"]) and g["key"] == ref["key"], tag
    assert g["frames"] == F, tag
    segs = segments(cfg, F)
    rows = got["rows"]
    assert len(segs) == ref["seg_raw"].shape[0] <= rows.shape[0], (tag, len(segs), ref["seg_raw"].shape, rows.shape)
    heuristic = cfg.enable_key_mode_heuristic or cfg.enable_key_minor_harmonic_bonus
    for s, (st, L, sw, gate) in enumerate(segs):
        row, cl = rows[s], ref["seg_clarity"][s]
        if not heuristic:  # the segment's table: key_from_raw's arithmetic over the trace's raw scores
            sc, ks = units.key_from_raw(ref["seg_raw"][s])
            assert _same(row[:24], sc) and np.array_equal(row[24:48], ks.astype(np.float32)), (tag, s)
            assert _same(oracle.key_clarity(sc), cl), (tag, s)
        assert _same(row[48], cl), (tag, s, row[48], cl)
        assert row[49] == (1.0 if cl >= gate else 0.0), (tag, s)
        assert _same(row[50], np.float32(cl) * sw), (tag, s)


def same_result(a, b, tag, cert=False):
    """Two probe results of the same call: every output bit-identical."""
    for x, y in zip(a, b):
        for k in ("mode", "tonic", "ok", "used_segments", "weights_used", "near"):
            assert x[k] == y[k], (tag, k, x[k], y[k])
        for k in ("conf", "clarity", "chroma_s", "weights") + (("wdel",) if cert else ()):
            assert _same(x[k], y[k]), (tag, k)
        assert ("rows" in x) == ("rows" in y), tag
        if "rows" in x:
            assert _same(x["rows"][:, :51], y["rows"][:, :51]), tag
            if cert:
                assert _same(x["rows"][:, 64:113], y["rows"][:, 64:113]), tag
            for k in ("tab", "order", "agg"):
                assert np.array_equal(_bits(x["dbg"][k]) if k != "order" else x["dbg"][k],
                                      _bits(y["dbg"][k]) if k != "order" else y["dbg"][k]), (tag, k)
            assert (x["dbg"]["key"], x["dbg"]["frames"], x["dbg"]["used"]) == (
                y["dbg"]["key"], y["dbg"]["frames"], y["dbg"]["used"]), tag


# ---- a. parity without a certificate ----
@pytest.mark.parametrize("name", sorted(kv.CONFIGS))
def test_parity_exact_path(name):
    cfg, opts, tracks, refs = case(name)
    got = sdsp.debug_key_vote(tracks, config=cfg)
    for t, (g, r) in enumerate(zip(got, refs)):
        check_track(g, r, cfg, (name, t, tracks[t][1].size))


def test_branches_are_reached():
    """The cases reach the branches they are named for (from the oracle alone)."""
    d = {n: case(n)[3] for n in kv.CONFIGS}
    fr = {n: kv.CONFIGS[n][1] for n in kv.CONFIGS}
    used = dict(zip(fr["default"], d["default"]))
    assert not used[9]["weights_used"] and not used[10]["weights_used"] and used[11]["weights_used"]
    assert [used[F]["seg_raw"].shape[0] for F in (1023, 1024, 2047, 2048, 2560, 4097)] == [0, 1, 2, 3, 4, 7]
    assert [r["seg_raw"].shape[0] for r in d["seg120_hop1"]] == [0, 1, 2, 281]
    assert [r["seg_raw"].shape[0] for r in d["hop_over_len"]] == [1, 1, 2, 3]
    assert all(r["used_segments"] == 0 and r["seg_raw"].shape[0] > 0 and r["full_raw"].shape[0] == 1
               for r in d["min_clarity_1"])
    et = dict(zip(fr["edge_trim"], d["edge_trim"]))
    assert et[199]["frames"] == 199 and (et[200]["t0"], et[200]["frames"]) == (30, 140)
    e49 = dict(zip(fr["edge_trim_0.49"], d["edge_trim_0.49"]))
    assert e49[2500]["frames"] == 2500 and (e49[2600]["t0"], e49[2600]["frames"]) == (1274, 52)
    assert all(not r["weights_used"] and r["weights"].size for r in d["min_tonal_0.9"])
    assert all(r["weights"].size == 0 for r in d["no_weighting"])
    assert all(r["full_raw"].shape[0] == 2 for r in d["ensemble"])
    ms = dict(zip(fr["multi_scale"], d["multi_scale"]))
    assert ms[119]["seg_raw"].shape[0] == 0 and ms[400]["seg_raw"].shape[0] == 5 and ms[1536]["seg_raw"].shape[0] == 24 + 9
    assert all(r["used_segments"] == 0 and r["seg_raw"].shape[0] > 0 for r in d["multi_scale_none_pass"])


def test_infinite_energy():
    """One +inf frame energy: the segment that holds it scores non-finite and drops out, the others
    vote; every field, the non-finite ones included, equals the oracle's on bits."""
    cfg = oracle.default_config()
    c, e = kv.make_track(77, 2049, 9, 0.15, 1.0)
    f = next(i for i in range(100, 200) if c[i].any())
    e[f] = np.inf
    ref = units.key_vote(c, e, cfg)
    assert not np.isfinite(ref["seg_raw"][0]).all() and np.isfinite(ref["seg_raw"][1:]).all()
    got = sdsp.debug_key_vote([(c, e)], config=cfg)[0]
    print("inf: oracle row 0", _bits(units.key_from_raw(ref["seg_raw"][0])[0])[:3], "probe", _bits(got["rows"][0, :3]),
          "weights", _bits(ref["weights"][f]), _bits(got["weights"][f]))
    check_track(got, ref, cfg, "inf")


def test_selection_and_single_calls():
    """A permuted subset votes as rerun_tail launches it (compact scratch offsets, frame prefix by
    track) and gives the full call's entries, leaving the other tracks' records untouched; a call
    of one track gives the ragged call's entry."""
    cfg, opts, tracks, refs = case("default")
    full = sdsp.debug_key_vote(tracks, config=cfg)
    sel = [16, 3, 9, 12, 0, 7]
    part = sdsp.debug_key_vote(tracks, sel=sel, config=cfg)
    for t in range(len(tracks)):
        if t in sel:
            same_result([part[t]], [full[t]], ("sel", t))
            check_track(part[t], refs[t], cfg, ("sel", t))
        else:
            assert part[t]["ok"] == -1 and part[t]["key"] == -1 and "rows" not in part[t], t
            assert not part[t]["chroma_s"].any() and not part[t]["weights"].any(), t
    for t in range(len(tracks)):
        one = sdsp.debug_key_vote([tracks[t]], config=cfg)
        same_result(one, [full[t]], ("single", t))


# ---- b. every instantiation ----
LAUNCHES = [dict(threads=256), dict(threads=512), dict(threads=1024), dict(threads=0, alone=False),
            dict(threads=0, alone=True)]


@pytest.mark.parametrize("name", ["default", "seg120_hop1", "multi_scale"])
def test_every_instantiation(name):
    cfg, opts, tracks, refs = case(name)
    base = None
    for kw in LAUNCHES:
        got = sdsp.debug_key_vote(tracks, config=cfg, **kw)
        for t, (g, r) in enumerate(zip(got, refs)):
            check_track(g, r, cfg, (name, kw, t))
        if base is not None:
            same_result(got, base, (name, kw))
        base = base or got


def test_launcher_choice_above_the_small_launch():
    """More tracks than the small-launch limit (96) and than the device has CUs: the launcher's own
    choice is <256> beside other work and <512> alone; both equal the forced <1024> and the oracle."""
    keep = []
    cfg = kv.config(kv.CONFIGS["seg120_hop1"][0], keep)
    tracks = [kv.make_track(5000 + i, 118 + i % 40, (5 * i) % 24, 0.15, 1.0) for i in range(320)]
    refs = [units.key_vote(c, e, cfg) for c, e in tracks]
    base = sdsp.debug_key_vote(tracks, config=cfg, threads=1024)
    for t, (g, r) in enumerate(zip(base, refs)):
        check_track(g, r, cfg, ("many", t))
    for alone in (False, True):
        same_result(sdsp.debug_key_vote(tracks, config=cfg, alone=alone), base, ("many", alone))


# ---- c, d. the certificate ----
D_VALUES = (2.0 ** -13, 0.01, 0.1)
_CERT = {}


def cert_sets():
    """name -> (cfg, opts, tracks, oracle votes, extra sign patterns per track)."""
    if not _CERT:
        keep = []
        clear = kv.clear_tracks()
        cfg = oracle.default_config()
        _CERT["clear"] = (cfg, {}, clear, [units.key_vote(c, e, cfg) for c, e in clear], [[] for _ in clear], keep)
        cont = kv.contested_tracks()
        cfg2 = kv.config(kv.CONTESTED, keep)
        xy = np.where((np.arange(400) // 8) % 2 == 0, 1.0, -1.0)
        _CERT["contested"] = (cfg2, kv.CONTESTED, cont, [units.key_vote(c, e, cfg2) for c, e in cont],
                              [[xy, -xy] for _ in cont], keep)
        long_ = kv.contested_long_tracks()
        xl = np.where((np.arange(2048) // 8) % 2 == 0, 1.0, -1.0)
        _CERT["contested_long"] = (cfg, {}, long_, [units.key_vote(c, e, cfg) for c, e in long_],
                                   [[xl, -xl] for _ in long_], keep)
    return _CERT


def decisions(v, cfg):
    """The discrete decisions the certificate covers, from an oracle vote."""
    gate = np.float32(min(max(cfg.key_segment_min_clarity, 0.0), 1.0))
    return (v["key"], v["weights_used"], v["used_segments"], kv.within_mode_tops(v["seg_raw"]).tolist(),
            (v["seg_clarity"] >= gate).tolist(), kv.within_mode_tops(v["full_raw"]).tolist())


_FLIPS = {}


def flips(name, d):
    """Per track: whether some adversarial energy pattern within the bound d changes a decision of
    the oracle's vote, and the largest confidence / clarity movement seen (oracle alone, cached)."""
    if (name, d) not in _FLIPS:
        cfg, opts, tracks, refs, extra = cert_sets()[name][:5]
        out = []
        for t, ((c, e), ref) in enumerate(zip(tracks, refs)):
            want, flip, move = decisions(ref, cfg), False, 0.0
            for p in kv.sign_patterns(ref, opts, 9000 + t) + extra[t]:
                v = units.key_vote(c, kv.adversarial_energies(e, d, p), cfg)
                flip |= decisions(v, cfg) != want
                move = max(move, abs(float(v["confidence"]) - float(ref["confidence"])),
                           abs(float(v["clarity"]) - float(ref["clarity"])))
            out.append((flip, move))
        _FLIPS[(name, d)] = out
    return _FLIPS[(name, d)]


def test_contested_set_has_teeth():
    """From the oracle alone: within the bound, the adversarial energies flip a decision of at least
    30 of the 40 contested tracks at d = 0.1 and of at least 5 at d = 0.01."""
    n1 = sum(f for f, _ in flips("contested", 0.1))
    n2 = sum(f for f, _ in flips("contested", 0.01))
    print(f"contested tracks whose decisions flip: {n1} of 40 at d = 0.1, {n2} of 40 at d = 0.01")
    assert n1 >= 30 and n2 >= 5


def test_clear_set_is_clear():
    """From the oracle alone: every segment's within-mode top-two relative gap is >= 0.005 in both
    modes, every clarity is >= 0.05 from the gate and the final confidence is >= 0.02."""
    cfg, opts, tracks, refs = cert_sets()["clear"][:4]
    gaps, dist, conf = [], [], []
    for r in refs:
        assert r["seg_raw"].shape[0] >= 1 and r["used_segments"] == r["seg_raw"].shape[0]
        for raw in r["seg_raw"]:
            for m in range(2):
                v = np.sort(raw[12 * m:12 * m + 12].astype(np.float64))[::-1]
                gaps.append((v[0] - v[1]) / v[0])
        dist += [abs(float(cl) - float(np.float32(cfg.key_segment_min_clarity))) for cl in r["seg_clarity"]]
        # The reported confidence (best - second) / best is exactly 0 on every such track: each mode's
        # top is normalised to 1 and gets the same bonus, so with the same two tops in every segment
        # the major and the minor leader tie exactly (the kernel's "structural tie", which the
        # certificate skips).  The gap that a perturbation must cross is the leader's to the best
        # key outside that tie.
        tab, tops = r["tab"], kv.within_mode_tops(r["seg_raw"])
        if r["confidence"] < 0.02:
            assert tab[0] == tab[1] and (tops == tops[0]).all()
            assert sorted(r["order"][:2]) == [tops[0][0], 12 + tops[0][1]]
        lower = tab[tab < tab[0]]
        conf.append(float((tab[0] - lower[0]) / tab[0]))
    print(f"clear set: min gap {min(gaps):.4f}, min clarity distance {min(dist):.4f}, min final gap {min(conf):.4f}")
    assert min(gaps) >= 0.005 and min(dist) >= 0.05 and min(conf) >= 0.02


@pytest.mark.parametrize("d", D_VALUES)
@pytest.mark.parametrize("name", ["clear", "contested", "contested_long"])
def test_certificate_is_sound(name, d):
    """An unflagged track makes the decisions of every reference whose energies lie within the bound;
    every track whose decisions some such reference flips is flagged.  Confidences and clarities
    move continuously with d and are not asserted; their worst movement is printed (measured at
    d = 2^-13: 3.2e-6 on the clear set, 6.7e-6 on the contested one; DESIGN.md §2 has the flag counts)."""
    cfg, opts, tracks, refs = cert_sets()[name][:4]
    got = sdsp.debug_key_vote(tracks, edel=[np.full(e.size, d, np.float32) for _, e in tracks], config=cfg)
    fl = flips(name, d)
    flagged = [g["near"] != 0 for g in got]
    bits = {}
    for g in got:
        bits[g["near"]] = bits.get(g["near"], 0) + 1
    print(f"{name} d = {d:g}: {sum(flagged)} of {len(got)} flagged (near -> tracks: {bits}); "
          f"{sum(f for f, _ in fl)} flip; worst confidence / clarity movement {max(m for _, m in fl):.3g}")
    for t, (g, r) in enumerate(zip(got, refs)):
        check_track(g, r, cfg, (name, d, t), near=None)  # the probe's own vote is the oracle's on e
        assert not (fl[t][0] and not flagged[t]), (name, d, t, "a decision flips within the bound, unflagged")
    if name == "clear" and d == D_VALUES[0]:
        assert not any(flagged), [(t, g["near"]) for t, g in enumerate(got) if g["near"]]


@pytest.mark.parametrize("d", D_VALUES[1:])
@pytest.mark.parametrize("name", ["clear", "contested", "contested_long"])
def test_certificate_every_instantiation(name, d):
    """near, wdel and the certificate's row columns are the same under every instantiation."""
    cfg, opts, tracks, refs = cert_sets()[name][:4]
    edel = [np.full(e.size, d, np.float32) for _, e in tracks]
    base = None
    for kw in LAUNCHES:
        got = sdsp.debug_key_vote(tracks, edel=edel, config=cfg, **kw)
        if base is not None:
            same_result(got, base, (name, kw), cert=True)
        base = base or got
    assert any(g["wdel"].any() for g in base)


def test_certificate_range_and_fixed_margins():
    """A bound of 0.25 or more on one used frame is outside the certificate's range (bit 16); the
    fixed margins flag a subset of what the rigorous certificate flags."""
    cfg, opts, tracks, refs = cert_sets()["contested"][:4]
    edel = [np.full(e.size, 0.01, np.float32) for _, e in tracks]
    f = int(np.flatnonzero(refs[0]["weights"] > 0)[5])
    edel[0][f] = 0.25
    rig = sdsp.debug_key_vote(tracks, edel=edel, config=cfg)
    fix = sdsp.debug_key_vote(tracks, edel=edel, config=cfg, cert_fixed=True)
    assert rig[0]["near"] & NEAR_RANGE
    assert not any(g["near"] & NEAR_RANGE for g in rig[1:])
    assert all(r["near"] != 0 for r, x in zip(rig, fix) if x["near"] != 0)
    assert sum(x["near"] != 0 for x in fix) <= sum(r["near"] != 0 for r in rig)
