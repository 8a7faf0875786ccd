"""Inputs of the candidate selection's stage tests (tests/test_tempo_decision_cases.py on the CPU,
tests/test_gpu_tempo_select.py on the GPU): tempogram lists built directly, no audio.

A list is what a tempogram produces: (bpm, value) pairs, finite, non-negative, sorted by value
descending with equal values in ascending grid order (the kernels' index tie-break).  The
autocorrelation list is the whole BPM grid of its configuration (min_bpm, min_bpm + res, ... in f32),
the FFT list any bins in range.  Every case names the branch or boundary it is for and carries a
check on the oracle's branch record (units.tempo_select); cases of one GROUP share a configuration
and the call's parameters, so a group is one ragged probe call.
"""
import numpy as np

import oracle

F = np.float32
VARIANTS = ("full", "low", "mid", "high", "mel")


def up(x, k=1):
    x = F(x)
    for _ in range(k):
        x = np.nextafter(x, F(np.inf))
    return x


def dn(x, k=1):
    x = F(x)
    for _ in range(k):
        x = np.nextafter(x, F(-np.inf))
    return x


def config(**opts):
    c = oracle.default_config()
    for k, v in opts.items():
        setattr(c, k, v)
    return c


def grid(cfg):
    """The autocorrelation tempogram's BPM grid (tempogram_autocorr.rs: bpm += res in f32)."""
    g, b = [], F(cfg.min_bpm)
    while b <= F(cfg.max_bpm):
        g.append(b)
        b = F(b + F(cfg.bpm_resolution))
    return np.array(g, F)


def acf_list(cfg, peaks):
    """The grid with `peaks` {bpm: value} (a bpm snaps to its nearest grid point), zero elsewhere."""
    g = grid(cfg)
    v = np.zeros(g.size, F)
    for b, x in peaks.items():
        v[int(np.argmin(np.abs(g - F(b))))] = F(x)
    order = np.argsort(-v, kind="stable")
    return np.stack([g[order], v[order]], axis=1)


def fft_list(pairs):
    a = np.array(pairs, F).reshape(-1, 2)
    return a[np.argsort(-a[:, 1], kind="stable")]


def weights(cfg):
    """The weight of each variant as analyze's BandCfg carries it (w_full is 1 without a BandCfg)."""
    used = cfg.enable_tempogram_band_fusion or cfg.enable_tempogram_mel_novelty or cfg.tempogram_band_consensus_bonus > 0
    return dict(full=F(cfg.tempogram_band_w_full) if used else F(1.0), low=F(cfg.tempogram_band_w_low),
                mid=F(cfg.tempogram_band_w_mid), high=F(cfg.tempogram_band_w_high), mel=F(cfg.tempogram_mel_weight))


def variants(cfg, present, trk):
    """units.tempo_select's variants of a track under `present`."""
    w = weights(cfg)
    return [(n, w[n], trk["fft"][n], trk["acf"][n]) for v, n in enumerate(VARIANTS) if present[v]]


def track(cfg, fft, acf, **per_variant):
    """A track whose variants all carry the lists (fft pairs, acf peaks) unless per_variant gives
    name=(fft pairs, acf peaks) of its own; the FFT lists of one track share their length."""
    t = dict(fft={}, acf={}, active=True)
    for n in VARIANTS:
        f, a = per_variant.get(n, (fft, acf))
        t["fft"][n], t["acf"][n] = fft_list(f), acf_list(cfg, a)
    assert len({len(t["fft"][n]) for n in VARIANTS}) == 1
    return t


def family_flip(cfg, base, other):
    """The two adjacent f32 values of the FFT entry at `other` between which the gate's family
    comparison (support >= 0.90 of the base's) flips, found with the oracle: (at, one step under)."""
    import units

    def fam(v):
        t = track(cfg, [(F(base), 1.0), (F(other), v)], {})
        r = units.tempo_select(variants(cfg, ALL, t), cfg.min_bpm, cfg.max_bpm, cfg.bpm_resolution, cfg)
        return r["family"]

    lo, hi = F(0.85), F(0.95)
    assert not fam(lo) and fam(hi)
    while up(lo) < hi:
        mid = F((lo.astype(np.float64) + hi.astype(np.float64)) / 2)
        mid = mid if lo < mid < hi else up(lo)
        lo, hi = (lo, mid) if fam(mid) else (mid, hi)
    return hi, lo


ALL = (1, 1, 1, 1, 1)
GROUPS = {}  # name -> dict(cfg, present, top_n, cand_cap, gate, cases=[(name, track, check)])


def group(name, cfg=None, present=ALL, top_n=25, cand_cap=25, gate=True):
    GROUPS[name] = dict(cfg=cfg if cfg is not None else config(), present=present, top_n=top_n, cand_cap=cand_cap,
                        gate=gate, cases=[])
    return GROUPS[name]


def case(g, name, trk, check=None):
    g["cases"].append((name, trk, check))


def _rand_track(cfg, seed, n_fft):
    """A generic track: random in-range FFT bins and a few grid peaks per variant."""
    rng = np.random.default_rng(seed)
    pv = {}
    for n in VARIANTS:
        f = [(F(rng.uniform(cfg.min_bpm, cfg.max_bpm)), F(rng.random() ** 3)) for _ in range(n_fft)]
        a = {float(rng.uniform(cfg.min_bpm, cfg.max_bpm)): float(rng.random()) for _ in range(6)}
        pv[n] = (f, a)
    return track(cfg, [], {}, **pv)


def build():
    GROUPS.clear()
    # ---- the default configuration: list lengths, generic tracks, the score penalties ----
    c = config()
    g = group("default", c)
    for n in (0, 1, 7, 8, 9, 1024):  # seeds are the first 8 entries; 1024 is the probe's maximum
        case(g, f"fft_n={n}", _rand_track(c, 100 + n, n), lambda r, n=n: r is not None)
    zero = track(c, [(F(100), F(0)), (F(150), F(0))], {})
    case(g, "all-zero values: the 1e-12 floors, conf 0", zero, lambda r: r["conf"] == 0 and not r["cands"][:, 1].any())
    inactive = _rand_track(c, 7, 5)
    inactive["active"] = False
    case(g, "inactive track between active ones", inactive)
    case(g, "generic after the inactive one", _rand_track(c, 8, 12), lambda r: r is not None)
    # seed images at the range's ends: 80 x 3 = 240 and 120 / 3 = 40 inside, one ulp further outside
    case(g, "images at max_bpm", track(c, [(F(80), 1.0), (up(80), 0.5)], {}), lambda r: r["n_in"] and r["n_out"])
    case(g, "images at min_bpm", track(c, [(F(80), 1.0), (dn(80), 0.5)], {}), lambda r: r["n_in"] and r["n_out"])
    # agreement with a peak exactly 2.0 away (not < 2.0) and just inside
    case(g, "agree 2", track(c, [(F(120), 1.0)], {120.0: 1.0}), lambda r: r["agree"] == 2)
    case(g, "agree 1: the autocorrelation peak exactly 2.0 from the best", track(c, [(F(122), 1.0)], {120.0: 1.0, 122.0: 0.5}),
         lambda r: r["bpm"] == 122 and r["ac_pb"] == 120 and r["agree"] == 1)
    case(g, "agree 2: the FFT peak one ulp inside 2.0 of the best", track(c, [(dn(122), 1.0)], {120.0: 1.0}),
         lambda r: r["bpm"] == 120 and r["fft_pb"] == dn(122) and r["agree"] == 2)
    # the octave fold (best above 180): no candidate at the half, kept out, let in
    strong = {190.0: 1.0}
    case(g, "fold: half let in, neither ratio above 2", track(c, [(F(190), 1.0), (F(95), 0.6)], {190.0: 1.0, 95.0: 0.6}),
         lambda r: r["fold"] == 4 and r["bpm"] == 95)
    case(g, "fold: both ratios above 2", track(c, [(F(190), 1.0), (F(95), 0.1)], {190.0: 1.0, 95.0: 0.1}),
         lambda r: r["fold"] == 3 and r["bpm"] == 190)
    case(g, "fold: one ratio above 2", track(c, [(F(190), 1.0), (F(95), 0.1)], {190.0: 1.0, 95.0: 0.9}),
         lambda r: r["fold"] == 4 and r["bpm"] == 95)
    case(g, "fold: the half is only an image of the best", track(c, [(F(200), 1.0)], strong),
         lambda r: r["fold"] == 4 and r["bpm"] == 95)
    case(g, "no fold: the best is the half already", track(c, [(F(190), 1.0), (F(95), 0.9)], {190.0: 1.0, 95.0: 0.9}),
         lambda r: r["fold"] == 0 and r["bpm"] == 95)
    # the best (190) is the 3/2 image of a seed and sits ninth in both lists (equal values, ascending
    # BPM), so neither it nor its half is seeded: no candidate within 0.75 of 95
    f9 = [(F(190.0 / 1.5), 1.0)] + [(F(b), 1.0) for b in range(181, 188)] + [(F(190), 1.0)]
    a9 = {float(b): 1.0 for b in list(range(150, 158)) + [190]}
    case(g, "fold: no candidate at the half", track(c, f9, a9), lambda r: r["fold"] == 2)
    # the folded value exactly at min_bpm (tried) and one ulp outside it (not tried)
    for lo, lab, want in ((F(95), "at", (3, 4)), (up(95), "one ulp under", (1,))):
        cf = config(min_bpm=float(lo))
        g = group(f"fold, half {lab} min_bpm", cf)
        case(g, f"fold: half {lab} min_bpm", track(cf, [(F(190), 1.0)], {190.0: 1.0}),
             lambda r, want=want: r["bpm"] in (F(95), F(190)) and r["fold"] in want)
    # ---- one narrow grid per exact boundary: few seeds, every candidate accounted for ----
    # a single unique candidate: the second score is 0, conf 1
    n1 = config(min_bpm=100.0, max_bpm=100.5)
    g = group("single", n1)
    case(g, "single unique candidate", track(n1, [(F(100), 1.0)], {100.0: 1.0}),
         lambda r: r["n_uniq"] == 1 and r["conf"] == 1)
    # every image outside the range: no candidate, Err
    g = group("no-candidate", config(min_bpm=100.0, max_bpm=100.5, bpm_resolution=1.0), gate=True)
    case(g, "all images outside", dict(fft={n: fft_list([(F(101), 1.0)]) for n in VARIANTS},
                                       acf={n: np.array([[101.0, 1.0]], F) for n in VARIANTS}, active=True),
         lambda r: r is None)
    # candidates at exactly 180 and 60 and one ulp either side (the 0.80 / 0.90 penalties), on a grid of
    # two points so that nothing dedupes them away
    for b, lo, hi in ((180, 170.0, 190.0), (60, 55.0, 65.0)):
        cp = config(min_bpm=lo, max_bpm=hi, bpm_resolution=hi - lo)
        g = group(f"penalty {b}", cp)
        for x, lab in ((F(b), "at"), (up(b), "above"), (dn(b), "below")):
            pen = int((b == 180 and x > 180) or (b == 60 and x < 60))
            case(g, f"candidate {lab} {b}", track(cp, [(x, 1.0)], {}),
                 lambda r, x=x, pen=pen, b=b: any(q[0] == x for q in r["cands"]) and
                 (r["n_pen_hi"] - 1 if b == 180 else r["n_pen_lo"] - 1) == pen)
    # the 0.75 dedupe on a fine grid: seeds exactly 0.75 apart (kept), one ulp under (dropped), a chain
    d = config(min_bpm=100.0, max_bpm=104.0, bpm_resolution=4.0)
    g = group("dedupe", d)
    case(g, "two seeds exactly 0.75 apart", track(d, [(F(101), 1.0), (F(101.75), 0.5)], {}),
         lambda r: any(q[0] == F(101.75) for q in r["cands"]))
    case(g, "two seeds one ulp under 0.75 apart", track(d, [(F(101), 1.0), (dn(101.75), 0.5)], {}),
         lambda r: r["n_dup"] >= 1 and not any(q[0] == dn(101.75) for q in r["cands"]))
    case(g, "three seeds in a 0.5 chain: the third is kept", track(d, [(F(101), 1.0), (F(101.5), 0.5), (F(102), 0.4)], {}),
         lambda r: [q for q in sorted(r["cands"][:, 0]) if 100.9 < q < 102.1] == [F(101), F(102)])
    case(g, "three seeds in a 0.75 chain: all kept", track(d, [(F(101), 1.0), (F(101.75), 0.5), (F(102.5), 0.4)], {}),
         lambda r: [q for q in sorted(r["cands"][:, 0]) if 100.9 < q < 102.6] == [F(101), F(101.75), F(102.5)])
    u = dn(101.75)  # one ulp under 0.75 from 101: dropped, and the third link is measured from 101
    case(g, "three seeds in a chain one ulp under 0.75", track(d, [(F(101), 1.0), (u, 0.5), (F(u + F(0.75)), 0.4)], {}),
         lambda r, u=u: [q for q in sorted(r["cands"][:, 0]) if 100.9 < q < 102.6] == [F(101), F(u + F(0.75))])
    # the nearest lookup: two entries equidistant from the query (the first in list order wins), an
    # entry exactly at the tolerance (taken) and one ulp past it
    # The query 101.5 is seeded by the low variant alone; the full variant, which scores it, has no
    # entry there but two at 0.25 on either side with different values, ninth and tenth in its list
    # (behind eight bins near 103 that dedupe into one candidate), so neither is a seed.
    lead = [(F(103.0 + 0.0625 * i), 1.0) for i in range(8)]
    for lab, va, vb in (("the lower BPM first", 0.6, 0.4), ("the higher BPM first", 0.4, 0.6)):
        full = lead + [(F(101.25), va), (F(101.75), vb)]
        low = [(F(101.5), 1.0)] + lead + [(F(103.5), 0.5)]
        case(g, f"lookup tie, {lab}: the first in list order wins", track(d, full, {}, low=(low, {})),
             lambda r: r["n_tie"] >= 1 and
             [q[2] for q in r["cands"] if q[0] == F(101.5)] == [F(F(F(0.4) * F(0.6)) / F(0.4))])
    score_at = lambda r, x: [q[1] for q in r["cands"] if q[0] == x]
    case(g, "entry exactly at the 0.75 tolerance: taken", track(d, [(F(103), 1.0)], {}, low=([(F(103.75), 1.0)], {})),
         lambda r: r["n_at_tol"] >= 1 and score_at(r, F(103.75)) and score_at(r, F(103.75))[0] > 0)
    case(g, "entry one ulp past the tolerance: not taken", track(d, [(F(103), 1.0)], {}, low=([(up(103.75), 1.0)], {})),
         lambda r: r["n_at_tol"] == 0 and score_at(r, up(103.75)) == [F(0)])
    # bpm_resolution below and above 0.5: the autocorrelation tolerance is max(res, 0.5)
    for res in (0.4, 2.0):
        cr = config(bpm_resolution=res)
        g = group(f"res={res}", cr)
        for s in (3, 4):
            case(g, f"generic {s}", _rand_track(cr, 40 + s, 20), lambda r: r is not None)
        # (an autocorrelation entry exactly at the tolerance is never the nearest: the grid covers
        # the range at a spacing of at most the tolerance; n_at_tol_ac stays 0 over the whole table)
        case(g, "peak one grid step from the query", track(cr, [(F(120), 1.0)], {120.0 + res: 1.0}),
             lambda r: r["bpm"] in (F(120), F(120 + res)) and r["n_at_tol_ac"] == 0)
    # ---- scoring over all variants: seed_only off, weights 0 and negative, the consensus bonus ----
    so = config(tempogram_band_seed_only=0)
    g = group("seed_only off", so)
    for s in (1, 2):
        case(g, f"generic {s}", _rand_track(so, 50 + s, 16), lambda r: r is not None)
    w0 = config(tempogram_band_seed_only=0, tempogram_mel_weight=0.0, tempogram_band_w_full=-0.5)
    g = group("weights 0 and negative", w0)
    for s in (1, 2):
        case(g, f"generic {s}", _rand_track(w0, 60 + s, 16), lambda r: r is not None)
    # supporting variants: 0, 1, 2 and 4 of the four auxiliary ones, and a value exactly at the threshold
    g = group("bonus", c)
    on, off = ([(F(120), 1.0), (F(97), 0.5)], {120.0: 1.0, 97.0: 0.5}), ([(F(97), 1.0), (F(120), 0.0)], {97.0: 1.0})
    for k in (0, 1, 2, 4):
        pv = {n: (on if i < k else off) for i, n in enumerate(VARIANTS[1:])}
        case(g, f"{k} supporting variants", track(c, *on, **pv), lambda r, k=k: r[f"sb{k}"] >= 1)
    thr = F(c.tempogram_band_support_threshold)
    at = ([(F(97), 1.0), (F(120), thr)], {97.0: 1.0})
    under = ([(F(97), 1.0), (F(120), dn(thr))], {97.0: 1.0})
    case(g, "support exactly at the threshold", track(c, *on, low=at, mid=at, high=off, mel=off), lambda r: r["sb2"] >= 1)
    case(g, "support one ulp under the threshold", track(c, *on, low=under, mid=under, high=off, mel=off),
         lambda r: r["sb2"] == 0 and r["sb0"] >= 1)
    # equal scores: a group at the top and one straddling top_n (the stable order is ascending BPM)
    g = group("ties", c, top_n=3, cand_cap=3)
    tie = [(F(b), 1.0) for b in (90, 100, 110, 130)]
    case(g, "equal scores at the top", track(c, tie, {float(b): 1.0 for b in (90, 100, 110, 130)}),
         lambda r: r["cands"][0, 1] == r["cands"][1, 1] == r["cands"][2, 1] == r["cands"][3, 1] > r["cands"][4, 1] and
         [float(q) for q in r["cands"][:4, 0]] == [90, 100, 110, 130])  # rows top_n - 1 and top_n tie; ascending BPM
    case(g, "generic", _rand_track(c, 77, 10), lambda r: r is not None)
    g = group("top_n above the unique count", n1, top_n=50, cand_cap=50)
    case(g, "single", track(n1, [(F(100), 1.0)], {100.0: 1.0}), lambda r: r["n_uniq"] == 1)
    g = group("cand_cap below top_n", c, top_n=10, cand_cap=4)
    case(g, "generic", _rand_track(c, 78, 10), lambda r: r["n_uniq"] > 10)
    # ---- present subsets: the full variant alone and every subset of the others ----
    for m in range(16):
        pres = (1,) + tuple((m >> i) & 1 for i in range(4))
        g = group(f"present={pres}", c, present=pres)
        for s in (1, 2):
            case(g, f"generic {s}", _rand_track(c, 90 + s, 12), lambda r: r is not None)
    # without a BandCfg: the full variant with weight 1, seed_only, no bonus
    nb = config(enable_tempogram_band_fusion=0, enable_tempogram_mel_novelty=0, tempogram_band_consensus_bonus=0.0)
    g = group("no BandCfg", nb, present=(1, 0, 0, 0, 0))
    case(g, "generic", _rand_track(nb, 5, 12), lambda r: r is not None)
    # ---- the gate: one narrow grid per base BPM, so the base estimate is the single peak ----
    for b in (55, 80, 170, 200):
        for x, lab in ((F(b), "at"), (dn(b), "below"), (up(b), "above")):
            cg = config(min_bpm=float(x), max_bpm=float(x) + 0.5, bpm_resolution=8.0)  # the grid is x alone
            g = group(f"gate {lab} {b}", cg)
            inside = 55 <= x <= 80 or 170 <= x <= 200
            case(g, f"base {lab} {b}", track(cg, [(x, 1.0)], {float(x): 1.0}),
                 lambda r, x=x, inside=inside: r["bpm"] == x and r["n_uniq"] == 1 and
                 bool(r["trap_low"] or r["trap_high"]) == inside)
    # family support at 0.90 of the base's exactly and under; weak by agreement and by confidence;
    # a supporting candidate ranked just inside and outside the gate's top_n (25)
    cgate = config(min_bpm=64.0, max_bpm=131.0)
    g = group("gate family", cgate)
    for which, base, other in (("s_2x", 65, 130), ("s_half", 130, 65)):
        at, under = family_flip(cgate, base, other)
        case(g, f"{which} at 0.90 of s_base", track(cgate, [(F(base), 1.0), (F(other), at)], {}),
             lambda r, base=base: r["bpm"] == base and r["family"] == 1)
        case(g, f"{which} one step under 0.90 of s_base", track(cgate, [(F(base), 1.0), (F(other), under)], {}),
             lambda r, base=base: r["bpm"] == base and r["family"] == 0)
    cw = config(min_bpm=84.0, max_bpm=100.0, bpm_resolution=16.0)
    g = group("gate weak", cw)
    # fold_into_trap: base x 2 in [170, 200]; weak by agree == 0 (no peaks agree) or by conf < 0.06
    case(g, "weak by agreement alone, folds into the trap", track(cw, [(F(90), 1.0), (F(95), 0.2)], {},
                                                               full=([(F(99), 1.0), (F(90), 0.9)], {})),
         lambda r: r["agree"] == 0 and r["conf"] >= F(0.06) and r["fold_into_trap"] and r["ambiguous"])
    case(g, "weak by confidence alone", track(cw, [(F(90), 1.0), (F(95), 0.97)], {}),
         lambda r: r["agree"] > 0 and r["conf"] < F(0.06) and r["fold_into_trap"])
    case(g, "not weak", track(cw, [(F(90), 1.0), (F(95), 0.2)], {}), lambda r: not r["weak"])
    cnf = config(min_bpm=100.0, max_bpm=116.0, bpm_resolution=16.0)
    g = group("gate weak, no fold", cnf)
    case(g, "weak by confidence, outside the fold", track(cnf, [(F(105), 1.0), (F(110), 0.97)], {}),
         lambda r: r["agree"] > 0 and r["conf"] < F(0.06) and not r["fold_into_trap"] and not r["ambiguous"])
    case(g, "weak by agreement, outside the fold", track(cnf, [(F(105), 1.0), (F(110), 0.2)], {},
                                                      full=([(F(115), 1.0), (F(105), 0.9)], {})),
         lambda r: r["agree"] == 0 and r["conf"] >= F(0.06) and not r["fold_into_trap"] and not r["ambiguous"])
    # a supporting candidate (the base's double) ranked last inside and first outside the gate's
    # top_n of 25: 30 FFT bins scored through the full variant, every one seeded by some variant's first 8
    cr = config(tempogram_band_consensus_bonus=0.0)
    g = group("gate rank", cr)
    bpms = [F(75)] + [F(b) for b in np.arange(61.3, 180.0, 4.1) if min(abs(b - 75), abs(b - 150), abs(b - 37.5)) > 3][:28]
    for k in (24, 25):
        vals = [F(1.0)] + [F(0.9 - 0.02 * i) for i in range(28)]
        pairs = list(zip(bpms, vals))
        pairs.insert(k, (F(150), F((float(pairs[k - 1][1]) + float(pairs[k][1])) / 2)))
        pv = {}
        for j, n in enumerate(VARIANTS):  # variant j leads with entries 8 j ... 8 j + 7 of the full list
            lead = pairs[8 * j:8 * j + 8] if j < 4 else pairs[22:30]
            rest = [q for q in pairs if not any(q[0] == l[0] for l in lead)]
            pv[n] = ([(b, F(2.0) if j else v) for b, v in lead] + [(b, v if not j else F(0.0)) for b, v in rest], {})
        pv["full"] = (pairs, {})
        case(g, f"the base's double ranked {k}", track(cr, [], {}, **pv),
             lambda r, k=k: r["bpm"] == 75 and r["cands"][k, 0] == 150 and (r["s_2x"] > 0) == (k == 24))
    return GROUPS
