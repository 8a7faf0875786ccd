"""Inputs of the multi-resolution fusion's stage tests (tests/test_tempo_decision_cases.py on the
CPU, tests/test_gpu_multires_stages.py on the GPU): candidate lists, hop-512 novelty curves and base
estimates built directly, no audio.

A candidate list is what the selection emits: rows (bpm, score, fft_norm, autocorr_norm) sorted by
score descending; None stands for a hop whose tempogram failed.  Every case names the branch or
boundary it is for and carries a check on the oracle's branch record (units.multires_fuse).  Cases
with the same configuration (cfg_key) and sample rate form one probe call.

One case a reader may look for cannot exist: a fold-down result that is folded up again.  Fold-down
needs best >= 170, so its result is >= 85, above fold-up's limit of 80; the table holds the lowest
result (85) and checks that the fold-up gate is not reached.
"""
import numpy as np

import oracle

F = np.float32


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


def cl(*pairs):
    """A candidate list from (bpm, score) pairs, sorted by score descending (stable)."""
    a = np.zeros((len(pairs), 4), F)
    for i, (b, s) in enumerate(pairs):
        a[i, 0], a[i, 1] = F(b), F(s)
    return a[np.argsort(-a[:, 1], kind="stable")] if len(pairs) else a


def noise(seed, n):
    return (np.random.default_rng(seed).random(n) ** 2).astype(F)


def period(sr, bpm):
    """beat_contrast's period in hop-512 frames."""
    return int(np.rint(F(F(60.0) * F(sr)) / F(F(bpm) * F(512.0))))


def boundary_curve(seed, n, seg, P):
    """Noise with large values within P frames of every multiple of `seg` (the segment ends of the
    kernel's staged walk), so a wrong halo or restart changes the result."""
    x = noise(seed, n) * F(0.1)
    rng = np.random.default_rng(seed + 1)
    for s in range(seg, n + seg, seg):
        for i in range(max(s - P, 0), min(s + P, n)):
            x[i] = F(1.0 + rng.random())
    return x


def segment_curve(seed, n, trains):
    """A curve around 1 with noise, large values within a period of every staging-segment end of each
    train's period, and per train (P, height) a pulse every P frames, phased so that a beat falls a
    quarter period before the first segment end: its half- and third-beat lookups land past it."""
    x = F(1.0) + noise(seed, n) * F(0.1)
    rng = np.random.default_rng(seed + 1)
    for P, _ in trains:
        seg = 4096 - P
        for s in range(seg, n + seg, seg):
            for i in range(max(s - P, 0), min(s + P, n)):
                x[i] = F(1.0 + rng.random())
    for P, h in trains:
        x[(4096 - P - 1 - P // 4) % P::P] += F(h)
    return x


def crosses(ph, P, n):
    """Whether phase ph of period P, over n frames, has a beat whose half- or third-beat lookup lies
    in the next staging segment (segments of 4096 - P frames): the kernel reads it from the halo."""
    seg = 4096 - P
    for i in range(ph, n, P):
        s1 = (i // seg + 1) * seg
        offs = ([P // 2] if P >= 6 else []) + ([P // 3, (2 * P) // 3] if P >= 9 else [])
        if any(s1 <= i + o < n for o in offs):
            return True
    return False


BASE = (F(100.0), F(0.5), 1, 0, 0)  # bpm, conf, agree, trap_low, trap_high
CASES = []


def case(name, c512, c256=(), c1024=(), nov=None, base=BASE, cfg=None, sr=44100, check=None, cfg_key="default"):
    ls = [None if c is None else (c if isinstance(c, np.ndarray) else cl(*c)) for c in (c256, c512, c1024)]
    CASES.append(dict(name=name, c256=ls[0], c512=ls[1], c1024=ls[2], nov=noise(1, 400) if nov is None else np.asarray(nov, F),
                      base=base, cfg=cfg if cfg is not None else config(), sr=sr, check=check, cfg_key=cfg_key))


def three(*pairs):
    """The same list at every hop."""
    return dict(c512=pairs, c256=pairs, c1024=pairs)


# the family of 120 BPM: 120, 180, 80, 160, 90, every member supported at all three hops
FAM5 = [(120, 0.9), (180, 0.5), (80, 0.5), (160, 0.5), (90, 0.5)]


def accept_flip(ratio, mr_bpm):
    """The adjacent f32 base BPMs between which |rel - ratio| < 0.05 flips on each side of `ratio`
    (rel = max(mr / base, base / mr) in f32): [(inside, outside), (inside, outside)]."""
    def fam(b):
        rel = max(F(F(mr_bpm) / b), F(b / F(mr_bpm)))
        return abs(F(rel - F(ratio))) < F(0.05)

    out = []
    for edge in (ratio + 0.05, ratio - 0.05):
        b = F(mr_bpm / edge)
        lo, hi = dn(b, 64), up(b, 64)
        assert fam(lo) != fam(hi)
        while up(lo) < hi:
            mid = F((np.float64(lo) + np.float64(hi)) / 2)
            mid = mid if lo < mid < hi else up(lo)
            lo, hi = (mid, hi) if fam(mid) == fam(lo) else (lo, mid)
        out.append((lo, hi) if fam(lo) else (hi, lo))
    return out


def build():
    CASES.clear()
    one = [(100, 0.8)]
    # ---- a failed hop in each position; no hypotheses ----
    case("hop 256 failed", one, c256=None, c1024=one, check=lambda r: not r["ok"])
    case("hop 512 failed", None, c256=one, c1024=one, check=lambda r: not r["ok"])
    case("hop 1024 failed", one, c256=one, c1024=None, check=lambda r: not r["ok"])
    case("every candidate out of range or not positive", [(500, 0.9), (0, 0.5), (19, 0.4)],
         check=lambda r: not r["ok"] and r["n_hyps"] == 0)
    case("plain: one candidate at every hop", **three((100, 0.8)), check=lambda r: r["ok"] and r["agree"] == 3 and r["conf"] == 1)
    # ---- the structural discounts, each alone ----
    case("1.02 alone (double time)", [(100, 0.5)], c256=[(100, 0.3), (200, 0.5)], c1024=[(100, 0.5), (200, 0.1), (50, 0.6)],
         check=lambda r: (r["n_2t102"], r["n_h102"], r["n_r2_110"], r["n_rh_110"]) == (1, 0, 0, 0))
    case("1.02 alone (half time)", [(100, 0.5)], c256=[(100, 0.3), (200, 0.5)], c1024=[(100, 0.5), (200, 0.6)],
         check=lambda r: r["n_h102"] == 1 and r["n_2t102"] == 0 and r["n_r2_110"] == 0)
    case("1.10 alone", [(100, 0.5)], c256=[(100, 0.5), (200, 0.52)], c1024=[(100, 0.5), (200, 0.5), (50, 0.6)],
         check=lambda r: (r["n_r2_110"], r["n_r2_100"], r["n_2t102"], r["n_h102"], r["n_rh_110"]) == (1, 0, 0, 0, 0))
    case("1.00 (and with it 1.10)", [(100, 0.5)], c256=[(100, 0.5), (200, 0.4)], c1024=[(100, 0.5), (200, 0.5), (50, 0.6)],
         check=lambda r: (r["n_r2_110"], r["n_r2_100"]) == (1, 1) and r["n_rh_110"] == 0)
    case("half-time ratio under 1.10 and under 1.00", [(100, 0.5)], c1024=[(100, 0.5), (50, 0.52)],
         check=lambda r: r["n_rh_110"] == 1 and r["n_rh_100"] == 0)
    case("no aux lists: both ratios are 1", [(100, 0.5)], check=lambda r: (r["n_r2_110"], r["n_rh_110"], r["n_r2_100"]) == (1, 1, 0))
    # ---- the band penalties at 210, 180 and 60 and an ulp either side ----
    for t, pens in ((F(210), (0, 1, 0)), (up(210), (1, 0, 0)), (dn(210), (0, 1, 0)), (F(180), (0, 0, 0)),
                    (up(180), (0, 1, 0)), (dn(180), (0, 0, 0)), (F(60), (0, 0, 0)), (dn(60), (0, 0, 1)), (up(60), (0, 0, 0))):
        case(f"band penalty at {float(t)!r}", [(t, 0.7)],
             check=lambda r, pens=pens, t=t: (r["n_pen210"], r["n_pen180"], r["n_pen60"]) == pens and r["bpm"] == t)
    # ---- the margin, the anchor reset and the human prior ----
    tiny = config(min_bpm=0.0001)
    for t, reset in ((F(0.002), 0), (up(0.002), 1)):  # |t / 2 - t| is exactly 1e-3f, then one ulp more
        case(f"margin low, |cb - t| at 1e-3 ({'reset' if reset else 'kept'})", [(t, 0.5)],
             c1024=[(F(t * F(0.5)), 0.3), (t, 0.1)], cfg=tiny, cfg_key="tiny",
             check=lambda r, reset=reset: r["n_margin_lo"] == 1 and r["n_reset"] == reset)
    case("margin above the threshold: the half-time hypothesis stands", [(100, 0.5)], c1024=[(50, 0.9), (100, 0.05)],
         check=lambda r: r["n_margin_lo"] == 0 and r["n_reset"] == 0 and r["n_hyps"] == 1)
    case("margin below the threshold: back to the anchor", [(100, 0.5)], c1024=[(50, 0.3), (100, 0.1)],
         check=lambda r: r["n_reset"] == 1 and r["bpm"] == 100)
    prior = config(tempogram_multi_res_use_human_prior=1)
    for t, inside in ((F(70), 1), (dn(70), 0), (F(180), 1), (up(180), 0)):
        for cfg, key, on in ((prior, "prior", 1), (None, "default", 0)):
            case(f"human prior {'on' if on else 'off'} at {float(t)!r}", [(t, 0.2)], cfg=cfg, cfg_key=key,
                 check=lambda r, want=inside * on, t=t: r["n_prior"] == want and r["n_margin_lo"] == 1 and r["bpm"] == t)
    # ---- the dedupe: duplicates within 0.75, the cap of 8 distinct hypotheses ----
    case("duplicate hypotheses within 0.75", [(100, 0.8), (100.5, 0.7), (130, 0.5)],
         check=lambda r: r["n_hyps"] == 3 and r["n_dup"] == 1 and r["n_uniq"] == 2)
    case("exactly 0.75 apart: both kept", [(100, 0.8), (100.75, 0.7)], check=lambda r: r["n_dup"] == 0 and r["n_uniq"] == 2)
    ten = [(b, 0.9 - 0.03 * i) for i, b in enumerate((83, 89, 97, 101, 107, 113, 127, 131, 137, 149))]
    case("ten distinct hypotheses: the cap of 8", ten, check=lambda r: r["n_hyps"] == 10 and r["n_uniq"] == 8)
    # ---- fold-down (best >= 170, half in [70, 120]): agreement 2 and 3, support ratio at 0.45 ----
    tn = F(2.0 ** -40)
    q45 = F(0.45)
    for lab, half, want in (("ratio at 0.45", q45, 8), ("ratio one ulp under 0.45", dn(q45), 7)):
        case(f"fold-down, three hops, {lab}", [(180, 0.5), (90, half)], c256=[(180, 0.25), (90, tn)],
             c1024=[(180, 0.25), (90, tn)],
             check=lambda r, want=want: r["fd_eval"] == want and r["fd"] == (want == 8) and r["fd_eval_a1"] == 3)
    case("fold-down refused: the half at two hops only", [(180, 0.9), (90, 0.7)], c256=[(180, 0.9), (90, 0.7)], c1024=[(180, 0.9)],
         check=lambda r: r["fd_eval"] == 1 + 2 + 1 and r["fd_eval_a1"] == 2 and not r["fd"])
    case("fold-down to the lowest half (85): a folded value is never folded up again", **three((170, 0.5), (85, 0.4)),
         check=lambda r: r["fd"] == 1 and r["fd_to"] == 85 and r["fu_eval"] == 0)
    # ---- fold-up (best <= 80, double in [70, 180]): agreement 1 and 2, support ratio at 0.55 ----
    q55 = F(0.55)
    for lab, dbl, want in (("ratio at 0.55", q55, 8), ("ratio one ulp under 0.55", dn(q55), 7)):
        case(f"fold-up, two hops, {lab}", [(60, 0.5), (120, dbl)], c256=[(60, 0.5), (120, tn)],
             check=lambda r, want=want: r["fu_eval"] == want and r["fu"] == (want == 8) and r["fu_eval_a1"] == 2)
    case("fold-up refused: the double at one hop only", [(60, 0.5), (120, 0.6)], c256=[(60, 0.5)],
         check=lambda r: r["fu_eval"] == 1 + 2 + 1 and r["fu_eval_a1"] == 1 and not r["fu"])
    # ---- the triplet family: 0, 1, 2 and 5 members, max_alt at 0.45 ----
    case("family of 0: the best at one hop only", [(120, 0.9)], check=lambda r: r["n_fam"] == 0)
    case("family of 1", **three((120, 0.9)), check=lambda r: r["n_fam"] == 1 and not r["fam_eval"])
    case("family of 2, max_alt at 0.45", [(120, 0.5), (180, q45)], c256=[(120, 0.5), (180, tn)],
         check=lambda r: r["n_fam"] == 2 and r["max_alt"] == q45 and r["fam_eval"] == 1)
    case("family of 2, max_alt one ulp under 0.45", [(120, 0.5), (180, dn(q45))], c256=[(120, 0.5), (180, tn)],
         check=lambda r: r["n_fam"] == 2 and r["max_alt"] == dn(q45) and r["fam_eval"] == 0)
    spikes = np.zeros(1200, F)
    spikes[::43] = 1.0  # a pulse every 43 frames: 120 BPM at 44.1 kHz
    case("family of 5, the chosen member is the current best", **three(*FAM5), nov=spikes,
         check=lambda r: r["n_fam"] == 5 and r["fam_eval"] == 1 and r["chosen"] == 0 and not r["tf"])
    sp29 = np.zeros(1200, F)
    sp29[::29] = 1.0  # a pulse every 29 frames (180 BPM) under a best of 120: the switch is taken
    case("family of 5, triplet switch taken", **three(*FAM5), nov=sp29,
         check=lambda r: r["n_fam"] == 5 and r["tf"] == 1 and r["tf_to"] == 180 and r["tf_label"] == 1)
    case("family over an all-zero novelty: the 1e-6 floors", **three(*FAM5), nov=np.zeros(500, F),
         check=lambda r: r["fam_eval"] == 1 and not r["fam_align"].any() and r["cur_align"] == 0)
    # the chosen member's alignment exactly at the current one + 0.40, and under it.  At 384 kHz the
    # best (80 BPM) has a period above 512, so its alignment is 0; the other member (120 BPM, period
    # 375) sees a curve of ones with a pulse of height v every 375 frames, whose contrast over the
    # mean is 0.4f exactly at v = 0x3fb3420c over 6,007 frames (found by stepping v through the
    # oracle) and 0.39999965 one ulp below
    v_at = np.array([0x3FB3420C], np.uint32).view(F)[0]
    for v, lab, want in ((v_at, "exactly at", 1), (dn(v_at), "one step under", 0)):
        x = np.ones(6007, F)
        x[::375] = v
        case(f"family of 2, alignment {lab} the current one + 0.40", **three((80, 0.9), (120, 0.5)), nov=x, sr=384000,
             check=lambda r, want=want: r["n_fam"] == 2 and r["cur_align"] == 0 and r["tf"] == want and
             (r["fam_align"][1] == F(0.4)) == bool(want) and r["fam_align"][1] > F(0.3999))
    # ---- novelty lengths: under 16 frames, and around the 4096-frame staging segment ----
    for n in (15, 16):
        case(f"novelty of {n} frames", **three(*FAM5), nov=noise(n, n),
             check=lambda r, n=n: r["fam_eval"] == 1 and bool(r["fam_align"].any()) == (n == 16))
    # The staging segment of a member with period P is 4096 - P frames.  Lengths: one segment - 1, one
    # segment, + 1, two segments and a frame, 3.5 segments, for the members with the longest (65) and
    # the shortest (29) period at 44.1 kHz, each once as the chosen member and once as the current
    # best of a family of two.  The triplet switch is taken in every case, so both alignments come
    # back in tf_al0 / tf_al1 and are compared bit for bit; both lie inside the +-10 clamp, and the
    # pulse trains make the winning phases the ones that read across the segment ends.
    for best, other in ((120, 80), (80, 120), (120, 180), (180, 120)):
        P = period(44100, 80 if 80 in (best, other) else 180)
        seg = 4096 - P
        for n in (seg - 1, seg, seg + 1, 2 * seg + 1, int(3.5 * seg)):
            Pb, Po = period(44100, best), period(44100, other)
            case(f"best {best}, chosen {other}: novelty of {n} frames (segments of {seg})",
                 **three((best, 0.9), (other, 0.5)), nov=segment_curve(n, n, ((Pb, 1.5), (Po, 4.0))),
                 check=lambda r, best=best, other=other, n=n, seg=seg, Pb=Pb, Po=Po: r["n_fam"] == 2 and r["tf"] == 1 and
                 r["tf_from"] == best and r["tf_to"] == other and abs(r["tf_al0"]) < 10 and abs(r["tf_al1"]) < 10 and
                 (n <= seg + 1 or (crosses(r["cur_phase"], Pb, n) and crosses(r["fam_phase"][r["chosen"]], Po, n))))
    # ---- sample rates: periods under 6, 6-8, 9 and above; above 64; around the 512 cap ----
    lo = {b: period(8000, b) for b in (120, 180, 80, 160, 90)}
    assert lo[180] < 6 <= lo[160] <= 8 < lo[90] and period(44100, 80) > 64
    case("8 kHz: periods 5 to 12", **three(*FAM5), nov=noise(5, 700), sr=8000, check=lambda r: r["fam_eval"] == 1)
    assert period(384000, 80) > 512 >= period(384000, 90) > 448
    case("384 kHz: periods around the 512 cap", **three(*FAM5), nov=boundary_curve(9, 9000, 4096 - 500, 500), sr=384000,
         check=lambda r: r["fam_eval"] == 1 and r["fam_align"][2] == 0 and r["fam_align"][4] != 0)
    # ---- the hypothesis array: top_k of 1, 25, 64, 65, 100 with at least top_k scorable candidates;
    # the strongest support sits behind the last candidates, so a cut list changes the result ----
    for k in (1, 25, 64, 65, 100):
        bp = [F(41 + 1.9 * i) for i in range(k + 3)]
        c512 = [(b, 0.9 - 0.005 * i) for i, b in enumerate(bp)]
        tail = [(bp[j], 1.0 - 0.1 * (k - 1 - j)) for j in range(max(k - 3, 0), k)]
        case(f"top_k {k}: {k} hypotheses", c512, c256=tail, c1024=tail, cfg=config(tempogram_multi_res_top_k=k),
             cfg_key=f"top_k={k}", check=lambda r, k=k: r["n_hyps"] == k)
        if k > 64:
            CASES[-1]["cut"] = 64  # the first 64 candidates alone give another estimate
    # top_k 300 over a 257-candidate hop-512 list: the list stays in global memory
    bp = [F(40 + 0.778 * i) for i in range(257)]
    case("top_k 300, 257 candidates", [(b, 0.9 - 0.003 * i) for i, b in enumerate(bp)], c256=[(bp[256], 1.0)], c1024=[(bp[256], 1.0)],
         cfg=config(tempogram_multi_res_top_k=300), cfg_key="top_k=300",
         check=lambda r: r["n_hyps"] == 257)
    # ---- the acceptance ----
    two = [(100, 1.0), (130, 0.2)]  # conf 0.8, agreement 1 at hop 512 alone
    case("accepted by confidence alone", [(100, 0.8)], base=(F(100), F(0.5), 3, 0, 0), check=lambda r: r["clause"] == 1 and r["used"])
    case("accepted by agreement alone", **three((100, 0.8)), base=(F(100), F(1.0), 0, 0, 0),
         check=lambda r: r["clause"] == 2 and r["used"])
    case("accepted by the trap-zone family alone", two, base=(F(66.5), F(0.9), 1, 1, 0),
         check=lambda r: r["clause"] == 4 and r["used"] and r["fam"])
    case("not accepted: the uploaded estimate comes back", two, base=(F(100), F(0.9), 1, 0, 0),
         check=lambda r: r["clause"] == 0 and not r["used"])
    case("forbidden: base at 180, estimate above", [(190, 0.8)], base=(F(180), F(0.1), 0, 1, 0),
         check=lambda r: r["forbid"] and r["clause"] and not r["used"])
    case("not forbidden: base one ulp above 180", [(190, 0.8)], base=(up(180), F(0.1), 0, 1, 0),
         check=lambda r: not r["forbid"] and r["used"])
    case("base BPM 0: rel is 1", [(100, 0.8)], base=(F(0), F(0.5), 3, 0, 0), check=lambda r: r["rel"] == 1 and r["used"])
    # rel at 2, 3/2 and 4/3 +- 0.05, from both sides: adjacent base BPMs in a trap zone whose estimate
    # (conf 0.8 against a base of 0.9, equal agreement) is accepted through the family clause alone
    for ratio, mr in ((2.0, 130.0), (1.5, 110.0), (4.0 / 3.0, 100.0)):
        for inside, outside in accept_flip(ratio, mr):
            for b, want in ((inside, 1), (outside, 0)):
                case(f"rel around {ratio:.3f}: base {float(b)!r}", [(mr, 1.0), (mr * 1.37, 0.2)], base=(b, F(0.9), 1, 1, 0),
                     check=lambda r, want=want, mr=mr: r["bpm"] == F(mr) and r["fam"] == want and r["used"] == want)
    return CASES
