"""The fingerprint request (include/stratum_hip.h, sdsp_fingerprint) written from the definition in
numpy f32 over key_timeline_ref.chroma_rows and sections_ref.cell_means, with the pair comparison by
plain Python loops.  Nothing here knows how the kernels split the work.
"""
import numpy as np

import key_timeline_ref as K
import sections_ref as S

f32 = np.float32
WORDS, MATCH = 1, 2
DEFAULTS = dict(cell_seconds=0.0, cell_samples=0, max_offset_words=16, min_overlap_words=32, max_ber=0.30,
                what=WORDS | MATCH)
MATCH_FIELDS = ("a", "b", "offset_words", "offset_samples", "bit_errors", "bits_compared", "ber")
MATCH_DTYPES = dict(a=np.uint64, b=np.uint64, offset_words=np.int32, offset_samples=np.int64, bit_errors=np.uint64,
                    bits_compared=np.uint64, ber=f32)


def plan(request, sample_rate, khop, stages_full=True, beat_rows=False, has_matches=True):
    """Cs of a request dict, or the reason it is refused as (status, reason)."""
    r = dict(DEFAULTS, **request)
    floats = [f32(r[k]) for k in ("cell_seconds", "max_ber")]
    if r["what"] == 0:
        return 1, "what == 0"
    if r["what"] & ~(WORDS | MATCH):
        return 1, "unknown bits"
    if (r["what"] & MATCH) and not has_matches:
        return 1, "no matches struct"
    if any(not np.isfinite(v) or v < 0 for v in floats):
        return 1, "float"
    if floats[1] > 1:
        return 1, "max_ber > 1"
    sec, smp = bool(floats[0] != 0), int(r["cell_samples"]) != 0
    if sec == smp:
        return 1, "both" if sec else "neither"
    if int(r["max_offset_words"]) > 255:
        return 1, "O"
    if sec:
        p = float(f32(floats[0] * f32(sample_rate)))
        Cs = int(p) if p < 2.0 ** 32 else 2 ** 32
    else:
        Cs = int(r["cell_samples"])
    if Cs >= 2 ** 31:
        return 1, "Cs >= 2^31"
    if Cs < khop or Cs == 0:
        return 1, "Cs too small"
    if not stages_full:
        return 1, "BPM only"
    if beat_rows:
        return 4, "beat rows"
    return Cs


def n_cells(F, khop, Cs):
    return (F * khop) // Cs


def cell_rows(rows, khop, Cs):
    """m (n_cells, 12): the sections request's fold over the key frames alone."""
    F = 0 if rows is None else int(np.asarray(rows).shape[0])
    n = n_cells(F, khop, Cs)
    return S.cell_means(rows, n, Cs, khop) if n else np.zeros((0, 12), f32)


def words_of(m):
    """The words (uint32) of the cell rows m (n_cells, 12)."""
    m = np.ascontiguousarray(m, f32).reshape(-1, 12)
    W = max(m.shape[0] - 2, 0)
    out = np.zeros(W, np.uint32)
    if W == 0:
        return out
    d = (m - np.roll(m, -1, axis=1)).astype(f32)  # d(c)[i] = m[c][i] - m[c][(i + 1) % 12]
    a = ((d[1:W + 1] - d[:W]).astype(f32) > 0)
    b = ((d[2:W + 2] - d[:W]).astype(f32) > 0)
    for i in range(12):
        out |= (a[:, i].astype(np.uint32) << np.uint32(i)) | (b[:, i].astype(np.uint32) << np.uint32(12 + i))
    return out


def count(A, B, o):
    """(e, n) of one offset, by the plain loop."""
    e = n = 0
    for p in range(max(0, -o), min(len(A), len(B) - o)):
        a, b = int(A[p]), int(B[p + o])
        if (a | b) != 0:
            n += 1
            e += bin(a ^ b).count("1")
    return e, n


def best_offset(A, B, O, min_overlap_words):
    """(o, e, n) of the best offset, or None without an eligible one."""
    need = max(int(min_overlap_words), 1)
    best = None
    for o in sorted(range(-O, O + 1), key=lambda v: (abs(v), v)):  # ties: the smaller |o|, then the negative one
        e, n = count(A, B, o)
        if n < need:
            continue
        if best is None or e * best[2] < best[1] * n:
            best = (o, e, n)
    return best


def ber(e, n):
    return f32(f32(e) / f32(24 * n))


def pair_records(words, O, min_overlap_words):
    """(T, T) arrays o, has, e, n as sdsp_debug_fingerprint_match returns them."""
    T = len(words)
    rec = {k: np.zeros((T, T), np.int64) for k in ("offset_words", "eligible", "bit_errors", "positions")}
    for a in range(T):
        for b in range(a + 1, T):
            r = best_offset(words[a], words[b], O, min_overlap_words)
            if r is not None:
                rec["offset_words"][a, b], rec["eligible"][a, b] = r[0], 1
                rec["bit_errors"][a, b], rec["positions"][a, b] = r[1], r[2]
    return rec


def match_list(words, status, first, Cs, request, rec=None):
    """The call's sdsp_fingerprint_matches as a dict, and n_matches per track, from every track's
    words (None or empty: not compared), status and first_sample.  rec: pair_records() of the same
    words and request, when the caller already has them."""
    r = dict(DEFAULTS, **request)
    T = len(words)
    who = [t for t in range(T) if status[t] == 0 and words[t] is not None and len(words[t]) >= 1]
    rows = {k: [] for k in MATCH_FIELDS}
    n_matches = [0] * T
    for i, a in enumerate(who):
        for b in who[i + 1:]:
            if rec is not None:
                got = (int(rec["offset_words"][a, b]), int(rec["bit_errors"][a, b]), int(rec["positions"][a, b])) \
                    if rec["eligible"][a, b] else None
            else:
                got = best_offset(words[a], words[b], int(r["max_offset_words"]), int(r["min_overlap_words"]))
            if got is None:
                continue
            o, e, n = got
            if not ber(e, n) <= f32(r["max_ber"]):
                continue
            for k, v in zip(MATCH_FIELDS, (a, b, o, (first[b] + o * Cs) - first[a], e, 24 * n, ber(e, n))):
                rows[k].append(v)
            n_matches[a] += 1
            n_matches[b] += 1
    nc = len(who)
    return dict(n_compared=nc, n_pairs=nc * (nc - 1) // 2, n_matches=len(rows["a"]),
                matches={k: np.array(rows[k], MATCH_DTYPES[k]) for k in MATCH_FIELDS}), n_matches


def track_words(x, sample_rate, cfg, Cs):
    """(status, first_sample, n_cells, words) of one track from the oracle's chain; words is None
    when the key path does not run."""
    status, first, rows = K.chroma_rows(x, sample_rate, cfg)
    if status != 0 or rows is None:
        return status, first if status == 0 else 0, 0, None
    _, khop = K.key_stft(cfg)
    m = cell_rows(rows, khop, Cs)
    return 0, first, int(m.shape[0]), words_of(m)


def fingerprint_ref(xs, sample_rate, cfg, request, chains=None):
    """What sdsp.analyze_batch_device_with(..., fingerprint=...) returns last for the tracks xs: a
    dict of `fingerprints` and `matches`.  chains: track_words() results to share between tests."""
    r = dict(DEFAULTS, **request)
    _, khop = K.key_stft(cfg)
    Cs = plan(r, sample_rate, khop)
    chains = chains if chains is not None else [track_words(x, sample_rate, cfg, Cs) for x in xs]
    status = [c[0] for c in chains]
    words = [c[3] if c[0] == 0 else None for c in chains]
    first = [c[1] for c in chains]
    if r["what"] & MATCH:
        ml, nm = match_list(words, status, first, Cs, r)
    else:
        ml, nm = dict(n_compared=0, n_pairs=0, n_matches=0, matches={k: np.zeros(0, MATCH_DTYPES[k]) for k in MATCH_FIELDS}), \
            [0] * len(xs)
    prints = []
    for t, c in enumerate(chains):
        w = words[t] if words[t] is not None else np.zeros(0, np.uint32)
        ok = c[0] == 0
        prints.append(dict(status=c[0], n_cells=c[2] if ok else 0, n_words=int(w.size) if ok else 0, cell_samples=Cs,
                           first_sample=c[1] if ok and words[t] is not None else 0, n_matches=nm[t],
                           words=w if (r["what"] & WORDS) and ok else np.zeros(0, np.uint32)))
    return dict(fingerprints=prints, matches=ml)


def assert_equal(got, want, what=""):
    """Every integer equal, every array equal, ber on its uint32 view."""
    assert len(got["fingerprints"]) == len(want["fingerprints"]), what
    for t, (g, w) in enumerate(zip(got["fingerprints"], want["fingerprints"])):
        for k in ("status", "n_cells", "n_words", "cell_samples", "first_sample", "n_matches"):
            assert g[k] == w[k], (what, t, k, g[k], w[k])
        S.assert_arrays_equal(g["words"], w["words"], (what, t, "words"))
    gm, wm = got["matches"], want["matches"]
    for k in ("n_compared", "n_pairs", "n_matches"):
        assert gm[k] == wm[k], (what, k, gm[k], wm[k])
    for k in MATCH_FIELDS:
        S.assert_arrays_equal(gm["matches"][k], wm["matches"][k], (what, "matches", k))


# ---- the synthetic material of the separation experiment ----
def random_triads(seed, seconds, sample_rate=44100, level=0.2):
    """Non-repeating random triads from key_timeline_ref.cadence's notes (four decaying harmonics per
    note around middle C, a short attack and an exponential decay), each chord on a random root, major
    or minor, 0.25, 0.5, 0.75 or 1.0 s long, never the chord before it again."""
    rng = np.random.RandomState(seed)
    out = np.zeros(int(seconds * sample_rate), np.float64)
    at, last = 0, None
    while at < out.size:
        root, minor = int(rng.randint(12)), bool(rng.randint(2))
        n_chord = int((0.25, 0.5, 0.75, 1.0)[int(rng.randint(4))] * sample_rate)
        if (root, minor) == last:
            continue
        last = (root, minor)
        t = np.arange(n_chord, dtype=np.float64) / sample_rate
        env = np.minimum(t / 0.01, 1.0) * np.exp(-3.0 * t)
        x = np.zeros(n_chord)
        for semis in (0, 3 if minor else 4, 7):
            pc = (root + semis) % 12
            f0 = 261.6255653005986 * 2.0 ** ((pc + (0 if pc < 6 else -12)) / 12.0)
            for h in range(1, 5):
                x += np.sin(2.0 * np.pi * f0 * h * t) / h
        seg = out[at:at + n_chord]
        seg += (x * env)[:seg.size]
        at += n_chord
    return (out * (level / 3.0)).astype(f32)


def with_noise(x, db_below, seed):
    """x plus white noise whose RMS lies db_below dB under x's."""
    rng = np.random.RandomState(seed)
    rms = np.sqrt(np.mean(x.astype(np.float64) ** 2))
    return (x + rng.standard_normal(x.size) * rms * 10.0 ** (-db_below / 20.0)).astype(f32)
