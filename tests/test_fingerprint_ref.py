"""tests/fingerprint_ref.py itself (CPU): the refusal table, the zero-sum property of a word, the tie
rule, and the separation experiment the header's "what the numbers are" rests on.
"""
import numpy as np
import pytest

import fingerprint_ref as R
import oracle

SR = 44100
f32 = np.float32


def test_refusal_table():
    ok = dict(cell_samples=5512)
    assert R.plan(ok, SR, 512) == 5512
    assert R.plan(dict(cell_seconds=0.125), SR, 512) == 5512
    assert R.plan(dict(cell_samples=512), SR, 512) == 512 and R.plan(dict(cell_samples=2 ** 31 - 1), SR, 512) == 2 ** 31 - 1
    assert R.plan(dict(ok, max_offset_words=255, max_ber=1.0, min_overlap_words=0), SR, 512) == 5512
    assert R.plan(dict(ok, what=R.WORDS), SR, 512, has_matches=False) == 5512
    bad = [dict(ok, what=0), dict(ok, what=4), dict(ok, what=7), dict(), dict(cell_seconds=0.125, cell_samples=5512),
           dict(cell_seconds=float("nan")), dict(cell_seconds=float("inf")), dict(cell_seconds=-0.125),
           dict(ok, max_ber=float("nan")), dict(ok, max_ber=-0.1), dict(ok, max_ber=1.5), dict(cell_samples=511),
           dict(cell_samples=2 ** 31), dict(cell_seconds=1e9), dict(ok, max_offset_words=256)]
    for r in bad:
        assert R.plan(r, SR, 512)[0] == 1, r
    assert R.plan(ok, SR, 512, has_matches=False)[0] == 1
    assert R.plan(ok, SR, 512, stages_full=False)[0] == 1
    assert R.plan(ok, SR, 512, beat_rows=True)[0] == 4
    assert R.plan(dict(cell_samples=4096), SR, 8192)[0] == 1  # Cs < khop


def test_a_word_is_zero_exactly_where_the_chroma_did_not_move():
    rng = np.random.RandomState(5)
    m = rng.rand(40, 12).astype(f32)
    m[10:16] = m[10]          # a held constant
    m[25:31] = 0              # silence
    w = R.words_of(m)
    assert w.size == 38 and (w >> np.uint32(24)).max() == 0
    d = (m - np.roll(m, -1, axis=1)).astype(f32)
    for k in range(w.size):
        if (int(w[k]) & 0xFFF) == 0:  # bits 0 to 11 all clear: the twelve differences sum to zero, so none is negative either
            assert np.array_equal(d[k + 1], d[k]), k
    assert np.all(w[10:14] == 0) and np.all(w[25:29] == 0)
    assert np.count_nonzero(w) == w.size - 8
    # gain invariance: a power of two scales every difference exactly
    assert np.array_equal(R.words_of((m * f32(0.5)).astype(f32)), w)
    for n in (0, 1, 2):
        assert R.words_of(m[:n]).size == 0
    assert R.words_of(m[:3]).size == 1


def test_tie_rule_and_eligibility_on_hand_made_words():
    # a periodic array against itself: e = 0 at every multiple of the period, the best is o = 0
    A = np.array([1, 2, 4, 8] * 8, np.uint32)
    assert R.best_offset(A, A, 8, 1) == (0, 0, 32)
    assert R.count(A, A, 4) == (0, 28) and R.count(A, A, -4) == (0, 28)
    # B is A moved by two words either way at once: -2 and +2 tie, the negative one wins
    A = np.array([0, 0, 5, 0, 0], np.uint32)
    B = np.array([5, 0, 0, 0, 5], np.uint32)
    assert R.count(A, B, -2) == R.count(A, B, 2) == (0, 1)
    assert R.best_offset(A, B, 2, 1) == (-2, 0, 1)
    # zeros against zeros are not counted; zeros against non-zeros are
    Z = np.zeros(6, np.uint32)
    assert R.best_offset(Z, Z, 3, 0) is None and R.best_offset(Z, Z, 3, 1) is None
    N = np.array([3, 0, 3, 0, 3, 0], np.uint32)
    assert R.count(Z, N, 0) == (6, 3)
    # min_overlap_words around n(o)
    assert R.best_offset(Z, N, 0, 3) == (0, 6, 3) and R.best_offset(Z, N, 0, 4) is None
    # the fraction rule: 1/3 beats 2/5 whatever the order
    assert 1 * 5 < 2 * 3
    assert R.ber(6, 3) == f32(f32(6) / f32(72))


_SEP = {}


def separation(Cs=5512):
    """The experiment's tracks and words, computed once: name -> (track, words)."""
    if Cs not in _SEP:
        cfg = oracle.default_config()
        x1 = R.random_triads(1, 24.0)
        xs = dict(original=x1, copy=x1.copy(), gain=(x1 * f32(0.5)).astype(f32), noise30=R.with_noise(x1, 30, 11),
                  noise20=R.with_noise(x1, 20, 12), cut1000=x1[1000:], cut2756=x1[2756:], cut5512=x1[5512:],
                  cut22350=x1[22350:], seed2=R.random_triads(2, 24.0), seed3=R.random_triads(3, 24.0))
        _SEP[Cs] = {k: (x, R.track_words(x, SR, cfg, Cs)) for k, x in xs.items()}
    return _SEP[Cs]


EXPECTED_OFFSET = dict(copy=0, gain=0, noise30=0, noise20=0, cut1000=0, cut2756=0, cut5512=-1, cut22350=-4)


def test_separation_of_duplicates_from_unrelated_tracks():
    """24 s of non-repeating random triads (fingerprint_ref.random_triads, seeds 1, 2, 3), default
    configuration, Cs = 5512, O = 16, min_overlap_words = 32, max_ber = 0.30: every variant of track 1
    matches it at the stated offset, seeds 2 and 3 match nothing.

    Measured here (best BER, offset in words):
      identical copy 0.000 (0), 0.5x gain 0.000 (0), noise 30 dB below 0.151 (0), noise 20 dB below
      0.194 (0), first 1,000 samples cut 0.033 (0), 2,756 cut 0.088 (0), 5,512 cut 0.010 (-1),
      22,350 cut 0.016 (-4); seed 2 against track 1 0.460, seed 3 0.478; the nearest wrong offset of
      a duplicate at least 0.164.  At Cs = 11025: duplicates at most 0.171, unrelated at least 0.442.
    The offsets are the issue's; the BERs differ from its table by up to 0.02 (0.164 / 0.207 there for
    the two noise levels, 0.049 / 0.104 / 0.013 / 0.020 for the cuts): the generator is rebuilt from its
    description (the chord sequence and the noise are this file's seeds), nothing was tuned.
    """
    sep = separation()
    names = list(sep)
    words = [sep[k][1][3] for k in names]
    status = [sep[k][1][0] for k in names]
    first = [sep[k][1][1] for k in names]
    assert status == [0] * len(names) and all(w.size >= 180 for w in words)
    ml, nm = R.match_list(words, status, first, 5512, dict(max_offset_words=16, min_overlap_words=32, max_ber=0.30))
    got = {(int(a), int(b)): (int(o), float(x)) for a, b, o, x in
           zip(ml["matches"]["a"], ml["matches"]["b"], ml["matches"]["offset_words"], ml["matches"]["ber"])}
    for k, o in EXPECTED_OFFSET.items():
        j = names.index(k)
        assert (0, j) in got, (k, R.best_offset(words[0], words[j], 16, 32))
        assert got[(0, j)][0] == o, (k, got[(0, j)])
        print(k, got[(0, j)])
    for k in ("seed2", "seed3"):
        j = names.index(k)
        assert nm[j] == 0, (k, [p for p in got if j in p])
        print(k, R.best_offset(words[0], words[j], 16, 32))
    assert ml["n_compared"] == len(names) and ml["n_pairs"] == len(names) * (len(names) - 1) // 2
    # offset_samples: what was cut from b's start, to within a cell
    j = names.index("cut22350")
    k = int(np.flatnonzero((ml["matches"]["a"] == 0) & (ml["matches"]["b"] == j))[0])
    assert abs(int(ml["matches"]["offset_samples"][k]) + 22350) <= 5512
