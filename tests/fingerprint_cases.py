"""Small shapes of the fingerprint request shared by the host-harness test and the GPU probe tests,
with their reference (tests/fingerprint_ref.py) computed once.

Words: tracks of chroma rows sized to an exact cell count (0, 1, 2, 3, 4, 63, 64, 65, 66, 130, 300) for
a layout with Cs a multiple of khop and for the uneven 43 / 44 frames per cell, plus all-zero rows and
constant rows, which give zero words.
Match: made-up word arrays.  MATCH_CALLS maps a name to (words, [(O, min_overlap_words), ...]).
"""
import numpy as np

import fingerprint_ref as R

f32 = np.float32
SR = 44100
LAYOUTS = {"two_frames": (512, 1024), "uneven_43_44": (512, 22050)}  # name: (khop, Cs)
CELL_COUNTS = (0, 1, 2, 3, 4, 63, 64, 65, 66, 130, 300)
_CACHE = {}


def _frames(n, Cs, hop, extra=0):
    """The fewest frames every `hop` whose span gives n cells of Cs, plus `extra` that add no cell."""
    F = -(-(n * Cs) // hop)
    while extra and (F + extra) * hop >= (n + 1) * Cs:
        extra -= 1
    return F + extra


def word_tracks(layout):
    """[(rows, tag)] of the layout."""
    key = ("tracks", layout)
    if key in _CACHE:
        return _CACHE[key]
    khop, Cs = LAYOUTS[layout]
    rng = np.random.default_rng(8800 + sorted(LAYOUTS).index(layout))
    out = []

    def make(n, tag, j=0):
        F = _frames(n, Cs, khop, extra=j % 2)
        rows = (rng.random((F, 12), dtype=f32) ** 2).astype(f32)
        assert R.n_cells(F, khop, Cs) == n, (layout, n, F)
        return [rows, tag]

    for j, n in enumerate(CELL_COUNTS):
        out.append(make(n, "n%d" % n, j))
    z = make(20, "zero_rows")
    z[0][:] = 0.0
    out.append(z)
    # a held constant: sixteenths, whose sums over a cell and means are exact, so every cell mean is the
    # row itself whether the cell has 43 frames or 44
    z = make(20, "constant_rows")
    z[0][:] = (rng.integers(0, 16, 12) / 16.0).astype(f32)
    out.append(z)
    # ... and with arbitrary values, where cells of 43 and of 44 frames may round their means apart
    z = make(20, "constant_rows_inexact")
    z[0][:] = z[0][0]
    out.append(z)
    z = make(66, "zero_and_constant_inside")
    F = z[0].shape[0]
    z[0][F // 8:F // 4] = 0.0
    z[0][F // 2:3 * F // 4] = z[0][F // 2]
    out.append(z)
    _CACHE[key] = out
    return out


def word_reference(layout):
    """Per track of word_tracks(layout): (m, words)."""
    key = ("ref", layout)
    if key not in _CACHE:
        khop, Cs = LAYOUTS[layout]
        _CACHE[key] = []
        for rows, _ in word_tracks(layout):
            m = R.cell_rows(rows, khop, Cs)
            _CACHE[key].append((m, R.words_of(m)))
    return _CACHE[key]


def _rand_words(rng, W, zeros=0.1):
    w = rng.integers(0, 1 << 24, W, dtype=np.uint32)
    w[rng.random(W) < zeros] = 0
    return w


def _related(rng, base, shift, flips, W):
    """W words: base moved by `shift` words (word p of the result is base[p + shift]), random outside,
    with `flips` single bits flipped."""
    out = _rand_words(rng, W)
    for p in range(W):
        if 0 <= p + shift < base.size:
            out[p] = base[p + shift]
    for p in rng.choice(W, min(flips, W), replace=False):
        out[p] ^= np.uint32(1 << int(rng.integers(24)))
    return out


def _calls():
    rng = np.random.default_rng(99)
    calls = {}
    # W from {1, 2, 63, 64, 65, 130, 300} in one call, some tracks related, every O of the table
    base = _rand_words(rng, 300)
    mixed = [_rand_words(rng, 1), _rand_words(rng, 2), _related(rng, base, 40, 3, 63), _related(rng, base, 100, 0, 64),
             _rand_words(rng, 65), _related(rng, base, -7, 9, 130), base]
    calls["mixed7"] = (mixed, [(0, 1), (1, 0), (31, 2), (32, 8), (63, 1), (64, 32), (255, 1)])
    calls["one_track"] = ([_rand_words(rng, 5)], [(3, 1)])
    calls["two_tracks"] = ([_rand_words(rng, 40), _rand_words(rng, 33)], [(0, 1), (31, 4), (32, 4)])
    b5 = _rand_words(rng, 48)
    calls["five_tracks"] = ([b5, _related(rng, b5, 3, 2, 40), _rand_words(rng, 44), _related(rng, b5, -5, 0, 48),
                             _rand_words(rng, 2)], [(1, 1), (31, 8), (64, 8)])
    b17 = _rand_words(rng, 24)
    calls["seventeen_tracks"] = ([_related(rng, b17, int(rng.integers(-3, 4)), int(rng.integers(4)), int(rng.integers(1, 25)))
                                  if t % 3 else _rand_words(rng, int(rng.integers(1, 25))) for t in range(17)],
                                 [(1, 1), (31, 2)])
    # 9 tracks of 3 words: crosses the 4 x 4 tile's edge in both directions, O >= W
    calls["tile_edge"] = ([_rand_words(rng, 3, zeros=0.0) for _ in range(9)], [(0, 1), (1, 1), (255, 1), (2, 3), (2, 4)])
    return calls


def match_calls():
    if "calls" not in _CACHE:
        _CACHE["calls"] = _calls()
    return _CACHE["calls"]


def match_reference(name, O, min_overlap_words):
    key = ("rec", name, O, min_overlap_words)
    if key not in _CACHE:
        _CACHE[key] = R.pair_records(match_calls()[name][0], O, min_overlap_words)
    return _CACHE[key]
