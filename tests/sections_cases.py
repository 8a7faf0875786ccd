"""Small shapes of the sections request shared by the host-harness test and the GPU probe test:
tracks of chroma rows and frame energies sized to an exact cell count, for every frames-per-cell
layout and kernel size of the test table, with their reference (tests/sections_ref.py) computed once.

Cell counts: 0, 1, 2K-1, 2K, 2K+1 (the first scored cell), 63, 64, 65, 130, 300 (tile seams and the
halo).  Layouts: 1 and 2 frames per cell, the uneven 43 / 44 (Cs = 22,050 at hop 512), and a key hop
of 256 against a base hop of 512.  Beside the random tracks: zero rows inside a track, an all-zero
energy array (gmax = 0), all-zero rows, and zero rows over alternating energies, whose novelty at
K = 1 is a plateau of equal values.
"""
import numpy as np

import sections_ref as S

f32 = np.float32
SR = 44100
LAYOUTS = {  # name: (khop, hop, Cs)
    "one_frame": (512, 512, 512),
    "two_frames": (512, 512, 1024),
    "uneven_43_44": (512, 512, 22050),
    "khop256_hop512": (256, 512, 1024),
}
KS = (1, 2, 16, 64)
GS = (0, 1, 8)
WEIGHT, MIN_STRENGTH = 0.75, 0.3
_CACHE = {}


def cell_counts(K):
    return sorted({0, 1, 2 * K - 1, 2 * K, 2 * K + 1, 63, 64, 65, 130, 300})


def _frames(n, Cs, hop, extra=0):
    """The fewest frames every `hop` whose span gives n cells of Cs, plus `extra` that add no cell."""
    F = -(-(n * Cs) // hop)
    while extra and (F + extra) * hop >= (n + 1) * Cs:
        extra -= 1
    return F + extra


def tracks(layout, K):
    """[(rows, energies, tag)] of the layout at kernel size K."""
    key = ("tracks", layout, K)
    if key in _CACHE:
        return _CACHE[key]
    khop, hop, Cs = LAYOUTS[layout]
    rng = np.random.default_rng(7700 + 13 * K + sorted(LAYOUTS).index(layout))
    out = []

    def make(n, tag, j=0):
        F, Fb = _frames(n, Cs, khop, extra=3 * (j % 2)), _frames(n, Cs, hop, extra=j % 3)
        rows = (rng.random((F, 12), dtype=f32) ** 2).astype(f32)
        E = (rng.random(Fb, dtype=f32) * f32(40.0)).astype(f32)
        # parts with their own chroma and level, so that the novelty has peaks to pick
        for p in range(0, F, max(F // 5, 1)):
            rows[p:p + max(F // 5, 1)] += (rng.random(12, dtype=f32) * f32(0.8)).astype(f32)
        for p in range(0, Fb, max(Fb // 4, 1)):
            E[p:p + max(Fb // 4, 1)] *= f32(rng.random() * 3.0 + 0.1)
        assert S.n_cells(F, khop, Fb, hop, Cs) == n, (layout, n, F, Fb)
        return [rows, E, tag]

    for j, n in enumerate(cell_counts(K)):
        out.append(make(n, "n%d" % n, j))
    z = make(65, "zero_rows_inside")
    z[0][z[0].shape[0] // 3:z[0].shape[0] // 2] = 0.0
    out.append(z)
    z = make(65, "zero_energy")
    z[1][:] = 0.0
    out.append(z)
    z = make(130, "zero_rows")
    z[0][:] = 0.0
    out.append(z)
    z = make(40, "plateau")
    z[0][:] = 0.0
    z[1] = (np.arange(z[1].size) * hop // Cs % 2).astype(f32)  # every frame of a cell alike: g = 0, 1, 0, 1, ...
    out.append(z)
    _CACHE[key] = out
    return out


def request(layout, K, G, **more):
    return dict(dict(cell_samples=LAYOUTS[layout][2], kernel_cells=K, min_gap_cells=G, energy_weight=WEIGHT,
                     min_strength=MIN_STRENGTH), **more)


def reference(layout, K):
    """Per track of tracks(layout, K) the cells_ref at G = 0 (m, g, N do not depend on G)."""
    key = ("ref", layout, K)
    if key not in _CACHE:
        khop, hop, _ = LAYOUTS[layout]
        _CACHE[key] = [S.cells_ref(r, e, request(layout, K, 0), SR, khop, hop) for r, e, _ in tracks(layout, K)]
    return _CACHE[key]


def boundaries(layout, K, G):
    key = ("bnd", layout, K, G)
    if key not in _CACHE:
        _CACHE[key] = [S.boundaries(c["novelty"], G, MIN_STRENGTH) for c in reference(layout, K)]
    return _CACHE[key]
