"""The sections request (include/stratum_hip.h, sdsp_sections) written from the definition in numpy
f32: the cell plan in Python integers, every ordered sum as an np.cumsum over f32 (sequential, from
0, ascending) or an explicit loop, never np.sum.  Nothing here knows how the kernels split the work.

The inputs of a track come from the oracle: the smoothed chroma rows of key_timeline_ref.chroma_rows
and the frame energies E[f] = the f32 sum over bins ascending of mag * mag over the spectrogram of
overview_ref.signal_and_mags.
"""
import numpy as np

import key_timeline_ref as K
import overview_ref

f32 = np.float32
LIST, CURVE = 1, 2
SECTION_FIELDS = ("start_cell", "end_cell", "start_time", "end_time", "strength", "mean_energy", "relative_energy",
                  "snapped_time", "downbeat")
DEFAULTS = dict(cell_seconds=0.0, cell_samples=0, kernel_cells=16, min_gap_cells=8, energy_weight=1.0, min_strength=0.5,
                snap_seconds=0.0, what=LIST | CURVE)


def seq_sum(v):
    """v[0] + v[1] + ... in f32, from 0, in order."""
    v = np.ascontiguousarray(v, f32).ravel()
    return f32(np.cumsum(v, dtype=f32)[-1]) if v.size else f32(0)


def frame_energies(mags):
    """E[f]: the f32 sum over bins ascending of mag * mag."""
    m = np.ascontiguousarray(mags, f32)
    if m.shape[0] == 0:
        return np.zeros(0, f32)
    return np.ascontiguousarray(np.cumsum((m * m).astype(f32), axis=1, dtype=f32)[:, -1])


def plan(request, sample_rate, khop, hop, stages_full=True, legacy=False, beat_rows=False):
    """Cs of a request dict, or the reason it is refused as (status, reason)."""
    r = dict(DEFAULTS, **request)
    floats = [f32(r[k]) for k in ("cell_seconds", "energy_weight", "min_strength", "snap_seconds")]
    if r["what"] == 0:
        return 1, "what == 0"
    if r["what"] & ~(LIST | CURVE):
        return 1, "unknown bits"
    if any(not np.isfinite(v) or v < 0 for v in floats):
        return 1, "float"
    sec, smp = bool(floats[0] != 0), int(r["cell_samples"]) != 0
    if sec == smp:
        return 1, "both" if sec else "neither"
    if not 1 <= int(r["kernel_cells"]) <= 64:
        return 1, "K"
    if int(r["min_gap_cells"]) >= 2 ** 31:
        return 1, "G"
    if sec:
        p = float(f32(floats[0] * f32(sample_rate)))
        Cs = int(p) if p < 2.0 ** 32 else 2 ** 32
    else:
        Cs = int(r["cell_samples"])
    if Cs >= 2 ** 31:
        return 1, "Cs >= 2^31"
    if Cs < max(khop, hop) or Cs == 0:
        return 1, "Cs too small"
    if not stages_full:
        return 1, "BPM only"
    if legacy:
        return 4, "legacy"
    if beat_rows:
        return 4, "beat rows"
    return Cs


def n_cells(F, khop, Fb, hop, Cs):
    return min(F * khop, Fb * hop) // Cs


def first_frame(c, Cs, hop):
    """The first frame whose start f * hop is >= c * Cs."""
    return -(-(c * Cs) // hop)


def cell_means(x, n, Cs, hop):
    """Per cell the f32 mean of x's frames (rows of a 2-D x alike) whose start lies in the cell."""
    x = np.ascontiguousarray(x, f32)
    out = np.zeros((n,) + x.shape[1:], f32)
    for c in range(n):
        f0, f1 = first_frame(c, Cs, hop), first_frame(c + 1, Cs, hop)
        assert f0 < f1 <= x.shape[0], (c, f0, f1, x.shape)
        out[c] = np.cumsum(x[f0:f1], axis=0, dtype=f32)[-1] / f32(f1 - f0)
    return out


def distances(m, e, w):
    """D(a, b) for every pair, each the sequential fold of the definition."""
    n = m.shape[0]
    D = np.zeros((n, n), f32)
    for i in range(12):
        d = (m[:, None, i] - m[None, :, i]).astype(f32)
        D = (D + (d * d).astype(f32)).astype(f32)
    de = (e[:, None] - e[None, :]).astype(f32)
    return (D + (f32(w) * (de * de).astype(f32)).astype(f32)).astype(f32)


def novelty(m, g, K, w):
    """(N, e, gmax) over the cell features m (n, 12) and g (n,)."""
    n = g.size
    N = np.zeros(n, f32)
    gmax = f32(g.max()) if n else f32(0)
    e = (g / gmax).astype(f32) if gmax > 0 else np.zeros(n, f32)
    if n < 2 * K:
        return N, e, gmax
    iu = np.triu_indices(K, 1)  # row-major: a ascending, b ascending within a
    # only the band |a - b| < 2 K is ever read: build D over windows to keep large tracks cheap
    for c in range(K, n - K + 1):
        lo = c - K
        D = distances(m[lo:c + K], e[lo:c + K], w)
        cross = seq_sum(D[:K, K:])
        x = f32(cross / f32(K * K))
        if K > 1:
            wp, wf = seq_sum(D[:K, :K][iu]), seq_sum(D[K:, K:][iu])
            x = f32(x - f32(f32(wp + wf) / f32(K * (K - 1))))
        N[c] = x
    return N, e, gmax


def boundaries(N, G, min_strength):
    """The boundary flag of every cell (uint8)."""
    n = N.size
    b = np.zeros(n, np.uint8)
    if n == 0:
        return b
    nmax = f32(N.max())
    thr = f32(f32(min_strength) * nmax)
    for c in range(n):
        v = N[c]
        if not (v > 0 and v >= thr):
            continue
        before, after = N[max(c - G, 0):c], N[c + 1:min(c + G, n - 1) + 1]
        if np.all(v > before) and np.all(v >= after):
            b[c] = 1
    return b


def snap(downs, t, snap_seconds):
    """(downbeat index or -1, snapped time)."""
    downs = np.ascontiguousarray(downs, f32)
    if downs.size == 0:
        return -1, f32(t)
    d = np.abs((downs - f32(t)).astype(f32))
    j = int(np.argmin(d))  # the first minimum
    return (j, downs[j]) if d[j] <= f32(snap_seconds) else (-1, f32(t))


def assemble(g, N, b, Cs, sample_rate, downs, snap_seconds):
    n = g.size
    starts = [0] + [int(c) for c in np.flatnonzero(b)] if n else []
    sec = {k: [] for k in SECTION_FIELDS}
    for s0, s1 in zip(starts, starts[1:] + [n]):
        t0 = f32(f32(s0 * Cs) / f32(sample_rate))
        j, st = snap(downs, t0, snap_seconds)
        row = (s0, s1, t0, f32(f32(s1 * Cs) / f32(sample_rate)), N[s0] if s0 else f32(0),
               f32(seq_sum(g[s0:s1]) / f32(s1 - s0)), f32(0), st, j)
        for k, v in zip(SECTION_FIELDS, row):
            sec[k].append(v)
    top = max(sec["mean_energy"]) if sec["mean_energy"] else f32(0)
    sec["relative_energy"] = [f32(v / top) if top > 0 else f32(0) for v in sec["mean_energy"]]
    dts = dict(start_cell=np.uint64, end_cell=np.uint64, downbeat=np.int32)
    return {k: np.array(sec[k], dts.get(k, f32)) for k in SECTION_FIELDS}


def cells_ref(rows, E, request, sample_rate, khop, hop):
    """m, g, N, boundary flags and n_cells of one track's rows (F, 12) and energies (Fb,)."""
    r = dict(DEFAULTS, **request)
    Cs = plan(r, sample_rate, khop, hop)
    F, Fb = (0 if rows is None else int(rows.shape[0])), (0 if E is None else int(E.size))
    n = n_cells(F, khop, Fb, hop, Cs)
    m = cell_means(rows, n, Cs, khop) if n else np.zeros((0, 12), f32)
    g = cell_means(E, n, Cs, hop) if n else np.zeros(0, f32)
    N, e, gmax = novelty(m, g, int(r["kernel_cells"]), r["energy_weight"])
    b = boundaries(N, int(r["min_gap_cells"]), r["min_strength"])
    return dict(n_cells=n, cell_samples=Cs, m=m, g=g, e=e, gmax=gmax, novelty=N, nmax=f32(N.max()) if n else f32(0),
                boundary=b)


def sections(rows, E, request, sample_rate, khop, hop, downs=()):
    """One track's sections as sdsp_sections carries them, from its rows and energies."""
    r = dict(DEFAULTS, **request)
    c = cells_ref(rows, E, r, sample_rate, khop, hop)
    out = dict(n_cells=c["n_cells"], cell_samples=c["cell_samples"], gmax=c["gmax"], nmax=c["nmax"])
    sec = assemble(c["g"], c["novelty"], c["boundary"], c["cell_samples"], sample_rate, downs, r["snap_seconds"])
    if not r["what"] & LIST:
        sec = {k: v[:0] for k, v in sec.items()}
    out["sections"] = sec
    out["n_sections"] = int(sec["start_cell"].size)
    curve = bool(r["what"] & CURVE)
    out["novelty"] = c["novelty"] if curve else np.zeros(0, f32)
    out["energy"] = c["g"] if curve else np.zeros(0, f32)
    out["n_curve"] = c["n_cells"] if curve else 0
    return out


def track_inputs(x, sample_rate, cfg):
    """(status, first_sample, rows, E) of one track from the oracle's chains; rows and E are None
    when the key path does not run."""
    status, first, rows = K.chroma_rows(x, sample_rate, cfg)
    if status != 0 or rows is None:
        return status, first if status == 0 else 0, None, None
    s2, first2, _, mags = overview_ref.signal_and_mags(x, sample_rate, cfg)
    assert s2 == 0 and first2 == first
    return 0, first, rows, frame_energies(mags)


def sections_ref(x, sample_rate, cfg, request, downs=(), chain=None):
    """One track's sections as sdsp.analyze_batch_device_with returns them.  `chain` is a
    track_inputs() result to share between requests; downs the result's downbeats."""
    status, first, rows, E = chain if chain is not None else track_inputs(x, sample_rate, cfg)
    kfs, khop = K.key_stft(cfg)
    Cs = plan(request, sample_rate, khop, int(cfg.hop_size))
    if status != 0:
        out = sections(None, None, request, sample_rate, khop, int(cfg.hop_size))
        out.update(status=status, first_sample=0, n_sections=0, sections={k: v[:0] for k, v in out["sections"].items()})
        return out
    out = sections(rows, E, request, sample_rate, khop, int(cfg.hop_size), downs)
    out.update(status=0, first_sample=first if rows is not None else 0, cell_samples=Cs)
    return out


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a, f32).view(np.uint32) if a.dtype.kind == "f" else a


def assert_arrays_equal(g, w, what=""):
    g, w = np.asarray(g), np.asarray(w)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(_bits(g) != _bits(w))
    assert bad.size == 0, (what, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def assert_equal(got, want, what=""):
    """Every scalar equal, every array equal, floats on their uint32 view."""
    for k in ("status", "n_cells", "cell_samples", "first_sample", "n_sections", "n_curve"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("gmax", "nmax"):
        assert _bits(f32(got[k])) == _bits(f32(want[k])), (what, k, got[k], want[k])
    for k in SECTION_FIELDS:
        assert_arrays_equal(got["sections"][k], want["sections"][k], (what, k))
    for k in ("novelty", "energy"):
        assert_arrays_equal(got[k], want[k], (what, k))
