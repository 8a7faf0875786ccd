"""The programme loudness request (include/stratum_hip.h, sdsp_r128) restated in numpy, as its header
comment defines it: the coefficients in double rounded to f32, the K-weighting recurrence restarted
one step before every step (vectorised over all (track, step) pairs of a call), the f32 block folds,
both gates with their ordered means, the order statistics of the loudness range, the maxima and the
peaks.  Every sum is a sequential f32 fold, every log10 the oracle's libm.

unbroken() is the other yardstick: the same coefficient formulas in double, one f64 filter over the
whole track, f64 blocks and gates (tests/test_r128_ref.py bounds the contract's distance from it)."""
import math

import numpy as np

import oracle

f32 = np.float32
NEG_INF = f32(-np.inf)
LOUDNESS, TRUE_PEAK, CURVES = 1, 2, 4
FLOATS = ("integrated_lufs", "range_lu", "range_low_lufs", "range_high_lufs", "max_momentary_lufs",
          "max_short_term_lufs", "sample_peak", "true_peak", "sample_peak_db", "true_peak_dbtp")
INTS = ("status", "has_integrated", "has_range", "n_samples", "step_samples", "n_steps", "n_momentary", "n_short_term",
        "n_gated_momentary", "n_gated_short_term")


def _log10(v):
    return f32(oracle.libm("log10", [f32(v)])[0])


def lufs(e):
    return f32(f32(-0.691) + f32(f32(10.0) * _log10(e)))


def db(v):
    return f32(f32(20.0) * _log10(v))


def gate_abs():
    return f32(oracle.libm("pow", [10.0], [f32(f32(-70.0) + f32(0.691)) / f32(10.0)])[0])


def coeffs64(sr):
    """(shelf, highpass) as b0 b1 b2 a1 a2 in double."""
    K = math.tan(math.pi * 1681.974450955533 / sr)
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    Q = 0.7071752369554196
    a0 = 1.0 + K / Q + K * K
    shelf = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    K = math.tan(math.pi * 38.13547087602444 / sr)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    hp = (1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    return shelf, hp


def coeffs(sr):
    shelf, hp = coeffs64(sr)
    return np.array(shelf, f32), np.array(hp, f32)


def taps():
    """h[p - 1][k], p = 1..3: the three interpolating phases of the 4x windowed sinc."""
    h = np.zeros((3, 12), f32)
    for p in (1, 2, 3):
        for k in range(12):
            t = (k - 5) - p / 4.0
            h[p - 1, k] = f32(math.sin(math.pi * t) / (math.pi * t) * (0.5 + 0.5 * math.cos(math.pi * t / 6.0)))
    return h


def _biquad(c, s, x1, x2):
    o = c[0] * s + x1
    return o, (c[1] * s + x2) - c[3] * o, c[2] * s - c[4] * o


def step_energies(tracks, sr):
    """z of every track: column (t, j) of one matrix holds samples [(j - 1) * step, (j + 1) * step) of
    track t (zeros in front of step 0, which leave the zero state as it is)."""
    step = sr // 10
    shelf, hp = coeffs(sr)
    Js = [len(x) // step for x in tracks]
    S = sum(Js)
    X = np.zeros((2 * step, S), f32)
    at = 0
    for x, J in zip(tracks, Js):
        x = np.asarray(x, f32)
        for j in range(J):
            a = max(j - 1, 0) * step
            seg = x[a:(j + 1) * step]
            X[2 * step - seg.size:, at + j] = seg
        at += J
    z = np.zeros(S, f32)
    a1 = np.zeros(S, f32)
    a2, b1, b2 = a1.copy(), a1.copy(), a1.copy()
    for k in range(2 * step):
        o, a1, a2 = _biquad(shelf, X[k], a1, a2)
        o, b1, b2 = _biquad(hp, o, b1, b2)
        if k >= step:
            z = z + o * o
    out, at = [], 0
    for J in Js:
        out.append(z[at:at + J].copy())
        at += J
    return out


def blocks(z, length, step):
    """The block means of `length` steps: the ascending f32 sum over the divisor."""
    n = max(len(z) - (length - 1), 0)
    acc = np.zeros(n, f32)
    for k in range(length):
        acc = acc + z[k:k + n]
    return acc / f32(length * step)


def _seq_mean(e):
    return f32(np.cumsum(e, dtype=f32)[-1] / f32(e.size))


def peaks(x, true_peak=True):
    x = np.asarray(x, f32)
    sp = f32(np.max(np.abs(x))) if x.size else f32(0.0)
    if not true_peak:
        return sp, f32(0.0)
    xp = np.concatenate([np.zeros(5, f32), x, np.zeros(6, f32)])
    tp = sp
    for h in taps():
        acc = np.zeros(x.size, f32)
        for k in range(12):
            acc = acc + h[k] * xp[k:k + x.size]
        if x.size:
            tp = max(tp, f32(np.max(np.abs(acc))))
    return sp, f32(tp)


def measure(tracks, sr, what=LOUDNESS | TRUE_PEAK | CURVES):
    """One dict per track with every field of sdsp_r128 (the curves as float32 arrays, empty without
    CURVES), plus `gates`: the blocks each gate dropped and kept (for the tests' own checks)."""
    step = sr // 10
    shelf, hp = coeffs(sr)
    ga = gate_abs()
    zs = step_energies(tracks, sr) if what & LOUDNESS else [np.zeros(0, f32) for _ in tracks]
    out = []
    for x, z in zip(tracks, zs):
        sp, tp = peaks(x, bool(what & TRUE_PEAK))
        r = dict(status=0, has_integrated=0, has_range=0, integrated_lufs=NEG_INF, range_lu=f32(0), range_low_lufs=f32(0),
                 range_high_lufs=f32(0), max_momentary_lufs=NEG_INF, max_short_term_lufs=NEG_INF, sample_peak=sp,
                 true_peak=tp, sample_peak_db=db(sp), true_peak_dbtp=db(tp), n_samples=len(x), step_samples=step,
                 n_steps=0, n_momentary=0, n_short_term=0, n_gated_momentary=0, n_gated_short_term=0, shelf=shelf,
                 highpass=hp, momentary=np.zeros(0, f32), short_term=np.zeros(0, f32), gates={})
        out.append(r)
        if not what & LOUDNESS:
            continue
        m, s = blocks(z, 4, step), blocks(z, 30, step)
        r.update(n_steps=len(z), n_momentary=m.size, n_short_term=s.size)
        if what & CURVES:
            r.update(momentary=m, short_term=s)
        a = m[m > ga]
        if a.size:
            gr = f32(_seq_mean(a) * f32(0.1))
            g = m[(m > ga) & (m > gr)]
            r["gates"]["momentary"] = (m.size - a.size, a.size - g.size, g.size)
            r["n_gated_momentary"] = g.size
            if g.size:
                r.update(has_integrated=1, integrated_lufs=lufs(_seq_mean(g)))
        b = s[s > ga]
        if b.size:
            gr = f32(_seq_mean(b) * f32(0.01))
            e = np.sort(s[(s > ga) & (s > gr)])
            r["gates"]["short_term"] = (s.size - b.size, b.size - e.size, e.size)
            r["n_gated_short_term"] = M = e.size
            if M:
                lo, hi = lufs(e[((M - 1) * 10 + 50) // 100]), lufs(e[((M - 1) * 95 + 50) // 100])
                r.update(has_range=1, range_low_lufs=lo, range_high_lufs=hi, range_lu=f32(hi - lo))
        if m.size:
            r["max_momentary_lufs"] = lufs(np.max(m))
        if s.size:
            r["max_short_term_lufs"] = lufs(np.max(s))
    return out


def unbroken(x, sr):
    """BS.1770 with one f64 filter over the whole track: (integrated LUFS, momentary LUFS per block,
    short-term LUFS per block), blocks on the same 100-ms grid."""
    step = sr // 10
    shelf, hp = coeffs64(sr)
    y = np.asarray(x, np.float64)
    for c in (shelf, hp):
        o = np.empty_like(y)
        x1 = x2 = 0.0
        b0, b1, b2, a1, a2 = c
        for i, s in enumerate(y.tolist()):
            v = b0 * s + x1
            x1 = b1 * s + x2 - a1 * v
            x2 = b2 * s - a2 * v
            o[i] = v
        y = o
    J = len(y) // step
    z = (y[:J * step].reshape(J, step) ** 2).sum(axis=1)
    m = np.array([z[j:j + 4].sum() / (4 * step) for j in range(max(J - 3, 0))])
    s = np.array([z[j:j + 30].sum() / (30 * step) for j in range(max(J - 29, 0))])
    L = lambda e: -0.691 + 10.0 * np.log10(e)
    ga = 10.0 ** ((-70.0 + 0.691) / 10.0)
    a = m[m > ga]
    integ = -np.inf
    if a.size:
        g = a[a > a.mean() * 0.1]
        integ = L(g.mean()) if g.size else -np.inf
    with np.errstate(divide="ignore"):
        return integ, L(m), L(s)
