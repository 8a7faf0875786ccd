"""The levels request (include/stratum_hip.h, sdsp_levels) restated in numpy: normalize()'s
LoudnessMetadata for each method (normalization.rs:262-547) and detect_and_trim's silence map
(silence.rs:102-279).  Every sum is the sequential f32 fold (np.cumsum(..., dtype=float32)[-1]),
every log10 / pow the oracle's libm; the K-weighting recurrence runs over the sample index on all
tracks of a call at once.  tests/test_levels_ref.py pins it to the oracle: raw * gain equals
oracle.normalize bit for bit, the map equals oracle.units.detect_and_trim's."""
import math

import numpy as np

import oracle

f32 = np.float32
EPS = f32(1e-10)
NEG_INF = f32(-np.inf)
PEAK, RMS, LOUDNESS = 0, 1, 2


def _pow10(e):
    return f32(oracle.libm("pow", [10.0], [f32(e)])[0])


def _log10(v):
    return f32(oracle.libm("log10", [f32(v)])[0])


def _db(v):
    return f32(f32(20.0) * _log10(v))


def params(sr):
    """normalize()'s constants for {-14 LUFS, 1 dB} at `sr`, as pipeline_params' loudness_params."""
    headroom, tl = f32(1.0), f32(-14.0)
    fsr = f32(sr)
    w0 = f32(f32(f32(2.0) * f32(3.14159274)) * f32(1681.9745)) / fsr
    cw, sw = f32(math.cos(float(w0))), f32(math.sin(float(w0)))
    alpha = f32(f32(sw / f32(2.0)) * np.sqrt(f32(1.0) / f32(0.707)))
    b0 = f32(f32(f32(1.0) + cw) / f32(2.0))
    b1 = f32(-f32(f32(1.0) + cw))
    a0 = f32(f32(1.0) + alpha)
    a1 = f32(f32(-2.0) * cw)
    a2 = f32(f32(1.0) - alpha)
    return {
        "target_peak": _pow10(f32(f32(0.0) - headroom) / f32(20.0)),
        "target_rms": _pow10(f32(f32(tl + f32(3.0)) - headroom) / f32(20.0)),
        "target_lufs": tl,
        "gate": _pow10(f32(f32(-70.0) + f32(0.691)) / f32(10.0)),
        "block": int(f32(fsr * f32(400.0)) / f32(1000.0)),
        "coef": tuple(f32(c / a0) for c in (b0, b1, b0, a1, a2)),
    }


def sumsq(x, g=None):
    """The sequential f32 fold of (x * g)^2 from 0 (x^2 without g)."""
    y = np.asarray(x, f32)
    if g is not None:
        y = y * f32(g)
    return f32(np.cumsum(y * y, dtype=f32)[-1]) if y.size else f32(0.0)


def peak(x):
    return f32(np.max(np.abs(np.asarray(x, f32)))) if len(x) else f32(0.0)


def kweighted(tracks, coef):
    """KWeightingFilter::process over every track (Direct Form II transposed), all tracks at once."""
    b0, b1, b2, a1, a2 = coef
    T, N = len(tracks), max((len(t) for t in tracks), default=0)
    X = np.zeros((N, T), f32)
    for t, x in enumerate(tracks):
        X[:len(x), t] = x
    Y = np.empty((N, T), f32)
    x1, x2 = np.zeros(T, f32), np.zeros(T, f32)
    for i in range(N):
        s = X[i]
        o = b0 * s + x1
        x1 = b1 * s + x2 - a1 * o
        x2 = b2 * s - a2 * o
        Y[i] = o
    return [np.ascontiguousarray(Y[:len(x), t]) for t, x in enumerate(tracks)]


def gated(y, P):
    """(gated sum, gated blocks) of one K-weighted track: calculate_lufs :209-239."""
    bs, gsum, gn = P["block"], f32(0.0), 0
    for s in range(0, len(y), bs):
        blk = y[s:s + bs]
        ms = f32(sumsq(blk) / f32(len(blk)))
        if ms > P["gate"]:
            gsum = f32(gsum + ms)
            gn += 1
    return gsum, gn


def _quiet():
    return {"status": 0, "measured": 1, "has_lufs": 0, "measured_lufs": NEG_INF, "peak_db": NEG_INF,
            "rms_db": NEG_INF, "gain_db": f32(0.0), "gain": f32(1.0)}


def _rms_db(ss, n):
    rms = np.sqrt(f32(ss / f32(n)))
    return _db(rms) if rms > EPS else NEG_INF


def peak_gain(pk, P):
    return f32(min(f32(P["target_peak"] / pk), f32(f32(1.0) / pk))) if pk > EPS else f32(1.0)


def normalize_peak(x, P):
    m, pk = _quiet(), peak(x)
    if pk <= EPS:
        return m
    m["peak_db"] = _db(pk)
    m["gain_db"] = _db(f32(P["target_peak"] / pk))
    m["gain"] = peak_gain(pk, P)
    m["rms_db"] = _rms_db(sumsq(x, m["gain"]), len(x))
    return m


def normalize_rms(x, P):
    m = _quiet()
    rms = np.sqrt(f32(sumsq(x) / f32(len(x))))
    if rms <= EPS:
        return m
    pk = peak(x)
    m["rms_db"], m["peak_db"] = _db(rms), _db(pk)
    g = f32(P["target_rms"] / rms)
    if f32(pk * g) > f32(1.0):
        g = f32(f32(1.0) / pk)
    m["gain"], m["gain_db"] = g, _db(g)
    return m


def normalize_loudness(x, y, P):
    """y: the K-weighted track (kweighted)."""
    gsum, gn = gated(y, P)
    if gn == 0:
        return normalize_peak(x, P)
    m, pk = _quiet(), peak(x)
    lufs = f32(f32(-0.691) + f32(f32(10.0) * _log10(f32(gsum / f32(gn)))))
    m["has_lufs"], m["measured_lufs"] = 1, lufs
    m["gain_db"] = f32(P["target_lufs"] - lufs)
    g = _pow10(f32(m["gain_db"] / f32(20.0)))
    m["peak_db"] = _db(pk)
    if f32(pk * g) > P["target_peak"]:
        g = f32(P["target_peak"] / pk)
        m["gain_db"] = _db(g)
    m["gain"] = g
    m["rms_db"] = _rms_db(sumsq(x, g), len(x))
    return m


def unmeasured():
    return {"status": 0, "measured": 0, "has_lufs": 0, "measured_lufs": f32(0.0), "peak_db": f32(0.0),
            "rms_db": f32(0.0), "gain_db": f32(0.0), "gain": f32(0.0)}


def loudness(tracks, sr, methods=(PEAK, RMS, LOUDNESS)):
    """Per track, {method: LoudnessMetadata dict} for the methods asked for (unmeasured() for the
    others), as sdsp_levels.method reports them."""
    P = params(sr)
    tracks = [np.asarray(t, f32) for t in tracks]
    ys = kweighted(tracks, P["coef"]) if LOUDNESS in methods else [None] * len(tracks)
    out = []
    for x, y in zip(tracks, ys):
        out.append({
            PEAK: normalize_peak(x, P) if PEAK in methods else unmeasured(),
            RMS: normalize_rms(x, P) if RMS in methods else unmeasured(),
            LOUDNESS: normalize_loudness(x, y, P) if LOUDNESS in methods else unmeasured(),
        })
    return out


def frame_rms(x, frame_size):
    """detect_and_trim's frame RMS: frames of frame_size every frame_size / 2 (one for a short track)."""
    x = np.asarray(x, f32)
    hop, n = frame_size // 2, len(x)
    nf = (n - frame_size) // hop + 1 if n >= frame_size else 1
    out = np.empty(nf, f32)
    for i in range(nf):
        fr = x[i * hop:min(i * hop + frame_size, n)]
        out[i] = np.sqrt(f32(sumsq(fr) / f32(len(fr)))) if len(fr) else f32(0.0)
    return out


def min_frames(sr, frame_size):
    hop = frame_size // 2
    return -(-int(f32(f32(500.0) / f32(1000.0)) * f32(sr)) // hop)


def silence_map(x, sr, frame_size=2048, threshold_db=-40.0):
    """detect_and_trim on x: (regions [(start, end)], trim_start, trim_end), silence.rs:171-256."""
    n, hop = len(x), frame_size // 2
    silent = frame_rms(x, frame_size) <= _pow10(f32(threshold_db) / f32(20.0))
    nf, mf = len(silent), min_frames(sr, frame_size)
    regions, start = [], None
    for f in range(nf):
        if silent[f] and start is None:
            start = f
        elif not silent[f] and start is not None:
            if f - start >= mf or start == 0:
                regions.append((start * hop, f * hop))
            start = None
    if start is not None and (nf - start >= mf or start == 0):
        regions.append((start * hop, n))
    ts = regions[0][1] if regions and regions[0][0] == 0 else 0
    te = regions[-1][0] if regions and regions[-1][1] == n else n
    ts = min(ts, te)
    te = max(te, ts)
    if not (ts < te <= n):
        ts = te = 0
    return regions, ts, te


def region_seconds(region, sr):
    return f32(f32(region[1] - region[0]) / f32(sr))
