"""The key timeline (include/stratum_hip.h, sdsp_key_timeline) written from the definition: the
chroma rows from the oracle's own stages, the segment plan in Python integers and numpy f32
scalars, each segment's key from the oracle's detect_key unit, the primary key and the changes in
plain Python.  Nothing here knows how the kernels split the work.

The rows are rebuilt by a chain of oracle units (trim bounds of analyze's trace, normalize, stft at
the key STFT's size and hop, key_stages, smooth_chroma).  For every track the chain's frame count
and its double-precision sums of the rows and of their squares, in frame-major order, must equal
the trace's own (n_key_frames, chroma_sum, chroma_sq) exactly: a configuration whose rows the chain
does not reproduce fails here, loudly, and not silently on the GPU.
"""
import numpy as np

import oracle
import units

f32 = np.float32
SEGMENT_FIELDS = ("start_frame", "timestamp", "key", "confidence", "clarity", "top_keys", "top_scores")
CHANGE_FIELDS = ("segment", "timestamp", "from_key", "to_key", "confidence")
SCALARS = ("n_segments", "n_changes", "n_frames", "first_sample", "segment_frames", "hop_frames", "frame_size",
           "hop_size", "primary_key", "primary_count", "status")


def key_stft(cfg):
    """(kfs, khop): the override's frame and hop, else frame_size and hop_size."""
    if cfg.enable_key_stft_override:
        return max(int(cfg.key_stft_frame_size), 256), max(int(cfg.key_stft_hop_size), 1)
    return int(cfg.frame_size), int(cfg.hop_size)


def _checksums(rows):
    cs = cq = 0.0
    for v in np.ascontiguousarray(rows, f32).ravel().tolist():  # f32 values as doubles, in order
        cs += v
        cq += v * v
    return cs, cq


def chroma_rows(x, sample_rate, cfg):
    """(status, first_sample, rows): the rows C of the definition for one track, (F, 12) float32, or
    None when the key path does not run (n < frame_size or n < kfs).  Asserts the trace's checksums."""
    x = np.ascontiguousarray(x, f32)
    st = oracle.analyze(x, sample_rate, cfg, trace=True) if x.size else (1, "Invalid input: Empty audio samples", None)
    if st[0] != 0:
        return st[0], 0, None
    tr = st[2]
    xn = x
    if cfg.enable_normalization:
        s, xn = oracle.normalize(x, int(cfg.normalization), sample_rate)
        assert s == 0, xn
    sig = xn[tr["trim_start"]:tr["trim_end"]]
    kfs, khop = key_stft(cfg)
    if sig.size < int(cfg.frame_size) or sig.size < kfs:
        assert tr["n_key_frames"] == 0, tr["n_key_frames"]
        return 0, int(tr["trim_start"]), None
    spec = oracle.stft(sig, kfs, khop)
    _, ch, _ = units.key_stages(spec, sample_rate, cfg)
    rows = units.smooth_chroma(ch, 5) if ch.shape[0] > 5 else np.ascontiguousarray(ch, f32)
    assert rows.shape[0] == tr["n_key_frames"], (rows.shape, tr["n_key_frames"])
    cs, cq = _checksums(rows)
    assert cs == tr["chroma_sum"] and cq == tr["chroma_sq"], (cs, tr["chroma_sum"], cq, tr["chroma_sq"])
    return 0, int(tr["trim_start"]), rows


def fps(sample_rate, khop):
    return f32(sample_rate) / f32(khop)


def plan(request, sample_rate, khop):
    """(L, H) of a request dict (segment_seconds, overlap_seconds | segment_frames, hop_frames), or
    the reason it is refused as a string."""
    ss, os_ = f32(request.get("segment_seconds", 0.0)), f32(request.get("overlap_seconds", 0.0))
    sf, hf = int(request.get("segment_frames", 0)), int(request.get("hop_frames", 0))
    mc = f32(request.get("min_change_confidence", -1.0))
    sec, frm = bool(ss != 0 or os_ != 0), bool(sf != 0 or hf != 0)
    if not sec and not frm:
        return "neither"
    if sec and frm:
        return "both"
    if sec and not (np.isfinite(ss) and np.isfinite(os_)):
        return "not finite"
    if sec and (ss < 0 or os_ < 0):
        return "negative"
    if np.isnan(mc):
        return "NaN"
    if sec:
        r = fps(sample_rate, khop)
        pl, po = float(f32(ss * r)), float(f32(os_ * r))  # f32 products, truncated
        L, O = (int(pl) if pl < 2.0 ** 32 else 2 ** 32), (int(po) if po < 2.0 ** 32 else 2 ** 32)
        if L == 0:
            return "L == 0"
        if O >= L:
            return "O >= L"
        H = L - O
    else:
        L, H = sf, hf
        if L == 0:
            return "L == 0"
        if H == 0:
            return "H == 0"
    if L >= 2 ** 31 or H >= 2 ** 31:
        return "2^31"
    return L, H


def n_segments(F, L, H):
    return 0 if F < L else (F - L) // H + 1


def primary(keys, confs):
    """(primary_key, primary_confidence f32, primary_count): most segments, ties to the key whose
    first segment is earliest; the f32 sum of its confidences in segment order over f32(count)."""
    if not keys:
        return -1, f32(0), 0
    count, first = {}, {}
    for s, k in enumerate(keys):
        count[k] = count.get(k, 0) + 1
        first.setdefault(k, s)
    best = min(count, key=lambda k: (-count[k], first[k]))
    tot = f32(0)
    for k, c in zip(keys, confs):
        if k == best:
            tot = f32(tot + f32(c))
    return best, f32(tot / f32(count[best])), count[best]


def changes(keys, confs, timestamps, min_change_confidence):
    out = []
    for i in range(1, len(keys)):
        if keys[i] == keys[i - 1]:
            continue
        c = f32(f32(f32(confs[i - 1]) + f32(confs[i])) / f32(2.0))
        if c > f32(min_change_confidence):
            out.append((i, f32(timestamps[i]), keys[i - 1], keys[i], c))
    return out


def segment_ref(rows):
    """detect_key and key clarity of one segment's rows: (key, confidence, clarity, top_keys, top_scores)."""
    key, conf, scores, _ = units.detect_key(np.ascontiguousarray(rows, f32))
    cl = oracle.key_clarity([s for _, s in scores])
    return key, f32(conf), f32(cl), [k for k, _ in scores[:3]], [f32(s) for _, s in scores[:3]]


def timeline(rows, L, H, sample_rate, khop, min_change_confidence=-1.0):
    """The segments, primary key and changes of one track's rows ((F, 12), or None / empty)."""
    F = 0 if rows is None else int(rows.shape[0])
    S = n_segments(F, L, H)
    r = fps(sample_rate, khop)
    seg = {k: [] for k in SEGMENT_FIELDS}
    for s in range(S):
        f0 = s * H
        assert 0 <= f0 and f0 + L <= F
        key, conf, cl, tk, ts = segment_ref(rows[f0:f0 + L])
        for k, v in zip(SEGMENT_FIELDS, (f0, f32(f32(f0) / r), key, conf, cl, tk, ts)):
            seg[k].append(v)
    pk, pc, pn = primary(seg["key"], seg["confidence"])
    ch = changes(seg["key"], seg["confidence"], seg["timestamp"], min_change_confidence)
    dts = dict(start_frame=np.uint64, timestamp=f32, key=np.int32, confidence=f32, clarity=f32, top_keys=np.int32,
               top_scores=f32, segment=np.uint64, from_key=np.int32, to_key=np.int32)
    out = {"n_segments": S, "n_changes": len(ch), "n_frames": F, "primary_key": pk, "primary_confidence": pc,
           "primary_count": pn}
    out["segments"] = {k: np.array(seg[k], dts[k]).reshape((S, 3) if k.startswith("top_") else (S,)) for k in SEGMENT_FIELDS}
    out["changes"] = {k: np.array([c[j] for c in ch], dts[k]) for j, k in enumerate(CHANGE_FIELDS)}
    return out


def timeline_ref(x, sample_rate, cfg, request, chain=None):
    """One track's timeline as sdsp.analyze_batch_device_requests returns it.  `chain` is a
    chroma_rows() result to share between requests."""
    status, first, rows = chain if chain is not None else chroma_rows(x, sample_rate, cfg)
    kfs, khop = key_stft(cfg)
    L, H = plan(request, sample_rate, khop)
    out = {"status": status, "segment_frames": L, "hop_frames": H, "frame_size": kfs, "hop_size": khop}
    if status != 0:
        t = timeline(None, L, H, sample_rate, khop)
        t.update(primary_key=0)  # a failed track's fields are all zero
        out.update(t, first_sample=0)
        return out
    out.update(timeline(rows, L, H, sample_rate, khop, request.get("min_change_confidence", -1.0)))
    out["first_sample"] = first if rows is not None else 0
    return out


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a, f32).view(np.uint32) if a.dtype.kind == "f" else a


def assert_equal(got, want, what=""):
    """Every scalar field equal, every array equal, floats on their uint32 view."""
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert _bits(f32(got["primary_confidence"])) == _bits(f32(want["primary_confidence"])), (what, "primary_confidence")
    for group, fields in (("segments", SEGMENT_FIELDS), ("changes", CHANGE_FIELDS)):
        for k in fields:
            g, w = np.asarray(got[group][k]), np.asarray(want[group][k])
            assert g.shape == w.shape, (what, group, k, g.shape, w.shape)
            bad = np.argwhere(_bits(g) != _bits(w))
            assert bad.size == 0, (what, group, k, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def cadence(tonic, seconds, sample_rate=44100, minor=False, chord_seconds=0.5, level=0.2):
    """I-IV-V-I cadences on pitch class `tonic` (0 = C): triads of four decaying harmonics per note
    around middle C, each chord with a short attack and an exponential decay."""
    n_chord = int(chord_seconds * sample_rate)
    t = np.arange(n_chord, dtype=np.float64) / sample_rate
    env = np.minimum(t / 0.01, 1.0) * np.exp(-3.0 * t)
    out = np.zeros(int(seconds * sample_rate), np.float64)
    for c in range(-(-out.size // n_chord)):
        root = tonic + (0, 5, 7, 0)[c % 4]
        third = 3 if minor and c % 4 != 2 else 4  # (a minor key's dominant stays major)
        x = np.zeros(n_chord)
        for semis in (0, third, 7):
            f0 = 261.6255653005986 * 2.0 ** (((root + semis) % 12 + (0 if (root + semis) % 12 < 6 else -12)) / 12.0)
            for h in range(1, 5):
                x += np.sin(2.0 * np.pi * f0 * h * t) / h
        seg = out[c * n_chord:(c + 1) * n_chord]
        seg += (x * env)[:seg.size]
    return (out * (level / 3.0)).astype(f32)


def modulating_track(seconds_each=16.0, sample_rate=44100, tonics=(0, 6)):
    """Cadences in C major, then in F sharp major (by default 16 s each)."""
    return np.concatenate([cadence(t, seconds_each, sample_rate) for t in tonics])
