"""The reference of the tempo map request (include/stratum_hip.h, sdsp_tempo_map), field by field.

Composed only from the oracle's units: oracle.hmm_track, units.detect_tempo_variations,
units.BayesianBeatTracker and units.detect_time_signature, in the order of generate_beat_grid
(beat_tracking/mod.rs:140-219): the whole-track HMM, the segments, per variable segment a tracker
update and a re-track, a stable sort.  units.BayesianBeatTracker rebuilds its state on every call, so
a new one is built from the carried tempo for each variable segment; that is exact, because an
update reads only the current tempo.  The oracle hands out the time signature's (beats per bar,
confidence) but not its three scores: signature_scores restates them (time_signature.rs:161-199) in
sequential f32, and tests/test_tempo_map_ref.py pins it to the oracle's pair by the last-maximum rule.
"""
import numpy as np

import oracle
import units

f32 = np.float32
EPS = f32(1e-10)
SEGMENT_FIELDS = ("start_time", "end_time", "bpm", "confidence", "is_variable", "updated", "n_onsets", "updated_bpm",
                  "updated_confidence", "n_beats")
_SEG_DTYPES = (f32, f32, f32, f32, np.uint8, np.uint8, np.uint32, f32, f32, np.uint32)
SCALARS = ("has_grid", "has_variation", "refined", "time_signature_scored", "hmm_beats", "beats_per_bar", "n_segments")
FLOATS = ("nominal_bpm", "nominal_confidence", "time_signature_confidence")


def _fold(a):
    """The sequential f32 sum from 0 (np.cumsum does not re-associate)."""
    a = np.asarray(a, f32)
    return f32(np.cumsum(a, dtype=f32)[-1]) if a.size else f32(0)


def positive_intervals(beats):
    d = np.diff(np.asarray(beats, f32))
    return d[d > 0]


def signature_scores(beats):
    """None where detect_time_signature scores nothing (fewer than 8 beats, no positive interval),
    else the f32 scores of 4/4, 3/4 and 6/8."""
    b = np.asarray(beats, f32)
    if b.size < 8:
        return None
    iv = positive_intervals(b)
    if iv.size == 0:
        return None
    mean = f32(_fold(iv) / f32(iv.size))
    out = []
    for lag in (4, 3, 6):
        if iv.size < lag or iv.size - lag <= 0:
            out.append(f32(0))
            continue
        d = np.abs(iv[:-lag] - iv[lag:]).astype(f32)
        terms = (f32(1) / (f32(1) + d / mean)).astype(f32)
        ac = f32(_fold(terms) / f32(terms.size))
        dev = (iv - mean).astype(f32)
        var = f32(_fold((dev * dev).astype(f32)) / f32(iv.size))
        cv = f32(np.sqrt(var) / mean) if mean > EPS else f32(1)
        cons = f32(f32(1) / f32(f32(1) + cv))
        out.append(min(f32(f32(ac * f32(0.7)) + f32(cons * f32(0.3))), f32(1)))
    return np.array(out, f32)


def pick_signature(scores):
    """(beats per bar, confidence) of three scores: max_by(partial_cmp) keeps the LAST maximum."""
    best, bs = 4, scores[0]
    if not scores[1] < bs:
        best, bs = 3, scores[1]
    if not scores[2] < bs:
        best, bs = 6, scores[2]
    return best, f32(min(max(bs, f32(0)), f32(1)))


def window_starts(hb):
    """The starts detect_tempo_variations visits (the sequential f32 accumulation), or None where it
    takes a single-segment fallback before its loop."""
    hb = np.asarray(hb, f32)
    if hb.size < 4:
        return None
    total = f32(hb[-1] - hb[0])
    if total < 2:
        return None
    seg_dur = min(max(f32(total / f32(4)), f32(4)), f32(8))
    step = f32(seg_dur - f32(seg_dur * f32(0.5)))
    out, cur = [], hb[0]
    while cur < hb[-1]:
        out.append(cur)
        cur = f32(cur + step)
    return out


def _empty(bpm, conf):
    m = {k: 0 for k in SCALARS}
    m["nominal_bpm"], m["nominal_confidence"] = f32(bpm), f32(conf)
    m["time_signature_confidence"] = f32(0)
    m["time_signature_scores"] = np.zeros(3, f32)
    m["segments"] = {k: np.zeros(0, t) for k, t in zip(SEGMENT_FIELDS, _SEG_DTYPES)}
    m["beats"] = np.zeros(0, f32)
    m["hmm"] = np.zeros(0, f32)
    return m


def reference(onsets, bpm, conf, sample_rate):
    """The map of one track from its consensus onsets (sample positions) and the tempo the beat stage
    ran with: the fields of sdsp.tempo_map_to_dict that depend on them, `beats` (the list the result
    publishes, reconstructed) and `hmm` (the whole-track HMM beats)."""
    on = np.asarray(onsets, np.uint32).astype(f32) / f32(sample_rate)
    bpm, conf = f32(bpm), f32(conf)
    m = _empty(bpm, conf)
    if not (bpm > 0 and on.size >= 2) or bpm > 300:  # src/lib.rs:913, generate_beat_grid's InvalidInput
        return m
    hb = oracle.hmm_track(float(bpm), on)
    if hb is None or hb.size == 0:
        return m
    try:
        segs = units.detect_tempo_variations(hb, float(bpm))
    except Exception:
        return m
    rows, refined, tempo = [], [], float(bpm)
    has_var = units.has_tempo_variation(segs)
    for start, end, sbpm, sconf, variable in segs:
        row = [f32(start), f32(end), f32(sbpm), f32(sconf), int(variable), 0, 0, f32(0), f32(0), 0]
        if has_var and variable:
            so = on[(on >= f32(start)) & (on <= f32(end))]
            if so.size:
                try:
                    ub, uc = units.BayesianBeatTracker(tempo, float(conf)).update_with_onsets(so, sample_rate)
                except Exception:
                    return m  # Err propagates: no grid
                tempo = ub
                sb = oracle.hmm_track(ub, so)
                row[5:10] = [1, so.size, f32(ub), f32(uc), 0 if sb is None else sb.size]
                if sb is not None:
                    refined.append(sb)
        elif has_var:
            sel = hb[(hb >= f32(start)) & (hb <= f32(end))]
            row[9] = sel.size
            refined.append(sel)
        rows.append(row)
    beats = hb
    if refined and sum(r.size for r in refined):
        beats = np.sort(np.concatenate(refined).astype(f32), kind="stable")
        m["refined"] = 1
    m["has_grid"], m["has_variation"], m["hmm_beats"], m["n_segments"] = 1, int(has_var), int(hb.size), len(rows)
    m["segments"] = {k: np.array([r[i] for r in rows], t) for i, (k, t) in enumerate(zip(SEGMENT_FIELDS, _SEG_DTYPES))}
    sc = signature_scores(beats)
    if sc is None:
        m["beats_per_bar"], m["time_signature_confidence"] = 4, f32(0.5)
    else:
        m["time_signature_scored"], m["time_signature_scores"] = 1, sc
        m["beats_per_bar"], m["time_signature_confidence"] = pick_signature(sc)
    m["beats"], m["hmm"] = np.asarray(beats, f32), np.asarray(hb, f32)
    return m


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def bits1(v):
    """The bits of one f32 as an int."""
    return int(f32(v).view(np.uint32))


def differences(got, ref, segments=True):
    """The fields of a tempo_map_to_dict that differ from a reference(), floats compared on their bits."""
    bad = [k for k in SCALARS if int(got[k]) != int(ref[k]) and (segments or k != "n_segments")]
    bad += [k for k in FLOATS if bits(got[k]) != bits(ref[k])]
    if not np.array_equal(bits(got["time_signature_scores"]), bits(ref["time_signature_scores"])):
        bad.append("time_signature_scores")
    if segments:
        for k, t in zip(SEGMENT_FIELDS, _SEG_DTYPES):
            a, b = got["segments"][k], ref["segments"][k]
            same = a.size == b.size and (np.array_equal(bits(a), bits(b)) if t is f32 else np.array_equal(a, b))
            if not same:
                bad.append("segments." + k)
    return bad
