"""Synthetic inputs of the key vote tests (test_gpu_key_vote.py, test_ref64_key_vote.py): chroma rows
and frame energies made directly, no audio and no STFT, so every branch and boundary of the vote is
reached on purpose, with the configurations that reach them and the adversarial energies of the
certificate's soundness test.
"""
import ctypes as C

import numpy as np

import oracle

TEMPERLEY = 1  # SDSP_TEMPLATES_TEMPERLEY


def make_track(seed, frames, keys, noise, sigma, x_scale=1.0, x_key=None):
    """(chroma (F, 12) f32, energies (F,) f32).  A row for key k is the L2-normalised K-K template row
    plus noise * N(0, 1) per class, clamped at 0, cubed (without the cube the rows' tonalness, and
    with it every frame weight, is close to 0), then L2-normalised.  Energies are exp(N(0, sigma));
    those of the frames of key x_key are scaled by x_scale.  A few rows are exact zeros of energy 0.
    keys: one key index for the track, or one per frame."""
    rng = np.random.default_rng(seed)
    T = oracle.key_templates().astype(np.float64)
    k = np.broadcast_to(np.asarray(keys, np.int64), (frames,))
    rows = np.maximum(T[k] + noise * rng.standard_normal((frames, 12)), 0.0) ** 3
    n = np.sqrt((rows * rows).sum(axis=1))
    rows = rows / np.where(n > 0, n, 1.0)[:, None]
    e = np.exp(rng.normal(0.0, sigma, frames))
    if x_key is not None:
        e = np.where(k == x_key, e * x_scale, e)
    nz = min(3, frames // 8)
    if nz:
        z = rng.choice(frames, nz, replace=False)
        rows[z] = 0.0
        e[z] = 0.0
    return rows.astype(np.float32), e.astype(np.float32)


# F <= 5 (no smoothing); 9 / 10 / 11 (one zero row each: 8, 9 and 10 used frames, the unweighted
# fallback's boundary); the edge trim's 200; the default segment length and its neighbours, two and
# three segments, block_seq_sum's 2048-frame chunk and the 4,097 rows of a long track
RAGGED_FRAMES = (1, 5, 6, 9, 10, 11, 199, 200, 201, 1023, 1024, 1025, 1536, 2047, 2048, 2049, 2560, 4097)


def ragged_tracks(frames=RAGGED_FRAMES, seed=1000):
    return [make_track(seed + i, F, (7 * i) % 24, 0.15, 1.0) for i, F in enumerate(frames)]


def clear_tracks():
    """12 tracks of one key each, clear enough that no decision is near (test d asserts how clear)."""
    return [make_track(2000 + t, (1024, 1536, 2049, 2560)[t % 4], (7 * t) % 24, 0.15, 1.0) for t in range(12)]


CONTESTED = dict(key_segment_len_frames=120, key_segment_hop_frames=40)


def contested_tracks(seeds=range(40)):
    """F = 400 with segments of 120 every 40: frames alternate in blocks of 8 between keys 0 and 7,
    and the energies of the key-0 frames are scaled so the two keys' segment scores nearly balance."""
    keys = np.where((np.arange(400) // 8) % 2 == 0, 0, 7)
    return [make_track(3000 + s, 400, keys, 0.05, 0.3, 1.0 + 0.02 * (s % 11 - 5), 0) for s in seeds]


def contested_long_tracks(seeds=range(12)):
    """The same alternation over F = 2048 under the default configuration's 1,024-frame segments:
    the certificate's pair pass then sums over more frames than any instantiation has threads."""
    keys = np.where((np.arange(2048) // 8) % 2 == 0, 0, 7)
    return [make_track(4000 + s, 2048, keys, 0.05, 0.3, 1.0 + 0.02 * (s % 11 - 5), 0) for s in seeds]


# name -> (configuration fields, frame counts of the ragged call that reach the branch)
_SEG120 = dict(key_segment_len_frames=120, key_segment_hop_frames=1)
CONFIGS = {
    "default": ({}, RAGGED_FRAMES),
    "seg120_hop1": (_SEG120, (119, 120, 121, 400)),  # F = 400: 281 segments, more than 256 threads
    "hop_over_len": (dict(key_segment_len_frames=120, key_segment_hop_frames=500), (120, 239, 240, 400)),
    "min_clarity_1": (dict(key_segment_min_clarity=1.0), (1024, 1536, 2049)),  # every gate fails: detect_full
    "edge_trim": (dict(enable_key_edge_trim=1), (71, 72, 199, 200, 201, 1463, 1464, 2049)),
    "edge_trim_0.49": (dict(enable_key_edge_trim=1, key_edge_trim_fraction=0.6), (200, 2500, 2600, 4097)),
    "sharpen2": (dict(chroma_sharpening_power=2.0), (5, 6, 200, 1024, 1536)),
    "no_weighting": (dict(enable_key_frame_weighting=0), (6, 11, 1024, 1536)),
    "min_tonal_0.9": (dict(key_min_tonalness=0.9), (11, 200, 1024, 1536)),  # forces the unweighted fallback
    "mode_heuristic": (dict(enable_key_mode_heuristic=1), (6, 200, 1024, 1536, 2049)),
    "minor_bonus": (dict(enable_key_minor_harmonic_bonus=1), (6, 200, 1024, 1536, 2049)),
    "heuristic_bonus": (dict(enable_key_mode_heuristic=1, enable_key_minor_harmonic_bonus=1,
                             key_mode_flip_min_score_ratio=0.5, key_minor_leading_tone_bonus_weight=1.0),
                        (6, 200, 1024, 1536, 2049)),
    "temperley": (dict(key_template_set=TEMPERLEY), (6, 200, 1024, 1536)),
    "ensemble": (dict(enable_key_ensemble=1), (1, 6, 11, 200, 1024, 2049)),
    "multi_scale": (dict(enable_key_multi_scale=1, key_multi_scale_lengths=[120, 256, 1024], key_multi_scale_hop=60,
                         key_multi_scale_weights=[1.0, 0.0, 2.0]), (119, 120, 255, 256, 400, 1023, 1024, 1536)),
    "multi_scale_long": (dict(enable_key_multi_scale=1, key_multi_scale_lengths=[120, 5000], key_multi_scale_hop=60,
                              key_multi_scale_weights=[1.0, -1.0]), (120, 400, 4097)),
    "multi_scale_none_pass": (dict(enable_key_multi_scale=1, key_multi_scale_min_clarity=1.0), (120, 400, 1024)),
}


def config(opts, keep):
    """The default configuration with `opts` set; keep holds the arrays its pointers refer to."""
    cfg = oracle.default_config()
    for k, v in opts.items():
        if k in ("key_multi_scale_lengths", "key_multi_scale_weights"):
            arr = np.ascontiguousarray(v, dtype=np.uint64 if k.endswith("lengths") else np.float32)
            keep.append(arr)
            ct = C.c_uint64 if k.endswith("lengths") else C.c_float
            setattr(cfg, k, arr.ctypes.data_as(C.POINTER(ct)))
            setattr(cfg, k + "_len", arr.size)
        else:
            setattr(cfg, k, v)
    return cfg


def adversarial_energies(e, d, signs):
    """e' = e (1 + s 0.999 d) in float64 rounded to f32, every value then stepped toward e until
    |e' - e| <= d e holds in float64 (the certificate's premise)."""
    e64 = e.astype(np.float64)
    out = (e64 * (1.0 + np.asarray(signs, np.float64) * 0.999 * d)).astype(np.float32)
    for _ in range(4):
        bad = np.abs(out.astype(np.float64) - e64) > d * e64
        if not bad.any():
            break
        out[bad] = np.nextafter(out[bad], e[bad])
    assert not (np.abs(out.astype(np.float64) - e64) > d * e64).any()
    return out


def within_mode_tops(raw):
    """key_from_raw's within-mode argmaxes (the last maximum) of (n, 24) raw scores: (n, 2)."""
    raw = np.asarray(raw, np.float32).reshape(-1, 24)
    return np.stack([11 - np.argmax(raw[:, :12][:, ::-1], axis=1), 11 - np.argmax(raw[:, 12:][:, ::-1], axis=1)], axis=1)


def sign_patterns(ref, cfg_opts, seed):
    """The sign patterns of the soundness test for one track from its oracle vote `ref`: all +, all -,
    random, and, for the three segments with the smallest relative within-mode top-two gap, + on the
    frames whose smoothed row favours the runner-up over the winner and - on the others, and that
    pattern negated.  Signs are over the track's frames."""
    F = ref["chroma_s"].shape[0]
    rng = np.random.default_rng(seed)
    pats = [np.ones(F), -np.ones(F), rng.choice([-1.0, 1.0], F)]
    raw = ref["seg_raw"]
    if raw.shape[0]:
        L = int(cfg_opts.get("key_segment_len_frames", 1024))
        hop = max(min(int(cfg_opts.get("key_segment_hop_frames", 512)), L), 1)
        T = oracle.key_templates().astype(np.float64)
        D = ref["chroma_s"].astype(np.float64) @ T.T  # (F, 24) template dots
        gaps = []
        for s in range(raw.shape[0]):
            for m in range(2):
                r = raw[s, 12 * m:12 * m + 12].astype(np.float64)
                o = np.argsort(-r, kind="stable")
                if r[o[0]] > 0:
                    gaps.append(((r[o[0]] - r[o[1]]) / r[o[0]], s, 12 * m + int(o[0]), 12 * m + int(o[1])))
        gaps.sort()
        for _, s, W, k in gaps[:3]:
            p = -np.ones(F)
            sl = slice(ref["t0"] + s * hop, ref["t0"] + s * hop + L)
            p[sl] = np.where(D[sl, k] > D[sl, W], 1.0, -1.0)
            pats += [p, -p]
    return pats
