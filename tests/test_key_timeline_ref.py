"""tests/key_timeline_ref.py against the oracle and against hand-written cases: the chain that
rebuilds the chroma rows reproduces the trace's checksums on the configurations and frame counts
the GPU tests use, the primary-key and change logic, and the known answer of a modulating track."""
import numpy as np
import pytest

import key_timeline_ref as K
import oracle
import synth

SR = 44100
f32 = np.float32


def _cfg(**opts):
    c = oracle.default_config()
    for k, v in opts.items():
        setattr(c, k, v)
    return c


CHAIN_CFGS = {
    "default": dict(),
    "override_off": dict(enable_key_stft_override=0),
    "kfs4096_hop1024": dict(key_stft_frame_size=4096, key_stft_hop_size=1024),
}


@pytest.mark.parametrize("case", sorted(CHAIN_CFGS))
def test_chain_reproduces_the_trace_checksums(case):
    cfg = _cfg(**CHAIN_CFGS[case])
    x = synth.make_track(8100, seconds=6.0)[0]
    status, first, rows = K.chroma_rows(x, SR, cfg)  # asserts n_key_frames, chroma_sum, chroma_sq
    kfs, khop = K.key_stft(cfg)
    assert status == 0 and rows.shape[1] == 12 and rows.shape[0] > 5
    assert (kfs, khop) == {"default": (8192, 512), "override_off": (2048, 512), "kfs4096_hop1024": (4096, 1024)}[case]
    assert rows.shape[0] <= (x.size - kfs) // khop + 1  # (trimming may shorten the track)


@pytest.mark.parametrize("F", [1, 5, 6, 7])
def test_chain_on_few_frames(F):
    """F <= 5 rows are not smoothed, F > 5 are: both sides of smooth_chroma's threshold."""
    cfg = _cfg(enable_silence_trimming=0)
    x = synth.make_track(8101, seconds=2.0)[0][1000:1000 + 8192 + (F - 1) * 512 + 100]
    status, first, rows = K.chroma_rows(x, SR, cfg)
    assert status == 0 and first == 0 and rows.shape == (F, 12)


def test_key_path_skipped_gives_no_rows():
    cfg = _cfg(enable_silence_trimming=0)
    x = synth.make_track(8102, seconds=1.0)[0][:8191]
    assert K.chroma_rows(x, SR, cfg) == (0, 0, None)
    t = K.timeline_ref(x, SR, cfg, dict(segment_frames=1, hop_frames=1))
    assert t["n_frames"] == 0 and t["n_segments"] == 0 and t["primary_key"] == -1 and t["status"] == 0


def test_primary_key_logic():
    assert K.primary([], []) == (-1, f32(0), 0)
    assert K.primary([5], [f32(0.25)]) == (5, f32(0.25), 1)
    # a count tie (two segments each) goes to the key whose first segment is earliest
    k, c, n = K.primary([7, 3, 3, 7, 1], [f32(0.1), f32(0.2), f32(0.4), f32(0.3), f32(0.9)])
    assert (k, n) == (7, 2) and c == f32(f32(f32(0.1) + f32(0.3)) / f32(2))
    k, c, n = K.primary([3, 7, 7, 3], [f32(0.5)] * 4)
    assert (k, n) == (3, 2)
    # no tie: the most frequent key, wherever it first occurs
    assert K.primary([1, 2, 2, 2, 1], [f32(0)] * 5)[::2] == (2, 3)
    # the f32 sum runs in segment order
    confs = [f32(1.0), f32(2.0 ** -24), f32(2.0 ** -24)]
    tot = f32(f32(f32(1.0) + confs[1]) + confs[2])
    assert K.primary([4, 4, 4], confs)[1] == f32(tot / f32(3))


def test_change_logic_threshold_is_strict():
    keys, confs, ts = [0, 0, 6, 6, 2], [f32(0.2), f32(0.2), f32(0.2), f32(0.6), f32(0.0)], [f32(i) for i in range(5)]
    every = K.changes(keys, confs, ts, -1.0)
    assert [(c[0], c[2], c[3]) for c in every] == [(2, 0, 6), (4, 6, 2)]
    assert every[0][4] == f32(0.2) and every[1][4] == f32(f32(f32(0.6) + f32(0.0)) / f32(2)) and every[0][1] == f32(2)
    # (0.2 + 0.2) / 2 == 0.2 is not > 0.2: the reference's threshold drops it, keeps 0.3
    assert [c[0] for c in K.changes(keys, confs, ts, 0.2)] == [4]
    assert [c[0] for c in K.changes(keys, confs, ts, f32(0.2) - f32(2.0 ** -26))] == [2, 4]
    assert K.changes(keys, confs, ts, 0.3) == []
    # a confidence of exactly 0 is reported only below 0
    assert len(K.changes([0, 1], [f32(0), f32(0)], ts, 0.0)) == 0 and len(K.changes([0, 1], [f32(0), f32(0)], ts, -1.0)) == 1
    assert K.changes([], [], [], -1.0) == [] and K.changes([3], [f32(1)], [f32(0)], -1.0) == []


def test_timeline_of_zero_and_one_segments():
    rows = np.random.default_rng(1).random((10, 12), dtype=f32)
    t0 = K.timeline(rows, 11, 1, SR, 512)
    assert t0["n_segments"] == 0 and t0["n_frames"] == 10 and t0["primary_key"] == -1 and t0["primary_count"] == 0
    assert t0["segments"]["top_keys"].shape == (0, 3) and t0["changes"]["segment"].shape == (0,)
    t1 = K.timeline(rows, 10, 10, SR, 512)
    assert t1["n_segments"] == 1 and t1["n_changes"] == 0 and t1["primary_count"] == 1
    assert t1["primary_key"] == int(t1["segments"]["key"][0]) and t1["primary_confidence"] == t1["segments"]["confidence"][0]
    assert t1["segments"]["start_frame"][0] == 0 and t1["segments"]["timestamp"][0] == 0.0


def test_seconds_form_truncates_f32_products():
    assert K.plan(dict(segment_seconds=8.0, overlap_seconds=2.0), 44100, 512) == (689, 517)
    assert K.plan(dict(segment_seconds=4.0, overlap_seconds=1.0), 44100, 512) == (344, 258)
    assert K.plan(dict(segment_frames=64, hop_frames=3), 44100, 512) == (64, 3)
    for bad in (dict(), dict(segment_seconds=1.0, segment_frames=4, hop_frames=1), dict(segment_seconds=float("inf")),
                dict(segment_seconds=-1.0), dict(segment_seconds=1.0, overlap_seconds=1.0), dict(segment_seconds=0.001),
                dict(segment_frames=4), dict(hop_frames=4), dict(segment_frames=2 ** 31, hop_frames=1),
                dict(segment_seconds=1.0, min_change_confidence=float("nan"))):
        assert isinstance(K.plan(bad, 44100, 512), str), bad


def test_modulating_track_known_answer():
    """16 s of C major cadences, then 16 s of F sharp major; 8 s segments overlapping by 2 s are 689
    frames every 517, so four segments starting at 0, 6, 12 and 18 s: C, C, then (its second half
    already F sharp, and louder in the smoothed rows' fold) F sharp, F sharp.  Every confidence is
    exactly 0 (both modes score, so the top major and top minor key tie at 1.2), which is why the
    reference's threshold of 0.2 reports nothing."""
    x = K.modulating_track()
    cfg = _cfg()
    chain = K.chroma_rows(x, SR, cfg)
    assert chain[2].shape[0] == 2741
    t = K.timeline_ref(x, SR, cfg, dict(segment_seconds=8.0, overlap_seconds=2.0), chain=chain)
    assert (t["segment_frames"], t["hop_frames"], t["n_segments"]) == (689, 517, 4)
    assert t["segments"]["key"].tolist() == [0, 0, 6, 6]
    assert t["segments"]["start_frame"].tolist() == [0, 517, 1034, 1551]
    assert not t["segments"]["confidence"].any()
    assert np.all(t["segments"]["top_scores"][:, :2] == f32(1.2))
    assert (t["primary_key"], t["primary_count"], float(t["primary_confidence"])) == (0, 2, 0.0)
    assert t["n_changes"] == 1 and t["changes"]["segment"].tolist() == [2]
    assert t["changes"]["timestamp"][0] == f32(f32(1034) / (f32(44100) / f32(512)))
    assert (t["changes"]["from_key"][0], t["changes"]["to_key"][0]) == (0, 6)
    ref = K.timeline_ref(x, SR, cfg, dict(segment_seconds=8.0, overlap_seconds=2.0, min_change_confidence=0.2), chain=chain)
    assert ref["n_changes"] == 0 and ref["segments"]["key"].tolist() == [0, 0, 6, 6]
