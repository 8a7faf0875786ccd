"""A second reading of the key vote (CPU only): ref64's float64 smoothing, frame weights, segment
voting and detect_key_weighted over the synthetic chroma rows and energies of the GPU vote tests
(key_vote_cases.py), against the oracle's exported vote (units.key_vote), which the kernel is held
to bit for bit.  A misreading of the reference shared by the oracle and the kernel shows up here.
"""
import numpy as np

import key_vote_cases as kv
import oracle
import ref64
import units


def test_key_vote_matches_the_float64_reading():
    cfg = oracle.default_config()
    tracks = kv.ragged_tracks() + kv.clear_tracks()
    skipped = 0
    for t, (c, e) in enumerate(tracks):
        ties = ref64.Ties()
        key, conf, clarity, used = ref64.key_vote64(c, e, ties=ties)
        if ties:  # a segment's clarity within 1e-4 of its gate: f32 rounding decides whether it votes
            skipped += 1
            continue
        v = units.key_vote(c, e, cfg)
        tag = (t, e.size)
        assert not v["err"], tag
        assert v["key"] == key and v["used_segments"] == used, (tag, v["key"], key, v["used_segments"], used)
        assert abs(float(v["confidence"]) - conf) <= 1e-4 and abs(float(v["clarity"]) - clarity) <= 1e-4, (
            tag, v["confidence"], conf, v["clarity"], clarity)
    assert skipped * 10 <= len(tracks), skipped
