"""tests/levels_ref.py (the GPU levels tests' reference) pinned to the oracle at 16 kHz: for every
method raw * gain equals oracle.normalize(raw, method) bit for bit, on the plain, the clip-limited,
the all-gated and the silent branch; the silence map and the trim bounds equal
oracle.units.detect_and_trim's."""
import numpy as np
import pytest

import levels_ref
import oracle
import units

SR = 16000
LENGTHS = {
    levels_ref.PEAK: (1, 5, 1023, 1024, 1025, 6399, 6400, 6401, 12805, 20000),
    levels_ref.RMS: (1, 5, 1023, 1024, 1025, 6399, 6400, 6401, 12805, 20000),
    levels_ref.LOUDNESS: (1, 1025, 6399, 6400, 6401, 12805, 20000),
}
AMPS = (0.1, 0.9, 1e-5, 0.0, "spike")  # plain; loud; every block gated; silent; quiet with one full-scale sample


def _noise(n, amp, seed):
    rng = np.random.default_rng(seed)
    if amp == "spike":  # the RMS and the LUFS gain would clip the one loud sample: both are limited by the peak
        x = (0.01 * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
        x[n // 2] = 0.99
        return x
    return (amp * rng.uniform(-1.0, 1.0, n)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("method", (levels_ref.PEAK, levels_ref.RMS, levels_ref.LOUDNESS))
def test_gain_matches_oracle_normalize(method):
    tracks = [_noise(n, amp, 100 * k + j) for k, n in enumerate(LENGTHS[method]) for j, amp in enumerate(AMPS)]
    meta = levels_ref.loudness(tracks, SR, methods=(method,))
    branches = set()
    for x, m in zip(tracks, meta):
        st, want = oracle.normalize(x, method, SR)
        assert st == 0, want
        g = m[method]["gain"]
        assert np.array_equal(_bits(x * g), _bits(want)), (method, len(x), float(g))
        assert m[method]["measured"] == 1 and m[method]["status"] == 0
        branches.add((int(m[method]["has_lufs"]), bool(np.isinf(m[method]["peak_db"])), float(g) == 1.0))
    # silent tracks leave the samples alone; Loudness sees both the measured and the all-gated branch
    assert any(b[1] for b in branches)
    if method == levels_ref.LOUDNESS:
        assert {b[0] for b in branches} == {0, 1}


def test_metadata_branches():
    P = levels_ref.params(SR)
    loud = _noise(20000, 0.9, 1)
    quiet = _noise(20000, 1e-5, 2)
    m = levels_ref.loudness([loud, quiet, np.zeros(3000, np.float32)], SR)
    # Peak: gain_db is that of target / peak, the applied gain the minimum with 1 / peak
    pk = levels_ref.peak(loud)
    assert m[0][levels_ref.PEAK]["gain"] == np.float32(min(P["target_peak"] / pk, np.float32(1.0) / pk))
    # a quiet track with one full-scale sample: the RMS gain is limited to 1 / peak, the LUFS gain to target / peak
    spike = _noise(20000, "spike", 6)
    ms = levels_ref.loudness([spike], SR)[0]
    assert ms[levels_ref.RMS]["gain"] == np.float32(np.float32(1.0) / np.float32(0.99))
    assert ms[levels_ref.LOUDNESS]["gain"] == np.float32(P["target_peak"] / np.float32(0.99))
    assert ms[levels_ref.LOUDNESS]["has_lufs"] == 1
    # Loudness with every block under the gate is the Peak metadata, without a LUFS value
    assert m[1][levels_ref.LOUDNESS] == m[1][levels_ref.PEAK] and m[1][levels_ref.LOUDNESS]["has_lufs"] == 0
    assert m[0][levels_ref.LOUDNESS]["has_lufs"] == 1 and np.isfinite(m[0][levels_ref.LOUDNESS]["measured_lufs"])
    # exact zeros: -inf, -inf, gain_db 0, gain 1, for every method
    for k in (levels_ref.PEAK, levels_ref.RMS, levels_ref.LOUDNESS):
        z = m[2][k]
        assert z["peak_db"] == -np.inf and z["rms_db"] == -np.inf and z["gain_db"] == 0.0 and z["gain"] == 1.0
    # the gate every gated mean exceeds lies far above the NumericalError threshold
    assert P["gate"] > 1e-7 > 1e-10


def _with_silence(n, runs, seed=3, amp=0.3):
    x = _noise(n, amp, seed)
    for a, b in runs:
        x[a:b] = 0.0
    return x


MAP_CASES = {
    "leading2": _with_silence(30000, [(0, 3 * 1024)]),                       # frames 0-1 silent: kept
    "interior7": _with_silence(40000, [(10 * 1024, 18 * 1024)]),             # 7 silent frames: dropped
    "interior8": _with_silence(40000, [(10 * 1024, 19 * 1024)]),             # 8: kept
    "trailing7": _with_silence(30 * 1024, [(22 * 1024, 30 * 1024)]),         # 7 trailing frames: dropped
    "trailing8": _with_silence(30 * 1024, [(21 * 1024, 30 * 1024)]),         # 8: kept
    "none": _noise(20000, 0.3, 4),
    "all": np.zeros(20000, np.float32),
    "short": _noise(700, 0.3, 5),
    "short_silent": np.zeros(700, np.float32),
}


@pytest.mark.parametrize("name", sorted(MAP_CASES))
def test_silence_map_matches_oracle(name):
    x = MAP_CASES[name]
    regions, ts, te = levels_ref.silence_map(x, SR)
    trimmed, want = units.detect_and_trim(x, SR)
    assert regions == want, (name, regions, want)
    assert te - ts == len(trimmed) and np.array_equal(x[ts:te], trimmed)
    frames = lambda r: (r[1] - r[0]) // 1024  # noqa: E731
    if name == "leading2":
        assert regions == [(0, 2 * 1024)]
    if name in ("interior7", "trailing7"):
        assert regions == [] and (ts, te) == (0, len(x))
    if name == "interior8":
        assert len(regions) == 1 and frames(regions[0]) == 8
    if name == "trailing8":
        assert len(regions) == 1 and regions[0][1] == len(x) and te == regions[0][0]
    if name == "all":
        assert regions == [(0, len(x))] and ts == te
