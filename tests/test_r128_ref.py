"""tests/r128_ref.py, the numpy statement of the programme loudness contract (include/stratum_hip.h,
sdsp_r128), against what it has to mean: the standard's coefficient table, the standard's own
conformance tone, an unbroken f64 BS.1770 filter over the whole track, and a tone whose true peak
lies between its samples."""
import numpy as np
import pytest

import r128_ref as R

f32 = np.float32
SR = 48000


def _noise(n, amp, seed):
    return (np.random.default_rng(seed).standard_normal(n) * amp).astype(f32).clip(-1.0, 1.0)


def two_level(sr, seed=31):
    """4 s of noise, then 5 s of it 30 dB lower: whole short-term blocks lie under both relative gates."""
    return np.concatenate([_noise(4 * sr, 0.25, seed), _noise(5 * sr, 0.25 * 10.0 ** (-30.0 / 20.0), seed + 1)])


def assert_gates_exercised(r):
    """The reference itself drops and keeps a block at each relative gate."""
    for k in ("momentary", "short_term"):
        under_abs, under_rel, kept = r["gates"][k]
        assert under_rel >= 1 and kept >= 1, (k, r["gates"][k])


def test_coefficients_at_48k_are_the_standards_table():
    shelf, hp = R.coeffs64(48000)
    assert np.max(np.abs(np.array(shelf) - [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241,
                                            0.73248077421585])) < 1e-12
    assert np.max(np.abs(np.array(hp) - [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621])) < 1e-12


@pytest.mark.parametrize("sr", [48000, 44100])
def test_conformance_sine_reads_minus_3_01(sr):
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(3 * sr) / sr).astype(f32)
    r = R.measure([x], sr, R.LOUDNESS)[0]
    print("997 Hz full scale at", sr, ":", r["integrated_lufs"])
    assert r["has_integrated"] == 1 and abs(float(r["integrated_lufs"]) + 3.01) <= 0.1


def test_contract_is_within_a_hundredth_of_an_unbroken_f64_filter():
    tracks = {"two_level": two_level(SR), "noise": _noise(5 * SR + 777, 0.1, 11),
              "dc": (_noise(5 * SR, 0.1, 12) + f32(0.3)).astype(f32)}
    got = R.measure(list(tracks.values()), SR, R.LOUDNESS | R.CURVES)
    assert_gates_exercised(got[0])  # before anything else: the two-level track does what it is there for
    worst = 0.0
    for (name, x), r in zip(tracks.items(), got):
        integ, m, s = R.unbroken(x, SR)
        dm = np.max(np.abs(np.array([float(R.lufs(e)) for e in r["momentary"]]) - m))
        ds = np.max(np.abs(np.array([float(R.lufs(e)) for e in r["short_term"]]) - s))
        di = abs(float(r["integrated_lufs"]) - integ)
        print(name, "integrated", r["integrated_lufs"], integ, "deviations", di, dm, ds)
        assert r["has_integrated"] == 1 and m.size == r["n_momentary"] and s.size == r["n_short_term"] and s.size > 0
        assert di <= 0.01 and dm <= 0.01 and ds <= 0.01, (name, di, dm, ds)
        worst = max(worst, di, dm, ds)
    print("largest deviation", worst)


def quarter_rate_sine(n=4096, ramp=64):
    """sin at sr/4 with phase 45 degrees (samples of +-0.7071, peaks of 1 half-way between them),
    faded in and out over `ramp` samples.  The fade belongs to the case: x is 0 outside the track, so
    an unfaded tone starts with a step from 0 to 0.7071, and any band-limited interpolator overshoots
    a step (this one reads +0.10 dBTP at sample 2 of the unfaded tone, -0.03 everywhere else).  The
    case is about the tone's inter-sample peak, not about that edge."""
    x = np.sin(2.0 * np.pi * np.arange(n) / 4.0 + np.pi / 4.0)
    w = np.ones(n)
    w[:ramp] = 0.5 - 0.5 * np.cos(np.pi * np.arange(ramp) / ramp)
    w[n - ramp:] = w[:ramp][::-1]
    return (x * w).astype(f32)


def test_true_peak_of_a_quarter_rate_sine():
    x = quarter_rate_sine()
    r = R.measure([x], SR, R.TRUE_PEAK)[0]
    print("sr/4 sine at 45 degrees:", r["sample_peak_db"], r["true_peak_dbtp"])
    assert abs(float(r["sample_peak_db"]) + 3.0103) < 0.005
    assert -0.15 <= float(r["true_peak_dbtp"]) <= 0.1
    assert r["n_steps"] == 0 and r["has_integrated"] == 0  # (no loudness was asked for)


def test_edges_of_the_definition():
    sr = 8000
    xs = [np.zeros(0, f32), _noise(1, 0.1, 1), _noise(799, 0.1, 2), _noise(800, 0.1, 3), _noise(3200, 0.1, 4),
          np.zeros(24000, f32), _noise(24000, 1e-5, 5)]
    r = R.measure(xs[1:], sr)
    assert [q["n_steps"] for q in r] == [0, 0, 1, 4, 30, 30]
    assert [q["n_momentary"] for q in r] == [0, 0, 0, 1, 27, 27] and [q["n_short_term"] for q in r] == [0, 0, 0, 0, 1, 1]
    assert r[3]["has_integrated"] == 1 and r[3]["has_range"] == 0
    zero, quiet = r[4], r[5]
    assert zero["has_integrated"] == 0 and zero["integrated_lufs"] == -np.inf and zero["max_momentary_lufs"] == -np.inf
    assert zero["sample_peak_db"] == -np.inf and zero["true_peak"] == 0
    # under the absolute gate: blocks, finite maxima, nothing integrated, no range
    assert quiet["has_integrated"] == 0 and quiet["has_range"] == 0 and np.isfinite(quiet["max_short_term_lufs"])
    assert float(quiet["max_momentary_lufs"]) < -70.0 and quiet["range_lu"] == 0
