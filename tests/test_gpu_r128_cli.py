"""analyze_batch --loudness: the "loudness" member of each JSON line holds the reference's values
(tests/r128_ref.py) for the same audio, and without the flag the lines are what they were."""
import json
import os
import subprocess

import numpy as np
import pytest

import r128_cases as RC
import r128_ref as R
import sdsp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "stratum-dsp_amd", "bin")
PLAIN_KEYS = ["file", "bpm", "bpm_confidence", "key", "key_confidence", "processing_time_ms", "tempogram_multi_res_triggered",
              "tempogram_multi_res_used", "tempogram_percussive_triggered", "tempogram_percussive_used"]
f32 = np.float32


def _rows(out):
    rows = []
    for ln in out.stdout.splitlines():
        r = json.loads(ln)
        r.pop("processing_time_ms", None)
        rows.append(r)
    return rows


def _f32(v):
    return f32(-np.inf) if v is None else f32(v)


def test_cli_loudness_member():
    path = os.path.join(GOLDEN, "120bpm_4bar.wav")
    base = [os.path.join(BIN, "analyze_batch"), "--json", "--jobs", "1", "--devices", "1"]
    plain = subprocess.run(base + [path], capture_output=True, text=True, timeout=300)
    tp = subprocess.run(base + ["--loudness=true-peak", path], capture_output=True, text=True, timeout=300)
    both = subprocess.run(base + ["--loudness=true-peak,curves", "--levels", "peak", path], capture_output=True, text=True,
                          timeout=300)
    bare = subprocess.run(base + ["--loudness", path], capture_output=True, text=True, timeout=300)
    for p in (plain, tp, both, bare):
        assert p.returncode == 0, p.stderr
    for arg in ("--loudness=", "--loudness=peak", "--loudness=true-peak,,curves"):
        bad = subprocess.run(base + [arg, path], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 1 and "--loudness=LIST takes" in bad.stderr, arg
    assert list(json.loads(plain.stdout.splitlines()[0])) == PLAIN_KEYS
    a = _rows(plain)
    x, sr = sdsp.decode_audio_file(path)
    ref = R.measure([np.ascontiguousarray(x, f32)], sr)[0]
    for out, what in ((tp, R.LOUDNESS | R.TRUE_PEAK), (both, RC.ALL), (bare, R.LOUDNESS)):
        r = _rows(out)[0]
        assert list(r)[-1] == "loudness"
        ld = r.pop("loudness")
        r.pop("levels", None)
        assert r == a[0]  # the other fields equal a run without the flag
        want = RC.masked(ref, what)
        assert ("true_peak" in ld) == bool(what & R.TRUE_PEAK) and ("momentary" in ld) == bool(what & R.CURVES)
        for k in ("status", "n_samples", "step_samples", "n_steps", "n_momentary", "n_short_term", "n_gated_momentary",
                  "n_gated_short_term"):
            assert ld[k] == int(want[k]), (what, k)
        assert (ld["integrated_lufs"] is not None) == bool(want["has_integrated"]) and (ld["range_lu"] is not None) == bool(want["has_range"])
        for k in R.FLOATS:
            if k in ld and not (k.startswith("range") and not want["has_range"]):
                assert RC.bits(_f32(ld[k]))[0] == RC.bits(want[k])[0], (what, k, ld[k], want[k])
        if what & R.CURVES:
            for k in ("momentary", "short_term"):
                assert np.array_equal(RC.bits(np.array(ld[k], f32)), RC.bits(want[k])), (what, k)
    assert ref["has_integrated"] == 1 and ref["n_momentary"] > 0
    assert "levels" in _rows(both)[0] and all("loudness" not in r for r in a)
