"""analyze_batch --tempo-map: the "tempo_map" member of each JSON line is what the binding returns for
the same audio, and without the flag the lines are what they were."""
import json
import os
import subprocess

import numpy as np
import pytest

import sdsp
import tempo_map_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "stratum-dsp_amd", "bin")
PLAIN_KEYS = ["file", "bpm", "bpm_confidence", "key", "key_confidence", "processing_time_ms", "tempogram_multi_res_triggered",
              "tempogram_multi_res_used", "tempogram_percussive_triggered", "tempogram_percussive_used"]


def _rows(out):
    rows = []
    for ln in out.stdout.splitlines():
        r = json.loads(ln)
        r.pop("processing_time_ms", None)
        rows.append(r)
    return rows


def test_cli_tempo_map_member():
    path = os.path.join(GOLDEN, "120bpm_4bar.wav")
    base = [os.path.join(BIN, "analyze_batch"), "--json", "--jobs", "1", "--devices", "1"]
    plain = subprocess.run(base + [path], capture_output=True, text=True, timeout=300)
    full = subprocess.run(base + ["--tempo-map", path], capture_output=True, text=True, timeout=300)
    part = subprocess.run(base + ["--tempo-map=segments", "--levels", "peak", path], capture_output=True, text=True, timeout=300)
    bad = subprocess.run(base + ["--tempo-map=beats", path], capture_output=True, text=True, timeout=300)
    for p in (plain, full, part):
        assert p.returncode == 0, p.stderr
    assert bad.returncode == 1 and "segments,onsets" in bad.stderr
    # without the flag: the members the line has always had, in their order, and nothing else
    assert list(json.loads(plain.stdout.splitlines()[0])) == PLAIN_KEYS
    a, f, p = _rows(plain), _rows(full), _rows(part)
    x, sr = sdsp.decode_audio_file(path)
    x = np.ascontiguousarray(x, np.float32)
    buf = sdsp.DeviceBuffer(x.size + 8)
    buf.from_host(x)
    for rows, what in ((f, ("segments", "onsets")), (p, ("segments",))):
        batch, _, _, _, maps = sdsp.analyze_batch_device_with(buf.ptr, [0], [x.size], sr, sdsp.default_config(),
                                                               tempo_map=sdsp.tempo_map_request(what))
        batch.free()
        want, r = maps[0], dict(rows[0])
        tm = r.pop("tempo_map")
        r.pop("levels", None)
        assert r == a[0]
        for k in ("status", "has_grid", "has_variation", "refined", "hmm_beats", "beats_per_bar", "time_signature_scored",
                  "first_sample", "n_segments", "n_onsets"):
            assert tm[k] == want[k], (what, k)
        for k in ("nominal_bpm", "nominal_confidence", "time_signature_confidence"):
            assert R.bits1(tm[k]) == R.bits1(want[k]), (what, k)
        assert np.array_equal(R.bits(tm["time_signature_scores"]), R.bits(want["time_signature_scores"]))
        assert tm["onsets"] == want["onsets"].tolist()
        assert len(tm["segments"]) == want["n_segments"]
        for i, row in enumerate(tm["segments"]):
            for j, k in enumerate(sdsp.TEMPO_SEGMENT_FIELDS):
                w = want["segments"][k][i]
                assert (R.bits1(row[j]) == R.bits1(w)) if w.dtype == np.float32 else row[j] == int(w), (what, i, k)
    assert f[0]["tempo_map"]["has_grid"] == 1 and f[0]["tempo_map"]["beats_per_bar"] == 3 and f[0]["tempo_map"]["n_onsets"] >= 2
    assert p[0]["tempo_map"]["n_onsets"] == 0 and "peak" in p[0]["levels"]
    assert all("tempo_map" not in r for r in a)
