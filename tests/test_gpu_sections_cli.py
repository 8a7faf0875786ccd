"""analyze_batch --sections: the "sections" member of each JSON line is what the binding returns for
the same audio, and without the flag the lines are what they were."""
import json
import os
import subprocess

import numpy as np
import pytest

import sdsp
import sections_ref as S

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


def test_cli_sections_member():
    path = os.path.join(GOLDEN, "120bpm_4bar.wav")
    base = [os.path.join(BIN, "analyze_batch"), "--json", "--jobs", "1", "--devices", "1"]
    plain = subprocess.run(base + [path], capture_output=True, text=True, timeout=300)
    full = subprocess.run(base + ["--sections", path], capture_output=True, text=True, timeout=300)
    part = subprocess.run(base + ["--sections=0.25:2:1:0.5:0.1", "--tempo-map=segments", path], capture_output=True, text=True,
                          timeout=300)
    for p in (plain, full, part):
        assert p.returncode == 0, p.stderr
    for arg in ("--sections=0", "--sections=0.5:65", "--sections=0.5:2:1.5", "--sections=0.5:2:1:1:1:1", "--sections=x"):
        bad = subprocess.run(base + [arg, path], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 1 and "--sections takes" in bad.stderr, arg
    assert list(json.loads(plain.stdout.splitlines()[0])) == PLAIN_KEYS
    a, f, p = _rows(plain), _rows(full), _rows(part)
    x, sr = sdsp.decode_audio_file(path)
    x = np.ascontiguousarray(x, f32)
    buf = sdsp.DeviceBuffer(x.size + 8)
    buf.from_host(x)
    for rows, req in ((f, dict(cell_seconds=0.5, kernel_cells=16, min_gap_cells=8, energy_weight=1.0, min_strength=0.5,
                               snap_seconds=0.5)),
                      (p, dict(cell_seconds=0.25, kernel_cells=2, min_gap_cells=1, energy_weight=0.5, min_strength=0.1,
                               snap_seconds=0.25))):
        out = sdsp.analyze_batch_device_with(buf.ptr, [0], [x.size], sr, sdsp.default_config(),
                                             sections=sdsp.sections_request(**req))
        out[0].free()
        want, r = out[-1][0], dict(rows[0])
        assert list(r)[-1] == "sections"
        sc = r.pop("sections")
        r.pop("tempo_map", None)
        assert r == a[0]
        got = dict(sc, gmax=f32(sc["gmax"]), nmax=f32(sc["nmax"]), novelty=np.array(sc["novelty"], f32),
                   energy=np.array(sc["energy"], f32))
        dts = dict(start_cell=np.uint64, end_cell=np.uint64, downbeat=np.int32)
        got["sections"] = {k: np.array([row[j] for row in sc["sections"]], dts.get(k, f32))
                           for j, k in enumerate(sdsp.SECTION_FIELDS)}
        S.assert_equal(got, want, req)
        assert sc["n_sections"] == len(sc["sections"]) >= 1 and sc["n_curve"] == sc["n_cells"] == len(sc["novelty"]) > 0
    assert f[0]["sections"]["cell_samples"] == 22050 and p[0]["sections"]["cell_samples"] == 11025
    assert "tempo_map" in p[0] and all("sections" not in r for r in a)
