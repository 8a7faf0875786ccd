"""bench.py's command line: a plain run prints the headline line alone, `--full` adds the legs that
take runs of their own, `--dump-outputs DIR` writes what the last timed step returned.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


@pytest.mark.parametrize("full", [False, True])
def test_dry_run_line_and_dump(tmp_path, full):
    """Without a GPU: --steps sets the timed steps, the line carries the headline fields and says
    whether it is a --full one, and the dump holds one status per track."""
    d = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--tracks", "5", "--seconds", "1", "--dry-run",
               "--dump-outputs", str(tmp_path / "o"), *(["--full"] if full else []))
    assert all(k in d for k in HEADLINE) and d["full"] is full
    assert d["steps"] == 3 and len(d["step_ms"]["all"]) == 3
    assert abs(d["value"] - 5 * 3 / (d["ms_per_step"] * 3 / 1000.0)) / d["value"] < 1e-2
    a = _load(str(tmp_path / "o"))
    assert a["status"].dtype == np.float32 and a["status"].tolist() == [0.0] * 5
    assert a["tracks"].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]


class _FakeBatch:
    """A result batch of n tracks, track i with 10 * (i % 7) beats, through the accessors
    dump_outputs uses (sdsp.ResultBatch.field / .values)."""

    def __init__(self, n):
        self.status = [0] * n

    def field(self, name, failed=0):
        return [float(i) for i in range(len(self.status))]

    def values(self, name, count):
        k = 10 if name == "beats" else 1
        return [np.full(k * (i % 7), i, np.float32) for i in range(len(self.status))]


def test_dump_cap_writes_a_fixed_sample(tmp_path, monkeypatch):
    """Past the size cap a seeded sample of the tracks is written: within the cap, the same tracks
    on every call, each array holding exactly those tracks' values."""
    sys.path.insert(0, ROOT)
    import bench

    n, cap = 200, 6000
    res = _FakeBatch(n)
    bench.dump_outputs(str(tmp_path / "all"), res, 0, 1)
    whole = _load(str(tmp_path / "all"))
    assert whole["tracks"].tolist() == [float(i) for i in range(n)]
    assert sum(v.nbytes for v in whole.values()) > cap
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", cap)
    bench.dump_outputs(str(tmp_path / "a"), res, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), res, 0, 1)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == sorted(b) == sorted(whole) and all(a[k].tobytes() == b[k].tobytes() for k in a)
    total = sum(v.nbytes for v in a.values())
    assert cap // 2 < total <= cap, total  # the cap is used, not merely respected
    t = a["tracks"].astype(int)
    assert 0 < t.size < n and (np.diff(t) > 0).all() and t.tolist() != list(range(t.size))  # a sample, not a prefix
    assert a["bpm"].tolist() == t.astype(float).tolist() and a["flags"].dtype == np.float64
    assert a["n_beats"].tolist() == [10.0 * (i % 7) for i in t]
    assert a["beats"].tolist() == [float(i) for i in t for _ in range(10 * (i % 7))]
    assert a["n_bars"].tolist() == [float(i % 7) for i in t] and a["bars"].size == int(a["n_bars"].sum())


@pytest.mark.gpu
def test_full_run_keeps_its_legs():
    """--full on four 20-s tracks: the line still carries the legs a plain run leaves out, and the
    CPU leg's parity sample covers the four tracks."""
    d = _bench("--gpus", "1", "--steps", "1", "--warmup", "0", "--tracks", "4", "--seconds", "20", "--full",
               "--cpu-1thread-tracks", "1")
    assert all(k in d for k in HEADLINE) and d["full"] is True and d["errors"] == 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["value_1thread"] > 0
    p = d["parity_sample"]
    assert p["checked"] == 4 and p["within_tolerance"] == 4 and p["key_equal"] == 4
    iso = d["roofline"]["isolated"]
    assert iso["ms_per_launch"] > 0 and iso["achieved"] > 0
    assert d["sine_30s"]["gpu_ms"] > 0 and d["sine_30s"]["cpu_port_1thread_ms"] > 0


@pytest.mark.gpu
def test_plain_run_and_dump_on_gpu(tmp_path):
    """Four 20-s tracks through a plain run: the line has none of the --full legs, and the dumped
    arrays are the results a caller of the same device batch receives (seeds 0..3), bit for bit."""
    import sdsp

    n, L = 4, 44100 * 20
    d = _bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--tracks", str(n), "--seconds", "20",
               "--dump-outputs", str(tmp_path / "o"))
    assert all(k in d for k in HEADLINE) and d["full"] is False and d["errors"] == 0
    assert d["cpu_baseline"] is None and d["parity_sample"] is None
    assert "isolated" not in d["roofline"] and "sine_30s" not in d and "sclk_mhz_timed" not in d
    a = _load(str(tmp_path / "o"))
    assert all(v.dtype == (np.float64 if k in ("flags", "methods_used") else np.float32) for k, v in a.items())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["sample_rate"].tolist() == [44100.0] * n
    buf = sdsp.DeviceBuffer(n * L)
    sdsp.generate_synthetic(buf.ptr, n, L, seed0=0)
    res = sdsp.analyze_batch_device(buf.ptr, np.arange(n) * L, np.full(n, L))
    f32 = np.float32
    assert a["status"].tolist() == [0.0] * n
    for k in ("bpm", "bpm_confidence", "key_confidence", "key_clarity", "grid_stability"):
        assert a[k].tobytes() == np.array([r[k] for r in res], f32).tobytes(), k
    assert a["key_mode"].tolist() == [float("Minor" in r["key"]) for r in res]
    assert a["key_tonic"].tolist() == [float(list(r["key"].values())[0]) for r in res]
    for k in ("beats", "downbeats", "bars"):
        assert a["n_" + k].tolist() == [float(len(r["beat_grid"][k])) for r in res], k
        assert a[k].tobytes() == np.array([t for r in res for t in r["beat_grid"][k]], f32).tobytes(), k
    assert a["n_beats"].sum() > 0
