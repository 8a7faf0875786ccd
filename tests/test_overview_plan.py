"""The overview envelope's column plan (stratum-dsp_amd/csrc/overview_plan.hpp) on the CPU.  The
same header is compiled into libstratum_hip.so, host and device; here a host harness
(tests/cpp/overview_plan_test.cpp), built stand-alone with the address and undefined-behaviour
sanitizers, checks it against the formulas of include/stratum_hip.h for F in {0, 1, 2, 63, 64, 65,
257, 15500}, columns in {1, 2, F - 1, F, F + 1, 1024} and frames_per_column in {1, 3, 64, F,
F + 1}: the columns partition [0, F) in order, none is empty, the sample ranges partition [0, n);
the band bins at 0, exactly on a bin, at Nyquist and above it; which requests are refused."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ovplan") / "overview_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "overview_plan_test.cpp")])
    return str(exe)


def test_overview_plan(harness):
    out = subprocess.run([harness], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-4000:], out.stderr[-4000:])
    assert out.stdout.startswith("ok overview_plan"), out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]


def test_python_plan_agrees_with_header_formulas():
    """tests/overview_ref.py's column starts (the GPU tests' reference) have the same properties."""
    import overview_ref

    for F in (0, 1, 2, 63, 64, 65, 257, 15500):
        for kw in ([{"columns": c} for c in (1, 2, F - 1, F, F + 1, 1024) if c >= 1] +
                   [{"frames_per_column": k} for k in (1, 3, 64, F, F + 1) if k >= 1]):
            f0 = overview_ref.column_starts(F, **kw)
            assert f0[0] == 0 and f0[-1] == F and all(a < b for a, b in zip(f0, f0[1:])), (F, kw)
            C = len(f0) - 1
            assert C == (min(kw["columns"], F) if "columns" in kw else -(-F // kw["frames_per_column"])), (F, kw)
    assert overview_ref.band_bins(250.0, 4000.0, 2048, 44100) == (11, 185)
    assert overview_ref.band_bins(0.0, 22050.0, 2048, 44100) == (0, 1024)
    assert overview_ref.band_bins(21.533203125, 30000.0, 2048, 44100) == (1, 1025)
