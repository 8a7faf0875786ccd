"""stratum-dsp_amd/csrc/r128_core.hpp on the CPU.  The header is compiled into libstratum_hip.so, host
and device; here a host harness (tests/cpp/r128_core_test.cpp), built stand-alone with the address and
undefined-behaviour sanitizers and contraction off, runs the small shapes of tests/r128_cases.py
through the same functions the kernels and the host call (coefficients, filter step, block folds,
gates, rank-counting order statistics, peaks, finishing logs) and prints the bits, which must equal
tests/r128_ref.py's; it also runs the request checks, the reading of all three generations of the
request set, and the public structs' layout against the ctypes mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import r128_cases as RC
import r128_ref as R
import sdsp_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("r128") / "r128_core_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "r128_core_test.cpp")])
    return str(exe)


def _run(harness, *args):
    out = subprocess.run([harness, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-4000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert "FAIL" not in out.stdout, out.stdout[-4000:]
    return out.stdout


def test_r128_core_self_checks(harness):
    assert _run(harness).startswith("ok r128_core")


def test_struct_layout_matches_ctypes(harness):
    rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in _run(harness, "layout").splitlines()}
    A = sdsp_abi
    for name, T in (("sdsp_r128_request", A.SdspR128Request), ("sdsp_r128", A.SdspR128)):
        assert rows[name] == [C.sizeof(T)] + [getattr(T, k).offset for k, _ in T._fields_], name
    Q = A.SdspRequestSetExt2
    assert rows["sdsp_request_set_ext2"] == [C.sizeof(Q), Q.base.offset, Q.r128_req.offset, Q.r128.offset]
    assert rows["older"] == [C.sizeof(A.SdspRequestSet), C.sizeof(A.SdspRequestSetExt)]
    assert Q.base.offset == 0 and Q.r128_req.offset == C.sizeof(A.SdspRequestSetExt)  # the pair lies at the older struct's end
    assert [k for k, _ in A.SdspRequestSetExt._fields_][-2:] == ["sc_req", "sections"]  # which keeps its own last pair


def _write(path, sr, what, tracks):
    with open(path, "wb") as f:
        f.write(np.array([sr, what], np.uint32).tobytes())
        f.write(np.array([len(tracks)], np.uint64).tobytes())
        for x in tracks:
            f.write(np.array([len(x)], np.uint64).tobytes())
            f.write(np.ascontiguousarray(x, f32).tobytes())


def _parse(text):
    out, lines = [], text.splitlines()
    assert len(lines) % 6 == 0

    def floats(ln, tag):
        w = ln.split()
        assert w[0] == tag and int(w[1]) == len(w) - 2
        return np.array([int(v, 16) for v in w[2:]], np.uint32).view(f32)

    for at in range(0, len(lines), 6):
        w = lines[at].split()
        assert w[0] == "T"
        r = dict(zip(R.INTS, (int(v) for v in w[1:])))
        r.update(zip(R.FLOATS, floats(lines[at + 1], "F")))
        r.update(shelf=floats(lines[at + 2], "C"), highpass=floats(lines[at + 3], "H"),
                 momentary=floats(lines[at + 4], "M"), short_term=floats(lines[at + 5], "S"))
        out.append(r)
    return out


@pytest.mark.parametrize("name,what", [("small", RC.ALL), ("small", R.LOUDNESS), ("small", R.TRUE_PEAK), ("odd", RC.ALL)])
def test_small_shapes_match_reference(harness, tmp_path, name, what):
    sr, xs, tags, ref = RC.case(name)
    if name == "small":
        from test_r128_ref import assert_gates_exercised
        assert_gates_exercised(ref[tags.index("two_level")])
        assert ref[tags.index("under_abs_gate")]["has_integrated"] == 0 and ref[tags.index("zero")]["sample_peak"] == 0
    path = tmp_path / "tracks.bin"
    _write(path, sr, what, xs)
    got = _parse(_run(harness, "tracks", str(path)))
    assert len(got) == len(xs)
    for g, r, tag in zip(got, ref, tags):
        RC.assert_equal(g, RC.masked(r, what), (name, what, tag))
