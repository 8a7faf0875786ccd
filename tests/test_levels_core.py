"""stratum-dsp_amd/csrc/levels_core.hpp on the CPU.  The header is compiled into libstratum_hip.so,
host and device; here a host harness (tests/cpp/levels_core_test.cpp), built stand-alone with the
address and undefined-behaviour sanitizers and contraction off, runs its fold steps and finishing
code on the vectors tests/test_levels_ref.py pins to the oracle and prints the bits, which must equal
tests/levels_ref.py's; it also checks the request validation, the keep-rule, the silence map's
capacity bound, and the public structs' layout against the ctypes mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import levels_ref
import sdsp_abi
from test_levels_ref import AMPS, LENGTHS, MAP_CASES, SR, _noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("levels") / "levels_core_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "levels_core_test.cpp")])
    return str(exe)


def _run(harness, *args):
    out = subprocess.run([harness, *args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-4000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    return out.stdout


def test_levels_core_self_checks(harness):
    assert _run(harness).startswith("ok levels_core")


def test_struct_layout_matches_ctypes(harness):
    rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in _run(harness, "layout").splitlines()}
    A = sdsp_abi
    assert rows["sdsp_levels_request"] == [C.sizeof(A.SdspLevelsRequest)]
    L = A.SdspLoudness
    assert rows["sdsp_loudness"] == [C.sizeof(L), L.measured.offset, L.has_lufs.offset, L.measured_lufs.offset, L.gain.offset]
    R = A.SdspSilenceRegion
    assert rows["sdsp_silence_region"] == [C.sizeof(R), R.duration_seconds.offset]
    V = A.SdspLevels
    assert rows["sdsp_levels"] == [C.sizeof(V), V.applied_gain.offset, V.n_samples.offset, V.frame_size.offset,
                                   V.n_regions.offset, V.regions.offset, V.status.offset]
    S = A.SdspRequestSet
    assert rows["sdsp_request_set"] == [C.sizeof(S), S.ov_req.offset, S.kt_req.offset, S.lv_req.offset, S.levels.offset]


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def test_folds_and_finish_match_reference(harness, tmp_path):
    lengths = sorted(set(LENGTHS[levels_ref.PEAK]) | set(LENGTHS[levels_ref.LOUDNESS]))
    tracks = [_noise(n, amp, 100 * k + j) for k, n in enumerate(lengths) for j, amp in enumerate(AMPS)]
    P = levels_ref.params(SR)
    path = tmp_path / "fold.bin"
    with open(path, "wb") as f:
        f.write(np.array([P["target_peak"], P["target_rms"], P["target_lufs"], P["gate"], *P["coef"]], np.float32).tobytes())
        f.write(np.array([P["block"]], np.int64).tobytes())
        f.write(np.array([len(tracks)], np.uint64).tobytes())
        for x in tracks:
            f.write(np.array([len(x)], np.uint64).tobytes())
            f.write(x.tobytes())
    want = levels_ref.loudness(tracks, SR)
    lines = _run(harness, "fold", str(path)).splitlines()
    assert len(lines) == 3 * len(tracks)
    seen = set()
    for ln in lines:
        w = ln.split()
        t, m = int(w[0]), int(w[1])
        ref = want[t][m]
        got = [int(w[2]), int(w[3]), int(w[4])] + [int(v, 16) for v in w[5:10]]
        exp = [ref["status"], ref["measured"], ref["has_lufs"]] + [_bits(ref[k]) for k in
                                                                    ("measured_lufs", "peak_db", "rms_db", "gain_db", "gain")]
        assert got == exp, (t, m, len(tracks[t]), got, exp)
        seen.add((m, ref["has_lufs"], bool(np.isinf(ref["peak_db"]))))
    assert {(2, 1, False), (2, 0, False), (2, 0, True)} <= seen  # Loudness: measured, all gated, silent


def test_silence_map_matches_reference(harness, tmp_path):
    names = sorted(MAP_CASES)
    path = tmp_path / "map.bin"
    thr = levels_ref._pow10(np.float32(-40.0) / np.float32(20.0))
    with open(path, "wb") as f:
        f.write(np.array([thr], np.float32).tobytes())
        f.write(np.array([levels_ref.min_frames(SR, 2048), 1024, len(names)], np.uint64).tobytes())
        for name in names:
            r = levels_ref.frame_rms(MAP_CASES[name], 2048)
            f.write(np.array([len(MAP_CASES[name]), len(r)], np.uint64).tobytes())
            f.write(r.tobytes())
    lines = _run(harness, "map", str(path)).splitlines()
    assert len(lines) == len(names)
    for name, ln in zip(names, lines):
        w = [int(v) for v in ln.split()]
        got = [(w[2 + 2 * i], w[3 + 2 * i]) for i in range(w[1])]
        assert got == levels_ref.silence_map(MAP_CASES[name], SR)[0], name
