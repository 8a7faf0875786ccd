"""stratum-dsp_amd/csrc/tempo_map_core.hpp on the CPU.  The header is compiled into libstratum_hip.so,
host and device; here a host harness (tests/cpp/tempo_map_core_test.cpp), built stand-alone with the
address and undefined-behaviour sanitizers and contraction off, replays detect_tempo_variations with
the kernel's window function over the HMM beats of every case of tests/beat_cases.py and prints the
bits, which must equal tests/tempo_map_ref.py's segments (themselves the oracle's); it also runs the
tracker's confidence and the signature pick on the values that reference pins, the request
validation, the segment-capacity bound over a sweep of spans and tempi, and the public structs'
layout against the ctypes mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import beat_cases as B
import sdsp_abi
import tempo_map_ref as R
import units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(B.cases())


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tempo_map") / "tempo_map_core_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "tempo_map_core_test.cpp")])
    return str(exe)


@pytest.fixture(scope="module")
def refs():
    out = {}
    for name in NAMES:
        t = B.cases()[name][0]
        out[name] = R.reference(t["onsets"], t["bpm"], t["conf"], B.SR)
    return out


def _run(harness, *args):
    out = subprocess.run([harness, *args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-4000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert "FAIL" not in out.stdout, out.stdout[-4000:]
    return out.stdout


def test_tempo_map_core_self_checks(harness):
    assert _run(harness).startswith("ok tempo_map_core")


def test_struct_layout_matches_ctypes(harness):
    rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in _run(harness, "layout").splitlines()}
    A = sdsp_abi
    assert rows["sdsp_tempo_map_request"] == [C.sizeof(A.SdspTempoMapRequest)]
    S = A.SdspTempoSegment
    assert rows["sdsp_tempo_segment"] == [C.sizeof(S)] + [getattr(S, k).offset for k, _ in S._fields_]
    M = A.SdspTempoMap
    assert rows["sdsp_tempo_map"] == [C.sizeof(M)] + [getattr(M, k).offset for k, _ in M._fields_]
    Q = A.SdspRequestSet
    assert rows["sdsp_request_set"] == [C.sizeof(Q), Q.tm_req.offset, Q.tempo_maps.offset]
    assert [k for k, _ in Q._fields_][-2:] == ["tm_req", "tempo_maps"]  # a new pair goes at the end


def test_windows_match_reference(harness, refs, tmp_path):
    grids = [k for k in NAMES if refs[k]["has_grid"]]
    assert len(grids) >= 30
    path = tmp_path / "windows.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(grids)], np.uint64).tobytes())
        for k in grids:
            f.write(np.array([refs[k]["nominal_bpm"]], np.float32).tobytes())
            f.write(np.array([refs[k]["hmm"].size], np.uint64).tobytes())
            f.write(refs[k]["hmm"].astype(np.float32).tobytes())
    lines = _run(harness, "windows", str(path)).splitlines()
    at, seen = 0, set()
    for k in grids:
        s = refs[k]["segments"]
        assert lines[at] == "T %d" % refs[k]["n_segments"], k
        for i in range(refs[k]["n_segments"]):
            w = lines[at + 1 + i].split()
            got = [int(v, 16) for v in w[:4]] + [int(w[4])]
            want = [R.bits1(s[f][i]) for f in ("start_time", "end_time", "bpm", "confidence")] + [int(s["is_variable"][i])]
            assert got == want, (k, i, got, want)
            seen.add((int(s["is_variable"][i]), float(s["confidence"][i]) in (0.0, 1.0)))
        at += 1 + refs[k]["n_segments"]
    assert at == len(lines)
    assert {(1, True), (1, False), (0, False), (0, True)} <= seen  # both clamps of the confidence, and between


def test_updates_and_signatures_match_reference(harness, refs, tmp_path):
    """The tracker's confidence from the oracle's own likelihood of the winning candidate, and the
    signature pick from the reference's scores."""
    triples, want_conf, scores, want_pick = [], [], [], []
    for k in NAMES:
        m, t = refs[k], B.cases()[k][0]
        if not m["has_grid"]:
            continue
        on = B.onsets_s(t)
        s, carried = m["segments"], float(m["nominal_bpm"])
        for i in np.flatnonzero(s["updated"]):
            so = on[(on >= s["start_time"][i]) & (on <= s["end_time"][i])]
            assert so.size == s["n_onsets"][i]
            cands = units.BayesianBeatTracker(carried, 0.8).generate_bpm_candidates()
            ub = float(s["updated_bpm"][i])
            lik = units.BayesianBeatTracker(carried, 0.8).compute_likelihood(so, ub) if cands else 0.0
            if not cands:
                assert ub == carried
            triples.append((lik, carried, ub))
            want_conf.append(R.bits1(s["updated_confidence"][i]))
            carried = ub
        if m["time_signature_scored"]:
            scores.append(m["time_signature_scores"])
            want_pick.append((m["beats_per_bar"], R.bits1(m["time_signature_confidence"])))
    assert len(triples) > 300 and len(scores) >= 30

    def run(mode, rows):
        path = tmp_path / (mode + ".bin")
        with open(path, "wb") as f:
            f.write(np.array([len(rows)], np.uint64).tobytes())
            f.write(np.array(rows, np.float32).tobytes())
        return _run(harness, mode, str(path)).splitlines()

    got = [int(ln, 16) for ln in run("update", triples)]
    assert got == want_conf, [(i, triples[i]) for i in range(len(got)) if got[i] != want_conf[i]][:5]
    got = [(int(ln.split()[0]), int(ln.split()[1], 16)) for ln in run("pick", scores)]
    assert got == want_pick
