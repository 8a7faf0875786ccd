"""stratum-dsp_amd/csrc/fingerprint_core.hpp on the CPU.  The header is compiled into
libstratum_hip.so, host and device; here a host harness (tests/cpp/fingerprint_core_test.cpp), built
stand-alone with the address and undefined-behaviour sanitizers and contraction off, runs the small
shapes of tests/fingerprint_cases.py through the same functions the kernels and the host call (cell
plan and fold, the word, n(o) and e(o), the best-offset rule, the match rule, list assembly) and prints
words and pair records, which must equal tests/fingerprint_ref.py's; it also runs the request checks
and the public structs' layout against the ctypes mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fingerprint_cases as FC
import fingerprint_ref as R
import sdsp_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fingerprint") / "fingerprint_core_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "fingerprint_core_test.cpp")])
    return str(exe)


def _run(harness, *args):
    out = subprocess.run([harness, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-4000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert "FAIL" not in out.stdout, out.stdout[-4000:]
    return out.stdout


def test_fingerprint_core_self_checks(harness):
    assert _run(harness).startswith("ok fingerprint_core")


def test_struct_layout_matches_ctypes(harness):
    rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in _run(harness, "layout").splitlines()}
    A = sdsp_abi
    for name, T in (("sdsp_fingerprint_request", A.SdspFingerprintRequest), ("sdsp_fingerprint", A.SdspFingerprint),
                    ("sdsp_fingerprint_match", A.SdspFingerprintMatch), ("sdsp_fingerprint_matches", A.SdspFingerprintMatches),
                    ("sdsp_request_set_ext3", A.SdspRequestSetExt3)):
        assert rows[name] == [C.sizeof(T)] + [getattr(T, k).offset for k, _ in T._fields_], name
    Q = A.SdspRequestSetExt3
    assert Q.base.offset == 0 and Q.fp_req.offset == C.sizeof(A.SdspRequestSetExt2)  # the fields lie at ext2's end
    assert C.sizeof(A.SdspDebugFingerprintPair) == 16


@pytest.mark.parametrize("layout", sorted(FC.LAYOUTS))
def test_words_of_small_shapes_match_reference(harness, tmp_path, layout):
    khop, Cs = FC.LAYOUTS[layout]
    tr, ref = FC.word_tracks(layout), FC.word_reference(layout)
    path = tmp_path / "words.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(tr)], np.uint64).tobytes())
        for rows, _ in tr:
            f.write(np.array([khop, Cs, rows.shape[0]], np.uint64).tobytes())
            f.write(np.ascontiguousarray(rows, f32).tobytes())
    lines, at = _run(harness, "words", str(path)).splitlines(), 0
    zero_words = 0
    for (rows, tag), (m, w) in zip(tr, ref):
        head = lines[at].split()
        assert head[0] == "T" and int(head[1]) == m.shape[0] and int(head[2]) == w.size, (layout, tag, head)
        n = m.shape[0]
        got_m = np.array([[int(v, 16) for v in ln.split()[1:]] for ln in lines[at + 1:at + 1 + n]], np.int64).reshape(n, 12)
        assert np.array_equal(got_m, m.view(np.uint32).astype(np.int64)), (layout, tag)
        got_w = np.array([int(v, 16) for v in lines[at + 1 + n].split()[1:]], np.int64)
        assert np.array_equal(got_w, w.astype(np.int64)), (layout, tag)
        at += n + 2
        if tag in ("zero_rows", "constant_rows"):
            assert w.size == 18 and not w.any(), tag
        zero_words += int((w == 0).sum())
    assert at == len(lines) and zero_words >= 36
    assert [r[1].size for r in ref[:len(FC.CELL_COUNTS)]] == [max(n - 2, 0) for n in FC.CELL_COUNTS]


def test_pair_records_and_lists_of_small_shapes_match_reference(harness, tmp_path):
    calls = FC.match_calls()
    items = [(name, O, mo) for name in sorted(calls) for O, mo in calls[name][1]]
    Cs, max_ber = 5512, 0.35
    path = tmp_path / "match.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(items)], np.uint64).tobytes())
        for name, O, mo in items:
            ws = calls[name][0]
            f.write(np.array([len(ws), O, mo, Cs], np.uint64).tobytes())
            f.write(np.array([max_ber], f32).tobytes())
            for t, w in enumerate(ws):
                f.write(np.array([1000 * t + 7, w.size], np.uint64).tobytes())
                f.write(np.ascontiguousarray(w, np.uint32).tobytes())
    lines, at = _run(harness, "match", str(path)).splitlines(), 0
    eligible = matches = 0
    for name, O, mo in items:
        ws = calls[name][0]
        T = len(ws)
        ref = FC.match_reference(name, O, mo)
        assert lines[at].split() == ["P", str(T)]
        at += 1
        for a in range(T):
            for b in range(a + 1, T):
                got = [int(v) for v in lines[at].split()]
                want = [a, b] + [int(ref[k][a, b]) for k in ("eligible", "offset_words", "bit_errors", "positions")]
                assert got == want, (name, O, mo, got, want)
                eligible += got[2]
                at += 1
        ml, _ = R.match_list(ws, [0] * T, [1000 * t + 7 for t in range(T)], Cs,
                             dict(max_offset_words=O, min_overlap_words=mo, max_ber=max_ber), rec=ref)
        assert lines[at].split() == ["M", str(ml["n_matches"])], (name, O, mo, lines[at])
        at += 1
        for i in range(ml["n_matches"]):
            w = lines[at].split()
            got = [int(v) for v in w[:6]] + [int(w[6], 16)]
            want = [int(ml["matches"][k][i]) for k in R.MATCH_FIELDS[:6]] + [int(ml["matches"]["ber"][i:i + 1].view(np.uint32)[0])]
            assert got == want, (name, O, mo, i, got, want)
            at += 1
        matches += ml["n_matches"]
    assert at == len(lines) and eligible > 50 and matches > 5
