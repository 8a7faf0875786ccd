"""stratum-dsp_amd/csrc/sections_core.hpp on the CPU.  The header is compiled into libstratum_hip.so,
host and device; here a host harness (tests/cpp/sections_core_test.cpp), built stand-alone with the
address and undefined-behaviour sanitizers and contraction off, runs the small shapes of
tests/sections_cases.py through the same functions the kernels and the host call (cell plan, cell
means, staged rows, novelty, boundary rule, section assembly, snap) and prints the bits, which must
equal tests/sections_ref.py's; it also runs the request checks and the public structs' layout
against the ctypes mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sdsp_abi
import sections_cases as SC
import sections_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sections") / "sections_core_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "sections_core_test.cpp")])
    return str(exe)


def _run(harness, *args):
    out = subprocess.run([harness, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-4000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert "FAIL" not in out.stdout, out.stdout[-4000:]
    return out.stdout


def test_sections_core_self_checks(harness):
    assert _run(harness).startswith("ok sections_core")


def test_struct_layout_matches_ctypes(harness):
    rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in _run(harness, "layout").splitlines()}
    A = sdsp_abi
    for name, T in (("sdsp_sections_request", A.SdspSectionsRequest), ("sdsp_section", A.SdspSection),
                    ("sdsp_sections", A.SdspSections)):
        assert rows[name] == [C.sizeof(T)] + [getattr(T, k).offset for k, _ in T._fields_], name
    Q = A.SdspRequestSetExt
    assert rows["sdsp_request_set_ext"] == [C.sizeof(Q), Q.base.offset, Q.sc_req.offset, Q.sections.offset]
    assert Q.base.offset == 0 and Q.sc_req.offset == C.sizeof(A.SdspRequestSet)  # the pair lies at the plain set's end
    assert [k for k, _ in Q._fields_][-2:] == ["sc_req", "sections"]  # a new pair goes at the end


def _write(path, items):
    """items: (khop, hop, Cs, K, G, w, min_strength, snap, sr, rows, E, downs)."""
    with open(path, "wb") as f:
        f.write(np.array([len(items)], np.uint64).tobytes())
        for khop, hop, Cs, K, G, w, ms, snap, sr, rows, E, downs in items:
            f.write(np.array([khop, hop, Cs, K, G], np.uint64).tobytes())
            f.write(np.array([w, ms, snap], f32).tobytes())
            f.write(np.array([sr], np.uint32).tobytes())
            for a, per in ((rows, 12), (E, 1), (downs, 1)):
                a = np.ascontiguousarray(a, f32).ravel()
                f.write(np.array([a.size // per], np.uint64).tobytes())
                f.write(a.tobytes())


def _parse(text):
    out, lines, at = [], text.splitlines(), 0
    while at < len(lines):
        w = lines[at].split()
        assert w[0] == "T"
        n = int(w[1])
        cells = np.array([[int(v, 16) for v in ln.split()[1:15]] + [int(ln.split()[15])] for ln in lines[at + 1:at + 1 + n]],
                         np.int64).reshape(n, 15)
        at += 1 + n
        ns = int(lines[at].split()[1])
        secs = [ln.split() for ln in lines[at + 1:at + 1 + ns]]
        at += 1 + ns
        out.append(dict(n=n, gmax=int(w[2], 16), nmax=int(w[3], 16), cells=cells, secs=secs))
    return out


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32).astype(np.int64)


@pytest.mark.parametrize("layout", sorted(SC.LAYOUTS))
@pytest.mark.parametrize("K", SC.KS)
def test_small_shapes_match_reference(harness, tmp_path, layout, K):
    khop, hop, Cs = SC.LAYOUTS[layout]
    tr, ref = SC.tracks(layout, K), SC.reference(layout, K)
    rng = np.random.default_rng(5)
    items, want = [], []
    for G in SC.GS:
        bnd = SC.boundaries(layout, K, G)
        for t, (rows, E, tag) in enumerate(tr):
            span = ref[t]["n_cells"] * Cs / SC.SR
            downs = np.sort(rng.random(7, dtype=f32) * f32(span)).astype(f32)
            items.append((khop, hop, Cs, K, G, SC.WEIGHT, SC.MIN_STRENGTH, 0.3, SC.SR, rows, E, downs))
            want.append((ref[t], bnd[t], downs, tag, G))
    path = tmp_path / "tracks.bin"
    _write(path, items)
    got = _parse(_run(harness, "tracks", str(path)))
    assert len(got) == len(want)
    peaks = 0
    for g, (c, b, downs, tag, G) in zip(got, want):
        what = (layout, K, G, tag)
        assert g["n"] == c["n_cells"], what
        assert g["gmax"] == int(_bits(c["gmax"])[0]) and g["nmax"] == int(_bits(c["nmax"])[0]), what
        if g["n"]:
            assert np.array_equal(g["cells"][:, :12], _bits(c["m"]).reshape(-1, 12)), what
            assert np.array_equal(g["cells"][:, 12], _bits(c["g"])), what
            assert np.array_equal(g["cells"][:, 13], _bits(c["novelty"])), what
            assert np.array_equal(g["cells"][:, 14], b.astype(np.int64)), what
        sec = S.assemble(c["g"], c["novelty"], b, Cs, SC.SR, downs, 0.3)
        assert len(g["secs"]) == sec["start_cell"].size == (int(b.sum()) + 1 if g["n"] else 0), what
        for i, w in enumerate(g["secs"]):
            row = [int(w[0]), int(w[1])] + [int(v, 16) for v in w[2:8]] + [int(w[8])]
            exp = [int(sec["start_cell"][i]), int(sec["end_cell"][i])] + \
                [int(_bits(sec[k][i:i + 1])[0]) for k in S.SECTION_FIELDS[2:8]] + [int(sec["downbeat"][i])]
            assert row == exp, (what, i, row, exp)
        peaks += int(b.sum())
        if tag == "plateau" and K == 1:
            assert np.flatnonzero(b).tolist() == ([1] if G else list(range(1, 40))), what
        if tag == "zero_energy":
            assert c["gmax"] == 0 and not c["e"].any()
    assert peaks > 0
