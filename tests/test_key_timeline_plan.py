"""The key timeline's segment plan (stratum-dsp_amd/csrc/key_timeline_plan.hpp) on the CPU.  The
same header is compiled into libstratum_hip.so, host and device; here a host harness
(tests/cpp/key_timeline_plan_test.cpp), built stand-alone with the address and undefined-behaviour
sanitizers, checks it against the formulas of include/stratum_hip.h: L, H and S for F in {0, 1, 2,
63, 64, 65, 689, 15500} and (L, H) in {(1, 1), (2, 1), (64, 64), (65, 3), (F, F), (F + 1, 1)}, seconds
that land exactly on and just below an integer frame count at 44100 / 512 and 48000 / 512, that the
segments stay inside [0, F), which requests are refused, the primary key and the changes; and that
tests/key_timeline_ref.py (the GPU tests' reference) plans the same."""
import os
import subprocess

import numpy as np
import pytest

import key_timeline_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ktplan") / "key_timeline_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "key_timeline_plan_test.cpp")])
    return str(exe)


def test_key_timeline_plan(harness):
    out = subprocess.run([harness], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-4000:], out.stderr[-4000:])
    assert out.stdout.startswith("ok key_timeline_plan"), out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]


REQUESTS = [
    (44100, 512, dict(segment_seconds=8.0, overlap_seconds=2.0)),
    (44100, 512, dict(segment_seconds=4.0, overlap_seconds=1.0)),
    (44100, 512, dict(segment_seconds=512.0)),
    (44100, 512, dict(segment_seconds=float(np.nextafter(np.float32(512.0), np.float32(0))))),
    (48000, 512, dict(segment_seconds=16.0, overlap_seconds=8.0)),
    (48000, 512, dict(segment_seconds=float(np.nextafter(np.float32(16.0), np.float32(0))), overlap_seconds=8.0)),
    (48000, 512, dict(segment_seconds=0.32)),
    (44100, 1024, dict(segment_seconds=3.3, overlap_seconds=0.7)),
    (22050, 441, dict(segment_seconds=1.0, overlap_seconds=0.99)),
    (44100, 512, dict(segment_frames=65, hop_frames=3)),
    (44100, 512, dict(segment_frames=2 ** 31 - 1, hop_frames=1)),
    (44100, 512, dict()),
    (44100, 512, dict(segment_seconds=8.0, segment_frames=3, hop_frames=1)),
    (44100, 512, dict(segment_seconds=float("inf"))),
    (44100, 512, dict(segment_seconds=-1.0)),
    (44100, 512, dict(segment_seconds=1.0, overlap_seconds=1.0)),
    (44100, 512, dict(segment_seconds=0.01)),
    (44100, 512, dict(segment_frames=4)),
    (44100, 512, dict(hop_frames=4)),
    (44100, 512, dict(segment_frames=2 ** 31, hop_frames=1)),
    (44100, 512, dict(segment_seconds=3e7)),
    (44100, 512, dict(segment_seconds=8.0, min_change_confidence=float("nan"))),
]


@pytest.mark.parametrize("sr,khop,req", REQUESTS)
def test_python_plan_agrees_with_the_header(harness, sr, khop, req):
    args = [repr(float(np.float32(req.get(k, 0.0)))) for k in ("segment_seconds", "overlap_seconds")]
    args += [str(req.get(k, 0)) for k in ("segment_frames", "hop_frames")] + [repr(float(req.get("min_change_confidence", -1.0)))]
    out = subprocess.run([harness, "plan", str(sr), str(khop)] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "runtime error" not in out.stderr, (out.stdout, out.stderr[-2000:])
    want = K.plan(req, sr, khop)
    if isinstance(want, str):
        assert out.stdout.startswith("refused ") and want in out.stdout, (want, out.stdout)
    else:
        assert out.stdout.split() == ["plan", str(want[0]), str(want[1])], (want, out.stdout)


def test_python_segments_stay_inside_the_track():
    for F in (0, 1, 2, 63, 64, 65, 689, 15500):
        for L, H in ((1, 1), (2, 1), (64, 64), (65, 3), (F, F), (F + 1, 1)):
            if L == 0:
                continue
            S = K.n_segments(F, L, H)
            assert S == sum(1 for s in range(F + 1) if s * H + L <= F), (F, L, H)
            assert S == 0 or (S - 1) * H + L <= F < S * H + L
