"""The key timeline entries at the drop-in boundary, without a GPU (CPU only).

* sdsp_abi's mirrors of sdsp_key_timeline_request, sdsp_key_segment, sdsp_key_change and
  sdsp_key_timeline have exactly the C layout (every field's offset against a compiled C11 probe of
  the headers, as test_abi.py does for the existing structs);
* every refused request fails the call with the stated status and its reason before any device is
  touched: on a machine without a GPU the answer is the request's error, not the device's;
* a good request without a GPU fails with "Processing error: no HIP device"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sdsp
import sdsp_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stratum_hip_debug.h")  # includes stratum_hip.h

STRUCTS = {"sdsp_key_timeline_request": sdsp_abi.SdspKeyTimelineRequest, "sdsp_key_segment": sdsp_abi.SdspKeySegment,
           "sdsp_key_change": sdsp_abi.SdspKeyChange, "sdsp_key_timeline": sdsp_abi.SdspKeyTimeline}


def test_key_timeline_struct_layouts_match_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-o", str(exe), str(src)])
    c = {}
    for ln in subprocess.check_output([str(exe)]).decode().split("\n"):
        if ln:
            k, v = ln.rsplit(" ", 1)
            c[k] = int(v)
    for cname, py in STRUCTS.items():
        assert c[f"{cname} size"] == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert c[f"{cname}.{f}"] == getattr(py, f).offset, f"{cname}.{f}"
    # the header's field lists, name by name
    src = open(os.path.join(ROOT, "include", "stratum_hip.h")).read()
    for cname, py in STRUCTS.items():
        body = src[src.index("typedef struct %s {" % cname):src.index("} %s;" % cname)]
        for f, _ in py._fields_:
            assert f in body, (cname, f)
    assert C.sizeof(sdsp_abi.SdspKeyTimelineRequest) == 20 and C.sizeof(sdsp_abi.SdspKeySegment) == 48
    assert np.dtype(sdsp_abi.SdspKeySegment).itemsize == 48 and np.dtype(sdsp_abi.SdspKeyChange).itemsize == 24


def test_entries_exported():
    L = sdsp.lib()
    for name in ("sdsp_analyze_batch_device_requests", "sdsp_key_timeline_free", "sdsp_debug_key_timeline",
                 "sdsp_analyze_batch_device_overview"):
        assert hasattr(L, name), name


INVALID, NOT_IMPLEMENTED = 1, 4
BAD = [
    (dict(), {}, sdsp.STAGES_FULL, "neither"),
    (dict(segment_seconds=8.0, segment_frames=64, hop_frames=1), {}, sdsp.STAGES_FULL, "both"),
    (dict(overlap_seconds=1.0, hop_frames=1), {}, sdsp.STAGES_FULL, "both"),
    (dict(segment_seconds=float("inf")), {}, sdsp.STAGES_FULL, "not finite"),
    (dict(segment_seconds=8.0, overlap_seconds=float("nan")), {}, sdsp.STAGES_FULL, "not finite"),
    (dict(segment_seconds=-8.0), {}, sdsp.STAGES_FULL, "negative"),
    (dict(segment_seconds=8.0, overlap_seconds=-0.5), {}, sdsp.STAGES_FULL, "negative"),
    (dict(segment_seconds=8.0, min_change_confidence=float("nan")), {}, sdsp.STAGES_FULL, "NaN"),
    (dict(segment_seconds=0.01), {}, sdsp.STAGES_FULL, "L == 0"),
    (dict(segment_seconds=8.0, overlap_seconds=8.0), {}, sdsp.STAGES_FULL, "O >= L"),
    (dict(segment_frames=8), {}, sdsp.STAGES_FULL, "H == 0"),
    (dict(hop_frames=8), {}, sdsp.STAGES_FULL, "L == 0"),
    (dict(segment_frames=2 ** 31, hop_frames=1), {}, sdsp.STAGES_FULL, "2^31"),
    (dict(segment_frames=8, hop_frames=2 ** 31), {}, sdsp.STAGES_FULL, "2^31"),
    (dict(segment_seconds=3e7), {}, sdsp.STAGES_FULL, "2^31"),
    # the seconds form goes through the key STFT's hop: 0.2 s is 17 frames at hop 512, none at hop 16384
    (dict(segment_seconds=0.2), dict(key_stft_hop_size=16384), sdsp.STAGES_FULL, "L == 0"),
    (dict(segment_seconds=8.0, overlap_seconds=2.0), {}, sdsp.STAGES_BPM_ONLY, "SDSP_STAGES_BPM_ONLY"),
]


@pytest.mark.parametrize("kw,opts,stages,why", BAD)
def test_bad_request_is_refused_before_the_device(kw, opts, stages, why):
    """A null device pointer and device 9999: had the call gone as far as a device, the error would
    be the device's (and on a machine without a GPU, "no HIP device")."""
    cfg = sdsp.default_config()
    for k, v in opts.items():
        setattr(cfg, k, v)
    with pytest.raises(sdsp.AnalysisError) as e:
        sdsp.analyze_batch_device_requests(0, [0, 100], [100, 50], config=cfg, device=9999, stages=stages,
                                           key_timeline=sdsp.key_timeline_request(**kw))
    assert e.value.code == INVALID and e.value.kind == "InvalidInput"
    assert "Invalid input: key timeline" in str(e.value) and why in str(e.value), str(e.value)


def test_beat_synchronous_chroma_is_not_implemented():
    cfg = sdsp.default_config()
    cfg.enable_key_beat_synchronous = 1
    cfg.enable_key_log_frequency = 0
    with pytest.raises(sdsp.AnalysisError) as e:
        sdsp.analyze_batch_device_requests(0, [0], [100], config=cfg, device=9999,
                                           key_timeline=sdsp.key_timeline_request(segment_seconds=8.0))
    assert e.value.code == NOT_IMPLEMENTED and "Not implemented: key timeline with beat-synchronous chroma" in str(e.value)


def test_a_bad_overview_request_is_refused_through_the_new_entry_too():
    with pytest.raises(sdsp.AnalysisError) as e:
        sdsp.analyze_batch_device_requests(0, [0], [100], device=9999, overview=sdsp.overview_request(columns=4, frames_per_column=4),
                                           key_timeline=sdsp.key_timeline_request(segment_seconds=8.0))
    assert e.value.code == INVALID and "both columns and frames_per_column" in str(e.value)


def test_bad_request_fills_every_slot():
    n = 3
    outs = (sdsp_abi.SdspResult * n)()
    kts = (sdsp_abi.SdspKeyTimeline * n)()
    ovs = (sdsp_abi.SdspOverview * n)()
    for t, o in zip(kts, ovs):
        t.n_segments = t.primary_count = 77  # stale contents the call must clear
        o.n_columns = 77
    offs, lens = np.zeros(n, np.uint64), np.full(n, 10, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    cfg = sdsp.default_config()
    oreq = sdsp.overview_request(columns=4)
    req = sdsp.key_timeline_request(segment_seconds=8.0, overlap_seconds=9.0)
    st = sdsp.lib().sdsp_analyze_batch_device_requests(None, offs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), n, 44100,
                                                       C.byref(cfg), 0, None, 0, outs, C.byref(oreq), ovs, C.byref(req), kts)
    assert st == INVALID
    for i in range(n):
        assert outs[i].status == INVALID and outs[i].error_message.decode().startswith("Invalid input: key timeline")
        assert kts[i].status == INVALID and kts[i].n_segments == 0 and kts[i].primary_count == 0 and not kts[i].segments
        assert ovs[i].status == INVALID and ovs[i].n_columns == 0


def test_debug_entry_refuses_a_bad_request_without_a_device():
    with pytest.raises(sdsp.AnalysisError) as e:
        sdsp.debug_key_timeline([np.zeros((4, 12), np.float32)], sdsp.key_timeline_request(), device=9999)
    assert e.value.code == INVALID


def test_good_request_without_gpu_fails_loudly():
    if sdsp.device_count() > 0:
        pytest.skip("a GPU is visible")
    for kw in (dict(segment_seconds=8.0, overlap_seconds=2.0), dict(segment_frames=64, hop_frames=1)):
        with pytest.raises(sdsp.AnalysisError) as e:
            sdsp.analyze_batch_device_requests(0, [0], [44100], key_timeline=sdsp.key_timeline_request(**kw))
        assert e.value.kind == "ProcessingError" and str(e.value).endswith("Processing error: no HIP device"), str(e.value)
