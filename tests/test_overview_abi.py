"""The overview entry at the drop-in boundary, without a GPU (CPU only).

* sdsp_abi's mirrors of sdsp_overview_request, sdsp_overview and sdsp_debug_overview_times have
  exactly the C layout (every field's offset against a compiled C11 probe of the headers, as
  test_abi.py does for the existing structs);
* every bad request fails the call with SDSP_ERR_INVALID_INPUT and its reason before any device is
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

STRUCTS = {"sdsp_overview_request": sdsp_abi.SdspOverviewRequest, "sdsp_overview": sdsp_abi.SdspOverview,
           "sdsp_debug_overview_times": sdsp_abi.SdspDebugOverviewTimes}


def test_overview_struct_layouts_match_header(tmp_path):
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
    # the header's field list, name by name and in order
    src = open(os.path.join(ROOT, "include", "stratum_hip.h")).read()
    body = src[src.index("typedef struct sdsp_overview {"):src.index("} sdsp_overview;")]
    for f, _ in sdsp_abi.SdspOverview._fields_:
        assert f in body, f


def test_entries_exported_and_existing_abi_untouched():
    L = sdsp.lib()
    for name in ("sdsp_analyze_batch_device_overview", "sdsp_overview_free", "sdsp_debug_last_overview_times"):
        assert hasattr(L, name), name
    assert C.sizeof(sdsp_abi.SdspOverviewRequest) == 16


BAD = [
    (dict(columns=0, frames_per_column=0), "neither columns nor frames_per_column"),
    (dict(columns=8, frames_per_column=8), "both columns and frames_per_column"),
    (dict(columns=8, low_max_hz=float("nan")), "not finite"),
    (dict(columns=8, mid_max_hz=float("nan")), "not finite"),
    (dict(columns=8, mid_max_hz=float("inf")), "not finite"),
    (dict(frames_per_column=8, low_max_hz=float("-inf")), "not finite"),
    (dict(columns=8, low_max_hz=-1.0), "negative"),
    (dict(frames_per_column=8, low_max_hz=0.0, mid_max_hz=-0.5), "negative"),
    (dict(columns=8, low_max_hz=4000.0, mid_max_hz=250.0), "low_max_hz > mid_max_hz"),
]


@pytest.mark.parametrize("kw,why", BAD)
def test_bad_request_is_refused_before_the_device(kw, why):
    """A null device pointer and device 9999: had the call gone as far as a device, the error would
    be the device's (and on a machine without a GPU, "no HIP device")."""
    with pytest.raises(sdsp.AnalysisError) as e:
        sdsp.analyze_batch_device_overview(0, [0, 100], [100, 50], device=9999, request=sdsp.overview_request(**kw))
    assert e.value.code == 1 and e.value.kind == "InvalidInput"
    assert "Invalid input: overview" in str(e.value) and why in str(e.value), str(e.value)


def test_bad_request_fills_every_slot():
    n = 3
    outs = (sdsp_abi.SdspResult * n)()
    ovs = (sdsp_abi.SdspOverview * n)()
    for o in ovs:
        o.n_columns = 77  # stale contents the call must clear
    offs, lens = np.zeros(n, np.uint64), np.full(n, 10, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    cfg = sdsp.default_config()
    req = sdsp.overview_request(columns=4, frames_per_column=4)
    st = sdsp.lib().sdsp_analyze_batch_device_overview(None, offs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), n, 44100,
                                                       C.byref(cfg), 0, None, 0, outs, C.byref(req), ovs)
    assert st == 1
    for i in range(n):
        assert outs[i].status == 1 and outs[i].error_message.decode().startswith("Invalid input: overview request")
        assert ovs[i].status == 1 and ovs[i].n_columns == 0 and not ovs[i].smin


def test_good_request_without_gpu_fails_loudly():
    if sdsp.device_count() > 0:
        pytest.skip("a GPU is visible")
    for kw in (dict(columns=256), dict(frames_per_column=7, low_max_hz=0.0, mid_max_hz=22050.0)):
        with pytest.raises(sdsp.AnalysisError) as e:
            sdsp.analyze_batch_device_overview(0, [0], [44100], request=sdsp.overview_request(**kw))
        assert e.value.kind == "ProcessingError" and str(e.value).endswith("Processing error: no HIP device"), str(e.value)
