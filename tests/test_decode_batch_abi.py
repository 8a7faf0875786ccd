"""The batched lossless decode entry at the drop-in boundary, without a GPU: the ctypes mirror of
sdsp_decode_stats has exactly the C layout (every field's offset against a compiled probe of the
header), the new entries are declared and exported, and with no HIP device the entry fails as the
FLAC entry does (SDSP_ERR_PROCESSING, the same text in every slot)."""
import ctypes as C
import os
import subprocess

import pytest

import alac_streams as als
import pcm_streams as ps
import sdsp
import sdsp_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stratum_hip.h")


def test_decode_stats_layout_matches_header(tmp_path):
    py = sdsp_abi.SdspDecodeStats
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(sdsp_decode_stats));']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(sdsp_decode_stats, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    c = dict(ln.rsplit(" ", 1) for ln in subprocess.check_output([str(exe)]).decode().splitlines() if ln)
    assert int(c["size"]) == C.sizeof(py)
    for f, _ in py._fields_:
        assert int(c[f]) == getattr(py, f).offset, f
    want = ["files", "device_files", "host_fallback_files", "error_files", "flac_files", "alac_files", "pcm_files",
            "alac_packets", "alac_packets_decoded", "alac_packets_skipped", "bytes_in", "samples_out", "upload_ms",
            "flac_ms", "alac_ms", "pcm_ms", "gather_ms", "total_ms"]
    assert [f for f, _ in py._fields_] == want


def test_entries_are_declared_and_exported():
    lib = sdsp.lib()
    pub = open(HEADER).read()
    dbg = open(os.path.join(ROOT, "include", "stratum_hip_debug.h")).read()
    for name in ("sdsp_decode_batch_device", "sdsp_last_decode_stats"):
        assert name + "(" in pub and hasattr(lib, name)
    for name in ("sdsp_debug_alac_decode_phased", "sdsp_debug_pcm_decode_planned"):
        assert name + "(" in dbg and hasattr(lib, name)


def test_without_a_device_the_call_fails_as_the_flac_entry_does():
    blobs = [als.matrix()[0][1], ps.matrix()[0][1]]
    if sdsp.device_count() > 0:  # with a GPU the same call decodes both files
        buf, offs, lens, rates, errors, st = sdsp.decode_batch_device(blobs)
        buf.free()
        assert errors == [None, None] and st["device_files"] == 2
        return
    for entry in (sdsp.decode_batch_device, sdsp.decode_flac_batch_device):
        with pytest.raises(sdsp.AnalysisError) as e:
            entry(blobs)
        assert e.value.kind == "ProcessingError" and str(e.value) == "Processing error: no HIP device"
    assert sdsp.decode_stats()["files"] == 0
