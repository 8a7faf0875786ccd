"""sdsp_decode_audio_batch_device at the drop-in boundary, without a GPU: the entries are declared
and exported, the ctypes mirror of sdsp_audio_decode_stats has exactly the C layout (every field's
offset against a compiled C11 probe of the header), and with no HIP device the entry fails as the
lossless entry does (SDSP_ERR_PROCESSING, the same text in every slot)."""
import ctypes as C
import os
import subprocess

import pytest

import sdsp
import sdsp_abi
import vorbis_streams as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stratum_hip.h")


def test_audio_decode_stats_layout_matches_header(tmp_path):
    py = sdsp_abi.SdspAudioDecodeStats
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(sdsp_audio_decode_stats));']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(sdsp_audio_decode_stats, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    c = dict(ln.rsplit(" ", 1) for ln in subprocess.check_output([str(exe)]).decode().splitlines() if ln)
    assert int(c["size"]) == C.sizeof(py)
    for f, _ in py._fields_:
        assert int(c[f]) == getattr(py, f).offset, f
    lossless = [f for f, _ in sdsp_abi.SdspDecodeStats._fields_]
    new = ["vorbis_files", "vorbis_packets", "vorbis_packets_zeroed", "vorbis_ms"]
    assert sorted(f for f, _ in py._fields_) == sorted(lossless + new)


def test_entries_are_declared_and_exported():
    lib = sdsp.lib()
    pub = open(HEADER).read()
    dbg = open(os.path.join(ROOT, "include", "stratum_hip_debug.h")).read()
    for name in ("sdsp_decode_audio_batch_device", "sdsp_last_audio_decode_stats"):
        assert name + "(" in pub and hasattr(lib, name)
    assert "sdsp_debug_vorbis_decode_phased(" in dbg and hasattr(lib, "sdsp_debug_vorbis_decode_phased")


def test_without_a_device_the_call_fails_as_the_lossless_entry_does():
    blobs = [vs.matrix()[1][1], vs.matrix()[2][1]]
    if sdsp.device_count() > 0:  # with a GPU the same call decodes both files
        buf, offs, lens, rates, errors, st = sdsp.decode_audio_batch_device(blobs)
        buf.free()
        assert errors == [None, None] and st["vorbis_files"] == 2
        return
    with pytest.raises(sdsp.AnalysisError) as e:
        sdsp.decode_audio_batch_device(blobs)
    assert e.value.kind == "ProcessingError" and str(e.value) == "Processing error: no HIP device"
    assert sdsp.audio_decode_stats()["files"] == 0
