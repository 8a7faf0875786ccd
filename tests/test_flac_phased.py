"""The device FLAC decoder's four phases on the CPU (sdsp_debug_flac_decode_phased: scan every
offset, decode every candidate, chain, gather) against the host decoder (sdsp_decode_audio_file),
through the frame-level code the kernels run (stratum-dsp_amd/csrc/flac_core.hpp).  CPU only.

Every comparison is np.array_equal on the uint32 view of the samples: no tolerance.  Also the
layout of sdsp_flac_decode_stats against a compiled probe of the header, and the loud failure of
sdsp_decode_flac_batch_device without a GPU.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flac_streams as fs
import sdsp
import sdsp_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stratum_hip.h")


def _host(tmp_path, data):
    p = tmp_path / "t.flac"
    p.write_bytes(data)
    return sdsp.decode_audio_file(str(p))


def _same(tmp_path, data):
    want, want_sr = _host(tmp_path, data)
    got, sr, counts = sdsp.debug_flac_decode_phased(data)
    assert sr == want_sr
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return got, counts


@pytest.mark.parametrize("i", range(len(fs.matrix())), ids=[n for n, _ in fs.matrix()])
def test_phased_equals_host_on_every_stream_class(tmp_path, i):
    x, (cand, acc, rej) = _same(tmp_path, fs.matrix()[i][1])
    assert x.size > 0 and acc > 0 and rej == 0 and cand >= acc


@pytest.mark.parametrize("i", range(len(fs.edge_block_sizes())), ids=[n for n, _ in fs.edge_block_sizes()])
def test_phased_equals_host_on_edge_block_sizes(tmp_path, i):
    x, (cand, acc, rej) = _same(tmp_path, fs.edge_block_sizes()[i][1])
    assert acc == 1 and rej == 0 and x.size > 0


@pytest.mark.parametrize("n", [63, 64, 65])
def test_phased_candidate_counts(tmp_path, n):
    x, counts = _same(tmp_path, fs.many_frames(n))
    assert counts == (n, n, 0) and x.size == 16 * n


@pytest.mark.parametrize("i", range(len(fs.damaged())), ids=[n for n, _ in fs.damaged()])
def test_phased_equals_host_on_damaged_streams(tmp_path, i):
    name, data = fs.damaged()[i]
    x, (cand, acc, rej) = _same(tmp_path, data)
    if name == "crc16_middle":
        assert (acc, rej) == (2, 1) and x.size == 2 * 1152  # the later samples move earlier
    elif name == "crc8_middle":
        assert acc == 2 and x.size == 2 * 1152  # never a candidate: the scan refuses the header
    elif name == "truncated_in_residual":
        assert (acc, rej) == (1, 1) and x.size == 1152
    elif name == "false_header_in_good_frame":
        assert cand > acc and (acc, rej) == (3, 0) and x.size == 3 * 1152  # the chain never looks inside a good frame
    else:
        assert acc == 2 and rej >= 2 and x.size == 2 * 1152  # the enclosing frame, then the planted header


@pytest.mark.parametrize("i", range(len(fs.error_blobs())), ids=[n for n, _ in fs.error_blobs()])
def test_phased_errors_equal_host(tmp_path, i):
    name, data = fs.error_blobs()[i]
    with pytest.raises(sdsp.AnalysisError) as want:
        _host(tmp_path, data)
    if name == "not_flac":  # not FLAC by its magic number: the front-end never reaches a FLAC decoder
        with pytest.raises(sdsp.AnalysisError) as got:
            sdsp.debug_flac_decode_phased(data)
        assert got.value.code == want.value.code == 2 and "not a FLAC stream" in str(got.value)
        return
    with pytest.raises(sdsp.AnalysisError) as got:
        sdsp.debug_flac_decode_phased(data)
    assert got.value.code == want.value.code == 2 and str(got.value) == str(want.value)


def test_flac_decode_stats_layout_matches_header(tmp_path):
    py = sdsp_abi.SdspFlacDecodeStats
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(sdsp_flac_decode_stats));']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(sdsp_flac_decode_stats, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    c = dict(ln.rsplit(" ", 1) for ln in subprocess.check_output([str(exe)]).decode().splitlines() if ln)
    assert int(c["size"]) == C.sizeof(py)
    assert len(py._fields_) == 14
    for f, _ in py._fields_:
        assert int(c[f]) == getattr(py, f).offset, f


def test_device_decode_without_gpu_fails_loudly():
    if sdsp.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(sdsp.AnalysisError) as e:
        sdsp.decode_flac_batch_device([fs.many_frames(63)])
    assert "no HIP device" in str(e.value) and e.value.code == 3
