"""The device FLAC decoder (sdsp_decode_flac_batch_device: k_flac_scan, k_flac_frames, k_flac_chain,
k_flac_gather) against the host decoder (sdsp_decode_audio_file) on the GPU.  Streams come from
tests/flac_enc.py (tests/flac_streams.py).  Every comparison is np.array_equal on the uint32 view
of the samples: no tolerance.
"""
import ctypes as C

import numpy as np
import pytest

import flac_enc as fe
import flac_streams as fs
import parity
import sdsp
import synth

pytestmark = pytest.mark.gpu


def _host(tmp_path, data):
    p = tmp_path / "t.flac"
    p.write_bytes(data)
    return sdsp.decode_audio_file(str(p))


def _alloc_stats():
    f = sdsp.lib().sdsp_debug_alloc_stats
    f.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    n, b = C.c_uint64(), C.c_uint64()
    assert f(C.byref(n), C.byref(b)) == 0
    return n.value, b.value


def _decode_and_compare(tmp_path, blobs):
    """One batch call; every good file's samples, length and rate equal the host decode, every bad
    file's status and text equal the host's.  Returns the stats."""
    buf, offs, lens, rates, errors, stats = sdsp.decode_flac_batch_device(blobs)
    try:
        allx = buf.to_host() if buf.n else np.zeros(0, np.float32)
        for i, data in enumerate(blobs):
            try:
                want, sr = _host(tmp_path, data)
            except sdsp.AnalysisError as e:
                assert errors[i] is not None and errors[i].code == e.code and str(errors[i]) == str(e), i
                assert lens[i] == 0
                continue
            assert errors[i] is None, (i, errors[i])
            assert int(lens[i]) == want.size and int(rates[i]) == sr, i
            got = allx[int(offs[i]):int(offs[i]) + int(lens[i])]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), i
    finally:
        buf.free()
    assert stats["files"] == len(blobs)
    return stats


def test_matrix_in_one_ragged_batch(tmp_path):
    blobs = [d for _, d in fs.matrix()]
    n = len(blobs)
    st = _decode_and_compare(tmp_path, blobs)
    assert st["device_files"] == n and st["host_fallback_files"] == 0 and st["error_files"] == 0
    assert st["frames_rejected"] == 0 and st["frames_accepted"] > n and st["candidates"] >= st["frames_accepted"]
    assert st["bytes_in"] == sum(len(b) for b in blobs) and st["samples_out"] > 0
    before = _alloc_stats()
    st2 = _decode_and_compare(tmp_path, blobs)
    assert _alloc_stats() == before  # a second identical call allocates nothing
    assert {k: v for k, v in st2.items() if not k.endswith("_ms")} == {k: v for k, v in st.items() if not k.endswith("_ms")}


def test_edge_block_sizes(tmp_path):
    blobs = [d for _, d in fs.edge_block_sizes()]
    st = _decode_and_compare(tmp_path, blobs)
    assert st["device_files"] == len(blobs) and st["host_fallback_files"] == 0
    assert st["frames_accepted"] == len(blobs) and st["frames_rejected"] == 0


@pytest.mark.parametrize("n", [63, 64, 65])
def test_candidate_counts_at_the_wave_edge(tmp_path, n):
    st = _decode_and_compare(tmp_path, [fs.many_frames(n)])
    assert st["candidates"] == n and st["frames_accepted"] == n and st["device_files"] == 1


def test_damaged_streams(tmp_path):
    names = [n for n, _ in fs.damaged()]
    for name, data in fs.damaged():  # one call each: the stats are per call
        st = _decode_and_compare(tmp_path, [data])
        assert st["device_files"] == 1 and st["host_fallback_files"] == 0, name
        if name == "crc16_middle":
            assert (st["frames_accepted"], st["frames_rejected"]) == (2, 1)
        elif name == "false_header_in_good_frame":
            assert st["candidates"] > st["frames_accepted"] == 3 and st["frames_rejected"] == 0
        elif name == "false_header_in_bad_frame":
            assert st["frames_accepted"] == 2 and st["frames_rejected"] >= 2  # the chain tried the planted header
    st = _decode_and_compare(tmp_path, [d for _, d in fs.damaged()])  # and all in one batch
    assert st["device_files"] == len(names)


def test_errors_in_a_batch(tmp_path):
    good = [fs.matrix()[0][1], fs.many_frames(64), fs.matrix()[-1][1]]
    bad = [d for _, d in fs.error_blobs()]
    blobs = [good[0], bad[0], good[1], bad[1], bad[2], good[2]]
    st = _decode_and_compare(tmp_path, blobs)
    assert st["error_files"] == 3 and st["device_files"] == 3 and st["host_fallback_files"] == 0


def test_device_decode_feeds_the_analysis(tmp_path):
    x, _, _, _ = synth.make_track(3, seconds=5.0)
    pcm = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int64)
    frames = [fe.frame([pcm[o:o + 4096]], 16, k, specs=[{"type": "fixed", "order": 2}])
              for k, o in enumerate(range(0, pcm.size, 4096))]
    data = fe.stream(frames, 44100, 1, 16, total=pcm.size)
    host, sr = _host(tmp_path, data)
    assert sr == 44100 and host.size == pcm.size
    buf, offs, lens, rates, errors, st = sdsp.decode_flac_batch_device([data])
    try:
        assert errors == [None] and st["device_files"] == 1 and int(lens[0]) == pcm.size
        got = sdsp.analyze_batch_device(buf.ptr, offs, lens, int(rates[0]))[0]
    finally:
        buf.free()
    ref = sdsp.analyze_batch([host], sr)[0]
    assert not isinstance(got, Exception) and not isinstance(ref, Exception)
    assert parity.diff_results(got, ref, tol=0.0) == []
