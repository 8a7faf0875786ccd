"""The batched lossless device decode (sdsp_decode_batch_device: the FLAC kernels, k_alac_frames /
k_alac_offsets / k_alac_gather, k_pcm_mono, host fallbacks, one output buffer) against the host
decoder (sdsp_decode_audio_file) on the GPU.  Streams come from tests/alac_streams.py,
tests/pcm_streams.py and tests/flac_streams.py.  Every comparison is np.array_equal on the uint32
view of the samples, and equality of lengths, rates, status codes and error texts: no tolerance.
"""
import ctypes as C
import os

import numpy as np
import pytest

import alac_streams as als
import flac_streams as fs
import parity
import pcm_streams as ps
import sdsp
import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _host(tmp_path, data):
    p = tmp_path / "t.bin"
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
    file's status and text equal the host's.  Returns (stats, rates)."""
    buf, offs, lens, rates, errors, stats = sdsp.decode_batch_device(blobs)
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
    assert stats["files"] == len(blobs) and stats["bytes_in"] == sum(len(b) for b in blobs)
    assert stats["device_files"] == stats["flac_files"] + stats["alac_files"] + stats["pcm_files"]
    assert stats["samples_out"] == int(lens.sum())
    return stats, rates


def _counts(st):
    return {k: v for k, v in st.items() if not k.endswith("_ms")}


def test_alac_matrix_in_one_ragged_batch(tmp_path):
    blobs = [d for _, d in als.matrix()]
    n = len(blobs)
    st, _ = _decode_and_compare(tmp_path, blobs)
    # the device bound on frame_length is a condition of the format, not of these streams: none may fall back
    assert st["alac_files"] == n and st["host_fallback_files"] == 0 and st["error_files"] == 0
    assert st["alac_packets_skipped"] == 0 and st["alac_packets_decoded"] == st["alac_packets"] > n
    before = _alloc_stats()
    st2, _ = _decode_and_compare(tmp_path, blobs)
    assert _alloc_stats() == before  # a second identical call allocates nothing
    assert _counts(st2) == _counts(st)


def test_packet_counts_at_the_wave_edge(tmp_path):
    for n in (63, 64, 65):
        st, _ = _decode_and_compare(tmp_path, [als.many_packets(n)])
        assert st["alac_packets"] == st["alac_packets_decoded"] == n and st["alac_files"] == 1
    st, _ = _decode_and_compare(tmp_path, [als.many_packets(n) for n in (63, 64, 65)])  # waves that span files
    assert st["alac_packets_decoded"] == 192


def test_alac_edges_and_damaged_files(tmp_path):
    for name, data, dec, skp in als.edges():  # one call each: the stats are per call
        st, _ = _decode_and_compare(tmp_path, [data])
        assert st["alac_files"] == 1 and st["host_fallback_files"] == 0 and st["error_files"] == 0, name
        assert (st["alac_packets_decoded"], st["alac_packets_skipped"]) == (dec, skp), name
    for name, data, text in als.refused():
        st, _ = _decode_and_compare(tmp_path, [data])
        assert st["error_files"] == 1 and st["device_files"] == 0 and st["host_fallback_files"] == 0, name
    blobs = [e[1] for e in als.edges()] + [e[1] for e in als.refused()]  # and all in one batch
    st, _ = _decode_and_compare(tmp_path, blobs)
    assert st["alac_files"] == len(als.edges()) and st["error_files"] == len(als.refused())
    assert st["alac_packets_decoded"] == sum(e[2] for e in als.edges())
    assert st["alac_packets_skipped"] == sum(e[3] for e in als.edges())


def test_long_frames_fall_back_to_the_host(tmp_path):
    st, _ = _decode_and_compare(tmp_path, [als.long_frames(), als.matrix()[0][1]])
    assert st["host_fallback_files"] == 1 and st["alac_files"] == 1 and st["error_files"] == 0


def test_pcm_matrix_and_edges_in_one_batch(tmp_path):
    linear = [d for _, d in ps.matrix()] + [d for _, d in ps.edges()]
    other = [d for _, d in ps.not_linear()]
    refused = [d for _, d in ps.refused()]
    blobs = linear[:10] + other[:2] + refused + linear[10:] + other[2:]
    st, _ = _decode_and_compare(tmp_path, blobs)
    assert st["pcm_files"] == len(linear) and st["host_fallback_files"] == len(other)
    assert st["error_files"] == len(refused) and st["alac_files"] == st["flac_files"] == 0
    before = _alloc_stats()
    st2, _ = _decode_and_compare(tmp_path, blobs)
    assert _alloc_stats() == before and _counts(st2) == _counts(st)


def test_wide_pcm_falls_back_to_the_host(tmp_path):
    st, _ = _decode_and_compare(tmp_path, [ps.wav_of("s16", 8, 100, 1), ps.wav_of("s16", 9, 100, 2)])
    assert st["pcm_files"] == 1 and st["host_fallback_files"] == 1


def test_mixed_batch(tmp_path):
    am = dict(als.matrix())
    pm = dict(ps.matrix())
    flac = fs.matrix()[0][1]
    ogg = open(os.path.join(GOLDEN, "real_libvorbis_keypress.ogg"), "rb").read()
    blobs = [flac, am["stereo16_mix2_1.m4a"], am["bits24_shift1.caf"], pm["wav_s24_2ch"], pm["aiff_s16_1ch"], ogg,
             flac[:len(flac) // 2], als.refused()[1][1], am["mono16_specs.m4a"], fs.matrix()[-2][1]]
    st, rates = _decode_and_compare(tmp_path, blobs)
    assert (st["flac_files"], st["alac_files"], st["pcm_files"]) == (3, 3, 2)
    assert st["host_fallback_files"] == 1 and st["error_files"] == 1
    assert len({int(r) for r in rates if r}) >= 3  # the rates differ across the files
    before = _alloc_stats()
    st2, _ = _decode_and_compare(tmp_path, blobs)
    assert _alloc_stats() == before and _counts(st2) == _counts(st)


def test_empty_batch_and_flac_entry_unchanged(tmp_path):
    buf, offs, lens, rates, errors, st = sdsp.decode_batch_device([])
    buf.free()
    assert st["files"] == 0 and st["samples_out"] == 0
    # the FLAC entry keeps its contract: a file that is not native FLAC goes to the host decoder there
    buf, offs, lens, rates, errors, st = sdsp.decode_flac_batch_device([fs.matrix()[0][1], dict(ps.matrix())["wav_s16_1ch"]])
    buf.free()
    assert errors == [None, None] and st["device_files"] == 1 and st["host_fallback_files"] == 1
    assert sdsp.flac_decode_stats()["files"] == 2


def test_device_decode_feeds_the_analysis(tmp_path):
    x, _, _, _ = synth.make_track(3, seconds=5.0)
    x = np.ascontiguousarray(x, np.float32)
    for data in (als.passage(x.tobytes()), ps.passage_wav24(x)):
        host, sr = _host(tmp_path, data)
        assert sr == 44100 and host.size == x.size
        buf, offs, lens, rates, errors, st = sdsp.decode_batch_device([data])
        try:
            assert errors == [None] and st["device_files"] == 1 and st["host_fallback_files"] == 0
            assert int(lens[0]) == x.size
            got = sdsp.analyze_batch_device(buf.ptr, offs, lens, int(rates[0]))[0]
        finally:
            buf.free()
        ref = sdsp.analyze_batch([host], sr)[0]
        assert not isinstance(got, Exception) and not isinstance(ref, Exception)
        assert parity.diff_results(got, ref, tol=0.0) == []
