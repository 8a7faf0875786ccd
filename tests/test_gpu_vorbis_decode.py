"""The device Vorbis decode (sdsp_decode_audio_batch_device: k_vorbis_packets, k_vorbis_imdct,
k_vorbis_ola) against the host decoder (sdsp_decode_audio_file) on the GPU.  Streams come from
tests/vorbis_streams.py.  Every comparison is np.array_equal on the uint32 view of the samples, and
equality of lengths, rates, status codes and error texts: no tolerance.  No test can pass by
falling back: the Vorbis file count, the fallback count and the error count are asserted.
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
import vorbis_streams as vs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REAL = os.path.join(GOLDEN, "real_libvorbis_keypress.ogg")


def _alloc_stats():
    f = sdsp.lib().sdsp_debug_alloc_stats
    f.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    n, b = C.c_uint64(), C.c_uint64()
    assert f(C.byref(n), C.byref(b)) == 0
    return n.value, b.value


_HOST = {}


def _host(tmp_path, data):
    """(samples, rate) or the AnalysisError of the host decoder, computed once per blob."""
    key = hash(data)
    if key not in _HOST:
        p = tmp_path / "t.ogg"
        p.write_bytes(data)
        try:
            _HOST[key] = sdsp.decode_audio_file(str(p))
        except sdsp.AnalysisError as e:
            _HOST[key] = e
    return _HOST[key]


def _planned(data):
    """True when the host plan takes the bytes as a Vorbis stream with a valid setup (then the device
    decodes it); False when the host refuses them or they are no Vorbis stream any more."""
    try:
        sdsp.debug_vorbis_decode_phased(data)
        return True
    except sdsp.AnalysisError:
        return False


def _decode_and_compare(tmp_path, blobs, entry=None):
    """One batch call; every file is compared with the host decode (none skipped).  Returns stats."""
    buf, offs, lens, rates, errors, stats = (entry or sdsp.decode_audio_batch_device)(blobs)
    n_err = 0
    try:
        allx = buf.to_host() if buf.n else np.zeros(0, np.float32)
        for i, data in enumerate(blobs):
            want = _host(tmp_path, data)
            if isinstance(want, sdsp.AnalysisError):
                assert errors[i] is not None and errors[i].code == want.code and str(errors[i]) == str(want), i
                assert lens[i] == 0
                n_err += 1
                continue
            want, sr = want
            assert errors[i] is None, (i, errors[i])
            assert int(lens[i]) == want.size and int(rates[i]) == sr, i
            got = allx[int(offs[i]):int(offs[i]) + int(lens[i])]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), i
    finally:
        buf.free()
    assert stats["files"] == len(blobs) and stats["bytes_in"] == sum(len(b) for b in blobs)
    assert stats["samples_out"] == int(lens.sum())
    assert stats["error_files"] == n_err
    return stats


def _counts(st):
    return {k: v for k, v in st.items() if not k.endswith("_ms")}


def test_matrix_in_one_ragged_batch(tmp_path):
    blobs = [d for _, d in vs.matrix()]
    st = _decode_and_compare(tmp_path, blobs)
    assert st["vorbis_files"] == st["device_files"] == len(blobs)
    assert st["host_fallback_files"] == 0 and st["error_files"] == 0
    assert st["vorbis_packets"] > 64 * 3 and st["vorbis_packets_zeroed"] >= 2
    before = _alloc_stats()
    st2 = _decode_and_compare(tmp_path, blobs)
    assert _alloc_stats() == before  # a second identical call allocates nothing
    assert _counts(st2) == _counts(st)


def test_damaged_variants_with_good_files_between(tmp_path):
    good = [d for _, d in vs.matrix()][:4]
    blobs = []
    for i, (_, d) in enumerate(vs.damaged()):
        blobs.append(d)
        if i % 10 == 0:
            blobs.append(good[(i // 10) % 4])
    planned = sum(_planned(d) for d in blobs)
    refused = sum(isinstance(_host(tmp_path, d), sdsp.AnalysisError) for d in blobs)
    assert 0 < refused < len(blobs)
    st = _decode_and_compare(tmp_path, blobs)
    assert st["vorbis_files"] == planned and st["error_files"] == refused
    assert st["host_fallback_files"] == 0  # what is not planned here is refused by the host as well
    assert planned + refused == len(blobs)


def test_real_file_alone_and_in_a_mixed_batch(tmp_path):
    ogg = open(REAL, "rb").read()
    st = _decode_and_compare(tmp_path, [ogg])
    assert st["vorbis_files"] == 1 and st["host_fallback_files"] == 0 and st["vorbis_packets"] == 26
    broken = ogg[:4000]
    # the comment header's page loses its capture pattern: no setup header where it belongs
    broken = broken[:60] + bytes([broken[60] ^ 0x10]) + broken[61:]
    blobs = [fs.matrix()[0][1], ogg, dict(als.matrix())["stereo16_mix2_1.m4a"], dict(ps.matrix())["wav_s24_2ch"], broken,
             dict(vs.matrix())["three_64_256_r0"]]
    st = _decode_and_compare(tmp_path, blobs)
    assert (st["flac_files"], st["alac_files"], st["pcm_files"], st["vorbis_files"]) == (1, 1, 1, 2)
    assert st["device_files"] == 5 and st["host_fallback_files"] == 0 and st["error_files"] == 1
    before = _alloc_stats()
    st2 = _decode_and_compare(tmp_path, blobs)
    assert _alloc_stats() == before and _counts(st2) == _counts(st)


def test_the_lossless_entry_still_leaves_ogg_to_the_host(tmp_path):
    ogg = open(REAL, "rb").read()
    st = _decode_and_compare(tmp_path, [ogg, dict(vs.matrix())["mono_64_mixed_r2"]], entry=sdsp.decode_batch_device)
    assert st["host_fallback_files"] == 2 and st["device_files"] == 0 and "vorbis_files" not in st


def test_device_decode_feeds_the_analysis(tmp_path):
    ogg = open(REAL, "rb").read()
    host, sr = _host(tmp_path, ogg)
    buf, offs, lens, rates, errors, st = sdsp.decode_audio_batch_device([ogg])
    try:
        assert errors == [None] and st["vorbis_files"] == 1 and st["host_fallback_files"] == 0
        assert int(lens[0]) == host.size and int(rates[0]) == sr
        got = sdsp.analyze_batch_device(buf.ptr, offs, lens, int(rates[0]))[0]
    finally:
        buf.free()
    try:
        ref = sdsp.analyze_audio(host, sr)
    except sdsp.AnalysisError as e:  # the file is half a second long: the analysis may refuse it, both ways alike
        assert isinstance(got, sdsp.AnalysisError) and (got.code, str(got)) == (e.code, str(e))
        return
    assert not isinstance(got, Exception), got
    assert parity.diff_results(got, ref, tol=0.0) == []
    assert parity.exact_fraction(got, ref, strict=True) == 1.0
