"""The device ALAC decoder's phases on the CPU (sdsp_debug_alac_decode_phased: the host plan, every
packet decoded into its own slot through csrc/alac_core.hpp, the offsets walk, the gather) against
the host decoder (sdsp_decode_audio_file), which runs the same core packet after packet.  Streams
come from tests/alac_enc.py (tests/alac_streams.py).  Every comparison is np.array_equal on the
uint32 view of the samples: no tolerance.  No GPU.
"""
import numpy as np
import pytest

import alac_streams as als
import sdsp


def _host(tmp_path, data, name="t.bin"):
    p = tmp_path / name
    p.write_bytes(data)
    return sdsp.decode_audio_file(str(p))


def _same(tmp_path, data):
    want, sr = _host(tmp_path, data)
    got, sr2, counts = sdsp.debug_alac_decode_phased(data)
    assert sr2 == sr and got.size == want.size
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return want, counts


@pytest.mark.parametrize("name,data", als.matrix(), ids=[n for n, _ in als.matrix()])
def test_matrix(tmp_path, name, data):
    want, (packets, decoded, skipped) = _same(tmp_path, data)
    assert want.size > 0 and packets == decoded > 0 and skipped == 0


@pytest.mark.parametrize("name,data,dec,skp", als.edges(), ids=[e[0] for e in als.edges()])
def test_edges(tmp_path, name, data, dec, skp):
    want, (packets, decoded, skipped) = _same(tmp_path, data)
    assert (decoded, skipped) == (dec, skp) and packets == dec + skp
    if name == "no_packets.caf":
        assert want.size == 0


def test_damaged_packets_leave_the_others_contiguous(tmp_path):
    """A skipped packet first, in the middle and last: the track is the other two packets back to back."""
    by = {n: d for n, d, _, _ in als.edges()}
    for ext in (".caf", ".m4a"):
        full = [_host(tmp_path, by[f"damaged_{w}{ext}"])[0] for w in ("first", "middle", "last")]
        a, b, c = full[1][:1024], full[0][:1024], full[0][1024:]  # packets 0, 1, 2
        assert np.array_equal(full[0], np.concatenate([b, c])) and np.array_equal(full[2], np.concatenate([a, b]))
        assert np.array_equal(full[1], np.concatenate([a, c]))
        for w in ("first", "middle", "last"):
            got, _, _ = sdsp.debug_alac_decode_phased(by[f"damaged_{w}{ext}"])
            assert got.size == 2048


@pytest.mark.parametrize("n", [63, 64, 65])
def test_many_packets(tmp_path, n):
    _, counts = _same(tmp_path, als.many_packets(n))
    assert counts == (n, n, 0)


def test_long_frames(tmp_path):
    want, counts = _same(tmp_path, als.long_frames())
    assert want.size == 32768 + 64 and counts == (2, 2, 0)


@pytest.mark.parametrize("name,data,text", als.refused(), ids=[e[0] for e in als.refused()])
def test_refused_files_carry_the_hosts_text(tmp_path, name, data, text):
    with pytest.raises(sdsp.AnalysisError) as want:
        _host(tmp_path, data)
    with pytest.raises(sdsp.AnalysisError) as got:
        sdsp.debug_alac_decode_phased(data)
    assert text in str(want.value)
    assert got.value.code == want.value.code and str(got.value) == str(want.value)


def test_other_containers_are_not_planned():
    import pcm_streams as ps
    for data in (ps.matrix()[0][1], b"fLaC" + bytes(64), b"OggS" + bytes(64)):
        with pytest.raises(sdsp.AnalysisError) as e:
            sdsp.debug_alac_decode_phased(data)
        assert e.value.kind == "NotImplemented" and "not planned" in str(e.value)
