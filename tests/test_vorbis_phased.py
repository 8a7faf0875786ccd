"""The device Vorbis decoder's phases on the CPU (sdsp_debug_vorbis_decode_phased: the host plan,
every packet's spectra, every (packet, channel) windowed block, every output sample from its packet
pair, through csrc/vorbis_core.hpp with the kernels' buffer layouts) equal the host decoder
(sdsp_decode_audio_file) bit for bit: samples as uint32, lengths, rates, status and error texts."""
import os

import numpy as np
import pytest

import sdsp
import vorbis_streams as vs

REAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_libvorbis_keypress.ogg")


def host(tmp_path, blob):
    p = tmp_path / "t.ogg"
    p.write_bytes(blob)
    try:
        return sdsp.decode_audio_file(str(p)), None
    except sdsp.AnalysisError as e:
        return None, (e.kind, str(e))


def same(tmp_path, blob):
    want, werr = host(tmp_path, blob)
    try:
        x, sr, info = sdsp.debug_vorbis_decode_phased(blob)
    except sdsp.AnalysisError as e:
        if e.kind == "NotImplemented":  # the first page was lost: not a Vorbis stream any more, the host decoder's file
            assert "not planned" in str(e) and werr == ("DecodingError", "Decoding error: unsupported Ogg stream")
        else:
            assert werr == (e.kind, str(e))
        return None
    assert werr is None
    assert sr == want[1] and x.shape == want[0].shape
    assert np.array_equal(x.view(np.uint32), want[0].view(np.uint32))
    return x, info


def test_generated_streams_are_accepted_finite_and_reach_the_paths(tmp_path):
    names = [n for n, _ in vs.matrix()]
    assert len(set(names)) == len(names)
    zeroed = 0
    for name, blob in vs.matrix():
        (x, sr), err = host(tmp_path, blob)
        assert err is None, (name, err)
        assert np.all(np.isfinite(x)), name
        if "single_packet" not in name:
            assert len(x) > 0 and np.any(x != 0), name
        zeroed += sdsp.debug_vorbis_decode_phased(blob)[2][1]
    assert zeroed >= 2  # the packets cut inside the floor
    big = dict(vs.matrix())["mono_64_short_150"]
    assert sdsp.debug_vorbis_decode_phased(big)[2][0] == 150  # more than one wave of packets
    # the skipped packets (empty, not audio, mode out of range) are dropped by the plan
    assert sdsp.debug_vorbis_decode_phased(dict(vs.matrix())["stereo_256_2048_r1_packets"])[2][0] == 12
    # the page that fails its CRC takes its packet with it
    assert sdsp.debug_vorbis_decode_phased(dict(vs.matrix())["stereo_256_2048_r0_pages"])[2][0] == 10


@pytest.mark.parametrize("name", [n for n, _ in vs.SPECS])
def test_phased_equals_host_on_the_matrix(tmp_path, name):
    assert same(tmp_path, dict(vs.matrix())[name]) is not None


def test_phased_equals_host_on_the_damaged_variants(tmp_path):
    decoded = errors = 0
    for name, blob in vs.damaged():
        if same(tmp_path, blob) is None:
            errors += 1
        else:
            decoded += 1
    assert decoded > 0 and errors > 0


def test_phased_equals_host_on_the_real_libvorbis_file(tmp_path):
    x, info = same(tmp_path, open(REAL, "rb").read())
    assert len(x) > 0 and info[0] > 0 and info[1] == 0


def test_phased_equals_host_on_the_encoder_streams(tmp_path):
    for name, blob in vs.encoder_streams():
        assert same(tmp_path, blob) is not None, name


def test_other_bytes_are_not_planned():
    with pytest.raises(sdsp.AnalysisError) as e:
        sdsp.debug_vorbis_decode_phased(b"RIFF" + bytes(40))
    assert e.value.kind == "NotImplemented" and "not planned" in str(e.value)
