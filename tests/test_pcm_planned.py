"""The device PCM path's steps on the CPU (sdsp_debug_pcm_decode_planned: the host plan of a
RIFF/WAVE or AIFF file, then csrc/pcm_core.hpp over the planned frames) against the host decoder
(sdsp_decode_audio_file) and against the conversion written out in numpy.  Files come from
tests/pcm_streams.py.  Every comparison is np.array_equal on the uint32 view: no tolerance.  No GPU.
"""
import numpy as np
import pytest

import pcm_streams as ps
import sdsp


def _host(tmp_path, data):
    p = tmp_path / "t.bin"
    p.write_bytes(data)
    return sdsp.decode_audio_file(str(p))


def _same(tmp_path, data):
    want, sr = _host(tmp_path, data)
    got, sr2, info = sdsp.debug_pcm_decode_planned(data)
    assert sr2 == sr and got.size == want.size == info[3]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return want, info


@pytest.mark.parametrize("name,data", ps.matrix(), ids=[n for n, _ in ps.matrix()])
def test_matrix(tmp_path, name, data):
    want, info = _same(tmp_path, data)
    assert want.size > 0


@pytest.mark.parametrize("name,data", ps.edges(), ids=[n for n, _ in ps.edges()])
def test_edges(tmp_path, name, data):
    want, info = _same(tmp_path, data)
    if "frames" in name and name[-1].isdigit():
        assert want.size == int(name.split("frames")[1])


def test_data_offsets_cover_every_alignment():
    offs = {sdsp.debug_pcm_decode_planned(d)[2][2] % 4 for n, d in ps.edges() if "_off" in n or "odd_chunk" in n}
    assert offs == {0, 1, 2, 3}


def test_overstated_chunks_are_clipped_to_the_file(tmp_path):
    by = dict(ps.edges())
    assert _same(tmp_path, by["wav_data_longer_than_file"])[0].size == 200
    assert _same(tmp_path, by["wav_data_cut_in_a_frame"])[0].size == 199
    assert _same(tmp_path, by["aiff_ssnd_longer_than_file"])[0].size == 100


@pytest.mark.parametrize("kind", ps.KINDS)
def test_conversion_values(kind):
    """The conversion itself, against numpy: (v - 128) / 128, / 2^(bits - 1), f32 as is, f64 -> f32;
    two channels summed from -0.0 in order and divided by the count."""
    v = ps.samples(kind, 2 * 64, 11)
    tag = 3 if kind in ("f32", "f64") else 1
    got, sr, info = sdsp.debug_pcm_decode_planned(ps.wav(tag, 8 * ps.WIDTH[kind], 2, ps.pack(kind, v, False), rate=32000))
    if kind == "u8":
        f = (v.astype(np.float32) - np.float32(128)) / np.float32(128)
    elif kind in ("f32", "f64"):
        f = v.astype(np.float32)
    else:
        f = v.astype(np.float32) / np.float32(2.0 ** (8 * ps.WIDTH[kind] - 1))
    want = ((np.float32(-0.0) + f[0::2]) + f[1::2]) / np.float32(2)
    assert sr == 32000 and info[1] == 2 and info[0] == ps.KINDS.index(kind)
    assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))


def test_float_specials_pass_through(tmp_path):
    """Mono f32 is copied bit for bit (NaN payloads, signalling NaNs, infinities, -0.0, denormals);
    an f64 that rounds to an f32 denormal gives that denormal."""
    by = dict(ps.edges())
    for name in ("wav_f32_specials_mono", "aifc_fl32_specials_mono"):
        got, _, _ = sdsp.debug_pcm_decode_planned(by[name])
        bits = got.view(np.uint32)
        assert bits[1] == 0x7FC12345 and bits[4] == 0xFFABCDEF and bits[7] == 0x80000000 and bits[8] == 1
    got, _, _ = sdsp.debug_pcm_decode_planned(by["wav_f64_to_denormals_mono"])
    bits = got.view(np.uint32)
    assert bits[2] == 1 and bits[3] == 0 and bits[4] == 1 and bits[8] == 0x7F800000 and bits[11] == 0x80000000
    assert 0 < bits[0] < 0x00800000  # 1e-40: a denormal


@pytest.mark.parametrize("name,data", ps.not_linear(), ids=[n for n, _ in ps.not_linear()])
def test_g711_and_adpcm_are_not_planned(tmp_path, name, data):
    want, sr = _host(tmp_path, data)  # the host decoder reads them
    assert want.size > 0
    with pytest.raises(sdsp.AnalysisError) as e:
        sdsp.debug_pcm_decode_planned(data)
    assert e.value.kind == "NotImplemented" and "not planned" in str(e.value)


@pytest.mark.parametrize("name,data", ps.refused(), ids=[n for n, _ in ps.refused()])
def test_refused_files_carry_the_hosts_text(tmp_path, name, data):
    with pytest.raises(sdsp.AnalysisError) as want:
        _host(tmp_path, data)
    with pytest.raises(sdsp.AnalysisError) as got:
        sdsp.debug_pcm_decode_planned(data)
    assert got.value.code == want.value.code and str(got.value) == str(want.value)
