"""Writes tests/golden/vorbis_host_hashes.json: per named stream of tests/vorbis_streams.py (and the
real libvorbis file) the SHA-256 of the host decoder's samples with the sample rate, or its error
text.  Run once against a build of the commit before the Vorbis core was split out of the host
decoder (SDSP_LIB_PATH names that build's libstratum_hip.so); tests/test_vorbis_host_unchanged.py
recomputes the hashes with the current build.

    SDSP_LIB_PATH=/path/to/old/libstratum_hip.so python tests/golden/make_vorbis_hashes.py
"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "stratum-dsp_amd", "python"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

import vorbis_streams as vs  # noqa: E402

LIB_PATH = os.environ.get("SDSP_LIB_PATH") or os.path.join(ROOT, "stratum-dsp_amd", "lib", "libstratum_hip.so")
_lib = None


def _decode(path):
    """sdsp_decode_audio_file through a binding of its own (an older build lacks the newer exports
    the package's binding declares)."""
    global _lib
    if _lib is None:
        _lib = C.CDLL(LIB_PATH)
        _lib.sdsp_decode_audio_file.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint64),
                                                C.POINTER(C.c_uint32), C.c_char_p, C.c_uint64]
        _lib.sdsp_decode_audio_file.restype = C.c_int32
        _lib.sdsp_free_samples.argtypes = [C.POINTER(C.c_float)]
        _lib.sdsp_free_samples.restype = None
    p, n, sr, err = C.POINTER(C.c_float)(), C.c_uint64(), C.c_uint32(), C.create_string_buffer(512)
    st = _lib.sdsp_decode_audio_file(os.fsencode(path), C.byref(p), C.byref(n), C.byref(sr), err, 512)
    if st != 0:
        return None, "Decoding error: " + err.value.decode(errors="replace")
    try:
        x = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.float32)
    finally:
        _lib.sdsp_free_samples(p)
    return x, sr.value


def named():
    real = open(os.path.join(HERE, "real_libvorbis_keypress.ogg"), "rb").read()
    return vs.all_named() + [("real_libvorbis_keypress", real)]


def digest(blob, tmpdir):
    path = os.path.join(tmpdir, "t.ogg")
    with open(path, "wb") as f:
        f.write(blob)
    x, sr = _decode(path)
    if x is None:
        return "error: " + sr
    return f"{sr} {len(x)} " + hashlib.sha256(x.tobytes()).hexdigest()


def hashes():
    with tempfile.TemporaryDirectory() as d:
        return {name: digest(blob, d) for name, blob in named()}


if __name__ == "__main__":
    with open(os.path.join(HERE, "vorbis_host_hashes.json"), "w") as f:
        json.dump(hashes(), f, indent=0, sort_keys=True)
        f.write("\n")
