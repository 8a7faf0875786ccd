"""analyze_batch --gpu-decode over a mixed folder on the GPU: ALAC in M4A (two rates) and CAF, a
24-bit WAV, an AIFF and a FLAC decoded by kernels, an Ogg Vorbis file by the host decoder inside the
same call, and a broken M4A; the JSONL must equal the run without the flag, line for line, once
processing_time_ms (wall clock) is removed."""
import json
import os
import subprocess

import numpy as np
import pytest

import alac_enc as ae
import alac_streams as als
import flac_enc as fe
import pcm_streams as ps
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "stratum-dsp_amd", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _pcm16(seed, seconds, sr):
    x, _, _, _ = synth.make_track(seed, seconds=seconds, sr=sr)
    return np.ascontiguousarray(x, np.float32), np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int64)


def _alac(pcm, sr, caf=False):
    cfg = ae.Config(bit_depth=16, channels=1, frame_length=4096, sample_rate=sr)
    pk = als.packets(cfg, [pcm], [{"ch": [{"na31": True}]}])
    return ae.caf(cfg, pk, pcm.size) if caf else ae.mp4(cfg, pk, [1] * len(pk))


def _rows(out):
    rows = []
    for ln in out.stdout.splitlines():
        r = json.loads(ln)
        r.pop("processing_time_ms", None)
        rows.append(json.dumps(r, sort_keys=False))
    return rows


def test_gpu_decode_gives_the_same_jsonl_for_a_mixed_folder(tmp_path):
    x1, p1 = _pcm16(1, 3.0, 44100)
    x2, p2 = _pcm16(2, 3.0, 48000)
    x3, p3 = _pcm16(3, 3.0, 44100)
    flac = fe.stream([fe.frame([p3[o:o + 4096]], 16, k, specs=[{"type": "fixed", "order": 2}])
                      for k, o in enumerate(range(0, p3.size, 4096))], 44100, 1, 16, total=p3.size)
    good = ae.mp4(ae.Config(), [b"\x00" * 10], [1])
    files = {"a.m4a": _alac(p1, 44100), "b.m4a": _alac(p2, 48000), "c.caf": _alac(p3, 44100, caf=True),
             "d.wav": ps.passage_wav24(x2, 48000),
             "e.aiff": ps.aiff(16, 1, p1.size, ps.pack("s16", p1, True), rate=44100), "f.flac": flac,
             "broken.m4a": good[:len(good) // 2]}
    paths = []
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    paths.insert(5, os.path.join(GOLDEN, "real_libvorbis_keypress.ogg"))
    base = [os.path.join(BIN, "analyze_batch"), "--json", "--jobs", "3", "--devices", "1"]
    plain = subprocess.run(base + paths, capture_output=True, text=True, timeout=300)
    gpu = subprocess.run(base + ["--gpu-decode"] + paths, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and gpu.returncode == 0, (plain.stderr, gpu.stderr)
    a, b = _rows(plain), _rows(gpu)
    assert len(a) == len(paths) and a == b
    ok = [json.loads(r) for r in a]
    assert [r["file"] for r in ok] == paths
    assert sum("bpm" in r for r in ok) >= 6 and ok[-1]["error"].startswith("decode failed: ")
