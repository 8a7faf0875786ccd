"""analyze_batch --gpu-decode on the GPU: native FLAC files are decoded by the device decoder and
analysed from the device buffer; the JSONL must equal the run without the flag, line for line,
once processing_time_ms (wall clock) is removed."""
import json
import os
import subprocess

import numpy as np
import pytest

import flac_enc as fe
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "stratum-dsp_amd", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _flac(seed, seconds, sr, stereo=False):
    x, _, _, _ = synth.make_track(seed, seconds=seconds, sr=sr)
    pcm = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int64)
    chans = [pcm, pcm // 2] if stereo else [pcm]
    frames = [fe.frame([c[o:o + 4096] for c in chans], 16, k, assign="mid_side" if stereo else "indep",
                       specs=[{"type": "fixed", "order": 2}] * len(chans))
              for k, o in enumerate(range(0, pcm.size, 4096))]
    return fe.stream(frames, sr, len(chans), 16, total=pcm.size)


def _rows(out):
    rows = []
    for ln in out.stdout.splitlines():
        r = json.loads(ln)
        r.pop("processing_time_ms", None)
        rows.append(json.dumps(r, sort_keys=False))
    return rows


def test_gpu_decode_gives_the_same_jsonl(tmp_path):
    files = {"a.flac": _flac(1, 4.0, 44100), "b.flac": _flac(2, 4.0, 22050), "c.flac": _flac(3, 3.0, 44100, stereo=True),
             "broken.flac": b"fLaC\x00\x00\x00\x22" + bytes(10)}
    paths = []
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    paths.insert(2, os.path.join(GOLDEN, "120bpm_4bar.wav"))
    base = [os.path.join(BIN, "analyze_batch"), "--json", "--jobs", "3", "--devices", "1"]
    plain = subprocess.run(base + paths, capture_output=True, text=True, timeout=300)
    gpu = subprocess.run(base + ["--gpu-decode"] + paths, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and gpu.returncode == 0, (plain.stderr, gpu.stderr)
    a, b = _rows(plain), _rows(gpu)
    assert len(a) == len(paths) and a == b
    ok = [json.loads(r) for r in a]
    assert [r["file"] for r in ok] == paths
    assert sum("bpm" in r for r in ok) == 4 and ok[-1]["error"].startswith("decode failed: truncated FLAC metadata")
    assert "Done: ok=4/5" in gpu.stderr
