"""analyze_batch --fingerprint: a WAV and its FLAC encoding (tests/flac_enc.py) come out as one
duplicate pair on the last line, each file's "fingerprint" member is what the binding returns for the
same audio, and without the flag the lines are what they were."""
import json
import os
import subprocess
import wave

import numpy as np
import pytest

import fingerprint_ref as R
import flac_enc as fe
import sdsp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "stratum-dsp_amd", "bin")
PLAIN_KEYS = ["file", "bpm", "bpm_confidence", "key", "key_confidence", "processing_time_ms", "tempogram_multi_res_triggered",
              "tempogram_multi_res_used", "tempogram_percussive_triggered", "tempogram_percussive_used"]
SR = 44100
f32 = np.float32


def _pcm(x):
    return np.clip(np.round(x.astype(np.float64) * 32767.0), -32768, 32767).astype(np.int64)


def _write_wav(path, pcm):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(SR)
        w.writeframes(pcm.astype("<i2").tobytes())


def _flac(pcm):
    frames = [fe.frame([pcm[o:o + 4096]], 16, k, specs=[{"type": "fixed", "order": 2}])
              for k, o in enumerate(range(0, pcm.size, 4096))]
    return fe.stream(frames, SR, 1, 16, total=pcm.size)


def _lines(out):
    rows = []
    for ln in out.stdout.splitlines():
        r = json.loads(ln)
        r.pop("processing_time_ms", None)
        rows.append(r)
    return rows


def test_cli_duplicates_line_for_a_wav_and_its_flac_encoding(tmp_path):
    a, b = _pcm(R.random_triads(1, 12.0)), _pcm(R.random_triads(2, 12.0))
    _write_wav(tmp_path / "a.wav", a)
    (tmp_path / "a_copy.flac").write_bytes(_flac(a))
    _write_wav(tmp_path / "b.wav", b)
    (tmp_path / "a_late.flac").write_bytes(_flac(a[5512:]))
    paths = [str(tmp_path / n) for n in ("a.wav", "b.wav", "a_copy.flac", "a_late.flac")]
    base = [os.path.join(BIN, "analyze_batch"), "--json", "--jobs", "2", "--devices", "1"]
    plain = subprocess.run(base + paths, capture_output=True, text=True, timeout=300)
    full = subprocess.run(base + ["--fingerprint"] + paths, capture_output=True, text=True, timeout=300)
    dev = subprocess.run(base + ["--fingerprint=0.125:2:0.3", "--gpu-decode"] + paths, capture_output=True, text=True,
                         timeout=300)
    for p in (plain, full, dev):
        assert p.returncode == 0, p.stderr
    for arg in ("--fingerprint=0", "--fingerprint=0.125:40", "--fingerprint=0.125:2:1.5", "--fingerprint=0.125:2:0.3:1",
                "--fingerprint=x"):
        bad = subprocess.run(base + [arg, paths[0]], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 1 and "--fingerprint takes" in bad.stderr, arg
    # without the flag: the plain lines, nothing more
    pl = _lines(plain)
    assert len(pl) == len(paths) and all(list(json.loads(ln)) == PLAIN_KEYS for ln in plain.stdout.splitlines())
    assert '"fingerprint":' not in plain.stdout and '{"duplicates"' not in plain.stdout
    for run in (full, dev):
        rows = _lines(run)
        assert len(rows) == len(paths) + 1 and list(rows[-1]) == ["duplicates"]
        dups = rows[-1]["duplicates"]
        assert [(d["a"], d["b"]) for d in dups] == [(paths[0], paths[2]), (paths[0], paths[3]), (paths[2], paths[3])], dups
        assert dups[0]["offset_seconds"] == 0 and dups[0]["ber"] == 0
        for d in dups[1:]:
            assert abs(d["offset_seconds"] + 5512 / SR) < 1e-8 and 0 < d["ber"] < 0.05, d  # (printed to 9 digits)
        for r, want in zip(rows[:-1], pl):
            assert list(r)[-1] == "fingerprint"
            fp = r.pop("fingerprint")
            assert r == want
            assert fp["status"] == 0 and fp["cell_samples"] == 5512 and len(fp["words"]) == 6 * fp["n_words"] > 0
        assert [r["fingerprint"]["n_matches"] for r in _lines(run)[:-1]] == [2, 0, 2, 2]
    # the words are the binding's for the same audio
    xs = [sdsp.decode_audio_file(p)[0] for p in paths]
    lens = np.array([x.size for x in xs], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    buf = sdsp.DeviceBuffer(int(lens.sum()) + 8)
    buf.from_host(np.concatenate([np.ascontiguousarray(x, f32) for x in xs] + [np.zeros(8, f32)]))
    out = sdsp.analyze_batch_device_with(buf.ptr, offs, lens, SR, sdsp.default_config(),
                                         fingerprint=sdsp.fingerprint_request(cell_seconds=0.125, max_offset_words=16))
    out[0].free()
    for r, want in zip(_lines(full)[:-1], out[-1]["fingerprints"]):
        fp = r["fingerprint"]
        assert fp["words"] == "".join("%06x" % int(w) for w in want["words"])
        assert {k: fp[k] for k in ("n_cells", "n_words", "first_sample", "n_matches")} == \
            {k: want[k] for k in ("n_cells", "n_words", "first_sample", "n_matches")}
    m = out[-1]["matches"]["matches"]
    assert list(zip(m["a"].tolist(), m["b"].tolist(), m["offset_words"].tolist())) == [(0, 2, 0), (0, 3, -1), (2, 3, -1)]
