"""Per-track overview envelopes on the GPU (sdsp_analyze_batch_device_overview, k_overview.hip)
against tests/overview_ref.py, numpy over the oracle's own normalised signal and spectrogram.

Every value is a minimum or a maximum, so all five arrays and all scalar fields are compared for
equality, bit for bit.  The sdsp_results of a call with a request are compared with the plain
entry's, field for field (processing_time_ms, a wall clock, aside).  Tracks sit in the device buffer
at offsets 1, 2, 3, 0 (mod 4) floats, so the 16-byte-aligned body of a hop segment and its
unaligned head and tail are all read.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
import overview_ref
import parity
import sdsp
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "stratum-dsp_amd", "bin")
WAVS = ("120bpm_4bar.wav", "128bpm_4bar.wav", "cmajor_scale.wav", "mixed_silence.wav")
SR = 44100


def _cfgs(**opts):
    c, o = sdsp.default_config(), oracle.default_config()
    for k, v in opts.items():
        setattr(c, k, v)
        setattr(o, k, v)
    return c, o


class Batch:
    """Host tracks packed into one device buffer at offsets that cycle through 1, 2, 3, 0 mod 4."""

    def __init__(self, tracks):
        self.tracks = [np.ascontiguousarray(t, np.float32) for t in tracks]
        offs, cur = [], 1
        for i, t in enumerate(self.tracks):
            cur += (1 + i - cur) % 4
            offs.append(cur)
            cur += t.size
        self.offs = np.array(offs, np.uint64)
        self.lens = np.array([t.size for t in self.tracks], np.uint64)
        self.buf = sdsp.DeviceBuffer(cur + 8)
        host = np.zeros(cur + 8, np.float32)
        for o, t in zip(offs, self.tracks):
            host[o:o + t.size] = t
        self.buf.from_host(host)

    def plain(self, cfg, sr=SR, stages=sdsp.STAGES_FULL):
        return sdsp.analyze_batch_device(self.buf.ptr, self.offs, self.lens, sr, cfg, stages=stages)

    def overview(self, cfg, request, sr=SR, stages=sdsp.STAGES_FULL):
        batch, ovs = sdsp.analyze_batch_device_overview(self.buf.ptr, self.offs, self.lens, sr, cfg, stages=stages,
                                                        request=request)
        res = [batch[i] for i in range(len(batch))]
        batch.free()
        return res, ovs


def _plainify(r):
    if isinstance(r, sdsp.AnalysisError):
        return ("error", r.code, str(r))
    d = json.loads(json.dumps(r))
    d["metadata"].pop("processing_time_ms", None)
    return d


def assert_same_results(got, want):
    """Two result lists of the engine, field for field and bit for bit (no tolerance anywhere)."""
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert _plainify(a) == _plainify(b), (i, a, b)
        if not isinstance(a, sdsp.AnalysisError):
            assert parity.exact_fraction(a, b, strict=True) == 1.0 and not parity.diff_results(a, b), i


def _status(r):
    return r.code if isinstance(r, sdsp.AnalysisError) else 0


def check(batch, cfg, ocfg, chains, kw, sr=SR, stages=sdsp.STAGES_FULL, plain=None, what=""):
    """One call with the request `kw`: every track's overview equals the reference's, its status the
    result's, and the results equal `plain` (the plain entry's, when given)."""
    res, ovs = batch.overview(cfg, sdsp.overview_request(**kw), sr=sr, stages=stages)
    assert len(ovs) == len(batch.tracks)
    for i, x in enumerate(batch.tracks):
        want = overview_ref.overview_ref(x, sr, ocfg, chain=chains[i], **kw)
        overview_ref.assert_equal(ovs[i], want, (what, kw, i))
        assert ovs[i]["status"] == _status(res[i]), (what, kw, i)
    if plain is not None:
        assert_same_results(res, plain)
    return res, ovs


def _chains(tracks, ocfg, sr=SR):
    return [overview_ref.signal_and_mags(x, sr, ocfg) for x in tracks]


# ---- fixtures and synthetic tracks: three request forms, both stage modes ----
_MAIN = {}


def _main():
    if not _MAIN:
        xs = [parity.load_wav(os.path.join(GOLDEN, n))[0] for n in WAVS]
        xs += [synth.make_track(7100 + k, seconds=20.0)[0] for k in range(4)]
        cfg, ocfg = _cfgs()
        b = Batch(xs)
        _MAIN.update(batch=b, cfg=cfg, ocfg=ocfg, chains=_chains(xs, ocfg),
                     plain={m: b.plain(cfg, stages=m) for m in (sdsp.STAGES_FULL, sdsp.STAGES_BPM_ONLY)})
    return _MAIN


@pytest.mark.parametrize("stages", [sdsp.STAGES_FULL, sdsp.STAGES_BPM_ONLY], ids=["full", "bpm_only"])
@pytest.mark.parametrize("kw", [dict(columns=256), dict(frames_per_column=1), dict(frames_per_column=7)],
                         ids=["columns256", "frames1", "frames7"])
def test_fixtures_and_synthetic_tracks(kw, stages):
    m = _main()
    _, ovs = check(m["batch"], m["cfg"], m["ocfg"], m["chains"], kw, stages=stages, plain=m["plain"][stages])
    assert all(o["status"] == 0 and o["n_columns"] > 0 for o in ovs)
    F = m["chains"][4][3].shape[0]  # a 20-s track: some 1,700 frames
    assert F > 1500 and ovs[4]["n_frames"] == F
    assert ovs[4]["n_columns"] == (256 if "columns" in kw else -(-F // kw["frames_per_column"]))


# ---- frame-count edges, one ragged batch with an empty and an all-zero track ----
EDGE_N = [2047, 2048, 2559, 2560] + [(F - 1) * 512 + 2048 + tail for F, tail in ((63, 0), (64, 17), (65, 0), (257, 301))]
EDGE_REQ = ([dict(columns=c) for c in (1, 3, 64, 100000)] + [dict(frames_per_column=k) for k in (1, 3, 64, 100000)])
_EDGE = {}


def _edge():
    if not _EDGE:
        src = synth.make_track(7200, seconds=4.0)[0]
        xs = [src[5 + 3 * k:5 + 3 * k + n].copy() for k, n in enumerate(EDGE_N)]
        xs.insert(3, np.zeros(0, np.float32))
        xs.append(np.zeros(5000, np.float32))
        cfg, ocfg = _cfgs(enable_silence_trimming=0)
        b = Batch(xs)
        _EDGE.update(batch=b, cfg=cfg, ocfg=ocfg, chains=_chains(xs, ocfg), plain=b.plain(cfg))
    return _EDGE


@pytest.mark.parametrize("kw", EDGE_REQ, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_frame_count_edges(kw):
    e = _edge()
    res, ovs = check(e["batch"], e["cfg"], e["ocfg"], e["chains"], kw, plain=e["plain"])
    lens = [int(n) for n in e["batch"].lens]
    frames = [o["n_frames"] for o in ovs]
    assert frames == [0 if n < 2048 else (n - 2048) // 512 + 1 for n in lens]
    assert frames[0] == 0 and frames[1] == 1 and frames[2] == 1 and frames[4] == 2 and frames[5:9] == [63, 64, 65, 257]
    # the empty track is an error with zero columns; a track shorter than a frame is no error
    assert isinstance(res[3], sdsp.AnalysisError) and ovs[3]["status"] == res[3].code != 0 and ovs[3]["n_columns"] == 0
    assert ovs[3]["n_samples"] == 0 and ovs[3]["frame_size"] == 2048 and ovs[3]["hop_size"] == 512
    assert ovs[0]["status"] == 0 and ovs[0]["n_columns"] == 0 and ovs[0]["n_samples"] == 2047
    assert ovs[2]["n_samples"] == 2559  # F = 1: the one column holds all 2559 samples, 511 past the hop
    for o in ovs:
        assert o["first_sample"] == 0  # trimming is off


# ---- band edges ----
BANDS = {
    "low_empty": (dict(low_max_hz=0.0, mid_max_hz=4000.0), [0, 185]),
    "high_empty_at_nyquist_plus": (dict(low_max_hz=250.0, mid_max_hz=30000.0), [11, 1025]),
    "last_bin_alone_in_high": (dict(low_max_hz=250.0, mid_max_hz=22050.0), [11, 1024]),
    "edge_on_a_bin_mid_one_bin_wide": (dict(low_max_hz=21.533203125, mid_max_hz=43.06640625), [1, 2]),
    "mid_empty": (dict(low_max_hz=4000.0, mid_max_hz=4000.0), [185, 185]),
    "all_low": (dict(low_max_hz=1e9, mid_max_hz=1e9), [1025, 1025]),
}


@pytest.mark.parametrize("case", sorted(BANDS))
def test_band_edges(case):
    m = _main()
    edges, bins = BANDS[case]
    _, ovs = check(m["batch"], m["cfg"], m["ocfg"], m["chains"], dict(frames_per_column=7, **edges))
    for o in ovs:
        assert o["band_bins"] == bins
        if bins[0] == 0:
            assert not o["low"].any()
        if bins[0] == bins[1]:
            assert not o["mid"].any()
        if bins[1] == 1025:
            assert not o["high"].any()
    if case == "last_bin_alone_in_high":  # bin B - 1 and nothing else
        mags = m["chains"][4][3]
        assert np.array_equal(ovs[4]["high"], np.maximum.reduceat(mags[:, 1024], np.arange(0, mags.shape[0], 7)))


# ---- other shapes of the pass ----
SHAPES = {
    "fs1024_hop441": dict(frame_size=1024, hop_size=441),
    "fs4096": dict(frame_size=4096),
    "rms": dict(normalization=1),
    "no_normalization": dict(enable_normalization=0),
}


@pytest.mark.parametrize("case", sorted(SHAPES))
def test_other_pass_shapes(case):
    """Trimming is on throughout: the silence-padded track has first_sample > 0, the all-zero track
    is silent after trimming and keeps that status with zero columns."""
    cfg, ocfg = _cfgs(**SHAPES[case])
    xs = [synth.make_track(7300, seconds=8.0, silence_pad=0.7)[0], synth.make_track(7301, seconds=6.0)[0] * np.float32(0.3),
          np.zeros(30000, np.float32)]
    b = Batch(xs)
    chains = _chains(xs, ocfg)
    plain = b.plain(cfg)
    for kw in (dict(columns=100), dict(frames_per_column=5)):
        res, ovs = check(b, cfg, ocfg, chains, kw, plain=plain, what=case)
        assert ovs[0]["first_sample"] > 0 and ovs[0]["n_samples"] < xs[0].size and ovs[0]["n_columns"] > 0
        assert ovs[0]["frame_size"] == int(cfg.frame_size) and ovs[0]["hop_size"] == int(cfg.hop_size)
        assert isinstance(res[2], sdsp.AnalysisError) and ovs[2]["status"] == res[2].code == 3 and ovs[2]["n_columns"] == 0


def test_sample_rate_other_than_44100():
    cfg, ocfg = _cfgs()
    xs = [synth.make_track(7400, seconds=8.0, sr=22050)[0]]
    b = Batch(xs)
    _, ovs = check(b, cfg, ocfg, _chains(xs, ocfg, sr=22050), dict(columns=50), sr=22050, plain=b.plain(cfg, sr=22050))
    assert ovs[0]["band_bins"] == [23, 371]


# ---- sub-batches ----
def test_sub_batches_give_the_same_overviews(monkeypatch):
    """Eight ragged tracks of about two minutes as one sub-batch and, under a 1 GB budget, as at
    least three: overviews and results equal; two tracks also against the reference."""
    n, L = 8, 135 * SR
    lens = np.array([(100 + 5 * k) * SR + 11 * k for k in range(n)], np.uint64)
    offs = np.array([k * L + (k + 1) % 4 for k in range(n)], np.uint64)
    buf = sdsp.DeviceBuffer(n * L + 8)
    sdsp.generate_synthetic(buf.ptr, n, L, seed0=7500)
    cfg, ocfg = _cfgs()
    req = sdsp.overview_request(columns=300)

    def run():
        batch, ovs = sdsp.analyze_batch_device_overview(buf.ptr, offs, lens, SR, cfg, request=req)
        res = [batch[i] for i in range(n)]
        batch.free()
        return res, ovs, sdsp.overview_times()

    monkeypatch.delenv("SDSP_HBM_BUDGET_GB", raising=False)
    one = run()
    monkeypatch.setenv("SDSP_HBM_BUDGET_GB", "1")
    split = run()
    monkeypatch.delenv("SDSP_HBM_BUDGET_GB", raising=False)
    assert one[2]["sub_batches"] == 1 and split[2]["sub_batches"] >= 3, (one[2], split[2])
    assert one[2]["columns"] == split[2]["columns"] == 300 * n
    assert_same_results(split[0], one[0])
    for i in range(n):
        overview_ref.assert_equal(split[1][i], one[1][i], i)
        assert one[1][i]["status"] == 0 and one[1][i]["n_columns"] == 300
    for i in (0, 5):
        x = buf.to_host(int(offs[i]), int(lens[i]))
        overview_ref.assert_equal(one[1][i], overview_ref.overview_ref(x, SR, ocfg, columns=300), i)


# ---- escalation ----
def test_escalated_tracks_keep_the_base_pass_overview():
    """Two tracks from config 5's BPM mix (176 and 184 BPM) escalate to the hop-256 / hop-1024
    passes; the overview is still the hop-512 pass's."""
    xs = [synth.make_track(503, seconds=20.0, bpm=176.0)[0], synth.make_track(504, seconds=20.0, bpm=184.0)[0]]
    cfg, ocfg = _cfgs()
    b = Batch(xs)
    plain = b.plain(cfg)
    assert all(r["metadata"]["tempogram_multi_res_triggered"] is True for r in plain), plain
    chains = _chains(xs, ocfg)
    for kw in (dict(columns=256), dict(frames_per_column=1)):
        _, ovs = check(b, cfg, ocfg, chains, kw, plain=plain)
        assert all(o["hop_size"] == 512 and o["n_frames"] == c[3].shape[0] > 1500 for o, c in zip(ovs, chains))


# ---- no request; allocations ----
def _alloc_stats():
    f = sdsp.lib().sdsp_debug_alloc_stats
    f.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    n, b = C.c_uint64(), C.c_uint64()
    assert f(C.byref(n), C.byref(b)) == 0
    return n.value, b.value


def test_no_request_is_the_plain_entry_and_repeats_allocate_nothing():
    m = _main()
    b, cfg = m["batch"], m["cfg"]
    for stages in (sdsp.STAGES_FULL, sdsp.STAGES_BPM_ONLY):
        res, ovs = b.overview(cfg, None, stages=stages)
        assert ovs == []
        assert_same_results(res, m["plain"][stages])
    t = sdsp.overview_times()
    assert t["sub_batches"] == 0 and t["columns"] == 0 and t["sample_ms"] == 0.0  # nothing ran for an overview
    a0 = _alloc_stats()
    res, _ = b.overview(cfg, None)
    assert_same_results(res, m["plain"][sdsp.STAGES_FULL])
    assert _alloc_stats() == a0
    for kw in (dict(columns=1), dict(frames_per_column=1)):  # the longest columns (pieces), the most columns
        req = sdsp.overview_request(**kw)
        first = b.overview(cfg, req)
        a1 = _alloc_stats()
        for _ in range(2):
            again = b.overview(cfg, req)
            for x, y in zip(again[1], first[1]):
                overview_ref.assert_equal(x, y, kw)
        assert _alloc_stats() == a1, kw
        t = sdsp.overview_times()
        assert t["sub_batches"] == 1 and t["sample_ms"] > 0.0 and t["band_ms"] > 0.0
        assert t["sample_bytes"] == 4.0 * sum(o["n_samples"] for o in first[1])
        assert t["band_bytes"] == 4.0 * 1025 * sum(o["n_frames"] for o in first[1])


# ---- CLI ----
def _rows(out):
    rows = []
    for ln in out.stdout.splitlines():
        r = json.loads(ln)
        r.pop("processing_time_ms", None)
        rows.append(r)
    return rows


def test_cli_overview_member():
    names = ("120bpm_4bar.wav", "mixed_silence.wav")
    paths = [os.path.join(GOLDEN, n) for n in names]
    base = [os.path.join(BIN, "analyze_batch"), "--json", "--jobs", "2", "--devices", "1"]
    plain = subprocess.run(base + paths, capture_output=True, text=True, timeout=300)
    ov = subprocess.run(base + ["--overview", "64"] + paths, capture_output=True, text=True, timeout=300)
    gd = subprocess.run(base + ["--overview", "64", "--gpu-decode"] + paths, capture_output=True, text=True, timeout=300)
    fr = subprocess.run(base + ["--overview-frames", "9"] + paths, capture_output=True, text=True, timeout=300)
    for p in (plain, ov, gd, fr):
        assert p.returncode == 0, p.stderr
    a, b, c, d = _rows(plain), _rows(ov), _rows(gd), _rows(fr)
    assert len(a) == len(b) == len(c) == len(d) == 2
    xs = [sdsp.decode_audio_file(p)[0] for p in paths]
    bt = Batch(xs)
    cfg = sdsp.default_config()
    for rows, kw in ((b, dict(columns=64)), (c, dict(columns=64)), (d, dict(frames_per_column=9))):
        _, lib_ovs = bt.overview(cfg, sdsp.overview_request(**kw))
        for i, r in enumerate(rows):
            assert list(r)[-1] == "overview"  # the last member of the object
            o = r.pop("overview")
            assert r == a[i], (kw, i)  # the rest of the line is the run without the flag
            got = dict(o, **{k: np.array(o[k], np.float64).astype(np.float32) for k in overview_ref.ARRAYS})
            overview_ref.assert_equal(got, lib_ovs[i], (kw, i))
            assert o["n_columns"] == len(o["smin"]) > 0
    assert all("overview" not in r for r in a)
    bad = subprocess.run(base + ["--overview", "4", "--overview-frames", "2"] + paths, capture_output=True, text=True)
    assert bad.returncode == 1 and "exclude each other" in bad.stderr
