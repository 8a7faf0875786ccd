"""The key timeline on the GPU (sdsp_analyze_batch_device_requests, sdsp_debug_key_timeline,
k_key_timeline.hip) against tests/key_timeline_ref.py: the oracle's detect_key and key clarity over
each segment of the oracle's own chroma rows, the plan, primary key and changes from the definition.

Everything is compared for equality, floats on their uint32 view: the kernel folds each score in
the reference's order and the decision is the reference's arithmetic, so there is no tolerance
anywhere.  The sdsp_results of a call with a request are compared with the plain entry's, field
for field (processing_time_ms, a wall clock, aside).
"""
import json
import os
import subprocess

import numpy as np
import pytest

import key_timeline_ref as K
import oracle
import overview_ref
import parity
import sdsp
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "stratum-dsp_amd", "bin")
SR = 44100
f32 = np.float32


def _cfgs(**opts):
    c, o = sdsp.default_config(), oracle.default_config()
    for k, v in opts.items():
        setattr(c, k, v)
        setattr(o, k, v)
    return c, o


def _plainify(r):
    if isinstance(r, sdsp.AnalysisError):
        return ("error", r.code, str(r))
    d = json.loads(json.dumps(r))
    d["metadata"].pop("processing_time_ms", None)
    return d


def assert_same_results(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert _plainify(a) == _plainify(b), (i, a, b)
        if not isinstance(a, sdsp.AnalysisError):
            assert parity.exact_fraction(a, b, strict=True) == 1.0 and not parity.diff_results(a, b), i


class Batch:
    """Host tracks packed into one device buffer at offsets that cycle through 1, 2, 3, 0 mod 4."""

    def __init__(self, tracks):
        self.tracks = [np.ascontiguousarray(t, f32) for t in tracks]
        offs, cur = [], 1
        for i, t in enumerate(self.tracks):
            cur += (1 + i - cur) % 4
            offs.append(cur)
            cur += t.size
        self.offs = np.array(offs, np.uint64)
        self.lens = np.array([t.size for t in self.tracks], np.uint64)
        self.buf = sdsp.DeviceBuffer(cur + 8)
        host = np.zeros(cur + 8, f32)
        for o, t in zip(offs, self.tracks):
            host[o:o + t.size] = t
        self.buf.from_host(host)

    def plain(self, cfg, stages=sdsp.STAGES_FULL):
        return sdsp.analyze_batch_device(self.buf.ptr, self.offs, self.lens, SR, cfg, stages=stages)

    def run(self, cfg, overview=None, key_timeline=None, stages=sdsp.STAGES_FULL):
        batch, ovs, kts = sdsp.analyze_batch_device_requests(self.buf.ptr, self.offs, self.lens, SR, cfg, stages=stages,
                                                             overview=overview, key_timeline=key_timeline)
        res = [batch[i] for i in range(len(batch))]
        batch.free()
        return res, ovs, kts


def check(batch, cfg, ocfg, chains, req, plain=None, what=""):
    res, _, kts = batch.run(cfg, key_timeline=sdsp.key_timeline_request(**req))
    assert len(kts) == len(batch.tracks)
    for i, x in enumerate(batch.tracks):
        want = K.timeline_ref(x, SR, ocfg, req, chain=chains[i])
        K.assert_equal(kts[i], want, (what, req, i))
        assert kts[i]["status"] == (res[i].code if isinstance(res[i], sdsp.AnalysisError) else 0), (what, i)
    if plain is not None:
        assert_same_results(res, plain)
    return res, kts


# ---- small shapes through the debug entry ----
SMALL_F = [1, 2, 5, 6, 63, 64, 65, 300]
SMALL_REQ = [(1, 1), (2, 1), (5, 5), (64, 64), (64, 1), (65, 3)] + [(F, F) for F in SMALL_F] + [(F + 1, 1) for F in SMALL_F]
SMALL_REQ = sorted(set(SMALL_REQ))
_SMALL = {}


def _small_tracks():
    """Random non-negative rows (an HPCP row's scale), a few all-zero rows, and one all-zero track:
    a segment of zero rows has both maxima <= 1e-9, the normalisation guard's other branch."""
    if not _SMALL:
        rng = np.random.default_rng(9100)
        rows = [(rng.random((F, 12), dtype=f32) ** 2).astype(f32) for F in SMALL_F]
        rows[4][10:13] = 0.0  # F = 63: three zero rows (whole zero segments at L <= 2, mixed ones above)
        rows[7][100:170] = 0.0  # F = 300: 70 zero rows (whole zero segments at L = 64, 65)
        rows[3][2] = 0.0
        rows.append(np.zeros((7, 12), f32))
        _SMALL["rows"] = rows
        _SMALL["ref"] = {}
    return _SMALL["rows"]


def _small_ref(t, L, H, minconf):
    rows = _small_tracks()
    key = (t, L, H, minconf)
    if key not in _SMALL["ref"]:
        _SMALL["ref"][key] = K.timeline(rows[t], L, H, SR, 512, minconf)
    return _SMALL["ref"][key]


def _small_check(got, t, L, H, minconf):
    want = dict(_small_ref(t, L, H, minconf), status=0, first_sample=0, segment_frames=L, hop_frames=H, frame_size=8192,
                hop_size=512)
    K.assert_equal(got, want, (t, L, H))


@pytest.mark.parametrize("L,H", SMALL_REQ, ids=lambda v: str(v))
def test_small_shapes_one_ragged_call(L, H):
    rows = _small_tracks()
    got = sdsp.debug_key_timeline(rows, sdsp.key_timeline_request(segment_frames=L, hop_frames=H), SR)
    assert len(got) == len(rows)
    for t in range(len(rows)):
        _small_check(got[t], t, L, H, -1.0)
        F = rows[t].shape[0]
        assert got[t]["n_frames"] == F and got[t]["n_segments"] == (0 if F < L else (F - L) // H + 1)
    z = got[-1]  # the all-zero track: scores 0, confidence 0, key 0 (the stable sort keeps key order)
    if z["n_segments"]:
        assert not z["segments"]["confidence"].any() and not z["segments"]["top_scores"].any()
        assert not z["segments"]["clarity"].any() and z["segments"]["top_keys"].tolist() == [[0, 1, 2]] * z["n_segments"]


def test_small_shapes_single_track_calls_equal_the_ragged_call():
    rows = _small_tracks()
    for L, H in ((1, 1), (64, 1), (65, 3), (5, 5)):
        req = sdsp.key_timeline_request(segment_frames=L, hop_frames=H)
        ragged = sdsp.debug_key_timeline(rows, req, SR)
        for t in range(len(rows)):
            one = sdsp.debug_key_timeline([rows[t]], req, SR)
            K.assert_equal(one[0], ragged[t], (t, L, H))
    # and in another order with an empty track between: the segment prefix has a zero-length entry
    order = [7, 8, 0, 4]
    req = sdsp.key_timeline_request(segment_frames=64, hop_frames=1)
    got = sdsp.debug_key_timeline([rows[t] for t in order[:2]] + [np.zeros((0, 12), f32)] + [rows[t] for t in order[2:]],
                                  req, SR)
    assert got[2]["n_frames"] == 0 and got[2]["n_segments"] == 0 and got[2]["primary_key"] == -1
    for g, t in zip(got[:2] + got[3:], order):
        _small_check(g, t, 64, 1, -1.0)


def test_small_shapes_threshold_and_seconds_form():
    rows = _small_tracks()
    # the random rows give confidences 0 (both modes score): the reference's 0.2 reports nothing,
    # 0.0 nothing (strict), a negative threshold every change
    for minconf in (0.2, 0.0, -0.5):
        got = sdsp.debug_key_timeline(rows, sdsp.key_timeline_request(segment_frames=5, hop_frames=5,
                                                                      min_change_confidence=minconf), SR)
        for t in range(len(rows)):
            _small_check(got[t], t, 5, 5, minconf)
        assert (got[7]["n_changes"] > 0) == (minconf < 0)
    got = sdsp.debug_key_timeline(rows, sdsp.key_timeline_request(segment_seconds=0.75, overlap_seconds=0.25), SR)
    L, H = K.plan(dict(segment_seconds=0.75, overlap_seconds=0.25), SR, 512)
    assert (L, H) == (64, 43)
    for t in range(len(rows)):
        _small_check(got[t], t, L, H, -1.0)


# ---- end to end ----
REQ_SECONDS = dict(segment_seconds=4.0, overlap_seconds=1.0)  # 344 frames every 258
REQ_FRAMES = dict(segment_frames=100, hop_frames=37)
_MAIN = {}


def _main():
    if not _MAIN:
        dev = sdsp.DeviceBuffer(15 * SR)
        sdsp.generate_synthetic(dev.ptr, 1, 15 * SR, seed0=9200)
        rng = np.random.default_rng(9201)
        xs = [K.modulating_track(8.0),
              dev.to_host(0, 15 * SR),
              (rng.standard_normal(12 * SR) * 0.1).astype(f32),
              parity.load_wav(os.path.join(GOLDEN, "cmajor_scale.wav"))[0],
              synth.make_track(9202, seconds=3.0)[0],  # 243 key frames: fewer than the seconds form's 344
              synth.make_track(9203, seconds=13.0)[0]]
        cfg, ocfg = _cfgs()
        b = Batch(xs)
        _MAIN.update(batch=b, cfg=cfg, ocfg=ocfg, chains=[K.chroma_rows(x, SR, ocfg) for x in xs], plain=b.plain(cfg))
    return _MAIN


@pytest.mark.parametrize("req", [REQ_SECONDS, REQ_FRAMES], ids=["seconds_4_1", "frames_100_37"])
def test_end_to_end(req):
    m = _main()
    _, kts = check(m["batch"], m["cfg"], m["ocfg"], m["chains"], req, plain=m["plain"])
    assert all(t["status"] == 0 and t["frame_size"] == 8192 and t["hop_size"] == 512 for t in kts)
    assert [t["n_frames"] for t in kts] == [c[2].shape[0] for c in m["chains"]]
    if req is REQ_SECONDS:
        assert kts[0]["segments"]["key"].tolist() == [0, 0, 6, 6] and kts[0]["changes"]["segment"].tolist() == [2]
        assert kts[0]["primary_key"] == 0 and kts[0]["primary_count"] == 2
        assert kts[4]["n_frames"] == 243 and kts[4]["n_segments"] == 0 and kts[4]["primary_key"] == -1
    else:
        assert kts[4]["n_segments"] == (243 - 100) // 37 + 1
    # (the 4-s scale has 329 key frames: no 344-frame segment either, and three of 100)
    assert [t["n_segments"] > 0 for t in kts] == [True, True, True, req is REQ_FRAMES, req is REQ_FRAMES, True]


def test_reference_threshold_and_short_and_failed_tracks():
    """min_change_confidence = 0.2 (the reference's constant) next to tracks whose key path is
    skipped (shorter than the key frame) and that fail (empty, silent)."""
    xs = [K.modulating_track(8.0)[:12 * SR], synth.make_track(9204, seconds=1.0)[0][:8000], np.zeros(0, f32),
          np.zeros(30000, f32)]
    cfg, ocfg = _cfgs()
    b = Batch(xs)
    chains = [K.chroma_rows(x, SR, ocfg) for x in xs]
    req = dict(REQ_SECONDS, min_change_confidence=0.2)
    res, kts = check(b, cfg, ocfg, chains, req, plain=b.plain(cfg))
    assert kts[0]["n_segments"] > 1 and kts[0]["n_changes"] == 0
    assert kts[1]["status"] == 0 and kts[1]["n_frames"] == 0 and kts[1]["n_segments"] == 0 and kts[1]["primary_key"] == -1
    for i in (2, 3):
        assert isinstance(res[i], sdsp.AnalysisError) and kts[i]["status"] == res[i].code != 0
        assert kts[i]["n_segments"] == 0 and kts[i]["n_frames"] == 0 and kts[i]["segment_frames"] == 344


# ---- other key paths ----
PATHS = {
    "override_off": dict(enable_key_stft_override=0),
    "non_band_kernels": dict(key_spectrogram_smooth_margin=8),
    "edge_trim": dict(enable_key_edge_trim=1),
}


@pytest.mark.parametrize("case", sorted(PATHS))
def test_other_key_paths(case):
    cfg, ocfg = _cfgs(**PATHS[case])
    xs = [K.modulating_track(6.0), synth.make_track(9300, seconds=12.0)[0]]
    b = Batch(xs)
    chains = [K.chroma_rows(x, SR, ocfg) for x in xs]
    plain = b.plain(cfg)
    for req in (REQ_SECONDS, REQ_FRAMES):
        _, kts = check(b, cfg, ocfg, chains, req, plain=plain, what=case)
        kfs, khop = K.key_stft(ocfg)
        assert all(t["frame_size"] == kfs and t["hop_size"] == khop and t["n_segments"] > 0 for t in kts)
    if case == "edge_trim":  # 12 s are more than 200 frames, so the vote trims; the timeline does not
        assert kts[1]["n_frames"] == chains[1][2].shape[0] >= 200
        assert int(kts[1]["segments"]["start_frame"][0]) == 0


# ---- sub-batches, the late join, near-decision tracks ----
def test_sub_batches_and_join_order_give_the_same_timelines(monkeypatch):
    """40 tracks of 20 s as one sub-batch, under a 1 GB budget as at least three (every join but the
    last one late, across sub-batch boundaries), and with the join at each sub-batch's end:
    timelines and results equal.  Tracks whose vote was near a decision (rerun exactly) and two
    fixed tracks also against the reference."""
    n, L = 40, 20 * SR + 37 * 40
    lens = np.array([20 * SR + 37 * k for k in range(n)], np.uint64)
    offs = np.array([k * L + (k + 1) % 4 for k in range(n)], np.uint64)
    buf = sdsp.DeviceBuffer(n * L + 8)
    sdsp.generate_synthetic(buf.ptr, n, L, seed0=9400, bpm_mode=1)
    cfg, ocfg = _cfgs()
    req = sdsp.key_timeline_request(**REQ_SECONDS)

    def run():
        batch, _, kts = sdsp.analyze_batch_device_requests(buf.ptr, offs, lens, SR, cfg, key_timeline=req)
        res = [batch[i] for i in range(n)]
        batch.free()
        return res, kts, sdsp.stage_times()["stft8192_launches"], sdsp.last_key_near(n).copy()

    for k in ("SDSP_HBM_BUDGET_GB", "SDSP_NO_KEY_DEFER", "SDSP_SERIAL_STREAMS", "SDSP_NO_ROW_REUSE"):
        monkeypatch.delenv(k, raising=False)
    one = run()
    monkeypatch.setenv("SDSP_HBM_BUDGET_GB", "1")
    split = run()
    monkeypatch.setenv("SDSP_NO_KEY_DEFER", "1")
    early = run()
    monkeypatch.delenv("SDSP_NO_KEY_DEFER", raising=False)
    monkeypatch.delenv("SDSP_HBM_BUDGET_GB", raising=False)
    plain = sdsp.analyze_batch_device(buf.ptr, offs, lens, SR, cfg)
    assert one[2] == 1 and split[2] >= 3 and early[2] >= 3, (one[2], split[2], early[2])
    assert_same_results(one[0], plain)
    for other in (split, early):
        assert_same_results(other[0], one[0])
        for i in range(n):
            K.assert_equal(other[1][i], one[1][i], i)
    assert all(t["status"] == 0 and t["n_segments"] == (t["n_frames"] - 344) // 258 + 1 > 4 for t in one[1])
    near = [int(i) for i in np.nonzero(one[3])[0]][:2]
    for i in sorted(set(near + [0, n - 1])):
        x = buf.to_host(int(offs[i]), int(lens[i]))
        K.assert_equal(one[1][i], K.timeline_ref(x, SR, ocfg, REQ_SECONDS), ("reference", i, i in near))


# ---- no request; both requests ----
def test_no_request_is_the_plain_entry_and_both_requests_share_one_analysis():
    m = _main()
    b, cfg = m["batch"], m["cfg"]
    res, ovs, kts = b.run(cfg)
    assert ovs == [] and kts == []
    assert_same_results(res, m["plain"])
    oreq, kreq = sdsp.overview_request(columns=64), sdsp.key_timeline_request(**REQ_SECONDS)
    both = b.run(cfg, overview=oreq, key_timeline=kreq)
    only_ov = b.run(cfg, overview=oreq)
    only_kt = b.run(cfg, key_timeline=kreq)
    old = sdsp.analyze_batch_device_overview(b.buf.ptr, b.offs, b.lens, SR, cfg, request=oreq)
    old[0].free()
    assert only_ov[2] == [] and only_kt[1] == [] and len(both[1]) == len(both[2]) == len(b.tracks)
    for r in (both, only_ov, only_kt):
        assert_same_results(r[0], m["plain"])
    for i in range(len(b.tracks)):
        overview_ref.assert_equal(both[1][i], only_ov[1][i], i)
        overview_ref.assert_equal(both[1][i], old[1][i], i)
        K.assert_equal(both[2][i], only_kt[2][i], i)


# ---- rejections ----
def test_rejections_on_a_device():
    m = _main()
    b = m["batch"]
    kreq = sdsp.key_timeline_request(**REQ_SECONDS)
    with pytest.raises(sdsp.AnalysisError) as e:
        b.run(m["cfg"], key_timeline=kreq, stages=sdsp.STAGES_BPM_ONLY)
    assert e.value.code == 1 and "SDSP_STAGES_BPM_ONLY" in str(e.value)
    cfg, _ = _cfgs(enable_key_beat_synchronous=1)
    with pytest.raises(sdsp.AnalysisError) as e:
        b.run(cfg, key_timeline=kreq)
    assert e.value.code == 4 and "beat-synchronous" in str(e.value)
    # log-frequency chroma rows are frames again: the request runs
    cfg, _ = _cfgs(enable_key_beat_synchronous=1, enable_key_log_frequency=1)
    _, _, kts = b.run(cfg, key_timeline=kreq)
    assert kts[0]["status"] == 0 and kts[0]["n_segments"] == 4
    # an overview alone still runs with BPM only
    res, ovs, _ = b.run(m["cfg"], overview=sdsp.overview_request(columns=8), stages=sdsp.STAGES_BPM_ONLY)
    assert ovs[0]["n_columns"] == 8


# ---- CLI ----
def _rows(out):
    rows = []
    for ln in out.stdout.splitlines():
        r = json.loads(ln)
        r.pop("processing_time_ms", None)
        rows.append(r)
    return rows


def _from_json(o):
    seg = {k: np.array([s[k] for s in o["segments"]], np.float64) for k in K.SEGMENT_FIELDS}
    chg = {k: np.array([c[k] for c in o["changes"]], np.float64) for k in K.CHANGE_FIELDS}
    dts = dict(start_frame=np.uint64, key=np.int32, top_keys=np.int32, segment=np.uint64, from_key=np.int32, to_key=np.int32)
    S = len(o["segments"])
    seg = {k: v.astype(dts.get(k, f32)).reshape((S, 3) if k.startswith("top_") else (S,)) for k, v in seg.items()}
    chg = {k: v.astype(dts.get(k, f32)) for k, v in chg.items()}
    return dict(o, segments=seg, changes=chg, primary_confidence=f32(o["primary_confidence"]))


KEY_NAMES = [n + m for m in ("", "m") for n in ("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B")]


def test_cli_key_timeline_member():
    names = ("cmajor_scale.wav", "120bpm_4bar.wav")
    paths = [os.path.join(GOLDEN, n) for n in names]
    base = [os.path.join(BIN, "analyze_batch"), "--json", "--jobs", "2", "--devices", "1"]
    runs = {k: subprocess.run(base + extra + paths, capture_output=True, text=True, timeout=300)
            for k, extra in (("plain", []), ("kt", ["--key-timeline", "4"]),
                             ("gd", ["--key-timeline", "4:1:-1", "--gpu-decode"]),
                             ("both", ["--key-timeline", "2:0.5:0.2", "--overview", "16"]))}
    for p in runs.values():
        assert p.returncode == 0, p.stderr
    rows = {k: _rows(p) for k, p in runs.items()}
    xs = [sdsp.decode_audio_file(p)[0] for p in paths]
    bt = Batch(xs)
    cfg = sdsp.default_config()
    for k, req in (("kt", REQ_SECONDS), ("gd", REQ_SECONDS),
                   ("both", dict(segment_seconds=2.0, overlap_seconds=0.5, min_change_confidence=0.2))):
        _, _, lib_kts = bt.run(cfg, key_timeline=sdsp.key_timeline_request(**req))
        for i, r in enumerate(rows[k]):
            assert list(r)[-1] == "key_timeline"
            o = r.pop("key_timeline")
            if k == "both":
                assert r.pop("overview")["n_columns"] == 16
            assert r == rows["plain"][i], (k, i)
            K.assert_equal(_from_json(o), lib_kts[i], (k, i))
            assert o["n_segments"] == len(o["segments"]) and o["n_changes"] == len(o["changes"])
            for g in o["segments"]:
                assert g["key_name"] == KEY_NAMES[g["key"]]
            for c in o["changes"]:
                assert (c["from_key_name"], c["to_key_name"]) == (KEY_NAMES[c["from_key"]], KEY_NAMES[c["to_key"]])
            assert o["primary_key_name"] == (KEY_NAMES[o["primary_key"]] if o["n_segments"] else "")
        assert sum(r_["n_segments"] for r_ in lib_kts) > 0
    assert all("key_timeline" not in r for r in rows["plain"])
    bad = subprocess.run(base + ["--key-timeline", "0"] + paths, capture_output=True, text=True)
    assert bad.returncode == 1 and "--key-timeline requires" in bad.stderr
