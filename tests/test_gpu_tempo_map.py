"""The tempo map request on the GPU (sdsp_analyze_batch_device_with, sdsp_debug_tempo_map;
k_tempo_map.hip) against tests/tempo_map_ref.py, which tests/test_tempo_map_ref.py pins to the oracle.

Stage probe: every case of tests/beat_cases.py in one ragged launch, every field of every map
compared bit for bit (floats on their uint32 views), the onsets echoed, the beat lists unchanged by
the request.  Full pipeline: the golden WAVs and seeded click tracks, of which the oracle's trace
says which are refined; the results equal the call's without the request, the map equals the
reference fed with the returned onsets and tempo, and the published beats equal the list that
reference reconstructs.  No tolerance anywhere.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import beat_cases as B
import oracle
import parity
import sdsp
import sdsp_abi
import tempo_map_ref as R
from test_gpu_overview import assert_same_results

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = list(B.cases())
ALONE = ("gate_bpm_0", "seg_lt4_hmm_beats", "seg_span_lt_2s", "var_bpm_120", "sort_gt_64", "hmm_frames_2049")
_PROBE = {}


def probe():
    """Every named case in one call with the request, and the same call without it (shared)."""
    if not _PROBE:
        tracks = [B.cases()[k][0] for k in NAMES]
        _PROBE["maps"], _PROBE["grids"] = sdsp.debug_tempo_map(tracks, sample_rate=B.SR)
        _PROBE["plain"] = sdsp.debug_beat_grid(tracks, B.SR)
    return _PROBE


def _ref(name):
    t = B.cases()[name][0]
    return R.reference(t["onsets"], t["bpm"], t["conf"], B.SR)


def _canon(m):
    return json.dumps(m, default=lambda a: R.bits(a).tolist() if isinstance(a, (np.ndarray, np.floating)) else repr(a))


def _same_grid(a, b):
    return (a["ok"] == b["ok"] and all(np.array_equal(R.bits(a[k]), R.bits(b[k])) for k in ("beats", "downbeats")) and
            R.bits(a["stability"]) == R.bits(b["stability"]))


# ---- stage probe ----
@pytest.mark.parametrize("name", NAMES)
def test_case_against_reference(name):
    k = NAMES.index(name)
    got, ref, trk = probe()["maps"][k], _ref(name), B.cases()[name][0]
    assert got["status"] == 0 and got["first_sample"] == 0, name
    bad = R.differences(got, ref)
    assert not bad, (name, bad, {f: (got.get(f), ref.get(f)) for f in bad if "." not in f})
    assert np.array_equal(got["onsets"], trk["onsets"]) and got["n_onsets"] == trk["onsets"].size, name
    grid = probe()["grids"][k]
    assert grid["ok"] == ref["has_grid"], name
    assert np.array_equal(R.bits(grid["beats"]), R.bits(ref["beats"])), name
    if got["refined"]:
        assert int(got["segments"]["n_beats"].sum()) == grid["beats"].size, name


def test_request_leaves_the_beats_alone():
    p = probe()
    for k, name in enumerate(NAMES):
        assert _same_grid(p["grids"][k], p["plain"][k]), name


def test_cases_alone_equal_the_ragged_launch():
    p = probe()
    for name in ALONE:
        maps, grids = sdsp.debug_tempo_map([B.cases()[name][0]], sample_rate=B.SR)
        k = NAMES.index(name)
        assert _canon(maps[0]) == _canon(p["maps"][k]), name
        assert _same_grid(grids[0], p["grids"][k]), name


def test_what_bits_select_the_lists():
    name = "var_bpm_120"
    k, trk = NAMES.index(name), B.cases()[name][0]
    full = probe()["maps"][k]
    seg = sdsp.debug_tempo_map([trk], what=("segments",), sample_rate=B.SR)[0][0]
    ons = sdsp.debug_tempo_map([trk], what=("onsets",), sample_rate=B.SR)[0][0]
    assert seg["n_onsets"] == 0 and seg["onsets"].size == 0 and _canon(seg["segments"]) == _canon(full["segments"])
    assert ons["n_segments"] == 0 and np.array_equal(ons["onsets"], trk["onsets"])
    assert not R.differences(seg, _ref(name)) and not R.differences(ons, _ref(name), segments=False)
    for what in (0, 4, 7):
        with pytest.raises(sdsp.AnalysisError) as e:
            sdsp.debug_tempo_map([trk], what=what, sample_rate=B.SR)
        assert e.value.code == 1


# ---- full pipeline ----
SR = 44100
CLICKS = [(120, 40, s) for s in (0, 1, 2, 3)] + [(100, 32, s) for s in (1, 2, 3)] + [(120, 40, None)]
_FULL = {}


def click_track(bpm, slots, seed, sr=SR):
    """Exponentially decaying 1 kHz bursts at slot k * 60 / bpm, each kept with probability 0.6
    (seed None: every slot), about 20 s."""
    n = int((slots * 60.0 / bpm + 1.0) * sr)
    x = np.zeros(n, np.float32)
    keep = np.ones(slots, bool) if seed is None else np.random.default_rng(seed).random(slots) < 0.6
    t = np.arange(int(0.05 * sr)) / sr
    burst = (0.8 * np.exp(-t / 0.01) * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)
    for k in np.flatnonzero(keep):
        at = int(round(k * 60.0 / bpm * sr))
        x[at:at + burst.size] += burst[:max(0, min(burst.size, n - at))]
    return x


class Batch:
    def __init__(self, tracks, first=1):
        self.tracks = [np.ascontiguousarray(t, np.float32) for t in tracks]
        self.lens = np.array([t.size for t in self.tracks], np.uint64)
        self.offs = (first + np.concatenate([[0], np.cumsum(self.lens)[:-1]])).astype(np.uint64)
        total = first + int(self.lens.sum())
        host = np.zeros(total + 8, np.float32)
        for o, t in zip(self.offs, self.tracks):
            host[int(o):int(o) + t.size] = t
        self.buf = sdsp.DeviceBuffer(total + 8)
        self.buf.from_host(host)

    def plain(self, cfg, stages=sdsp.STAGES_FULL):
        return sdsp.analyze_batch_device(self.buf.ptr, self.offs, self.lens, SR, cfg, stages=stages)

    def call(self, cfg, **req):
        out = sdsp.analyze_batch_device_with(self.buf.ptr, self.offs, self.lens, SR, cfg, **req)
        res = [out[0][i] for i in range(len(out[0]))]
        out[0].free()
        return (res,) + tuple(out[1:])


def full():
    """The golden WAVs and the click tracks: the oracle's traces (CPU) first, then one call with the
    request and one without."""
    if not _FULL:
        xs = []
        for name in sorted(os.listdir(GOLDEN)):
            if name.endswith(".wav"):
                x, sr = parity.load_wav(os.path.join(GOLDEN, name))
                assert sr == SR, name
                xs.append(x)
        xs += [click_track(*c) for c in CLICKS]
        cfg = oracle.default_config()
        traces = []
        for x in xs:
            out = oracle.analyze(x, SR, cfg, trace=True)
            traces.append((out[0], out[-1]))
        refined = [st == 0 and bool(tr["beat_refined"]) for st, tr in traces]
        assert any(refined) and not all(refined), refined  # (before the GPU is touched)
        b = Batch(xs)
        plain = b.plain(sdsp.default_config())
        res, _, _, _, maps = b.call(sdsp.default_config(), tempo_map=sdsp.tempo_map_request())
        _FULL.update(batch=b, traces=traces, plain=plain, res=res, maps=maps, refined=refined)
    return _FULL


def test_results_unchanged_by_the_request():
    f = full()
    assert_same_results(f["res"], f["plain"])


def test_maps_against_oracle_trace_and_reference():
    f = full()
    assert sum(f["refined"]) >= 3
    for i, (m, r, (st, tr)) in enumerate(zip(f["maps"], f["res"], f["traces"])):
        assert not isinstance(r, sdsp.AnalysisError) and st == 0 and m["status"] == 0, i
        assert (m["has_variation"], m["refined"], m["beats_per_bar"]) == (tr["beat_variable"], tr["beat_refined"],
                                                                          tr["beats_per_bar"]), i
        assert R.bits(m["nominal_bpm"]) == R.bits(r["bpm"]) and R.bits(m["nominal_confidence"]) == R.bits(r["bpm_confidence"]), i
        assert m["n_onsets"] == m["onsets"].size and m["n_onsets"] >= 2 and np.all(np.diff(m["onsets"].astype(np.int64)) > 0), i
        ref = R.reference(m["onsets"], m["nominal_bpm"], m["nominal_confidence"], SR)
        bad = R.differences(m, ref)
        assert not bad, (i, bad)
        beats = np.array(r["beat_grid"]["beats"], np.float32)
        assert np.array_equal(R.bits(beats), R.bits(ref["beats"])), i
        if m["refined"]:
            assert int(m["segments"]["n_beats"].sum()) == beats.size, i


# ---- combined requests and refusals ----
def test_all_four_requests_in_one_call():
    xs = full()["batch"].tracks[4:6]
    b, cfg = Batch(xs, first=3), sdsp.default_config()
    reqs = dict(overview=sdsp.overview_request(columns=32),
                key_timeline=sdsp.key_timeline_request(segment_seconds=4.0, overlap_seconds=1.0),
                levels=sdsp.levels_request(15), tempo_map=sdsp.tempo_map_request())
    plain = b.plain(cfg)
    res, ovs, kts, lvs, tms = b.call(cfg, **reqs)
    assert_same_results(res, plain)
    assert len(tms) == 2 and all(m["status"] == 0 and m["has_grid"] for m in tms)
    names = ("overview", "key_timeline", "levels", "tempo_map")
    for k, name in enumerate(names):
        out = b.call(cfg, **{name: reqs[name]})
        assert_same_results(out[0], plain)
        one = out[1 + k]
        assert _canon(one) == _canon((ovs, kts, lvs, tms)[k]), name
    t = sdsp.tempo_map_times()
    assert t["tracks"] == 2 and t["map_ms"] > 0.0
    b.call(cfg, levels=reqs["levels"])
    assert sdsp.tempo_map_times()["tracks"] == 0  # nothing ran for the map in the last call


def _raw_call(b, cfg, rs, stages=0, device=0):
    n = len(b.tracks)
    outs = (sdsp_abi.SdspResult * n)()
    u64p = C.POINTER(C.c_uint64)
    st = sdsp.lib().sdsp_analyze_batch_device_with(C.c_void_p(b.buf.ptr), b.offs.ctypes.data_as(u64p), b.lens.ctypes.data_as(u64p),
                                                   n, SR, C.byref(cfg), device, None, stages, outs, C.byref(rs))
    msgs = [outs[i].error_message.decode() for i in range(n)]
    stats = [outs[i].status for i in range(n)]
    for i in range(n):
        sdsp.lib().sdsp_result_free(C.byref(outs[i]))
    return st, stats, msgs


def test_refused_requests():
    rng = np.random.default_rng(5)
    b, cfg = Batch([rng.normal(0, 0.1, 20000).astype(np.float32) for _ in range(2)]), sdsp.default_config()
    n = 2

    def rset(what, with_array=True, size=None):
        rs = sdsp_abi.SdspRequestSet()
        rs.struct_size = C.sizeof(rs) if size is None else size
        req = sdsp_abi.SdspTempoMapRequest(what)
        tms = (sdsp_abi.SdspTempoMap * n)()
        for i in range(n):
            tms[i].status = 77
        rs.tm_req = C.pointer(req)
        if with_array:
            rs.tempo_maps = tms
        return rs, tms, req

    for device in (0, 1 << 20):  # an invalid device index still reports the validation error
        for what in (0, 4, 1 | 8, 0x80000000):
            rs, tms, _keep = rset(what)
            st, stats, msgs = _raw_call(b, cfg, rs, device=device)
            assert st == 1 and stats == [1, 1] and all("tempo map request" in t for t in msgs), (what, st, msgs)
            assert [tms[i].status for i in range(n)] == [1, 1] and tms[0].n_onsets == 0
        rs, tms, _keep = rset(3, with_array=False)
        st, stats, msgs = _raw_call(b, cfg, rs, device=device)
        assert st == 1 and stats == [1, 1] and "without a tempo map array" in msgs[0]
        rs, tms, _keep = rset(3)
        st, stats, msgs = _raw_call(b, cfg, rs, stages=sdsp.STAGES_BPM_ONLY, device=device)
        assert st == 1 and stats == [1, 1] and "SDSP_STAGES_BPM_ONLY" in msgs[0] and tms[1].status == 1
    # a caller built against the header before this request: its struct ends before the pair
    rs, tms, _keep = rset(0, size=sdsp_abi.SdspRequestSet.tm_req.offset)
    st, stats, _ = _raw_call(b, cfg, rs)
    assert st == 0 and tms[0].status == 77
    with pytest.raises(sdsp.AnalysisError) as e:
        b.call(cfg, tempo_map=sdsp.tempo_map_request(0))
    assert e.value.kind == "InvalidInput"
