"""The sections request on the GPU (sdsp_analyze_batch_device_with, sdsp_debug_sections,
k_sections.hip) against tests/sections_ref.py: the definition in numpy f32 over the oracle's own
chroma rows and spectrogram.

Everything is compared for equality, floats on their uint32 view: the kernels fold every sum in the
definition's order, so there is no tolerance anywhere.  The sdsp_results of a call with a request are
compared with the plain entry's, field for field (processing_time_ms, a wall clock, aside).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import key_timeline_ref as K
import oracle
import parity
import sdsp
import sdsp_abi
import sections_cases as SC
import sections_ref as S
import synth
from test_sections_ref import BEHAVIOURAL_REQUEST, behavioural_track

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SR = 44100
f32 = np.float32


# ---- small shapes through the debug entry ----
@pytest.mark.parametrize("layout", sorted(SC.LAYOUTS))
@pytest.mark.parametrize("K_", SC.KS)
def test_small_shapes_one_ragged_call(layout, K_):
    """Cell counts 0, 1, 2K-1, 2K, 2K+1, 63, 64, 65, 130, 300 with zero rows, gmax = 0 and a plateau of
    equal N, all tracks of a layout in one call, at G = 0, 1, 8."""
    khop, hop, _ = SC.LAYOUTS[layout]
    tr, ref = SC.tracks(layout, K_), SC.reference(layout, K_)
    for G in SC.GS:
        got = sdsp.debug_sections([t[0] for t in tr], [t[1] for t in tr], sdsp.sections_request(**SC.request(layout, K_, G)),
                                  SR, khop, hop)
        bnd = SC.boundaries(layout, K_, G)
        assert len(got) == len(tr)
        for t, (g, c) in enumerate(zip(got, ref)):
            what = (layout, K_, G, tr[t][2])
            assert g["n_cells"] == c["n_cells"], what
            S.assert_arrays_equal(g["m"], c["m"], what + ("m",))
            S.assert_arrays_equal(g["g"], c["g"], what + ("g",))
            S.assert_arrays_equal(g["novelty"], c["novelty"], what + ("N",))
            assert np.array_equal(g["boundary"], bnd[t]), (what, np.flatnonzero(g["boundary"]), np.flatnonzero(bnd[t]))
    assert sum(int(b.sum()) for b in SC.boundaries(layout, K_, 1)) > 0


def test_small_shapes_single_track_calls_equal_the_ragged_call():
    layout, K_ = "uneven_43_44", 2
    khop, hop, _ = SC.LAYOUTS[layout]
    tr = SC.tracks(layout, K_)
    req = sdsp.sections_request(**SC.request(layout, K_, 8))
    ragged = sdsp.debug_sections([t[0] for t in tr], [t[1] for t in tr], req, SR, khop, hop)
    for t in (0, 1, 4, 7, 9, len(tr) - 1):
        one = sdsp.debug_sections([tr[t][0]], [tr[t][1]], req, SR, khop, hop)[0]
        for k in ("m", "g", "novelty", "boundary"):
            S.assert_arrays_equal(one[k], ragged[t][k], (t, k))


def test_debug_entry_refuses_a_bad_request():
    rows, E = np.zeros((10, 12), f32), np.zeros(10, f32)
    for bad in (dict(cell_samples=511), dict(cell_samples=512, kernel_cells=65), dict(cell_samples=512, what=0)):
        with pytest.raises(sdsp.AnalysisError) as e:
            sdsp.debug_sections([rows], [E], sdsp.sections_request(**bad), SR)
        assert e.value.code == 1


# ---- end to end ----
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

    def run(self, cfg, stages=sdsp.STAGES_FULL, **requests):
        out = sdsp.analyze_batch_device_with(self.buf.ptr, self.offs, self.lens, SR, cfg, stages=stages, **requests)
        res = [out[0][i] for i in range(len(out[0]))]
        out[0].free()
        return (res,) + tuple(out[1:])


def _downs(r):
    return [] if isinstance(r, sdsp.AnalysisError) else r["beat_grid"]["downbeats"]


def check(batch, cfg, ocfg, chains, req, plain=None, what=""):
    out = batch.run(cfg, sections=sdsp.sections_request(**req))
    res, secs = out[0], out[-1]
    assert len(secs) == len(batch.tracks)
    for i, x in enumerate(batch.tracks):
        want = S.sections_ref(x, SR, ocfg, req, downs=_downs(res[i]), chain=chains[i])
        S.assert_equal(secs[i], want, (what, req, i))
        assert secs[i]["status"] == (res[i].code if isinstance(res[i], sdsp.AnalysisError) else 0), (what, i)
    if plain is not None:
        assert_same_results(res, plain)
    return res, secs


def _assert_same_dict(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        if isinstance(a[k], dict):
            _assert_same_dict(a[k], b[k], (what, k))
        elif isinstance(a[k], np.ndarray):
            S.assert_arrays_equal(a[k], b[k], (what, k))
        else:
            assert S._bits(a[k]) == S._bits(b[k]) if isinstance(a[k], np.floating) else a[k] == b[k], (what, k)


_MAIN = {}


def _main():
    if not _MAIN:
        xs = [behavioural_track(), parity.load_wav(os.path.join(GOLDEN, "120bpm_4bar.wav"))[0],
              synth.make_track(9501, seconds=1.0)[0][:8000]]  # (shorter than the key frame: the key path is skipped)
        cfg, ocfg = _cfgs()
        b = Batch(xs)
        _MAIN.update(batch=b, cfg=cfg, ocfg=ocfg, chains=[S.track_inputs(x, SR, ocfg) for x in xs], plain=b.plain(cfg))
    return _MAIN


def test_behavioural_track_golden_wav_and_short_track_in_one_ragged_batch():
    m = _main()
    req = dict(BEHAVIOURAL_REQUEST, snap_seconds=0.5)
    res, secs = check(m["batch"], m["cfg"], m["ocfg"], m["chains"], req, plain=m["plain"])
    s = secs[0]
    assert s["n_sections"] == 3 and s["cell_samples"] == 22050 and s["n_curve"] == s["n_cells"] >= 94
    for got, sec in zip(s["sections"]["start_cell"][1:].tolist(), (16.0, 32.0)):
        assert abs(got - (sec * SR - s["first_sample"]) / 22050) <= 1.0, s["sections"]["start_cell"]
    assert s["sections"]["relative_energy"][1] < 0.25
    assert secs[1]["status"] == 0 and secs[1]["n_cells"] > 0 and secs[1]["n_sections"] >= 1
    assert secs[2]["status"] == 0 and secs[2]["n_cells"] == 0 and secs[2]["n_sections"] == 0 and secs[2]["n_curve"] == 0
    # the list alone, the curves alone, cells in samples, another kernel
    for more in (dict(what=S.LIST), dict(what=S.CURVE), dict(cell_seconds=0.0, cell_samples=11025, kernel_cells=3,
                                                             min_gap_cells=0, energy_weight=0.0, min_strength=0.0)):
        _, got = check(m["batch"], m["cfg"], m["ocfg"], m["chains"], dict(req, **more), plain=m["plain"], what=more)
        assert (got[0]["n_sections"] > 0) == (more.get("what") != S.CURVE)
        assert (got[0]["n_curve"] > 0) == (more.get("what") != S.LIST)


def test_a_batch_where_tracks_fail_analysis():
    xs = [K.cadence(0, 6.0, SR), np.zeros(0, f32), np.zeros(30000, f32), K.cadence(7, 5.0, SR, level=0.1)]
    cfg, ocfg = _cfgs()
    b = Batch(xs)
    chains = [S.track_inputs(x, SR, ocfg) for x in xs]
    res, secs = check(b, cfg, ocfg, chains, dict(cell_seconds=0.25, kernel_cells=4, min_gap_cells=2), plain=b.plain(cfg))
    for i in (1, 2):
        assert isinstance(res[i], sdsp.AnalysisError) and secs[i]["status"] == res[i].code != 0
        assert secs[i]["n_cells"] == 0 and secs[i]["n_sections"] == 0 and secs[i]["cell_samples"] == 11025
    assert secs[0]["n_cells"] > 8 and secs[3]["n_cells"] > 8


def test_two_sub_batches_and_the_deferred_join(monkeypatch):
    """24 tracks of 20 s as one sub-batch and, under a 1 GB budget, as several (every key join but the
    last one late, reading the other parity's buffers): sections and results equal, two tracks also
    against the reference."""
    n, L = 24, 20 * SR + 37 * 24
    lens = np.array([20 * SR + 37 * k for k in range(n)], np.uint64)
    offs = np.array([k * L + (k + 1) % 4 for k in range(n)], np.uint64)
    buf = sdsp.DeviceBuffer(n * L + 8)
    sdsp.generate_synthetic(buf.ptr, n, L, seed0=9600, bpm_mode=1)
    cfg, ocfg = _cfgs()
    rq = dict(cell_seconds=0.5, kernel_cells=4, min_gap_cells=4, snap_seconds=0.25)
    req = sdsp.sections_request(**rq)

    def run():
        out = sdsp.analyze_batch_device_with(buf.ptr, offs, lens, SR, cfg, sections=req)
        res = [out[0][i] for i in range(n)]
        out[0].free()
        return res, out[-1], sdsp.stage_times()["stft8192_launches"]

    for k in ("SDSP_HBM_BUDGET_GB", "SDSP_NO_KEY_DEFER", "SDSP_SERIAL_STREAMS", "SDSP_NO_ROW_REUSE"):
        monkeypatch.delenv(k, raising=False)
    one = run()
    monkeypatch.setenv("SDSP_HBM_BUDGET_GB", "1")
    split = run()
    monkeypatch.delenv("SDSP_HBM_BUDGET_GB", raising=False)
    plain = sdsp.analyze_batch_device(buf.ptr, offs, lens, SR, cfg)
    assert one[2] == 1 and split[2] >= 2, (one[2], split[2])
    assert_same_results(one[0], plain)
    assert_same_results(split[0], one[0])
    for i in range(n):
        S.assert_equal(split[1][i], one[1][i], i)
    assert all(s["status"] == 0 and s["n_cells"] >= 38 for s in one[1])
    for i in (0, n - 1):
        x = buf.to_host(int(offs[i]), int(lens[i]))
        S.assert_equal(one[1][i], S.sections_ref(x, SR, ocfg, rq, downs=_downs(one[0][i])), ("reference", i))


def test_refusals():
    m = _main()
    b, cfg = m["batch"], m["cfg"]
    ok = dict(cell_seconds=0.5)
    bad = [dict(), dict(cell_seconds=0.5, cell_samples=22050), dict(cell_seconds=float("nan")), dict(cell_seconds=-0.5),
           dict(ok, energy_weight=float("inf")), dict(ok, min_strength=-1.0), dict(ok, snap_seconds=float("nan")),
           dict(ok, what=0), dict(ok, what=4), dict(ok, kernel_cells=0), dict(ok, kernel_cells=65),
           dict(ok, min_gap_cells=2 ** 31), dict(cell_samples=511), dict(cell_samples=2 ** 31), dict(cell_seconds=1e9)]
    for r in bad:
        assert S.plan(r, SR, 512, 512)[0] == 1
        with pytest.raises(sdsp.AnalysisError) as e:
            b.run(cfg, sections=sdsp.sections_request(**r))
        assert e.value.code == 1 and "sections" in str(e.value), r
    with pytest.raises(sdsp.AnalysisError) as e:
        b.run(cfg, sections=sdsp.sections_request(**ok), stages=sdsp.STAGES_BPM_ONLY)
    assert e.value.code == 1 and "SDSP_STAGES_BPM_ONLY" in str(e.value)
    # no output array
    ext = sdsp_abi.SdspRequestSetExt()
    rs = ext.base
    rs.struct_size = C.sizeof(ext)
    rq = sdsp.sections_request(**ok)
    ext.sc_req = C.pointer(rq)
    outs = (sdsp_abi.SdspResult * len(b.tracks))()
    u64p = C.POINTER(C.c_uint64)
    st = sdsp.lib().sdsp_analyze_batch_device_with(C.c_void_p(b.buf.ptr), b.offs.ctypes.data_as(u64p),
                                                   b.lens.ctypes.data_as(u64p), len(b.tracks), SR, C.byref(cfg), 0,
                                                   C.c_void_p(0), sdsp.STAGES_FULL, outs, C.byref(rs))
    assert st == 1 and b"without a sections array" in bytes(outs[0].error_message)
    # a caller built before the pair existed: the request is not read, the call is the plain entry
    rs.struct_size = C.sizeof(sdsp_abi.SdspRequestSet)
    st = sdsp.lib().sdsp_analyze_batch_device_with(C.c_void_p(b.buf.ptr), b.offs.ctypes.data_as(u64p),
                                                   b.lens.ctypes.data_as(u64p), len(b.tracks), SR, C.byref(cfg), 0,
                                                   C.c_void_p(0), sdsp.STAGES_FULL, outs, C.byref(rs))
    assert st == 0 and outs[0].status == 0
    for i in range(len(b.tracks)):
        sdsp.lib().sdsp_result_free(C.byref(outs[i]))
    for opts, word in ((dict(force_legacy_bpm=1), "force_legacy_bpm"), (dict(enable_key_beat_synchronous=1), "beat-synchronous")):
        c2, _ = _cfgs(**opts)
        with pytest.raises(sdsp.AnalysisError) as e:
            b.run(c2, sections=sdsp.sections_request(**ok))
        assert e.value.code == 4 and word in str(e.value)
    # log-frequency chroma rows are frames again: the request runs
    c2, _ = _cfgs(enable_key_beat_synchronous=1, enable_key_log_frequency=1)
    secs = b.run(c2, sections=sdsp.sections_request(**ok))[-1]
    assert secs[0]["status"] == 0 and secs[0]["n_cells"] >= 94


def test_with_a_key_timeline_and_a_tempo_map_in_one_call():
    m = _main()
    b, cfg = m["batch"], m["cfg"]
    req = dict(BEHAVIOURAL_REQUEST, snap_seconds=0.5)
    sreq, kreq, treq = sdsp.sections_request(**req), sdsp.key_timeline_request(segment_seconds=4.0, overlap_seconds=1.0), \
        sdsp.tempo_map_request()
    res, ovs, kts, lvs, tms, secs = b.run(cfg, key_timeline=kreq, tempo_map=treq, sections=sreq)
    assert ovs == [] and lvs == [] and len(kts) == len(tms) == len(secs) == len(b.tracks)
    assert_same_results(res, m["plain"])
    only_s = b.run(cfg, sections=sreq)
    only_k = b.run(cfg, key_timeline=kreq)
    only_t = b.run(cfg, tempo_map=treq)
    for i in range(len(b.tracks)):
        S.assert_equal(secs[i], only_s[-1][i], i)
        K.assert_equal(kts[i], only_k[2][i], i)
        _assert_same_dict(tms[i], only_t[-1][i], i)
    # without a request: the plain entry, nothing returned for sections
    out = b.run(cfg)
    assert len(out) == 4 and out[1:] == ([], [], [])
    assert_same_results(out[0], m["plain"])
