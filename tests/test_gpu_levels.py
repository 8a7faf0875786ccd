"""The levels request on the GPU (sdsp_analyze_batch_device_with; k_levels.hip) against
tests/levels_ref.py, which tests/test_levels_ref.py pins to the oracle.  16 kHz: a 6,400-sample
LUFS block against the kernel's 512-sample chunk (lengths around one, two and four chunks, around one
and two blocks), and 8 minimum silent frames at frame size 2,048.

Every value is compared bit for bit: the five floats and the flags of each method, the applied
gain (applied_gain * raw equals oracle.normalize), the trim bounds, every region and its duration.
The sdsp_results of a call with the request equal the same call's without it.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import levels_ref
import oracle
import sdsp
import sdsp_abi
import synth
from test_gpu_overview import assert_same_results
from test_levels_ref import MAP_CASES, _noise, _with_silence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "stratum-dsp_amd", "bin")
SR = 16000
NAMES = ("peak", "rms", "loudness")
FLOATS = ("measured_lufs", "peak_db", "rms_db", "gain_db", "gain")
ALL = 15


def _cfg(**opts):
    c = sdsp.default_config()
    for k, v in opts.items():
        setattr(c, k, v)
    return c


def _bits(v):
    return int(np.float32(v).view(np.uint32))


class Batch:
    """Host tracks packed back to back into one device buffer, from float offset `first` on."""

    def __init__(self, tracks, first=0):
        self.tracks = [np.ascontiguousarray(t, np.float32) for t in tracks]
        self.lens = np.array([t.size for t in self.tracks], np.uint64)
        self.offs = (first + np.concatenate([[0], np.cumsum(self.lens)[:-1]])).astype(np.uint64)
        total = first + int(self.lens.sum())
        host = np.zeros(total + 8, np.float32)
        for o, t in zip(self.offs, self.tracks):
            host[int(o):int(o) + t.size] = t
        self.buf = sdsp.DeviceBuffer(total + 8)
        self.buf.from_host(host)

    def plain(self, cfg, sr=SR, stages=sdsp.STAGES_FULL):
        return sdsp.analyze_batch_device(self.buf.ptr, self.offs, self.lens, sr, cfg, stages=stages)

    def call(self, cfg, sr=SR, stages=sdsp.STAGES_FULL, **req):
        batch, ovs, kts, lvs = sdsp.analyze_batch_device_with(self.buf.ptr, self.offs, self.lens, sr, cfg, stages=stages, **req)
        res = [batch[i] for i in range(len(batch))]
        batch.free()
        return res, ovs, kts, lvs


def assert_methods(lv, ref, what, tag):
    for m, name in enumerate(NAMES):
        got = lv["methods"][name]
        want = ref[m] if what & (1 << m) else levels_ref.unmeasured()
        assert (got["status"], got["measured"], got["has_lufs"]) == (want["status"], want["measured"], want["has_lufs"]), (tag, name)
        for k in FLOATS:
            assert _bits(got[k]) == _bits(want[k]), (tag, name, k, got[k], want[k])


def assert_map(lv, x, what, tag, sr=SR, trimming=True, frame_size=2048, threshold_db=-40.0):
    """Trim bounds and regions against detect_and_trim on raw * applied_gain."""
    regions, ts, te = levels_ref.silence_map(x * lv["applied_gain"], sr, frame_size, threshold_db)
    assert lv["n_samples"] == len(x) and lv["frame_size"] == frame_size and _bits(lv["threshold_db"]) == _bits(threshold_db)
    assert (lv["trim_start"], lv["trim_end"]) == ((ts, te) if trimming else (0, len(x))), (tag, lv["trim_start"], lv["trim_end"])
    if not what & 8:
        assert lv["n_regions"] == 0 and lv["regions"] == [], tag
        return regions
    assert [(a, b) for a, b, _ in lv["regions"]] == regions, (tag, lv["regions"], regions)
    for (a, b, s), r in zip(lv["regions"], regions):
        assert _bits(s) == _bits(levels_ref.region_seconds(r, sr)), (tag, r)
    return regions


# ---- levels: 19 tracks (two fold workgroups), every alignment, every branch; three more around one chunk ----
LENGTHS = (1, 3, 1023, 1024, 1025, 2047, 2048, 2049, 6399, 6400, 6401, 12800, 12805, 20000, 33000)
_LV = {}


def _levels_batch():
    if not _LV:
        xs = [_noise(n, 0.1, 900 + k) for k, n in enumerate(LENGTHS)]
        xs += [_noise(20000, 0.9, 950), _noise(20000, 1e-5, 951), np.zeros(12805, np.float32), _noise(20000, "spike", 952)]
        assert len(xs) == 19
        xs += [_noise(n, 0.1, 980 + n) for n in (511, 512, 513)]
        b = Batch(xs)
        assert {int(o) % 4 for o in b.offs[:19]} == {0, 1, 2, 3}
        _LV.update(batch=b, ref=levels_ref.loudness(xs, SR), plain={})
    return _LV


def _plain(m, cfg, key, stages=sdsp.STAGES_FULL):
    if (key, stages) not in m["plain"]:
        m["plain"][(key, stages)] = m["batch"].plain(cfg, stages=stages)
    return m["plain"][(key, stages)]


@pytest.mark.parametrize("what", [1, 2, 4, 8, ALL], ids=["peak", "rms", "loudness", "silence", "all"])
def test_each_bit_alone_and_all_together(what):
    m = _levels_batch()
    b, cfg = m["batch"], _cfg()
    res, _, _, lvs = b.call(cfg, levels=sdsp.levels_request(what))
    assert len(lvs) == 22
    for i, x in enumerate(b.tracks):
        assert lvs[i]["status"] == 0, (i, lvs[i])  # every track: 16 kHz is a supported configuration
        assert_methods(lvs[i], m["ref"][i], what, (what, i))
        assert_map(lvs[i], x, what, (what, i))
    assert_same_results(res, _plain(m, cfg, "default"))
    # the branches the tracks were chosen for
    r = m["ref"]
    assert r[16][2]["has_lufs"] == 0 and np.isfinite(r[16][2]["peak_db"])  # every block gated: the Peak metadata
    assert r[17][0]["gain"] == 1.0 and r[17][1]["peak_db"] == -np.inf      # exact zeros
    assert r[18][1]["gain"] == np.float32(np.float32(1.0) / np.float32(0.99))  # limited by the peak


CONFIGURED = {"peak": dict(normalization=0), "rms": dict(normalization=1), "loudness": dict(normalization=2),
              "off": dict(enable_normalization=0)}


@pytest.mark.parametrize("name", sorted(CONFIGURED))
@pytest.mark.parametrize("stages", [sdsp.STAGES_FULL, sdsp.STAGES_BPM_ONLY], ids=["full", "bpm_only"])
def test_configured_normalisation(name, stages):
    """method[] does not depend on the configuration; applied_gain is the configured method's."""
    m = _levels_batch()
    b, cfg = m["batch"], _cfg(**CONFIGURED[name])
    res, _, _, lvs = b.call(cfg, stages=stages, levels=sdsp.levels_request(ALL))
    for i, x in enumerate(b.tracks):
        assert lvs[i]["status"] == 0, (name, i)
        assert_methods(lvs[i], m["ref"][i], ALL, (name, i))
        g = lvs[i]["applied_gain"]
        if name == "off":
            assert g == 1.0
        else:
            st, want = oracle.normalize(x, cfg.normalization, SR)
            assert st == 0 and np.array_equal((x * g).view(np.uint32), want.view(np.uint32)), (name, i, g)
        assert_map(lvs[i], x, ALL, (name, i))
    assert_same_results(res, _plain(m, cfg, name, stages))


# ---- the silence map ----
_MAP = {}


def _map_batch():
    if not _MAP:
        names = sorted(MAP_CASES) + ["tile_edge"]
        # 300,000 samples, 291 frames: a silent run over frames 250-269, across the kernel's 256-frame tile edge
        xs = [MAP_CASES[k] for k in sorted(MAP_CASES)] + [_with_silence(300000, [(250 * 1024, 271 * 1024)], seed=8)]
        _MAP.update(names=names, batch=Batch(xs, first=1))
    return _MAP


@pytest.mark.parametrize("opts", [dict(hop_size=512), dict(hop_size=384), dict(enable_silence_trimming=0)],
                         ids=["hop512_shared_rows", "hop384", "trimming_off"])
def test_silence_map(opts):
    m = _map_batch()
    b, cfg = m["batch"], _cfg(**opts)
    res, _, _, lvs = b.call(cfg, levels=sdsp.levels_request(8 | 1))
    got = {}
    for i, (name, x) in enumerate(zip(m["names"], b.tracks)):
        assert lvs[i]["status"] == 0, name
        st, want = oracle.normalize(x, 0, SR)
        assert np.array_equal((x * lvs[i]["applied_gain"]).view(np.uint32), want.view(np.uint32)), name
        got[name] = assert_map(lvs[i], x, 8, (opts, name), trimming=bool(cfg.enable_silence_trimming))
    n = {k: len(x) for k, x in zip(m["names"], b.tracks)}
    assert got["leading2"] == [(0, 2048)]
    assert got["interior7"] == [] and got["trailing7"] == [] and got["none"] == [] and got["short"] == []
    assert got["interior8"] == [(10 * 1024, 18 * 1024)]
    assert got["trailing8"] == [(21 * 1024, n["trailing8"])]
    assert got["all"] == [(0, n["all"])] and got["short_silent"] == [(0, n["short_silent"])]
    assert got["tile_edge"] == [(250 * 1024, 270 * 1024)]
    if cfg.enable_silence_trimming:
        i = m["names"].index("all")
        assert isinstance(res[i], sdsp.AnalysisError) and "entirely silent" in str(res[i])
        i = m["names"].index("trailing7")
        assert lvs[i]["trim_end"] == n["trailing7"]
    assert_same_results(res, b.plain(cfg))


# ---- sub-batches ----
def test_sub_batches_give_the_same_levels(monkeypatch):
    """Eight ragged tracks of about two minutes and two short ones, as one sub-batch and, under a 1 GB
    budget, as at least three (counted by an overview request in the same call): equal levels and
    results; the short tracks, and a long one's Peak and RMS, also against the reference."""
    sr, n = 44100, 8
    L = 135 * sr
    lens = np.array([(100 + 5 * k) * sr + 11 * k for k in range(n)] + [20000, 33001], np.uint64)
    offs = np.array([k * L + (k + 1) % 4 for k in range(n)] + [n * L + 1, n * L + 20001 + 4], np.uint64)
    buf = sdsp.DeviceBuffer(n * L + 60000)
    sdsp.generate_synthetic(buf.ptr, n, L, seed0=7600)
    short = [_noise(20000, 0.1, 960), _with_silence(33001, [(4096, 33001)], seed=961)]
    for o, x in zip(offs[n:], short):  # behind the generated ones
        buf.from_host(x, start=int(o))
    cfg = _cfg(normalization=2)

    def run():
        batch, ovs, _, lvs = sdsp.analyze_batch_device_with(buf.ptr, offs, lens, sr, cfg, overview=sdsp.overview_request(columns=64),
                                                            levels=sdsp.levels_request(ALL))
        res = [batch[i] for i in range(len(batch))]
        batch.free()
        return res, lvs, sdsp.overview_times()["sub_batches"]

    monkeypatch.delenv("SDSP_HBM_BUDGET_GB", raising=False)
    one = run()
    monkeypatch.setenv("SDSP_HBM_BUDGET_GB", "1")
    split = run()
    monkeypatch.delenv("SDSP_HBM_BUDGET_GB", raising=False)
    assert one[2] == 1 and split[2] >= 3, (one[2], split[2])
    assert_same_results(split[0], one[0])
    assert json.dumps(split[1], default=repr) == json.dumps(one[1], default=repr)
    assert all(l["status"] == 0 and l["methods"]["loudness"]["has_lufs"] == 1 for l in one[1][:n])
    ref = levels_ref.loudness(short, sr)
    for k, x in enumerate(short):
        assert_methods(one[1][n + k], ref[k], ALL, ("short", k))
        assert_map(one[1][n + k], x, ALL, ("short", k), sr=sr)
    x = buf.to_host(int(offs[3]), int(lens[3]))
    long_ref = levels_ref.loudness([x], sr, methods=(levels_ref.PEAK, levels_ref.RMS))[0]
    assert_methods(dict(one[1][3], methods=dict(one[1][3]["methods"], loudness=levels_ref.unmeasured())), long_ref, 3, "long")


# ---- the extensible entry ----
def _two_tracks():
    xs = [synth.make_track(7700 + k, seconds=12.0)[0] for k in range(2)]
    return Batch(xs, first=3), sdsp.default_config()


def test_all_three_requests_in_one_call_and_the_forwarder():
    b, cfg = _two_tracks()
    sr = 44100
    ov, kt, lv = sdsp.overview_request(columns=32), sdsp.key_timeline_request(segment_seconds=4.0, overlap_seconds=1.0), \
        sdsp.levels_request(ALL)
    plain = b.plain(cfg, sr=sr)
    res, ovs, kts, lvs = b.call(cfg, sr=sr, overview=ov, key_timeline=kt, levels=lv)
    assert_same_results(res, plain)
    # the old entry forwards to the new one: the same overviews and timelines
    batch, ovs2, kts2 = sdsp.analyze_batch_device_requests(b.buf.ptr, b.offs, b.lens, sr, cfg, overview=ov, key_timeline=kt)
    assert_same_results([batch[i] for i in range(2)], plain)
    batch.free()
    assert json.dumps(ovs, default=repr) == json.dumps(ovs2, default=repr) and len(ovs) == 2
    assert json.dumps(kts, default=repr) == json.dumps(kts2, default=repr) and kts[0]["n_segments"] > 0
    # the levels alone: the same levels
    res3, o3, k3, lvs3 = b.call(cfg, sr=sr, levels=lv)
    assert o3 == [] and k3 == [] and json.dumps(lvs3, default=repr) == json.dumps(lvs, default=repr)
    assert_same_results(res3, plain)
    ref = levels_ref.loudness([x[:40000] for x in b.tracks], sr)  # (a prefix keeps the reference quick)
    bp = Batch([x[:40000] for x in b.tracks], first=2)
    _, _, _, lp = bp.call(cfg, sr=sr, levels=lv)
    for i, x in enumerate(bp.tracks):
        assert_methods(lp[i], ref[i], ALL, ("prefix", i))
        assert_map(lp[i], x, ALL, ("prefix", i), sr=sr)
    # set == NULL, and a set with every request NULL, are the plain entry
    for rs in (False, True):
        r4, o4, k4, l4 = b.call(cfg, sr=sr, request_set=rs)
        assert o4 == [] and k4 == [] and l4 == []
        assert_same_results(r4, plain)
    t = sdsp.levels_times()
    assert t["tracks"] == 0 and t["fold_ms"] == 0.0  # nothing ran for the levels in the last call


def _raw_call(b, cfg, rs, sr=SR):
    n = len(b.tracks)
    outs = (sdsp_abi.SdspResult * n)()
    u64p = C.POINTER(C.c_uint64)
    st = sdsp.lib().sdsp_analyze_batch_device_with(C.c_void_p(b.buf.ptr), b.offs.ctypes.data_as(u64p), b.lens.ctypes.data_as(u64p),
                                                   n, sr, C.byref(cfg), 0, None, 0, outs, C.byref(rs))
    msgs = [outs[i].error_message.decode() for i in range(n)]
    stats = [outs[i].status for i in range(n)]
    for i in range(n):
        sdsp.lib().sdsp_result_free(C.byref(outs[i]))
    return st, stats, msgs


def test_refused_requests():
    b, cfg = Batch([_noise(20000, 0.1, 970), _noise(6401, 0.1, 971)]), sdsp.default_config()
    n = 2

    def rset(what, with_array=True, size=None):
        rs = sdsp_abi.SdspRequestSet()
        rs.struct_size = C.sizeof(rs) if size is None else size
        req = sdsp_abi.SdspLevelsRequest(what)
        lvs = (sdsp_abi.SdspLevels * n)()
        for i in range(n):
            lvs[i].status = 77
        rs.lv_req = C.pointer(req)
        if with_array:
            rs.levels = lvs
        return rs, lvs, req

    for what in (0, 16, 8 | 32, 0x80000000):
        rs, lvs, _keep = rset(what)
        st, stats, msgs = _raw_call(b, cfg, rs)
        assert st == 1 and stats == [1, 1] and all("levels request" in t for t in msgs), (what, st, msgs)
        assert [lvs[i].status for i in range(n)] == [1, 1] and lvs[0].n_samples == 0
    rs, lvs, _keep = rset(ALL, with_array=False)
    st, stats, msgs = _raw_call(b, cfg, rs)
    assert st == 1 and stats == [1, 1] and "without a levels array" in msgs[0]
    for size in (0, 4, sdsp_abi.SdspRequestSet.overviews.offset + C.sizeof(C.c_void_p) - 1):
        rs, lvs, _keep = rset(ALL, size=size)
        st, stats, msgs = _raw_call(b, cfg, rs)
        assert st == 1 and stats == [1, 1] and "struct_size" in msgs[0], (size, msgs)
        assert lvs[0].status == 77  # the levels pointer lies past the caller's struct: not touched
    # a caller whose struct ends before the levels pair: its levels request is not read
    rs, lvs, _keep = rset(0, size=sdsp_abi.SdspRequestSet.lv_req.offset)
    st, stats, _ = _raw_call(b, cfg, rs)
    assert st == 0 and lvs[0].status == 77
    with pytest.raises(sdsp.AnalysisError) as e:
        b.call(cfg, levels=sdsp.levels_request(0))
    assert e.value.kind == "InvalidInput"


# ---- CLI ----
def _rows(out):
    rows = []
    for ln in out.stdout.splitlines():
        r = json.loads(ln)
        r.pop("processing_time_ms", None)
        rows.append(r)
    return rows


def test_cli_levels_member():
    names = ("120bpm_4bar.wav", "mixed_silence.wav")
    paths = [os.path.join(GOLDEN, k) for k in names]
    base = [os.path.join(BIN, "analyze_batch"), "--json", "--jobs", "2", "--devices", "1"]
    plain = subprocess.run(base + paths, capture_output=True, text=True, timeout=300)
    full = subprocess.run(base + ["--levels"] + paths, capture_output=True, text=True, timeout=300)
    part = subprocess.run(base + ["--levels", "peak,silence", "--overview", "16", "--key-timeline", "2"] + paths,
                          capture_output=True, text=True, timeout=300)
    for p in (plain, full, part):
        assert p.returncode == 0, p.stderr
    a, f, p = _rows(plain), _rows(full), _rows(part)
    decoded = [sdsp.decode_audio_file(q) for q in paths]
    assert len({sr for _, sr in decoded}) == 1
    sr = decoded[0][1]
    bt = Batch([x for x, _ in decoded])
    cfg = sdsp.default_config()
    for rows, what in ((f, ALL), (p, 1 | 8)):
        _, _, _, lvs = bt.call(cfg, sr=sr, levels=sdsp.levels_request(what))
        for i, r in enumerate(rows):
            r = dict(r)
            lv = r.pop("levels")
            r.pop("overview", None)
            r.pop("key_timeline", None)
            assert r == a[i], (what, i)
            want = lvs[i]
            for k in ("status", "n_samples", "trim_start", "trim_end", "frame_size", "n_regions"):
                assert lv[k] == want[k], (what, i, k)
            assert _bits(lv["applied_gain"]) == _bits(want["applied_gain"])
            for m, name in enumerate(NAMES):
                assert (name in lv) == bool(what & (1 << m))
                if name in lv:
                    for k in FLOATS:
                        w = want["methods"][name][k]
                        if k == "measured_lufs" and not want["methods"][name]["has_lufs"]:
                            assert lv[name][k] is None
                        elif np.isinf(w):
                            assert lv[name][k] is None
                        else:
                            assert _bits(lv[name][k]) == _bits(w), (name, k)
            assert [(s, e) for s, e, _ in lv["regions"]] == [(s, e) for s, e, _ in want["regions"]]
            assert [_bits(t) for _, _, t in lv["regions"]] == [_bits(t) for _, _, t in want["regions"]]
    assert f[1]["levels"]["n_regions"] > 0  # mixed_silence.wav has silence
    assert all("levels" not in r for r in a)
    assert all("overview" in r and "key_timeline" in r for r in _rows(part))
