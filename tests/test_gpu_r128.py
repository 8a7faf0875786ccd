"""The programme loudness request on the GPU (sdsp_analyze_batch_device_with; k_r128.hip) against
tests/r128_ref.py, which tests/test_r128_ref.py pins to the standard's table, its conformance tone and
an unbroken f64 filter.  Every float is compared bit for bit, the curves included.

16 kHz (step 1,600): lengths around every block size (1, 4 and 30 steps), the branches of the
definition (a zero track, a track under the absolute gate, the two-level track that both relative
gates cut, a spike among the first and among the last 6 samples, steps 0 and 1 in every measured
track), 20 tracks in one call at offsets of every alignment modulo 4.
8 kHz (step 800): lengths around one and two of the step kernel's 512-step workgroups and around
the peak kernel's 1,024-sample tile.  11,025 Hz (step 1,102): a step that is no multiple of the step
kernel's 32-sample staging chunk, so its last chunk of every segment is a partial one.
The sdsp_results of a call with the request equal the same call's without it."""
import ctypes as C
import json

import numpy as np
import pytest

import r128_cases as RC
import r128_ref as R
import sdsp
import sdsp_abi
import synth
from test_gpu_overview import assert_same_results
from test_r128_ref import assert_gates_exercised

pytestmark = pytest.mark.gpu
f32 = np.float32


class Batch:
    """Host tracks packed into one device buffer at offsets that cycle through 1, 2, 3, 0 mod 4."""

    def __init__(self, tracks, sr):
        self.sr = sr
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
        self._plain = {}

    def plain(self, cfg, stages=sdsp.STAGES_FULL):
        if stages not in self._plain:
            self._plain[stages] = sdsp.analyze_batch_device(self.buf.ptr, self.offs, self.lens, self.sr, cfg, stages=stages)
        return self._plain[stages]

    def run(self, cfg, stages=sdsp.STAGES_FULL, **requests):
        out = sdsp.analyze_batch_device_with(self.buf.ptr, self.offs, self.lens, self.sr, cfg, stages=stages, **requests)
        res = [out[0][i] for i in range(len(out[0]))]
        out[0].free()
        return (res,) + tuple(out[1:])


_B = {}


def _batch(name):
    if name not in _B:
        sr, xs, tags, ref = RC.case(name)
        _B[name] = Batch(xs, sr)
    return (_B[name],) + RC.case(name)[2:]


def _check(name, what, stages=sdsp.STAGES_FULL):
    b, tags, ref = _batch(name)
    cfg = sdsp.default_config()
    plain = b.plain(cfg, stages)  # (first: the event times below are the last call's)
    out = b.run(cfg, stages=stages, loudness=sdsp.loudness_request(what))
    res, louds = out[0], out[-1]
    assert len(out) == 5 and len(louds) == len(b.tracks)
    for i, tag in enumerate(tags):
        assert louds[i]["status"] == 0, (name, tag, louds[i]["status"])  # n > 0, a supported configuration
        RC.assert_equal(louds[i], RC.masked(ref[i], what), (name, what, tag))
    assert_same_results(res, plain)
    return res, louds


def test_small_batch_every_length_and_branch():
    b, tags, ref = _batch("small")
    assert len(b.tracks) >= 19 and {int(o) % 4 for o in b.offs} == {0, 1, 2, 3}
    assert_gates_exercised(ref[tags.index("two_level")])
    res, louds = _check("small", RC.ALL)
    z, q = louds[tags.index("zero")], louds[tags.index("under_abs_gate")]
    assert z["has_integrated"] == 0 and z["integrated_lufs"] == -np.inf and z["sample_peak_db"] == -np.inf
    assert q["has_integrated"] == 0 and q["n_momentary"] == 28 and np.isfinite(q["max_momentary_lufs"])
    assert louds[tags.index("len1")]["n_steps"] == 0 and louds[tags.index("len1")]["sample_peak"] > 0
    assert louds[tags.index("len6400")]["n_momentary"] == 1 and louds[tags.index("len48000")]["n_short_term"] == 1
    for k in ("spike_first", "spike_last"):
        assert louds[tags.index(k)]["true_peak"] >= louds[tags.index(k)]["sample_peak"] == f32(0.9)
    s = louds[tags.index("quarter_sine")]
    assert abs(float(s["sample_peak_db"]) + 3.0103) < 0.005 and -0.15 <= float(s["true_peak_dbtp"]) <= 0.1
    t = sdsp.r128_times()
    assert t["tracks"] == len(b.tracks) and t["steps"] == sum(r["n_steps"] for r in ref) and t["steps_ms"] > 0.0


@pytest.mark.parametrize("what", [R.LOUDNESS, R.TRUE_PEAK, R.LOUDNESS | R.TRUE_PEAK, R.LOUDNESS | R.CURVES],
                         ids=["loudness", "true_peak", "loudness_true_peak", "loudness_curves"])
def test_each_combination_of_bits(what):
    _check("small", what)


def test_bpm_only_stages():
    _check("small", RC.ALL, stages=sdsp.STAGES_BPM_ONLY)


def test_step_that_is_no_multiple_of_the_staging_chunk():
    _check("odd", RC.ALL)


def test_around_one_and_two_step_workgroups_and_the_peak_tile():
    _check("wide", RC.ALL)


def test_known_answer_sine_at_48k():
    sr = 48000
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(3 * sr) / sr).astype(f32)
    b = Batch([x], sr)
    louds = b.run(sdsp.default_config(), loudness=sdsp.loudness_request(R.LOUDNESS | R.TRUE_PEAK))[-1]
    RC.assert_equal(louds[0], RC.masked(R.measure([x], sr)[0], R.LOUDNESS | R.TRUE_PEAK), "sine")
    assert abs(float(louds[0]["integrated_lufs"]) + 3.01) <= 0.1
    assert np.max(np.abs(louds[0]["shelf"].astype(np.float64) - [1.53512485958697, -2.69169618940638, 1.19839281085285,
                                                                 -1.69065929318241, 0.73248077421585])) < 1e-7


def test_beside_levels_and_sections_in_one_call():
    sr = 44100
    xs = [synth.make_track(8800 + k, seconds=12.0)[0] for k in range(2)]
    b = Batch(xs, sr)
    cfg = sdsp.default_config()
    lreq, lvreq, sreq = sdsp.loudness_request(RC.ALL), sdsp.levels_request(15), sdsp.sections_request(cell_seconds=0.5)
    res, ovs, kts, lvs, secs, louds = b.run(cfg, levels=lvreq, sections=sreq, loudness=lreq)
    assert ovs == [] and kts == [] and len(lvs) == len(secs) == len(louds) == 2
    assert_same_results(res, b.plain(cfg))
    alone = b.run(cfg, loudness=lreq)
    only_lv = b.run(cfg, levels=lvreq)
    only_sc = b.run(cfg, sections=sreq)
    assert len(alone) == 5 and len(only_sc) == 5 and len(only_lv) == 4
    ref = R.measure(xs, sr)
    for i in range(2):
        RC.assert_equal(louds[i], ref[i], ("together", i))
        RC.assert_equal(alone[-1][i], ref[i], ("alone", i))
        assert json.dumps(lvs[i], default=repr) == json.dumps(only_lv[3][i], default=repr)
        assert json.dumps(secs[i], default=repr) == json.dumps(only_sc[-1][i], default=repr)
    # without the request: the 4-tuple of existing callers, and nothing ran for it
    out = b.run(cfg)
    assert len(out) == 4 and out[1:] == ([], [], [])
    assert sdsp.r128_times() == dict(steps_ms=0.0, peak_ms=0.0, track_ms=0.0, tracks=0, steps=0)


def test_sub_batches_give_the_same_loudness(monkeypatch):
    """Eight ragged tracks of about two minutes and a short one, as one sub-batch and, under a 1 GB
    budget, as at least three (counted by an overview request in the same call): the request is queued
    once per call, so its values and the results are equal; the short track and a long one also against
    the reference."""
    sr, n = 44100, 8
    L = 135 * sr
    lens = np.array([(100 + 5 * k) * sr + 11 * k for k in range(n)] + [33001], np.uint64)
    offs = np.array([k * L + (k + 1) % 4 for k in range(n)] + [n * L + 1], np.uint64)
    buf = sdsp.DeviceBuffer(n * L + 40000)
    sdsp.generate_synthetic(buf.ptr, n, L, seed0=8900)
    short = RC._noise(33001, 0.2, 8901)
    buf.from_host(short, start=int(offs[n]))
    cfg = sdsp.default_config()
    req = sdsp.loudness_request(R.LOUDNESS | R.TRUE_PEAK)

    def run():
        out = sdsp.analyze_batch_device_with(buf.ptr, offs, lens, sr, cfg, overview=sdsp.overview_request(columns=64), loudness=req)
        res = [out[0][i] for i in range(len(out[0]))]
        out[0].free()
        return res, out[-1], sdsp.overview_times()["sub_batches"]

    monkeypatch.delenv("SDSP_HBM_BUDGET_GB", raising=False)
    one = run()
    monkeypatch.setenv("SDSP_HBM_BUDGET_GB", "1")
    split = run()
    monkeypatch.delenv("SDSP_HBM_BUDGET_GB", raising=False)
    assert one[2] == 1 and split[2] >= 3, (one[2], split[2])
    assert_same_results(split[0], one[0])
    for i in range(n + 1):
        RC.assert_equal(split[1][i], one[1][i], ("split", i))
    assert all(l["status"] == 0 and l["has_integrated"] == 1 and l["has_range"] == 1 for l in one[1][:n])
    x = buf.to_host(int(offs[2]), int(lens[2]))
    ref = R.measure([short, x], sr, R.LOUDNESS | R.TRUE_PEAK)
    RC.assert_equal(one[1][n], ref[0], "short")
    RC.assert_equal(one[1][2], ref[1], "long")


def test_refusals():
    b, tags, ref = _batch("odd")
    cfg = sdsp.default_config()
    for what, text in ((0, "what == 0"), (8, "unknown bits"), (0x80000001, "unknown bits"), (R.CURVES, "without SDSP_R128_LOUDNESS"),
                       (R.CURVES | R.TRUE_PEAK, "without SDSP_R128_LOUDNESS")):
        with pytest.raises(sdsp.AnalysisError) as e:
            b.run(cfg, loudness=sdsp.loudness_request(what))
        assert e.value.code == 1 and "loudness request" in str(e.value) and text in str(e.value), (what, str(e.value))
    n = len(b.tracks)
    u64p = C.POINTER(C.c_uint64)

    def raw(rs, sr):
        outs = (sdsp_abi.SdspResult * n)()
        st = sdsp.lib().sdsp_analyze_batch_device_with(C.c_void_p(b.buf.ptr), b.offs.ctypes.data_as(u64p),
                                                       b.lens.ctypes.data_as(u64p), n, sr, C.byref(cfg), 0, C.c_void_p(0),
                                                       sdsp.STAGES_FULL, outs, C.byref(rs))
        msgs = [outs[i].error_message.decode() for i in range(n)]
        stats = [outs[i].status for i in range(n)]
        for i in range(n):
            sdsp.lib().sdsp_result_free(C.byref(outs[i]))
        return st, stats, msgs

    ext2 = sdsp_abi.SdspRequestSetExt2()
    rs = ext2.base.base
    rs.struct_size = C.sizeof(ext2)
    rq = sdsp.loudness_request(R.LOUDNESS)
    ext2.r128_req = C.pointer(rq)
    st, stats, msgs = raw(rs, b.sr)  # no output array
    assert st == 1 and stats == [1] * n and "without an r128 array" in msgs[0]
    arr = (sdsp_abi.SdspR128 * n)()
    for i in range(n):
        arr[i].status = 77
    ext2.r128 = arr
    st, stats, msgs = raw(rs, 7999)  # a sample rate under 8000 Hz
    assert st == 1 and stats == [1] * n and "under 8000 Hz" in msgs[0]
    assert [arr[i].status for i in range(n)] == [1] * n and arr[0].n_samples == 0
    # callers built before the pair existed: the request is not read, the call is the plain entry
    for size in (C.sizeof(sdsp_abi.SdspRequestSetExt), C.sizeof(sdsp_abi.SdspRequestSet)):
        for i in range(n):
            arr[i].status = 77
        rs.struct_size = size
        st, stats, _ = raw(rs, b.sr)
        assert st == 0 and arr[0].status == 77, size
