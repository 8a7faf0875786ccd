"""The fingerprint request on the GPU (sdsp_analyze_batch_device_with, sdsp_debug_fingerprint,
sdsp_debug_fingerprint_match, k_fingerprint.hip) against tests/fingerprint_ref.py: the definition in
numpy f32 over the oracle's own chroma rows, pairs by plain loops.

Everything is compared for equality, floats on their uint32 view.  The sdsp_results of a call with the
request are compared with the plain entry's, field for field (processing_time_ms aside).
"""
import ctypes as C
import os

import numpy as np
import pytest

import fingerprint_cases as FC
import fingerprint_ref as R
import key_timeline_ref as K
import oracle
import parity
import sdsp
import sdsp_abi
import sections_ref as S
import synth
from test_gpu_sections import Batch, _assert_same_dict, _cfgs, assert_same_results

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SR = 44100
f32 = np.float32
u32 = np.uint32


# ---- words through the debug entry ----
@pytest.mark.parametrize("layout", sorted(FC.LAYOUTS))
def test_words_one_ragged_call_and_single_track_calls(layout):
    """Cell counts 0, 1, 2, 3, 4, 63, 64, 65, 66, 130, 300 with all-zero and constant rows in one
    call, Cs a multiple of khop and not (43 or 44 frames per cell); single-track calls equal it."""
    khop, Cs = FC.LAYOUTS[layout]
    tr, ref = FC.word_tracks(layout), FC.word_reference(layout)
    req = sdsp.fingerprint_request(cell_samples=Cs)
    got = sdsp.debug_fingerprint([t[0] for t in tr], req, SR, khop)
    assert len(got) == len(tr)
    for g, (m, w), (_, tag) in zip(got, ref, tr):
        assert g["n_cells"] == m.shape[0] and g["n_words"] == w.size, (layout, tag)
        S.assert_arrays_equal(g["m"], m, (layout, tag, "m"))
        S.assert_arrays_equal(g["words"], w, (layout, tag, "words"))
        if tag in ("zero_rows", "constant_rows"):
            assert g["n_words"] == 18 and not g["words"].any(), tag
    assert [g["n_words"] for g in got[:len(FC.CELL_COUNTS)]] == [max(n - 2, 0) for n in FC.CELL_COUNTS]
    for t in (0, 3, 5, 8, 10, len(tr) - 1):
        one = sdsp.debug_fingerprint([tr[t][0]], req, SR, khop)[0]
        for k in ("m", "words"):
            S.assert_arrays_equal(one[k], got[t][k], (layout, t, k))


def test_debug_entries_refuse_a_bad_request():
    rows = np.zeros((10, 12), f32)
    for bad in (dict(cell_samples=511), dict(cell_samples=512, what=0), dict(cell_samples=512, max_offset_words=256)):
        with pytest.raises(sdsp.AnalysisError) as e:
            sdsp.debug_fingerprint([rows], sdsp.fingerprint_request(**bad), SR)
        assert e.value.code == 1
    with pytest.raises(sdsp.AnalysisError) as e:
        sdsp.debug_fingerprint_match([np.ones(3, u32), np.ones(3, u32)], sdsp.fingerprint_request(cell_samples=512,
                                                                                                   max_offset_words=256))
    assert e.value.code == 1


# ---- the match through the debug entry, on made-up word arrays ----
def _match(words, O, mo):
    return sdsp.debug_fingerprint_match(words, sdsp.fingerprint_request(cell_samples=5512, max_offset_words=O,
                                                                        min_overlap_words=mo))


def _assert_records(got, ref, what):
    for k in ("eligible", "offset_words", "bit_errors", "positions"):
        assert np.array_equal(got[k].astype(np.int64), ref[k]), (what, k, np.argwhere(got[k].astype(np.int64) != ref[k])[:4])


@pytest.mark.parametrize("name", sorted(FC.match_calls()))
def test_match_records_of_made_up_words(name):
    """W from {1, 2, 63, 64, 65, 130, 300} mixed in one call; 1, 2, 5, 17 tracks and 9 tracks of 3 words
    (across the 4 x 4 tile's edge both ways); O from {0, 1, 31, 32, 63, 64, 255}: O >= W and both sides
    of a 64-lane pass."""
    words, runs = FC.match_calls()[name]
    eligible = 0
    for O, mo in runs:
        got = _match(words, O, mo)
        assert got.shape == (len(words), len(words))
        _assert_records(got, FC.match_reference(name, O, mo), (name, O, mo))
        eligible += int(got["eligible"].sum())
    assert eligible > 0 or len(words) == 1
    if name == "mixed7":  # the planted relations are found once O reaches them
        got = _match(words, 255, 1)
        assert (got["offset_words"][2, 6], got["bit_errors"][2, 6]) == (40, 3)  # (zero words of both are not counted)
        assert (got["offset_words"][3, 6], got["bit_errors"][3, 6]) == (100, 0)
        assert (got["offset_words"][5, 6], got["bit_errors"][5, 6]) == (-7, 9)


def test_match_rules_on_hand_made_pairs():
    rng = np.random.default_rng(3)
    # min_overlap_words at n(o) - 1, n(o), n(o) + 1 of a known pair: 40 non-zero words against themselves at O = 0
    A = rng.integers(1, 1 << 24, 40, dtype=u32)
    for mo, has in ((39, 1), (40, 1), (41, 0)):
        r = _match([A, A.copy()], 0, mo)[0, 1]
        assert (r["eligible"], r["positions"], r["bit_errors"]) == ((1, 40, 0) if has else (0, 0, 0)), mo
    # all-zero arrays: nothing is counted, no eligible offset, whatever min_overlap_words
    Z = np.zeros(50, u32)
    for mo in (0, 1):
        r = _match([Z, Z.copy()], 5, mo)[0, 1]
        assert (r["eligible"], r["offset_words"], r["bit_errors"], r["positions"]) == (0, 0, 0, 0)
    # zeros meeting non-zeros are counted: e = the non-zero words' bits
    N = np.array([3, 0, 7, 0, 1, 0], u32)
    r = _match([np.zeros(6, u32), N], 0, 1)[0, 1]
    assert (r["eligible"], r["offset_words"], r["bit_errors"], r["positions"]) == (1, 0, 6, 3)
    # a periodic array against itself: e = 0 at every multiple of the period, the best is o = 0
    P = np.array([1, 2, 4, 8] * 20, u32)
    for O in (8, 64, 255):
        r = _match([P, P.copy()], O, 1)[0, 1]
        assert (r["eligible"], r["offset_words"], r["bit_errors"], r["positions"]) == (1, 0, 0, 80), O
    # a constructed tie between -2 and +2 gives -2
    r = _match([np.array([0, 0, 5, 0, 0], u32), np.array([5, 0, 0, 0, 5], u32)], 2, 1)[0, 1]
    assert (r["eligible"], r["offset_words"], r["bit_errors"], r["positions"]) == (1, -2, 0, 1)
    assert R.best_offset([0, 0, 5, 0, 0], [5, 0, 0, 0, 5], 2, 1) == (-2, 0, 1)
    # a shifted copy with a few flipped bits: exact o, e and n.  B[p + 11] = A[p] for p in [0, 189)
    A = rng.integers(1, 1 << 24, 200, dtype=u32)
    B = np.concatenate([rng.integers(1, 1 << 24, 11, dtype=u32), A[:189]])
    for p, bit in ((20, 0), (20, 5), (100, 23), (199, 7)):
        B[p] ^= u32(1 << bit)
    for O in (11, 31, 32, 100):
        r = _match([A, B], O, 32)[0, 1]
        assert (r["eligible"], r["offset_words"], r["bit_errors"], r["positions"]) == (1, 11, 4, 189), O
    r = _match([A, B], 10, 32)[0, 1]
    assert r["eligible"] == 1 and r["offset_words"] != 11 and r["bit_errors"] > 1000


def test_match_in_two_row_bands():
    """2,100 one-word tracks: the records of a launch stay under 64 MB, so the rows go in two bands
    (1,996 and 103 rows) and the second launch runs with row0 > 0.  At O = 0 a pair of one-word
    tracks has n = 1 unless both words are zero, and e = popcount(a ^ b): a closed form."""
    T = 2100
    assert (64 << 20) // (16 * T) // 4 * 4 < T - 1  # (two bands, by fp_match_bands' bound)
    rng = np.random.default_rng(41)
    w = rng.integers(0, 1 << 24, T, dtype=u32)
    w[rng.random(T) < 0.05] = 0
    got = _match([w[t:t + 1] for t in range(T)], 0, 1)
    upper = np.triu(np.ones((T, T), bool), 1)
    x = w[:, None] ^ w[None, :]
    e = np.zeros((T, T), np.int64)
    for bit in range(24):
        e += (x >> u32(bit)) & u32(1)
    n = (((w[:, None] | w[None, :]) != 0) & upper).astype(np.int64)
    assert np.array_equal(got["eligible"].astype(np.int64), n)
    assert np.array_equal(got["positions"].astype(np.int64), n)
    assert np.array_equal(got["bit_errors"].astype(np.int64), e * n)
    assert not got["offset_words"].any()
    assert n[1996:].sum() > 1000 and (n[upper] == 0).sum() > 0


# ---- end to end ----
REQ =dict(cell_samples=5512, max_offset_words=16, min_overlap_words=32, max_ber=0.30)
_MAIN = {}


def _main():
    if not _MAIN:
        x = R.random_triads(1, 14.0)
        xs = [x, (x * f32(0.5)).astype(f32), x[5512:], R.random_triads(2, 12.0), R.random_triads(3, 13.0),
              parity.load_wav(os.path.join(GOLDEN, "120bpm_4bar.wav"))[0],
              synth.make_track(9501, seconds=1.0)[0][:8000],  # (shorter than the key frame: the key path is skipped)
              np.zeros(0, f32)]  # (empty: the track fails)
        cfg, ocfg = _cfgs()
        b = Batch(xs)
        _MAIN.update(batch=b, cfg=cfg, ocfg=ocfg, chains=[R.track_words(x, SR, ocfg, 5512) for x in xs], plain=b.plain(cfg))
    return _MAIN


def test_one_ragged_call_equals_the_reference():
    m = _main()
    b = m["batch"]
    want = R.fingerprint_ref(b.tracks, SR, m["ocfg"], REQ, chains=m["chains"])
    out = b.run(m["cfg"], fingerprint=sdsp.fingerprint_request(**REQ))
    assert len(out) == 5
    R.assert_equal(out[-1], want)
    assert_same_results(out[0], m["plain"])
    fp, ml = out[-1]["fingerprints"], out[-1]["matches"]
    pairs = list(zip(ml["matches"]["a"].tolist(), ml["matches"]["b"].tolist(), ml["matches"]["offset_words"].tolist()))
    assert pairs == [(0, 1, 0), (0, 2, -1), (1, 2, -1)], pairs
    assert ml["matches"]["bit_errors"][0] == 0 and ml["matches"]["offset_samples"][1] == -5512
    assert [f["n_matches"] for f in fp] == [2, 2, 2, 0, 0, 0, 0, 0]
    assert ml["n_compared"] == 6 and ml["n_pairs"] == 15
    assert fp[6]["status"] == 0 and fp[6]["n_cells"] == 0 and fp[6]["n_words"] == 0
    assert fp[7]["status"] == 1 and fp[7]["cell_samples"] == 5512 and fp[7]["n_cells"] == 0
    assert isinstance(out[0][7], sdsp.AnalysisError)
    # the words alone; the match alone; cells in seconds
    for more in (dict(what=R.WORDS), dict(what=R.MATCH), dict(cell_samples=0, cell_seconds=0.125)):
        rq = dict(REQ, **more)
        got = b.run(m["cfg"], fingerprint=sdsp.fingerprint_request(**rq))[-1]
        R.assert_equal(got, R.fingerprint_ref(b.tracks, SR, m["ocfg"], rq, chains=m["chains"]), more)
        assert (got["matches"]["n_matches"] == 3) == (more.get("what") != R.WORDS)
        assert (got["fingerprints"][0]["words"].size > 0) == (more.get("what") != R.MATCH)


def test_two_sub_batches_match_across_them(monkeypatch):
    """24 tracks of 20 s as one sub-batch and, under a 1 GB budget, as several, track 23 a copy of
    track 0: the match pairs tracks of different sub-batches; words and list equal in both runs, two
    tracks also against the reference."""
    n, L = 24, 20 * SR + 37 * 24
    lens = np.array([20 * SR + 37 * k for k in range(n)], np.uint64)
    offs = np.array([k * L + (k + 1) % 4 for k in range(n)], np.uint64)
    buf = sdsp.DeviceBuffer(n * L + 8)
    sdsp.generate_synthetic(buf.ptr, n, L, seed0=9600, bpm_mode=1)
    host = buf.to_host(0, n * L + 8)
    x0 = host[int(offs[0]):int(offs[0]) + int(lens[0])].copy()
    host[int(offs[23]):int(offs[23]) + x0.size] = x0  # (track 23 is the longer one: a copy of track 0 and a tail)
    buf.from_host(host)
    cfg, ocfg = _cfgs()
    req = sdsp.fingerprint_request(**REQ)

    def run():
        out = sdsp.analyze_batch_device_with(buf.ptr, offs, lens, SR, cfg, fingerprint=req)
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
    R.assert_equal(split[1], one[1], "split against one")
    ml = one[1]["matches"]
    assert ml["n_compared"] == n and ml["n_pairs"] == n * (n - 1) // 2
    k = np.flatnonzero((ml["matches"]["a"] == 0) & (ml["matches"]["b"] == 23))
    assert k.size == 1 and ml["matches"]["offset_words"][k[0]] == 0 and ml["matches"]["ber"][k[0]] < 0.05, ml["matches"]
    chains = [R.track_words(host[int(offs[i]):int(offs[i]) + int(lens[i])], SR, ocfg, 5512) for i in (0, 23)]
    want = R.fingerprint_ref([None, None], SR, ocfg, REQ, chains=chains)
    for j, i in enumerate((0, 23)):
        g, w = one[1]["fingerprints"][i], want["fingerprints"][j]
        for key in ("status", "n_cells", "n_words", "first_sample"):
            assert g[key] == w[key], (i, key)
        S.assert_arrays_equal(g["words"], w["words"], (i, "words"))
    wm = want["matches"]["matches"]
    assert want["matches"]["n_matches"] == 1
    for key in R.MATCH_FIELDS[2:]:
        S.assert_arrays_equal(ml["matches"][key][k], wm[key], key)


def test_combined_requests_and_an_older_struct_size():
    m = _main()
    b, cfg = m["batch"], m["cfg"]
    freq = sdsp.fingerprint_request(**REQ)
    sreq = sdsp.sections_request(cell_seconds=0.5, kernel_cells=4, min_gap_cells=2)
    kreq = sdsp.key_timeline_request(segment_seconds=4.0, overlap_seconds=1.0)
    lreq = sdsp.loudness_request(("loudness",))
    res, ovs, kts, lvs, secs, louds, fp = b.run(cfg, key_timeline=kreq, sections=sreq, loudness=lreq, fingerprint=freq)
    assert ovs == [] and lvs == [] and len(kts) == len(secs) == len(louds) == len(fp["fingerprints"]) == len(b.tracks)
    assert_same_results(res, m["plain"])
    only_f = b.run(cfg, fingerprint=freq)[-1]
    only_s = b.run(cfg, sections=sreq)[-1]
    only_k = b.run(cfg, key_timeline=kreq)[2]
    only_l = b.run(cfg, loudness=lreq)[-1]
    R.assert_equal(fp, only_f)
    for i in range(len(b.tracks)):
        S.assert_equal(secs[i], only_s[i], i)
        K.assert_equal(kts[i], only_k[i], i)
        _assert_same_dict(louds[i], only_l[i], i)
    # a caller built against sdsp_request_set_ext2: no fingerprint, no error, the other request as ever
    n = len(b.tracks)
    ext = sdsp_abi.SdspRequestSetExt3()
    rs = ext.base.base.base
    rs.struct_size = C.sizeof(sdsp_abi.SdspRequestSetExt2)
    fps, fpm, lds = (sdsp_abi.SdspFingerprint * n)(), sdsp_abi.SdspFingerprintMatches(), (sdsp_abi.SdspR128 * n)()
    C.memset(fps, 0xAB, C.sizeof(fps))
    C.memset(C.byref(fpm), 0xAB, C.sizeof(fpm))
    ext.fp_req, ext.fingerprints, ext.fp_matches = C.pointer(freq), fps, C.pointer(fpm)
    ext.base.r128_req, ext.base.r128 = C.pointer(lreq), lds
    outs = (sdsp_abi.SdspResult * n)()
    u64p = C.POINTER(C.c_uint64)
    st = sdsp.lib().sdsp_analyze_batch_device_with(C.c_void_p(b.buf.ptr), b.offs.ctypes.data_as(u64p),
                                                   b.lens.ctypes.data_as(u64p), n, SR, C.byref(cfg), 0, C.c_void_p(0),
                                                   sdsp.STAGES_FULL, outs, C.byref(rs))
    assert st == 0
    assert bytes(fps) == b"\xab" * C.sizeof(fps) and bytes(fpm) == b"\xab" * C.sizeof(fpm)  # never written
    for i in range(n):
        _assert_same_dict(sdsp.r128_to_dict(lds[i]), only_l[i], i)
        sdsp.lib().sdsp_r128_free(C.byref(lds[i]))
        assert outs[i].status == (m["plain"][i].code if isinstance(m["plain"][i], sdsp.AnalysisError) else 0)
        sdsp.lib().sdsp_result_free(C.byref(outs[i]))
    # without a request: the plain entry, nothing returned for fingerprints
    out = b.run(cfg)
    assert len(out) == 4 and out[1:] == ([], [], [])


def test_refusals():
    m = _main()
    b, cfg = m["batch"], m["cfg"]
    ok = dict(cell_samples=5512)
    bad = [dict(ok, what=0), dict(ok, what=4), dict(), dict(cell_seconds=0.125, cell_samples=5512),
           dict(cell_seconds=float("nan")), dict(cell_seconds=-0.125), dict(ok, max_ber=float("inf")), dict(ok, max_ber=-0.5),
           dict(ok, max_ber=1.5), dict(cell_samples=511), dict(cell_samples=2 ** 31), dict(cell_seconds=1e9),
           dict(ok, max_offset_words=256)]
    for r in bad:
        assert R.plan(r, SR, 512)[0] == 1
        with pytest.raises(sdsp.AnalysisError) as e:
            b.run(cfg, fingerprint=sdsp.fingerprint_request(**r))
        assert e.value.code == 1 and "fingerprint" in str(e.value), r
    with pytest.raises(sdsp.AnalysisError) as e:
        b.run(cfg, fingerprint=sdsp.fingerprint_request(**ok), stages=sdsp.STAGES_BPM_ONLY)
    assert e.value.code == 1 and "SDSP_STAGES_BPM_ONLY" in str(e.value)
    # no output array; SDSP_FP_MATCH without the matches struct
    n = len(b.tracks)
    u64p = C.POINTER(C.c_uint64)
    for with_out, word in ((False, b"without a fingerprints array"), (True, b"without a matches struct")):
        ext = sdsp_abi.SdspRequestSetExt3()
        rs = ext.base.base.base
        rs.struct_size = C.sizeof(ext)
        rq = sdsp.fingerprint_request(**ok)
        ext.fp_req = C.pointer(rq)
        fps = (sdsp_abi.SdspFingerprint * n)()
        if with_out:
            ext.fingerprints = fps
        outs = (sdsp_abi.SdspResult * n)()
        st = sdsp.lib().sdsp_analyze_batch_device_with(C.c_void_p(b.buf.ptr), b.offs.ctypes.data_as(u64p),
                                                       b.lens.ctypes.data_as(u64p), n, SR, C.byref(cfg), 0, C.c_void_p(0),
                                                       sdsp.STAGES_FULL, outs, C.byref(rs))
        assert st == 1 and word in bytes(outs[0].error_message), word
        for i in range(n):
            sdsp.lib().sdsp_result_free(C.byref(outs[i]))
    c2, _ = _cfgs(enable_key_beat_synchronous=1)
    with pytest.raises(sdsp.AnalysisError) as e:
        b.run(c2, fingerprint=sdsp.fingerprint_request(**ok))
    assert e.value.code == 4 and "beat-synchronous" in str(e.value)
    # force_legacy_bpm is not refused (no energies are used), and the fingerprints are the same
    c2, _ = _cfgs(force_legacy_bpm=1)
    got = b.run(c2, fingerprint=sdsp.fingerprint_request(**REQ))[-1]
    want = b.run(cfg, fingerprint=sdsp.fingerprint_request(**REQ))[-1]
    R.assert_equal(got, want)
