"""Option branches across several sub-batches (GPU, through the C ABI).

Every option branch has an oracle parity test of its own, but in calls that fit one sub-batch; only
the default configuration is also tested split into several.  What a stage hands to the next one
(frame prefixes over the surviving tracks, the escalated and fallback subsets, the per-parity key
uploads E0.* / E1.*, the pending key join) is rebuilt per sub-batch, so a fault there shows only
when an option runs across sub-batch boundaries: state left from the previous sub-batch, a join
taken on the wrong pending record, a prefix indexed by batch position where the position among the
surviving tracks was meant.

One ragged device batch (escalation-heavy synthetic tracks of about 20 s, a 2,048-sample track, a
5,000-sample track and an all-zero track that fails after trimming inside a sub-batch) is analysed
per case once whole and once under a 1 GB budget (>= 3 sub-batches: both parity buffer sets are
reused and the late join crosses a boundary twice).  Every track of the split run equals the whole
run's bit for bit, error or result, tempogram candidates included; five tracks of the split run are
compared with the oracle.
"""
import concurrent.futures as cf

import numpy as np
import pytest

import oracle
import parity
import sdsp

pytestmark = pytest.mark.gpu

N_LONG = 40  # ~57 MB of budget each at the default configuration: 3 sub-batches under 1 GB
SHORT_A, ZERO, SHORT_B = 5, 21, 36  # batch positions of the 2,048-sample, silent and 5,000-sample tracks
ZERO_LEN = 44100 * 3

CASES = {
    "default": {},
    "hpss_perc_cands": dict(enable_hpss_onsets=1, enable_tempogram_percussive_fallback=1, emit_tempogram_candidates=1),
    "hop256_cands": dict(hop_size=256, emit_tempogram_candidates=1),
    "beat_sync": dict(enable_key_beat_synchronous=1),
    "bpm_fusion": dict(enable_bpm_fusion=1),
    "debug_track": dict(has_debug_track_id=1, debug_track_id=7),
}

_BATCH = None


def _batch():
    """The device batch, generated once and left unchanged: (buffer, offsets, lengths)."""
    global _BATCH
    if _BATCH is None:
        lens = [44100 * 20 + 37 * k for k in range(N_LONG)]
        lens.insert(SHORT_A, 2048)
        lens.insert(ZERO, ZERO_LEN)
        lens.insert(SHORT_B, 5000)
        lens = np.asarray(lens, dtype=np.uint64)
        Lmax = int(lens.max())
        buf = sdsp.DeviceBuffer(len(lens) * Lmax)
        sdsp.generate_synthetic(buf.ptr, len(lens), Lmax, seed0=3100, bpm_mode=1)
        offs = (np.arange(len(lens)) * Lmax).astype(np.uint64)
        buf.from_host(np.zeros(ZERO_LEN, np.float32), int(offs[ZERO]))
        _BATCH = (buf, offs, lens)
    return _BATCH


def _apply(cfg, opts):
    for k, v in opts.items():
        setattr(cfg, k, v)
    return cfg


def _strip(r):
    if isinstance(r, sdsp.AnalysisError):
        return ("err", r.code, str(r))
    m = dict(r["metadata"])
    m.pop("processing_time_ms", None)
    return {k: v for k, v in r.items() if k != "metadata"} | {"metadata": m}


@pytest.mark.parametrize("case", list(CASES))
def test_options_across_sub_batches(case, monkeypatch):
    buf, offs, lens = _batch()
    cfg = _apply(sdsp.default_config(), CASES[case])
    ocfg = _apply(oracle.default_config(), CASES[case])
    for k in ("SDSP_HBM_BUDGET_GB", "SDSP_NO_KEY_DEFER", "SDSP_SERIAL_STREAMS", "SDSP_NO_ROW_REUSE"):
        monkeypatch.delenv(k, raising=False)
    whole = sdsp.analyze_batch_device(buf.ptr, offs, lens, config=cfg)
    assert sdsp.stage_times()["stft8192_launches"] == 1
    monkeypatch.setenv("SDSP_HBM_BUDGET_GB", "1")
    split = sdsp.analyze_batch_device(buf.ptr, offs, lens, config=cfg)
    assert sdsp.stage_times()["stft8192_launches"] >= 3
    assert isinstance(whole[ZERO], sdsp.AnalysisError) and "silent" in str(whole[ZERO])
    for i, (a, b) in enumerate(zip(whole, split)):
        assert _strip(a) == _strip(b), (case, i)
        if not isinstance(a, sdsp.AnalysisError):
            assert parity.exact_fraction(a, b, strict=True) == 1.0, (case, i)
    # the first, one of the middle sub-batch, the last long one and the two short ones
    pick = (0, ZERO + 1, len(lens) - 1, SHORT_A, SHORT_B)
    xs = [buf.to_host(int(offs[i]), int(lens[i])) for i in pick]
    with cf.ThreadPoolExecutor(len(pick)) as ex:
        refs = list(ex.map(lambda x: oracle.analyze(x, 44100, ocfg), xs))
    for i, (st, ref) in zip(pick, refs):
        if st != 0:
            assert isinstance(split[i], sdsp.AnalysisError) and (split[i].code, str(split[i])) == (st, ref), (case, i)
            continue
        assert not isinstance(split[i], sdsp.AnalysisError), (case, i, split[i])
        bad = parity.diff_results(split[i], ref)
        assert not bad, f"{case} track {i}: {bad}"
        assert parity.exact_fraction(split[i], ref, cfg=cfg) == 1.0, (case, i)
