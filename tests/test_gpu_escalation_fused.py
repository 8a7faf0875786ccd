"""The escalation's shared feature walk against the complete passes (GPU, through the C ABI).

By default the hop-256 escalation pass's k_features walk also folds the hop-1024 pass's SuperFlux,
the hop-1024 pass copies E / H / MEL from the hop-512 pass and launches no features, and neither
computes the spectral flux.  With SDSP_NO_ROW_REUSE both passes are complete and separate (their own
STFT, their own feature launch): the control.  Every fold runs in the same bin order on the same
values either way, so the two must agree bit for bit, tempogram candidates included.

Two ragged device batches of synthetic tracks (bpm_mode = 1, the escalation-heavy mix), each analysed
once by the default path and once by the control, and by the oracle on the host copies.  A track
reaches the fused walk only if it escalates, so the oracle's tempogram_multi_res_triggered flag is
asserted track by track.

"long" (default configuration plus emitted candidates):
  - the same 8 s signal cut at four lengths 256 samples apart: hop-256 frame counts in all four
    residues mod 4 (which lanes store a hop-1024 value, and whether the last frame has one), each
    spanning several 240-frame tiles with a partial last tile;
  - ragged tracks of 4-8 s, adjacent in every frame prefix, with short ones between them.
  Every track of 4 s or more must escalate.

"short" (min_bpm 175, max_bpm 200: at the default range no track this short is ambiguous, whatever
its signal; with this one every track of at least two hop-512 frames is):
  - one hop-1024 frame (no pair), two (one pair) and three;
  - fewer hop-256 frames than one wave's 60, in all four residues mod 4, and just over 60;
  - tracks of 2-5 s between them, next to them in every frame prefix: the shortest tracks'
    hop-1024 tempograms have too few frames to change a result, so a store that left its track
    would show in a neighbour's;
  - a track below one 2,048-sample frame in the same call, which cannot escalate.
  Every other track must escalate.
"""
import concurrent.futures as cf

import numpy as np
import pytest

import oracle
import parity
import sdsp
import units

pytestmark = pytest.mark.gpu

SR = 44100
BASE = SR * 8
# The generator's bpm_mode = 1 draws track i's tempo from [55, 80] (i % 3 = 0), [170, 200] (1) or
# [80, 170] (2); at these lengths the slow third seldom escalates, so it holds the short tracks.
SCHED_ENV = ("SDSP_HBM_BUDGET_GB", "SDSP_NO_KEY_DEFER", "SDSP_SERIAL_STREAMS", "SDSP_NO_ROW_REUSE",
             "SDSP_BATCH_CHUNK_TRACKS")
BATCHES = {
    "long": dict(
        lens=[1500, BASE, BASE + 256,
              2048 + 700, BASE + 512, BASE + 768,
              3072 + 700, SR * 6 + 123, SR * 5 + 77,
              12000, SR * 7, SR * 4 + 1000,
              2048 + 300, SR * 7 + 4242, SR * 8 + 333],
        same=(1, 2, 4, 5),  # one signal (track 1's) at four lengths
        seed0=3304, opts={}, must=lambda n: n >= SR * 4),
    "short": dict(
        lens=[2048 + 700, SR * 3 + 11, 3072 + 700, SR * 2 + 500, 4096 + 700,  # 1, 2, 3 hop-1024 frames
              SR * 4 + 77,
              12000, 12000 + 256, 12000 + 512, 12000 + 768,  # 39-42 hop-256 frames
              SR * 3 + 900, 16000, SR * 2 + 33, 17408 + 300,  # 55 and 62 hop-256 frames
              1500, SR * 5],
        same=(6, 7, 8, 9),
        seed0=3304, opts=dict(min_bpm=175.0, max_bpm=200.0), must=lambda n: n >= 2048 + 700),
}

_RUNS = {}
_REFS = {}


def _cfg(c, opts):
    c.emit_tempogram_candidates = 1
    for k, v in opts.items():
        setattr(c, k, v)
    return c


def _strip(r):
    if isinstance(r, sdsp.AnalysisError):
        return ("err", r.code, str(r))
    m = dict(r["metadata"])
    m.pop("processing_time_ms", None)
    return {k: v for k, v in r.items() if k != "metadata"} | {"metadata": m}


def _runs(name):
    """Batch `name` analysed once by the default path and once by the control (shared, unchanged):
    (host copies of the tracks, default results, control results)."""
    if name not in _RUNS:
        import os

        B = BATCHES[name]
        saved = {k: os.environ.pop(k, None) for k in SCHED_ENV}
        try:
            lens = np.asarray(B["lens"], dtype=np.uint64)
            Lmax = int(lens.max())
            buf = sdsp.DeviceBuffer(len(lens) * Lmax)
            sdsp.generate_synthetic(buf.ptr, len(lens), Lmax, seed0=B["seed0"], bpm_mode=1)
            offs = (np.arange(len(lens)) * Lmax).astype(np.uint64)
            x0 = buf.to_host(int(offs[B["same"][0]]), Lmax)
            for k in B["same"][1:]:
                buf.from_host(x0, int(offs[k]))
            cfg = _cfg(sdsp.default_config(), B["opts"])
            fused = sdsp.analyze_batch_device(buf.ptr, offs, lens, config=cfg)
            os.environ["SDSP_NO_ROW_REUSE"] = "1"
            control = sdsp.analyze_batch_device(buf.ptr, offs, lens, config=cfg)
            xs = [buf.to_host(int(offs[i]), int(lens[i])) for i in range(len(lens))]
        finally:
            os.environ.pop("SDSP_NO_ROW_REUSE", None)
            for k, v in saved.items():
                if v is not None:
                    os.environ[k] = v
        _RUNS[name] = (xs, fused, control)
    return _RUNS[name]


def _refs(name):
    """The oracle's (status, result) of every track of batch `name`, computed once."""
    if name not in _REFS:
        xs, _, _ = _runs(name)
        ocfg = _cfg(oracle.default_config(), BATCHES[name]["opts"])
        with cf.ThreadPoolExecutor(8) as ex:
            _REFS[name] = list(ex.map(lambda x: oracle.analyze(x, SR, ocfg), xs))
    return _REFS[name]


@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_escalates(name):
    """By the oracle, every track the batch names as an edge of the fused walk escalates (else the
    default path and the control are equal trivially there), and so do at least half of all."""
    B = BATCHES[name]
    trig = [st == 0 and ref["metadata"]["tempogram_multi_res_triggered"] is True for st, ref in _refs(name)]
    print(name, "escalated:", [i for i, t in enumerate(trig) if t], "of", len(trig))
    for i, n in enumerate(B["lens"]):
        if B["must"](n):
            assert trig[i], (name, i, n)
    assert 2 * sum(trig) >= len(trig), (name, trig)


@pytest.mark.parametrize("name", list(BATCHES))
def test_default_path_equals_separate_passes(name):
    _, fused, control = _runs(name)
    for i, (a, b) in enumerate(zip(fused, control)):
        if isinstance(a, sdsp.AnalysisError) or isinstance(b, sdsp.AnalysisError):
            assert _strip(a) == _strip(b), i
            continue
        for k in ("bpm", "bpm_confidence"):
            assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes(), (i, k, a[k], b[k])
        for k in ("tempogram_multi_res_triggered", "tempogram_multi_res_used", "tempogram_candidates"):
            assert a["metadata"].get(k) == b["metadata"].get(k), (i, k)
        assert np.array_equal(np.asarray(a["beat_grid"]["beats"], np.float32).view(np.uint32),
                              np.asarray(b["beat_grid"]["beats"], np.float32).view(np.uint32)), i
        assert _strip(a) == _strip(b), i
        assert parity.exact_fraction(a, b, strict=True) == 1.0, i


@pytest.mark.parametrize("name", list(BATCHES))
def test_oracle_parity(name):
    _, fused, _ = _runs(name)
    cfg = _cfg(sdsp.default_config(), BATCHES[name]["opts"])
    for i, (st, ref) in enumerate(_refs(name)):
        if st != 0:
            assert isinstance(fused[i], sdsp.AnalysisError) and (fused[i].code, str(fused[i])) == (st, ref), i
            continue
        assert not isinstance(fused[i], sdsp.AnalysisError), (i, fused[i])
        bad = parity.diff_results(fused[i], ref)
        assert not bad, f"track {i}: {bad}"
        assert parity.exact_fraction(fused[i], ref, cfg=cfg) == 1.0, i


@pytest.mark.parametrize("hop", [256, 1024])
def test_stage_probe_keeps_spectral_flux(hop):
    """The stage probe's pass stays complete at the escalation hops: SFO as the oracle's."""
    rng = np.random.default_rng(900 + hop)
    specs = [(rng.random((F, 1025), dtype=np.float32) ** 4 * np.float32(50)).astype(np.float32) for F in (61, 130)]
    _, tracks = sdsp.debug_tempo_stages(specs, hop=hop)
    for spec, got in zip(specs, tracks):
        sfo = units.spectral_flux_curve(spec)
        assert np.array_equal(np.asarray(got["SFO"], np.float32).view(np.uint32), np.asarray(sfo, np.float32).view(np.uint32))
