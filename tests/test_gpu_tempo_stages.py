"""Stage-level parity of the tempo kernels: k_features, k_novelty / k_mel_flux / k_mel_norm,
k_acf_tempogram and k_fft_tempogram against the oracle's stage exports, bit for bit.

The result fields see the band and mel variants only as the BPM positions of their top-8 tempogram
entries and a thresholded support bit, so a wrong value in those curves, a band edge off by a bin, a
mel weight off by an ulp or a fold that drops a term can leave every result unchanged.  Here the
pipeline's own tempo pass (sdsp_debug_tempo_stages: the same parameter set-up and launches as an
analysis call, fed a spectrogram instead of an STFT) returns every stage buffer, and each is compared
on its uint32 view with what the oracle's tempogram_impl computed the same variant from
(units.tempo_stages; pinned to the whole-track oracle in test_oracle_stage_exports.py).

Inputs are random non-negative spectrograms (magnitudes over many exponents), with rows of zeros, a
constant spectrogram and a track of repeating frames: the last two have novelty 0, so every
tempogram entry ties and the lists must come out in the stable order.
"""
import numpy as np
import pytest

import oracle
import sdsp
import units
from test_gpu_feature_configs import CASES

pytestmark = pytest.mark.gpu

VAR = sdsp.VARIANTS


def _spec(seed, frames, bins=1025):
    rng = np.random.default_rng(seed)
    return (rng.random((frames, bins), dtype=np.float32) ** 4 * np.float32(50)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _cfgs(opts):
    c, o = sdsp.default_config(), oracle.default_config()
    for k, v in opts.items():
        setattr(c, k, v)
        setattr(o, k, v)
    return c, o


def _first_diff(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return f"shape {a.shape} vs {b.shape}"
    i = np.argwhere(_bits(a) != _bits(b))
    return f"{len(i)} of {a.size} differ, first at {tuple(i[0])}: {a[tuple(i[0])]!r} vs {b[tuple(i[0])]!r}"


def check_track(spec, got, meta, sr, hop, ocfg):
    """Every stage of one track against the oracle export, in pipeline order (the first assertion
    that fails names the first stage that differs)."""
    F = spec.shape[0]
    ref = units.tempo_stages(spec, sr, hop, ocfg)
    present = [VAR[v] for v in range(5) if meta["present"][v]]
    assert present == list(ref), (present, list(ref))
    for v, name in enumerate(VAR[:4]):
        if name in ref:
            assert (meta["bs"][v], meta["be"][v]) == (ref[name]["s"], ref[name]["e"]), name
            assert meta["band_on"][v]
    # k_features
    for v, name in enumerate(VAR[:4]):
        if name not in ref:
            continue
        r = ref[name]
        assert _same(got["E"][v], r["energy"]), ("E", name, _first_diff(got["E"][v], r["energy"]))
        assert _same(got["H"][v], r["hfc"]), ("H", name, _first_diff(got["H"][v], r["hfc"]))
        assert _same(got["SFX"][v], r["sfx_raw"]), ("SFX", name, _first_diff(got["SFX"][v], r["sfx_raw"]))
    sfo = units.spectral_flux_curve(spec)
    assert _same(got["SFO"], sfo), ("SFO", _first_diff(got["SFO"], sfo))
    if "mel" in ref:
        assert meta["n_mels"] == ref["mel"]["e"]
        assert _same(got["MEL"].T, ref["mel"]["melf"]), ("MEL", _first_diff(got["MEL"].T, ref["mel"]["melf"]))
    # k_novelty / k_mel_flux / k_mel_norm; nov_sum is the curve's sequential f32 sum, the numerator of
    # the mean fft_tempogram removes (sum / len in f32 on both sides)
    for name in present:
        nov = ref[name]["nov"]
        assert len(nov) == F - 1
        assert _same(got["nov"][name], nov), ("nov", name, _first_diff(got["nov"][name], nov))
        seq = np.cumsum(nov, dtype=np.float32)[-1]
        assert _bits(got["nov_sum"][name]) == _bits(seq), ("nov_sum", name, got["nov_sum"][name], seq)
        assert _bits(got["nov_sum"][name] / np.float32(F - 1)) == _bits(seq / np.float32(F - 1))
    # k_acf_tempogram, k_fft_tempogram: (bpm, value) pairs in order
    for name in present:
        assert meta["NB"] == len(ref[name]["acf"])
        assert _same(got["acf"][name], ref[name]["acf"]), ("acf", name, _first_diff(got["acf"][name], ref[name]["acf"]))
        assert _same(got["fft"][name], ref[name]["fft"]), ("fft", name, _first_diff(got["fft"][name], ref[name]["fft"]))
    return ref


def _same_track(a, b):
    for k in ("E", "H", "SFX", "SFO", "MEL"):
        if not _same(a[k], b[k]):
            return k
    for k in ("nov", "acf", "fft"):
        if list(a[k]) != list(b[k]) or not all(_same(a[k][n], b[k][n]) for n in a[k]):
            return k
    if any(_bits(a["nov_sum"][n]) != _bits(b["nov_sum"][n]) for n in a["nov_sum"]):
        return "nov_sum"
    return None


COUNTS = [2, 3, 6, 17, 63, 64, 65, 252, 253, 254, 505]
_RAGGED = None


def ragged():
    """One ragged call over COUNTS (find_track, tile_pfx, frame 0 without a predecessor): FT_STEP =
    252 frames per k_features tile, 63 frames per wave plus the helper lane, curves shorter than
    k_novelty's 16-frame local mean and 5-frame smoothing."""
    global _RAGGED
    if _RAGGED is None:
        specs = [_spec(100 + F, F) for F in COUNTS]
        meta, tracks = sdsp.debug_tempo_stages(specs)
        _RAGGED = (specs, meta, tracks)
    return _RAGGED


@pytest.mark.parametrize("k", range(len(COUNTS)), ids=[str(F) for F in COUNTS])
def test_ragged_call_against_oracle(k):
    specs, meta, tracks = ragged()
    assert meta["present"] == [1, 1, 1, 1, 1] and meta["n_mels"] == 40 and meta["NB"] == 201
    ref = check_track(specs[k], tracks[k], meta, 44100, 512, oracle.default_config())
    # the oracle gives no FFT entry below 63 frames and 2 at 63; 201 ACF entries whatever the length
    n_fft = {F: 0 for F in (2, 3, 6, 17)}
    n_fft[63] = 2
    if COUNTS[k] in n_fft:
        assert all(len(tracks[k]["fft"][n]) == n_fft[COUNTS[k]] == len(ref[n]["fft"]) for n in VAR)
    assert all(len(tracks[k]["acf"][n]) == 201 for n in VAR)


def test_single_track_calls_equal_the_ragged_call():
    specs, meta, tracks = ragged()
    for k, F in enumerate(COUNTS):
        m1, t1 = sdsp.debug_tempo_stages([specs[k]])
        assert m1 == meta
        assert _same_track(t1[0], tracks[k]) is None, (F, _same_track(t1[0], tracks[k]))


def test_zero_rows_constant_and_repeating_frames():
    """Rows of exact zeros inside a random track; a constant spectrogram and a track whose frames
    repeat: their novelty is 0 everywhere, every tempogram value ties and the lists keep the grid's
    order (the oracle's stable sort)."""
    a = _spec(31, 70)
    a[[0, 5, 6, 33, 69]] = 0.0
    b = np.full((66, 1025), 0.37, np.float32)
    c = np.tile(_spec(32, 1), (130, 1))
    specs = [a, b, c]
    meta, tracks = sdsp.debug_tempo_stages(specs)
    cfg = oracle.default_config()
    for s, t in zip(specs, tracks):
        check_track(s, t, meta, 44100, 512, cfg)
    for t in tracks[1:]:
        for n in VAR:
            assert not t["nov"][n].any() and not t["acf"][n][:, 1].any() and not t["fft"][n][:, 1].any()
            assert np.all(np.diff(t["acf"][n][:, 0]) > 0) and np.all(np.diff(t["fft"][n][:, 0]) > 0)
    # 130 frames: the slowest tempi's lags exceed the curve; still 201 entries
    assert len(tracks[2]["acf"]["full"]) == 201


@pytest.mark.parametrize("case", sorted(CASES))
def test_feature_configs(case):
    """test_gpu_feature_configs.py's cases (mel counts and ranges, mel k 1 and 3, bands moved, high
    band to Nyquist, superflux k 2 and 6: the runtime-K k_features instantiations, no band fusion, no
    mel) on one 65-frame and one 253-frame track."""
    cfg, ocfg = _cfgs(CASES[case])
    specs = [_spec(400, 65), _spec(401, 253)]
    meta, tracks = sdsp.debug_tempo_stages(specs, config=cfg)
    for s, t in zip(specs, tracks):
        check_track(s, t, meta, 44100, 512, ocfg)


@pytest.mark.parametrize("sr", [22050, 48000])
def test_sample_rates(sr):
    """Other sample rates move every band and mel edge across k_features' 8-bin chunk flags."""
    spec = _spec(500 + sr, 65)
    meta, tracks = sdsp.debug_tempo_stages([spec], sample_rate=sr)
    check_track(spec, tracks[0], meta, sr, 512, oracle.default_config())


@pytest.mark.parametrize("L", [4095, 4096, 4097, 8192, 8193])
def test_tempogram_sizes(L):
    """Curves of F - 1 = L values: 4095 / 4096 / 4097 around k_acf_tempogram's ACF_CH = 4096 chunk
    and its halo; 8192 the last size of k_fft_tempogram<LDS>, 8193 the global-scratch instantiation."""
    spec = _spec(600 + L, L + 1)
    meta, tracks = sdsp.debug_tempo_stages([spec])
    check_track(spec, tracks[0], meta, 44100, 512, oracle.default_config())


def test_acf_global_path_by_grid_size():
    """bpm_resolution 0.5: NB = 401 BPMs > 256 threads, k_acf_tempogram's global path."""
    cfg, ocfg = _cfgs(dict(bpm_resolution=0.5))
    specs = [_spec(700, 130), _spec(701, 600)]
    meta, tracks = sdsp.debug_tempo_stages(specs, config=cfg)
    assert meta["NB"] == 401
    for s, t in zip(specs, tracks):
        check_track(s, t, meta, 44100, 512, ocfg)


def test_acf_global_path_by_lag():
    """96 kHz, hop 256, min_bpm 20: lag 1125 > ACF_HMAX = 1024, the global path again (NB = 221)."""
    cfg, ocfg = _cfgs(dict(min_bpm=20.0))
    specs = [_spec(710, 1300), _spec(711, 4200)]
    meta, tracks = sdsp.debug_tempo_stages(specs, sample_rate=96000, hop=256, config=cfg)
    assert meta["NB"] == 221
    for s, t in zip(specs, tracks):
        check_track(s, t, meta, 96000, 256, ocfg)
