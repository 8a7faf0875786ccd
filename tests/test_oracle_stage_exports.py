"""The oracle's stage exports (oracle/units.py: tempo_stages, spectral_flux_curve, key_stages, key_vote,
tempo_select, multires_fuse) pinned against exports that are already pinned.  The stage tests on the
GPU (test_gpu_tempo_stages.py, test_gpu_key_stages.py, test_gpu_key_vote.py, test_gpu_tempo_select.py,
test_gpu_multires_stages.py) compare kernels with these exports, so the exports themselves must be the
arithmetic the whole-track oracle runs: they are taken from inside tempogram_impl, multi_resolution
and analyze and from the key conditioning analyze calls, not restated.
"""
import numpy as np
import pytest

import oracle
import synth
import units


def _spec(seed, frames, bins):
    rng = np.random.default_rng(seed)
    return (rng.random((frames, bins)) ** 4 * 50).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("frames", [2, 3, 17, 65, 130])
def test_full_variant_is_novelty_full(frames):
    m = _spec(11 + frames, frames, 1025)
    st = units.tempo_stages(m)
    assert list(st) == ["full", "low", "mid", "high", "mel"]
    assert _same(st["full"]["nov"], oracle.novelty_full(m))
    assert (st["full"]["s"], st["full"]["e"]) == (0, 1025)
    assert st["mel"]["melf"].shape == (frames, 40) and len(st["mel"]["nov"]) == frames - 1


@pytest.mark.parametrize("frames", [2, 17, 65])
def test_pieces_are_the_unit_novelties(frames):
    """The full band's pieces are the unit exports: the normalised superflux, and the raw energies
    and HFC whose normalised positive differences are energy_flux_novelty / hfc_novelty; the raw
    superflux divided by its maximum is the normalised one."""
    m = _spec(23 + frames, frames, 1025)
    f = units.tempo_stages(m)["full"]
    assert _same(f["sf"], units.superflux_novelty(m, 4))

    def flux_norm(x):
        d = np.maximum(x[1:] - x[:-1], np.float32(0))
        mx = d.max() if d.size else np.float32(0)
        return d / mx if mx > np.float32(1e-10) else d

    assert _same(flux_norm(f["energy"]), units.energy_flux_novelty(m))
    assert _same(flux_norm(f["hfc"]), units.hfc_novelty(m, 44100))
    mx = f["sfx_raw"].max()
    assert _same(f["sfx_raw"] / mx if mx > np.float32(1e-10) else f["sfx_raw"], f["sf"])
    # the band variants' energies are the same fold over their own bins
    st = units.tempo_stages(m)
    for name in ("low", "mid", "high"):
        s, e = st[name]["s"], st[name]["e"]
        acc = np.zeros(frames, np.float32)
        for b in range(s, e):
            acc = acc + m[:, b] * m[:, b]
        assert _same(acc, st[name]["energy"]), name


def test_spectral_flux_curve_is_the_unit_novelty_before_normalisation():
    m = _spec(5, 33, 1025)
    c = units.spectral_flux_curve(m)
    assert c.shape == (32,) and _same(c / c.max(), units.spectral_flux_novelty(m))
    assert units.spectral_flux_curve(m[:1]).size == 0


@pytest.mark.parametrize("opts", [{}, {"key_spectrogram_smooth_margin": 8}, {"key_harmonic_mask_power": 1.0},
                                  {"enable_key_harmonic_mask": 0, "enable_key_spectrogram_time_smoothing": 1},
                                  {"key_hpcp_peaks_per_frame": 8}])
def test_key_stage_energies_are_the_sequential_fold(opts):
    """The returned energies are the f32 sequential sum of squares of the returned masked rows
    (extractor.rs:1133), and the default configuration's chroma is the pinned HPCP export's."""
    cfg = oracle.default_config()
    for k, v in opts.items():
        setattr(cfg, k, v)
    x = _spec(77, 30, 4097)
    x[7] = 0.0
    masked, chroma, energy = units.key_stages(x, 44100, cfg)
    if not opts:
        assert not np.array_equal(masked, x)
    sq = masked * masked
    ref = np.cumsum(sq, axis=1, dtype=np.float32)[:, -1]  # cumsum folds in order, one f32 rounding per step
    assert _same(energy, ref)
    if cfg.enable_key_harmonic_mask:  # a mask scales the row; time smoothing fills it from its neighbours
        assert energy[7] == 0.0 and not chroma[7].any()
    if not opts:
        ch, en = oracle.chroma("hpcp", masked, 44100, 8192)
        assert _same(ch, chroma) and _same(en, energy)


_KV_SYNTH = {"synth3": (3, 30.0, 1), "synth11": (11, 24.0, 0), "synth17": (17, 40.0, 1), "synth29": (29, 12.0, None)}


def _key_vote_audio(name):
    import os

    import parity

    if name in _KV_SYNTH:
        seed, sec, mode = _KV_SYNTH[name]
        return synth.make_track(seed, seconds=sec, mode=mode)[0], 44100
    return parity.load_wav(os.path.join(os.path.dirname(__file__), "golden", name))


@pytest.mark.parametrize("name", ["120bpm_4bar.wav", "128bpm_4bar.wav", "cmajor_scale.wav", "mixed_silence.wav",
                                  *_KV_SYNTH])
def test_key_vote_export_is_the_analysis_vote(name):
    """The whole-track oracle's key spectrogram (peak normalisation, trim, 8192-point STFT) through
    key_stages and then key_vote gives analyze's key fields, weights_used, used_segments and the
    trace's chroma / energy / weight checksums, bit for bit: the export is analyze's own vote."""
    x, sr = _key_vote_audio(name)
    rc, r, tr = oracle.analyze(x, sr, trace=True)
    assert rc == 0, r
    cfg = oracle.default_config()
    st_n, xn = oracle.normalize(x, 0, sr)
    assert st_n == 0
    ks = oracle.stft(xn[tr["trim_start"]:tr["trim_end"]], int(cfg.key_stft_frame_size), int(cfg.key_stft_hop_size))
    assert ks.shape[0] == tr["n_key_frames"] and ks.shape[0] > 0
    _, chroma, energy = units.key_stages(ks, sr, cfg)
    v = units.key_vote(chroma, energy, cfg)
    assert not v["err"]
    assert {"Minor" if v["mode"] else "Major": v["tonic"]} == r["key"]
    assert _same([v["confidence"], v["clarity"]], [r["key_confidence"], r["key_clarity"]])
    assert (int(v["weights_used"]), v["used_segments"]) == (tr["weights_used"], tr["used_segments"])

    def fold(a):  # the trace's checksums: sequential sums in double
        a = np.asarray(a, np.float64).ravel()
        return float(np.cumsum(a)[-1]) if a.size else 0.0

    cs = v["chroma_s"].astype(np.float64)
    assert fold(cs) == tr["chroma_sum"] and fold(cs * cs) == tr["chroma_sq"]
    assert fold(energy) == tr["energy_sum"] and fold(v["weights"]) == tr["weights_sum"]
    # the trace the export returns: one row of raw scores and a clarity per segment it voted on
    assert v["seg_raw"].shape[0] == v["seg_clarity"].size >= v["used_segments"]
    assert int((v["seg_clarity"] >= np.float32(cfg.key_segment_min_clarity)).sum()) == v["used_segments"]
    for raw, cl in zip(v["seg_raw"], v["seg_clarity"]):
        assert _same(oracle.key_clarity(units.key_from_raw(raw)[0]), cl)


@pytest.mark.parametrize("seed,bpm", [(7, 120.0), (8101, 126.0)])
def test_chained_exports_reproduce_the_base_estimate(seed, bpm):
    """The whole-track oracle's spectrogram (peak normalisation, trim, STFT) through the export:
    every variant's novelty through units._tempogram gives the export's own tempogram lists, and the
    estimate tempogram_impl made from them is the analysis trace's base estimate."""
    x = synth.make_track(seed, seconds=20.0, bpm=bpm)[0]
    rc, _, tr = oracle.analyze(x, 44100, trace=True)
    assert rc == 0 and tr["has_tempogram"]
    st_n, xn = oracle.normalize(x, 0)
    assert st_n == 0
    m = oracle.stft(xn[tr["trim_start"]:tr["trim_end"]], 2048, 512)
    cfg = oracle.default_config()
    st = units.tempo_stages(m, 44100, 512, cfg)
    est = units.tempo_stages_estimate()
    assert list(st) == ["full", "low", "mid", "high", "mel"]
    for name, v in st.items():
        fft = units._tempogram(0, v["nov"], 44100, 512, cfg.min_bpm, cfg.max_bpm, cfg.bpm_resolution)
        acf = units._tempogram(1, v["nov"], 44100, 512, cfg.min_bpm, cfg.max_bpm, cfg.bpm_resolution)
        assert _same(np.array(fft, np.float32).reshape(-1, 2), v["fft"]), name
        assert _same(np.array(acf, np.float32).reshape(-1, 2), v["acf"]), name
    base = tr["base"]
    assert est[0] > 0 and _same(est[:2], base[:2]) and est[2] == base[2], (est, base)


# ---- the tempo decision stages: tempo_select and multires_fuse are the functions tempogram_impl,
# multi_resolution and analyze call, so over the whole-track oracle's own lists they give its results ----
_FIXTURES = ["120bpm_4bar.wav", "128bpm_4bar.wav", "cmajor_scale.wav", "mixed_silence.wav"]


def _variants(cfg, st):
    import tempo_select_cases as S

    w = S.weights(cfg)
    return [(n, w[n], v["fft"], v["acf"]) for n, v in st.items()]


def _select(m, sr, hop, cfg):
    st = units.tempo_stages(m, sr, hop, cfg)
    est = units.tempo_stages_estimate()
    return st, est, units.tempo_select(_variants(cfg, st), cfg.min_bpm, cfg.max_bpm, cfg.bpm_resolution, cfg)


@pytest.mark.parametrize("what", _FIXTURES + ["spec:130", "spec:301"])
def test_tempo_select_over_stage_lists_is_the_stage_estimate(what):
    """tempo_select over the lists tempo_stages exports equals the estimate tempogram_impl made from
    them, bit for bit; on the fixtures also analyze's base estimate, candidates and gate decision."""
    import os

    import parity

    cfg = oracle.default_config()
    if what.startswith("spec:"):
        m, sr, tr = _spec(int(what[5:]), int(what[5:]), 1025), 44100, None
    else:
        x, sr = parity.load_wav(os.path.join(os.path.dirname(__file__), "golden", what))
        rc, _, tr = oracle.analyze(x, sr, trace=True)
        assert rc == 0 and tr["has_tempogram"]
        _, xn = oracle.normalize(x, 0, sr)
        m = oracle.stft(xn[tr["trim_start"]:tr["trim_end"]], 2048, 512)
    st, est, sel = _select(m, sr, 512, cfg)
    assert sel is not None and est[0] > 0
    assert _same([sel["bpm"], sel["conf"]], est[:2]) and sel["agree"] == est[2]
    if tr is not None and tr["has_tempogram"]:
        assert _same(est[:2], tr["base"][:2]) and est[2] == tr["base"][2]
        bc = np.array(tr["base_cands"], np.float32).reshape(-1, 4)
        assert _same(sel["cands"][:len(bc)], bc)
        assert sel["ambiguous"] == tr["ambiguous"]


@pytest.mark.parametrize("seed,bpm", [(301, 90.0), (306, 188.0), (319, 198.0), (310, 180.5)])
def test_multires_fuse_over_hop_lists_is_the_escalation(seed, bpm):
    """On escalating tracks, the candidate lists tempogram_impl gives at hops 256, 512 and 1024 (each
    through tempo_stages and tempo_select, truncated as multi_resolution truncates them) and the hop-512
    novelty, through multires_fuse, give analyze's multi-resolution estimate and acceptance, bit for bit."""
    x = synth.make_track(seed, seconds=20.0, bpm=bpm)[0]
    rc, _, tr = oracle.analyze(x, 44100, trace=True)
    assert rc == 0 and tr["ambiguous"] and tr["ran_mr"]
    cfg = oracle.default_config()
    _, xn = oracle.normalize(x, 0)
    xt = xn[tr["trim_start"]:tr["trim_end"]]
    top_k = int(cfg.tempogram_multi_res_top_k)
    aux_k = min(max(4 * top_k, 25), 200)
    lists, base, nov = {}, None, None
    for hop, k in ((256, aux_k), (512, top_k), (1024, aux_k)):
        st, _, sel = _select(oracle.stft(xt, 2048, hop), 44100, hop, cfg)
        lists[hop] = sel["cands"][:k]
        if hop == 512:
            assert _same([sel["bpm"], sel["conf"]], tr["base"][:2])
            base = (sel["bpm"], sel["conf"], sel["agree"], sel["trap_low"], sel["trap_high"])
            nov = st["full"]["nov"]
    r = units.multires_fuse(lists[256], lists[512], lists[1024], nov, 44100, base, cfg)
    assert r["ok"]
    assert _same([r["bpm"], r["conf"]], tr["mr"][:2]) and r["agree"] == tr["mr"][2], (r["bpm"], r["conf"], tr["mr"])
    assert r["used"] == tr["used_mr"]
