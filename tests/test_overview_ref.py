"""tests/overview_ref.py, the GPU overview tests' reference, pinned on the four golden WAVs (CPU
only): over all columns the extrema of smin / smax are the signal's, the maximum over columns and
bands is the spectrogram's, and the two request forms agree where they describe one partition
(columns = F against frames_per_column = 1)."""
import os

import numpy as np
import pytest

import oracle
import overview_ref
import parity

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WAVS = ("120bpm_4bar.wav", "128bpm_4bar.wav", "cmajor_scale.wav", "mixed_silence.wav")

_chain = {}


def chain(name):
    if name not in _chain:
        x, sr = parity.load_wav(os.path.join(GOLDEN, name))
        _chain[name] = (x, sr, overview_ref.signal_and_mags(x, sr, oracle.default_config()))
    return _chain[name]


@pytest.mark.parametrize("name", WAVS)
def test_reference_on_golden_wavs(name):
    x, sr, ch = chain(name)
    status, first, sig, mags = ch
    assert status == 0 and sig.size > 2048 and mags.shape[0] == (sig.size - 2048) // 512 + 1
    cfg = oracle.default_config()
    F = mags.shape[0]
    for kw in (dict(columns=256), dict(columns=1), dict(frames_per_column=7), dict(frames_per_column=1)):
        o = overview_ref.overview_ref(x, sr, cfg, chain=ch, **kw)
        assert o["status"] == 0 and o["n_frames"] == F and o["n_samples"] == sig.size and o["first_sample"] == first
        assert o["n_columns"] == len(o["smin"]) == len(o["high"]) > 0
        assert o["smax"].max() == sig.max() and o["smin"].min() == sig.min(), kw
        assert max(o["low"].max(), o["mid"].max(), o["high"].max()) == mags.max(), kw
        assert np.all(o["smin"] <= o["smax"])
        assert o["band_bins"] == [11, 185]
    a = overview_ref.overview_ref(x, sr, cfg, chain=ch, columns=F)
    b = overview_ref.overview_ref(x, sr, cfg, chain=ch, frames_per_column=1)
    overview_ref.assert_equal(a, b, name)
    # one frame per column: a column's band maxima are that row's
    assert np.array_equal(b["low"], mags[:, :11].max(axis=1)) and np.array_equal(b["high"], mags[:, 185:].max(axis=1))
    # the first column's samples are the first hop, the last column's run to the end
    assert b["smax"][0] == sig[:512].max() and b["smin"][-1] == sig[(F - 1) * 512:].min()


def test_reference_band_and_zero_conventions():
    sig = np.zeros(4096, np.float32)
    sig[5], sig[600] = -0.0, 0.25
    mags = np.arange(5 * 1025, dtype=np.float32).reshape(5, 1025)
    o = overview_ref.envelope(sig, mags, 2048, 512, 44100, frames_per_column=1, low_max_hz=0.0, mid_max_hz=30000.0)
    assert o["band_bins"] == [0, 1025] and not o["low"].any() and not o["high"].any()
    assert np.array_equal(o["mid"], mags.max(axis=1))
    assert np.signbit(o["smin"][0]) and o["smin"][0] == 0.0 and not np.signbit(o["smax"][0])  # -0 < +0
    assert o["smax"][1] == 0.25 and not np.signbit(o["smin"][1])
    o = overview_ref.envelope(sig[:2047], mags[:0], 2048, 512, 44100, columns=3)
    assert o["n_columns"] == 0 and o["n_frames"] == 0 and o["smin"].size == 0
