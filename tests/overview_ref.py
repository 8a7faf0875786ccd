"""The overview envelope (include/stratum_hip.h, sdsp_overview) in numpy, written from the
definition: the column plan in Python integers, the sample extrema and the band maxima as
reductions over the oracle's own normalised signal and spectrogram.  Nothing here knows how the
kernels split the work.

The only choice the definition leaves to a minimum or maximum is the sign of a zero where both
occur in a column; it is settled as the header says, -0 < +0, by reducing on order-preserving
integer keys of the f32 bits.
"""
import numpy as np

import oracle

ARRAYS = ("smin", "smax", "low", "mid", "high")
SCALARS = ("n_columns", "n_frames", "first_sample", "n_samples", "frame_size", "hop_size", "band_bins", "status")


def n_frames(n, frame_size, hop):
    return 0 if n < frame_size else (n - frame_size) // hop + 1


def column_starts(F, columns=0, frames_per_column=0):
    """f0(0) .. f0(C) as Python integers (C + 1 entries; [0] for F == 0)."""
    assert (columns > 0) != (frames_per_column > 0)
    if columns > 0:
        C = min(columns, F)
        return [c * F // C for c in range(C)] + [F] if C else [0]
    C = -(-F // frames_per_column)
    return [min(c * frames_per_column, F) for c in range(C)] + [F] if C else [0]


def band_bins(low_max_hz, mid_max_hz, frame_size, sample_rate):
    """(b1, b2): the edges go through f32 (the request's fields), the products through f64."""
    B = frame_size // 2 + 1

    def edge(hz):
        v = float(np.float32(hz)) * float(frame_size) / float(sample_rate)
        return B if v >= B else int(np.floor(v))

    b1 = min(B, edge(low_max_hz))
    return b1, min(B, max(b1, edge(mid_max_hz)))


def _keys(x):
    """u32 keys ascending in the f32 value, -0 below +0."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _unkeys(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def envelope(signal, mags, frame_size, hop, sample_rate, columns=0, frames_per_column=0, low_max_hz=250.0,
             mid_max_hz=4000.0):
    """The five arrays and C, F, (b1, b2) of one normalised, trimmed signal and its spectrogram."""
    signal = np.ascontiguousarray(signal, np.float32)
    n = signal.size
    F = n_frames(n, frame_size, hop)
    assert mags.shape == (F, frame_size // 2 + 1)
    f0 = column_starts(F, columns, frames_per_column)
    C = len(f0) - 1
    b1, b2 = band_bins(low_max_hz, mid_max_hz, frame_size, sample_rate)
    out = {"n_columns": C, "n_frames": F, "band_bins": [b1, b2]}
    if C == 0:
        out.update({k: np.zeros(0, np.float32) for k in ARRAYS})
        return out
    assert all(a < b for a, b in zip(f0, f0[1:])) and f0[0] == 0 and f0[-1] == F
    fr = np.array(f0[:-1], np.int64)
    keys = _keys(signal)
    out["smin"] = _unkeys(np.minimum.reduceat(keys, fr * hop))  # the last column runs to n
    out["smax"] = _unkeys(np.maximum.reduceat(keys, fr * hop))
    B = frame_size // 2 + 1
    for name, (a, b) in (("low", (0, b1)), ("mid", (b1, b2)), ("high", (b2, B))):
        if a == b:
            out[name] = np.zeros(C, np.float32)
        else:
            out[name] = np.maximum.reduceat(mags[:, a:b].max(axis=1), fr).astype(np.float32)
    return out


def signal_and_mags(x, sample_rate, cfg):
    """(status, first_sample, normalised trimmed signal, spectrogram) of one track from the oracle:
    the trim bounds of analyze's trace, normalize's samples, stft's magnitudes."""
    x = np.ascontiguousarray(x, np.float32)
    st = oracle.analyze(x, sample_rate, cfg, trace=True) if x.size else (1, "Invalid input: Empty audio samples", None)
    if st[0] != 0:
        return st[0], 0, None, None
    tr = st[2]
    xn = x
    if cfg.enable_normalization:
        s, xn = oracle.normalize(x, int(cfg.normalization), sample_rate)
        assert s == 0, xn
    sig = xn[tr["trim_start"]:tr["trim_end"]]
    return 0, int(tr["trim_start"]), sig, oracle.stft(sig, int(cfg.frame_size), int(cfg.hop_size))


def overview_ref(x, sample_rate, cfg, columns=0, frames_per_column=0, low_max_hz=250.0, mid_max_hz=4000.0, chain=None):
    """One track's overview as sdsp.analyze_batch_device_overview returns it.  `chain` is a
    signal_and_mags() result to share between requests."""
    status, first, sig, mags = chain if chain is not None else signal_and_mags(x, sample_rate, cfg)
    fs, hop = int(cfg.frame_size), int(cfg.hop_size)
    b1, b2 = band_bins(low_max_hz, mid_max_hz, fs, sample_rate)
    out = {"status": status, "frame_size": fs, "hop_size": hop, "band_bins": [b1, b2], "n_columns": 0, "n_frames": 0,
           "first_sample": 0, "n_samples": 0}
    out.update({k: np.zeros(0, np.float32) for k in ARRAYS})
    if status != 0:
        return out
    out.update(envelope(sig, mags, fs, hop, sample_rate, columns, frames_per_column, low_max_hz, mid_max_hz))
    out["first_sample"], out["n_samples"] = first, int(sig.size)
    return out


def assert_equal(got, want, what=""):
    """Every scalar field equal, every array equal bit for bit."""
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ARRAYS:
        g, w = np.asarray(got[k], np.float32), np.asarray(want[k], np.float32)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.nonzero(g.view(np.uint32) != w.view(np.uint32))[0]
        assert bad.size == 0, (what, k, int(bad.size), int(bad[0]), float(g[bad[0]]), float(w[bad[0]]))
