"""The programme loudness tests' tracks and their reference values (tests/r128_ref.py), built once and
shared by tests/test_r128_core.py (the host core) and tests/test_gpu_r128.py (the kernels).

SMALL: 16 kHz (step 1,600), the lengths around every block size and the branches of the definition.
ODD:   11,025 Hz (step 1,102, no multiple of the step kernel's 32-sample staging chunk).
WIDE:  8 kHz (step 800), lengths around one and two of the step kernel's 512-step workgroups and
       around the peak kernel's 1,024-sample tile."""
import numpy as np

import r128_ref as R
from test_r128_ref import _noise, quarter_rate_sine, two_level

f32 = np.float32
ALL = R.LOUDNESS | R.TRUE_PEAK | R.CURVES


def _spiked(n, at, seed):
    x = _noise(n, 0.05, seed)
    x[at] = f32(0.9)
    return x


def small():
    sr, st = 16000, 1600
    lengths = (1, 11, st - 1, st, st + 1, 2 * st, 4 * st - 1, 4 * st, 4 * st + 1, 30 * st - 1, 30 * st, 30 * st + 1, 33 * st + 7)
    xs = [_noise(n, 0.1, 4100 + k) for k, n in enumerate(lengths)]
    tags = ["len%d" % n for n in lengths]
    xs += [np.zeros(31 * st, f32), _noise(31 * st + 5, 1e-5, 4150), two_level(sr), _spiked(4 * st + 2, 3, 4151),
           _spiked(4 * st + 2, 4 * st - 2, 4152), quarter_rate_sine(), _noise(40 * st + 3, 0.5, 4153)]
    tags += ["zero", "under_abs_gate", "two_level", "spike_first", "spike_last", "quarter_sine", "loud"]
    return sr, xs, tags


def odd():
    sr, st = 11025, 1102
    lengths = (st - 1, 4 * st, 4 * st + 31, 31 * st + 1, 37 * st + 33)
    return sr, [_noise(n, 0.1, 4200 + k) for k, n in enumerate(lengths)], ["len%d" % n for n in lengths]


def wide():
    sr, st = 8000, 800
    lengths = (1023, 1024, 1025, 2049, 511 * st + 799, 512 * st, 513 * st, 1024 * st + 1, 1025 * st + 3)
    return sr, [_noise(n, 0.1, 4300 + k) for k, n in enumerate(lengths)], ["len%d" % n for n in lengths]


SETS = {"small": small, "odd": odd, "wide": wide}
_CACHE = {}


def case(name):
    """(sample rate, tracks, tags, reference of the full request)."""
    if name not in _CACHE:
        sr, xs, tags = SETS[name]()
        _CACHE[name] = (sr, xs, tags, R.measure(xs, sr, ALL))
    return _CACHE[name]


def masked(ref, what):
    """The reference of a request with fewer bits, from the full one's (the fields are independent)."""
    r = dict(ref)
    if not what & R.TRUE_PEAK:
        r.update(true_peak=f32(0.0), true_peak_dbtp=R.NEG_INF)
    if not what & R.CURVES:
        r.update(momentary=np.zeros(0, f32), short_term=np.zeros(0, f32))
    if not what & R.LOUDNESS:
        r.update(has_integrated=0, has_range=0, integrated_lufs=R.NEG_INF, range_lu=f32(0), range_low_lufs=f32(0),
                 range_high_lufs=f32(0), max_momentary_lufs=R.NEG_INF, max_short_term_lufs=R.NEG_INF, n_steps=0,
                 n_momentary=0, n_short_term=0, n_gated_momentary=0, n_gated_short_term=0)
    return r


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32).astype(np.int64)


def assert_equal(got, want, tag):
    """Every field of an r128 dict (sdsp.r128_to_dict, or the core harness's) against the reference, bit for bit."""
    for k in R.INTS:
        assert int(got[k]) == int(want[k]), (tag, k, got[k], want[k])
    for k in R.FLOATS:
        assert int(bits(got[k])[0]) == int(bits(want[k])[0]), (tag, k, got[k], want[k])
    for k in ("shelf", "highpass", "momentary", "short_term"):
        assert np.array_equal(bits(got[k]), bits(want[k])), (tag, k)
