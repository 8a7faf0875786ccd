"""FLAC streams for the phased (CPU) and device decoder tests (TEST INFRASTRUCTURE), written with
tests/flac_enc.py: the stream classes of tests/test_flac_decode.py at small block sizes, the edge
block sizes, the damaged streams and the error blobs.  Every builder is cached: a test process
encodes each stream once.
"""
import functools

import numpy as np

import flac_enc as fe


def signal(n, bps, seed, step=1):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    amp = (1 << (bps - 1)) - 1
    x = 0.6 * np.sin(2 * np.pi * t * (220 + 30 * seed) / 44100) + 0.2 * rng.standard_normal(n) * 0.3
    v = np.clip(np.round(x * amp), -amp - 1, amp).astype(np.int64)
    return (v // step) * step


def _mono_stream(frames, bps=16, rate=44100, nch=1, **kw):
    return fe.stream(frames, rate, nch, bps, **kw)


@functools.lru_cache(maxsize=None)
def matrix():
    """[(name, bytes)]: every stream class of tests/test_flac_decode.py."""
    out = []
    for order in range(5):
        for method in (0, 1):
            frames = [fe.frame([signal(1024, 16, 10 + k)], 16, k,
                               specs=[{"type": "fixed", "order": order, "method": method, "porder": po}])
                      for k, po in enumerate([0, 2, 4])]
            out.append((f"fixed{order}_m{method}", _mono_stream(frames)))
    for order, prec, shift in [(1, 12, 10), (2, 15, 13), (8, 12, 9), (12, 14, 11), (32, 15, 14)]:
        rng = np.random.default_rng(order)
        coefs = [int(c) for c in rng.integers(-(1 << (prec - 2)), 1 << (prec - 2), size=order)]
        coefs[0] = (1 << shift) - 1
        s = signal(1152, 24, order)
        frames = [fe.frame([s], 24, 0, specs=[{"type": "lpc", "coefs": coefs, "prec": prec, "shift": shift,
                                               "method": 1, "porder": 3}])]
        out.append((f"lpc{order}", _mono_stream(frames, bps=24)))
    c = np.full(1152, -1234, np.int64)
    v, e, w = signal(1152, 16, 3), signal(2304, 16, 4), signal(2304, 16, 5, step=8)
    out.append(("const_verbatim_escape_wasted", _mono_stream([
        fe.frame([c], 16, 0, specs=[{"type": "constant"}]),
        fe.frame([v], 16, 1, specs=[{"type": "verbatim"}]),
        fe.frame([e], 16, 2, specs=[{"type": "fixed", "order": 2, "porder": 2, "escape": (0, 3)}]),
        fe.frame([w], 16, 3, specs=[{"type": "fixed", "order": 1, "wasted": 3}]),
        fe.frame([w], 16, 4, specs=[{"type": "verbatim", "wasted": 3}]),
        fe.frame([np.zeros(576, np.int64)], 16, 5, specs=[{"type": "fixed", "order": 0, "escape": (0,)}]),
    ])))
    for assign in ("indep", "left_side", "side_right", "mid_side"):
        for bps in (16, 24):
            frames = []
            for k in range(3):
                left, right = signal(1024, bps, 20 + k), signal(1024, bps, 40 + k)
                if k == 2:  # full-scale opposite extremes: the side channel needs bps + 1 bits
                    left[:8] = (1 << (bps - 1)) - 1
                    right[:8] = -(1 << (bps - 1))
                frames.append(fe.frame([left, right], bps, k, assign=assign,
                                       specs=[{"type": "fixed", "order": 2, "porder": 1},
                                              {"type": "lpc", "coefs": [3, -1], "prec": 6, "shift": 1}]))
            out.append((f"stereo_{assign}_{bps}", fe.stream(frames, 44100, 2, bps)))
    for bps in (8, 12, 20, 32):
        s = signal(1024, bps, bps)
        s[:4] = [(1 << (bps - 1)) - 1, -(1 << (bps - 1)), 0, -1]
        frames = [fe.frame([s], bps, 0, specs=[{"type": "verbatim"}]),
                  fe.frame([s], bps, 1, specs=[{"type": "fixed", "order": 1, "method": 1}], bps_mode="stream")]
        out.append((f"bps{bps}", _mono_stream(frames, bps=bps)))
    for nch in (3, 6, 8):
        chans = [signal(576, 16, 60 + c) for c in range(nch)]
        frames = [fe.frame(chans, 16, 0, specs=[{"type": "fixed", "order": c % 5} for c in range(nch)])]
        out.append((f"channels{nch}", fe.stream(frames, 44100, nch, 16)))
    sizes = [192, 576, 1152, 2304, 4608, 256, 512, 1024, 2048, 4096, 8192, 16384, 100, 7000]
    modes = ["stream", "code", "khz", "hz", "tens"]
    frames, pos = [], 0
    for k, n in enumerate(sizes):
        frames.append(fe.frame([signal(n, 16, 80 + k)], 16, pos, variable=True, rate=48000,
                               rate_mode=modes[k % len(modes)], specs=[{"type": "fixed", "order": 2, "porder": 0}]))
        pos += n
    frames.append(fe.frame([signal(256, 16, 99)], 16, pos, variable=True, bs_mode="8", rate=48000))
    frames.append(fe.frame([signal(4096, 16, 98)], 16, pos + 256, variable=True, bs_mode="16", rate=48000))
    out.append(("bs_and_rate_codes", fe.stream(frames, 48000, 1, 16)))
    s = signal(192, 16, 7)
    nums = [0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x1FFFFF, 0x200000, 0x3FFFFFF, 0x4000000, 0x7FFFFFFF]
    out.append(("large_frame_numbers", _mono_stream([fe.frame([s], 16, v, specs=[{"type": "verbatim"}]) for v in nums])))
    out.append(("id3_and_garbage", fe.stream([fe.frame([signal(2048, 16, 11)], 16, 0)], 22050, 1, 16, id3=True)
                + b"\x00\x01garbage"))
    return out


@functools.lru_cache(maxsize=None)
def edge_block_sizes():
    """[(name, bytes)]: one frame each, the block sizes at which the header or the residual layout
    takes another form."""
    def one(name, n, spec, **kw):
        return (name, _mono_stream([fe.frame([signal(n, 16, n % 97)], 16, 0, specs=[spec], **kw)]))

    return [
        one("bs1", 1, {"type": "verbatim"}),
        one("bs16", 16, {"type": "fixed", "order": 2}),
        one("bs17_code8", 17, {"type": "fixed", "order": 1}),
        one("bs4608", 4608, {"type": "fixed", "order": 2, "porder": 3}),
        one("bs65536_code16", 65536, {"type": "fixed", "order": 2, "porder": 4}),
        one("bs_eq_order", 4, {"type": "fixed", "order": 4}),
        one("bs_eq_lpc_order", 8, {"type": "lpc", "coefs": [5, -3, 2, 1, -1, 1, 0, 1], "prec": 5, "shift": 2}),
        one("empty_first_partition", 16, {"type": "fixed", "order": 4, "porder": 2}),
    ]


@functools.lru_cache(maxsize=None)
def many_frames(n):
    """One stream of n tiny VERBATIM frames (block size 16): n candidates, one per frame."""
    return _mono_stream([fe.frame([signal(16, 16, k)], 16, k, specs=[{"type": "verbatim"}]) for k in range(n)])


def false_header():
    """A frame header as six bytes: sync, block-size code 12 / rate code 9, mono 16-bit, number 0, CRC-8."""
    h = bytes([0xFF, 0xF8, 0xC9, 0x08, 0x00])
    return h + bytes([fe.crc8(h)])


@functools.lru_cache(maxsize=None)
def damaged():
    """[(name, bytes)]: streams whose decode skips or loses frames."""
    a, b, c = signal(1152, 16, 1), signal(1152, 16, 2), signal(1152, 16, 3)
    fa, fb, fc = (fe.frame([x], 16, k, specs=[{"type": "verbatim"}]) for k, x in enumerate((a, b, c)))
    out = []
    bad = bytearray(fb)
    bad[len(bad) // 2] ^= 0x10
    out.append(("crc16_middle", _mono_stream([fa, bytes(bad), fc])))
    bad = bytearray(fb)
    bad[4] ^= 0x01  # the frame number: the header CRC-8 no longer matches
    out.append(("crc8_middle", _mono_stream([fa, bytes(bad), fc])))
    r = fe.frame([signal(4096, 16, 5)], 16, 1, specs=[{"type": "fixed", "order": 2, "porder": 2}])
    out.append(("truncated_in_residual", _mono_stream([fa, r])[:-len(r) // 2]))
    # a false header in a VERBATIM payload: 16-bit samples are byte aligned behind the frame header
    # and the one-byte subframe header
    fh = false_header()
    planted = b.copy()
    planted[500:503] = [int.from_bytes(fh[2 * i:2 * i + 2], "big", signed=True) for i in range(3)]
    fp = fe.frame([planted], 16, 1, specs=[{"type": "verbatim"}])
    assert fh in fp
    out.append(("false_header_in_good_frame", _mono_stream([fa, fp, fc])))
    bad = bytearray(fp)
    bad[-10] ^= 0x40  # behind the planted header: the enclosing frame fails its CRC-16
    out.append(("false_header_in_bad_frame", _mono_stream([fa, bytes(bad), fc])))
    return out


def error_blobs():
    """[(name, bytes)]: what the decoders refuse."""
    return [("not_flac", b"fLaX" + bytes(40)), ("truncated_metadata", b"fLaC\x00\x00\x00\x22" + bytes(10)),
            ("missing_streaminfo", b"fLaC" + bytes([0x81, 0, 0, 4]) + bytes(4))]
