"""ALAC streams for the phased (CPU) and device decoder tests (TEST INFRASTRUCTURE), written with
tests/alac_enc.py: the stream classes of tests/test_alac_decode.py in both containers, the edge
frame lengths and packet shapes, the damaged files and the files the plan refuses.  Every builder
is cached: a test process encodes each stream once.
"""
import functools

import numpy as np

import alac_enc as ae

MONO_SPECS = [
    {"ch": [{"coefs": [], "den": 9}]},                                      # numactive 0
    {"ch": [{"na31": True}]},                                               # numactive 31: first-order
    {"ch": [{"coefs": [1024, -512, 256, -128], "den": 9, "pbf": 4}]},       # 4 taps
    {"ch": [{"coefs": [600, 300, -100, 50, 20, -10, 5, 2], "den": 9}]},     # 8 taps
    {"ch": [{"mode": 15, "coefs": [400, -200, 100, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7], "den": 10,
             "pbf": 2}]},                                                   # mode 15, 16 taps
    {"escape": True},                                                       # raw samples
]
TAPS4 = {"coefs": [800, -300, 100, 20], "den": 9}


def sig(n, bits, seed, amp=0.5, noise=0.05, silence=()):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = amp * np.sin(2 * np.pi * t * (180 + 23 * seed) / 44100) + noise * rng.standard_normal(n)
    top = (1 << (bits - 1)) - 1
    v = np.clip(np.round(x * top), -top - 1, top).astype(np.int64)
    for a, b in silence:
        v[a:b] = 0
    return v


def packets(cfg, chans, specs):
    """Channel arrays split into frame_length packets, one spec per packet (cycled)."""
    n = len(chans[0])
    return [ae.frame(cfg, [c[s:s + cfg.frame_length] for c in chans], [specs[k % len(specs)]])
            for k, s in enumerate(range(0, n, cfg.frame_length))]


def _chunks(npk):
    return [1] * npk if npk < 3 else [2] + [1] * (npk - 2)


def both(name, cfg, pk, n):
    """The packets in CAF and in ISO MP4 (several chunk runs)."""
    return [(name + ".caf", ae.caf(cfg, pk, n)), (name + ".m4a", ae.mp4(cfg, pk, _chunks(len(pk))))]


@functools.lru_cache(maxsize=None)
def matrix():
    """[(name, bytes)]: every stream class, in both containers.  frame_length <= 1024 throughout."""
    out = []
    cfg = ae.Config(bit_depth=16, channels=1, frame_length=1024)
    s = sig(6 * 1024 + 333, 16, 1, silence=[(2100, 2900), (5000, 5003)])  # zero runs; a partial last packet
    out += both("mono16_specs", cfg, packets(cfg, [s], MONO_SPECS), s.size)
    for mix in [(0, 0), (2, 1), (3, -2)]:
        cfg = ae.Config(bit_depth=16, channels=2, frame_length=1024, sample_rate=48000)
        l = sig(3000, 16, 2, amp=0.4)
        r = (0.7 * l + sig(3000, 16, 3, amp=0.1)).astype(np.int64)
        ch = [TAPS4, {"coefs": [900, -400], "den": 9, "mode": 15}]
        pk = packets(cfg, [l, r], [{"mix": mix, "ch": ch}, {"escape": True}, {"mix": mix, "ch": ch[::-1]}])
        out += both(f"stereo16_mix{mix[0]}_{mix[1]}", cfg, pk, 3000)
    for bits, shift, nch in [(20, 0, 1), (24, 0, 2), (24, 1, 2), (24, 2, 2), (32, 1, 1), (32, 2, 1)]:
        cfg = ae.Config(bit_depth=bits, channels=nch, frame_length=1024, sample_rate=32000 if bits == 24 else 44100)
        chans = [sig(2500, bits, 7 + c, amp=0.3 if nch == 2 else 0.6) for c in range(nch)]
        ch = [{"coefs": [700, -200, 60, -10], "den": 9}] * nch
        pk = packets(cfg, chans, [{"shift": shift, "mix": (2, 1), "ch": ch}, {"escape": True}])
        out += both(f"bits{bits}_shift{shift}", cfg, pk, 2500)
    cfg = ae.Config(bit_depth=16, channels=1, frame_length=512, kb=10)
    rng = np.random.default_rng(5)
    s = rng.integers(-32768, 32768, 2048).astype(np.int64)  # white noise: Golomb escapes
    s[100:110] = [32767, -32768] * 5
    pk = packets(cfg, [s], [{"ch": [{"coefs": [], "den": 9}]}, {"ch": [{"coefs": [512, -256], "den": 9}]}])
    out += both("noise_escapes", cfg, pk, s.size)
    cfg = ae.Config(bit_depth=16, channels=1, frame_length=1024)
    s = sig(3 * 1024, 16, 9, silence=[(10, 1800), (2000, 2001), (2500, 3072)])  # runs across and to the end of packets
    out += both("zero_runs", cfg, packets(cfg, [s], [{"ch": [TAPS4]}, {"ch": [{"na31": True}]}]), s.size)
    return out


def _bad_tag(p):
    bad = bytearray(p)
    bad[0] = 0xA0  # element tag 5 (PCE): not decodable -> the packet is skipped
    return bytes(bad)


@functools.lru_cache(maxsize=None)
def edges():
    """[(name, bytes, decoded packets, skipped packets)]: files the plan accepts."""
    out = []

    def add(name, cfg, pk, n, dec, skp):
        for nm, data in both(name, cfg, pk, n):
            out.append((nm, data, dec, skp))

    spec = [{"ch": [TAPS4]}]
    cfg = ae.Config(bit_depth=16, channels=1, frame_length=16)
    s = sig(100, 16, 21)
    add("fl16", cfg, packets(cfg, [s], spec), 100, 7, 0)
    cfg = ae.Config(bit_depth=16, channels=2, frame_length=512)
    l, r = sig(1100, 16, 22), sig(1100, 16, 23)
    add("fl512", cfg, packets(cfg, [l, r], [{"mix": (2, 1), "ch": [TAPS4, TAPS4]}]), 1100, 3, 0)
    cfg = ae.Config(bit_depth=16, channels=1, frame_length=1024)
    s = sig(1025, 16, 24)
    add("last_packet_1", cfg, packets(cfg, [s], spec), 1025, 2, 0)
    s = sig(1024 + 3, 16, 25)  # the last packet holds 3 samples <= numactive (4 and 8 taps)
    add("n_le_numactive4", cfg, packets(cfg, [s], spec), s.size, 2, 0)
    add("n_le_numactive8", cfg, packets(cfg, [s], [MONO_SPECS[3]]), s.size, 2, 0)
    out.append(("no_packets.caf", ae.caf(cfg, [], 0), 0, 0))
    s = sig(3 * 1024, 16, 26)
    pk = packets(cfg, [s], spec)
    add("empty_packet", cfg, [pk[0], b"", pk[2]], 2048, 2, 1)
    add("damaged_first", cfg, [_bad_tag(pk[0]), pk[1], pk[2]], 2048, 2, 1)
    add("damaged_middle", cfg, [pk[0], _bad_tag(pk[1]), pk[2]], 2048, 2, 1)
    add("damaged_last", cfg, [pk[0], pk[1], _bad_tag(pk[2])], 2048, 2, 1)
    add("truncated_packet", cfg, [pk[0], pk[1][:len(pk[1]) // 2], pk[2]], 2048, 2, 1)
    return out


@functools.lru_cache(maxsize=None)
def refused():
    """[(name, bytes, text in the host's error)]: files whose plan fails with the host's error."""
    cfg = ae.Config(bit_depth=16, channels=1, frame_length=1024)
    s = sig(2048, 16, 27)
    pk = packets(cfg, [s], [{"ch": [TAPS4]}])
    m4a = ae.mp4(cfg, pk, [1, 1])
    return [("packet_outside.m4a", m4a[:len(m4a) - len(pk[1]) // 2], "ALAC packet outside the file"),
            ("aac.m4a", ae.mp4(ae.Config(), [b"\x00" * 10], [1], codec=b"mp4a"), "AAC")]


@functools.lru_cache(maxsize=None)
def many_packets(n):
    """One CAF file of n packets of 16 raw samples each."""
    cfg = ae.Config(bit_depth=16, channels=1, frame_length=16)
    s = sig(16 * n, 16, n)
    return ae.caf(cfg, packets(cfg, [s], [{"escape": True}]), s.size)


@functools.lru_cache(maxsize=None)
def long_frames():
    """A file whose cookie declares frame_length 32768 (above the device bound): one full packet of
    raw samples and a partial one."""
    cfg = ae.Config(bit_depth=16, channels=1, frame_length=32768)
    s = sig(32768 + 64, 16, 31)
    return ae.mp4(cfg, packets(cfg, [s], [{"escape": True}, {"ch": [TAPS4]}]), [1, 1])


@functools.lru_cache(maxsize=None)
def passage(x, sample_rate=44100):
    """A float passage as 16-bit ALAC stereo in M4A (both channels the passage; fixed 4-tap specs)."""
    pcm = np.clip(np.round(np.frombuffer(x, np.float32) * 32767.0), -32768, 32767).astype(np.int64)
    cfg = ae.Config(bit_depth=16, channels=2, frame_length=4096, sample_rate=sample_rate)
    pk = packets(cfg, [pcm, pcm], [{"mix": (0, 0), "ch": [TAPS4, TAPS4]}])
    return ae.mp4(cfg, pk, _chunks(len(pk)))
