"""Seeded random Ogg Vorbis bitstreams for the device decoder's tests (TEST INFRASTRUCTURE).

tests/vorbis_enc.py encodes audio with one setup at block sizes 256 / 2048.  Bit equality between
two decoders does not need audio that sounds like anything: it needs valid bitstreams that reach
every decoder path.  This writer emits its own identification and setup headers from parameters
and audio packets of random valid symbols (floor Y values, classwords, VQ entries), following the
decoder's own read order (Vorbis I §4.3, §7.2, §8.6).  VQ values are a few units and the floor is
at most 1, so no block comes near the float range: every decode is finite (the generator's test
asserts that on the host decoder).

Pages are written here (page(), ogg()) rather than by vorbis_enc.ogg_stream, which puts every
packet on a page of its own: the matrix needs a packet across two pages, a page with a bad CRC and a
second logical stream.

matrix() is the list of (name, ogg bytes) the tests share; damaged() adds seeded truncations, bit
flips of the file (which the page CRC catches) and bit flips inside audio packets before paging
(which reach the packet decoder).
"""
import functools
import random
import struct

from vorbis_enc import LBitWriter, float32_pack, ilog, make_words


def _complete(n, short):
    a = (1 << (short + 1)) - n
    assert 0 <= a <= n
    return [short] * a + [short + 1] * (n - a)


class Book:
    def __init__(self, lengths, dims=1, lookup=None, ordered=False, sparse=False):
        self.lengths, self.dims, self.lookup, self.ordered, self.sparse = lengths, dims, lookup, ordered, sparse
        self.used = [i for i, ln in enumerate(lengths) if ln > 0]
        self.words = make_words(lengths) if len(self.used) > 1 else None

    def header(self, w):
        L = self.lengths
        w.put(0x564342, 24)
        w.put(self.dims, 16)
        w.put(len(L), 24)
        if self.ordered:
            w.put(1, 1)
            w.put(L[0] - 1, 5)
            cur, ln = 0, L[0]
            while cur < len(L):
                num = sum(1 for x in L[cur:] if x == ln)
                w.put(num, ilog(len(L) - cur))
                cur += num
                ln += 1
        else:
            w.put(0, 1)
            w.put(int(self.sparse), 1)
            for x in L:
                if self.sparse:
                    w.put(int(x > 0), 1)
                    if not x:
                        continue
                w.put(x - 1, 5)
        if self.lookup is None:
            w.put(0, 4)
            return
        typ, mn, dl, vbits, seq, mults = self.lookup
        w.put(typ, 4)
        w.put(float32_pack(mn), 32)
        w.put(float32_pack(dl), 32)
        w.put(vbits - 1, 4)
        w.put(seq, 1)
        for m in mults:
            w.put(m, vbits)

    def emit(self, w, rng):
        """One random used entry; returns it."""
        e = rng.choice(self.used)
        if self.words is None:
            w.put(0, 1)  # a single used entry: one bit, either value decodes it
        else:
            w.code(self.words[e], self.lengths[e])
        return e


def books(rng):
    return [
        Book([5] * 32),                                                              # 0 floor Y: dense
        Book(_complete(9, 3), dims=2),                                               # 1 classbook: 3 classes, 2 per word
        Book(_complete(25, 4) + [0, 0], dims=2, sparse=True,                         # 2 VQ lookup 1, 2 dims, unused entries
             lookup=(1, -2.0, 1.0, 3, 0, [0, 1, 2, 3, 4])),
        Book([3] * 8, dims=4, ordered=True,                                          # 3 VQ lookup 2, sequence_p, ordered
             lookup=(2, -3.5, 0.5, 3, 1, [rng.randrange(8) for _ in range(32)])),
        Book([0, 0, 1, 0], dims=1, sparse=True, lookup=(1, -1.0, 1.0, 2, 0, [0, 1, 2, 3])),  # 4 a single used entry
        Book([2, 2, 2, 2]),                                                          # 5 floor master book
        Book([1, 2, 3, 4, 4], ordered=True),                                         # 6 floor Y: ordered, mixed lengths
    ]


class Floor:
    def __init__(self, rng, multiplier, rangebits, part_class, classes):
        self.multiplier, self.rangebits, self.part_class, self.classes = multiplier, rangebits, part_class, classes
        count = sum(classes[c][0] for c in part_class)
        self.X = rng.sample(range(1, 1 << rangebits), count)

    def header(self, w):
        w.put(1, 16)
        w.put(len(self.part_class), 5)
        for c in self.part_class:
            w.put(c, 4)
        for dim, sub, master, subbooks in self.classes:
            w.put(dim - 1, 3)
            w.put(sub, 2)
            if sub:
                w.put(master, 8)
            assert len(subbooks) == 1 << sub
            for b in subbooks:
                w.put(b + 1, 8)
        w.put(self.multiplier - 1, 2)
        w.put(self.rangebits, 4)
        for x in self.X:
            w.put(x, self.rangebits)

    def packet(self, w, B, rng):
        rng_bits = ilog([256, 128, 86, 64][self.multiplier - 1] - 1)
        w.put(rng.randrange(1 << rng_bits), rng_bits)
        w.put(rng.randrange(1 << rng_bits), rng_bits)
        for c in self.part_class:
            dim, sub, master, subbooks = self.classes[c]
            cval = B[master].emit(w, rng) if sub else 0
            for _ in range(dim):
                b = subbooks[cval & ((1 << sub) - 1)]
                cval >>= sub
                if b >= 0:
                    B[b].emit(w, rng)


class Residue:
    def __init__(self, rtype, begin, end, psize, classbook, cascade):
        self.type, self.begin, self.end, self.psize, self.classbook, self.cascade = rtype, begin, end, psize, classbook, cascade

    def header(self, w):
        w.put(self.type, 16)
        w.put(self.begin, 24)
        w.put(self.end, 24)
        w.put(self.psize - 1, 24)
        w.put(len(self.cascade) - 1, 6)
        w.put(self.classbook, 8)
        for cl in self.cascade:
            bits = sum(1 << p for p, b in enumerate(cl) if b is not None)
            w.put(bits & 7, 3)
            w.put(int(bits >> 3 != 0), 1)
            if bits >> 3:
                w.put(bits >> 3, 5)
        for cl in self.cascade:
            for b in cl:
                if b is not None:
                    w.put(b, 8)

    def packet(self, w, B, rng, n2, skip):
        """The decoder's read order (host_vorbis / vorbis_core residue decode)."""
        cb = B[self.classbook]
        cw, classes = cb.dims, len(self.cascade)
        if self.type == 2:
            if all(skip):
                return
            size, sk = n2 * len(skip), [False]
        else:
            size, sk = n2, skip
        lb, le = min(self.begin, size), min(self.end, size)
        parts = (le - lb) // self.psize if le > lb else 0
        if parts == 0:
            return
        cls = [[0] * (parts + cw) for _ in sk]
        for ps in range(8):
            pc = 0
            while pc < parts:
                if ps == 0:
                    for j in range(len(sk)):
                        if sk[j]:
                            continue
                        temp = cb.emit(w, rng)
                        for i in range(cw - 1, -1, -1):
                            cls[j][i + pc] = temp % classes
                            temp //= classes
                i = 0
                while i < cw and pc < parts:
                    for j in range(len(sk)):
                        if sk[j]:
                            continue
                        b = self.cascade[cls[j][pc]][ps]
                        if b is None:
                            continue
                        vb = B[b]
                        count = self.psize // vb.dims if self.type == 0 else -(-self.psize // vb.dims)
                        for _ in range(count):
                            vb.emit(w, rng)
                    i += 1
                    pc += 1


class Setup:
    """channels 1 / 2 / 3, block sizes bs, residue type rtype.  Three modes (so the mode number takes
    two bits and 3 is out of range): 0 short, 1 long, 2 long through the short mapping."""

    def __init__(self, seed, channels, bs, rtype, rate=44100):
        rng = random.Random(seed)
        self.C, self.bs, self.rate = channels, bs, rate
        self.B = books(rng)
        lg0, lg1 = ilog(bs[0] // 2 - 1), ilog(bs[1] // 2 - 1)
        plain = (2, 0, 0, [0])        # class_sub 0
        master = (2, 1, 5, [-1, 0])   # a master book, sub-book 0 unused
        ordered = (1, 0, 0, [6])
        self.floors = [Floor(rng, 1, lg0 + 1, [0, 1], [plain, master]),   # X values past n/2 too
                       Floor(rng, 4, lg1, [0, 1, 2, 2], [plain, master, ordered])]
        two = [[None] * 8, [2] + [None] * 7, [2, None, 4] + [None] * 5]  # no pass | one | two passes
        alt = [[None] * 8, [3] + [None] * 7, [None, 3] + [None] * 6]
        mul = channels if rtype == 2 else 1
        self.residues = [Residue(rtype, bs[0] // 16 * mul, (bs[0] // 2 - bs[0] // 16) * mul, 8, 1, two),
                         Residue(rtype, bs[1] // 16 * mul, (bs[1] // 2 - bs[1] // 16) * mul, 8, 1, two),
                         Residue(1, 0, bs[1], 8, 1, alt)]  # end past n/2: clamped
        if channels == 1:
            coup, mux, subs = [], [0], [[(0, 0)], [(1, 1)]]
        elif channels == 2:
            coup, mux, subs = [(0, 1)], [0, 0], [[(0, 0)], [(1, 1)]]
        else:
            coup, mux, subs = [(0, 1), (2, 0)], [0, 0, 1], [[(0, 0), (1, 2)], [(1, 1), (0, 2)]]
        self.maps = [(coup, mux, subs[0]), (coup, mux, subs[1])]
        self.modes = [(0, 0), (1, 1), (1, 0)]

    def headers(self):
        idh = LBitWriter()
        idh.put(0, 32)
        idh.put(self.C, 8)
        idh.put(self.rate, 32)
        for _ in range(3):
            idh.put(0, 32)
        idh.put(ilog(self.bs[0]) - 1, 4)
        idh.put(ilog(self.bs[1]) - 1, 4)
        idh.put(1, 1)
        cw = LBitWriter()
        cw.put(0, 32)
        cw.put(0, 32)
        cw.put(1, 1)
        s = LBitWriter()
        s.put(len(self.B) - 1, 8)
        for b in self.B:
            b.header(s)
        s.put(0, 6)
        s.put(0, 16)
        s.put(len(self.floors) - 1, 6)
        for f in self.floors:
            f.header(s)
        s.put(len(self.residues) - 1, 6)
        for r in self.residues:
            r.header(s)
        s.put(len(self.maps) - 1, 6)
        for coup, mux, subs in self.maps:
            s.put(0, 16)
            s.put(int(len(subs) > 1), 1)
            if len(subs) > 1:
                s.put(len(subs) - 1, 4)
            s.put(int(bool(coup)), 1)
            if coup:
                s.put(len(coup) - 1, 8)
                for m, a in coup:
                    s.put(m, ilog(self.C - 1))
                    s.put(a, ilog(self.C - 1))
            s.put(0, 2)
            if len(subs) > 1:
                for c in range(self.C):
                    s.put(mux[c], 4)
            for fl, rs in subs:
                s.put(0, 8)
                s.put(fl, 8)
                s.put(rs, 8)
        s.put(len(self.modes) - 1, 6)
        for bf, mp in self.modes:
            s.put(bf, 1)
            s.put(0, 16)
            s.put(0, 16)
            s.put(mp, 8)
        s.put(1, 1)
        return [b"\x01vorbis" + idh.bytes(), b"\x03vorbis" + cw.bytes(), b"\x05vorbis" + s.bytes()]

    def packet(self, rng, mode_no, prev_long, next_long, unused, cut=None):
        """One audio packet of random valid symbols; unused: per channel, the floor's 'unused' flag.
        cut: "floor" / "residue" ends the packet inside that part."""
        w = LBitWriter()
        bits = lambda: len(w.out) * 8 + w.n
        w.put(0, 1)
        w.put(mode_no, ilog(len(self.modes) - 1))
        bf, mp = self.modes[mode_no]
        if bf:
            w.put(int(prev_long), 1)
            w.put(int(next_long), 1)
        n2 = self.bs[bf] // 2
        coup, mux, subs = self.maps[mp]
        hdr_end = bits()
        first_floor_end = None
        for c in range(self.C):
            w.put(int(not unused[c]), 1)
            if not unused[c]:
                self.floors[subs[mux[c]][0]].packet(w, self.B, rng)
            if first_floor_end is None:
                first_floor_end = bits()
        floor_end = bits()
        skip = list(unused)
        for m, a in coup:
            if not unused[m] or not unused[a]:
                skip[m] = skip[a] = False
        for sm, (fl, rs) in enumerate(subs):
            self.residues[rs].packet(w, self.B, rng, n2, [skip[c] for c in range(self.C) if mux[c] == sm])
        out = w.bytes()
        if cut == "floor":
            assert first_floor_end - hdr_end > 16  # the middle of the first channel's floor
            out = out[:max(1, (hdr_end + (first_floor_end - hdr_end) // 2) // 8)]
        elif cut == "residue":
            assert bits() - floor_end > 16
            out = out[:(floor_end + (bits() - floor_end) // 2) // 8]
        return out


_CRC = []
for _i in range(256):
    _r = _i << 24
    for _ in range(8):
        _r = ((_r << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if _r & 0x80000000 else (_r << 1) & 0xFFFFFFFF
    _CRC.append(_r)


def _crc(page):
    crc = 0
    for b in page:
        crc = ((crc << 8) & 0xFFFFFFFF) ^ _CRC[((crc >> 24) ^ b) & 0xFF]
    return crc


def page(serial, seq, granule, flags, lacing, payload, bad_crc=False):
    hdr = b"OggS" + bytes([0, flags]) + struct.pack("<qIII", granule, serial, seq, 0) + bytes([len(lacing)]) + bytes(lacing)
    pg = bytearray(hdr + payload)
    struct.pack_into("<I", pg, 22, _crc(pg) ^ (0x1234 if bad_crc else 0))
    return bytes(pg)


def _lacing(n):
    return [255] * (n // 255) + [n % 255]


def ogg(packets, granules, span=None, bad_crc=None, second_stream=False, serial=0x5EED):
    """One page per packet (headers at granule 0).  span: index of a packet (>= 255 bytes) written
    across two pages; bad_crc: index of a packet whose page fails its CRC; second_stream: pages of
    another logical stream between this one's."""
    out, seq, seq2 = [], 0, 0
    for i, (p, g) in enumerate(zip(packets, granules)):
        flags = (2 if i == 0 else 0) | (4 if i == len(packets) - 1 else 0)
        if i == span:
            assert len(p) >= 256
            k = (len(p) - 1) // 255 // 2 + 1  # whole 255-byte segments on the first page, at least one
            k = min(k, len(p) // 255)
            out.append(page(serial, seq, -1, flags & 2, [255] * k, p[:255 * k]))
            seq += 1
            out.append(page(serial, seq, g, 1 | (flags & 4), _lacing(len(p) - 255 * k), p[255 * k:]))
        else:
            out.append(page(serial, seq, g, flags, _lacing(len(p)), p, bad_crc=(i == bad_crc)))
        seq += 1
        if second_stream and i % 3 == 0:
            junk = bytes([7 * i % 251] * (40 + i % 17))
            out.append(page(serial ^ 0xABCDEF, seq2, 5 * i, 2 if seq2 == 0 else 0, _lacing(len(junk)), junk))
            seq2 += 1
    return b"".join(out)


MIXED = [0, 1, 0, 1, 1, 1, 0, 0]  # a long block after / before every (short, long) pair of neighbours


def stream(seed, channels, bs, rtype, pattern, specials=(), final=None, packet_flips=0, **paging):
    """pattern: block flags; specials: {position: kind} of extra packets put before the block at that
    position ("empty", "nonaudio", "badmode") or cuts of it ("cutfloor", "cutresidue"); final: the
    last granule relative to the decoded length (None: exact)."""
    S = Setup(seed, channels, bs, rtype)
    rng = random.Random(seed * 7919 + 1)
    specials = dict(specials)
    pk, gr, total, prev_n = [], [], 0, 0
    for k, bf in enumerate(pattern):
        sp = specials.get(k)
        if sp == "empty":
            pk.append(b"")
            gr.append(total)
        elif sp == "nonaudio":
            pk.append(bytes([0x81, 0x55, 0xAA]))
            gr.append(total)
        elif sp == "badmode":
            pk.append(bytes([0x06, 0x12, 0x34]))  # audio, mode number 3 of 3 modes
            gr.append(total)
        prev_long = bool(pattern[k - 1]) if k else True
        next_long = bool(pattern[k + 1]) if k + 1 < len(pattern) else True
        mode_no = 0 if not bf else (2 if k % 4 == 3 else 1)
        unused = [False] * channels
        if k % 5 == 2:
            unused[0] = True          # one side of a coupled pair (or the only channel)
        if k % 7 == 4:
            unused = [True] * channels
        if k % 11 == 6 and channels > 1:
            unused[-1] = True
        cut = {"cutfloor": "floor", "cutresidue": "residue"}.get(sp)
        if cut:
            unused = [False] * channels
        pk.append(S.packet(rng, mode_no, prev_long, next_long, unused, cut=cut))
        n = bs[bf]
        if prev_n:
            total += prev_n // 4 + n // 4
        prev_n = n
        gr.append(total)
    for _ in range(packet_flips):  # damage inside audio packets: the page CRCs stay valid
        i = rng.randrange(len(pk))
        if pk[i]:
            b = bytearray(pk[i])
            b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
            pk[i] = bytes(b)
    if final is not None:
        gr[-1] = max(0, total + final)
    if "span" in paging and paging["span"] == "auto":
        paging["span"] = 3 + next(i for i, p in enumerate(pk) if len(p) >= 256)
    return ogg(S.headers() + pk, [0, 0, 0] + gr, **paging)


SPECS = [
    # name, stream() arguments
    ("mono_64_short_150", dict(seed=1, channels=1, bs=(64, 64), rtype=0, pattern=[0] * 150)),
    ("mono_64_long_only", dict(seed=2, channels=1, bs=(64, 64), rtype=1, pattern=[1] * 6)),
    ("mono_64_mixed_r2", dict(seed=3, channels=1, bs=(64, 64), rtype=2, pattern=MIXED)),
    ("stereo_256_2048_r2", dict(seed=4, channels=2, bs=(256, 2048), rtype=2, pattern=MIXED * 2)),
    ("stereo_256_2048_r1_packets", dict(seed=5, channels=2, bs=(256, 2048), rtype=1, pattern=MIXED + [0, 1, 1, 0],
                                        specials={2: "empty", 3: "nonaudio", 5: "badmode", 6: "cutfloor", 8: "cutresidue",
                                                  9: "cutfloor", 10: "cutresidue"})),
    ("stereo_256_2048_r0_pages", dict(seed=6, channels=2, bs=(256, 2048), rtype=0, pattern=MIXED + [1, 1, 0],
                                      span="auto", bad_crc=3 + 6, second_stream=True)),
    ("stereo_2048_8192_r2", dict(seed=7, channels=2, bs=(2048, 8192), rtype=2, pattern=[1, 1, 0, 1, 0])),
    ("three_256_2048_r1", dict(seed=8, channels=3, bs=(256, 2048), rtype=1, pattern=MIXED + [1, 0, 0])),
    ("three_64_256_r0", dict(seed=9, channels=3, bs=(64, 256), rtype=0, pattern=MIXED * 3)),
    ("mono_256_2048_r1", dict(seed=10, channels=1, bs=(256, 2048), rtype=1, pattern=[0, 0, 1, 1, 0, 1, 0])),
    ("mono_64_cut_in_last_block", dict(seed=11, channels=1, bs=(64, 256), rtype=1, pattern=[0, 1, 1, 0, 1], final=-37)),
    ("stereo_64_granule_past_end", dict(seed=12, channels=2, bs=(64, 256), rtype=2, pattern=[1, 0, 0, 1], final=1000)),
    ("mono_64_single_packet", dict(seed=13, channels=1, bs=(64, 64), rtype=0, pattern=[0])),
]


@functools.lru_cache(maxsize=None)
def matrix():
    """[(name, ogg bytes)]: the undamaged streams."""
    return [(name, stream(**kw)) for name, kw in SPECS]


@functools.lru_cache(maxsize=None)
def damaged():
    """[(name, bytes)]: per stream, seeded truncations and bit flips of the file, and bit flips inside
    audio packets (valid page CRCs)."""
    out = []
    for q, (name, kw) in enumerate(SPECS):
        blob = dict(matrix())[name]
        rng = random.Random(1000 + q)
        for t in range(2):
            out.append((f"{name}/trunc{t}", blob[:rng.randrange(60, len(blob))]))
        for t in range(2):
            b = bytearray(blob)
            b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
            out.append((f"{name}/flip{t}", bytes(b)))
        for t in range(2):
            out.append((f"{name}/pkflip{t}", stream(**dict(kw, seed=kw["seed"]), packet_flips=1 + 3 * t)))
    return out


@functools.lru_cache(maxsize=None)
def encoder_streams():
    """[(name, ogg bytes)]: streams of the audio encoder tests/vorbis_enc.py (256 / 2048, one setup)."""
    import numpy as np

    import vorbis_enc as ve

    out = []
    pattern = [1, 1, 0, 0, 0, 1, 0, 1, 1]
    span = sum([256, 2048][pattern[k - 1]] // 4 + [256, 2048][pattern[k]] // 4 for k in range(1, len(pattern)))
    t = np.arange(span) / 44100
    for nch, rtype in ((1, 0), (2, 1), (2, 2)):
        x = [0.4 * np.sin(2 * np.pi * (220 + 110 * c) * t) + 0.2 * np.sin(2 * np.pi * 1375 * t) for c in range(nch)]
        pk, gr, _ = ve.encode(x, 44100, pattern, rtype=rtype, silent_blocks=(3,) if nch == 1 else ())
        out.append((f"enc_{nch}ch_r{rtype}", ve.ogg_stream(ve.headers(nch, 44100, rtype), pk, gr, final_len=gr[-1] - 100)))
    return out


def all_named():
    """Every named stream the hash file covers."""
    return matrix() + damaged() + encoder_streams()


if __name__ == "__main__":  # python tests/vorbis_streams.py DIR: the streams tools/vorbis_core_check.cpp reads
    import os
    import sys

    os.makedirs(sys.argv[1], exist_ok=True)
    for name, blob in matrix() + encoder_streams() + [(n, b) for n, b in damaged() if "/pkflip" in n]:
        with open(os.path.join(sys.argv[1], name.replace("/", "_") + ".ogg"), "wb") as f:
            f.write(blob)
