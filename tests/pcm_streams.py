"""Linear-PCM files for the planned (CPU) and device conversion tests (TEST INFRASTRUCTURE): a small
RIFF/WAVE writer (plain and WAVE_FORMAT_EXTENSIBLE headers, an optional chunk before the data) and
a small AIFF / AIFF-C writer (the SSND offset field), the sample layouts the front-end reads, the
edge shapes (data alignment, frame counts, overstated chunks, float specials) and the files that are
not linear PCM.  Every builder is cached.
"""
import functools
import struct

import numpy as np

KINDS = ("u8", "s16", "s24", "s32", "f32", "f64")
WIDTH = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8}


def samples(kind, n, seed):
    """n channel samples of `kind`: random over the whole range, the extremes first."""
    rng = np.random.default_rng(seed)
    if kind == "u8":
        v = rng.integers(0, 256, n)
        v[:3] = [0, 255, 128][:n]
        return v.astype(np.int64)
    if kind in ("s16", "s24", "s32"):
        b = 8 * WIDTH[kind]
        v = rng.integers(-(1 << (b - 1)), 1 << (b - 1), n)
        v[:4] = [-(1 << (b - 1)), (1 << (b - 1)) - 1, 0, -1][:n]
        return v.astype(np.int64)
    return (rng.standard_normal(n) * 0.4).astype(np.float32 if kind == "f32" else np.float64)


def pack(kind, v, big):
    """Interleaved samples -> bytes in the file's byte order."""
    e = ">" if big else "<"
    if kind == "u8":
        return np.asarray(v, np.uint8).tobytes()
    if kind == "s24":
        raw = (np.asarray(v, np.int64) & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3]
        return (raw[:, ::-1] if big else raw).tobytes()
    if kind in ("f32", "f64"):
        bits = np.asarray(v).view(np.uint32 if kind == "f32" else np.uint64)  # keeps NaN payloads
        return bits.astype(e + ("u4" if kind == "f32" else "u8")).tobytes()
    return np.asarray(v, np.int64).astype(e + {"s16": "i2", "s32": "i4"}[kind]).tobytes()


def wav(tag, bits, ch, payload, rate=44100, extensible=False, before=None, data_len=None, block_align=None, extra=b""):
    """RIFF/WAVE: fmt (tag, or EXTENSIBLE with the tag in the sub-format GUID), an optional chunk
    `before` = (id, body) ahead of the data, and the data chunk (data_len overrides its size field)."""
    ba = ch * ((bits + 7) // 8) if block_align is None else block_align
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, ch, rate, rate * ba, ba, bits)
    if extensible:
        fmt += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
    fmt += extra
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
    if before:
        cid, cb = before
        body += cid + struct.pack("<I", len(cb)) + cb + (b"\0" if len(cb) & 1 else b"")
    body += b"data" + struct.pack("<I", len(payload) if data_len is None else data_len) + payload
    return b"RIFF" + struct.pack("<I", len(body)) + body


def _ext80(rate):
    e = 16383 + int(rate).bit_length() - 1
    return struct.pack(">HQ", e, int(rate) << (64 - int(rate).bit_length()))


def aiff(bits, ch, frames, payload, rate=44100, comp=None, offset=0, ssnd_len=None):
    """AIFF (comp None) or AIFF-C: COMM and SSND with `offset` unused bytes before the samples."""
    comm = struct.pack(">hIh", ch, frames, bits) + _ext80(rate)
    if comp:
        comm += comp + b"\0\0"
    ssnd = struct.pack(">II", offset, 0) + bytes(range(1, offset + 1)) + payload
    body = (b"AIFC" if comp else b"AIFF") + b"COMM" + struct.pack(">I", len(comm)) + comm
    body += b"SSND" + struct.pack(">I", len(ssnd) if ssnd_len is None else ssnd_len) + ssnd
    body += b"\0" if len(ssnd) & 1 else b""
    return b"FORM" + struct.pack(">I", len(body)) + body


def wav_of(kind, ch, frames, seed, **kw):
    tag = 3 if kind in ("f32", "f64") else 1
    return wav(tag, 8 * WIDTH[kind], ch, pack(kind, samples(kind, frames * ch, seed), False), **kw)


def aiff_of(kind, ch, frames, seed, comp=None, big=True, **kw):
    return aiff(8 * WIDTH[kind], ch, frames, pack(kind, samples(kind, frames * ch, seed), big), comp=comp, **kw)


@functools.lru_cache(maxsize=None)
def matrix():
    """[(name, bytes)]: every sample layout, 1 to 3 channels, plain and EXTENSIBLE headers, AIFF and
    AIFF-C.  All linear PCM."""
    out = []
    seed = 0
    for kind in KINDS:
        for ch in (1, 2, 3):
            seed += 1
            out.append((f"wav_{kind}_{ch}ch", wav_of(kind, ch, 300 + seed, seed, rate=[44100, 48000, 22050][ch - 1])))
        seed += 1
        out.append((f"wav_ext_{kind}_2ch", wav_of(kind, 2, 290 + seed, seed, extensible=True)))
    for kind in ("s16", "s24", "s32"):
        for ch in (1, 2):
            seed += 1
            out.append((f"aiff_{kind}_{ch}ch", aiff_of(kind, ch, 310 + seed, seed, rate=48000)))
    for comp, kind, big in ((b"sowt", "s16", False), (b"fl32", "f32", True), (b"fl64", "f64", True), (b"NONE", "s24", True)):
        seed += 1
        out.append((f"aifc_{comp.decode()}_2ch", aiff_of(kind, 2, 320 + seed, seed, comp=comp, big=big)))
    return out


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def edges():
    """[(name, bytes)]: linear-PCM files at the shapes where the conversion kernel can break."""
    out = []
    for off in (0, 1, 2, 3):  # the first sample at every alignment mod 4 (the SSND offset field)
        out.append((f"aiff_s24_off{off}", aiff_of("s24", 2, 263, 40 + off, offset=off)))
        out.append((f"aiff_s16_off{off}", aiff_of("s16", 1, 261, 50 + off, offset=off)))
        out.append((f"aifc_fl64_off{off}", aiff_of("f64", 2, 259, 60 + off, comp=b"fl64", offset=off)))
        out.append((f"aifc_fl32_off{off}", aiff_of("f32", 3, 258, 70 + off, comp=b"fl32", offset=off)))
    out.append(("wav_s24_after_odd_chunk", wav_of("s24", 2, 262, 80, before=(b"LIST", b"x"))))
    out.append(("wav_s16_after_odd_chunk", wav_of("s16", 1, 262, 81, before=(b"LIST", b"abc"))))
    for frames in (1, 255, 256, 257, 4095, 4096, 4097):  # the block's lane count and its frame count
        out.append((f"wav_s24_frames{frames}", wav_of("s24", 2, frames, 90 + frames % 7)))
    out.append(("wav_s16_no_frames", wav_of("s16", 2, 0, 1)))
    pay = pack("s16", samples("s16", 2 * 200, 91), False)
    out.append(("wav_data_longer_than_file", wav(1, 16, 2, pay, data_len=len(pay) + 1000)))
    out.append(("wav_data_cut_in_a_frame", wav(1, 16, 2, pay, data_len=len(pay) + 1000)[:-3]))
    pay = pack("s24", samples("s24", 2 * 100, 92), True)
    out.append(("aiff_ssnd_longer_than_file", aiff(24, 2, 100, pay, ssnd_len=8 + len(pay) + 500)))
    # f32: NaN payloads (quiet, signalling, negative), infinities, -0.0, denormals, the largest finite
    special = _f32([0x7FC00000, 0x7FC12345, 0x7F800001, 0xFFC00001, 0xFFABCDEF, 0x7F800000, 0xFF800000, 0x80000000,
                    0x00000001, 0x807FFFFF, 0x00400000, 0x7F7FFFFF, 0x00800000, 0x3F800000])
    out.append(("wav_f32_specials_mono", wav(3, 32, 1, pack("f32", special, False))))
    out.append(("aifc_fl32_specials_mono", aiff(32, 1, special.size, pack("f32", special, True), comp=b"fl32")))
    # stereo: the mix adds and divides; infinities of one sign, -0.0 + -0.0, denormal sums
    pairs = _f32([0x7F800000, 0x3F800000, 0xFF800000, 0xFF800000, 0x80000000, 0x80000000, 0x80000000, 0x00000000,
                  0x00000001, 0x00000001, 0x807FFFFF, 0x00000003, 0x00800000, 0x80000001, 0x7F7FFFFF, 0x7F7FFFFF])
    out.append(("wav_f32_specials_stereo", wav(3, 32, 2, pack("f32", pairs, False))))
    # f64 values that round to f32 denormals, to zero, to the smallest normal and to infinity
    d = np.array([1e-40, -1e-40, 2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -40), 1e-46, 2.0 ** -126 * (1 - 2.0 ** -30),
                  3.0 * 2.0 ** -149 * 0.5, 1e39, -1e39, 3.4028235677973366e38, -0.0], np.float64)
    out.append(("wav_f64_to_denormals_mono", wav(3, 64, 1, pack("f64", d, False))))
    out.append(("wav_f64_to_denormals_stereo", wav(3, 64, 2, pack("f64", np.concatenate([d[:8], d[:8]]), False))))
    return out


@functools.lru_cache(maxsize=None)
def not_linear():
    """[(name, bytes)]: files the front-end decodes that are not linear PCM (the host decoder's)."""
    rng = np.random.default_rng(7)
    g = rng.integers(0, 256, 400).astype(np.uint8).tobytes()
    ima = rng.integers(0, 256, 2 * 64, dtype=np.uint8)
    ima[2::32] = 40  # a legal step index in every block header (2 channels x 4 bytes, then data)
    ima[6::32] = 40
    return [("wav_alaw", wav(6, 8, 2, g)), ("wav_ulaw", wav(7, 8, 1, g)),
            ("wav_ima_adpcm", wav(0x11, 4, 2, ima.tobytes(), block_align=32, extra=struct.pack("<HH", 2, 25))),
            ("aifc_alaw", aiff(8, 2, 200, g, comp=b"alaw")), ("aifc_ulaw", aiff(8, 1, 400, g, comp=b"ulaw"))]


@functools.lru_cache(maxsize=None)
def refused():
    """[(name, bytes)]: RIFF/WAVE and AIFF files the plan refuses with the host's text."""
    pay = pack("s16", samples("s16", 64, 3), False)
    return [("wav_12_bits", wav(1, 12, 1, pay, block_align=2)), ("wav_bad_block_align", wav(1, 16, 2, pay, block_align=6)),
            ("wav_no_data", wav(1, 16, 1, pay)[:36]), ("wav_zero_channels", wav(1, 16, 0, pay, block_align=2)),
            ("aiff_8_bits", aiff(8, 1, 64, pay[:64])), ("aiff_no_ssnd", aiff(16, 1, 32, pay)[:38]),
            ("aifc_unknown", aiff(16, 1, 32, pay, comp=b"ima4"))]


def passage_wav24(x, sample_rate=44100):
    """A float passage as 24-bit stereo WAV (both channels the passage)."""
    v = np.clip(np.round(np.asarray(x, np.float64) * 8388607.0), -8388608, 8388607).astype(np.int64)
    return wav(1, 24, 2, pack("s24", np.repeat(v, 2), False), rate=sample_rate)
