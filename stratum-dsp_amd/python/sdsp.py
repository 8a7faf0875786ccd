"""Python binding of libstratum_hip.so (the MI355X analyze_audio engine).

This is the ctypes stub a Python caller of the reference's API would use: `analyze_audio`
mirrors `stratum_dsp::analyze_audio(samples, sample_rate, AnalysisConfig)` (reference
src/lib.rs:86) and raises `AnalysisError` with the reference's Display text on failure.

There is no CPU fallback: if the HIP library is missing or no GPU is visible, every compute
call raises.
"""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

from sdsp_abi import (ERROR_NAMES, FLAG_NAMES, SdspAudioDecodeStats, SdspConfidence, SdspConfig, SdspDebugOverviewTimes,
                      SdspDecodeStats, SdspFlacDecodeStats, SdspOverview, SdspOverviewRequest, SdspResult,
                      SdspStageTimes, OVERVIEW_ARRAYS, result_to_dict, SdspKeyChange, SdspKeySegment, SdspKeyTimeline,
                      SdspKeyTimelineRequest, SdspDebugLevelsTimes, SdspLevels, SdspLevelsRequest, SdspLoudness,
                      SdspRequestSet, SdspSilenceRegion, LEVELS_BITS, SdspDebugTempoMapTimes, SdspTempoMap,
                      SdspTempoMapRequest, SdspTempoSegment, TEMPO_MAP_BITS, SdspDebugSectionsOut,
                      SdspDebugSectionsTimes, SdspSection, SdspSections, SdspSectionsRequest, SECTIONS_BITS, SdspRequestSetExt,
                      SdspDebugR128Times, SdspR128, SdspR128Request, SdspRequestSetExt2, R128_BITS,
                      SdspDebugFingerprintOut, SdspDebugFingerprintPair, SdspDebugFingerprintTimes, SdspFingerprint,
                      SdspFingerprintMatch, SdspFingerprintMatches, SdspFingerprintRequest, SdspRequestSetExt3, FP_BITS)

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("SDSP_LIB_PATH") or os.path.join(PKG, "lib", "libstratum_hip.so")  # override: layout/ablation builds
# the test build (-DSDSP_TEST_HOOKS): the same library with failure injection and the device
# override compiled in; only test_hooks(fail_chunk=..., devices=...) switches to it
TESTHOOKS_LIB_PATH = os.path.join(PKG, "lib", "libstratum_hip_testhooks.so")
_lib = None
_lib_th = None


class AnalysisError(Exception):
    """AnalysisError (reference src/error.rs:7-34); .kind is the variant name."""

    def __init__(self, code, message):
        super().__init__(message)
        self.code = code
        self.kind = ERROR_NAMES.get(code, "Unknown")


def build():
    subprocess.check_call(["make", "-s", "-j8", "-C", PKG])


def lib():
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH)
    return _lib


def _load(path):
    """ctypes handle of one build of the engine, with the ABI's argument types declared."""
    if True:
        if not os.path.exists(path):
            raise RuntimeError(f"{os.path.basename(path)} not built ({path}); run __graft_entry__.build()")
        L = C.CDLL(path)
        fp = C.POINTER(C.c_float)
        u64p = C.POINTER(C.c_uint64)
        L.sdsp_config_default.argtypes = [C.POINTER(SdspConfig)]
        L.sdsp_version.restype = C.c_char_p
        L.sdsp_analyze_audio.argtypes = [fp, C.c_uint64, C.c_uint32, C.POINTER(SdspConfig), C.POINTER(SdspResult),
                                         C.c_char_p, C.c_uint64]
        L.sdsp_analyze_audio.restype = C.c_int32
        L.sdsp_analyze_batch.argtypes = [C.POINTER(fp), u64p, C.c_uint64, C.c_uint32, C.POINTER(SdspConfig), C.c_uint32,
                                         C.POINTER(SdspResult)]
        L.sdsp_analyze_batch.restype = C.c_int32
        L.sdsp_analyze_batch_device.argtypes = [C.c_void_p, u64p, u64p, C.c_uint64, C.c_uint32, C.POINTER(SdspConfig),
                                                C.c_int32, C.c_void_p, C.POINTER(SdspResult)]
        L.sdsp_analyze_batch_device.restype = C.c_int32
        L.sdsp_analyze_batch_device_ex.argtypes = [C.c_void_p, u64p, u64p, C.c_uint64, C.c_uint32,
                                                   C.POINTER(SdspConfig), C.c_int32, C.c_void_p, C.c_int32,
                                                   C.POINTER(SdspResult)]
        L.sdsp_analyze_batch_device_ex.restype = C.c_int32
        L.sdsp_result_free.argtypes = [C.POINTER(SdspResult)]
        L.sdsp_analyze_batch_device_overview.argtypes = [C.c_void_p, u64p, u64p, C.c_uint64, C.c_uint32,
                                                         C.POINTER(SdspConfig), C.c_int32, C.c_void_p, C.c_int32,
                                                         C.POINTER(SdspResult), C.POINTER(SdspOverviewRequest),
                                                         C.POINTER(SdspOverview)]
        L.sdsp_analyze_batch_device_overview.restype = C.c_int32
        L.sdsp_analyze_batch_device_requests.argtypes = [C.c_void_p, u64p, u64p, C.c_uint64, C.c_uint32,
                                                         C.POINTER(SdspConfig), C.c_int32, C.c_void_p, C.c_int32,
                                                         C.POINTER(SdspResult), C.POINTER(SdspOverviewRequest),
                                                         C.POINTER(SdspOverview), C.POINTER(SdspKeyTimelineRequest),
                                                         C.POINTER(SdspKeyTimeline)]
        L.sdsp_analyze_batch_device_requests.restype = C.c_int32
        L.sdsp_analyze_batch_device_with.argtypes = [C.c_void_p, u64p, u64p, C.c_uint64, C.c_uint32,
                                                     C.POINTER(SdspConfig), C.c_int32, C.c_void_p, C.c_int32,
                                                     C.POINTER(SdspResult), C.POINTER(SdspRequestSet)]
        L.sdsp_analyze_batch_device_with.restype = C.c_int32
        L.sdsp_levels_free.argtypes = [C.POINTER(SdspLevels)]
        L.sdsp_levels_free.restype = None
        L.sdsp_sections_free.argtypes = [C.POINTER(SdspSections)]
        L.sdsp_sections_free.restype = None
        L.sdsp_debug_last_sections_times.argtypes = [C.c_int32, C.POINTER(SdspDebugSectionsTimes)]
        L.sdsp_debug_last_sections_times.restype = C.c_int32
        L.sdsp_fingerprint_free.argtypes = [C.POINTER(SdspFingerprint)]
        L.sdsp_fingerprint_free.restype = None
        L.sdsp_fingerprint_matches_free.argtypes = [C.POINTER(SdspFingerprintMatches)]
        L.sdsp_fingerprint_matches_free.restype = None
        L.sdsp_debug_last_fingerprint_times.argtypes = [C.c_int32, C.POINTER(SdspDebugFingerprintTimes)]
        L.sdsp_debug_last_fingerprint_times.restype = C.c_int32
        L.sdsp_r128_free.argtypes = [C.POINTER(SdspR128)]
        L.sdsp_r128_free.restype = None
        L.sdsp_debug_last_r128_times.argtypes = [C.c_int32, C.POINTER(SdspDebugR128Times)]
        L.sdsp_debug_last_r128_times.restype = C.c_int32
        L.sdsp_tempo_map_free.argtypes = [C.POINTER(SdspTempoMap)]
        L.sdsp_tempo_map_free.restype = None
        L.sdsp_debug_last_tempo_map_times.argtypes = [C.c_int32, C.POINTER(SdspDebugTempoMapTimes)]
        L.sdsp_debug_last_tempo_map_times.restype = C.c_int32
        L.sdsp_debug_last_levels_times.argtypes = [C.c_int32, C.POINTER(SdspDebugLevelsTimes)]
        L.sdsp_debug_last_levels_times.restype = C.c_int32
        L.sdsp_key_timeline_free.argtypes = [C.POINTER(SdspKeyTimeline)]
        L.sdsp_key_timeline_free.restype = None
        L.sdsp_debug_key_timeline.argtypes = [C.POINTER(C.c_float), u64p, C.c_uint64, C.c_uint32, C.POINTER(SdspConfig),
                                              C.POINTER(SdspKeyTimelineRequest), C.POINTER(SdspKeyTimeline), C.c_int32]
        L.sdsp_debug_key_timeline.restype = C.c_int32
        L.sdsp_overview_free.argtypes = [C.POINTER(SdspOverview)]
        L.sdsp_overview_free.restype = None
        L.sdsp_debug_last_overview_times.argtypes = [C.c_int32, C.POINTER(SdspDebugOverviewTimes)]
        L.sdsp_debug_last_overview_times.restype = C.c_int32
        L.sdsp_generate_synthetic.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int32,
                                              C.c_int32, C.c_void_p, fp, C.POINTER(C.c_int32)]
        L.sdsp_generate_synthetic.restype = C.c_int32
        L.sdsp_last_stage_times.argtypes = [C.c_int32, C.POINTER(SdspStageTimes)]
        L.sdsp_last_stage_times.restype = C.c_int32
        L.sdsp_debug_stft.argtypes = [fp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_float, fp, fp, C.c_int32]
        L.sdsp_debug_stft.restype = C.c_int32
        u64p = C.POINTER(C.c_uint64)
        L.sdsp_debug_frame_rms.argtypes = [fp, C.c_uint64, u64p, u64p, fp, C.c_uint64, C.c_uint64, C.c_uint64,
                                           C.c_int32, fp, C.c_int32]
        L.sdsp_debug_frame_rms.restype = C.c_int32
        L.sdsp_device_count.restype = C.c_int32
        L.sdsp_device_malloc.argtypes = [C.c_int32, C.c_uint64, C.POINTER(C.c_void_p)]
        L.sdsp_device_free.argtypes = [C.c_int32, C.c_void_p]
        L.sdsp_memcpy_h2d.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64]
        L.sdsp_memcpy_d2h.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64]
        L.sdsp_device_synchronize.argtypes = [C.c_int32]
        L.sdsp_compute_confidence.argtypes = [C.POINTER(SdspResult), C.POINTER(SdspConfidence)]
        L.sdsp_key_name.argtypes = [C.c_int32, C.c_uint32, C.c_char_p, C.c_uint64]
        L.sdsp_decode_audio_file.argtypes = [C.c_char_p, C.POINTER(fp), u64p, C.POINTER(C.c_uint32), C.c_char_p,
                                             C.c_uint64]
        L.sdsp_free_samples.argtypes = [fp]
        u32p = C.POINTER(C.c_uint32)
        L.sdsp_decode_flac_batch_device.argtypes = [C.POINTER(C.c_char_p), u64p, C.c_uint64, C.c_int32, C.c_void_p,
                                                    C.POINTER(C.c_void_p), u64p, u64p, u32p, C.POINTER(C.c_int32),
                                                    C.c_char_p]
        L.sdsp_decode_flac_batch_device.restype = C.c_int32
        L.sdsp_last_flac_decode_stats.argtypes = [C.c_int32, C.POINTER(SdspFlacDecodeStats)]
        L.sdsp_last_flac_decode_stats.restype = C.c_int32
        L.sdsp_debug_flac_decode_phased.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(fp), u64p, u32p, u64p, C.c_char_p,
                                                    C.c_uint64]
        L.sdsp_debug_flac_decode_phased.restype = C.c_int32
        L.sdsp_decode_batch_device.argtypes = L.sdsp_decode_flac_batch_device.argtypes
        L.sdsp_decode_batch_device.restype = C.c_int32
        L.sdsp_last_decode_stats.argtypes = [C.c_int32, C.POINTER(SdspDecodeStats)]
        L.sdsp_last_decode_stats.restype = C.c_int32
        L.sdsp_decode_audio_batch_device.argtypes = L.sdsp_decode_flac_batch_device.argtypes
        L.sdsp_decode_audio_batch_device.restype = C.c_int32
        L.sdsp_last_audio_decode_stats.argtypes = [C.c_int32, C.POINTER(SdspAudioDecodeStats)]
        L.sdsp_last_audio_decode_stats.restype = C.c_int32
        for f in ("sdsp_debug_alac_decode_phased", "sdsp_debug_pcm_decode_planned", "sdsp_debug_vorbis_decode_phased"):
            getattr(L, f).argtypes = L.sdsp_debug_flac_decode_phased.argtypes
            getattr(L, f).restype = C.c_int32
        L.sdsp_free_samples.restype = None
        for f in ("sdsp_device_malloc", "sdsp_device_free", "sdsp_memcpy_h2d", "sdsp_memcpy_d2h",
                  "sdsp_device_synchronize", "sdsp_compute_confidence", "sdsp_key_name", "sdsp_decode_audio_file"):
            getattr(L, f).restype = C.c_int32
        L.sdsp_debug_key_energy_blocked.argtypes = [C.POINTER(SdspConfig), C.c_uint32]
        L.sdsp_debug_key_energy_blocked.restype = C.c_int32
        L.sdsp_debug_set_test_hooks.argtypes = [C.c_int64, C.POINTER(C.c_int32), C.c_uint32, C.c_int32]
        L.sdsp_debug_set_test_hooks.restype = C.c_int32
        return L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def device_mem_info(device=0):
    """(free, total) bytes of HBM on `device` (sdsp_debug_mem_info)."""
    L = lib()
    f = L.sdsp_debug_mem_info
    f.argtypes = [C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    f.restype = C.c_int32
    fr, to = C.c_uint64(), C.c_uint64()
    if f(device, C.byref(fr), C.byref(to)) != 0:
        raise RuntimeError("sdsp_debug_mem_info failed")
    return fr.value, to.value


@contextlib.contextmanager
def test_hooks(fail_chunk=-1, devices=(), stft_frame_parallel=False):
    """Sets the library's test hooks (include/stratum_hip_debug.h, sdsp_debug_set_test_hooks)
    for the duration of the block, then resets them.  The library reads none of them from the
    environment.  Failure injection and the device override exist only in the test build
    (libstratum_hip_testhooks.so): with either set, every call inside the block goes to it."""
    global _lib, _lib_th, _schedule_set
    test_build = fail_chunk >= 0 or len(devices) > 0
    prev = lib()
    if test_build:
        if _lib_th is None:
            _lib_th = _load(TESTHOOKS_LIB_PATH)
        _lib, _schedule_set = _lib_th, None
    f = _lib.sdsp_debug_set_test_hooks
    dev = (C.c_int32 * max(len(devices), 1))(*devices)
    assert f(fail_chunk, dev if devices else None, len(devices), int(bool(stft_frame_parallel))) == 0
    try:
        yield
    finally:
        f(-1, None, 0, 0)
        if test_build:
            _lib, _schedule_set = prev, None


@contextlib.contextmanager
def key_cert_fixed():
    """sdsp_debug_set_key_cert(1) for the duration of the block: the key vote flags near-decision
    tracks by the fixed round-5 margins alone instead of the rigorous certificate, for
    comparing the two flagged sets."""
    f = lib().sdsp_debug_set_key_cert
    f.argtypes = [C.c_int32]
    f.restype = C.c_int32
    assert f(1) == 0
    try:
        yield
    finally:
        f(0)


def last_key_near(n, device=0):
    """sdsp_debug_last_key_near: per track of the last analysis call on `device`, whether its key
    vote was near an energy-dependent decision (and the track was analysed again exactly): 0, or
    the reason bits (1 within-mode argmax, 2 segment gate, 4 final key gap, 8 weight-sum fallback)."""
    out = np.zeros(max(int(n), 1), np.uint8)
    f = lib().sdsp_debug_last_key_near
    f.argtypes = [C.c_int32, C.c_void_p, C.c_uint64]
    f.restype = C.c_int32
    if f(device, out.ctypes.data, int(n)) != 0:
        raise RuntimeError("sdsp_debug_last_key_near failed")
    return out[: int(n)]


def key_energy_blocked(config=None, sample_rate=44100):
    """sdsp_debug_key_energy_blocked: True when `config` at `sample_rate` takes the default key
    path's block-folded HPCP frame energies (key_confidence / key_clarity re-associated, DESIGN.md
    §2); no device is touched."""
    cfg = config if config is not None else default_config()
    v = lib().sdsp_debug_key_energy_blocked(C.byref(cfg), sample_rate)
    if v < 0:
        raise ValueError("sdsp_debug_key_energy_blocked: bad arguments")
    return bool(v)


_SCHEDULE_ENV = ("SDSP_SERIAL_STREAMS", "SDSP_NO_KEY_DEFER", "SDSP_NO_ROW_REUSE", "SDSP_HOST_TRACE",
                 "SDSP_BATCH_CHUNK_TRACKS", "SDSP_HBM_BUDGET_GB")
_schedule_set = None


def _schedule_from_env():
    """The library reads no environment variable: the test and profiling schedule switches
    (SDSP_SERIAL_STREAMS, SDSP_NO_KEY_DEFER, SDSP_NO_ROW_REUSE, SDSP_HOST_TRACE,
    SDSP_BATCH_CHUNK_TRACKS, SDSP_HBM_BUDGET_GB) are read here, before each analysis call, and passed
    through sdsp_debug_set_schedule (include/stratum_hip_debug.h) when they change."""
    global _schedule_set
    e = os.environ
    knobs = (int(bool(e.get("SDSP_SERIAL_STREAMS"))), int(bool(e.get("SDSP_NO_KEY_DEFER"))),
             int(bool(e.get("SDSP_NO_ROW_REUSE"))), int(bool(e.get("SDSP_HOST_TRACE"))),
             max(int(e.get("SDSP_BATCH_CHUNK_TRACKS") or 0), 0), max(float(e.get("SDSP_HBM_BUDGET_GB") or 0.0), 0.0))
    if knobs == _schedule_set:
        return
    f = lib().sdsp_debug_set_schedule
    f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_double]
    f.restype = C.c_int32
    if f(*knobs) != 0:
        raise RuntimeError("sdsp_debug_set_schedule failed")
    _schedule_set = knobs


def default_config():
    """AnalysisConfig::default() (reference src/config.rs:594-744)."""
    c = SdspConfig()
    lib().sdsp_config_default(C.byref(c))
    return c


def version():
    return lib().sdsp_version().decode()


def analyze_audio(samples, sample_rate=44100, config=None):
    """analyze_audio(samples, sample_rate, config) -> AnalysisResult dict; raises AnalysisError."""
    x = np.ascontiguousarray(samples, dtype=np.float32)
    cfg = config if config is not None else default_config()
    r = SdspResult()
    err = C.create_string_buffer(512)
    _schedule_from_env()
    st = lib().sdsp_analyze_audio(_fp(x), x.size, sample_rate, C.byref(cfg), C.byref(r), err, 512)
    if st != 0:
        raise AnalysisError(st, err.value.decode())
    try:
        return result_to_dict(r)
    finally:
        lib().sdsp_result_free(C.byref(r))


def _batch_error(outs, n, what):
    """Whole-batch failure: the first per-track message, and free whatever was filled."""
    msg = outs[0].error_message.decode() if n > 0 and outs[0].error_message[0:1] != b"\0" else ""
    for i in range(n):
        lib().sdsp_result_free(C.byref(outs[i]))
    return f"{what}: {msg}" if msg else what


def analyze_batch(tracks, sample_rate=44100, config=None, device_mask=0, strict=True):
    """Batch form: list of per-track results; failed tracks come back as AnalysisError objects.
    strict: raise when the call as a whole reports a failure (a failed chunk); otherwise return
    the per-track results, the failed chunk's tracks as AnalysisError."""
    arrs = [np.ascontiguousarray(t, dtype=np.float32) for t in tracks]
    n = len(arrs)
    ptrs = (C.POINTER(C.c_float) * n)(*[_fp(a) for a in arrs])
    lens = np.array([a.size for a in arrs], dtype=np.uint64)
    outs = (SdspResult * n)()
    cfg = config if config is not None else default_config()
    _schedule_from_env()
    st = lib().sdsp_analyze_batch(ptrs, lens.ctypes.data_as(C.POINTER(C.c_uint64)), n, sample_rate, C.byref(cfg),
                                  device_mask, outs)
    if st != 0 and strict:
        raise AnalysisError(st, _batch_error(outs, n, "batch failed"))
    res = []
    for i in range(n):
        if outs[i].status != 0:
            res.append(AnalysisError(outs[i].status, outs[i].error_message.decode()))
        else:
            res.append(result_to_dict(outs[i]))
        lib().sdsp_result_free(C.byref(outs[i]))
    return res


def compute_confidence(result):
    """compute_confidence (src/analysis/confidence.rs:121) through the C ABI, on an
    AnalysisResult dict (as analyze_audio returns).  Returns the AnalysisConfidence fields plus
    the confidence_level() string (confidence.rs:218-228)."""
    r = SdspResult()
    r.bpm = result["bpm"]
    r.bpm_confidence = result["bpm_confidence"]
    r.key_confidence = result["key_confidence"]
    r.key_clarity = result["key_clarity"]
    r.grid_stability = result["grid_stability"]
    md = result.get("metadata", {})
    r.flags = sum(1 << FLAG_NAMES.index(f) for f in set(md.get("flags", [])))
    warns = [w.encode() for w in md.get("confidence_warnings", [])]
    arr = (C.c_char_p * max(len(warns), 1))(*warns)
    r.warnings = C.cast(arr, C.POINTER(C.c_char_p))
    r.n_warnings = len(warns)
    out = SdspConfidence()
    if lib().sdsp_compute_confidence(C.byref(r), C.byref(out)) != 0:
        raise AnalysisError(1, "Invalid input: compute_confidence")
    overall = out.overall_confidence
    level = "High" if overall >= 0.7 else "Low" if overall < 0.5 else "Medium"
    return {"bpm_confidence": out.bpm_confidence, "key_confidence": out.key_confidence,
            "grid_stability": out.grid_stability, "overall_confidence": overall,
            "flags": [FLAG_NAMES[out.flag_list[i]] for i in range(out.n_flags)], "confidence_level": level}


def decode_audio_file(path):
    """The decode front-end (sdsp_decode_audio_file): RIFF/WAVE or FLAC -> (mono float32 array, sample_rate),
    converted as examples/analyze_file.rs:25-180 does.  Raises AnalysisError(DecodingError)."""
    p = C.POINTER(C.c_float)()
    n = C.c_uint64()
    sr = C.c_uint32()
    err = C.create_string_buffer(512)
    st = lib().sdsp_decode_audio_file(os.fsencode(path), C.byref(p), C.byref(n), C.byref(sr), err, 512)
    if st != 0:
        raise AnalysisError(st, "Decoding error: " + err.value.decode(errors="replace"))
    try:
        x = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.float32)
    finally:
        lib().sdsp_free_samples(p)
    return x, sr.value


def flac_decode_stats(device=0):
    """sdsp_last_flac_decode_stats: counters and phase times of the last device FLAC decode on `device`."""
    t = SdspFlacDecodeStats()
    if lib().sdsp_last_flac_decode_stats(device, C.byref(t)) != 0:
        raise RuntimeError("sdsp_last_flac_decode_stats failed")
    return {k: getattr(t, k) for k, _ in SdspFlacDecodeStats._fields_}


def _decode_batch(entry, stats, what, blobs, device, stream):
    blobs = [bytes(b) for b in blobs]
    n = len(blobs)
    ptrs = (C.c_char_p * max(n, 1))(*blobs)
    sizes = np.array([len(b) for b in blobs], np.uint64)
    offs, lens = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
    rates, status = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.int32)
    errs = C.create_string_buffer(256 * max(n, 1))
    d = C.c_void_p()
    u64p = C.POINTER(C.c_uint64)
    st = entry(ptrs, sizes.ctypes.data_as(u64p), n, device, C.c_void_p(stream or 0),
               C.byref(d), offs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p),
               rates.ctypes.data_as(C.POINTER(C.c_uint32)),
               status.ctypes.data_as(C.POINTER(C.c_int32)), errs)
    text = [errs.raw[256 * i:256 * (i + 1)].split(b"\0", 1)[0].decode(errors="replace") for i in range(n)]
    if st != 0:
        raise AnalysisError(st, text[0] if n and text[0] else what + " failed")
    buf = DeviceBuffer.__new__(DeviceBuffer)
    buf.device, buf.ptr = device, d.value
    buf.n = int((offs[:n] + lens[:n]).max()) if n else 0
    errors = [AnalysisError(int(status[i]), "Decoding error: " + text[i]) if status[i] != 0 else None for i in range(n)]
    return buf, offs[:n].copy(), lens[:n].copy(), rates[:n].copy(), errors, stats(device)


def decode_flac_batch_device(blobs, device=0, stream=None):
    """sdsp_decode_flac_batch_device: the FLAC files in `blobs` (bytes objects) decoded on `device`.
    Returns (DeviceBuffer of the concatenated mono f32 tracks, offsets, lens, rates, errors, stats):
    track i is buffer[offsets[i] : offsets[i] + lens[i]] at rates[i]; errors[i] is None or the
    AnalysisError sdsp.decode_audio_file raises for the same bytes (then lens[i] == 0).  Raises
    AnalysisError when the call itself cannot run (no HIP device)."""
    return _decode_batch(lib().sdsp_decode_flac_batch_device, flac_decode_stats, "device FLAC decode", blobs, device, stream)


def decode_stats(device=0):
    """sdsp_last_decode_stats: counters and phase times of the last sdsp_decode_batch_device call on `device`."""
    t = SdspDecodeStats()
    if lib().sdsp_last_decode_stats(device, C.byref(t)) != 0:
        raise RuntimeError("sdsp_last_decode_stats failed")
    return {k: getattr(t, k) for k, _ in SdspDecodeStats._fields_}


def decode_batch_device(blobs, device=0, stream=None):
    """sdsp_decode_batch_device: the files in `blobs` (bytes objects: FLAC, ALAC in M4A / CAF, WAV, AIFF
    on the device; anything else the front-end reads through the host decoder) decoded into one
    device buffer.  Returns the same tuple as decode_flac_batch_device, with the decode_stats dict."""
    return _decode_batch(lib().sdsp_decode_batch_device, decode_stats, "device decode", blobs, device, stream)


def audio_decode_stats(device=0):
    """sdsp_last_audio_decode_stats: counters and phase times of the last sdsp_decode_audio_batch_device call on `device`."""
    t = SdspAudioDecodeStats()
    if lib().sdsp_last_audio_decode_stats(device, C.byref(t)) != 0:
        raise RuntimeError("sdsp_last_audio_decode_stats failed")
    return {k: getattr(t, k) for k, _ in SdspAudioDecodeStats._fields_}


def decode_audio_batch_device(blobs, device=0, stream=None):
    """sdsp_decode_audio_batch_device: decode_batch_device with Ogg Vorbis decoded on the device too.
    Returns the same tuple, with the audio_decode_stats dict."""
    return _decode_batch(lib().sdsp_decode_audio_batch_device, audio_decode_stats, "device decode", blobs, device, stream)


def debug_flac_decode_phased(data):
    """sdsp_debug_flac_decode_phased: the device decoder's four phases on the CPU.  Returns (mono
    float32 array, sample_rate, (candidates, accepted, rejected)); raises AnalysisError as
    decode_audio_file does."""
    data = bytes(data)
    p = C.POINTER(C.c_float)()
    n = C.c_uint64()
    sr = C.c_uint32()
    counts = (C.c_uint64 * 3)()
    err = C.create_string_buffer(512)
    st = lib().sdsp_debug_flac_decode_phased(data, len(data), C.byref(p), C.byref(n), C.byref(sr), counts, err, 512)
    if st != 0:
        raise AnalysisError(st, "Decoding error: " + err.value.decode(errors="replace"))
    try:
        x = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.float32)
    finally:
        lib().sdsp_free_samples(p)
    return x, sr.value, tuple(int(v) for v in counts)


def _debug_decode(entry, data, n_info):
    data = bytes(data)
    p = C.POINTER(C.c_float)()
    n = C.c_uint64()
    sr = C.c_uint32()
    info = (C.c_uint64 * n_info)()
    err = C.create_string_buffer(512)
    st = entry(data, len(data), C.byref(p), C.byref(n), C.byref(sr), info, err, 512)
    if st != 0:
        text = err.value.decode(errors="replace")
        raise AnalysisError(st, ("Decoding error: " if st == 2 else "Not implemented: ") + text)
    try:
        x = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.float32)
    finally:
        lib().sdsp_free_samples(p)
    return x, sr.value, tuple(int(v) for v in info)


def debug_alac_decode_phased(data):
    """sdsp_debug_alac_decode_phased: the device ALAC decoder's phases on the CPU.  Returns (mono
    float32 array, sample_rate, (packets, decoded, skipped)); raises AnalysisError as decode_audio_file
    does, or AnalysisError(NotImplemented, "... not planned ...") for bytes that are no ALAC container."""
    return _debug_decode(lib().sdsp_debug_alac_decode_phased, data, 3)


def debug_vorbis_decode_phased(data):
    """sdsp_debug_vorbis_decode_phased: the device Vorbis decoder's phases on the CPU.  Returns (mono
    float32 array, sample_rate, (packets, zeroed)); raises AnalysisError as decode_audio_file does, or
    AnalysisError(NotImplemented, "... not planned ...") for bytes that are no Ogg Vorbis stream."""
    return _debug_decode(lib().sdsp_debug_vorbis_decode_phased, data, 2)


def debug_pcm_decode_planned(data):
    """sdsp_debug_pcm_decode_planned: the host plan, then pcm_core over the planned frames.  Returns
    (mono float32 array, sample_rate, (kind | big << 8, channels, data offset, frames)); raises
    AnalysisError as decode_audio_file does, or AnalysisError(NotImplemented, "... not planned ...")
    for a file that is not linear PCM in RIFF/WAVE or AIFF."""
    return _debug_decode(lib().sdsp_debug_pcm_decode_planned, data, 4)


class ResultBatch:
    """The C-ABI result array of one batch call, kept as native structs (no per-track Python
    objects are built until asked for).  Index it for AnalysisResult dicts / AnalysisError."""

    def __init__(self, outs, n):
        self._outs = outs
        self.n = n
        self.status = [outs[i].status for i in range(n)]

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        o = self._outs[i]
        if o.status != 0:
            return AnalysisError(o.status, o.error_message.decode())
        return result_to_dict(o)

    def count(self, field, value=1):
        """How many successful tracks have the native result field == value (e.g.
        tempogram_multi_res_triggered), without building result dicts."""
        return sum(1 for i in range(self.n) if self.status[i] == 0 and getattr(self._outs[i], field) == value)

    def field(self, name, failed=0):
        """The native scalar result field `name` of every track (`failed` for a failed track),
        without building result dicts."""
        return [getattr(self._outs[i], name) if self.status[i] == 0 else failed for i in range(self.n)]

    def values(self, name, count):
        """The native float list `name` of every track, `count` naming its length field (beats /
        n_beats, downbeats / n_downbeats, bars / n_bars), as float32 arrays (copies; empty for a
        failed track)."""
        out = []
        for i in range(self.n):
            k = int(getattr(self._outs[i], count)) if self.status[i] == 0 else 0
            out.append(np.ctypeslib.as_array(getattr(self._outs[i], name), shape=(k,)).copy() if k
                       else np.zeros(0, np.float32))
        return out

    def free(self):
        if self._outs is not None:
            for i in range(self.n):
                lib().sdsp_result_free(C.byref(self._outs[i]))
            self._outs = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


STAGES_FULL = 0
STAGES_BPM_ONLY = 1  # stages a1-a19 (src/lib.rs:86-910): no key path, no beat grid


def analyze_batch_device(d_ptr, offsets, lens, sample_rate=44100, config=None, device=0, stream=None, raw=False,
                         stages=STAGES_FULL):
    """Tracks already resident in HBM (d_ptr: device address).  Returns a list of results
    (dicts / AnalysisError), or with raw=True the native ResultBatch.  stages=STAGES_BPM_ONLY runs
    the tempo path alone (sdsp_analyze_batch_device_ex)."""
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    n = ln.size
    outs = (SdspResult * n)()
    cfg = config if config is not None else default_config()
    _schedule_from_env()
    st = lib().sdsp_analyze_batch_device_ex(C.c_void_p(d_ptr), offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            ln.ctypes.data_as(C.POINTER(C.c_uint64)), n, sample_rate, C.byref(cfg),
                                            device, C.c_void_p(stream or 0), stages, outs)
    if st != 0:
        raise AnalysisError(st, _batch_error(outs, n, "device batch failed"))
    batch = ResultBatch(outs, n)
    if raw:
        return batch
    res = [batch[i] for i in range(n)]
    batch.free()
    return res


def overview_to_dict(o):
    """The scalar fields and the five arrays (float32 copies) of one sdsp_overview."""
    n = int(o.n_columns)
    d = {"n_columns": n, "n_frames": int(o.n_frames), "first_sample": int(o.first_sample),
         "n_samples": int(o.n_samples), "frame_size": int(o.frame_size), "hop_size": int(o.hop_size),
         "band_bins": [int(o.band_bins[0]), int(o.band_bins[1])], "status": int(o.status)}
    for k in OVERVIEW_ARRAYS:
        p = getattr(o, k)
        d[k] = np.ctypeslib.as_array(p, shape=(n,)).copy() if n and p else np.zeros(0, np.float32)
    return d


def overview_request(columns=0, frames_per_column=0, low_max_hz=250.0, mid_max_hz=4000.0):
    """An sdsp_overview_request: `columns` columns per track, or one column per `frames_per_column`
    frames (exactly one of the two), and the upper edges of the low and the mid band in Hz."""
    return SdspOverviewRequest(columns, frames_per_column, low_max_hz, mid_max_hz)


def analyze_batch_device_overview(d_ptr, offsets, lens, sample_rate=44100, config=None, device=0, stream=None,
                                  stages=STAGES_FULL, request=None):
    """sdsp_analyze_batch_device_overview: analyze_batch_device(raw=True) that also returns every
    track's overview envelope.  `request` is an SdspOverviewRequest (overview_request()); None
    passes NULL, which is sdsp_analyze_batch_device_ex itself.  Returns (ResultBatch, overviews):
    overviews[i] is a dict of track i's scalar fields (n_columns, n_frames, first_sample, n_samples,
    frame_size, hop_size, band_bins, status) and its five float32 arrays smin, smax, low, mid, high
    (include/stratum_hip.h has the definition); [] without a request.  Raises AnalysisError when the
    call as a whole fails (a bad request: InvalidInput, before any device is touched)."""
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    n = ln.size
    outs = (SdspResult * n)()
    ovs = (SdspOverview * max(n, 1))() if request is not None else None
    cfg = config if config is not None else default_config()
    _schedule_from_env()
    u64p = C.POINTER(C.c_uint64)
    st = lib().sdsp_analyze_batch_device_overview(C.c_void_p(d_ptr), offs.ctypes.data_as(u64p), ln.ctypes.data_as(u64p),
                                                  n, sample_rate, C.byref(cfg), device, C.c_void_p(stream or 0), stages,
                                                  outs, C.byref(request) if request is not None else None, ovs)
    if st != 0:
        raise AnalysisError(st, _batch_error(outs, n, "device batch failed"))
    overviews = []
    if ovs is not None:
        for i in range(n):
            overviews.append(overview_to_dict(ovs[i]))
            lib().sdsp_overview_free(C.byref(ovs[i]))
    return ResultBatch(outs, n), overviews


KEY_SEGMENT_FIELDS = ("start_frame", "timestamp", "key", "confidence", "clarity", "top_keys", "top_scores")
KEY_CHANGE_FIELDS = ("segment", "timestamp", "from_key", "to_key", "confidence")


def _records(ptr, n, ctype):
    """n library-owned structs as a numpy record array (a copy)."""
    dt = np.dtype(ctype)
    if not n or not ptr:
        return np.zeros(0, dt)
    return np.frombuffer(C.string_at(ptr, n * C.sizeof(ctype)), dtype=dt).copy()


def key_timeline_to_dict(t):
    """One sdsp_key_timeline: its scalar fields, and `segments` / `changes` as dicts of numpy
    arrays, one per field (KEY_SEGMENT_FIELDS, KEY_CHANGE_FIELDS; top_keys / top_scores (S, 3))."""
    d = {k: int(getattr(t, k)) for k in ("n_segments", "n_changes", "n_frames", "first_sample", "segment_frames",
                                         "hop_frames", "frame_size", "hop_size", "primary_key", "primary_count", "status")}
    d["primary_confidence"] = np.float32(t.primary_confidence)
    seg = _records(t.segments, d["n_segments"], SdspKeySegment)
    chg = _records(t.changes, d["n_changes"], SdspKeyChange)
    d["segments"] = {k: seg[k].copy() for k in KEY_SEGMENT_FIELDS}
    d["changes"] = {k: chg[k].copy() for k in KEY_CHANGE_FIELDS}
    return d


def key_timeline_request(segment_seconds=0.0, overlap_seconds=0.0, segment_frames=0, hop_frames=0,
                         min_change_confidence=-1.0):
    """An sdsp_key_timeline_request: segments of segment_seconds overlapping by overlap_seconds, or
    of segment_frames key frames every hop_frames (exactly one form).  min_change_confidence: the
    reference's fixed value is 0.2; a negative one (the default here) reports every change."""
    return SdspKeyTimelineRequest(segment_seconds, overlap_seconds, segment_frames, hop_frames, min_change_confidence)


def analyze_batch_device_requests(d_ptr, offsets, lens, sample_rate=44100, config=None, device=0, stream=None,
                                  stages=STAGES_FULL, overview=None, key_timeline=None):
    """sdsp_analyze_batch_device_requests: analyze_batch_device(raw=True) with both optional
    requests, an SdspOverviewRequest and an SdspKeyTimelineRequest (key_timeline_request()); None
    passes NULL.  Returns (ResultBatch, overviews, timelines): overviews as
    analyze_batch_device_overview returns them, timelines[i] a key_timeline_to_dict(); each [] without
    its request.  Raises AnalysisError when the call as a whole fails (a refused request)."""
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    n = ln.size
    outs = (SdspResult * n)()
    ovs = (SdspOverview * max(n, 1))() if overview is not None else None
    kts = (SdspKeyTimeline * max(n, 1))() if key_timeline is not None else None
    cfg = config if config is not None else default_config()
    _schedule_from_env()
    u64p = C.POINTER(C.c_uint64)
    st = lib().sdsp_analyze_batch_device_requests(C.c_void_p(d_ptr), offs.ctypes.data_as(u64p), ln.ctypes.data_as(u64p),
                                                  n, sample_rate, C.byref(cfg), device, C.c_void_p(stream or 0), stages,
                                                  outs, C.byref(overview) if overview is not None else None, ovs,
                                                  C.byref(key_timeline) if key_timeline is not None else None, kts)
    if st != 0:
        raise AnalysisError(st, _batch_error(outs, n, "device batch failed"))
    overviews, timelines = [], []
    for i in range(n):
        if ovs is not None:
            overviews.append(overview_to_dict(ovs[i]))
            lib().sdsp_overview_free(C.byref(ovs[i]))
        if kts is not None:
            timelines.append(key_timeline_to_dict(kts[i]))
            lib().sdsp_key_timeline_free(C.byref(kts[i]))
    return ResultBatch(outs, n), overviews, timelines


LOUDNESS_FIELDS = ("measured_lufs", "peak_db", "rms_db", "gain_db", "gain")
LEVELS_METHODS = ("peak", "rms", "loudness")  # index = enum sdsp_normalization


def levels_request(what=("peak", "rms", "loudness", "silence")):
    """An sdsp_levels_request: `what` is a mask of sdsp_levels_what bits, or names out of peak, rms,
    loudness, silence (the default asks for all four)."""
    if not isinstance(what, int):
        mask = 0
        for name in what:
            mask |= LEVELS_BITS[name]
        what = mask
    return SdspLevelsRequest(what)


def levels_to_dict(l):
    """One sdsp_levels: its scalar fields, `methods` (peak / rms / loudness -> dict of status,
    measured, has_lufs and the np.float32 fields of LOUDNESS_FIELDS) and `regions`, a list of
    (start_sample, end_sample, np.float32 duration_seconds)."""
    d = {k: int(getattr(l, k)) for k in ("n_samples", "trim_start", "trim_end", "frame_size", "n_regions", "status")}
    d["applied_gain"] = np.float32(l.applied_gain)
    d["threshold_db"] = np.float32(l.threshold_db)
    d["methods"] = {}
    for m, name in enumerate(LEVELS_METHODS):
        e = l.method[m]
        md = {"status": int(e.status), "measured": int(e.measured), "has_lufs": int(e.has_lufs)}
        for k in LOUDNESS_FIELDS:
            md[k] = np.float32(getattr(e, k))
        d["methods"][name] = md
    reg = _records(l.regions, d["n_regions"], SdspSilenceRegion)
    d["regions"] = [(int(r["start_sample"]), int(r["end_sample"]), np.float32(r["duration_seconds"])) for r in reg]
    return d


TEMPO_SEGMENT_FIELDS = tuple(k for k, _ in SdspTempoSegment._fields_)


def tempo_map_request(what=("segments", "onsets")):
    """An sdsp_tempo_map_request: `what` is a mask of sdsp_tempo_map_what bits, or names out of
    segments, onsets (the default asks for both)."""
    if not isinstance(what, int):
        mask = 0
        for name in what:
            mask |= TEMPO_MAP_BITS[name]
        what = mask
    return SdspTempoMapRequest(what)


def tempo_map_to_dict(m):
    """One sdsp_tempo_map: its integer fields as int, its float fields as np.float32,
    time_signature_scores a float32 array of 3, `segments` a dict of numpy arrays, one per field of
    TEMPO_SEGMENT_FIELDS, and `onsets` a uint32 array."""
    d = {k: int(getattr(m, k)) for k in ("status", "has_grid", "has_variation", "refined", "time_signature_scored",
                                         "hmm_beats", "beats_per_bar", "first_sample", "n_segments", "n_onsets")}
    for k in ("nominal_bpm", "nominal_confidence", "time_signature_confidence"):
        d[k] = np.float32(getattr(m, k))
    d["time_signature_scores"] = np.array(list(m.time_signature_scores), np.float32)
    seg = _records(m.segments, d["n_segments"], SdspTempoSegment)
    d["segments"] = {k: seg[k].copy() for k in TEMPO_SEGMENT_FIELDS}
    d["onsets"] = _records(m.onsets, d["n_onsets"], C.c_uint32).astype(np.uint32)
    return d


def tempo_map_times(device=0):
    """sdsp_debug_last_tempo_map_times: k_tempo_map's and k_beat's event times of the last call with
    a tempo map request on `device`."""
    t = SdspDebugTempoMapTimes()
    if lib().sdsp_debug_last_tempo_map_times(device, C.byref(t)) != 0:
        raise RuntimeError("sdsp_debug_last_tempo_map_times failed")
    return {k: getattr(t, k) for k, _ in SdspDebugTempoMapTimes._fields_}


SECTION_FIELDS = tuple(k for k, _ in SdspSection._fields_)


def sections_request(cell_seconds=0.0, cell_samples=0, kernel_cells=16, min_gap_cells=8, energy_weight=1.0,
                     min_strength=0.5, snap_seconds=0.0, what=("list", "curve")):
    """An sdsp_sections_request: the cell as cell_seconds or cell_samples (exactly one), K, G, the
    energy weight, the strength floor and the snap distance; `what` is a mask of sdsp_sections_what
    bits, or names out of list, curve (the default asks for both)."""
    if not isinstance(what, int):
        mask = 0
        for name in what:
            mask |= SECTIONS_BITS[name]
        what = mask
    return SdspSectionsRequest(what, cell_seconds, cell_samples, kernel_cells, min_gap_cells, energy_weight, min_strength,
                               snap_seconds)


def sections_to_dict(s):
    """One sdsp_sections: its integer fields as int, gmax and nmax as np.float32, `sections` a dict
    of numpy arrays, one per field of SECTION_FIELDS, `novelty` and `energy` float32 arrays."""
    d = {k: int(getattr(s, k)) for k in ("status", "n_cells", "cell_samples", "first_sample", "n_sections", "n_curve")}
    d["gmax"], d["nmax"] = np.float32(s.gmax), np.float32(s.nmax)
    sec = _records(s.sections, d["n_sections"], SdspSection)
    d["sections"] = {k: sec[k].copy() for k in SECTION_FIELDS}
    d["novelty"] = _records(s.novelty, d["n_curve"], C.c_float).astype(np.float32)
    d["energy"] = _records(s.energy, d["n_curve"], C.c_float).astype(np.float32)
    return d


def sections_times(device=0):
    """sdsp_debug_last_sections_times: the event times of the three section steps of the last call
    with a sections request on `device`."""
    t = SdspDebugSectionsTimes()
    if lib().sdsp_debug_last_sections_times(device, C.byref(t)) != 0:
        raise RuntimeError("sdsp_debug_last_sections_times failed")
    return {k: getattr(t, k) for k, _ in SdspDebugSectionsTimes._fields_}


R128_FLOATS = ("integrated_lufs", "range_lu", "range_low_lufs", "range_high_lufs", "max_momentary_lufs",
               "max_short_term_lufs", "sample_peak", "true_peak", "sample_peak_db", "true_peak_dbtp")
R128_INTS = ("status", "has_integrated", "has_range", "n_samples", "step_samples", "n_steps", "n_momentary", "n_short_term",
             "n_gated_momentary", "n_gated_short_term")


def loudness_request(what=("loudness", "true-peak")):
    """An sdsp_r128_request: `what` is a mask of sdsp_r128_what bits, or names out of loudness,
    true-peak, curves."""
    if not isinstance(what, int):
        mask = 0
        for name in what:
            mask |= R128_BITS[name]
        what = mask
    return SdspR128Request(what)


def r128_to_dict(r):
    """One sdsp_r128: its integer fields as int, its floats as np.float32, `shelf` and `highpass`
    float32 arrays of b0 b1 b2 a1 a2, `momentary` and `short_term` float32 arrays (empty without the
    curves)."""
    d = {k: int(getattr(r, k)) for k in R128_INTS}
    for k in R128_FLOATS:
        d[k] = np.float32(getattr(r, k))
    d["shelf"] = np.array(list(r.shelf), np.float32)
    d["highpass"] = np.array(list(r.highpass), np.float32)
    d["momentary"] = _records(r.momentary, d["n_momentary"] if r.momentary else 0, C.c_float).astype(np.float32)
    d["short_term"] = _records(r.short_term, d["n_short_term"] if r.momentary else 0, C.c_float).astype(np.float32)
    return d


def r128_times(device=0):
    """sdsp_debug_last_r128_times: the event times of the three programme loudness kernels of the
    last call with a loudness request on `device`."""
    t = SdspDebugR128Times()
    if lib().sdsp_debug_last_r128_times(device, C.byref(t)) != 0:
        raise RuntimeError("sdsp_debug_last_r128_times failed")
    return {k: getattr(t, k) for k, _ in SdspDebugR128Times._fields_}


FP_MATCH_FIELDS = ("a", "b", "offset_words", "offset_samples", "bit_errors", "bits_compared", "ber")


def fingerprint_request(cell_seconds=0.0, cell_samples=0, max_offset_words=16, min_overlap_words=32, max_ber=0.30,
                        what=("words", "match")):
    """An sdsp_fingerprint_request: cells of cell_seconds, or of cell_samples samples (exactly one
    of the two); `what` a mask of sdsp_fingerprint_what bits, or names out of words, match."""
    if not isinstance(what, int):
        mask = 0
        for name in what:
            mask |= FP_BITS[name]
        what = mask
    return SdspFingerprintRequest(what, cell_seconds, cell_samples, max_offset_words, min_overlap_words, max_ber)


def fingerprint_to_dict(f):
    """One sdsp_fingerprint: its integer fields as int and `words` a uint32 array (empty without
    the words)."""
    d = {k: int(getattr(f, k)) for k in ("status", "n_cells", "n_words", "cell_samples", "first_sample", "n_matches")}
    d["words"] = _records(f.words, d["n_words"] if f.words else 0, C.c_uint32).astype(np.uint32)
    return d


def fingerprint_matches_to_dict(m):
    """One sdsp_fingerprint_matches: n_compared, n_pairs, n_matches and `matches`, a dict of numpy
    arrays, one per field (FP_MATCH_FIELDS; ber float32)."""
    d = {k: int(getattr(m, k)) for k in ("n_compared", "n_pairs", "n_matches")}
    rec = _records(m.matches, d["n_matches"], SdspFingerprintMatch)
    d["matches"] = {k: rec[k].copy() for k in FP_MATCH_FIELDS}
    return d


def fingerprint_times(device=0):
    """sdsp_debug_last_fingerprint_times: the event times of the three fingerprint kernels of the
    last call with a fingerprint request on `device`."""
    t = SdspDebugFingerprintTimes()
    if lib().sdsp_debug_last_fingerprint_times(device, C.byref(t)) != 0:
        raise RuntimeError("sdsp_debug_last_fingerprint_times failed")
    return {k: getattr(t, k) for k, _ in SdspDebugFingerprintTimes._fields_}


def analyze_batch_device_with(d_ptr, offsets, lens, sample_rate=44100, config=None, device=0, stream=None,
                              stages=STAGES_FULL, overview=None, key_timeline=None, levels=None, request_set=True,
                              tempo_map=None, sections=None, loudness=None, fingerprint=None):
    """sdsp_analyze_batch_device_with: analyze_batch_device(raw=True) with any of the optional
    requests: an SdspOverviewRequest, an SdspKeyTimelineRequest, an SdspLevelsRequest
    (levels_request()), an SdspTempoMapRequest (tempo_map_request()); None leaves a request out.
    request_set=False passes set == NULL.  Returns (ResultBatch, overviews, timelines, levels), and
    with a tempo map request a fifth element, the tempo maps: levels[i] a levels_to_dict(), maps[i]
    a tempo_map_to_dict(); each list [] without its request.  Raises AnalysisError when the call as
    a whole fails (a refused request).  With a sections request (sections_request()) the sections,
    each a sections_to_dict(), are one more element at the end of the tuple, and with a loudness
    request (loudness_request()) the programme loudness, each an r128_to_dict(), one more after that.
    With a fingerprint request (fingerprint_request()) one more element at the very end: a dict with
    `fingerprints`, a fingerprint_to_dict() per track, and `matches`, the call's
    fingerprint_matches_to_dict()."""
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    n = ln.size
    outs = (SdspResult * n)()
    ovs = (SdspOverview * max(n, 1))() if overview is not None else None
    kts = (SdspKeyTimeline * max(n, 1))() if key_timeline is not None else None
    lvs = (SdspLevels * max(n, 1))() if levels is not None else None
    tms = (SdspTempoMap * max(n, 1))() if tempo_map is not None else None
    scs = (SdspSections * max(n, 1))() if sections is not None else None
    cfg = config if config is not None else default_config()
    _schedule_from_env()
    r128s = (SdspR128 * max(n, 1))() if loudness is not None else None
    fps = (SdspFingerprint * max(n, 1))() if fingerprint is not None else None
    fpm = SdspFingerprintMatches() if fingerprint is not None else None
    ext3 = SdspRequestSetExt3()  # (a call without the later requests passes the older structs' sizes)
    ext2 = ext3.base
    ext = ext2.base
    rs = ext.base
    rs.struct_size = C.sizeof(SdspRequestSetExt3 if fingerprint is not None else
                              SdspRequestSetExt2 if loudness is not None else
                              SdspRequestSetExt if sections is not None else SdspRequestSet)
    if overview is not None:
        rs.ov_req = C.pointer(overview)
        rs.overviews = ovs
    if key_timeline is not None:
        rs.kt_req = C.pointer(key_timeline)
        rs.timelines = kts
    if levels is not None:
        rs.lv_req = C.pointer(levels)
        rs.levels = lvs
    if tempo_map is not None:
        rs.tm_req = C.pointer(tempo_map)
        rs.tempo_maps = tms
    if sections is not None:
        ext.sc_req = C.pointer(sections)
        ext.sections = scs
    if loudness is not None:
        ext2.r128_req = C.pointer(loudness)
        ext2.r128 = r128s
    if fingerprint is not None:
        ext3.fp_req = C.pointer(fingerprint)
        ext3.fingerprints = fps
        ext3.fp_matches = C.pointer(fpm)
    u64p = C.POINTER(C.c_uint64)
    st = lib().sdsp_analyze_batch_device_with(C.c_void_p(d_ptr), offs.ctypes.data_as(u64p), ln.ctypes.data_as(u64p), n,
                                              sample_rate, C.byref(cfg), device, C.c_void_p(stream or 0), stages, outs,
                                              C.byref(rs) if request_set else None)
    if st != 0:
        raise AnalysisError(st, _batch_error(outs, n, "device batch failed"))
    overviews, timelines, lv, maps, secs, louds = [], [], [], [], [], []
    for i in range(n if request_set else 0):
        if ovs is not None:
            overviews.append(overview_to_dict(ovs[i]))
            lib().sdsp_overview_free(C.byref(ovs[i]))
        if kts is not None:
            timelines.append(key_timeline_to_dict(kts[i]))
            lib().sdsp_key_timeline_free(C.byref(kts[i]))
        if lvs is not None:
            lv.append(levels_to_dict(lvs[i]))
            lib().sdsp_levels_free(C.byref(lvs[i]))
        if tms is not None:
            maps.append(tempo_map_to_dict(tms[i]))
            lib().sdsp_tempo_map_free(C.byref(tms[i]))
        if scs is not None:
            secs.append(sections_to_dict(scs[i]))
            lib().sdsp_sections_free(C.byref(scs[i]))
        if r128s is not None:
            louds.append(r128_to_dict(r128s[i]))
            lib().sdsp_r128_free(C.byref(r128s[i]))
    ret = (ResultBatch(outs, n), overviews, timelines, lv)
    if tempo_map is not None:
        ret += (maps,)
    if sections is not None:
        ret += (secs,)
    if loudness is not None:
        ret += (louds,)
    if fingerprint is not None:
        prints = []
        for i in range(n if request_set else 0):
            prints.append(fingerprint_to_dict(fps[i]))
            lib().sdsp_fingerprint_free(C.byref(fps[i]))
        matches = fingerprint_matches_to_dict(fpm) if request_set else None
        if request_set:
            lib().sdsp_fingerprint_matches_free(C.byref(fpm))
        ret += (dict(fingerprints=prints, matches=matches),)
    return ret


def levels_times(device=0):
    """sdsp_debug_last_levels_times: the levels folds' event times of the last call with a levels
    request on `device`."""
    t = SdspDebugLevelsTimes()
    if lib().sdsp_debug_last_levels_times(device, C.byref(t)) != 0:
        raise RuntimeError("sdsp_debug_last_levels_times failed")
    return {k: getattr(t, k) for k, _ in SdspDebugLevelsTimes._fields_}


def debug_key_timeline(chroma_list, request, sample_rate=44100, config=None, device=0):
    """sdsp_debug_key_timeline: the timeline kernel and host logic over host chroma rows, one (F, 12)
    array per track (F = 0 allowed), taken as the smoothed rows of the definition.  Returns one
    key_timeline_to_dict() per track."""
    cfg = config if config is not None else default_config()
    rows = [np.ascontiguousarray(c, np.float32).reshape(-1, 12) for c in chroma_list]
    frames = np.array([r.shape[0] for r in rows], np.uint64)
    flat = np.ascontiguousarray(np.concatenate(rows, axis=0) if rows else np.zeros((0, 12), np.float32))
    out = (SdspKeyTimeline * max(len(rows), 1))()
    st = lib().sdsp_debug_key_timeline(_fp(flat), frames.ctypes.data_as(C.POINTER(C.c_uint64)), len(rows), sample_rate,
                                       C.byref(cfg), C.byref(request), out, device)
    if st != 0:
        raise AnalysisError(st, "debug_key_timeline failed")
    res = []
    for i in range(len(rows)):
        res.append(key_timeline_to_dict(out[i]))
        lib().sdsp_key_timeline_free(C.byref(out[i]))
    return res


def overview_times(device=0):
    """sdsp_debug_last_overview_times: the overview kernels' event times and bytes of the last call
    with a request on `device`."""
    t = SdspDebugOverviewTimes()
    if lib().sdsp_debug_last_overview_times(device, C.byref(t)) != 0:
        raise RuntimeError("sdsp_debug_last_overview_times failed")
    return {k: getattr(t, k) for k, _ in SdspDebugOverviewTimes._fields_}


def generate_synthetic(d_ptr, n_tracks, length, sample_rate=44100, seed0=0, bpm_mode=0, device=0, stream=None):
    bpm = np.zeros(n_tracks, np.float32)
    key = np.zeros(n_tracks, np.int32)
    st = lib().sdsp_generate_synthetic(C.c_void_p(d_ptr), n_tracks, length, sample_rate, seed0, bpm_mode, device,
                                       C.c_void_p(stream or 0), _fp(bpm), key.ctypes.data_as(C.POINTER(C.c_int32)))
    if st != 0:
        raise AnalysisError(st, "synthetic generation failed")
    return bpm, key


def stage_times(device=0):
    t = SdspStageTimes()
    lib().sdsp_last_stage_times(device, C.byref(t))
    return {k: getattr(t, k) for k, _ in SdspStageTimes._fields_}


class DeviceBuffer:
    """A float32 buffer in HBM owned through the engine's own HIP runtime."""

    def __init__(self, n_floats, device=0):
        self.device = device
        self.n = int(n_floats)
        p = C.c_void_p()
        if lib().sdsp_device_malloc(device, self.n * 4, C.byref(p)) != 0:
            raise MemoryError(f"sdsp_device_malloc({self.n * 4} bytes) failed")
        self.ptr = p.value

    def to_host(self, start=0, count=None):
        count = self.n - start if count is None else count
        out = np.empty(count, np.float32)
        if lib().sdsp_memcpy_d2h(self.device, out.ctypes.data, self.ptr + 4 * start, 4 * count) != 0:
            raise RuntimeError("sdsp_memcpy_d2h failed")
        return out

    def from_host(self, arr, start=0):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        if lib().sdsp_memcpy_h2d(self.device, self.ptr + 4 * start, a.ctypes.data, 4 * a.size) != 0:
            raise RuntimeError("sdsp_memcpy_h2d failed")

    def free(self):
        if self.ptr:
            lib().sdsp_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_count():
    return int(lib().sdsp_device_count())


def synchronize(device=0):
    if lib().sdsp_device_synchronize(device) != 0:
        raise RuntimeError("sdsp_device_synchronize failed")


def debug_frame_rms(tracks, gains, fs, hop, per_frame=False, device=0):
    """Frame RMS of each track (silence-trimming framing), concatenated over tracks."""
    arrs = [np.ascontiguousarray(t, dtype=np.float32) for t in tracks]
    lens = np.array([a.size for a in arrs], np.uint64)
    offs = np.zeros(len(arrs), np.uint64)
    if len(arrs) > 1:
        offs[1:] = np.cumsum(lens)[:-1]
    x = np.concatenate(arrs) if arrs else np.zeros(0, np.float32)
    frames = sum(((int(n) - fs) // hop + 1) if n >= fs else (1 if n > 0 else 0) for n in lens)
    out = np.empty(max(frames, 1), np.float32)
    g = np.ascontiguousarray(gains, dtype=np.float32)
    u64p = C.POINTER(C.c_uint64)
    st = lib().sdsp_debug_frame_rms(_fp(x), x.size, offs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), _fp(g),
                                    len(arrs), fs, hop, 1 if per_frame else 0, _fp(out), device)
    if st != 0:
        raise AnalysisError(st, "debug_frame_rms failed")
    return out[:frames]


def debug_stft(x, nfft, hop, gain=1.0, device=0):
    x = np.ascontiguousarray(x, dtype=np.float32)
    frames = (x.size - nfft) // hop + 1
    out = np.empty((frames, nfft // 2 + 1), np.float32)
    fmax = np.empty(frames, np.float32)
    st = lib().sdsp_debug_stft(_fp(x), x.size, nfft, hop, gain, _fp(out), _fp(fmax), device)
    if st != 0:
        raise AnalysisError(st, "debug_stft failed")
    return out, fmax


class SdspDebugTempoOut(C.Structure):
    """sdsp_debug_tempo_out (include/stratum_hip_debug.h)."""
    _fields_ = ([(n, C.POINTER(C.c_float)) for n in ("E", "H", "SFX", "SFO", "MEL", "nov", "nov_sum", "acf", "fft")] +
                [("acf_n", C.POINTER(C.c_int32)), ("fft_n", C.POINTER(C.c_int32)),
                 ("mel_cap", C.c_uint32), ("acf_cap", C.c_uint32), ("fft_cap", C.c_uint32),
                 ("n_mels", C.c_int32), ("NB", C.c_int32),
                 ("bs", C.c_int32 * 4), ("be", C.c_int32 * 4), ("band_on", C.c_int32 * 4), ("present", C.c_int32 * 5)])


def _packed_specs(specs, bins=None):
    arrs = [np.ascontiguousarray(s, dtype=np.float32) for s in specs]
    if not arrs or any(a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != arrs[0].shape[1] for a in arrs):
        raise ValueError("tracks are (frames >= 1, bins) arrays of one width")
    if bins is not None and arrs[0].shape[1] != bins:
        raise ValueError(f"rows of {bins} bins expected")
    frames = np.array([a.shape[0] for a in arrs], np.uint64)
    return np.ascontiguousarray(np.concatenate(arrs, axis=0)), frames


VARIANTS = ("full", "low", "mid", "high", "mel")


def debug_tempo_stages(specs, sample_rate=44100, hop=512, config=None, device=0):
    """The tempo pass's stages over host magnitude spectrograms (sdsp_debug_tempo_stages): a list of
    tracks, each (frames, frame_size / 2 + 1).  Returns (meta, tracks): meta holds bs, be, band_on,
    present, n_mels, NB; tracks[t] holds E, H (4, F), SFX (4, F - 1), SFO (F - 1), MEL (n_mels, F),
    nov {variant: F - 1 values}, nov_sum {variant: value}, acf / fft {variant: (n, 2) array of
    (bpm, value) in the kernels' order} for the present variants."""
    cfg = config if config is not None else default_config()
    x, frames = _packed_specs(specs, int(cfg.frame_size) // 2 + 1)
    T, total = len(frames), int(frames.sum())
    mel_cap, acf_cap = 48, 512
    fft_cap = max(1 << max(int(f) - 2, 0).bit_length() for f in frames) // 2 + 1
    f32 = lambda *shape: np.zeros(shape, np.float32)
    buf = dict(E=f32(4, total), H=f32(4, total), SFX=f32(4, total), SFO=f32(total), MEL=f32(mel_cap, total),
               nov=f32(5, total), nov_sum=f32(5, T), acf=f32(T, 5, acf_cap, 2), fft=f32(T, 5, fft_cap, 2))
    acf_n, fft_n = np.zeros((T, 5), np.int32), np.zeros((T, 5), np.int32)
    o = SdspDebugTempoOut(mel_cap=mel_cap, acf_cap=acf_cap, fft_cap=fft_cap)
    for k, v in buf.items():
        setattr(o, k, _fp(v))
    i32p = C.POINTER(C.c_int32)
    o.acf_n, o.fft_n = acf_n.ctypes.data_as(i32p), fft_n.ctypes.data_as(i32p)
    f = lib().sdsp_debug_tempo_stages
    f.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(SdspConfig),
                  C.POINTER(SdspDebugTempoOut), C.c_int32]
    f.restype = C.c_int32
    st = f(_fp(x), frames.ctypes.data_as(C.POINTER(C.c_uint64)), T, sample_rate, hop, C.byref(cfg), C.byref(o), device)
    if st != 0:
        raise AnalysisError(st, "debug_tempo_stages failed")
    meta = dict(bs=list(o.bs), be=list(o.be), band_on=list(o.band_on), present=list(o.present), n_mels=o.n_mels,
                NB=o.NB)
    tracks, g0 = [], 0
    for t in range(T):
        F = int(frames[t])
        sl, pr = slice(g0, g0 + F), slice(g0, g0 + F - 1)
        on = [v for v in range(5) if o.present[v] and F >= 2]
        tracks.append(dict(
            E=buf["E"][:, sl].copy(), H=buf["H"][:, sl].copy(), SFX=buf["SFX"][:, pr].copy(), SFO=buf["SFO"][pr].copy(),
            MEL=buf["MEL"][:o.n_mels, sl].copy(),
            nov={VARIANTS[v]: buf["nov"][v, pr].copy() for v in on},
            nov_sum={VARIANTS[v]: buf["nov_sum"][v, t] for v in on},
            acf={VARIANTS[v]: buf["acf"][t, v, :acf_n[t, v]].copy() for v in on},
            fft={VARIANTS[v]: buf["fft"][t, v, :fft_n[t, v]].copy() for v in on}))
        g0 += F
    return meta, tracks


class SdspDebugTempoEst(C.Structure):
    """sdsp_debug_tempo_est (include/stratum_hip_debug.h)."""
    _fields_ = [("bpm", C.c_float), ("conf", C.c_float), ("agree", C.c_int32), ("ok", C.c_int32), ("n_cands", C.c_int32),
                ("ambiguous", C.c_int32), ("trap_low", C.c_int32), ("trap_high", C.c_int32)]


class SdspDebugMrDbg(C.Structure):
    """sdsp_debug_mr_dbg (include/stratum_hip_debug.h)."""
    _fields_ = ([(n, C.c_int32) for n in ("fd", "fu", "tf")] + [(n, C.c_float) for n in ("fd_from", "fd_to", "fd_ratio")] +
                [(n, C.c_int32) for n in ("fd_a0", "fd_a1")] + [(n, C.c_float) for n in ("fu_from", "fu_to", "fu_ratio")] +
                [(n, C.c_int32) for n in ("fu_a0", "fu_a1")] +
                [(n, C.c_float) for n in ("tf_from", "tf_to", "tf_sup0", "tf_sup1", "tf_al0", "tf_al1")] +
                [("tf_label", C.c_int32), ("rel", C.c_float)] + [(n, C.c_int32) for n in ("fam", "forbid", "better")])


class SdspDebugMultiresIn(C.Structure):
    """sdsp_debug_multires_in (include/stratum_hip_debug.h)."""
    _fields_ = ([(n, C.POINTER(C.c_float)) for n in ("c256", "c512", "c1024")] +
                [(n, C.POINTER(C.c_int32)) for n in ("n256", "n512", "n1024")] +
                [("cap_aux", C.c_uint32), ("cap_base", C.c_uint32), ("nov512", C.POINTER(C.c_float)),
                 ("nov_n", C.POINTER(C.c_uint64)), ("base", C.POINTER(SdspDebugTempoEst)),
                 ("items", C.POINTER(C.c_int32)), ("n_items", C.c_uint64), ("n_tracks", C.c_uint64),
                 ("own512", C.c_int32)])


class SdspDebugMultiresOut(C.Structure):
    """sdsp_debug_multires_out (include/stratum_hip_debug.h)."""
    _fields_ = [("mr", C.POINTER(SdspDebugTempoEst)), ("dbg", C.POINTER(SdspDebugMrDbg)), ("used", C.POINTER(C.c_int32)),
                ("final_bpm", C.POINTER(C.c_float)), ("final_conf", C.POINTER(C.c_float))]


def _est_dict(e):
    return dict(bpm=np.float32(e.bpm), conf=np.float32(e.conf), agree=e.agree, ok=e.ok, n_cands=e.n_cands,
                ambiguous=e.ambiguous, trap_low=e.trap_low, trap_high=e.trap_high)


def debug_tempo_select(tracks, present=(1, 1, 1, 1, 1), top_n=10, cand_cap=10, gate=False, config=None,
                       sample_rate=44100, device=0):
    """The candidate selection over host tempogram lists (sdsp_debug_tempo_select).  tracks: dicts of
    fft and acf ({variant name: (n, 2) array of (bpm, value)} for the present variants; the fft lists
    of one track share their length, the acf lists of the call theirs) and optionally active
    (default True).  Returns per track the TempoEst fields (bpm, conf, agree, ok, n_cands, ambiguous,
    trap_low, trap_high) and cands (n_cands, 4)."""
    cfg = config if config is not None else default_config()
    T = len(tracks)
    on = [VARIANTS[v] for v in range(5) if present[v]]

    def length(lists):
        ns = {np.asarray(lists[k], np.float32).reshape(-1, 2).shape[0] for k in on}
        if len(ns) != 1:
            raise ValueError("one list length per track over the present variants")
        return ns.pop()

    fft_n = np.array([length(t["fft"]) for t in tracks], np.int32)
    nbs = {length(t["acf"]) for t in tracks}
    if len(nbs) != 1:
        raise ValueError("one autocorrelation list length per call")
    NB = nbs.pop()
    fft = np.zeros((5 * int(fft_n.sum()) + 1, 2), np.float32)
    acf = np.zeros((T, 5, max(NB, 1), 2), np.float32)
    at = 0
    for t, trk in enumerate(tracks):
        K = int(fft_n[t])
        for v in range(5):
            if present[v]:
                fft[at + v * K:at + (v + 1) * K] = np.asarray(trk["fft"][VARIANTS[v]], np.float32).reshape(-1, 2)
                acf[t, v, :NB] = np.asarray(trk["acf"][VARIANTS[v]], np.float32).reshape(-1, 2)
        at += 5 * K
    acf = np.ascontiguousarray(acf[:, :, :NB]) if NB else acf
    active = np.array([1 if t.get("active", True) else 0 for t in tracks], np.int32)
    pres = (C.c_int32 * 5)(*[int(bool(p)) for p in present])
    est = (SdspDebugTempoEst * T)()
    cand = np.zeros((T, max(cand_cap, 1), 4), np.float32)
    f = lib().sdsp_debug_tempo_select
    fp, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    f.argtypes = [fp, i32p, fp, C.c_uint32, i32p, i32p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_uint32,
                  C.POINTER(SdspConfig), C.POINTER(SdspDebugTempoEst), fp, C.c_int32]
    f.restype = C.c_int32
    st = f(_fp(fft), fft_n.ctypes.data_as(i32p), _fp(acf), NB, pres, active.ctypes.data_as(i32p), T, top_n, cand_cap,
           int(bool(gate)), sample_rate, C.byref(cfg), est, _fp(cand), device)
    if st != 0:
        raise AnalysisError(st, "debug_tempo_select failed")
    out = []
    for t in range(T):
        d = _est_dict(est[t])
        d["cands"] = cand[t, :est[t].n_cands].copy()
        out.append(d)
    return out


def debug_multires(items, tracks, base, own512=False, cap_aux=None, cap_base=None, config=None, sample_rate=44100,
                   used=None, final_bpm=None, final_conf=None, device=0):
    """The multi-resolution fusion over host candidate lists (sdsp_debug_multires).  base: one
    (bpm, conf, agree, trap_low, trap_high) per track of the call; items: dicts of track (ascending),
    c256 and c1024 ((n, 4) arrays, or None for a failed hop) and, with own512, c512 and nov; tracks
    (without own512): one dict of c512 and nov per track of the call.  used / final_bpm / final_conf:
    the values uploaded first (default: 0 and the base estimate).  Returns (per item: the
    multi-resolution TempoEst fields and dbg, the MrDbg fields), used, final_bpm, final_conf."""
    cfg = config if config is not None else default_config()
    NR, NE = len(base), len(items)
    top_k = max(int(cfg.tempogram_multi_res_top_k), 1)
    rows = items if own512 else tracks

    def pack(lists, cap):
        n = np.array([-1 if a is None else len(a) for a in lists], np.int32)
        buf = np.zeros((max(len(lists), 1), cap, 4), np.float32)
        for r, a in enumerate(lists):
            if a is not None and len(a):  # a list longer than cap keeps its count: the probe refuses it
                buf[r, :min(len(a), cap)] = np.asarray(a, np.float32).reshape(-1, 4)[:cap]
        return buf, n

    lens = [len(a) for it in items for a in (it["c256"], it["c1024"]) if a is not None]
    cap_aux = cap_aux if cap_aux is not None else max(lens + [1])
    l512 = [r["c512"] for r in rows]
    cap_base = cap_base if cap_base is not None else max([len(a) for a in l512 if a is not None] + [1])
    cap512 = top_k if own512 else cap_base
    c256, n256 = pack([it["c256"] for it in items], cap_aux)
    c1024, n1024 = pack([it["c1024"] for it in items], cap_aux)
    c512, n512 = pack(l512, cap512)
    novs = [np.asarray(r["nov"], np.float32).ravel() for r in rows]
    nov_n = np.array([a.size for a in novs] + [0], np.uint64)
    nov = np.ascontiguousarray(np.concatenate(novs + [np.zeros(1, np.float32)]))
    b = (SdspDebugTempoEst * NR)()
    for t, e in enumerate(base):
        b[t].bpm, b[t].conf, b[t].agree, b[t].ok = e[0], e[1], int(e[2]), 1
        b[t].trap_low, b[t].trap_high = int(bool(e[3])), int(bool(e[4]))
    E = np.array([int(it["track"]) for it in items] + [0], np.int32)
    u = np.zeros(NR, np.int32) if used is None else np.array(used, np.int32)
    fb = np.array([e[0] for e in base], np.float32) if final_bpm is None else np.array(final_bpm, np.float32)
    fc = np.array([e[1] for e in base], np.float32) if final_conf is None else np.array(final_conf, np.float32)
    mr, dbg = (SdspDebugTempoEst * max(NE, 1))(), (SdspDebugMrDbg * max(NE, 1))()
    fp, i32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    i = SdspDebugMultiresIn(_fp(c256), _fp(c512), _fp(c1024), n256.ctypes.data_as(i32p), n512.ctypes.data_as(i32p),
                            n1024.ctypes.data_as(i32p), cap_aux, cap_base, _fp(nov), nov_n.ctypes.data_as(u64p), b,
                            E.ctypes.data_as(i32p), NE, NR, int(bool(own512)))
    o = SdspDebugMultiresOut(mr, dbg, u.ctypes.data_as(i32p), _fp(fb), _fp(fc))
    f = lib().sdsp_debug_multires
    f.argtypes = [C.POINTER(SdspDebugMultiresIn), C.c_uint32, C.POINTER(SdspConfig), C.POINTER(SdspDebugMultiresOut),
                  C.c_int32]
    f.restype = C.c_int32
    st = f(C.byref(i), sample_rate, C.byref(cfg), C.byref(o), device)
    if st != 0:
        raise AnalysisError(st, "debug_multires failed")
    out = []
    for k in range(NE):
        d = _est_dict(mr[k])
        d["dbg"] = {n: (np.float32(getattr(dbg[k], n)) if ty is C.c_float else getattr(dbg[k], n))
                    for n, ty in SdspDebugMrDbg._fields_}
        out.append(d)
    return out, u, fb, fc


KV_ROW = 128  # floats per segment scratch row of the key vote (csrc/kernels.hpp)


class SdspDebugKeyOut(C.Structure):
    _fields_ = [("mode", C.c_int32), ("tonic", C.c_int32), ("conf", C.c_float), ("clarity", C.c_float),
                ("ok", C.c_int32), ("used_segments", C.c_int32), ("weights_used", C.c_int32), ("near", C.c_int32)]


class SdspDebugKeyDbg(C.Structure):
    _fields_ = [("tab", C.c_float * 24), ("order", C.c_int32 * 24), ("key", C.c_int32), ("agg", C.c_float * 12),
                ("frames", C.c_int32), ("used", C.c_int32)]


class SdspDebugKeyVoteOut(C.Structure):
    _fields_ = [("key", C.POINTER(SdspDebugKeyOut)), ("chroma_s", C.POINTER(C.c_float)),
                ("weights", C.POINTER(C.c_float)), ("wdel", C.POINTER(C.c_float)), ("seg_rows", C.POINTER(C.c_float)),
                ("seg_row_pfx", C.POINTER(C.c_uint64)), ("seg_rows_cap", C.c_uint64), ("dbg", C.POINTER(SdspDebugKeyDbg))]


def _key_vote_rows_bound(cfg, F):
    """An upper bound of the vote's segment scratch rows for an F-row track (the pipeline's own
    sizing is checked by the probe against the capacity this gives)."""
    ns = 0
    if cfg.enable_key_segment_voting and cfg.key_segment_len_frames >= 120 and cfg.key_segment_hop_frames >= 1:
        L = max(int(cfg.key_segment_len_frames), 1)
        hop = max(min(int(cfg.key_segment_hop_frames), L), 1)
        ns = (F - L) // hop + 1 if F >= L else 0
    nm = 0
    if cfg.enable_key_multi_scale:
        hop = max(int(cfg.key_multi_scale_hop), 1)
        for j in range(int(cfg.key_multi_scale_lengths_len)):
            L = int(cfg.key_multi_scale_lengths[j])
            if L != 0 and L <= F:
                nm += (F - L) // hop + 1
    return max(ns, nm)


def debug_key_vote(tracks, edel=None, sel=None, config=None, threads=0, alone=False, cert_fixed=False, sample_rate=44100,
                   device=0):
    """The key vote over host chroma rows and frame energies (sdsp_debug_key_vote).  tracks: one
    (chroma (F, 12), energy (F,)) pair per track; edel: None (the exact path's launch) or one (F,)
    array of relative energy bounds per track (the band path's launch with its certificate); sel:
    None or the track indices to vote on.  Returns one dict per track: the KeyOut fields (mode,
    tonic, key, conf, clarity, ok, used_segments, weights_used, near; key = -1 and ok = -1 for a track
    outside sel, whose record the probe left as it was), chroma_s (F, 12), weights (F,), wdel (F,;
    with edel), and for a voted track rows (n, 128; the segment scratch rows sized for it) and dbg
    (tab, order, key, agg, frames, used)."""
    cfg = config if config is not None else default_config()
    T = len(tracks)
    frames = np.array([np.asarray(c).reshape(-1, 12).shape[0] for c, _ in tracks], np.uint64)
    total = int(frames.sum())
    ch = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1, 12) for c, _ in tracks]))
    en = np.ascontiguousarray(np.concatenate([np.asarray(e, np.float32).reshape(-1) for _, e in tracks]))
    if en.size != total:
        raise ValueError("one energy per chroma row")
    ed = None
    if edel is not None:
        ed = np.ascontiguousarray(np.concatenate([np.asarray(e, np.float32).reshape(-1) for e in edel]))
        if ed.size != total:
            raise ValueError("one energy bound per chroma row")
    items = list(range(T)) if sel is None else [int(s) for s in sel]
    sel_a = None if sel is None else np.ascontiguousarray(items, dtype=np.int32)
    cap = sum(_key_vote_rows_bound(cfg, int(frames[k])) for k in items if 0 <= k < T)
    key = (SdspDebugKeyOut * T)()
    for t in range(T):  # a sentinel the kernel never writes: untouched records stay recognisable
        key[t].mode, key[t].ok = -1, -1
    dbg = (SdspDebugKeyDbg * max(len(items), 1))()
    cs, w = np.zeros((total, 12), np.float32), np.zeros(total, np.float32)
    wd = np.zeros(total, np.float32)
    rows = np.zeros((max(cap, 1), KV_ROW), np.float32)
    pfx = np.zeros(len(items) + 1, np.uint64)
    out = SdspDebugKeyVoteOut(key, _fp(cs), _fp(w), _fp(wd), _fp(rows), pfx.ctypes.data_as(C.POINTER(C.c_uint64)), cap, dbg)
    f = lib().sdsp_debug_key_vote
    fp, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    f.argtypes = [fp, fp, fp, u64p, C.c_uint64, C.POINTER(C.c_int32), C.c_uint64, C.c_uint32, C.POINTER(SdspConfig),
                  C.c_int32, C.c_int32, C.c_int32, C.POINTER(SdspDebugKeyVoteOut), C.c_int32]
    f.restype = C.c_int32
    st = f(_fp(ch), _fp(en), _fp(ed) if ed is not None else None, frames.ctypes.data_as(u64p), T,
           sel_a.ctypes.data_as(C.POINTER(C.c_int32)) if sel_a is not None and sel_a.size else None,
           0 if sel_a is None else sel_a.size, sample_rate, C.byref(cfg), threads, int(bool(alone)), int(bool(cert_fixed)),
           C.byref(out), device)
    if st != 0:
        raise AnalysisError(st, "debug_key_vote failed")
    res, g0 = [], 0
    for t in range(T):
        sl = slice(g0, g0 + int(frames[t]))
        k = key[t]
        d = dict(mode=k.mode, tonic=k.tonic, key=k.mode * 12 + k.tonic if k.mode >= 0 else -1,
                 conf=np.float32(k.conf), clarity=np.float32(k.clarity), ok=k.ok, used_segments=k.used_segments,
                 weights_used=k.weights_used, near=k.near, chroma_s=cs[sl].copy(), weights=w[sl].copy())
        if ed is not None:
            d["wdel"] = wd[sl].copy()
        res.append(d)
        g0 += int(frames[t])
    for i, t in enumerate(items):
        g = dbg[i]
        res[t]["rows"] = rows[int(pfx[i]):int(pfx[i + 1])].copy()
        res[t]["dbg"] = dict(tab=np.array(g.tab[:], np.float32), order=np.array(g.order[:], np.int32), key=g.key,
                             agg=np.array(g.agg[:], np.float32), frames=g.frames, used=g.used)
    return res


def debug_key_stages(specs, sample_rate=44100, config=None, mode=0, device=0):
    """The key path's conditioning and chroma over host key spectrograms (sdsp_debug_key_stages;
    mode 0 the configured path, 1 the in-place rerun's sequence, 2 the nested rerun's).  Returns
    (info, tracks): info holds st_lo, st_hi, band, bins; tracks[t] holds masked (F, bins), chroma
    (F, 12), energy (F) and, on mode 0's band path, edel (F)."""
    cfg = config if config is not None else default_config()
    x, frames = _packed_specs(specs)
    T, total, bins = len(frames), int(frames.sum()), x.shape[1]
    masked, chroma = np.zeros((total, bins), np.float32), np.zeros((total, 12), np.float32)
    energy, edel = np.zeros(total, np.float32), np.full(total, np.nan, np.float32)
    info = (C.c_int32 * 4)()
    f = lib().sdsp_debug_key_stages
    fp = C.POINTER(C.c_float)
    f.argtypes = [fp, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint32, C.POINTER(SdspConfig), C.c_int32, fp, fp, fp, fp,
                  C.POINTER(C.c_int32), C.c_int32]
    f.restype = C.c_int32
    if key_fft_bins(cfg) != bins:
        raise ValueError(f"rows of {key_fft_bins(cfg)} bins expected")
    st = f(_fp(x), frames.ctypes.data_as(C.POINTER(C.c_uint64)), T, sample_rate, C.byref(cfg), mode, _fp(masked),
           _fp(chroma), _fp(energy), _fp(edel), info, device)
    if st != 0:
        raise AnalysisError(st, "debug_key_stages failed")
    meta = dict(st_lo=info[0], st_hi=info[1], band=bool(info[2]), bins=info[3])
    tracks, g0 = [], 0
    for t in range(T):
        sl = slice(g0, g0 + int(frames[t]))
        d = dict(masked=masked[sl].copy(), chroma=chroma[sl].copy(), energy=energy[sl].copy())
        if meta["band"] and mode == 0:
            d["edel"] = edel[sl].copy()
        tracks.append(d)
        g0 += int(frames[t])
    return meta, tracks


class SdspDebugOnsetOut(C.Structure):
    """sdsp_debug_onset_out (include/stratum_hip_debug.h)."""
    _fields_ = ([(n, C.POINTER(C.c_uint32)) for n in ("energy", "spectral", "hfc", "hpss", "chosen")] +
                [(n, C.POINTER(C.c_int32)) for n in ("n_energy", "n_spectral", "n_hfc", "n_hpss", "n_chosen")])


def debug_onset_stages(tracks, sample_rate=44100, hop=512, config=None, device=0):
    """The onset detectors and their consensus over per-frame curves (sdsp_debug_onset_stages).
    tracks: dicts of rms, hfc, sfo (F >= 1 values each; sfo may have F - 1), optionally hpe, and
    n_trim.  Returns per track a dict of the energy, spectral, hfc, hpss and chosen lists (uint32
    sample positions)."""
    cfg = config if config is not None else default_config()
    frames = np.array([np.asarray(t["rms"]).size for t in tracks], np.uint64)
    T, total = len(tracks), int(frames.sum())

    def curve(key):
        parts = []
        for t, F in zip(tracks, frames):
            a = np.asarray(t[key], dtype=np.float32).ravel()
            if key == "sfo" and a.size == int(F) - 1:
                a = np.concatenate([a, np.zeros(1, np.float32)])
            if a.size != int(F):
                raise ValueError(f"{key}: {int(F)} values expected")
            parts.append(a)
        return np.ascontiguousarray(np.concatenate(parts))

    rms, hfc, sfo = curve("rms"), curve("hfc"), curve("sfo")
    with_hpe = [t.get("hpe") is not None for t in tracks]
    if any(with_hpe) and not all(with_hpe):
        raise ValueError("hpe: for every track or none")
    hpe = curve("hpe") if all(with_hpe) and T else None
    n_trim = np.array([int(t["n_trim"]) for t in tracks], np.uint64)
    names = ("energy", "spectral", "hfc", "hpss", "chosen")
    u32p, i32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    lists = {k: np.zeros((4 if k == "chosen" else 1) * max(total, 1), np.uint32) for k in names}
    counts = {k: np.full(max(T, 1), -1, np.int32) for k in names}
    o = SdspDebugOnsetOut()
    for k in names:
        setattr(o, k, lists[k].ctypes.data_as(u32p))
        setattr(o, "n_" + k, counts[k].ctypes.data_as(i32p))
    f = lib().sdsp_debug_onset_stages
    fp = C.POINTER(C.c_float)
    f.argtypes = [fp, fp, fp, fp, u64p, u64p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(SdspConfig),
                  C.POINTER(SdspDebugOnsetOut), C.c_int32]
    f.restype = C.c_int32
    st = f(_fp(rms), _fp(hfc), _fp(sfo), _fp(hpe) if hpe is not None else None, frames.ctypes.data_as(u64p),
           n_trim.ctypes.data_as(u64p), T, sample_rate, hop, C.byref(cfg), C.byref(o), device)
    if st != 0:
        raise AnalysisError(st, "debug_onset_stages failed")
    out, g0 = [], 0
    for t in range(T):
        d = {}
        for k in names:
            at = (4 if k == "chosen" else 1) * g0
            d[k] = lists[k][at:at + int(counts[k][t])].copy()
        out.append(d)
        g0 += int(frames[t])
    return out


class SdspDebugBeatOut(C.Structure):
    """sdsp_debug_beat_out (include/stratum_hip_debug.h)."""
    _fields_ = ([(n, C.POINTER(C.c_int32)) for n in ("ok", "n_beats", "n_down")] +
                [(n, C.POINTER(C.c_float)) for n in ("stability", "beats", "downs")])


def debug_beat_grid(tracks, sample_rate=44100, config=None, device=0):
    """The beat stage over consensus onsets and tempo estimates (sdsp_debug_beat_grid).  tracks: dicts
    of onsets (ascending uint32 sample positions), frames, n_trim, bpm, conf.  Returns per track a dict
    of ok, beats, downbeats (float32 arrays; empty unless ok = 1) and stability (float32)."""
    cfg = config if config is not None else default_config()
    T = len(tracks)
    ons = [np.ascontiguousarray(t["onsets"], dtype=np.uint32).ravel() for t in tracks]
    n_on = np.array([a.size for a in ons], np.uint64)
    allon = np.ascontiguousarray(np.concatenate(ons + [np.zeros(1, np.uint32)]))
    frames = np.array([int(t["frames"]) for t in tracks], np.uint64)
    n_trim = np.array([int(t["n_trim"]) for t in tracks], np.uint64)
    bpm = np.array([t["bpm"] for t in tracks], np.float32)
    conf = np.array([t["conf"] for t in tracks], np.float32)
    cap = sum(max(12 * (int(n) // sample_rate + 1) + 64, 3 * int(F) + 8) for n, F in zip(n_trim, frames))
    ok, nb, nd = (np.zeros(max(T, 1), np.int32) for _ in range(3))
    stab, beats, downs = np.zeros(max(T, 1), np.float32), np.zeros(max(cap, 1), np.float32), np.zeros(max(cap, 1), np.float32)
    i32p, u64p = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    o = SdspDebugBeatOut(ok.ctypes.data_as(i32p), nb.ctypes.data_as(i32p), nd.ctypes.data_as(i32p), _fp(stab), _fp(beats),
                         _fp(downs))
    f = lib().sdsp_debug_beat_grid
    fp = C.POINTER(C.c_float)
    f.argtypes = [C.POINTER(C.c_uint32), u64p, u64p, u64p, fp, fp, C.c_uint64, C.c_uint32, C.POINTER(SdspConfig),
                  C.POINTER(SdspDebugBeatOut), C.c_int32]
    f.restype = C.c_int32
    st = f(allon.ctypes.data_as(C.POINTER(C.c_uint32)), n_on.ctypes.data_as(u64p), frames.ctypes.data_as(u64p),
           n_trim.ctypes.data_as(u64p), _fp(bpm), _fp(conf), T, sample_rate, C.byref(cfg), C.byref(o), device)
    if st != 0:
        raise AnalysisError(st, "debug_beat_grid failed")
    out, b0, d0 = [], 0, 0
    for t in range(T):
        kb, kd = (int(nb[t]), int(nd[t])) if ok[t] > 0 else (0, 0)
        out.append(dict(ok=int(ok[t]), beats=beats[b0:b0 + kb].copy(), downbeats=downs[d0:d0 + kd].copy(),
                        stability=stab[t].copy()))
        b0 += kb
        d0 += kd
    return out


def debug_sections(rows, energies, request, sample_rate=44100, khop=512, hop=512, device=0):
    """The sections kernels over uploaded chroma rows and frame energies (sdsp_debug_sections).
    rows[t]: (F_t, 12) float32, khop samples apart; energies[t]: (Fb_t,) float32, hop samples apart.
    Returns per track a dict with n_cells, m (n_cells, 12), g, novelty (float32) and boundary (uint8)."""
    T = len(rows)
    rs = [np.ascontiguousarray(r, np.float32).reshape(-1, 12) for r in rows]
    es = [np.ascontiguousarray(e, np.float32).ravel() for e in energies]
    frames = np.array([r.shape[0] for r in rs], np.uint64)
    bframes = np.array([e.size for e in es], np.uint64)
    allr = np.ascontiguousarray(np.concatenate([r.ravel() for r in rs] + [np.zeros(12, np.float32)]))
    alle = np.ascontiguousarray(np.concatenate(es + [np.zeros(1, np.float32)]))
    cs = int(request.cell_samples) or int(np.float32(request.cell_seconds) * np.float32(sample_rate))
    cap = sum(min(int(f) * khop, int(b) * hop) // cs for f, b in zip(frames, bframes)) if cs > 0 else 0
    nc = np.zeros(max(T, 1), np.uint64)
    m, g, nov = np.zeros(12 * max(cap, 1), np.float32), np.zeros(max(cap, 1), np.float32), np.zeros(max(cap, 1), np.float32)
    bnd = np.zeros(max(cap, 1), np.uint8)
    u64p = C.POINTER(C.c_uint64)
    o = SdspDebugSectionsOut(cap, nc.ctypes.data_as(u64p), _fp(m), _fp(g), _fp(nov), bnd.ctypes.data_as(C.POINTER(C.c_uint8)))
    f = lib().sdsp_debug_sections
    fp = C.POINTER(C.c_float)
    f.argtypes = [fp, u64p, fp, u64p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(SdspSectionsRequest),
                  C.POINTER(SdspDebugSectionsOut), C.c_int32]
    f.restype = C.c_int32
    st = f(_fp(allr), frames.ctypes.data_as(u64p), _fp(alle), bframes.ctypes.data_as(u64p), T, sample_rate, khop, hop,
           C.byref(request), C.byref(o), device)
    if st != 0:
        raise AnalysisError(st, "debug_sections failed")
    out, at = [], 0
    for t in range(T):
        k = int(nc[t])
        out.append(dict(n_cells=k, m=m[12 * at:12 * (at + k)].reshape(k, 12).copy(), g=g[at:at + k].copy(),
                        novelty=nov[at:at + k].copy(), boundary=bnd[at:at + k].copy()))
        at += k
    return out


def debug_fingerprint(rows, request, sample_rate=44100, khop=512, device=0):
    """k_fp_cells and k_fp_words over uploaded chroma rows (sdsp_debug_fingerprint).  rows[t]:
    (F_t, 12) float32, khop samples apart.  Returns per track a dict with n_cells, n_words,
    m (n_cells, 12) float32 and words (uint32)."""
    T = len(rows)
    rs = [np.ascontiguousarray(r, np.float32).reshape(-1, 12) for r in rows]
    frames = np.array([r.shape[0] for r in rs], np.uint64)
    allr = np.ascontiguousarray(np.concatenate([r.ravel() for r in rs] + [np.zeros(12, np.float32)]))
    cs = int(request.cell_samples) or int(np.float32(request.cell_seconds) * np.float32(sample_rate))
    cells = [int(f) * khop // cs for f in frames] if cs > 0 else [0] * T
    cap, wcap = sum(cells), sum(max(c - 2, 0) for c in cells)
    nc, nw = np.zeros(max(T, 1), np.uint64), np.zeros(max(T, 1), np.uint64)
    m, words = np.zeros(12 * max(cap, 1), np.float32), np.zeros(max(wcap, 1), np.uint32)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    o = SdspDebugFingerprintOut(cap, wcap, nc.ctypes.data_as(u64p), nw.ctypes.data_as(u64p), _fp(m),
                                words.ctypes.data_as(u32p))
    f = lib().sdsp_debug_fingerprint
    f.argtypes = [C.POINTER(C.c_float), u64p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(SdspFingerprintRequest),
                  C.POINTER(SdspDebugFingerprintOut), C.c_int32]
    f.restype = C.c_int32
    st = f(_fp(allr), frames.ctypes.data_as(u64p), T, sample_rate, khop, C.byref(request), C.byref(o), device)
    if st != 0:
        raise AnalysisError(st, "debug_fingerprint failed")
    out, at, wat = [], 0, 0
    for t in range(T):
        k, w = int(nc[t]), int(nw[t])
        out.append(dict(n_cells=k, n_words=w, m=m[12 * at:12 * (at + k)].reshape(k, 12).copy(), words=words[wat:wat + w].copy()))
        at += k
        wat += w
    return out


def debug_fingerprint_match(words, request, device=0):
    """k_fp_match over uploaded word arrays (sdsp_debug_fingerprint_match), every track compared.
    words[t]: uint32, at least one word.  Returns a record array (T, T) with offset_words, eligible,
    bit_errors, positions: the pair (a, b), a < b, at [a, b], the other entries zero."""
    T = len(words)
    ws = [np.ascontiguousarray(w, np.uint32).ravel() for w in words]
    nw = np.array([w.size for w in ws], np.uint64)
    allw = np.ascontiguousarray(np.concatenate(ws))
    rec = (SdspDebugFingerprintPair * (T * T))()
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    f = lib().sdsp_debug_fingerprint_match
    f.argtypes = [u32p, u64p, C.c_uint64, C.POINTER(SdspFingerprintRequest), C.POINTER(SdspDebugFingerprintPair), C.c_int32]
    f.restype = C.c_int32
    st = f(allw.ctypes.data_as(u32p), nw.ctypes.data_as(u64p), T, C.byref(request), rec, device)
    if st != 0:
        raise AnalysisError(st, "debug_fingerprint_match failed")
    return np.frombuffer(bytes(rec), dtype=np.dtype(SdspDebugFingerprintPair)).reshape(T, T).copy()


def debug_tempo_map(tracks, what=("segments", "onsets"), sample_rate=44100, config=None, device=0):
    """The beat stage with the tempo map step behind it (sdsp_debug_tempo_map).  tracks: as
    debug_beat_grid's.  Returns (maps, grids): per track a tempo_map_to_dict(), and what
    debug_beat_grid returns, from the same launch."""
    cfg = config if config is not None else default_config()
    req = tempo_map_request(what)
    T = len(tracks)
    ons = [np.ascontiguousarray(t["onsets"], dtype=np.uint32).ravel() for t in tracks]
    n_on = np.array([a.size for a in ons], np.uint64)
    allon = np.ascontiguousarray(np.concatenate(ons + [np.zeros(1, np.uint32)]))
    frames = np.array([int(t["frames"]) for t in tracks], np.uint64)
    n_trim = np.array([int(t["n_trim"]) for t in tracks], np.uint64)
    bpm = np.array([t["bpm"] for t in tracks], np.float32)
    conf = np.array([t["conf"] for t in tracks], np.float32)
    cap = sum(max(12 * (int(n) // sample_rate + 1) + 64, 3 * int(F) + 8) for n, F in zip(n_trim, frames))
    ok, nb, nd = (np.zeros(max(T, 1), np.int32) for _ in range(3))
    stab, beats, downs = np.zeros(max(T, 1), np.float32), np.zeros(max(cap, 1), np.float32), np.zeros(max(cap, 1), np.float32)
    i32p, u64p = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    o = SdspDebugBeatOut(ok.ctypes.data_as(i32p), nb.ctypes.data_as(i32p), nd.ctypes.data_as(i32p), _fp(stab), _fp(beats),
                         _fp(downs))
    maps = (SdspTempoMap * max(T, 1))()
    f = lib().sdsp_debug_tempo_map
    fp = C.POINTER(C.c_float)
    f.argtypes = [C.POINTER(C.c_uint32), u64p, u64p, u64p, fp, fp, C.c_uint64, C.c_uint32, C.POINTER(SdspConfig),
                  C.c_uint32, C.POINTER(SdspTempoMap), C.POINTER(SdspDebugBeatOut), C.c_int32]
    f.restype = C.c_int32
    st = f(allon.ctypes.data_as(C.POINTER(C.c_uint32)), n_on.ctypes.data_as(u64p), frames.ctypes.data_as(u64p),
           n_trim.ctypes.data_as(u64p), _fp(bpm), _fp(conf), T, sample_rate, C.byref(cfg), req.what, maps, C.byref(o),
           device)
    if st != 0:
        raise AnalysisError(st, "debug_tempo_map failed")
    out, grids, b0, d0 = [], [], 0, 0
    for t in range(T):
        out.append(tempo_map_to_dict(maps[t]))
        lib().sdsp_tempo_map_free(C.byref(maps[t]))
        kb, kd = (int(nb[t]), int(nd[t])) if ok[t] > 0 else (0, 0)
        grids.append(dict(ok=int(ok[t]), beats=beats[b0:b0 + kb].copy(), downbeats=downs[d0:d0 + kd].copy(),
                          stability=stab[t].copy()))
        b0 += kb
        d0 += kd
    return out, grids


def key_fft_bins(cfg):
    """Bins per row of the key spectrogram: the override's frame size (>= 256), else frame_size."""
    n = max(int(cfg.key_stft_frame_size), 256) if cfg.enable_key_stft_override else int(cfg.frame_size)
    return n // 2 + 1


def last_tail_reruns(device=0):
    """Tracks the last analysis call reran in place (sdsp_debug_last_tail_reruns)."""
    f = lib().sdsp_debug_last_tail_reruns
    f.argtypes = [C.c_int32, C.POINTER(C.c_uint64)]
    f.restype = C.c_int32
    n = C.c_uint64()
    if f(device, C.byref(n)) != 0:
        raise RuntimeError("sdsp_debug_last_tail_reruns failed")
    return int(n.value)
