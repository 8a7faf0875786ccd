#!/usr/bin/env python3
"""What a programme loudness request costs an analysis call, on the benchmark's own workload, beside
the levels request's sequential loudness fold it is meant to beat.

bench.py's batch (1,024 synthetic three-minute 44.1 kHz tracks, seeds 0 .., AnalysisConfig::default())
is generated once in HBM and analysed in this one process, warm, --reps times (default 7, at least 5)
in each of four legs that alternate (the order flips from one repetition to the next):

  none        sdsp_analyze_batch_device_with with set = NULL (sdsp_analyze_batch_device_ex itself)
  loudness    SDSP_R128_LOUDNESS: the step energies and the per-track kernel, and the sample peak
  full        SDSP_R128_LOUDNESS | SDSP_R128_TRUE_PEAK: also the 4x-interpolated true peak
  levels      the levels request with SDSP_LEVELS_LOUDNESS alone: one sequential fold per track

A leg's time is the wall time of the C entry.  Reported: every repetition, each leg's median and
spread (max - min), each leg's median minus none's, and of the r128 legs' last call the HIP event
times of the three kernels (sdsp_debug_last_r128_times; they lie on the vote stream beside the first
sub-batch, so they include what the kernels shared the device with) with the steps measured.  A
"bench_py" member already in --out (bench.py on the parent commit's build and on this one,
alternating, recorded beside this tool's result) is kept.  Written to --out (default
profiles/r128.json) and printed as one JSON line.

  python tools/r128_bench.py [--tracks 1024] [--seconds 180] [--reps 7] [--out PATH]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stratum-dsp_amd", "python"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r128.json"))
    args = ap.parse_args()
    import sdsp
    from sdsp_abi import SdspLevels, SdspR128, SdspRequestSetExt2, SdspResult

    reps = max(args.reps, 5)
    sr, n = 44100, args.tracks
    L = int(args.seconds * sr)
    lens = np.full(n, L, np.uint64)
    offs = (np.arange(n, dtype=np.uint64) * np.uint64(L)).astype(np.uint64)
    buf = sdsp.DeviceBuffer(n * L, device=args.device)
    sdsp.generate_synthetic(buf.ptr, n, L, sr, seed0=0, bpm_mode=0, device=args.device)
    cfg = sdsp.default_config()
    lib = sdsp.lib()
    u64p = C.POINTER(C.c_uint64)
    legs = {"none": None, "loudness": ("r128", sdsp.loudness_request(1)), "full": ("r128", sdsp.loudness_request(3)),
            "levels": ("levels", sdsp.levels_request(("loudness",)))}

    def call(leg):
        outs = (SdspResult * n)()
        ext2 = SdspRequestSetExt2()
        rs = ext2.base.base
        rs.struct_size = C.sizeof(ext2)
        r128s = lvs = None
        if leg is not None and leg[0] == "r128":
            r128s = (SdspR128 * n)()
            ext2.r128_req = C.pointer(leg[1])
            ext2.r128 = r128s
        elif leg is not None:
            lvs = (SdspLevels * n)()
            rs.lv_req = C.pointer(leg[1])
            rs.levels = lvs
        t = time.perf_counter()
        st = lib.sdsp_analyze_batch_device_with(C.c_void_p(buf.ptr), offs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), n,
                                                sr, C.byref(cfg), args.device, None, 0, outs, C.byref(rs) if leg is not None else None)
        dt = time.perf_counter() - t
        assert st == 0, outs[0].error_message
        errors = sum(1 for i in range(n) if outs[i].status != 0)
        lufs = []
        for i in range(n):
            lib.sdsp_result_free(C.byref(outs[i]))
            if r128s is not None:
                errors += r128s[i].status != 0
                lufs.append(float(r128s[i].integrated_lufs))
                lib.sdsp_r128_free(C.byref(r128s[i]))
            if lvs is not None:
                errors += lvs[i].status != 0
                lib.sdsp_levels_free(C.byref(lvs[i]))
        return dt, errors, lufs

    clock = None
    try:
        import bench

        clock = bench.ClockSampler(args.device)
        clock.__enter__()
    except Exception:
        clock = None
    for leg in legs.values():  # warm: the grow-only buffers reach their size
        call(leg)
    secs = {k: [] for k in legs}
    last = {}
    names = list(legs)
    for r in range(reps):
        for name in (names if r % 2 == 0 else names[::-1]):
            dt, errors, lufs = call(legs[name])
            assert errors == 0
            secs[name].append(dt)
            if legs[name] is not None and legs[name][0] == "r128":
                last[name] = dict(sdsp.r128_times(args.device), median_integrated_lufs=round(statistics.median(lufs), 3))
            elif legs[name] is not None:
                last[name] = sdsp.levels_times(args.device)
    if clock:
        clock.__exit__(None, None, None)
    res = {"tool": "tools/r128_bench.py", "tracks": n, "seconds_per_track": args.seconds, "reps": reps,
           "workload": f"{n} synthetic {args.seconds:.0f}-s 44.1 kHz mono tracks (bench.py's generator, seeds 0 ..), "
                       "full analysis, one process, legs alternating", "legs": {}}
    for name in legs:
        med = statistics.median(secs[name])
        leg = {"seconds": [round(v, 4) for v in secs[name]], "median_seconds": round(med, 4),
               "spread_seconds": round(max(secs[name]) - min(secs[name]), 4), "tracks_per_s": round(n / med, 1)}
        if name in last and "steps_ms" in last[name]:
            t = last[name]
            leg["r128_last_call"] = {"tracks": t["tracks"], "steps": t["steps"], "k_r128_steps_ms": round(t["steps_ms"], 3),
                                     "k_r128_track_ms": round(t["track_ms"], 3), "k_r128_peak_ms": round(t["peak_ms"], 3),
                                     "median_integrated_lufs": t["median_integrated_lufs"]}
        elif name in last:
            leg["levels_last_call"] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in last[name].items()}
        res["legs"][name] = leg
    m = {k: res["legs"][k]["median_seconds"] for k in legs}
    for k in names[1:]:
        res[f"{k}_minus_none_ms"] = round(1e3 * (m[k] - m["none"]), 2)
    res["sclk_mhz"] = clock.report() if clock else None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        prev = {}
        if os.path.exists(args.out):  # keep the bench.py comparison recorded beside it
            try:
                prev = json.load(open(args.out))
            except Exception:
                prev = {}
        if "bench_py" in prev:
            res["bench_py"] = prev["bench_py"]
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
