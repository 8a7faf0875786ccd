#!/usr/bin/env python3
"""What a levels request costs an analysis call, on the benchmark's own workload.

bench.py's batch (1,024 synthetic three-minute 44.1 kHz tracks, seeds 0 .., AnalysisConfig::default())
is generated once in HBM and analysed in this one process, warm, --reps times (default 5, at least 5)
in each of four legs, interleaved so that every leg sees the same machine state:

  none          (a) sdsp_analyze_batch_device_with with set = NULL (sdsp_analyze_batch_device_ex itself)
  levels        (b) all four bits: the folds run on the vote stream beside the first sub-batch
  loud          (d) normalization = Loudness, no request: k_loudness_gain before the sub-batches
  loud_levels   (d) normalization = Loudness with all four bits: one fold (k_levels_fold) gives the
                configured gain and the levels; k_loudness_gain does not run

A leg's time is the wall time of the C entry.  Reported: every repetition, the median of each leg,
(b) - (a), (d with) - (d without), and the fold launches' HIP event times of each leg's last call
(sdsp_debug_last_levels_times).  (c), the levels kernels alone on an idle device, is the first
launch's event time of the loud_levels leg: there the pipeline waits for that launch before the
first sub-batch starts, so nothing runs beside it (peak kernels and the three first-launch chains).
The second launch (Loudness' rms_db chain) always runs beside a sub-batch; its event time includes
what it waited for and is reported as measured.  Written to --out (default profiles/levels.json)
and printed as one JSON line.

  python tools/levels_bench.py [--tracks 1024] [--seconds 180] [--reps 5] [--out PATH]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels.json"))
    args = ap.parse_args()
    import sdsp
    from sdsp_abi import SdspLevels, SdspRequestSet, SdspResult

    reps = max(args.reps, 5)
    sr, n = 44100, args.tracks
    L = int(args.seconds * sr)
    lens = np.full(n, L, np.uint64)
    offs = (np.arange(n, dtype=np.uint64) * np.uint64(L)).astype(np.uint64)
    buf = sdsp.DeviceBuffer(n * L, device=args.device)
    sdsp.generate_synthetic(buf.ptr, n, L, sr, seed0=0, bpm_mode=0, device=args.device)
    cfg, loud = sdsp.default_config(), sdsp.default_config()
    loud.normalization = 2
    lib = sdsp.lib()
    u64p = C.POINTER(C.c_uint64)
    req = sdsp.levels_request(15)
    legs = {"none": (cfg, False), "levels": (cfg, True), "loud": (loud, False), "loud_levels": (loud, True)}

    def call(c, with_req):
        outs = (SdspResult * n)()
        lvs = (SdspLevels * n)() if with_req else None
        rs = SdspRequestSet()
        rs.struct_size = C.sizeof(rs)
        if with_req:
            rs.lv_req = C.pointer(req)
            rs.levels = lvs
        t = time.perf_counter()
        st = lib.sdsp_analyze_batch_device_with(C.c_void_p(buf.ptr), offs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), n,
                                                sr, C.byref(c), args.device, None, 0, outs, C.byref(rs) if with_req else None)
        dt = time.perf_counter() - t
        assert st == 0, outs[0].error_message
        errors = sum(1 for i in range(n) if outs[i].status != 0)
        regions = 0
        for i in range(n):
            lib.sdsp_result_free(C.byref(outs[i]))
            if lvs is not None:
                errors += lvs[i].status != 0
                regions += int(lvs[i].n_regions)
                lib.sdsp_levels_free(C.byref(lvs[i]))
        return dt, errors, regions

    clock = None
    try:
        import bench

        clock = bench.ClockSampler(args.device)
        clock.__enter__()
    except Exception:
        clock = None
    for c, w in legs.values():  # warm: the grow-only buffers reach their size
        call(c, w)
    secs = {k: [] for k in legs}
    last = {}
    for _ in range(reps):
        for name, (c, w) in legs.items():
            dt, errors, regions = call(c, w)
            assert errors == 0
            secs[name].append(dt)
            last[name] = dict(sdsp.levels_times(args.device), regions=regions)
    if clock:
        clock.__exit__(None, None, None)
    res = {"tool": "tools/levels_bench.py", "tracks": n, "seconds_per_track": args.seconds, "reps": reps,
           "workload": f"{n} synthetic {args.seconds:.0f}-s 44.1 kHz mono tracks (bench.py's generator, seeds 0 ..), "
                       "full analysis, one process, legs interleaved", "legs": {}}
    for name in legs:
        med = statistics.median(secs[name])
        leg = {"seconds": [round(v, 4) for v in secs[name]], "median_seconds": round(med, 4), "tracks_per_s": round(n / med, 1)}
        if legs[name][1]:
            t = last[name]
            leg["folds_last_call"] = {"tracks": t["tracks"], "first_launch_ms": round(t["fold_ms"], 3),
                                      "second_launch_ms": round(t["fold2_ms"], 3), "regions": t["regions"]}
        res["legs"][name] = leg
    m = {k: res["legs"][k]["median_seconds"] for k in legs}
    res["b_minus_a_ms"] = round(1e3 * (m["levels"] - m["none"]), 2)
    res["d_with_minus_without_ms"] = round(1e3 * (m["loud_levels"] - m["loud"]), 2)
    res["c_first_launch_idle_ms"] = res["legs"]["loud_levels"]["folds_last_call"]["first_launch_ms"]
    res["c_second_launch_beside_sub_batch_ms"] = res["legs"]["loud_levels"]["folds_last_call"]["second_launch_ms"]
    res["step_cost_levels_vs_none"] = round(m["levels"] / m["none"] - 1.0, 4)
    res["step_cost_loud_levels_vs_loud"] = round(m["loud_levels"] / m["loud"] - 1.0, 4)
    res["sclk_mhz"] = clock.report() if clock else None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
