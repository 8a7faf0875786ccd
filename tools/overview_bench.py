#!/usr/bin/env python3
"""What an overview request costs an analysis call, on the benchmark's own workload.

bench.py's batch (1,024 synthetic three-minute 44.1 kHz tracks, seeds 0 .., AnalysisConfig::default())
is generated once in HBM and analysed in this one process, warm, --reps times (default 5, at least 5)
in each of three legs, interleaved so that every leg sees the same machine state:

  none      sdsp_analyze_batch_device_overview with req = NULL (sdsp_analyze_batch_device_ex itself)
  columns   columns = 1024: about 15 frames per column
  frames    frames_per_column = 1: one column per frame, the cross-lane fold paid per frame and
            the most output (5 x 4 bytes per frame to download and hand over)

A leg's time is the wall time of the C entry (results and overviews produced, nothing converted to
Python objects).  Reported: every repetition, the median tracks/s of each leg, the two kernels' HIP
event times of each leg's last call (sdsp_debug_last_overview_times) and their bytes per second by
the definition's byte counts beside the chip's measured read ceiling (6.29 TB/s,
profiles/r04j_hbm_ceiling.txt), and the shader clock sampled during the run.  Written to --out
(default profiles/overview.json) and printed as one JSON line.

  python tools/overview_bench.py [--tracks 1024] [--seconds 180] [--reps 5] [--out PATH]
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

HBM_READ_CEILING_GBS = 6290.0  # profiles/r04j_hbm_ceiling.txt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overview.json"))
    args = ap.parse_args()
    import sdsp
    from sdsp_abi import SdspOverview, SdspResult

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
    legs = {"none": None, "columns": sdsp.overview_request(columns=1024), "frames": sdsp.overview_request(frames_per_column=1)}

    def call(req):
        outs = (SdspResult * n)()
        ovs = (SdspOverview * n)() if req is not None else None
        t = time.perf_counter()
        st = lib.sdsp_analyze_batch_device_overview(C.c_void_p(buf.ptr), offs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p),
                                                    n, sr, C.byref(cfg), args.device, None, 0, outs,
                                                    C.byref(req) if req is not None else None, ovs)
        dt = time.perf_counter() - t
        assert st == 0, outs[0].error_message
        errors = sum(1 for i in range(n) if outs[i].status != 0)
        cols = sum(int(ovs[i].n_columns) for i in range(n)) if ovs is not None else 0
        for i in range(n):
            lib.sdsp_result_free(C.byref(outs[i]))
            if ovs is not None:
                lib.sdsp_overview_free(C.byref(ovs[i]))
        return dt, errors, cols

    clock = None
    try:
        import bench

        clock = bench.ClockSampler(args.device)
        clock.__enter__()
    except Exception:
        clock = None
    for req in legs.values():  # warm: the grow-only buffers reach their size
        call(req)
    secs = {k: [] for k in legs}
    last = {}
    for _ in range(reps):
        for name, req in legs.items():
            dt, errors, cols = call(req)
            assert errors == 0
            secs[name].append(dt)
            last[name] = dict(sdsp.overview_times(args.device), columns_returned=cols)
    if clock:
        clock.__exit__(None, None, None)
    res = {"tool": "tools/overview_bench.py", "tracks": n, "seconds_per_track": args.seconds, "reps": reps,
           "workload": f"{n} synthetic {args.seconds:.0f}-s 44.1 kHz mono tracks (bench.py's generator, seeds 0 ..), "
                       "AnalysisConfig::default(), full analysis, one process, legs interleaved",
           "hbm_read_ceiling_GBps": HBM_READ_CEILING_GBS, "legs": {}}
    for name in legs:
        med = statistics.median(secs[name])
        leg = {"seconds": [round(v, 4) for v in secs[name]], "median_seconds": round(med, 4),
               "tracks_per_s": round(n / med, 1)}
        if legs[name] is not None:
            t = last[name]
            leg["request"] = {"columns": legs[name].columns, "frames_per_column": legs[name].frames_per_column}
            leg["kernels_last_call"] = {
                "sub_batches": t["sub_batches"], "columns": t["columns"],
                "k_ov_segments_ms": round(t["sample_ms"], 3), "k_ov_segments_bytes": t["sample_bytes"],
                "k_ov_segments_GBps": round(t["sample_bytes"] / t["sample_ms"] / 1e6, 1) if t["sample_ms"] else None,
                "k_ov_columns_ms": round(t["band_ms"], 3), "k_ov_columns_bytes": t["band_bytes"],
                "k_ov_columns_GBps": round(t["band_bytes"] / t["band_ms"] / 1e6, 1) if t["band_ms"] else None,
            }
            k = leg["kernels_last_call"]
            for key in ("k_ov_segments_GBps", "k_ov_columns_GBps"):
                k[key.replace("GBps", "frac_of_ceiling")] = round(k[key] / HBM_READ_CEILING_GBS, 3) if k[key] else None
        res["legs"][name] = leg
    base = res["legs"]["none"]["median_seconds"]
    for name in ("columns", "frames"):
        res["legs"][name]["step_cost_vs_none"] = round(res["legs"][name]["median_seconds"] / base - 1.0, 4)
    res["sclk_mhz"] = clock.report() if clock else None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
