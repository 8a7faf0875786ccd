#!/usr/bin/env python3
"""What a key timeline request costs an analysis call, on the benchmark's own workload.

bench.py's batch (1,024 synthetic three-minute 44.1 kHz tracks, seeds 0 .., AnalysisConfig::default())
is generated once in HBM and analysed in this one process, warm, --reps times (default 5, at least 5)
in each of two legs, as alternating pairs so that both legs see the same machine state:

  none      sdsp_analyze_batch_device_requests with both requests NULL (sdsp_analyze_batch_device_ex itself)
  timeline  segment_seconds = 8, overlap_seconds = 2: 689 key frames every 517, 29 segments per track

A leg's time is the wall time of the C entry (results and timelines produced, nothing converted to
Python objects).  Reported: every repetition, each leg's median tracks/s, the timeline leg's cost
against the other leg of the same run (never against a number from elsewhere), the segments
returned, and the shader clock sampled during the run.  Written to --out (default
profiles/key_timeline.json) and printed as one JSON line.

  python tools/key_timeline_bench.py [--tracks 1024] [--seconds 180] [--reps 5] [--out PATH]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_timeline.json"))
    args = ap.parse_args()
    import sdsp
    from sdsp_abi import SdspKeyTimeline, SdspResult

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
    legs = {"none": None, "timeline": sdsp.key_timeline_request(segment_seconds=8.0, overlap_seconds=2.0)}

    def call(req):
        outs = (SdspResult * n)()
        kts = (SdspKeyTimeline * n)() if req is not None else None
        t = time.perf_counter()
        st = lib.sdsp_analyze_batch_device_requests(C.c_void_p(buf.ptr), offs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p),
                                                    n, sr, C.byref(cfg), args.device, None, 0, outs, None, None,
                                                    C.byref(req) if req is not None else None, kts)
        dt = time.perf_counter() - t
        assert st == 0, outs[0].error_message
        errors = sum(1 for i in range(n) if outs[i].status != 0)
        segs = sum(int(kts[i].n_segments) for i in range(n)) if kts is not None else 0
        chg = sum(int(kts[i].n_changes) for i in range(n)) if kts is not None else 0
        for i in range(n):
            lib.sdsp_result_free(C.byref(outs[i]))
            if kts is not None:
                lib.sdsp_key_timeline_free(C.byref(kts[i]))
        return dt, errors, segs, chg

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
            dt, errors, segs, chg = call(req)
            assert errors == 0
            secs[name].append(dt)
            last[name] = dict(segments=segs, changes=chg, stage_times=sdsp.stage_times(args.device))
    if clock:
        clock.__exit__(None, None, None)
    res = {"tool": "tools/key_timeline_bench.py", "tracks": n, "seconds_per_track": args.seconds, "reps": reps,
           "workload": f"{n} synthetic {args.seconds:.0f}-s 44.1 kHz mono tracks (bench.py's generator, seeds 0 ..), "
                       "AnalysisConfig::default(), full analysis, one process, legs in alternating pairs",
           "legs": {}}
    for name in legs:
        med = statistics.median(secs[name])
        leg = {"seconds": [round(v, 4) for v in secs[name]], "median_seconds": round(med, 4),
               "tracks_per_s": round(n / med, 1), "key_ms_last_call": round(last[name]["stage_times"]["key_ms"], 2),
               "total_ms_last_call": round(last[name]["stage_times"]["total_ms"], 2)}
        if legs[name] is not None:
            leg["request"] = {"segment_seconds": 8.0, "overlap_seconds": 2.0, "min_change_confidence": -1.0}
            leg["segments_returned"] = last[name]["segments"]
            leg["changes_returned"] = last[name]["changes"]
        res["legs"][name] = leg
    res["legs"]["timeline"]["step_cost_vs_none"] = round(
        res["legs"]["timeline"]["median_seconds"] / res["legs"]["none"]["median_seconds"] - 1.0, 4)
    res["pairwise_cost"] = [round(b / a - 1.0, 4) for a, b in zip(secs["none"], secs["timeline"])]
    res["sclk_mhz"] = clock.report() if clock else None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
