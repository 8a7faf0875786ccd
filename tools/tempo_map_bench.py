#!/usr/bin/env python3
"""What a tempo map request costs an analysis call, on the benchmark's own workload.

bench.py's batch (1,024 synthetic three-minute 44.1 kHz tracks, seeds 0 .., AnalysisConfig::default())
is generated once in HBM and analysed in this one process, warm, --reps times (default 7, at least 5)
in each of three legs, interleaved so that every leg sees the same machine state (the order of the
legs rotates from one repetition to the next, so no leg always follows the same one):

  none       sdsp_analyze_batch_device_with with set = NULL (sdsp_analyze_batch_device_ex itself)
  segments   SDSP_TEMPO_MAP_SEGMENTS: k_tempo_map behind k_beat, its maps and segments downloaded
  both       ... and SDSP_TEMPO_MAP_ONSETS: the onset gather and its download

A leg's time is the wall time of the C entry.  Reported: every repetition, each leg's median and
spread (max - min), both - none and segments - none, and of each leg's last call the beat stage's
time (sdsp_last_stage_times' beat_ms: k_beat's HIP events) beside k_tempo_map's own event time
(sdsp_debug_last_tempo_map_times), so the added kernel can be set against the stage it follows.
A "bench_py" member already in --out (bench.py on the parent commit's build and on this one,
alternating, recorded beside this tool's result) is kept.  Written to --out (default
profiles/tempo_map.json) and printed as one JSON line.

  python tools/tempo_map_bench.py [--tracks 1024] [--seconds 180] [--reps 7] [--out PATH]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempo_map.json"))
    args = ap.parse_args()
    import sdsp
    from sdsp_abi import SdspRequestSet, SdspResult, SdspTempoMap

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
    legs = {"none": None, "segments": sdsp.tempo_map_request(("segments",)), "both": sdsp.tempo_map_request()}

    def call(req):
        outs = (SdspResult * n)()
        tms = (SdspTempoMap * n)() if req is not None else None
        rs = SdspRequestSet()
        rs.struct_size = C.sizeof(rs)
        if req is not None:
            rs.tm_req = C.pointer(req)
            rs.tempo_maps = tms
        t = time.perf_counter()
        st = lib.sdsp_analyze_batch_device_with(C.c_void_p(buf.ptr), offs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), n,
                                                sr, C.byref(cfg), args.device, None, 0, outs, C.byref(rs) if req is not None else None)
        dt = time.perf_counter() - t
        assert st == 0, outs[0].error_message
        errors = sum(1 for i in range(n) if outs[i].status != 0)
        tot = dict(segments=0, onsets=0, refined=0, variable=0)
        for i in range(n):
            lib.sdsp_result_free(C.byref(outs[i]))
            if tms is not None:
                errors += tms[i].status != 0
                tot["segments"] += int(tms[i].n_segments)
                tot["onsets"] += int(tms[i].n_onsets)
                tot["refined"] += int(tms[i].refined)
                tot["variable"] += int(tms[i].has_variation)
                lib.sdsp_tempo_map_free(C.byref(tms[i]))
        return dt, errors, tot

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
    names = list(legs)
    for r in range(reps):
        for name in names[r % len(names):] + names[:r % len(names)]:
            req = legs[name]
            dt, errors, tot = call(req)
            assert errors == 0
            secs[name].append(dt)
            last[name] = dict(sdsp.tempo_map_times(args.device), stage_beat_ms=sdsp.stage_times(args.device)["beat_ms"], **tot)
    if clock:
        clock.__exit__(None, None, None)
    res = {"tool": "tools/tempo_map_bench.py", "tracks": n, "seconds_per_track": args.seconds, "reps": reps,
           "workload": f"{n} synthetic {args.seconds:.0f}-s 44.1 kHz mono tracks (bench.py's generator, seeds 0 ..), "
                       "full analysis, one process, legs interleaved", "legs": {}}
    for name in legs:
        med = statistics.median(secs[name])
        t = last[name]
        leg = {"seconds": [round(v, 4) for v in secs[name]], "median_seconds": round(med, 4),
               "spread_seconds": round(max(secs[name]) - min(secs[name]), 4), "tracks_per_s": round(n / med, 1),
               "beat_ms_last_call": round(t["stage_beat_ms"], 3)}
        if legs[name] is not None:
            leg["tempo_map_last_call"] = {"tracks": t["tracks"], "k_tempo_map_ms": round(t["map_ms"], 3),
                                          "k_beat_ms": round(t["beat_ms"], 3), "segments": t["segments"],
                                          "onsets": t["onsets"], "variable_tracks": t["variable"], "refined_tracks": t["refined"]}
        res["legs"][name] = leg
    m = {k: res["legs"][k]["median_seconds"] for k in legs}
    res["segments_minus_none_ms"] = round(1e3 * (m["segments"] - m["none"]), 2)
    res["both_minus_none_ms"] = round(1e3 * (m["both"] - m["none"]), 2)
    res["step_cost_both_vs_none"] = round(m["both"] / m["none"] - 1.0, 4)
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
