#!/usr/bin/env python3
"""What a fingerprint request costs an analysis call, on the benchmark's own workload.

bench.py's batch (1,024 synthetic three-minute 44.1 kHz tracks, seeds 0 .., AnalysisConfig::default())
is generated once in HBM and analysed in this one process, warm, --reps times (default 7, at least 5)
in each of two legs that alternate (the order flips from one repetition to the next):

  none          sdsp_analyze_batch_device_with with set = NULL (sdsp_analyze_batch_device_ex itself)
  fingerprint   Cs = 5512, max_offset_words = 16, min_overlap_words = 32, max_ber = 0.30, words and match

A leg's time is the wall time of the C entry.  Reported: every repetition, each leg's median and
spread (max - min), fingerprint - none, and of the fingerprint leg's last call the HIP event times of
the three kernels (sdsp_debug_last_fingerprint_times: k_fp_cells and k_fp_words on the vote stream,
summed over the sub-batches, k_fp_match on the main stream after the last join) with the words, the
tracks compared, the pairs and the matches.  A "bench_py" member already in --out (bench.py on the
parent commit's build and on this one, alternating, recorded beside this tool's result) is kept.
Written to --out (default profiles/fingerprint.json) and printed as one JSON line.

  python tools/fingerprint_bench.py [--tracks 1024] [--seconds 180] [--reps 7] [--out PATH]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fingerprint.json"))
    args = ap.parse_args()
    import sdsp
    from sdsp_abi import SdspFingerprint, SdspFingerprintMatches, SdspRequestSetExt3, SdspResult

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
    legs = {"none": None, "fingerprint": sdsp.fingerprint_request(cell_samples=5512, max_offset_words=16,
                                                                  min_overlap_words=32, max_ber=0.30)}

    def call(req):
        outs = (SdspResult * n)()
        fps = (SdspFingerprint * n)() if req is not None else None
        fpm = SdspFingerprintMatches()
        ext = SdspRequestSetExt3()
        rs = ext.base.base.base
        rs.struct_size = C.sizeof(ext)
        if req is not None:
            ext.fp_req = C.pointer(req)
            ext.fingerprints = fps
            ext.fp_matches = C.pointer(fpm)
        t = time.perf_counter()
        st = lib.sdsp_analyze_batch_device_with(C.c_void_p(buf.ptr), offs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), n,
                                                sr, C.byref(cfg), args.device, None, 0, outs, C.byref(rs) if req is not None else None)
        dt = time.perf_counter() - t
        assert st == 0, outs[0].error_message
        errors = sum(1 for i in range(n) if outs[i].status != 0)
        tot = dict(matches=int(fpm.n_matches))
        for i in range(n):
            lib.sdsp_result_free(C.byref(outs[i]))
            if fps is not None:
                errors += fps[i].status != 0
                lib.sdsp_fingerprint_free(C.byref(fps[i]))
        if req is not None:
            lib.sdsp_fingerprint_matches_free(C.byref(fpm))
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
        for name in (names if r % 2 == 0 else names[::-1]):
            dt, errors, tot = call(legs[name])
            assert errors == 0
            secs[name].append(dt)
            last[name] = dict(sdsp.fingerprint_times(args.device), **tot)
    if clock:
        clock.__exit__(None, None, None)
    res = {"tool": "tools/fingerprint_bench.py", "tracks": n, "seconds_per_track": args.seconds, "reps": reps,
           "request": "Cs 5512, max_offset_words 16, min_overlap_words 32, max_ber 0.30, words and match",
           "workload": f"{n} synthetic {args.seconds:.0f}-s 44.1 kHz mono tracks (bench.py's generator, seeds 0 ..), "
                       "full analysis, one process, legs alternating", "legs": {}}
    for name in legs:
        med = statistics.median(secs[name])
        leg = {"seconds": [round(v, 4) for v in secs[name]], "median_seconds": round(med, 4),
               "spread_seconds": round(max(secs[name]) - min(secs[name]), 4), "tracks_per_s": round(n / med, 1)}
        if legs[name] is not None:
            t = last[name]
            leg["fingerprint_last_call"] = {"words": t["words"], "compared": t["compared"], "pairs": t["pairs"],
                                            "matches": t["matches"], "k_fp_cells_ms": round(t["cells_ms"], 3),
                                            "k_fp_words_ms": round(t["words_ms"], 3), "k_fp_match_ms": round(t["match_ms"], 3)}
        res["legs"][name] = leg
    m = {k: res["legs"][k]["median_seconds"] for k in legs}
    res["fingerprint_minus_none_ms"] = round(1e3 * (m["fingerprint"] - m["none"]), 2)
    res["step_cost_fingerprint_vs_none"] = round(m["fingerprint"] / m["none"] - 1.0, 4)
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
