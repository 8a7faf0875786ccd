#!/usr/bin/env python3
"""Decode throughput of the device FLAC decoder against the host decoder, on the same files.

One 20-s stereo 16-bit passage is encoded with tests/flac_enc.py (mid/side, LPC order 8, Rice
partition order 4, block size 4096), its frame sequence is repeated to three minutes (neither
decoder reads the frame number) and the file is replicated --files times (default 256).  Timed in
this one process, warm, as the median of --reps repetitions (default 5, at least 5):

  (a) sdsp_decode_audio_file on --threads host threads (default 16), the files in RAM-backed storage;
  (b) sdsp_decode_flac_batch_device, the upload of the compressed bytes included.

Writes tracks/s for both, the stats struct of the last device call and the sampled shader clock to
--out (default profiles/flac_decode.json) and prints the same JSON line.

  python tools/flac_decode_bench.py [--files 256] [--reps 5] [--threads 16] [--seconds 20] [--out PATH]
  rocprofv3 --kernel-trace --stats -- python tools/flac_decode_bench.py --device-only   # per-kernel times
"""
import argparse
import concurrent.futures
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stratum-dsp_amd", "python"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import flac_enc as fe  # noqa: E402
import sdsp  # noqa: E402
import synth  # noqa: E402


def lpc_coefs(s, order, prec, shift):
    """Least-squares predictor of s from its `order` predecessors, quantised to prec bits at 2^-shift."""
    x = np.asarray(s, np.float64)
    a = np.stack([x[order - 1 - j:len(x) - 1 - j] for j in range(order)], axis=1)
    c, *_ = np.linalg.lstsq(a, x[order:], rcond=None)
    lim = (1 << (prec - 1)) - 1
    return [int(v) for v in np.clip(np.round(c * (1 << shift)), -lim - 1, lim)]


def passage(seconds, reps):
    left, _, _, _ = synth.make_track(11, seconds=seconds)
    right, _, _, _ = synth.make_track(12, seconds=seconds)
    a = np.clip(np.round(0.6 * left * 32767.0), -32768, 32767).astype(np.int64)
    b = np.clip(np.round(0.6 * (0.7 * left + 0.3 * right) * 32767.0), -32768, 32767).astype(np.int64)
    n = (min(a.size, b.size) // 4096) * 4096
    a, b = a[:n], b[:n]
    prec, shift = 12, 9
    specs = [{"type": "lpc", "coefs": lpc_coefs((a + b) >> 1, 8, prec, shift), "prec": prec, "shift": shift, "porder": 4},
             {"type": "lpc", "coefs": lpc_coefs(a - b, 8, prec, shift), "prec": prec, "shift": shift, "porder": 4}]
    frames = [fe.frame([a[o:o + 4096], b[o:o + 4096]], 16, k, assign="mid_side", specs=specs)
              for k, o in enumerate(range(0, n, 4096))]
    return fe.stream(frames * reps, 44100, 2, 16, total=n * reps), n * reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=20.0, help="length of the encoded passage")
    ap.add_argument("--repeat", type=int, default=9, help="repetitions of the passage's frames per file")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--device-only", action="store_true", help="skip the host leg (profiler runs); writes no file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flac_decode.json"))
    args = ap.parse_args()
    reps = max(args.reps, 5)

    t0 = time.perf_counter()
    data, n_samples = passage(args.seconds, args.repeat)
    encode_s = time.perf_counter() - t0
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="flac_bench_", dir=base)
    try:
        first = os.path.join(tmp, "f0000.flac")
        with open(first, "wb") as f:
            f.write(data)
        paths = [first]
        for i in range(1, args.files):  # the same bytes under --files names
            p = os.path.join(tmp, f"f{i:04d}.flac")
            os.link(first, p)
            paths.append(p)

        L = sdsp.lib()

        def host_one(path):
            p, n, sr = C.POINTER(C.c_float)(), C.c_uint64(), C.c_uint32()
            err = C.create_string_buffer(512)
            st = L.sdsp_decode_audio_file(os.fsencode(path), C.byref(p), C.byref(n), C.byref(sr), err, 512)
            assert st == 0, err.value
            first4 = [p[i] for i in range(4)]
            L.sdsp_free_samples(p)
            return n.value, first4

        def host_all(pool):
            t = time.perf_counter()
            out = list(pool.map(host_one, paths))
            return time.perf_counter() - t, out

        def device_all():
            t = time.perf_counter()
            buf, offs, lens, rates, errors, stats = sdsp.decode_flac_batch_device(blobs, device=args.device)
            dt = time.perf_counter() - t
            return dt, buf, lens, errors, stats

        blobs = [data] * args.files
        clock = None
        try:
            import bench

            clock = bench.ClockSampler(args.device)
        except Exception:
            clock = None
        with concurrent.futures.ThreadPoolExecutor(args.threads) as pool:
            if not args.device_only:
                host_all(pool)  # warm
            _, buf, lens, errors, stats = device_all()  # warm: the grow-only buffers reach their size
            assert all(e is None for e in errors) and stats["device_files"] == args.files, stats
            assert all(int(v) == n_samples for v in lens)
            head = buf.to_host(0, 4096)
            buf.free()
            want, _ = sdsp.decode_audio_file(paths[0])
            assert np.array_equal(head.view(np.uint32), want[:4096].view(np.uint32))
            host_s, dev_s = [], []
            if clock:
                clock.__enter__()
            for _ in range(reps):  # interleaved: both legs see the same machine state
                if not args.device_only:
                    dt, out = host_all(pool)
                    assert all(n == n_samples for n, _ in out)
                    host_s.append(dt)
                dt, buf, lens, errors, stats = device_all()
                buf.free()
                dev_s.append(dt)
            if clock:
                clock.__exit__(None, None, None)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    if args.device_only:
        print(json.dumps({"device_seconds": dev_s, "tracks_per_s": round(args.files / statistics.median(dev_s), 2),
                          "stats_last_call": stats}))
        return
    hm, dm = statistics.median(host_s), statistics.median(dev_s)
    res = {
        "tool": "tools/flac_decode_bench.py",
        "workload": f"{args.files} files, each {n_samples / 44100.0:.1f} s of 44.1 kHz 16-bit stereo FLAC (mid/side, LPC order 8, "
                    f"Rice partition order 4, block size 4096), {len(data)} bytes",
        "files": args.files, "samples_per_file": n_samples, "bytes_per_file": len(data), "reps": reps,
        "encode_seconds": round(encode_s, 2),
        "host": {"what": f"sdsp_decode_audio_file on {args.threads} threads, files in {base or 'the temporary directory'}",
                 "seconds": [round(v, 4) for v in host_s], "median_seconds": round(hm, 4),
                 "tracks_per_s": round(args.files / hm, 2)},
        "device": {"what": "sdsp_decode_flac_batch_device, upload of the compressed bytes included",
                   "seconds": [round(v, 4) for v in dev_s], "median_seconds": round(dm, 4),
                   "tracks_per_s": round(args.files / dm, 2), "stats_last_call": stats},
        "speedup": round(hm / dm, 3),
        "sclk_mhz": clock.report() if clock else None,
    }
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
