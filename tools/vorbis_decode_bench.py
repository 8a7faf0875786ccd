#!/usr/bin/env python3
"""Decode throughput of the device Vorbis decode (sdsp_decode_audio_batch_device) against the host
decoder, on the same files.

A short stereo passage is encoded once by tests/vorbis_enc.py as long blocks (2048) with residue
type 2 and square-polar coupling; Vorbis audio packets decode independently, so the packet list
repeated to three minutes is a valid stream.  Every file of the batch is that same file, replicated
--files times (default 256): files decode independently, but the numbers say nothing about how
throughput varies with the bitstream.  Timed in this one process, warm, as the median of --reps
repetitions (default 5, at least 5), the legs interleaved:

  (a) sdsp_decode_audio_file on --threads host threads (default 16), the files in RAM-backed storage;
  (b) sdsp_decode_audio_batch_device, the host plan and the upload of the packets included.

Leg (a) runs this tree's host decoder, which already runs csrc/vorbis_core.hpp.  --host-lib PATH
also times leg (a) once through another build of the library (the decoder before the core was
split out), in a child process.

Writes tracks/s for both, the stats struct of the last device call and the sampled shader clock to
--out (default profiles/vorbis_decode.json) and prints the same JSON line.

  python tools/vorbis_decode_bench.py [--files 256] [--reps 5] [--threads 16] [--minutes 3] [--out PATH]
"""
import argparse
import concurrent.futures
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stratum-dsp_amd", "python"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import synth  # noqa: E402
import vorbis_enc as ve  # noqa: E402
import vorbis_streams as vs  # noqa: E402

BLOCKS = 24  # long blocks in the encoded passage


def make_ogg(minutes):
    left, _, _, _ = synth.make_track(11, seconds=2.0)
    right, _, _, _ = synth.make_track(12, seconds=2.0)
    span = (BLOCKS - 1) * 1024
    x = [0.6 * left[:span], 0.6 * (0.7 * left[:span] + 0.3 * right[:span])]
    pk, _, _ = ve.encode(x, 44100, [1] * BLOCKS, rtype=2)
    repeat = max(1, int(round(minutes * 60 * 44100 / (BLOCKS * 1024))))
    packets = pk * repeat
    granules = [1024 * i for i in range(len(packets))]
    return vs.ogg(ve.headers(2, 44100, 2) + packets, [0, 0, 0] + granules), granules[-1]


def host_leg(lib_path, paths, threads):
    """Seconds for sdsp_decode_audio_file over `paths` on `threads` threads, and the lengths."""
    L = C.CDLL(lib_path)
    L.sdsp_decode_audio_file.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32), C.c_char_p, C.c_uint64]
    L.sdsp_decode_audio_file.restype = C.c_int32
    L.sdsp_free_samples.argtypes = [C.POINTER(C.c_float)]
    L.sdsp_free_samples.restype = None

    def one(path):
        p, n, sr = C.POINTER(C.c_float)(), C.c_uint64(), C.c_uint32()
        err = C.create_string_buffer(512)
        st = L.sdsp_decode_audio_file(os.fsencode(path), C.byref(p), C.byref(n), C.byref(sr), err, 512)
        assert st == 0, err.value
        L.sdsp_free_samples(p)
        return n.value

    pool = concurrent.futures.ThreadPoolExecutor(threads)

    def run():
        t = time.perf_counter()
        out = list(pool.map(one, paths))
        return time.perf_counter() - t, out

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--minutes", type=float, default=3.0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host-lib", default=None, help="another build of libstratum_hip.so whose host decoder is timed once")
    ap.add_argument("--host-only", default=None, help=argparse.SUPPRESS)  # the child of --host-lib: a directory of files
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vorbis_decode.json"))
    args = ap.parse_args()
    if args.host_only:
        paths = sorted(os.path.join(args.host_only, f) for f in os.listdir(args.host_only))
        run = host_leg(args.host_lib, paths, args.threads)
        run()
        print(json.dumps({"seconds": [round(run()[0], 4) for _ in range(2)]}))
        return
    import sdsp

    reps = max(args.reps, 5)
    t0 = time.perf_counter()
    data, n_samples = make_ogg(args.minutes)
    encode_s = time.perf_counter() - t0
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    clock = None
    try:
        import bench

        clock = bench.ClockSampler(args.device)
    except Exception:
        clock = None
    res = {"tool": "tools/vorbis_decode_bench.py", "files": args.files, "reps": reps, "threads": args.threads}
    tmp = tempfile.mkdtemp(prefix="vorbis_bench_", dir=base)
    try:
        first = os.path.join(tmp, "f0000.ogg")
        with open(first, "wb") as f:
            f.write(data)
        paths = [first]
        for i in range(1, args.files):  # the same bytes under --files names
            p = os.path.join(tmp, f"f{i:04d}.ogg")
            os.link(first, p)
            paths.append(p)
        blobs = [data] * args.files
        host_all = host_leg(sdsp.LIB_PATH, paths, args.threads)

        def device_all():
            t = time.perf_counter()
            buf, offs, lens, rates, errors, stats = sdsp.decode_audio_batch_device(blobs, device=args.device)
            return time.perf_counter() - t, buf, lens, errors, stats

        if clock:
            clock.__enter__()
        host_all()  # warm
        _, buf, lens, errors, stats = device_all()  # warm: the grow-only buffers reach their size
        assert all(e is None for e in errors), errors[0]
        assert stats["vorbis_files"] == args.files and stats["host_fallback_files"] == 0, stats
        assert all(int(v) == n_samples for v in lens)
        head = buf.to_host(0, 65536)
        buf.free()
        want, _ = sdsp.decode_audio_file(paths[0])
        assert np.array_equal(head.view(np.uint32), want[:65536].view(np.uint32))
        host_s, dev_s = [], []
        for _ in range(reps):  # interleaved: both legs see the same machine state
            dt, out = host_all()
            assert all(n == n_samples for n in out)
            host_s.append(dt)
            dt, buf, lens, errors, stats = device_all()
            buf.free()
            dev_s.append(dt)
        if clock:
            clock.__exit__(None, None, None)
        other = None
        if args.host_lib:
            out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--host-only", tmp, "--host-lib",
                                           args.host_lib, "--threads", str(args.threads)])
            other = json.loads(out.decode().strip().splitlines()[-1])["seconds"]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    hm, dm = statistics.median(host_s), statistics.median(dev_s)
    res.update({
        "workload": f"{args.files} copies of one file: {n_samples / 44100.0:.1f} s of 44.1 kHz stereo Ogg Vorbis, long blocks "
                    f"(2048), residue type 2, coupled, {len(data)} bytes",
        "samples_per_file": n_samples, "bytes_per_file": len(data), "encode_seconds": round(encode_s, 2),
        "host": {"what": f"sdsp_decode_audio_file (this tree: vorbis_core.hpp) on {args.threads} threads, files in "
                         f"{base or 'the temporary directory'}",
                 "seconds": [round(v, 4) for v in host_s], "median_seconds": round(hm, 4), "tracks_per_s": round(args.files / hm, 2)},
        "device": {"what": "sdsp_decode_audio_batch_device, host plan and upload included",
                   "seconds": [round(v, 4) for v in dev_s], "median_seconds": round(dm, 4),
                   "tracks_per_s": round(args.files / dm, 2), "stats_last_call": stats},
        "speedup": round(hm / dm, 3),
        "host_other_build_seconds": other,
        "sclk_mhz": clock.report() if clock else None,
    })
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
