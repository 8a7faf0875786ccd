#!/usr/bin/env python3
"""Decode throughput of the batched lossless device decode (sdsp_decode_batch_device) against the
host decoder, on the same files, for ALAC and linear PCM.

One 20-s stereo passage is encoded once per format and repeated to three minutes:

  m4a   16-bit stereo ALAC in ISO MP4 (tests/alac_enc.py: frame length 4096, mix (2, 1), 4-tap
        adaptive predictors); ALAC packets are independent, so repeating the packet list is a
        valid stream;
  wav   24-bit stereo RIFF/WAVE.

Each file is replicated --files times (default 256).  Per format, timed in this one process, warm,
as the median of --reps repetitions (default 5, at least 5), the legs interleaved:

  (a) sdsp_decode_audio_file on --threads host threads (default 16), the files in RAM-backed storage;
  (b) sdsp_decode_batch_device, the upload of the files' bytes included.

Writes tracks/s for both, the stats struct of the last device call and the sampled shader clock to
--out (default profiles/lossless_decode.json) and prints the same JSON line.

  python tools/decode_bench.py [--files 256] [--reps 5] [--threads 16] [--seconds 20] [--formats m4a,wav] [--out PATH]
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

import alac_enc as ae  # noqa: E402
import alac_streams as als  # noqa: E402
import pcm_streams as ps  # noqa: E402
import sdsp  # noqa: E402
import synth  # noqa: E402


def passage(seconds):
    left, _, _, _ = synth.make_track(11, seconds=seconds)
    right, _, _, _ = synth.make_track(12, seconds=seconds)
    a = 0.6 * left
    b = 0.6 * (0.7 * left + 0.3 * right)
    n = (min(a.size, b.size) // 4096) * 4096
    return a[:n], b[:n]


def make_m4a(a, b, repeat):
    l = np.clip(np.round(a * 32767.0), -32768, 32767).astype(np.int64)
    r = np.clip(np.round(b * 32767.0), -32768, 32767).astype(np.int64)
    cfg = ae.Config(bit_depth=16, channels=2, frame_length=4096, sample_rate=44100)
    pk = als.packets(cfg, [l, r], [{"mix": (2, 1), "ch": [als.TAPS4, als.TAPS4]}]) * repeat
    return ae.mp4(cfg, pk, [1] * len(pk)), l.size * repeat


def make_wav(a, b, repeat):
    l = np.clip(np.round(a * 8388607.0), -8388608, 8388607).astype(np.int64)
    r = np.clip(np.round(b * 8388607.0), -8388608, 8388607).astype(np.int64)
    inter = np.stack([l, r], axis=1).reshape(-1)
    return ps.wav(1, 24, 2, ps.pack("s24", inter, False) * repeat, rate=44100), l.size * repeat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=20.0, help="length of the encoded passage")
    ap.add_argument("--repeat", type=int, default=9, help="repetitions of the passage per file")
    ap.add_argument("--formats", default="m4a,wav")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lossless_decode.json"))
    args = ap.parse_args()
    reps = max(args.reps, 5)
    a, b = passage(args.seconds)
    L = sdsp.lib()
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    clock = None
    try:
        import bench

        clock = bench.ClockSampler(args.device)
    except Exception:
        clock = None

    def host_one(path):
        p, n, sr = C.POINTER(C.c_float)(), C.c_uint64(), C.c_uint32()
        err = C.create_string_buffer(512)
        st = L.sdsp_decode_audio_file(os.fsencode(path), C.byref(p), C.byref(n), C.byref(sr), err, 512)
        assert st == 0, err.value
        L.sdsp_free_samples(p)
        return n.value

    res = {"tool": "tools/decode_bench.py", "files": args.files, "reps": reps, "threads": args.threads, "formats": {}}
    if clock:
        clock.__enter__()
    for fmt in args.formats.split(","):
        t0 = time.perf_counter()
        data, n_samples = (make_m4a if fmt == "m4a" else make_wav)(a, b, args.repeat)
        encode_s = time.perf_counter() - t0
        tmp = tempfile.mkdtemp(prefix="decode_bench_", dir=base)
        try:
            first = os.path.join(tmp, "f0000." + fmt)
            with open(first, "wb") as f:
                f.write(data)
            paths = [first]
            for i in range(1, args.files):  # the same bytes under --files names
                p = os.path.join(tmp, f"f{i:04d}.{fmt}")
                os.link(first, p)
                paths.append(p)
            blobs = [data] * args.files

            def device_all():
                t = time.perf_counter()
                buf, offs, lens, rates, errors, stats = sdsp.decode_batch_device(blobs, device=args.device)
                return time.perf_counter() - t, buf, lens, errors, stats

            with concurrent.futures.ThreadPoolExecutor(args.threads) as pool:
                def host_all():
                    t = time.perf_counter()
                    out = list(pool.map(host_one, paths))
                    return time.perf_counter() - t, out

                host_all()  # warm
                _, buf, lens, errors, stats = device_all()  # warm: the grow-only buffers reach their size
                assert all(e is None for e in errors) and stats["device_files"] == args.files, stats
                assert stats["host_fallback_files"] == 0 and all(int(v) == n_samples for v in lens)
                head = buf.to_host(0, 8192)
                buf.free()
                want, _ = sdsp.decode_audio_file(paths[0])
                assert np.array_equal(head.view(np.uint32), want[:8192].view(np.uint32))
                host_s, dev_s = [], []
                for _ in range(reps):  # interleaved: both legs see the same machine state
                    dt, out = host_all()
                    assert all(n == n_samples for n in out)
                    host_s.append(dt)
                    dt, buf, lens, errors, stats = device_all()
                    buf.free()
                    dev_s.append(dt)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        hm, dm = statistics.median(host_s), statistics.median(dev_s)
        res["formats"][fmt] = {
            "workload": f"{args.files} files, each {n_samples / 44100.0:.1f} s of 44.1 kHz stereo "
                        + ("16-bit ALAC in ISO MP4 (frame length 4096)" if fmt == "m4a" else "24-bit PCM in RIFF/WAVE")
                        + f", {len(data)} bytes",
            "samples_per_file": n_samples, "bytes_per_file": len(data), "encode_seconds": round(encode_s, 2),
            "host": {"what": f"sdsp_decode_audio_file on {args.threads} threads, files in {base or 'the temporary directory'}",
                     "seconds": [round(v, 4) for v in host_s], "median_seconds": round(hm, 4),
                     "tracks_per_s": round(args.files / hm, 2)},
            "device": {"what": "sdsp_decode_batch_device, upload of the files' bytes included",
                       "seconds": [round(v, 4) for v in dev_s], "median_seconds": round(dm, 4),
                       "tracks_per_s": round(args.files / dm, 2), "stats_last_call": stats},
            "speedup": round(hm / dm, 3),
        }
    if clock:
        clock.__exit__(None, None, None)
    res["sclk_mhz"] = clock.report() if clock else None
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
