#!/usr/bin/env python3
"""Timings of the batched cosine transforms on one GPU: standalone, one process, one
set of buffers, the method of tools/bench_stft.py.

  python tools/bench_dct.py [--reps 7] [--iters 3] [--batch 4096] [--n 65536] [--sine]

--batch rows of --n reals: hsfft_dct_batched as DCT-II and as DCT-III (DST-II / DST-III with
--sine: the same kernels with other indices).  Beside each figure stand two yardsticks timed in the
same process:
  * the row transform alone on the same rows -- hsfft_r2c_batched_compact, respectively
    hsfft_c2r_batched -- the floor the composition cannot beat;
  * hsfft_bench_copy of the bytes the two kernels around the transform must move: per row the
    permutation reads and writes N x 8 bytes and the rotation reads (N/2+1) x 16 and writes N x 8,
    about 32 N in all, and a copy of half that many bytes reads and writes as much.  It is compared
    with the time the call spends over its floor.

Every figure is the median over --reps repetitions of an event-timed run of --iters calls after
one untimed warm-up call; the spread is (max - min) / median.  A repetition times every variant
once, so the variants alternate and share whatever else the machine is doing.  Prints one JSON
line per measurement.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_2d import Timer, stats  # noqa: E402  (puts the package on sys.path)

import hsfft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--sine", action="store_true")
    args = ap.parse_args()
    if hsfft.device_count() < 1:
        raise SystemExit("bench_dct: no GPU")
    hsfft.check(hsfft.lib().hsfft_set_device(0), "set_device")
    tm = Timer()
    batch, n, kind = args.batch, args.n, hsfft.KIND_SIN if args.sine else hsfft.KIND_COS
    bins, words = n // 2 + 1, batch * n
    chunk_mb = float(os.environ.get("HSFFT_DCT_CHUNK_MB", 1024.0))
    rf, ri = hsfft.RealPlan(n, 1), hsfft.RealPlan(n, -1)
    dx, dy, dz = (hsfft.DeviceBuffer(words * 8) for _ in range(3))
    hsfft.fill_real(dx, words, 0xDC)
    spec = hsfft.DeviceBuffer(batch * bins * 16)    # the r2c floor's output
    wide = hsfft.DeviceBuffer(batch * (n + 1) * 16) # spectra at the pitch n hsfft_c2r_batched reads; the copy's source
    dest = hsfft.DeviceBuffer(batch * (n + 1) * 16) # the copy's destination
    hsfft.fill_complex(wide, words, 0xDD)
    moved = batch * (n * 8 + n * 8 + bins * 16 + n * 8)
    copy_bytes = moved // 2 // 16 * 16
    assert copy_bytes <= batch * (n + 1) * 16

    variants = {
        "dct2": lambda: hsfft.dct_batched(kind, 2, dx, dy, n, batch),
        "r2c_batched_compact": lambda: hsfft.r2c_batched_compact(rf, dx, spec, batch),
        "dct3": lambda: hsfft.dct_batched(kind, 3, dy, dz, n, batch),
        "c2r_batched": lambda: hsfft.c2r_batched(ri, wide, dz, batch),
    }
    # the round trip's error, printed and not asserted: type 3 of type 2 of x is 2 n x
    variants["dct2"]()
    variants["dct3"]()
    hsfft.synchronize()
    x0, z0 = dx.to_array(np.float64, count=n), dz.to_array(np.float64, count=n)
    round_trip = float(np.abs(z0 / (2.0 * n) - x0).max())

    samples = {k: [] for k in variants}
    samples["copy"] = []
    for _ in range(args.reps):
        for what in ("dct2", "dct3", "r2c_batched_compact", "c2r_batched"):
            samples[what].append(tm.ms(variants[what], args.iters))
        samples["copy"].append(hsfft.bench_copy(wide, dest, copy_bytes, args.iters) / args.iters)
    med = {k: stats(v) for k, v in samples.items()}
    base = dict(batch=batch, n=n, kind="sine" if args.sine else "cosine", reps=args.reps, iters=args.iters, chunk_mb=chunk_mb)
    copy_ms, copy_sp = med["copy"]
    print(json.dumps(dict(base, what="copy", bytes=copy_bytes, ms=copy_ms, spread=copy_sp, gbs=2 * copy_bytes / copy_ms / 1e6)),
          flush=True)
    for what, floor in (("dct2", "r2c_batched_compact"), ("dct3", "c2r_batched")):
        ms, sp = med[what]
        fms, fsp = med[floor]
        print(json.dumps(dict(base, what=floor, ms=fms, spread=fsp)), flush=True)
        print(json.dumps(dict(base, what=what, ms=ms, spread=sp, gsamples_s=words / ms / 1e6, floor_ms=fms,
                              over_floor=ms / fms, beyond_floor_ms=ms - fms, moved_bytes=moved, copy_ms=copy_ms,
                              copy_rate_fraction=copy_ms / (ms - fms) if ms > fms else None,
                              round_trip_max_error=round_trip)), flush=True)
    hsfft.synchronize()
    for d in (dx, dy, dz, spec, wide, dest):
        d.free()
    rf.close()
    ri.close()
    hsfft.finalize()


if __name__ == "__main__":
    main()
