#!/usr/bin/env python3
"""Timings of the batched 2D cosine transforms and of the transpose of 8-byte elements on one GPU
(DESIGN.md §14): standalone, one process, one set of buffers, the method of tools/bench_dct.py.

  python tools/bench_dct2d.py [--reps 7] [--iters 3] [--shapes 1024x1024x512,512x2048x512] [--sine]

For every shape n0 x n1 x batch (real images; the defaults hold 4 GiB per buffer):
  * hsfft_dct_2d_batched as type 2 and as type 3 (DST with --sine: the same kernels);
  * floor 1, the two hsfft_dct_batched calls on the same bytes: batch x n0 rows of n1, then
    batch x n1 rows of n0;
  * floor 2, the two transposes of the call alone -- hsfft_transpose_real_batched of n0 x n1 and of
    n1 x n0 -- beside two hsfft_bench_copy of the same bytes, and beside the 16-byte
    hsfft_transpose_batched of the same bytes (n0 x n1/2 and n1/2 x n0 elements), the rate
    DESIGN.md §8 reports.
  The call's yardstick is floor 1 + floor 2: what the driver costs over its four parts.

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


def run_shape(tm, args, n0, n1, batch, bufs):
    dx, dy, dz = bufs
    kind = hsfft.KIND_SIN if args.sine else hsfft.KIND_COS
    words = n0 * n1 * batch
    nbytes = words * 8

    def rows(type, src, mid, dst):
        hsfft.dct_batched(kind, type, src, mid, n1, batch * n0)
        hsfft.dct_batched(kind, type, mid, dst, n0, batch * n1)

    def transposes8():
        hsfft.transpose_real_batched(dx, dz, n0, n1, batch)
        hsfft.transpose_real_batched(dz, dx, n1, n0, batch)  # dx holds its own words again

    def transposes16():
        hsfft.transpose_batched(dx, dz, n0, n1 // 2, batch)
        hsfft.transpose_batched(dz, dx, n1 // 2, n0, batch)

    variants = {
        "dct2d_type2": lambda: hsfft.dct_2d_batched(kind, kind, 2, dx, dy, n0, n1, batch),
        "dct2d_type3": lambda: hsfft.dct_2d_batched(kind, kind, 3, dy, dz, n0, n1, batch),
        "rows_type2": lambda: rows(2, dx, dy, dz),
        "rows_type3": lambda: rows(3, dx, dy, dz),
        "transposes8": transposes8,
        "transposes16": transposes16,
    }
    # the round trip's error, printed and not asserted: type 3 of type 2 of x is 4 n0 n1 x
    hsfft.fill_real(dx, words, 0xDC2)
    variants["dct2d_type2"]()
    variants["dct2d_type3"]()
    hsfft.synchronize()
    x0, z0 = dx.to_array(np.float64, count=n0 * n1), dz.to_array(np.float64, count=n0 * n1)
    round_trip = float(np.abs(z0 / (4.0 * n0 * n1) - x0).max())

    order = ("dct2d_type2", "dct2d_type3", "rows_type2", "rows_type3", "transposes8", "transposes16")
    samples = {k: [] for k in order}
    samples["copies"] = []
    for _ in range(args.reps):
        for what in order:
            samples[what].append(tm.ms(variants[what], args.iters))
        samples["copies"].append(hsfft.bench_copy(dx, dz, nbytes, 2 * args.iters) / args.iters)  # two copies per sample
    med = {k: stats(v) for k, v in samples.items()}
    base = dict(n0=n0, n1=n1, batch=batch, bytes=nbytes, kind="sine" if args.sine else "cosine", reps=args.reps,
                iters=args.iters, chunk_mb=float(os.environ.get("HSFFT_2D_CHUNK_MB", 1024.0)))
    rate = lambda ms: 2 * 2 * nbytes / ms / 1e6  # two passes, each reads and writes nbytes: GB/s
    cms, csp = med["copies"]
    print(json.dumps(dict(base, what="two copies", ms=cms, spread=csp, gbs=rate(cms))), flush=True)
    for what in ("transposes16", "transposes8"):
        ms, sp = med[what]
        print(json.dumps(dict(base, what="two " + what, ms=ms, spread=sp, gbs=rate(ms), copy_rate_fraction=cms / ms)),
              flush=True)
    tms = med["transposes8"][0]
    for type in (2, 3):
        rms, rsp = med["rows_type%d" % type]
        ms, sp = med["dct2d_type%d" % type]
        print(json.dumps(dict(base, what="rows_type%d" % type, ms=rms, spread=rsp)), flush=True)
        print(json.dumps(dict(base, what="dct2d_type%d" % type, ms=ms, spread=sp, gsamples_s=words / ms / 1e6,
                              rows_ms=rms, transposes_ms=tms, floor_ms=rms + tms, over_floor=ms / (rms + tms),
                              round_trip_max_error=round_trip)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--shapes", default="1024x1024x512,512x2048x512")
    ap.add_argument("--sine", action="store_true")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    for n0, n1, batch in shapes:
        if n0 < 2 or n0 % 2 or n1 < 2 or n1 % 2 or batch < 1:
            raise SystemExit("bench_dct2d: a shape is n0 x n1 x batch with n0 and n1 even")
    if hsfft.device_count() < 1:
        raise SystemExit("bench_dct2d: no GPU")
    hsfft.check(hsfft.lib().hsfft_set_device(0), "set_device")
    tm = Timer()
    most = max(n0 * n1 * batch for n0, n1, batch in shapes)
    bufs = [hsfft.DeviceBuffer(most * 8) for _ in range(3)]
    for n0, n1, batch in shapes:
        run_shape(tm, args, n0, n1, batch, bufs)
    hsfft.synchronize()
    for d in bufs:
        d.free()
    hsfft.finalize()


if __name__ == "__main__":
    main()
