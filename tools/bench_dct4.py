#!/usr/bin/env python3
"""Timings of the batched type-IV transforms and of the MDCT / IMDCT on one GPU:
standalone, one process, one set of buffers per case, the method of tools/bench_dct.py.

  python tools/bench_dct4.py [--reps 7] [--iters 3]

Cases: 4096 rows of 65536 and 65536 rows of 4096 reals through hsfft_dct4_batched, in the cosine and
in the sine form (the same kernels with other indices); 64 rows of 2^20 through hsfft_mdct_batched
and hsfft_imdct_batched at the hop N = 1024 with a sine window.  Beside each figure stand two yardsticks timed in the same process on the same buffers:
  * the floor: hsfft_exec_batched of the forward plan of length N/2 on as many rows -- the inner
    transform alone, which the composition cannot beat;
  * hsfft_bench_copy: the rate of a plain copy, and the time that rate needs for the bytes the
    kernels around the transform must move.  Per DCT-IV row the input rotation reads and writes
    N x 8 bytes and the output rotation as many, 32 N in all; per MDCT frame the fold adds a read
    and a write of N x 8 (every sample lies in two frames; the second read is counted as cached),
    and per IMDCT frame the overlap-add as much, 48 N in all.  It is compared with the time the call
    spends over its floor.

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


def measure(tm, args, base, variants, floor, rows, words, moved, copy):
    """time every variant and the copy `reps` times in turn; one JSON line for the copy, one for the
    floor and one per variant.  copy: (source, destination, bytes)"""
    samples = {k: [] for k in variants}
    samples["copy"] = []
    for _ in range(args.reps):
        for what, call in variants.items():
            samples[what].append(tm.ms(call, args.iters))
        samples["copy"].append(hsfft.bench_copy(copy[0], copy[1], copy[2], args.iters) / args.iters)
    med = {k: stats(v) for k, v in samples.items()}
    copy_ms, copy_sp = med["copy"]
    gbs = 2 * copy[2] / copy_ms / 1e6
    moved_ms = moved / gbs / 1e6
    print(json.dumps(dict(base, what="copy", bytes=copy[2], ms=copy_ms, spread=copy_sp, gbs=gbs)), flush=True)
    fms, fsp = med[floor]
    print(json.dumps(dict(base, what=floor, rows=rows, ms=fms, spread=fsp)), flush=True)
    for what in variants:
        if what == floor:
            continue
        ms, sp = med[what]
        print(json.dumps(dict(base, what=what, ms=ms, spread=sp, gsamples_s=words / ms / 1e6, floor_ms=fms,
                              over_floor=ms / fms, beyond_floor_ms=ms - fms, moved_bytes=moved, moved_at_copy_rate_ms=moved_ms,
                              copy_rate_fraction=moved_ms / (ms - fms) if ms > fms else None)), flush=True)


def bench_dct4(tm, args, batch, n):
    h, words = n // 2, batch * n
    plan = hsfft.Plan(h, 1)
    dx, dy, dz = (hsfft.DeviceBuffer(words * 8) for _ in range(3))
    hsfft.fill_real(dx, words, 0xD4)
    variants = {
        "dct4": lambda: hsfft.dct4_batched(hsfft.KIND_COS, dx, dy, n, batch),
        "dst4": lambda: hsfft.dct4_batched(hsfft.KIND_SIN, dx, dy, n, batch),
        "exec_batched_half": lambda: hsfft.exec_batched(plan, dx, dz, batch),  # the rows read as n/2 complex
    }
    # the round trip's error, printed and not asserted: either transform twice is 2 n x
    errs = {}
    for what, kind in (("dct4", hsfft.KIND_COS), ("dst4", hsfft.KIND_SIN)):
        hsfft.dct4_batched(kind, dx, dy, n, batch)
        hsfft.dct4_batched(kind, dy, dz, n, batch)
        hsfft.synchronize()
        errs[what] = float(np.abs(dz.to_array(np.float64, count=n) / (2.0 * n) - dx.to_array(np.float64, count=n)).max())
    base = dict(case="dct4", batch=batch, n=n, reps=args.reps, iters=args.iters,
                chunk_mb=float(os.environ.get("HSFFT_DCT_CHUNK_MB", 1024.0)), round_trip_max_error=errs)
    measure(tm, args, base, variants, "exec_batched_half", batch, words, batch * 32 * n, (dx, dz, words * 8))
    hsfft.synchronize()
    for d in (dx, dy, dz):
        d.free()
    plan.close()


def bench_mdct(tm, args, batch, n, N):
    nframes = hsfft.mdct_shape(n, N, False)[0]
    frames, words = batch * nframes, batch * n
    plan = hsfft.Plan(N // 2, 1)
    dx, dback = hsfft.DeviceBuffer(words * 8), hsfft.DeviceBuffer(words * 8)
    dX, dflo = hsfft.DeviceBuffer(frames * N * 8), hsfft.DeviceBuffer(frames * N * 8)
    dw = hsfft.DeviceBuffer.from_array(np.sin(np.pi * (np.arange(2 * N) + 0.5) / (2 * N)))
    hsfft.fill_real(dx, words, 0x3D)
    variants = {
        "mdct": lambda: hsfft.mdct_batched(dx, n, dw, N, False, dX, batch),
        "imdct": lambda: hsfft.imdct_batched(dX, nframes, dw, N, False, dback, n, batch),
        "exec_batched_half": lambda: hsfft.exec_batched(plan, dX, dflo, frames),  # the coefficients read as N/2 complex
    }
    variants["mdct"]()
    variants["imdct"]()
    hsfft.synchronize()
    # perfect reconstruction of the samples two frames cover, printed and not asserted
    x0, b0 = dx.to_array(np.float64, count=n), dback.to_array(np.float64, count=n)
    err = float(np.abs(b0 - x0)[N:n - N].max())
    base = dict(case="mdct", batch=batch, n=n, hop=N, nframes=nframes, reps=args.reps, iters=args.iters,
                chunk_mb=float(os.environ.get("HSFFT_MDCT_CHUNK_MB", 1024.0)), round_trip_max_error=err)
    measure(tm, args, base, variants, "exec_batched_half", frames, words, frames * 48 * N, (dX, dflo, frames * N * 8))
    hsfft.synchronize()
    for d in (dx, dback, dX, dflo, dw):
        d.free()
    plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    if hsfft.device_count() < 1:
        raise SystemExit("bench_dct4: no GPU")
    hsfft.check(hsfft.lib().hsfft_set_device(0), "set_device")
    tm = Timer()
    bench_dct4(tm, args, 4096, 65536)
    bench_dct4(tm, args, 65536, 4096)
    bench_mdct(tm, args, 64, 1 << 20, 1024)
    hsfft.finalize()


if __name__ == "__main__":
    main()
