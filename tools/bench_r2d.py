#!/usr/bin/env python3
"""Timings of the 2D real transforms on one GPU: standalone, one process, one pair
of buffers, the method of tools/bench_2d.py.

  python tools/bench_r2d.py [--reps 7] [--iters 5]

Every figure is the median over --reps repetitions of an event-timed run of --iters calls, after
one untimed warm-up call; the spread is (max - min) / median over the repetitions.  Per shape
n0 x n1 x batch, with w = n1/2 + 1 and the half spectrum n0 x w:
  (a) hsfft_bench_copy of the half spectrum's bytes;
  (b) hsfft_r2c_batched_compact over the batch x n0 rows alone;
  (c) the c2c of p0 over the batch x w columns as contiguous rows alone (hsfft_time_batched);
  (d) hsfft_r2c_2d, with (d) / ((b) + (c) + 2 x (a)): the floor of its four trips;
  (e) hsfft_r2c_2d_full;
  (f) hsfft_c2r_2d;
  (g) hsfft_exec_2d on the same images widened to complex, and (d) / (g);
  (h) the mirrored transpose alone (hsfft_bench_transpose_herm) against a copy that moves the
      same number of bytes (it reads w x n0 and writes n0 x n1 elements per image).
Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_2d import Timer, stats  # noqa: E402  (puts the package on sys.path)

import hsfft  # noqa: E402

SHAPES = [(4096, 4096, 16), (1024, 1024, 256), (512, 32768, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    if hsfft.device_count() < 1:
        raise SystemExit("bench_r2d: no GPU")
    hsfft.check(hsfft.lib().hsfft_set_device(0), "set_device")
    tm = Timer()
    count = max(n0 * n1 * batch for n0, n1, batch in SHAPES)  # complex elements of the largest full spectrum
    a, b = hsfft.DeviceBuffer(count * 16), hsfft.DeviceBuffer(count * 16)

    def timed(call):
        return stats([tm.ms(call, args.iters) for _ in range(args.reps)])

    def copy(nbytes):
        nbytes -= nbytes % 16
        return stats([hsfft.bench_copy(a, b, nbytes, args.iters) / args.iters for _ in range(args.reps)])

    for n0, n1, batch in SHAPES:
        w = n1 // 2 + 1
        half_bytes, full_bytes = n0 * w * batch * 16, n0 * n1 * batch * 16
        p0, p1, r1 = hsfft.Plan(n0, 1), hsfft.Plan(n1, 1), hsfft.RealPlan(n1, 1)
        q0, s1 = hsfft.Plan(n0, -1), hsfft.RealPlan(n1, -1)
        hsfft.fill_complex(a, count, 0x2D)
        hsfft.synchronize()
        res = dict(what="r2c_2d", n0=n0, n1=n1, batch=batch, half_bytes=half_bytes)
        res["a_copy_ms"], res["a_spread"] = copy(half_bytes)
        res["b_r2c_rows_ms"], res["b_spread"] = timed(lambda: hsfft.r2c_batched_compact(r1, a, b, batch * n0))
        hsfft.time_batched(p0, a, b, batch * w, 1)  # warm-up
        res["c_col_rows_ms"], res["c_spread"] = stats([hsfft.time_batched(p0, a, b, batch * w, args.iters)[0] / args.iters
                                                       for _ in range(args.reps)])
        res["h_herm_ms"], res["h_spread"] = stats([hsfft.bench_transpose_herm(a, b, n0, n1, batch, args.iters) / args.iters
                                                   for _ in range(args.reps)])
        res["h_copy_ms"], res["h_copy_spread"] = copy((half_bytes + full_bytes) // 2)
        res["h_fraction_of_copy"] = res["h_copy_ms"] / res["h_herm_ms"]
        res["e_r2c_2d_full_ms"], res["e_spread"] = timed(lambda: hsfft.r2c_2d_full(p0, r1, a, b, batch))
        res["d_r2c_2d_ms"], res["d_spread"] = timed(lambda: hsfft.r2c_2d(p0, r1, a, b, batch))
        # b now holds the half spectra of a: the input of c2r_2d, whose output overwrites a
        res["f_c2r_2d_ms"], res["f_spread"] = timed(lambda: hsfft.c2r_2d(q0, s1, b, a, batch))
        hsfft.fill_complex(a, count, 0x2D)
        res["g_exec_2d_ms"], res["g_spread"] = timed(lambda: hsfft.exec_2d(p0, p1, a, b, batch))
        res["floor_ms"] = res["b_r2c_rows_ms"] + res["c_col_rows_ms"] + 2 * res["a_copy_ms"]
        res["d_over_floor"] = res["d_r2c_2d_ms"] / res["floor_ms"]
        res["d_over_g"] = res["d_r2c_2d_ms"] / res["g_exec_2d_ms"]
        res["gsamples_s"] = n0 * n1 * batch / res["d_r2c_2d_ms"] / 1e6
        print(json.dumps(res), flush=True)
        for p in (p0, p1, r1, q0, s1):
            p.close()
    hsfft.synchronize()
    a.free()
    b.free()
    hsfft.finalize()


if __name__ == "__main__":
    main()
