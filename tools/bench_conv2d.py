#!/usr/bin/env python3
"""Timings of the batched 2D convolution on one GPU: standalone, one process, one
set of buffers, the method of tools/bench_r2d.py.

  python tools/bench_conv2d.py [--reps 7] [--iters 5] [--batch 64] [--image 1000] [--kernel 25]

Every figure is the median over --reps repetitions of an event-timed run of --iters calls, after
one untimed warm-up call; the spread is (max - min) / median over the repetitions.  One shape:
--batch images of --image x --image with kernels of --kernel x --kernel, mode "same", linear
(the default pads to P = 1024 x 1024, w = 513).
  (a) hsfft_convolve_2d_batched with a shared kernel and with one kernel per image;
  (b) the three public transforms such a convolution consists of, alone, on buffers that already
      hold padded images: hsfft_r2c_2d twice and hsfft_c2r_2d once, with (a) / (b).  (b) has
      neither padding nor product nor window, so it is a floor for any composition from the
      public calls, not a convolution.
Every buffer is allocated with the size the call that uses it needs, from the expressions below;
nothing here copies a byte count between buffers of another size.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_2d import Timer, stats  # noqa: E402  (puts the package on sys.path)

import hsfft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--image", type=int, default=1000)
    ap.add_argument("--kernel", type=int, default=25)
    args = ap.parse_args()
    if hsfft.device_count() < 1:
        raise SystemExit("bench_conv2d: no GPU")
    hsfft.check(hsfft.lib().hsfft_set_device(0), "set_device")
    tm = Timer()
    batch, n, m = args.batch, args.image, args.kernel
    orows, ocols, P0, P1 = hsfft.convolve_2d_shape("same", "linear", n, n, m, m)
    w = P1 // 2 + 1
    real_bytes, kern_bytes, out_bytes = batch * n * n * 8, batch * m * m * 8, batch * orows * ocols * 8
    pad_bytes, half_bytes = batch * P0 * P1 * 8, batch * P0 * w * 16
    da, db, out = hsfft.DeviceBuffer(real_bytes), hsfft.DeviceBuffer(kern_bytes), hsfft.DeviceBuffer(out_bytes)
    pa, sa = hsfft.DeviceBuffer(pad_bytes), hsfft.DeviceBuffer(half_bytes)
    hsfft.fill_real(da, real_bytes // 8, 0xC2)
    hsfft.fill_real(db, kern_bytes // 8, 0xD2)
    hsfft.fill_real(pa, pad_bytes // 8, 0xE2)
    hsfft.synchronize()

    def timed(call):
        return stats([tm.ms(call, args.iters) for _ in range(args.reps)])

    res = dict(what="convolve_2d", batch=batch, image=n, kernel=m, pad_rows=P0, pad_cols=P1, out_rows=orows,
               out_cols=ocols, reps=args.reps, iters=args.iters)
    res["call_shared_ms"], res["call_shared_spread"] = timed(
        lambda: hsfft.convolve_2d_batched("same", "linear", da, n, n, db, m, m, 1, out, batch))
    res["call_per_image_ms"], res["call_per_image_spread"] = timed(
        lambda: hsfft.convolve_2d_batched("same", "linear", da, n, n, db, m, m, batch, out, batch))

    p0, q0 = hsfft.Plan(P0, 1), hsfft.Plan(P0, -1)
    r1, t1 = hsfft.RealPlan(P1, 1), hsfft.RealPlan(P1, -1)
    # pa: batch x P0 x P1 reals; sa: batch x P0 x w complex -- the sizes hsfft_r2c_2d / hsfft_c2r_2d read and write
    res["r2c_2d_ms"], res["r2c_2d_spread"] = timed(lambda: hsfft.r2c_2d(p0, r1, pa, sa, batch))
    res["c2r_2d_ms"], res["c2r_2d_spread"] = timed(lambda: hsfft.c2r_2d(q0, t1, sa, pa, batch))
    res["transforms_ms"] = 2 * res["r2c_2d_ms"] + res["c2r_2d_ms"]
    res["call_per_image_over_transforms"] = res["call_per_image_ms"] / res["transforms_ms"]
    res["call_shared_over_transforms"] = res["call_shared_ms"] / res["transforms_ms"]
    res["gsamples_s_shared"] = batch * n * n / res["call_shared_ms"] / 1e6
    print(json.dumps(res), flush=True)
    for p in (p0, q0, r1, t1):
        p.close()
    hsfft.synchronize()
    for d in (da, db, out, pa, sa):
        d.free()
    hsfft.finalize()


if __name__ == "__main__":
    main()
