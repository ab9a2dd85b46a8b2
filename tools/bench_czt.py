#!/usr/bin/env python3
"""Timings of the batched chirp-z transform on one GPU: standalone, one process,
one set of buffers per case, the method of tools/bench_dct4.py.

  python tools/bench_czt.py [--reps 7] [--iters 3]

Cases: 4096 real rows of n = 16384 to m = 1024 bins (L = 32768), 64 real rows of n = 2^20 to m = 4096
bins (L = 2^21), and 4096 complex rows of n = 16384 to m = 1024 bins.  Beside each figure stand
yardsticks timed in the same process on the same buffers:
  * the floor: two hsfft_exec_batched calls at the length L on as many rows, forward then inverse
    -- the two transforms alone, which the composition cannot beat; and the same two transforms
    walked as the call walks them, in chunks of HSFFT_CZT_CHUNK_MB / (2 x L x 16) rows, which tells
    what of the time beyond the floor is the chunk walk's and what the three kernels';
  * hsfft_bench_copy: the rate of a plain copy, and the time that rate needs for the bytes the three
    kernels around the transforms must move.  Per row the input rotation reads n x 8 (complex: n x
    16) bytes and writes L x 16, the spectral product reads and writes L x 16 (the shared V is
    counted as cached), and the output rotation reads and writes m x 16.  It is compared with the
    time the call spends over its floor;
  * for context, on the real cases: hsfft_r2c_batched_compact at the power of two P >= 1/df, what a
    caller pays today for the same resolution by zero-padding every row to P samples and discarding
    the bins outside the band.  It is timed on --context-rows rows and scaled to the batch.

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


def spot_error(dx, dy, real, n, m, f0, df):
    """the first row's bins 0, 1, m/2 and m-1 against a long-double direct sum: max |difference| / max
    |X|, printed and not asserted"""
    x = dx.to_array(np.float64 if real else np.complex128, count=n).astype(np.clongdouble)
    y = dy.to_array(np.complex128, count=m)
    j = np.arange(n, dtype=np.longdouble)
    two_pi = 2 * np.longdouble("3.14159265358979323846264338327950288")
    errs, mags = [], []
    for k in sorted({0, min(1, m - 1), m // 2, m - 1}):
        a = j * (np.longdouble(f0) + k * np.longdouble(df))
        a = two_pi * (a - np.floor(a))
        want = np.sum(x * (np.cos(a) - 1j * np.sin(a)))
        errs.append(float(abs(np.clongdouble(y[k]) - want)))
        mags.append(float(abs(want)))
    return max(errs) / max(mags)


def bench(tm, args, real, batch, n, m, f0, df, context):
    L = hsfft.czt_shape(n, m)
    esz = 8 if real else 16
    fwd, inv = hsfft.Plan(L, 1), hsfft.Plan(L, -1)
    dx, dy = hsfft.DeviceBuffer(batch * n * esz), hsfft.DeviceBuffer(batch * m * 16)
    da, db = hsfft.DeviceBuffer(batch * L * 16), hsfft.DeviceBuffer(batch * L * 16)
    (hsfft.fill_real if real else hsfft.fill_complex)(dx, batch * n, 0xC2)
    hsfft.fill_complex(da, batch * L, 0xC3)

    def floor():
        hsfft.exec_batched(fwd, da, db, batch)
        hsfft.exec_batched(inv, db, da, batch)

    # the same two transforms walked as the call walks them, in chunks of HSFFT_CZT_CHUNK_MB / (2 x L x 16) rows
    chunk_mb = float(os.environ.get("HSFFT_CZT_CHUNK_MB", 1024.0))
    c = max(1, min(batch, max(1 << 20, int(chunk_mb * (1 << 20))) // (2 * L * 16)))

    def floor_chunked():
        for b0 in range(0, batch, c):
            rows = min(c, batch - b0)
            a, b = hsfft.DeviceView(da, b0 * L * 16), hsfft.DeviceView(db, b0 * L * 16)
            hsfft.exec_batched(fwd, a, b, rows)
            hsfft.exec_batched(inv, b, a, rows)

    variants = {"czt": lambda: hsfft.czt_batched(dx, real, n, dy, m, f0, df, batch), "exec_batched_fwd_inv": floor,
                "exec_batched_fwd_inv_chunked": floor_chunked}
    variants["czt"]()
    hsfft.synchronize()
    err = spot_error(dx, dy, real, n, m, f0, df)
    moved = batch * (n * esz + L * 16 + 2 * L * 16 + 2 * m * 16)
    samples = {k: [] for k in variants}
    samples["copy"] = []
    copy_bytes = batch * L * 16
    for _ in range(args.reps):
        for what, call in variants.items():
            samples[what].append(tm.ms(call, args.iters))
        samples["copy"].append(hsfft.bench_copy(da, db, copy_bytes, args.iters) / args.iters)
    med = {k: stats(v) for k, v in samples.items()}
    base = dict(case="czt_real" if real else "czt_complex", batch=batch, n=n, m=m, L=L, f0=f0, df=df, reps=args.reps,
                iters=args.iters, chunk_mb=float(os.environ.get("HSFFT_CZT_CHUNK_MB", 1024.0)), spot_error=err)
    copy_ms, copy_sp = med["copy"]
    gbs = 2 * copy_bytes / copy_ms / 1e6
    moved_ms = moved / gbs / 1e6
    print(json.dumps(dict(base, what="copy", bytes=copy_bytes, ms=copy_ms, spread=copy_sp, gbs=gbs)), flush=True)
    fms, fsp = med["exec_batched_fwd_inv"]
    print(json.dumps(dict(base, what="exec_batched_fwd_inv", rows=batch, ms=fms, spread=fsp)), flush=True)
    cms, csp = med["exec_batched_fwd_inv_chunked"]
    print(json.dumps(dict(base, what="exec_batched_fwd_inv_chunked", rows_per_chunk=c, ms=cms, spread=csp)), flush=True)
    ms, sp = med["czt"]
    print(json.dumps(dict(base, what="czt", ms=ms, spread=sp, gbins_s=batch * m / ms / 1e6, floor_ms=fms, over_floor=ms / fms,
                          beyond_floor_ms=ms - fms, moved_bytes=moved, moved_at_copy_rate_ms=moved_ms,
                          copy_rate_fraction=moved_ms / (ms - fms) if ms > fms else None,
                          chunked_floor_ms=cms, copy_rate_fraction_beyond_chunked_floor=moved_ms / (ms - cms) if ms > cms else None)),
          flush=True)
    hsfft.synchronize()
    for d in (dx, dy, da, db):
        d.free()
    fwd.close()
    inv.close()
    if context:
        # the zero-padded r2c a caller needs today for bins df apart: P >= 1/df samples per row
        P = 1 << max(1, int(np.ceil(np.log2(1.0 / abs(df)))))
        rows = min(batch, args.context_rows)
        rp = hsfft.RealPlan(P, 1)
        dp, ds = hsfft.DeviceBuffer(rows * P * 8), hsfft.DeviceBuffer(rows * (P // 2 + 1) * 16)
        hsfft.fill_real(dp, rows * P, 0xC4)
        t = [tm.ms(lambda: hsfft.r2c_batched_compact(rp, dp, ds, rows), args.iters) for _ in range(args.reps)]
        rms, rsp = stats(t)
        print(json.dumps(dict(base, what="r2c_compact_zero_padded", P=P, rows_timed=rows, ms=rms, spread=rsp,
                              ms_scaled_to_batch=rms * batch / rows, czt_ms=ms, speedup=rms * batch / rows / ms)), flush=True)
        hsfft.synchronize()
        dp.free()
        ds.free()
        rp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--context-rows", type=int, default=32)
    args = ap.parse_args()
    if hsfft.device_count() < 1:
        raise SystemExit("bench_czt: no GPU")
    hsfft.check(hsfft.lib().hsfft_set_device(0), "set_device")
    tm = Timer()
    bench(tm, args, True, 4096, 16384, 1024, 0.125, 1.0 / (1 << 20), True)
    bench(tm, args, True, 64, 1 << 20, 4096, 0.125, 1.0 / (1 << 24), True)
    bench(tm, args, False, 4096, 16384, 1024, 0.125, 1.0 / (1 << 20), False)
    hsfft.finalize()


if __name__ == "__main__":
    main()
