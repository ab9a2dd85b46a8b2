#!/usr/bin/env python3
"""Timings of the batched analytic signal and of Fourier resampling on one GPU:
standalone, one process, one set of buffers per case, the method of tools/bench_czt.py.

  python tools/bench_spectral.py [--reps 7] [--iters 3]

Cases: the analytic signal of 4096 rows of 65536 and of 64 rows of 2^20; resampling 4096 rows of 65536
to 32768 and 4096 rows of 16384 to 65536.  Beside each figure stand yardsticks timed in the same
process:
  * the bare transforms the call contains, walked as the call walks them, in chunks of
    hsfft_spectral_chunk_rows rows: hsfft_r2c_batched_compact at n from the call's input into a
    chunk-sized buffer, then hsfft_exec_batched of the inverse plan at n (the analytic signal) or
    hsfft_c2r_batched at m (resampling) from a second chunk-sized buffer into the call's output.  The
    composition cannot beat them.  (hsfft_c2r_batched reads its m/2+1 bins at the row pitch m, where
    the call reads them at the pitch m/2+1: the same bins, further apart.);
  * hsfft_bench_copy: the rate of a plain copy that moves as many bytes as the call's one new kernel
    does -- per row it reads the n/2+1 bins (resampling: the min(n, m)/2+1 it keeps) and writes n words
    (resampling: m/2+1), 16 bytes each.  The kernel's own time is the call's time beyond the bare
    transforms; its rate is those bytes over that time, and is given as a fraction of the copy's.

Every figure is the median over --reps repetitions of an event-timed run of --iters calls after one
untimed warm-up call; the spread is (max - min) / median.  A repetition times every variant once, so
the variants alternate and share whatever else the machine is doing.  Prints one JSON line per
measurement.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_2d import Timer, stats  # noqa: E402  (puts the package on sys.path)

import hsfft  # noqa: E402


def spot_error(dx, dy, n, m):
    """the first row against numpy's own composition, max |difference| / max |value|, printed and not
    asserted"""
    x = dx.to_array(np.float64, count=n)
    if m:
        K = min(n, m) // 2
        S = np.fft.rfft(x)
        Y = np.zeros(m // 2 + 1, dtype=np.complex128)
        Y[:K + 1] = S[:K + 1]
        if m > n:
            Y[K] *= 0.5
        elif m < n:
            Y[K] = 2 * Y[K].real
        want = np.fft.irfft(Y, n=m) * (m / n)
        got = dy.to_array(np.float64, count=m)
    else:
        g = np.zeros(n)
        g[0] = g[n // 2] = 1.0
        g[1:n // 2] = 2.0
        want = np.fft.ifft(np.fft.fft(x) * g)
        got = dy.to_array(np.complex128, count=n)
    return float(np.abs(got - want).max() / np.abs(want).max())


def bench(tm, args, batch, n, m):
    """m == 0: the analytic signal; else resampling n -> m"""
    c = min(batch, hsfft.spectral_chunk_rows(n, m))
    rn = hsfft.RealPlan(n, 1)
    inv = hsfft.RealPlan(m, -1) if m else hsfft.Plan(n, -1)
    out_row = m * 8 if m else n * 16
    mid_words = m if m else n  # the bare inverse transform's input row, in complex words
    dx, dy = hsfft.DeviceBuffer(batch * n * 8), hsfft.DeviceBuffer(batch * out_row)
    dS, dE = hsfft.DeviceBuffer(c * (n // 2 + 1) * 16), hsfft.DeviceBuffer(c * mid_words * 16)
    hsfft.fill_real(dx, batch * n, 0x5C)
    hsfft.fill_complex(dE, c * mid_words, 0x5D)

    def call():
        if m:
            hsfft.resample_batched(dx, n, dy, m, batch)
        else:
            hsfft.hilbert_batched(dx, dy, n, batch)

    def bare():
        for b0 in range(0, batch, c):
            rows = min(c, batch - b0)
            hsfft.r2c_batched_compact(rn, hsfft.DeviceView(dx, b0 * n * 8), dS, rows)
            o = hsfft.DeviceView(dy, b0 * out_row)
            if m:
                hsfft.c2r_batched(inv, dE, o, rows)
            else:
                hsfft.exec_batched(inv, dE, o, rows)

    call()
    hsfft.synchronize()
    err = spot_error(dx, dy, n, m)
    moved = batch * 16 * ((min(n, m) // 2 + 1) + (m // 2 + 1) if m else (n // 2 + 1) + n)
    copy_bytes = (moved // 2 + 15) // 16 * 16
    ca, cb = hsfft.DeviceBuffer(copy_bytes), hsfft.DeviceBuffer(copy_bytes)
    hsfft.fill_real(ca, copy_bytes // 8, 0x5E)
    variants = {"call": call, "bare": bare}
    samples = {k: [] for k in variants}
    samples["copy"] = []
    for _ in range(args.reps):
        for what, fn in variants.items():
            samples[what].append(tm.ms(fn, args.iters))
        samples["copy"].append(hsfft.bench_copy(ca, cb, copy_bytes, args.iters) / args.iters)
    med = {k: stats(v) for k, v in samples.items()}
    name = "resample" if m else "hilbert"
    base = dict(case=name, batch=batch, n=n, m=m, rows_per_chunk=c, reps=args.reps, iters=args.iters,
                chunk_mb=float(os.environ.get("HSFFT_SPECTRAL_CHUNK_MB", 1024.0)), spot_error=err)
    copy_ms, copy_sp = med["copy"]
    copy_gbs = 2 * copy_bytes / copy_ms / 1e6
    print(json.dumps(dict(base, what="copy", bytes=copy_bytes, ms=copy_ms, spread=copy_sp, gbs=copy_gbs)), flush=True)
    bms, bsp = med["bare"]
    print(json.dumps(dict(base, what="r2c+c2r_chunked" if m else "r2c+c2c_chunked", ms=bms, spread=bsp)), flush=True)
    ms, sp = med["call"]
    kernel_ms = ms - bms
    print(json.dumps(dict(base, what=name, ms=ms, spread=sp, gsamples_in_s=batch * n / ms / 1e6, bare_ms=bms, over_bare=ms / bms,
                          kernel_ms=kernel_ms, kernel_bytes=moved, kernel_gbs=moved / kernel_ms / 1e6 if kernel_ms > 0 else None,
                          copy_gbs=copy_gbs, copy_rate_fraction=moved / kernel_ms / 1e6 / copy_gbs if kernel_ms > 0 else None)),
          flush=True)
    hsfft.synchronize()
    for d in (dx, dy, dS, dE, ca, cb):
        d.free()
    rn.close()
    inv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    if hsfft.device_count() < 1:
        raise SystemExit("bench_spectral: no GPU")
    hsfft.check(hsfft.lib().hsfft_set_device(0), "set_device")
    tm = Timer()
    bench(tm, args, 4096, 65536, 0)
    bench(tm, args, 64, 1 << 20, 0)
    bench(tm, args, 4096, 65536, 32768)
    bench(tm, args, 4096, 16384, 65536)
    hsfft.finalize()


if __name__ == "__main__":
    main()
