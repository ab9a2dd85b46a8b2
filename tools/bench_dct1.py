#!/usr/bin/env python3
"""Timings of the batched type-I cosine and sine transforms on one GPU: standalone,
one process, one set of buffers per case, the method of tools/bench_spectral.py.

  python tools/bench_dct1.py [--reps 7] [--iters 3] [--case NAME]

Cases (--case runs one of them, for a kernel trace of one shape): `rows_cos` 4096 rows of 65537
(cosine, L = 2^17), `rows_sin` 4096 rows of 65535 (sine, L = 2^17), `short_cos` 65536 rows of 4097
(cosine, L = 2^13), `img_cos` 512 images of 1025 x 1025 (cosine) and `img_sin` 512 images of 1023 x 1023
(sine, L = 2^11 on both axes).  Beside each figure stand yardsticks timed in the same process:
  * the bare transforms the call contains, walked as the call walks them: hsfft_r2c_batched_compact at
    L on rows of L doubles, in chunks of HSFFT_DCT_CHUNK_MB / (L x 8 + (L/2+1) x 16) rows, from one
    chunk-sized buffer into another; for an image both axes' rows, and beside them the two
    hsfft_transpose_real_batched a 2D call makes.  The composition cannot beat them;
  * hsfft_bench_copy: the rate of a plain copy that moves as many bytes as the call's two new kernels
    do -- per row of n the extension reads n x 8 bytes and writes L x 8, and the output kernel reads n
    bins of 16 bytes and writes n x 8.  The kernels' own time is the call's time beyond the bare
    transforms (and transposes); their rate is those bytes over that time, given as a fraction of the
    copy's.  Each kernel's own time comes from a kernel trace of one case.

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

CASES = {
    "rows_cos": (hsfft.KIND_COS, 4096, 0, 65537),
    "rows_sin": (hsfft.KIND_SIN, 4096, 0, 65535),
    "short_cos": (hsfft.KIND_COS, 65536, 0, 4097),
    "img_cos": (hsfft.KIND_COS, 512, 1025, 1025),
    "img_sin": (hsfft.KIND_SIN, 512, 1023, 1023),
}


def chunk_rows(L):
    """the call's rule: bytes of the knob over the scratch bytes of one row"""
    mb = float(os.environ.get("HSFFT_DCT_CHUNK_MB", 1024.0))
    return max(1, max(1 << 20, int(mb * (1 << 20))) // (L * 8 + (L // 2 + 1) * 16))


def spot_error(kind, x, got):
    """one row against numpy's own composition, max |difference| / max |value|, printed and not asserted"""
    n = x.size
    if kind == hsfft.KIND_SIN:
        e = np.concatenate([[0.0], x, [0.0], -x[::-1]])
        want = -np.fft.rfft(e).imag[1:n + 1]
    else:
        e = np.concatenate([x, x[n - 2:0:-1]])
        want = np.fft.rfft(e).real[:n]
    return float(np.abs(got - want).max() / np.abs(want).max())


def bench(tm, args, name):
    kind, batch, n0, n1 = CASES[name]
    two_d = n0 > 0
    words = batch * (n0 if two_d else 1) * n1
    axes = [(n1, words // n1)] + ([(n0, words // n0)] if two_d else [])  # (row length, rows) of every pass
    dx, dy = hsfft.DeviceBuffer(words * 8), hsfft.DeviceBuffer(words * 8)
    hsfft.fill_real(dx, words, 0xD1)
    bare_bufs, plans, moved = [], [], 0
    for n, rows in axes:
        L, bins = hsfft.dct1_shape(kind, n)
        c = min(rows, chunk_rows(L))
        r, s = hsfft.DeviceBuffer(c * L * 8), hsfft.DeviceBuffer(c * bins * 16)
        hsfft.fill_real(r, c * L, 0xD2)
        plans.append(hsfft.RealPlan(L, 1))
        bare_bufs.append((L, rows, c, r, s))
        moved += rows * (n * 8 + L * 8 + n * 16 + n * 8)

    def call():
        if two_d:
            hsfft.dct1_2d_batched(kind, kind, dx, dy, n0, n1, batch)
        else:
            hsfft.dct1_batched(kind, dx, dy, n1, batch)

    def bare():
        for plan, (L, rows, c, r, s) in zip(plans, bare_bufs):
            for b0 in range(0, rows, c):
                hsfft.r2c_batched_compact(plan, r, s, min(c, rows - b0))

    def transposes():
        hsfft.transpose_real_batched(dx, dy, n0, n1, batch)
        hsfft.transpose_real_batched(dx, dy, n1, n0, batch)

    call()
    hsfft.synchronize()
    if two_d:  # the first image of the batch against the convenience on that image alone: absolute, 0 expected
        x = dx.to_array(np.float64, count=n0 * n1)
        back = hsfft.dct1n(x.reshape(n0, n1)) if kind == hsfft.KIND_COS else hsfft.dst1n(x.reshape(n0, n1))
        err = float(np.abs(dy.to_array(np.float64, count=n0 * n1).reshape(n0, n1) - back).max())
    else:
        err = spot_error(kind, dx.to_array(np.float64, count=n1), dy.to_array(np.float64, count=n1))
    copy_bytes = (moved // 2 + 15) // 16 * 16
    ca, cb = hsfft.DeviceBuffer(copy_bytes), hsfft.DeviceBuffer(copy_bytes)
    hsfft.fill_real(ca, copy_bytes // 8, 0xD3)
    variants = {"call": call, "bare": bare}
    if two_d:
        variants["transposes"] = transposes
    samples = {k: [] for k in variants}
    samples["copy"] = []
    for _ in range(args.reps):
        for what, fn in variants.items():
            samples[what].append(tm.ms(fn, args.iters))
        samples["copy"].append(hsfft.bench_copy(ca, cb, copy_bytes, args.iters) / args.iters)
    med = {k: stats(v) for k, v in samples.items()}
    base = dict(case=name, kind="sine" if kind == hsfft.KIND_SIN else "cosine", batch=batch, n0=n0, n1=n1,
                L=[b[0] for b in bare_bufs], rows_per_chunk=[b[2] for b in bare_bufs], reps=args.reps, iters=args.iters,
                chunk_mb=float(os.environ.get("HSFFT_DCT_CHUNK_MB", 1024.0)), spot_error=err)
    copy_ms, copy_sp = med["copy"]
    copy_gbs = 2 * copy_bytes / copy_ms / 1e6
    print(json.dumps(dict(base, what="copy", bytes=copy_bytes, ms=copy_ms, spread=copy_sp, gbs=copy_gbs)), flush=True)
    bms, bsp = med["bare"]
    print(json.dumps(dict(base, what="r2c_chunked", ms=bms, spread=bsp)), flush=True)
    tms = 0.0
    if two_d:
        tms, tsp = med["transposes"]
        print(json.dumps(dict(base, what="two_transposes", ms=tms, spread=tsp)), flush=True)
    ms, sp = med["call"]
    kernel_ms = ms - bms - tms
    print(json.dumps(dict(base, what="dct1_2d" if two_d else "dct1", ms=ms, spread=sp, gsamples_s=words / ms / 1e6, bare_ms=bms,
                          over_bare=ms / bms, transposes_ms=tms, kernels_ms=kernel_ms, kernels_bytes=moved,
                          kernels_gbs=moved / kernel_ms / 1e6 if kernel_ms > 0 else None, copy_gbs=copy_gbs,
                          copy_rate_fraction=moved / kernel_ms / 1e6 / copy_gbs if kernel_ms > 0 else None)), flush=True)
    hsfft.synchronize()
    for d in [dx, dy, ca, cb] + [b for bb in bare_bufs for b in bb[3:]]:
        d.free()
    for p in plans:
        p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--case", choices=sorted(CASES), default=None)
    args = ap.parse_args()
    if hsfft.device_count() < 1:
        raise SystemExit("bench_dct1: no GPU")
    hsfft.check(hsfft.lib().hsfft_set_device(0), "set_device")
    tm = Timer()
    for name in ([args.case] if args.case else list(CASES)):
        bench(tm, args, name)
    hsfft.finalize()


if __name__ == "__main__":
    main()
