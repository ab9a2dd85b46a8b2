#!/usr/bin/env python3
"""Timings of the batched overlap-add filter on one GPU: standalone, one process,
one set of buffers, the method of tools/bench_conv2d.py.

  python tools/bench_filter.py [--reps 7] [--iters 3] [--batch 64] [--log2n 20]

--batch rows of 2^--log2n samples are filtered by one kernel of m taps, m in {65, 1025}, mode
"full", by hsfft_filter_batched with block in {2048, 4096, 8192, 16384, 32768} and automatic (0).
Beside every run stands the one-shot path on the same rows: hsfft_convolve_batched with the kernel
replicated into --batch rows.  That function is the yardstick: it exists without the filter.

Every figure is the median over --reps repetitions of an event-timed run of --iters calls after
one untimed warm-up call; the spread is (max - min) / median.  A repetition times every variant of
one m once, the one-shot path first, so the variants alternate and share whatever else the machine
is doing.  Before the timing, each variant's first and last output rows are compared with the
one-shot path's (different block lengths round differently: the largest difference is printed
relative to the largest output, it is not asserted).  Scratch bytes are computed from the
documented rules: what each call holds in the library's pool while it runs (the one-shot path's
result buffer, allocated per call, included), the row transforms' inner intermediate counted
apart.  Prints one JSON line per variant.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_2d import Timer, stats  # noqa: E402  (puts the package on sys.path)

import hsfft  # noqa: E402

BLOCKS = (2048, 4096, 8192, 16384, 32768, 0)
TAPS = (65, 1025)


def filter_scratch(P, m, blocks, chunk_mb=1024.0):
    """(pool bytes of hsfft_filter_batched, bytes of the row transforms' inner intermediate)"""
    per = P * 8 + (P // 2 + 1) * 16
    c = max(1, min(blocks, int(chunk_mb * (1 << 20)) // per))
    return c * per + (P // 2 + 1) * 16 + m * 8, c * (P // 2) * 16


def oneshot_scratch(P, batch):
    """the same for hsfft_convolve_batched: both padded operands, both compact spectra and the
    padded result; the inner intermediate of its row transforms"""
    return 2 * batch * P * 8 + 2 * batch * (P // 2 + 1) * 16 + batch * P * 8, batch * (P // 2) * 16


def rows(buf, olen, which):
    return [buf.to_array(np.float64, count=olen, offset_bytes=r * olen * 8) for r in which]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--log2n", type=int, default=20)
    args = ap.parse_args()
    if hsfft.device_count() < 1:
        raise SystemExit("bench_filter: no GPU")
    hsfft.check(hsfft.lib().hsfft_set_device(0), "set_device")
    tm = Timer()
    batch, n = args.batch, 1 << args.log2n
    chunk_mb = float(os.environ.get("HSFFT_FILTER_CHUNK_MB", 1024.0))
    dx = hsfft.DeviceBuffer(batch * n * 8)
    hsfft.fill_real(dx, batch * n, 0xF1)
    for m in TAPS:
        olen = n + m - 1
        P1 = 1 << (olen - 1).bit_length()
        dh1, dhb = hsfft.DeviceBuffer(m * 8), hsfft.DeviceBuffer(batch * m * 8)
        hsfft.fill_real(dh1, m, 0xF2)
        hrep = np.tile(dh1.to_array(np.float64), batch)  # kept alive until the synchronous copy returns
        hsfft.check(hsfft.lib().hsfft_memcpy_h2d(dhb.ptr, hrep.ctypes.data, hrep.nbytes), "h2d")
        ref, out = hsfft.DeviceBuffer(batch * olen * 8), hsfft.DeviceBuffer(batch * olen * 8)
        L = hsfft.lib()

        def oneshot():
            hsfft.check(L.hsfft_convolve_batched(b"full", b"linear", dx.ptr, n, dhb.ptr, m, ref.ptr, batch), "convolve")

        def filt(block):
            return lambda: hsfft.filter_batched("full", dx, n, dh1, m, block, out, batch)

        oneshot()
        hsfft.synchronize()
        want = rows(ref, olen, (0, batch - 1))
        scale = max(float(np.abs(w).max()) for w in want)
        diffs = {}
        for block in BLOCKS:
            filt(block)()
            hsfft.synchronize()
            got = rows(out, olen, (0, batch - 1))
            diffs[block] = max(float(np.abs(g - w).max()) for g, w in zip(got, want)) / scale
        samples = {"oneshot": []}
        samples.update({block: [] for block in BLOCKS})
        for _ in range(args.reps):
            samples["oneshot"].append(tm.ms(oneshot, args.iters))
            for block in BLOCKS:
                samples[block].append(tm.ms(filt(block), args.iters))
        one_ms, one_sp = stats(samples["oneshot"])
        pool, inner = oneshot_scratch(P1, batch)
        base = dict(batch=batch, n=n, m=m, reps=args.reps, iters=args.iters)
        print(json.dumps(dict(base, what="convolve_batched", P=P1, ms=one_ms, spread=one_sp,
                              gsamples_s=batch * n / one_ms / 1e6, scratch_bytes=pool, inner_bytes=inner)), flush=True)
        for block in BLOCKS:
            ms, sp = stats(samples[block])
            _, P, Lb, nseg = hsfft.filter_shape("full", n, m, block)
            pool, inner = filter_scratch(P, m, batch * nseg, chunk_mb)
            print(json.dumps(dict(base, what="filter_batched", block=block, P=P, L=Lb, blocks=batch * nseg, ms=ms,
                                  spread=sp, gsamples_s=batch * n / ms / 1e6, over_oneshot=ms / one_ms,
                                  scratch_bytes=pool, inner_bytes=inner, max_rel_diff_vs_oneshot=diffs[block])),
                  flush=True)
        hsfft.synchronize()
        for d in (dh1, dhb, ref, out):
            d.free()
        hsfft.check(L.hsfft_release_scratch(), "release_scratch")
    dx.free()
    hsfft.finalize()


if __name__ == "__main__":
    main()
