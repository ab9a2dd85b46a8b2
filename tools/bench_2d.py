#!/usr/bin/env python3
"""Transpose and 2D-transform timings on one GPU: standalone, one process, one
set of buffers.

  python tools/bench_2d.py [--reps 7] [--iters 5] [--variants]

Every figure is the median over --reps repetitions of an event-timed run of --iters calls, after
one untimed warm-up call; the spread is (max - min) / median over the repetitions.
  (a) hsfft_bench_copy of the same byte count: the box's practical copy rate;
  (b) hsfft_transpose_batched, reported as a fraction of (a);
  (c) hsfft_exec_2d;
  (d) the two 1D row runs (hsfft_time_batched) a 2D call consists of;
  and (c) / ((d) + 2 x (a)): the floor of the four-trip design is (d) + 2 x (a), so the ratio is
  what the driver and the transposes cost over it.
--variants repeats (b) for the other tile size and tile order (HSFFT_TR_TILE, HSFFT_TR_DIAG).
Prints one JSON line per measurement.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mixed-radix-fast-fourier-transform_amd"))

import hsfft  # noqa: E402

VP = ctypes.c_void_p


class Timer:
    """HIP events on the library stream around a loop of calls"""

    def __init__(self):
        try:
            self.hip = ctypes.CDLL("libamdhip64.so")
        except OSError:
            self.hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.e0, self.e1 = VP(), VP()
        assert self.hip.hipEventCreate(ctypes.byref(self.e0)) == 0 and self.hip.hipEventCreate(ctypes.byref(self.e1)) == 0
        self.stream = VP(hsfft.lib().hsfft_get_stream())

    def ms(self, call, iters):
        call()  # warm-up
        self.hip.hipEventRecord(self.e0, self.stream)
        for _ in range(iters):
            call()
        self.hip.hipEventRecord(self.e1, self.stream)
        self.hip.hipEventSynchronize(self.e1)
        t = ctypes.c_float(0)
        assert self.hip.hipEventElapsedTime(ctypes.byref(t), self.e0, self.e1) == 0
        return t.value / iters


def stats(samples):
    med = statistics.median(samples)
    return med, (max(samples) - min(samples)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--variants", action="store_true")
    args = ap.parse_args()
    if hsfft.device_count() < 1:
        raise SystemExit("bench_2d: no GPU")
    hsfft.check(hsfft.lib().hsfft_set_device(0), "set_device")
    tm = Timer()
    count = 4096 * 4096 * 16  # every case below holds this many samples: 4 GiB per buffer
    nbytes = count * 16
    a, b = hsfft.DeviceBuffer(nbytes), hsfft.DeviceBuffer(nbytes)
    hsfft.fill_complex(a, count, 0x2D)
    hsfft.synchronize()

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    copy_ms, copy_sp = stats([hsfft.bench_copy(a, b, nbytes, args.iters) / args.iters for _ in range(args.reps)])
    emit(what="copy", bytes=nbytes, ms=copy_ms, spread=copy_sp, gbs=2 * nbytes / copy_ms / 1e6)

    def transposes(tag):
        for rows, cols, batch in [(4096, 4096, 16), (512, 32768, 16), (32768, 512, 16)]:
            ms, sp = stats([tm.ms(lambda: hsfft.transpose_batched(a, b, rows, cols, batch), args.iters)
                            for _ in range(args.reps)])
            emit(what="transpose", variant=tag, rows=rows, cols=cols, batch=batch, ms=ms, spread=sp,
                 gbs=2 * nbytes / ms / 1e6, fraction_of_copy=copy_ms / ms)

    transposes("default")
    if args.variants:
        for tile in ("32", "64"):
            for diag in ("1", "0"):
                os.environ["HSFFT_TR_TILE"], os.environ["HSFFT_TR_DIAG"] = tile, diag
                transposes(f"tile{tile}-diag{diag}")
        del os.environ["HSFFT_TR_TILE"], os.environ["HSFFT_TR_DIAG"]

    for n0, n1, batch in [(4096, 4096, 16), (1024, 1024, 256)]:
        p0 = hsfft.Plan(n0, 1)
        p1 = hsfft.Plan(n1, 1)
        ms2, sp2 = stats([tm.ms(lambda: hsfft.exec_2d(p0, p1, a, b, batch), args.iters) for _ in range(args.reps)])
        rows_ms = []
        for p, nrows in ((p1, batch * n0), (p0, batch * n1)):
            hsfft.time_batched(p, a, b, nrows, 1)  # warm-up
            ms, _ = stats([hsfft.time_batched(p, a, b, nrows, args.iters)[0] / args.iters for _ in range(args.reps)])
            rows_ms.append(ms)
        floor = sum(rows_ms) + 2 * copy_ms
        emit(what="exec_2d", n0=n0, n1=n1, batch=batch, ms=ms2, spread=sp2, rows_ms=rows_ms, copy_ms=copy_ms,
             floor_ms=floor, ratio_to_floor=ms2 / floor, gsamples_s=count / ms2 / 1e6)
        p0.close()
        p1.close()
    hsfft.synchronize()
    a.free()
    b.free()
    hsfft.finalize()


if __name__ == "__main__":
    main()
