#!/usr/bin/env python3
"""Timings of the batched STFT and its inverse on one GPU: standalone, one process,
one set of buffers, the method of tools/bench_filter.py.

  python tools/bench_stft.py [--reps 7] [--iters 3] [--batch 64] [--log2n 20] [--nfft 1024] [--hop 256]

--batch rows of 2^--log2n samples, frames of --nfft samples --hop apart, periodic Hann window,
centred: hsfft_stft_batched, and hsfft_istft_batched (normalised) on the spectra it wrote.  Beside
each figure stand two yardsticks timed in the same process:
  * the row transform alone on the same number of ready-made frames -- hsfft_r2c_batched_compact,
    respectively hsfft_c2r_batched -- the floor the composition cannot beat;
  * hsfft_bench_copy of the bytes the frame gather, respectively the overlap-add, must move (the
    signal once and the frame matrix once: a copy of half that many bytes reads and writes as
    much), to be compared with the time the call spends over its floor.

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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--nfft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=256)
    args = ap.parse_args()
    if hsfft.device_count() < 1:
        raise SystemExit("bench_stft: no GPU")
    hsfft.check(hsfft.lib().hsfft_set_device(0), "set_device")
    tm = Timer()
    batch, n, N, hop = args.batch, 1 << args.log2n, args.nfft, args.hop
    nframes, bins, lpad = hsfft.stft_shape(n, N, hop, True)
    frames = batch * nframes
    chunk_mb = float(os.environ.get("HSFFT_STFT_CHUNK_MB", 1024.0))
    rf, ri = hsfft.RealPlan(N, 1), hsfft.RealPlan(N, -1)
    dx, dy = hsfft.DeviceBuffer(batch * n * 8), hsfft.DeviceBuffer(batch * n * 8)
    hsfft.fill_real(dx, batch * n, 0x57)
    dw = hsfft.DeviceBuffer.from_array(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N))
    spec = hsfft.DeviceBuffer(frames * bins * 16)   # the STFT's output, the inverse's input, the r2c floor's output
    ready = hsfft.DeviceBuffer(frames * N * 8)      # ready-made frames: the r2c floor's input, the c2r floor's output
    wide = hsfft.DeviceBuffer(frames * N * 16)      # spectra at the pitch N hsfft_c2r_batched reads; the copy's two halves
    hsfft.fill_real(ready, frames * N, 0x58)
    hsfft.fill_complex(wide, frames * N, 0x59)
    moved = batch * n * 8 + frames * N * 8          # what the gather reads and writes; the overlap-add the same, reversed
    copy_bytes = moved // 2 // 16 * 16
    half = hsfft.DeviceView(wide, frames * N * 8)
    assert copy_bytes <= frames * N * 8

    variants = {
        "stft_batched": lambda: hsfft.stft_batched(rf, dx, n, dw, hop, True, spec, batch),
        "r2c_batched_compact": lambda: hsfft.r2c_batched_compact(rf, ready, spec, frames),
        "istft_batched": lambda: hsfft.istft_batched(ri, spec, nframes, dw, hop, True, True, dy, n, batch),
        "c2r_batched": lambda: hsfft.c2r_batched(ri, wide, ready, frames),
    }
    # the round trip's error, printed and not asserted: the spectra in `spec` must be the STFT's when the inverse runs
    variants["stft_batched"]()
    variants["istft_batched"]()
    hsfft.synchronize()
    x0, y0 = dx.to_array(np.float64, count=n), dy.to_array(np.float64, count=n)
    round_trip = float(np.abs(y0 - x0).max())

    samples = {k: [] for k in variants}
    samples["copy"] = []
    for _ in range(args.reps):
        for what in ("stft_batched", "istft_batched", "r2c_batched_compact", "c2r_batched"):
            if what == "istft_batched":  # on the STFT's spectra, not on the floor's
                variants["stft_batched"]()
            samples[what].append(tm.ms(variants[what], args.iters))
        samples["copy"].append(hsfft.bench_copy(wide, half, copy_bytes, args.iters) / args.iters)
    med = {k: stats(v) for k, v in samples.items()}
    base = dict(batch=batch, n=n, nfft=N, hop=hop, center=1, nframes=nframes, frames=frames, reps=args.reps,
                iters=args.iters, chunk_mb=chunk_mb)
    copy_ms, copy_sp = med["copy"]
    print(json.dumps(dict(base, what="copy", bytes=copy_bytes, ms=copy_ms, spread=copy_sp, gbs=2 * copy_bytes / copy_ms / 1e6)),
          flush=True)
    for what, floor in (("stft_batched", "r2c_batched_compact"), ("istft_batched", "c2r_batched")):
        ms, sp = med[what]
        fms, fsp = med[floor]
        print(json.dumps(dict(base, what=floor, ms=fms, spread=fsp)), flush=True)
        print(json.dumps(dict(base, what=what, ms=ms, spread=sp, gsamples_s=batch * n / ms / 1e6, floor_ms=fms,
                              over_floor=ms / fms, beyond_floor_ms=ms - fms, moved_bytes=moved, copy_ms=copy_ms,
                              copy_rate_fraction=copy_ms / (ms - fms) if ms > fms else None,
                              round_trip_max_error=round_trip)), flush=True)
    hsfft.synchronize()
    for d in (dx, dy, dw, spec, ready, wide):
        d.free()
    rf.close()
    ri.close()
    hsfft.finalize()


if __name__ == "__main__":
    main()
