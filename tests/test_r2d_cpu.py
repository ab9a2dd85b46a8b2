"""CPU-only checks of the 2D real entry points (hsfft_r2c_2d, hsfft_r2c_2d_full, hsfft_c2r_2d of
include/hsfft_gpu.h):
  * the symbols are exported, declared and bound, and the Python callables exist;
  * every bad-argument case is rejected with HSFFT_ERR_ARG and a message before any device is
    touched (so it is testable here), and batch == 0 returns 0;
  * the yardstick of test_gpu_r2d.py -- the expectations composed from the 1D oracle in
    hsfft_r2d_testlib -- is the 2D real DFT: checked against numpy.fft.

No call made here has valid arguments and a non-zero batch: nothing is ever launched, the
pointers are never dereferenced.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hsfft_r2d_testlib as R
import hsfft_testlib as T

import hsfft

NAMES = ("hsfft_r2c_2d", "hsfft_r2c_2d_full", "hsfft_c2r_2d")

# The library is loaded in a child process, as in test_2d_cpu.py (test_kernel_resources.py lets
# objcopy rewrite lib/libhsfft.so while later tests run).  Plans: p0 of 8, r1 of 6 (w = 4), so a
# real image is 8 x 6 x 8 = 384 bytes, a half spectrum 8 x 4 x 16 = 512 and a full one 768.
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import hsfft
L = hsfft.lib()
A, B = 0x10000, 0x20000  # two distinct non-NULL "device pointers" (never dereferenced)
p0, r1 = hsfft.Plan(8, 1), hsfft.RealPlan(6, 1)
P, R = p0.ptr, r1.ptr
def cases(real_first, real_bytes, cplx_bytes):
    # (in, out) pairs whose byte ranges overlap although the pointers differ: the output starts
    # inside the input, and the input starts inside the output (each range with its own size)
    in_bytes, out_bytes = (real_bytes, cplx_bytes) if real_first else (cplx_bytes, real_bytes)
    return [("NULL p0", (None, R, A, B, 1)), ("NULL r1", (P, None, A, B, 1)), ("NULL in", (P, R, None, B, 1)),
            ("NULL out", (P, R, A, None, 1)), ("in == out", (P, R, A, A, 1)), ("negative batch", (P, R, A, B, -1)),
            ("out starts in the input's last 16 bytes", (P, R, A, A + in_bytes - 16, 1)),
            ("in starts in the output's last 16 bytes", (P, R, A + out_bytes - 16, A, 1)),
            ("ranges overlap only at batch 3", (P, R, A, A + 2 * in_bytes, 3))]
bad = {"hsfft_r2c_2d": cases(True, 384, 512), "hsfft_r2c_2d_full": cases(True, 384, 768),
       "hsfft_c2r_2d": cases(False, 384, 512)}
# accepted: batch 0, also with pointers whose ranges would overlap at any other batch
zero = {n: [(P, R, A, B, 0), (P, R, A, A + 16, 0)] for n in bad}
out = {"exported": {n: hasattr(L, n) for n in bad}, "bad": {}, "zero": {}, "raised": {}}
for name, cs in bad.items():
    out["bad"][name] = [(what, getattr(L, name)(*args), L.hsfft_last_error().decode()) for what, args in cs]
    out["zero"][name] = [getattr(L, name)(*args) for args in zero[name]]
class Ptr:
    ptr = A
for what in ("r2c_2d", "r2c_2d_full", "c2r_2d"):
    try:
        getattr(hsfft, what)(p0, r1, Ptr, Ptr, 1)
        out["raised"][what] = None
    except hsfft.HsfftError as e:
        out["raised"][what] = str(e)
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def child():
    """what a fresh process saw: no call in it has valid arguments and a non-zero batch, so
    nothing is launched wherever it runs"""
    res = subprocess.run([sys.executable, "-c", CHILD, T.PKG_DIR], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_symbols_exported_and_declared(child):
    assert os.path.exists(hsfft.LIB_PATH)
    header = open(os.path.join(T.REPO, "include", "hsfft_gpu.h")).read()
    for name in NAMES:
        assert child["exported"][name], name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in hsfft.SIGNATURES, name
    for name in ("r2c_2d", "r2c_2d_full", "c2r_2d", "rfft2", "irfft2"):
        assert callable(getattr(hsfft, name, None)), name
    # the contract's wording on the mirror half: a copy with a sign flip, not a second transform
    assert re.search(r"mirror half.*copy with a sign\s+\*?\s*flip", header, flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_bad_arguments_are_rejected(child, name):
    """HSFFT_ERR_ARG and a message for every bad-argument case, before any device is touched;
    batch == 0 returns 0"""
    assert len(child["bad"][name]) >= 6
    assert any("overlap" in what or "starts in" in what for what, _, _ in child["bad"][name])
    for what, rc, msg in child["bad"][name]:
        assert rc == hsfft.HSFFT_ERR_ARG, (name, what, rc)
        assert msg, (name, what)
    assert child["zero"][name] and all(rc == 0 for rc in child["zero"][name]), child["zero"][name]


def test_bad_arguments_raise_in_python(child):
    """the binding turns the error code into HsfftError with the library's message"""
    assert set(child["raised"]) == {"r2c_2d", "r2c_2d_full", "c2r_2d"}
    for what, msg in child["raised"].items():
        assert msg and "invalid arguments" in msg, (what, msg)


def test_conveniences_reject_bad_shapes_before_loading_anything():
    with pytest.raises(ValueError):
        hsfft.rfft2(np.zeros(8))
    with pytest.raises(ValueError):
        hsfft.rfft2(np.zeros((4, 5)))  # odd n1: the real plan refuses it
    with pytest.raises(ValueError):
        hsfft.irfft2(np.zeros((4, 4), dtype=np.complex128), 8)  # 8/2+1 = 5 bins expected
    assert hsfft.rfft2(np.zeros((0, 4, 6))).shape == (0, 4, 4)
    assert hsfft.rfft2(np.zeros((0, 4, 6)), full=True).shape == (0, 4, 6)
    assert hsfft.irfft2(np.zeros((0, 4, 4), dtype=np.complex128), 6).shape == (0, 4, 6)


# The composed expectations against numpy.  As test_2d_cpu.py explains, the oracle is the
# reference, defects included: with flags 0 a length with a radix-3 stage is not a DFT (D2), so
# 8x6 (inner real plan 3) and 100x60 (inner 30) use the oracle's exact-twiddle flavour, and 97x64
# (Bluestein columns, inner 32) is compared as it is.  Bounds: the normwise error of the oracle
# measured here (max|y - ref| / (eps max|ref|), larger of the two images and of the listed
# transforms), x 4.  An axis or mirror mix-up gives an O(1) relative error, 1e15 in these units.
YARDSTICK = [
    # shape, flags, 4 x measured for the r2c builders, 4 x measured for the c2r builder
    ((8, 6), T.ORC_EXACT, 4 * 2.01e4, 4 * 1.79e4),     # measured 20053.8 (half, full, mixed); c2r 17898.1
    ((100, 60), T.ORC_EXACT, 4 * 8.9e4, 4 * 1.2e5),    # measured 84679.4, 84680.3, mixed 88874.8; c2r 119114.5
    ((97, 64), 0, 4 * 3.71, 4 * 8.09),                 # measured 3.087, 3.085, mixed 3.706; c2r 8.083
]


@pytest.mark.parametrize("shape,flags,bound_r2c,bound_c2r", YARDSTICK, ids=["8x6", "100x60", "97x64"])
def test_composed_oracle_is_the_2d_real_dft(shape, flags, bound_r2c, bound_c2r):
    n0, n1 = shape
    x = R.real_images(n0, n1, 2)
    half = R.oracle_r2c_2d(x, 1, 1, flags)
    errs = {"r2c_2d": max(T.normwise_err(half[b], np.fft.rfft2(x[b])) for b in range(2))}
    full = R.oracle_r2c_2d_full(x, 1, 1, flags)
    errs["r2c_2d_full"] = max(T.normwise_err(full[b], np.fft.fft2(x[b])) for b in range(2))
    # mixed signs: forward rows, inverse columns
    mixed = R.oracle_r2c_2d(x, -1, 1, flags)
    errs["r2c_2d mixed"] = max(T.normwise_err(mixed[b], np.fft.ifft(np.fft.rfft(x[b], axis=1), axis=0) * n0)
                               for b in range(2))
    # c2r of numpy's own half spectrum, so that the two directions are checked independently
    X = np.fft.rfft2(x)
    y = R.oracle_c2r_2d(X, n1, -1, -1, flags)
    errs["c2r_2d"] = max(T.normwise_err(y[b], np.fft.irfft2(X[b], s=(n0, n1)) * (n0 * n1)) for b in range(2))
    bounds = {what: bound_c2r if what == "c2r_2d" else bound_r2c for what in errs}
    for what, err in errs.items():
        print(shape, what, "normwise error", err, "bound", bounds[what])
    for what, err in errs.items():
        assert err <= bounds[what], (shape, what, err)


@pytest.mark.parametrize("shape", [(1, 2), (2, 2), (3, 4), (8, 6), (97, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_full_layout_is_the_half_spectrum_and_its_sign_flipped_mirror(shape):
    """the full-layout builder word by word: columns 0..h are the half spectrum, and the word at
    [k0][k1 > h] is the word at [(n0-k0) % n0][n1-k1] with the sign bit of im flipped, re as it is
    (checked with explicit loops, not with the indexing the builder uses)"""
    n0, n1 = shape
    h = n1 // 2
    x = R.real_images(n0, n1, 2, salt=0xF1)
    half = R.oracle_r2c_2d(x, 1, 1)
    full = R.oracle_r2c_2d_full(x, 1, 1)
    assert full.shape == (2, n0, n1)
    assert T.mismatches(full[:, :, :h + 1], half) == 0
    fw = full.view(np.uint64).reshape(2, n0, n1, 2)
    sign = np.uint64(1 << 63)
    for b in range(2):
        for k0 in range(n0):
            for k1 in range(h + 1, n1):
                src = fw[b, (n0 - k0) % n0, n1 - k1]
                assert fw[b, k0, k1, 0] == src[0] and fw[b, k0, k1, 1] == src[1] ^ sign, (b, k0, k1)


def test_mirror_flips_the_sign_of_zeros_and_nans():
    """complete_full on hand-made words: +0 -> -0, -0 -> +0, and a NaN keeps its payload"""
    half = np.zeros((1, 2, 3), dtype=np.complex128)  # n0 = 2, n1 = 4: one mirror column, k1 = 3 <- 1
    w = half.view(np.uint64).reshape(1, 2, 3, 2)
    w[0, 0, 1] = (0x8000000000000000, 0x0000000000000000)  # (-0, +0)
    w[0, 1, 1] = (0x3FF0000000000000, 0x7FF8000000000123)  # (1, NaN with a payload)
    full = R.complete_full(half, 4).view(np.uint64).reshape(1, 2, 4, 2)
    assert tuple(full[0, 0, 3]) == (0x8000000000000000, 0x8000000000000000)
    assert tuple(full[0, 1, 3]) == (0x3FF0000000000000, 0xFFF8000000000123)
