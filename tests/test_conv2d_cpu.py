"""CPU-only checks of the batched 2D convolution (hsfft_convolve_2d_shape,
hsfft_convolve_2d_batched of include/hsfft_gpu.h):
  * the symbols are exported, declared and bound, and the Python callables exist;
  * hsfft_convolve_2d_shape equals the restated per-axis rule over a grid of sizes;
  * every bad-argument case is rejected with HSFFT_ERR_ARG and a message before any device is
    touched (so it is testable here), and batch == 0 returns 0;
  * the yardstick of test_gpu_conv2d.py -- the expectation composed in hsfft_conv2d_testlib -- is
    pinned to the reference's own fft_convolve (one-row images, so P0 = 1) word for word, and is
    the 2D convolution: checked against a direct sum.

No call made here has valid arguments and a non-zero batch: nothing is ever launched, the
pointers are never dereferenced.
"""
import itertools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hsfft_conv2d_testlib as C
import hsfft_testlib as T

import hsfft

NAMES = ("hsfft_convolve_2d_shape", "hsfft_convolve_2d_batched")

SHAPE_GRID = [(1, 2, 1, 1), (2, 1, 1, 2), (1, 5, 1, 3), (5, 7, 3, 2), (3, 9, 8, 2), (8, 2, 3, 9), (4, 4, 4, 4),
              (33, 33, 32, 32), (40, 70, 30, 60), (100, 200, 29, 57), (2, 200000, 1, 60000), (1000, 1000, 25, 25)]

# The library is loaded in a child process, as in test_r2d_cpu.py (test_kernel_resources.py lets
# objcopy rewrite lib/libhsfft.so while later tests run).  a is 4 x 6 (192 bytes an image), b is
# 3 x 2 (48 bytes), so a full linear output is 6 x 7 doubles = 336 bytes.
CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import hsfft
L = hsfft.lib()
A, B, O = 0x10000, 0x20000, 0x30000  # distinct non-NULL "device pointers" (never dereferenced)
F, LIN = b"full", b"linear"
def call(t=F, ct=LIN, a=A, ar=4, ac=6, b=B, br=3, bc=2, bb=1, o=O, n=1):
    return (t, ct, a, ar, ac, b, br, bc, bb, o, n)
bad = [("NULL conv_type", call(ct=None)), ("NULL a", call(a=None)), ("NULL b", call(b=None)), ("NULL out", call(o=None)),
       ("unknown type", call(t=b"most")), ("unknown type, circular", call(t=b"most", ct=b"circular")),
       ("unknown conv_type", call(ct=b"spiral")),
       ("a_rows 0", call(ar=0)), ("a_cols 0", call(ac=0)), ("b_rows 0", call(br=0)), ("b_cols -1", call(bc=-1)),
       ("negative batch", call(n=-1)), ("b_batch 2 of batch 3", call(bb=2, n=3)), ("b_batch 0", call(bb=0, n=3)),
       ("both widths 1", call(ac=1, bc=1)), ("both widths 1, circular", call(ct=b"circular", ac=1, bc=1)),
       ("out == a", call(o=A)), ("out == b", call(o=B)),
       ("out starts in a's last 8 bytes", call(o=A + 192 - 8)),
       ("a starts in out's last 8 bytes", call(a=O + 336 - 8)),
       ("out starts in b's last 8 bytes", call(o=B + 48 - 8)),
       ("b starts in out's last 8 bytes", call(b=O + 336 - 8)),
       ("out overlaps a only at batch 3", call(o=A + 2 * 192, n=3)),
       ("out overlaps per-image b only at batch 3", call(o=B + 2 * 48, bb=3, n=3))]
zero = [call(n=0), call(n=0, bb=5), call(n=0, o=A + 8)]
out = {"exported": {n: hasattr(L, n) for n in ("hsfft_convolve_2d_shape", "hsfft_convolve_2d_batched")}}
out["bad"] = [(what, L.hsfft_convolve_2d_batched(*args), L.hsfft_last_error().decode()) for what, args in bad]
out["zero"] = [L.hsfft_convolve_2d_batched(*args) for args in zero]
v = [ctypes.c_int(-7) for _ in range(4)]
refs = [ctypes.byref(x) for x in v]
out["shape_bad"] = [(what, L.hsfft_convolve_2d_shape(*args, *refs), L.hsfft_last_error().decode()) for what, args in [
    ("NULL conv_type", (F, None, 4, 6, 3, 2)), ("unknown type", (b"most", LIN, 4, 6, 3, 2)),
    ("unknown conv_type", (F, b"spiral", 4, 6, 3, 2)), ("dimension 0", (F, LIN, 4, 0, 3, 2)),
    ("both widths 1", (F, LIN, 4, 1, 3, 1))]]
out["shape_untouched"] = [x.value for x in v]
out["shape_null_type"] = (L.hsfft_convolve_2d_shape(None, LIN, 4, 6, 3, 2, *refs), [x.value for x in v])
out["shape_null_results"] = L.hsfft_convolve_2d_shape(F, LIN, 4, 6, 3, 2, None, None, None, None)
out["grid"] = []
for ar, ac, br, bc in json.loads(sys.argv[2]):
    for t in ("full", "same", "valid"):
        for ct in ("linear", "circular"):
            out["grid"].append(((t, ct, ar, ac, br, bc), list(hsfft.convolve_2d_shape(t, ct, ar, ac, br, bc))))
class Ptr:
    ptr = A
out["raised"] = {}
for what, fn in [
        ("convolve_2d_batched", lambda: hsfft.convolve_2d_batched("full", "linear", Ptr, 4, 6, Ptr, 3, 2, 1, Ptr, 1)),
        ("convolve_2d_shape", lambda: hsfft.convolve_2d_shape("most", "linear", 4, 6, 3, 2))]:
    try:
        fn()
        out["raised"][what] = None
    except hsfft.HsfftError as e:
        out["raised"][what] = str(e)
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def child():
    """what a fresh process saw: no call in it has valid arguments and a non-zero batch, so
    nothing is launched wherever it runs"""
    res = subprocess.run([sys.executable, "-c", CHILD, T.PKG_DIR, json.dumps(SHAPE_GRID)], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_symbols_exported_and_declared(child):
    assert os.path.exists(hsfft.LIB_PATH)
    header = open(os.path.join(T.REPO, "include", "hsfft_gpu.h")).read()
    for name in NAMES:
        assert child["exported"][name], name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in hsfft.SIGNATURES, name
    for name in ("convolve_2d_shape", "convolve_2d_batched", "convolve2d"):
        assert callable(getattr(hsfft, name, None)), name
    # the chunk rule the GPU test relies on is documented
    assert re.search(r"HSFFT_2D_CHUNK_MB / \(3 x P0 x \(P1/2\+1\) x 16\)", header)


def test_shape_matches_the_restated_rule(child):
    assert len(child["grid"]) == 6 * len(SHAPE_GRID)
    for (t, ct, ar, ac, br, bc), got in child["grid"]:
        assert tuple(got) == C.shape_rule(t, ct, ar, ac, br, bc), (t, ct, ar, ac, br, bc, got)
    # spot values, written out: 1000 x 1000 with a 25 x 25 kernel pads to 1024 x 1024
    grid = {tuple(k): tuple(v) for k, v in child["grid"]}
    assert grid[("same", "linear", 1000, 1000, 25, 25)] == (1000, 1000, 1024, 1024)
    assert grid[("valid", "linear", 3, 9, 8, 2)] == (6, 8, 16, 16)
    assert grid[("full", "circular", 5, 7, 3, 2)] == (8, 8, 8, 8)
    assert grid[("full", "linear", 2, 200000, 1, 60000)] == (2, 259999, 2, 1 << 18)


def test_shape_rejects_bad_arguments(child):
    for what, rc, msg in child["shape_bad"]:
        assert rc == hsfft.HSFFT_ERR_ARG, (what, rc)
        assert msg, what
    assert child["shape_untouched"] == [-7] * 4  # a rejected call writes no result
    assert child["shape_null_type"] == [0, [6, 7, 8, 8]]  # NULL type is "full"
    assert child["shape_null_results"] == 0


def test_bad_arguments_are_rejected(child):
    """HSFFT_ERR_ARG and a message for every bad-argument case, before any device is touched;
    batch == 0 returns 0"""
    assert len(child["bad"]) >= 20
    for what, rc, msg in child["bad"]:
        assert rc == hsfft.HSFFT_ERR_ARG, (what, rc, msg)
        assert msg, what
    assert child["zero"] == [0, 0, 0]


def test_bad_arguments_raise_in_python(child):
    assert set(child["raised"]) == {"convolve_2d_batched", "convolve_2d_shape"}
    assert "overlaps" in child["raised"]["convolve_2d_batched"]
    assert "output type" in child["raised"]["convolve_2d_shape"]


def test_convolve2d_rejects_bad_shapes_before_loading_anything():
    z = np.zeros
    for a, b, kw in [(z(8), z((2, 2)), {}), (z((4, 4)), z(3), {}), (z((2, 4, 4)), z((3, 2, 2)), {}),
                     (z((2, 4, 4)), z((1, 2, 2)), {}), (z((4, 1)), z((2, 1)), {}), (z((4, 0)), z((2, 2)), {}),
                     (z((4, 4)), z((2, 2)), {"mode": "most"}), (z((4, 4)), z((2, 2)), {"boundary": "spiral"})]:
        with pytest.raises(ValueError):
            hsfft.convolve2d(a, b, **kw)
    assert hsfft.convolve2d(z((0, 4, 6)), z((3, 2))).shape == (0, 6, 7)
    assert hsfft.convolve2d(z((0, 4, 6)), z((0, 3, 2)), mode="valid").shape == (0, 2, 5)
    assert hsfft.convolve2d(z((0, 2, 4, 6)), z((3, 2)), mode="same").shape == (0, 2, 4, 6)
    assert hsfft.convolve2d(z((0, 5, 7)), z((3, 2)), boundary="circular").shape == (0, 8, 8)


# ---------------------------------------------------------------- the yardstick, pinned
@pytest.mark.parametrize("ct", C.CONV_TYPES)
@pytest.mark.parametrize("typ", C.TYPES)
def test_one_row_images_equal_the_reference_1d_convolution(typ, ct):
    """a_rows = b_rows = 1, so P0 = 1 and the column transforms are the reference's length-1 copy:
    the composed 2D expectation equals the oracle's fft_convolve word for word"""
    for n, m in [(5, 3), (3, 5), (16, 16), (100, 7), (7, 100), (1, 4), (4, 1), (33, 32), (1000, 25)]:
        a, b = C.images(1, n, 1, salt=0x1D), C.images(1, m, 1, salt=0x2D)
        want = T.oracle_convolve(typ.encode(), ct.encode(), a[0, 0], b[0, 0])
        got = C.oracle_convolve_2d(typ, ct, a, b)
        assert got.shape == (1, 1, want.size), (typ, ct, n, m, got.shape, want.size)
        assert T.mismatches(got[0, 0], want) == 0, (typ, ct, n, m)


def _direct(a, b):
    """full linear 2D convolution of one pair by a sum over the kernel's taps (no FFT)"""
    out = np.zeros((a.shape[0] + b.shape[0] - 1, a.shape[1] + b.shape[1] - 1))
    for k, l in itertools.product(range(b.shape[0]), range(b.shape[1])):
        out[k:k + a.shape[0], l:l + a.shape[1]] += a * b[k, l]
    return out


def _fold(full, P0, P1):
    """the circular result of period P0 x P1 from the full linear one"""
    out = np.zeros((P0, P1))
    for i0, j0 in itertools.product(range(0, full.shape[0], P0), range(0, full.shape[1], P1)):
        blk = full[i0:i0 + P0, j0:j0 + P1]
        out[:blk.shape[0], :blk.shape[1]] += blk
    return out


# Bounds: the normwise error of the composed expectation against the direct sum measured here
# (max|y - ref| / (eps max|ref|), the larger of the two pairs and of the three windows), x 4.  An
# axis or window mix-up gives an O(1) relative error, 1e15 in these units.
YARDSTICK = [
    # a shape, b shape, 4 x measured linear, 4 x measured circular
    ((5, 7), (3, 2), 4 * 1.50, 4 * 1.50),      # measured 1.498 (full, same, valid); circular 1.498
    ((33, 20), (8, 31), 4 * 3.74, 4 * 3.85),   # measured 3.428, 3.428, valid 3.732; circular 3.842
    ((100, 60), (9, 9), 4 * 4.36, 4 * 4.16),   # measured 4.038, 4.038, valid 4.352; circular 4.151
]


@pytest.mark.parametrize("ash,bsh,bound_lin,bound_circ", YARDSTICK, ids=["5x7*3x2", "33x20*8x31", "100x60*9x9"])
def test_composed_oracle_is_the_2d_convolution(ash, bsh, bound_lin, bound_circ):
    a, b = C.images(*ash, 2, salt=0xA), C.images(*bsh, 2, salt=0xB)
    full = [_direct(a[i], b[i]) for i in range(2)]
    errs = {}
    for typ in C.TYPES:
        got = C.oracle_convolve_2d(typ, "linear", a, b)
        _, s0, l0 = C.axis_rule(typ, "linear", ash[0], bsh[0])
        _, s1, l1 = C.axis_rule(typ, "linear", ash[1], bsh[1])
        assert got.shape == (2, l0, l1)
        errs["linear " + typ] = max(T.normwise_err(got[i], full[i][s0:s0 + l0, s1:s1 + l1]) for i in range(2))
    P0, P1 = C.shape_rule("full", "circular", *ash, *bsh)[2:]
    got = C.oracle_convolve_2d("full", "circular", a, b)
    assert got.shape == (2, P0, P1)
    errs["circular"] = max(T.normwise_err(got[i], _fold(full[i], P0, P1)) for i in range(2))
    # a shared kernel is the same arithmetic: broadcasting b over the batch changes no word
    shared = C.oracle_convolve_2d("same", "linear", a, b[:1])
    assert T.mismatches(shared[0], C.oracle_convolve_2d("same", "linear", a[:1], b[:1])[0]) == 0
    bounds = {what: bound_circ if what == "circular" else bound_lin for what in errs}
    for what, err in errs.items():
        print(ash, bsh, what, "normwise error", err, "bound", bounds[what])
    for what, err in errs.items():
        assert err <= bounds[what], (ash, bsh, what, err)
