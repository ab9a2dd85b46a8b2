"""CPU-only checks of the batched overlap-add filter (hsfft_filter_shape, hsfft_filter_batched of
include/hsfft_gpu.h):
  * the symbols are exported, declared and bound, and the Python callables exist;
  * hsfft_filter_shape equals the restated rule over a grid of sizes, types and blocks, rejects
    what the rule rejects with a message, and its automatic block follows the formula;
  * every bad-argument case of hsfft_filter_batched is rejected with HSFFT_ERR_ARG and a message
    before any device is touched (so it is testable here), and batch == 0 returns 0;
  * the yardstick of test_gpu_filter.py -- the expectation composed in hsfft_filter_testlib from
    the reference's own fft_convolve per block -- is the linear convolution, as accurate as the
    reference's one-shot result, and with one block it is that result word for word.

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

import hsfft_filter_testlib as F
import hsfft_testlib as T

import hsfft

NAMES = ("hsfft_filter_shape", "hsfft_filter_batched")

GRID_N, GRID_M, GRID_BLOCK = (1, 2, 9, 100, 8128, 8129), (1, 2, 4, 33, 200), (0, 2, 8, 64, 4096)

# The library is loaded in a child process, as in test_conv2d_cpu.py (test_kernel_resources.py lets
# objcopy rewrite lib/libhsfft.so while later tests run).  x is 3 rows of 100 (2400 bytes), h has 7
# taps (56 bytes), so a full output is 3 x 106 doubles = 2544 bytes.
CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import hsfft
L = hsfft.lib()
X, H, O = 0x10000, 0x20000, 0x30000  # distinct non-NULL "device pointers" (never dereferenced)
def call(t=b"full", x=X, n=100, h=H, m=7, blk=0, o=O, b=3):
    return (t, x, n, h, m, blk, o, b)
bad = [("NULL x", call(x=None)), ("NULL h", call(h=None)), ("NULL out", call(o=None)), ("negative batch", call(b=-1)),
       ("unknown type", call(t=b"most")), ("n 0", call(n=0)), ("m 0", call(m=0)), ("m -1", call(m=-1)),
       ("clen above 2^30", call(n=1 << 30, m=2)),
       ("block not a power of two", call(blk=48)), ("block 1", call(m=1, blk=1)), ("block below m", call(blk=4)),
       ("negative block", call(blk=-8)), ("L below m - 1 with several blocks", call(m=7, blk=8)),
       ("out == x", call(o=X)), ("out == h", call(o=H)),
       ("out starts in x's last 8 bytes", call(o=X + 2400 - 8)),
       ("x starts in out's last 8 bytes", call(x=O + 2544 - 8)),
       ("out starts in h's last 8 bytes", call(o=H + 56 - 8)),
       ("h starts in out's last 8 bytes", call(h=O + 2544 - 8)),
       ("out overlaps x only at batch 3", call(o=X + 2 * 800))]
fine_at_one_row = call(o=X + 2 * 800, b=0)
zero = [call(b=0), call(b=0, o=X), fine_at_one_row]
out = {"exported": {n: hasattr(L, n) for n in ("hsfft_filter_shape", "hsfft_filter_batched")}}
out["bad"] = [(what, L.hsfft_filter_batched(*args), L.hsfft_last_error().decode()) for what, args in bad]
out["zero"] = [L.hsfft_filter_batched(*args) for args in zero]
v = [ctypes.c_int(-7) for _ in range(4)]
refs = [ctypes.byref(x) for x in v]
out["shape_bad"] = [(what, L.hsfft_filter_shape(*args, *refs), L.hsfft_last_error().decode()) for what, args in [
    ("block not a power of two", (b"full", 100, 7, 48)), ("block below m", (b"full", 100, 7, 4)),
    ("L below m - 1 with several blocks", (b"full", 100, 7, 8)), ("unknown type", (b"most", 100, 7, 0)),
    ("n 0", (b"full", 0, 7, 0)), ("n -5", (b"same", -5, 7, 0)), ("clen above 2^30", (b"full", 1 << 30, 2, 0))]]
out["shape_untouched"] = [x.value for x in v]
out["shape_null_type"] = (L.hsfft_filter_shape(None, 100, 7, 32, *refs), [x.value for x in v])
out["shape_null_results"] = L.hsfft_filter_shape(b"full", 100, 7, 32, None, None, None, None)
# L == m - 1 with several blocks is the edge that is still allowed
out["shape_edge"] = (L.hsfft_filter_shape(b"full", 100, 5, 8, *refs), [x.value for x in v])
grid = json.loads(sys.argv[2])
out["grid"] = []
for n in grid["n"]:
    for m in grid["m"]:
        for t in ("full", "same", "valid"):
            for blk in grid["block"]:
                rc = L.hsfft_filter_shape(t.encode(), n, m, blk, *refs)
                out["grid"].append(((t, n, m, blk), rc, [x.value for x in v] if rc == 0 else None,
                                    L.hsfft_last_error().decode()))
out["auto"] = {"%d,%d" % nm: list(hsfft.filter_shape("full", nm[0], nm[1], 0))
               for nm in [(1 << 29, 1), (40000, 33), (40000, 2000), (100, 7)]}
class Ptr:
    ptr = X
out["raised"] = {}
for what, fn in [("filter_batched", lambda: hsfft.filter_batched("full", Ptr, 100, Ptr, 7, 0, Ptr, 3)),
                 ("filter_shape", lambda: hsfft.filter_shape("most", 100, 7))]:
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
    grid = json.dumps({"n": GRID_N, "m": GRID_M, "block": GRID_BLOCK})
    res = subprocess.run([sys.executable, "-c", CHILD, T.PKG_DIR, grid], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def floor(child):
    """HSFFT_FILTER_BLOCK_MIN as the library applies it: the automatic block of a one-tap kernel on
    a row long enough not to cap it; the header states the same value"""
    F_ = child["auto"]["%d,%d" % (1 << 29, 1)][1]
    header = open(os.path.join(T.REPO, "include", "hsfft_gpu.h")).read()
    assert re.search(r"#define\s+HSFFT_FILTER_BLOCK_MIN\s+%d\b" % F_, header)
    assert F_ >= 2 and F_ & (F_ - 1) == 0
    return F_


def test_symbols_exported_and_declared(child):
    assert os.path.exists(hsfft.LIB_PATH)
    header = open(os.path.join(T.REPO, "include", "hsfft_gpu.h")).read()
    for name in NAMES:
        assert child["exported"][name], name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in hsfft.SIGNATURES, name
    for name in ("filter_shape", "filter_batched", "oaconvolve"):
        assert callable(getattr(hsfft, name, None)), name
    # the chunk rule the GPU test relies on, and the pin to the reference's fft_convolve, are documented
    assert re.search(r"HSFFT_FILTER_CHUNK_MB / \(P x 8 \+ \(P/2\+1\) x 16\)", header)
    assert re.search(r'fft_convolve\("full", "linear", u_s\[0\.\.L\), L, h, m', header)


def test_shape_matches_the_restated_rule(child, floor):
    assert len(child["grid"]) == len(GRID_N) * len(GRID_M) * 3 * len(GRID_BLOCK)
    accepted = 0
    for (t, n, m, blk), rc, got, msg in child["grid"]:
        want = F.shape_rule(t, n, m, blk, floor)
        if want is None:
            assert rc == hsfft.HSFFT_ERR_ARG and msg, (t, n, m, blk, rc, got)
        else:
            assert rc == 0 and tuple(got) == want, (t, n, m, blk, rc, got, want)
            accepted += 1
    assert accepted >= len(child["grid"]) // 2  # the grid is mostly valid calls, not mostly rejections
    grid = {tuple(k): (rc, v) for k, rc, v, _ in child["grid"]}
    # spot values, written out
    assert grid[("full", 9, 4, 8)] == (0, [12, 8, 5, 2])
    assert grid[("same", 100, 2, 2)] == (0, [100, 2, 1, 100])
    assert grid[("valid", 8128, 33, 4096)] == (0, [8096, 4096, 4064, 2])
    assert grid[("valid", 8129, 33, 4096)] == (0, [8097, 4096, 4064, 3])
    assert grid[("full", 100, 200, 64)][0] == hsfft.HSFFT_ERR_ARG   # block < m
    assert grid[("full", 100, 33, 64)] == (0, [132, 64, 32, 4])     # L = 32 = m - 1: still allowed
    assert grid[("full", 9, 33, 64)] == (0, [41, 64, 32, 1])


def test_shape_rejects_bad_arguments(child):
    for what, rc, msg in child["shape_bad"]:
        assert rc == hsfft.HSFFT_ERR_ARG, (what, rc)
        assert msg, what
    assert child["shape_untouched"] == [-7] * 4  # a rejected call writes no result
    assert child["shape_null_type"] == [0, [106, 32, 26, 4]]  # NULL type is "full"
    assert child["shape_null_results"] == 0
    assert child["shape_edge"] == [0, [104, 8, 4, 25]]  # L = 4 = m - 1


def test_automatic_block(child, floor):
    def auto(n, m):
        return tuple(child["auto"]["%d,%d" % (n, m)])

    for n, m in [(40000, 33), (40000, 2000), (100, 7)]:
        assert auto(n, m) == F.shape_rule("full", n, m, 0, floor), (n, m)
    P = max(floor, 256)
    assert auto(40000, 33)[1:] == (P, P - 32, -(-40000 // (P - 32)))
    P = max(floor, 8192)  # next_pow2(8000)
    assert auto(40000, 2000)[1:] == (P, P - 1999, -(-40000 // (P - 1999)))
    assert auto(100, 7) == (106, 128, 122, 1)  # capped at Q = next_pow2(106): one block


def test_bad_arguments_are_rejected(child):
    """HSFFT_ERR_ARG and a message for every bad-argument case, before any device is touched;
    batch == 0 returns 0"""
    assert len(child["bad"]) >= 20
    for what, rc, msg in child["bad"]:
        assert rc == hsfft.HSFFT_ERR_ARG, (what, rc, msg)
        assert msg, what
    assert child["zero"] == [0, 0, 0]


def test_bad_arguments_raise_in_python(child):
    assert set(child["raised"]) == {"filter_batched", "filter_shape"}
    assert "overlaps" in child["raised"]["filter_batched"]
    assert "output type" in child["raised"]["filter_shape"]


def test_oaconvolve_rejects_bad_shapes_before_loading_anything():
    z = np.zeros
    for x, h, kw in [(z((2, 3, 8)), z(3), {}), (z(8), z((2, 3)), {}), (z(8), z((1, 3)), {}), (z(0), z(3), {}), (z((2, 0)), z(3), {}), (z(8), z(0), {}), (z(8), z(3), {"mode": "most"}),
                     (z(8), z(3), {"block": 48}), (z(8), z(3), {"block": 2}), (z(8), z(3), {"block": -4}),
                     (z(8), z(1), {"block": 1})]:
        with pytest.raises(ValueError):
            hsfft.oaconvolve(x, h, **kw)
    assert hsfft.oaconvolve(z((0, 100)), z(7)).shape == (0, 106)
    assert hsfft.oaconvolve(z((0, 100)), z(7), mode="same").shape == (0, 100)
    assert hsfft.oaconvolve(z((0, 100)), z(7), mode="valid", block=64).shape == (0, 94)


# ---------------------------------------------------------------- the yardstick, pinned
def _direct(x, h):
    """linear convolution in long double, by the definition"""
    return np.convolve(x.astype(np.longdouble), h.astype(np.longdouble))


@pytest.mark.parametrize("n,m,P", F.CASES, ids=["%dx%d@%d" % c for c in F.CASES])
def test_composed_oracle_is_the_convolution(n, m, P):
    """The largest error of the overlap-added expectation against a long-double direct convolution
    is at most 2 x that of the reference's own one-shot fft_convolve on the same input: the
    yardstick is the reference's own error (shorter transforms round less, and an add per
    overlapped word costs half an ulp; the margin of 2 covers inputs other than these).  A block
    put in the wrong place or a missing overlap gives an error of the order of the data, 1e13
    times larger."""
    x, h = F.rows(n, 1, salt=0xF1)[0], F.kernel(m, salt=0xF1)
    assert F.shape_rule("full", n, m, P)[1] == P
    want = _direct(x, h)
    got = F.oracle_filter("full", x, h, P)
    one = T.oracle_convolve(b"full", b"linear", x, h)
    assert got.shape == one.shape == want.shape
    err = float(np.abs(got - want).max())
    ref = float(np.abs(one - want).max())
    print(n, m, P, "overlap-add error", err, "one-shot reference error", ref, "ratio", err / ref if ref else np.inf)
    assert err <= 2 * ref, (n, m, P, err, ref)


@pytest.mark.parametrize("typ", F.TYPES)
def test_one_block_is_the_reference_convolution(typ):
    """P == Q: one block, nothing to add; the expectation is the reference's one-shot result"""
    for n, m in [(9, 4), (1000, 33), (100, 7), (7, 100), (1, 2), (2, 1), (4064, 33)]:
        Q = max(2, F.next_pow2(n + m - 1))
        assert F.shape_rule(typ, n, m, Q)[2:] == (Q - m + 1, 1)
        x, h = F.rows(n, 1, salt=0xF2)[0], F.kernel(m, salt=0xF2)
        # the block is the row zero-extended to L = Q - m + 1 >= n samples: the reference pads both to Q anyway
        got = F.oracle_filter(typ, x, h, Q)
        want = T.oracle_convolve(typ.encode(), b"linear", x, h)
        assert got.shape == want.shape, (typ, n, m)
        assert T.mismatches(got, want) == 0, (typ, n, m)
