"""CPU-only checks of the 2D / column / transpose entry points (include/hsfft_gpu.h):
  * the three symbols are exported and declared;
  * every bad-argument case is rejected with HSFFT_ERR_ARG and a message before any device is
    touched (so it is testable here), and batch == 0 returns 0;
  * the yardstick of test_gpu_2d.py -- the 2D expectation composed from the 1D oracle -- is the
    2D DFT: checked against numpy.fft.fft2.

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

import hsfft_2d_testlib as D
import hsfft_testlib as T

import hsfft

NAMES = ("hsfft_transpose_batched", "hsfft_exec_2d", "hsfft_exec_columns")

# The library is loaded in a child process, not in the test process: test_kernel_resources.py,
# which runs after this file, lets objcopy rewrite lib/libhsfft.so, and a process that has the
# file mapped at that moment does not survive it.  The child makes every call and prints what it
# saw; the tests below assert on that.
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import hsfft
L = hsfft.lib()
A, B = 0x10000, 0x20000  # two distinct non-NULL "device pointers" (never dereferenced)
p0, p1 = hsfft.Plan(8, 1), hsfft.Plan(6, -1)
bad = {
    "hsfft_transpose_batched": [("NULL in", (None, B, 4, 4, 1)), ("NULL out", (A, None, 4, 4, 1)),
        ("in == out", (A, A, 4, 4, 1)), ("negative batch", (A, B, 4, 4, -1)), ("rows 0", (A, B, 0, 4, 1)),
        ("cols 0", (A, B, 4, 0, 1)), ("rows < 0", (A, B, -3, 4, 1)), ("cols < 0", (A, B, 4, -3, 1)),
        ("overlapping ranges", (A, A + 16, 4, 4, 1))],
    "hsfft_exec_2d": [("NULL p0", (None, p1.ptr, A, B, 1)), ("NULL p1", (p0.ptr, None, A, B, 1)),
        ("NULL in", (p0.ptr, p1.ptr, None, B, 1)), ("NULL out", (p0.ptr, p1.ptr, A, None, 1)),
        ("in == out", (p0.ptr, p1.ptr, A, A, 1)), ("negative batch", (p0.ptr, p1.ptr, A, B, -1))],
    "hsfft_exec_columns": [("NULL plan", (None, A, B, 5, 1)), ("NULL in", (p0.ptr, None, B, 5, 1)),
        ("NULL out", (p0.ptr, A, None, 5, 1)), ("in == out", (p0.ptr, A, A, 5, 1)),
        ("negative batch", (p0.ptr, A, B, 5, -1)), ("ncols 0", (p0.ptr, A, B, 0, 1)),
        ("ncols < 0", (p0.ptr, A, B, -5, 1))],
}
zero = {"hsfft_transpose_batched": [(A, B, 4, 4, 0)], "hsfft_exec_2d": [(p0.ptr, p1.ptr, A, B, 0), (p0.ptr, p0.ptr, A, B, 0)],
        "hsfft_exec_columns": [(p0.ptr, A, B, 5, 0)]}
out = {"exported": {n: hasattr(L, n) for n in bad}, "bad": {}, "zero": {}, "raised": {}}
for name, cases in bad.items():
    out["bad"][name] = [(what, getattr(L, name)(*args), L.hsfft_last_error().decode()) for what, args in cases]
    out["zero"][name] = [getattr(L, name)(*args) for args in zero[name]]
class Ptr:
    ptr = A
for what, call in [("transpose_batched", lambda: hsfft.transpose_batched(Ptr, Ptr, 1, 1, 1)),
                   ("exec_2d", lambda: hsfft.exec_2d(p0, p0, Ptr, Ptr, 1)),
                   ("exec_columns", lambda: hsfft.exec_columns(p0, Ptr, Ptr, 3, 1))]:
    try:
        call()
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
    for name in ("transpose_batched", "exec_2d", "exec_columns", "fft2"):
        assert callable(getattr(hsfft, name, None)), name


@pytest.mark.parametrize("name", NAMES)
def test_bad_arguments_are_rejected(child, name):
    """HSFFT_ERR_ARG and a message for every bad-argument case, before any device is touched;
    batch == 0 returns 0"""
    assert len(child["bad"][name]) >= 6
    for what, rc, msg in child["bad"][name]:
        assert rc == hsfft.HSFFT_ERR_ARG, (name, what, rc)
        assert msg, (name, what)
    assert child["zero"][name] and all(rc == 0 for rc in child["zero"][name]), child["zero"][name]


def test_bad_arguments_raise_in_python(child):
    """the binding turns the error code into HsfftError with the library's message"""
    for what, msg in child["raised"].items():
        assert msg and "invalid arguments" in msg, (what, msg)


# The composed expectation against numpy.  The oracle is the reference, defects included: as it is
# (flags 0, what every GPU comparison uses) a length with a radix-3 stage is not a DFT at all
# (6 and 60 here; measured 3e15 eps), so 8x6 and 100x60 use the oracle's
# exact-twiddle flavour, whose error is that of the reference's butterfly constants; 97x64
# (Bluestein x radix 8) is compared as it is.  Bounds: measured here from the oracle, x 4.  An
# axis mix-up in the builder gives O(1) relative error, 1e15 in these units.
YARDSTICK = [
    ((8, 6), T.ORC_EXACT, 4 * 1.54e4),     # measured 15309.1 (sgn 1), 15309.0 (sgn -1); rows alone 16860
    ((100, 60), T.ORC_EXACT, 4 * 7.8e4),   # measured 75153.7, 77786.9; rows alone 44463
    ((97, 64), 0, 4 * 3.8),                # measured 3.41, 3.70; rows alone 1.34
]


@pytest.mark.parametrize("shape,flags,bound", YARDSTICK, ids=["8x6", "100x60", "97x64"])
def test_composed_oracle_is_the_2d_dft(shape, flags, bound):
    n0, n1 = shape
    x = D.images(n0, n1, 2)
    for sgn in (1, -1):
        y = D.oracle_2d(x, sgn, sgn, flags)
        ref = np.fft.fft2(x) if sgn == 1 else np.fft.ifft2(x) * (n0 * n1)
        err = max(T.normwise_err(y[b], ref[b]) for b in range(2))
        print(shape, sgn, "normwise error", err, "bound", bound)
        assert err <= bound, (shape, sgn, err)
    # mixed signs: forward rows, inverse columns
    y = D.oracle_2d(x, -1, 1, flags)
    ref = np.fft.ifft(np.fft.fft(x, axis=2), axis=1) * n0
    assert max(T.normwise_err(y[b], ref[b]) for b in range(2)) <= bound
    # the columns alone
    y = D.oracle_columns(x, 1, flags)
    assert max(T.normwise_err(y[b], np.fft.fft(x, axis=1)[b]) for b in range(2)) <= bound
