"""CPU-only checks of the batched 2D cosine and sine transforms and the transpose of 8-byte elements
(hsfft_dct_2d_batched, hsfft_transpose_real_batched of include/hsfft_gpu.h):
  * the symbols are exported, declared and bound, the Python callables exist and the chunk rule is
    in the header;
  * every bad-argument case of both entry points is rejected with HSFFT_ERR_ARG and a message
    before any device is touched (so it is testable here), and batch == 0 returns 0;
  * the Python conveniences reject bad shapes before the library is loaded;
  * the yardstick of test_gpu_dct2d.py -- hsfft_dct2d_testlib.oracle_2d, the 1D expectation on the
    rows and then on the columns -- computes scipy's transforms (long-double separable direct sums)
    and inverts itself as accurately as two axes of the reference's own round trip allow;
  * the new kernel is in the gfx950 code object, in one tile size, and does not spill.

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

import hsfft_dct2d_testlib as D2
import hsfft_dct_testlib as D
import hsfft_testlib as T
import test_kernel_resources as KR

import hsfft

NAMES = ("hsfft_transpose_real_batched", "hsfft_dct_2d_batched")

# The library is loaded in a child process, as in test_dct_cpu.py.  The valid calls are 3 images of
# 10 x 8 doubles: 640 bytes per image, 1920 bytes in and out.
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import hsfft
out = {"early": {}}
z = np.zeros
for name in ("dctn", "dstn", "idctn", "idstn"):
    fn, n = getattr(hsfft, name), 0
    for x, kw in [(z(64), {}), (z(()), {}), (z((7, 8)), {}), (z((8, 7)), {}), (z((3, 1, 8)), {}), (z((3, 8, 0)), {}),
                  (z((0, 8)), {}), (z((8, 8)), {"type": 1}), (z((8, 8)), {"type": 4})]:
        try:
            fn(x, **kw)
        except ValueError:
            n += 1
    out["early"][name] = [n, fn(z((0, 8, 6))).shape, str(fn(z((0, 8, 6)), type=3).dtype)]
out["loaded_by_conveniences"] = hsfft._lib is not None
L = hsfft.lib()
X, O = 0x100000, 0x300000  # distinct non-NULL "device pointers" (never dereferenced)
def call(k0=0, k1=0, type=2, x=X, o=O, n0=10, n1=8, b=3):
    return (k0, k1, type, x, o, n0, n1, b)
BIG = 1 << 30
COMBOS = [(k0, k1, t) for k0 in (0, 1) for k1 in (0, 1) for t in (2, 3)]
bad_kt = [("kind0 2", call(k0=2)), ("kind0 -1", call(k0=-1)), ("kind1 2", call(k1=2)), ("kind1 -1", call(k1=-1)),
          ("type 1", call(type=1)), ("type 4", call(type=4)), ("type 0", call(type=0))]
bad = [("n0 odd", call(n0=11)), ("n0 1", call(n0=1)), ("n0 0", call(n0=0)), ("n0 -2", call(n0=-2)),
       ("n0 above 2^30", call(n0=BIG + 2)),
       ("n1 odd", call(n1=9)), ("n1 1", call(n1=1)), ("n1 0", call(n1=0)), ("n1 -2", call(n1=-2)),
       ("n1 above 2^30", call(n1=BIG + 2)), ("negative batch", call(b=-1)),
       ("n0 x n1 x batch above 2^40", call(n0=BIG, n1=1 << 10, b=2)),
       ("n0 x n1 above 2^40", call(n0=BIG, n1=BIG, b=1)),
       ("NULL in", call(x=None)), ("NULL out", call(o=None)), ("in == out", call(o=X)),
       ("out starts in the input's last 8 bytes", call(o=X + 1920 - 8)),
       ("in starts in the output's last 8 bytes", call(x=O + 1920 - 8)),
       ("out overlaps the input only at batch 3", call(o=X + 2 * 640))]
f = L.hsfft_dct_2d_batched
out["bad"] = [(what, [f(*a)], L.hsfft_last_error().decode()) for what, a in bad_kt]
out["bad"] += [(what, [f(*c, *a[3:]) for c in COMBOS], L.hsfft_last_error().decode()) for what, a in bad]
out["zero"] = [f(*call(k0=c[0], k1=c[1], type=c[2], b=0)) for c in COMBOS]
out["zero"].append(f(*call(b=0, n0=BIG, n1=BIG)))
out["ok_message"] = L.hsfft_last_error().decode()
def tcall(x=X, o=O, rows=10, cols=8, b=3):
    return (x, o, rows, cols, b)
tbad = [("NULL in", tcall(x=None)), ("NULL out", tcall(o=None)), ("in == out", tcall(o=X)),
        ("negative batch", tcall(b=-1)), ("rows 0", tcall(rows=0)), ("rows -1", tcall(rows=-1)),
        ("cols 0", tcall(cols=0)), ("cols -1", tcall(cols=-1)),
        ("out starts in the input's last 8 bytes", tcall(o=X + 1920 - 8)),
        ("in starts in the output's last 8 bytes", tcall(x=O + 1920 - 8)),
        ("out overlaps the input only at batch 3", tcall(o=X + 2 * 640))]
g = L.hsfft_transpose_real_batched
out["tbad"] = [(what, g(*a), L.hsfft_last_error().decode()) for what, a in tbad]
out["tzero"] = [g(*tcall(b=0)), g(*tcall(b=0, rows=1, cols=1))]
class Ptr:
    ptr = X
out["raised"] = {}
for what, fn in [("dct_2d_batched", lambda: hsfft.dct_2d_batched(0, 1, 2, Ptr, Ptr, 10, 8, 3)),
                 ("transpose_real_batched", lambda: hsfft.transpose_real_batched(Ptr, Ptr, 10, 8, 3))]:
    try:
        fn()
        out["raised"][what] = None
    except hsfft.HsfftError as e:
        out["raised"][what] = str(e)
out["exported"] = {n: hasattr(L, n) for n in ("hsfft_transpose_real_batched", "hsfft_dct_2d_batched")}
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def child():
    """what a fresh process saw: no call in it has valid arguments and a non-zero batch, so nothing
    is launched wherever it runs"""
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
    assert len(hsfft.SIGNATURES["hsfft_transpose_real_batched"][1]) == 5
    assert len(hsfft.SIGNATURES["hsfft_dct_2d_batched"][1]) == 8
    for name in ("transpose_real_batched", "dct_2d_batched", "dctn", "dstn", "idctn", "idstn"):
        assert callable(getattr(hsfft, name, None)), name
    # the chunk rule the GPU test relies on
    assert "HSFFT_2D_CHUNK_MB / (n0 x n1 x 8) images" in header


def test_bad_arguments_of_the_2d_transform_are_rejected(child):
    """HSFFT_ERR_ARG and a message for every bad-argument case, the shape and pointer cases with all
    eight (kind0, kind1, type), before any device is touched; batch == 0 returns 0"""
    assert len(child["bad"]) == 7 + 19
    for what, rcs, msg in child["bad"]:
        assert rcs == [hsfft.HSFFT_ERR_ARG] * len(rcs) and len(rcs) in (1, 8), (what, rcs, msg)
        assert msg, what
    assert child["zero"] == [0] * 9
    assert child["ok_message"] == ""


def test_bad_arguments_of_the_transpose_are_rejected(child):
    assert len(child["tbad"]) == 11
    for what, rc, msg in child["tbad"]:
        assert rc == hsfft.HSFFT_ERR_ARG and msg, (what, rc, msg)
    assert child["tzero"] == [0, 0]


def test_bad_arguments_raise_in_python(child):
    assert set(child["raised"]) == {"dct_2d_batched", "transpose_real_batched"}
    assert "overlaps" in child["raised"]["dct_2d_batched"]
    assert "invalid arguments" in child["raised"]["transpose_real_batched"]


def test_conveniences_reject_bad_shapes_before_loading_the_library(child):
    """fewer than two dimensions, an odd or too-short axis, a bad type: ValueError in a process that
    has not loaded the library, and it is still not loaded afterwards; an empty batch comes back
    empty"""
    assert child["loaded_by_conveniences"] is False
    for name in ("dctn", "dstn", "idctn", "idstn"):
        raised, shape, dtype = child["early"][name]
        assert raised == 9 and shape == [0, 8, 6] and dtype == "float64", (name, child["early"][name])
    for fn in (hsfft.dctn, hsfft.dstn, hsfft.idctn, hsfft.idstn):
        with pytest.raises(ValueError):
            fn(np.zeros(64))
        with pytest.raises(ValueError):
            fn(np.zeros((2, 6, 7)))


# ---------------------------------------------------------------- the yardstick, pinned
SHAPES = [(2, 2), (2, 8), (8, 2), (4, 16), (8, 8), (16, 4), (32, 32), (64, 16), (16, 128), (128, 128)]


@pytest.mark.parametrize("combo", D2.COMBOS, ids=D2.combo_id)
def test_expectation_is_scipys_transform(combo):
    """oracle_2d against the long-double separable direct sum of scipy's definitions on uniform
    [-1, 1) images, by the Frobenius-norm relative error: within 8 eps, twice the 1D file's bound of
    4, one share per axis -- each axis transform is orthogonal up to scale and first-order errors
    add.  Powers of two only, as in the 1D file: the reference's twiddles at other radices are good
    to about 1e-11, which is its accuracy and not the composition's.  A swapped axis, kind or index
    gives an error of the order of the data, 1e15 in these units."""
    kind0, kind1, type = combo
    worst = 0.0
    for n0, n1 in SHAPES:
        x = D2.images(n0, n1, 1, salt=0xB0 + 8 * kind0 + 4 * kind1 + type)
        got, want = D2.oracle_2d(kind0, kind1, type, x)[0], D2.direct_2d(kind0, kind1, type, x[0])
        err = D2.frobenius_err(got, want)
        print(D2.combo_id(combo), (n0, n1), "Frobenius error in eps", err)
        worst = max(worst, err)
        assert err <= 8, (combo, n0, n1, err)
    print(D2.combo_id(combo), "largest", worst)


def test_mixed_kinds_are_told_apart():
    """(COS, SIN) and (SIN, COS) differ on a non-square image, so a swap of kind0 and kind1 shows"""
    x = D2.images(4, 16, 1, salt=0xB8)
    for type in (2, 3):
        assert T.mismatches(D2.oracle_2d(D.COS, D.SIN, type, x), D2.oracle_2d(D.SIN, D.COS, type, x)) > 0


@pytest.mark.parametrize("kinds", D2.KIND_PAIRS, ids=["cos_cos", "cos_sin", "sin_cos", "sin_sin"])
def test_round_trip_is_as_accurate_as_the_reference(kinds):
    """type 3 of type 2 of a 32 x 64 image, / 4 n0 n1, against the image: within 8 x the error of the
    reference's own 1D r2c -> c2r -> / N round trip at N = 64 (the 1D file's 4 x, for two axes)"""
    _, _, ref = D.round_trip_errors(64)
    err = D2.round_trip_error(kinds[0], kinds[1], 32, 64)
    print(kinds, "round trip error", err, "reference 1D round trip error", ref, "ratio", err / ref if ref else np.inf)
    assert ref > 0
    assert err <= 8 * ref, (kinds, err, ref)


def test_the_kernel_exists_and_does_not_spill():
    kernels = KR._metadata()
    hits = {k: v for k, v in kernels.items() if re.match(r"^_ZN4tr2d12k_transpose8ILi\d+EEE", k)}
    assert len(hits) == 1, sorted(hits)  # one tile size in the product
    for k, res in hits.items():
        assert re.match(r"^_ZN4tr2d12k_transpose8ILi64EEE", k), k
        assert res.get("vgpr_spill_count", 0) == 0, (k, res)
        assert 0 < res.get("vgpr_count", 0) <= 64, (k, res)  # 16 doubles in flight per lane: 8 waves per SIMD fit
