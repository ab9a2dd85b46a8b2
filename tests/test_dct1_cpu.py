"""CPU-only checks of the batched type-I cosine and sine transforms (hsfft_dct1_shape,
hsfft_dct1_batched, hsfft_dct1_2d_batched of include/hsfft_gpu.h):
  * the symbols are exported, declared and bound, and the Python callables exist;
  * every bad-argument case is rejected with HSFFT_ERR_ARG and a message before any device is
    touched (so it is testable here), from C and from Python, and batch == 0 returns 0;
  * hsfft_dct1_shape gives L = 2(n-1) or 2(n+1) and L/2+1, and rejects what the batched call rejects;
  * hsfft.dct(x, type=1) and its siblings still raise: type I has entry points of its own;
  * the yardstick of test_gpu_dct1.py -- hsfft_dct1_testlib's numpy extension around the reference's
    own r2c -- computes scipy's DCT-I and DST-I: against long-double direct sums on the lengths whose
    extension is a power of two, and bit for bit against the oracle alone elsewhere (the reference's
    radix-3 quirk and radix-5 accuracy put other lengths far from the definition for its r2c alone);
  * the two kernels are in the gfx950 code object in both forms and do not spill.

No call made here has valid arguments and a non-zero batch: nothing is ever launched, the
pointers are never dereferenced.
"""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import hsfft_dct1_testlib as D1
import hsfft_testlib as T
import test_kernel_resources as KR

import hsfft

NAMES = ("hsfft_dct1_shape", "hsfft_dct1_batched", "hsfft_dct1_2d_batched")
PY_NAMES = ("dct1_shape", "dct1_batched", "dct1_2d_batched", "dct1", "dst1", "idct1", "idst1", "dct1n", "dst1n", "idct1n", "idst1n")
HALF = 1 << 29  # the cosine takes n <= 2^29 + 1 and the sine n <= 2^29 - 1: L <= 2^30
SHAPE_CASES = ((0, 2), (0, 3), (0, 7), (0, 4097), (0, HALF + 1), (1, 1), (1, 2), (1, 15), (1, 4095), (1, HALF - 1))

# The library is loaded in a child process, as in test_dct_cpu.py.  The valid calls are 3 rows of
# 101 doubles (2424 bytes in and out) and 3 images of 5 x 7 (840 bytes).
CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import hsfft
L = hsfft.lib()
X, O = 0x100008, 0x300008  # distinct non-NULL "device pointers" (never dereferenced), 8-byte aligned only
HALF = 1 << 29
def err(rc):
    return (rc, L.hsfft_last_error().decode())
out = {"exported": {n: hasattr(L, n) for n in json.loads(sys.argv[2])}}
def row(kind=0, x=X, o=O, n=101, b=3):
    return err(L.hsfft_dct1_batched(kind, x, o, n, b))
def img(k0=0, k1=0, x=X, o=O, n0=5, n1=7, b=3):
    return err(L.hsfft_dct1_2d_batched(k0, k1, x, o, n0, n1, b))
out["rows"] = [(what,) + row(**kw) for what, kw in [
    ("kind 2", dict(kind=2)), ("kind -1", dict(kind=-1)),
    ("n 1 cosine", dict(n=1)), ("n 0 cosine", dict(n=0)), ("n 0 sine", dict(kind=1, n=0)), ("n -3 cosine", dict(n=-3)),
    ("n -3 sine", dict(kind=1, n=-3)), ("n above the cosine's limit", dict(n=HALF + 2)),
    ("n above the sine's limit", dict(kind=1, n=HALF)), ("n 2^31 - 1", dict(kind=1, n=2147483647)),
    ("negative batch", dict(b=-1)), ("rows above 2^40", dict(n=HALF + 1, b=2048)),
    ("NULL in", dict(x=None)), ("NULL out", dict(o=None)), ("in == out", dict(o=X)),
    ("out starts in the input's last 8 bytes", dict(o=X + 2424 - 8)),
    ("in starts in the output's last 8 bytes", dict(x=O + 2424 - 8)),
    ("out overlaps the input only at batch 3", dict(o=X + 2 * 808))]]
out["rows_ok"] = [row(b=0)[0], row(kind=1, b=0)[0], row(b=0, o=X)[0], row(b=0, n=HALF + 1)[0], row(kind=1, b=0, n=HALF - 1)[0],
                  row(kind=1, n=1, b=0)[0], row(n=2, b=0)[0], row(o=X + 2424, b=0)[0]]
out["images"] = [(what,) + img(**kw) for what, kw in [
    ("kind0 2", dict(k0=2)), ("kind1 -1", dict(k1=-1)),
    ("n0 1 cosine", dict(n0=1)), ("n1 1 cosine", dict(n1=1)), ("n0 0 sine", dict(k0=1, n0=0)), ("n1 0 sine", dict(k1=1, n1=0)),
    ("n0 above the cosine's limit", dict(n0=HALF + 2)), ("n1 above the sine's limit", dict(k1=1, n1=HALF)),
    ("negative batch", dict(b=-1)), ("images above 2^40", dict(n0=1 << 20, n1=1 << 20, b=2)),
    ("one image above 2^40", dict(n0=1 << 21, n1=1 << 20, b=1)),
    ("NULL in", dict(x=None)), ("NULL out", dict(o=None)), ("in == out", dict(o=X)),
    ("out starts in the input's last 8 bytes", dict(o=X + 840 - 8)),
    ("in starts in the output's last 8 bytes", dict(x=O + 840 - 8)),
    ("out overlaps the input only at batch 3", dict(o=X + 2 * 280))]]
out["images_ok"] = [img(b=0)[0], img(k0=1, k1=1, n0=1, n1=1, b=0)[0], img(k0=0, k1=1, n0=2, n1=1, b=0)[0], img(b=0, o=X)[0],
                    img(n0=HALF + 1, n1=2, b=0)[0]]
Lv, Bv = ctypes.c_int(-7), ctypes.c_int(-7)
out["bad_shape"] = [(what,) + err(L.hsfft_dct1_shape(kind, n, ctypes.byref(Lv), ctypes.byref(Bv)))
                    for what, kind, n in [("kind 2", 2, 8), ("kind -1", -1, 8), ("n 1 cosine", 0, 1), ("n 0 sine", 1, 0),
                                          ("n -3 cosine", 0, -3), ("n above the cosine's limit", 0, HALF + 2),
                                          ("n above the sine's limit", 1, HALF), ("n 2^31 - 1", 0, 2147483647)]]
out["shape_untouched"] = (Lv.value, Bv.value) == (-7, -7)
out["shape_null"] = [L.hsfft_dct1_shape(0, 9, None, None), L.hsfft_dct1_shape(1, 9, ctypes.byref(Lv), None), Lv.value]
out["shapes"] = []
for kind, n in json.loads(sys.argv[3]):
    rc = L.hsfft_dct1_shape(kind, n, ctypes.byref(Lv), ctypes.byref(Bv))
    out["shapes"].append((rc, Lv.value, Bv.value, list(hsfft.dct1_shape(kind, n))))
class Ptr:
    ptr = X
out["raised"] = {}
for what, fn in [("dct1_batched", lambda: hsfft.dct1_batched(0, Ptr, Ptr, 101, 3)),
                 ("dct1_batched length", lambda: hsfft.dct1_batched(0, Ptr, Ptr, 1, 3)),
                 ("dct1_2d_batched", lambda: hsfft.dct1_2d_batched(0, 1, Ptr, Ptr, 5, 7, 3)),
                 ("dct1_2d_batched kind", lambda: hsfft.dct1_2d_batched(0, 2, Ptr, Ptr, 5, 7, 3)),
                 ("dct1_shape", lambda: hsfft.dct1_shape(0, 1))]:
    try:
        fn()
        out["raised"][what] = None
    except hsfft.HsfftError as e:
        out["raised"][what] = str(e)
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def child():
    """what a fresh process saw: no call in it has valid arguments and a non-zero batch, so nothing
    is launched wherever it runs"""
    res = subprocess.run([sys.executable, "-c", CHILD, T.PKG_DIR, json.dumps(NAMES), json.dumps(SHAPE_CASES)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_symbols_exported_and_declared(child):
    assert os.path.exists(hsfft.LIB_PATH)
    header = open(os.path.join(T.REPO, "include", "hsfft_gpu.h")).read()
    for name in NAMES:
        assert child["exported"][name], name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in hsfft.SIGNATURES, name
    for name in PY_NAMES:
        assert callable(getattr(hsfft, name, None)), name
    # the chunk rules the GPU tests rely on, the twiddle-mode caveat and the alignment contract are documented
    assert re.search(r"HSFFT_DCT_CHUNK_MB / \(L x 8 \+ \(L/2\+1\) x 16\)\s+\*?\s*rows", header)
    assert re.search(r"HSFFT_2D_CHUNK_MB / \(16 x ceil\(n0 x n1 / 2\)\) images", header)
    block = header[header.index("batched type-I cosine and sine"):header.index("int hsfft_dct1_2d_batched")]
    assert "twiddle mode" in block and "quirk" in block and "alignment of a" in block and "2^30" in block


def _all_rejected(cases, count, who):
    assert len(cases) == count
    for what, rc, msg in cases:
        assert rc == hsfft.HSFFT_ERR_ARG and msg.startswith(who + ": "), (what, rc, msg)
        if what.startswith("kind"):
            assert "is not 0 (cosine) or 1 (sine)" in msg, (what, msg)
        elif what[0] == "n" and what[:3] != "neg":
            assert "is below" in msg and "above 2^30" in msg, (what, msg)
        elif what.startswith("NULL") or what == "negative batch":
            assert "NULL pointer or negative batch" in msg, (what, msg)
        elif "above 2^40" in what:
            assert "more than the call can index" in msg, (what, msg)
        else:
            assert "overlaps" in msg, (what, msg)


def test_bad_arguments_are_rejected(child):
    """HSFFT_ERR_ARG and the case's own message for every bad-argument case of both entry points, before
    any device is touched; batch == 0 returns 0 at every valid length, the limits included"""
    _all_rejected(child["rows"], 18, "hsfft_dct1_batched")
    _all_rejected(child["images"], 17, "hsfft_dct1_2d_batched")
    assert child["rows_ok"] == [0] * 8 and child["images_ok"] == [0] * 5


def test_shape_values(child):
    _all_rejected(child["bad_shape"], 8, "hsfft_dct1_shape")
    assert child["shape_untouched"] and child["shape_null"] == [0, 0, 20]
    for (kind, n), (rc, L, bins, bound) in zip(SHAPE_CASES, child["shapes"]):
        want = 2 * (n + 1) if kind else 2 * (n - 1)
        assert rc == 0 and L == want == D1.ext_len(kind, n) and bins == want // 2 + 1 and bound == [L, bins], (kind, n, L, bins)
        assert L % 2 == 0 and L <= D1.MAX_LEN
    by = dict(zip(SHAPE_CASES, child["shapes"]))
    assert by[(0, 2)][1:3] == [2, 2] and by[(1, 1)][1:3] == [4, 3] and by[(0, HALF + 1)][1] == by[(1, HALF - 1)][1] == 1 << 30


def test_bad_arguments_raise_in_python(child):
    r = child["raised"]
    assert set(r) == {"dct1_batched", "dct1_batched length", "dct1_2d_batched", "dct1_2d_batched kind", "dct1_shape"}
    assert "overlaps" in r["dct1_batched"] and "overlaps" in r["dct1_2d_batched"]
    assert "is below 2" in r["dct1_batched length"] and "is below 2" in r["dct1_shape"]
    assert "is not 0 (cosine) or 1 (sine)" in r["dct1_2d_batched kind"]


def test_conveniences_reject_bad_shapes_before_loading_anything():
    z = np.zeros
    for fn in (hsfft.dct1, hsfft.idct1):
        for x in (z((2, 3, 8)), z(()), z(1), z((3, 1)), z(0), z((2, 0))):
            with pytest.raises(ValueError):
                fn(x)
        assert fn(z((0, 7))).shape == (0, 7) and fn(z((0, 7))).dtype == np.float64
    for fn in (hsfft.dst1, hsfft.idst1):
        for x in (z((2, 3, 8)), z(()), z(0), z((2, 0))):
            with pytest.raises(ValueError):
                fn(x)
        assert fn(z((0, 1))).shape == (0, 1) and fn(z((0, 1))).dtype == np.float64
    for fn in (hsfft.dct1n, hsfft.idct1n):
        for x in (z(8), z(()), z((1, 8)), z((8, 1)), z((2, 8, 1)), z((0, 8)), z((3, 8, 0))):
            with pytest.raises(ValueError):
                fn(x)
        assert fn(z((0, 3, 5))).shape == (0, 3, 5)
    for fn in (hsfft.dst1n, hsfft.idst1n):
        for x in (z(8), z(()), z((0, 8)), z((3, 8, 0))):
            with pytest.raises(ValueError):
                fn(x)
        assert fn(z((0, 1, 1))).shape == (0, 1, 1)


def test_the_older_conveniences_still_reject_type_1():
    z = np.zeros
    for fn in (hsfft.dct, hsfft.dst, hsfft.idct, hsfft.idst):
        with pytest.raises(ValueError):
            fn(z(64), type=1)
    for fn in (hsfft.dctn, hsfft.dstn, hsfft.idctn, hsfft.idstn):
        with pytest.raises(ValueError):
            fn(z((8, 8)), type=1)


# ---------------------------------------------------------------- the yardstick, pinned
NAME_OF = {D1.COS: "DCT-I", D1.SIN: "DST-I"}


@pytest.mark.parametrize("kind", [D1.COS, D1.SIN], ids=["DCT-I", "DST-I"])
def test_expectation_is_scipys_transform(kind):
    """the composed expectation against a long-double direct sum of scipy's definition (norm=None),
    the angle reduced exactly by integers mod L, on the lengths whose extension is a power of two --
    n = 2^p + 1 (cosine) and 2^p - 1 (sine) for p = 1..12 -- on a uniform [-1, 1) row: the normwise
    error is within the suite's bound of 4.  Measured on the oracle alone: worst 1.62 (cosine) and 1.40
    (sine).  This also pins the sign of the sine output, -Im S[k+1]: a wrong index or sign gives an
    error of the order of the data, 1e15 in these units."""
    worst = 0.0
    for p in range(1, 13):
        n = (1 << p) - 1 if kind == D1.SIN else (1 << p) + 1
        x = D1.rows(n, 1, salt=0xB0 + kind)
        err = T.normwise_err(D1.oracle(kind, x)[0].astype(np.longdouble), D1.direct(kind, x[0]))
        print(NAME_OF[kind], "n", n, "normwise error", err)
        worst = max(worst, err)
        assert err <= 4, (kind, n, err)
    print(NAME_OF[kind], "largest", worst)


@pytest.mark.parametrize("kind,n", [(D1.COS, 7), (D1.COS, 10), (D1.COS, 100), (D1.SIN, 5), (D1.SIN, 11), (D1.SIN, 101)])
def test_other_lengths_carry_the_references_quirk(kind, n):
    """extended lengths 12, 18, 198, 12, 24 and 204, whose inner complex transforms have lengths 6, 9,
    99, 6, 12 and 102: in the default twiddle mode the reference's r2c of such lengths is far from the
    DFT (absolute errors of 0.7 to 14 on rows in [-1, 1) were measured here), so the expectation is held to the oracle's words alone: it is the named component of the
    oracle's r2c of the extension, restated here without the testlib's helpers.  In the exact mode the
    same composition meets the definition to about 1e-10."""
    x = D1.rows(n, 2, salt=0xB4)
    L = D1.ext_len(kind, n)
    e = np.zeros((2, L))
    for b in range(2):
        for j in range(n):
            if kind == D1.SIN:
                e[b, j + 1], e[b, L - 1 - j] = x[b, j], -x[b, j]
            else:
                e[b, j] = x[b, j]
                e[b, (L - j) % L] = x[b, j]
    Sp = T.oracle_r2c(e)
    want = -Sp.imag[:, 1:n + 1] if kind == D1.SIN else Sp.real[:, :n]
    assert T.mismatches(D1.oracle(kind, x), np.ascontiguousarray(want)) == 0
    exact = D1.oracle(kind, x, flags=T.ORC_EXACT)[0]
    off = float(np.abs(D1.oracle(kind, x)[0] - D1.direct(kind, x[0])).max())
    print(NAME_OF[kind], "n", n, "L", L, "default mode off the definition by", off, "exact mode by",
          float(np.abs(exact - D1.direct(kind, x[0])).max()))
    assert float(np.abs(exact - D1.direct(kind, x[0])).max()) < 1e-8


@pytest.mark.parametrize("kind,n", [(D1.COS, 65), (D1.COS, 257), (D1.COS, 4097), (D1.SIN, 63), (D1.SIN, 255), (D1.SIN, 4095)])
def test_round_trip_is_as_accurate_as_the_reference(kind, n):
    """T(T(x)) / factor against x: within 4 x the error of the reference's own r2c -> c2r -> / L round
    trip on the extended row (the margin of test_dct_cpu.py: two forward transforms stand against one
    forward and one inverse of the same length).  Measured on the oracle alone: ratios 0.67 to 1.0."""
    _, err, ref = D1.round_trip_errors(kind, n)
    print(NAME_OF[kind], "n", n, "round trip error", err, "reference r2c -> c2r round trip error", ref, "ratio",
          err / ref if ref else np.inf)
    assert ref > 0
    assert err <= 4 * ref, (kind, n, err, ref)


@pytest.mark.parametrize("n", [1, 2, 5, 63, 100])
def test_sine_transform_is_r2c_of_the_odd_extension(n):
    """the sine form restated with np.copysign instead of np.negative: the extension's mirrored half
    has the sign bit of every word flipped, signed zeros and NaN included, and its two fixed words are
    +0.0"""
    x = D1.rows(n, 3, salt=0xB9)
    flipped = lambda a: np.copysign(a, np.where(np.signbit(a), 1.0, -1.0))
    e = D1.extend(D1.SIN, x)
    L = 2 * (n + 1)
    assert e.shape == (3, L) and T.zero_words(e[:, [0, n + 1]]) == 6 and not np.signbit(e[:, [0, n + 1]]).any()
    assert T.mismatches(e[:, 1:n + 1], x) == 0 and T.mismatches(np.ascontiguousarray(e[:, :n + 1:-1]), flipped(x)) == 0
    Sp = T.oracle_r2c(e)
    assert T.mismatches(D1.oracle(D1.SIN, x), np.ascontiguousarray(flipped(Sp.imag[:, 1:n + 1]))) == 0
    z = np.array([[0.0, -0.0, np.nan, -np.nan, 1.0]])
    ez = D1.extend(D1.SIN, z)
    assert list(np.signbit(ez[0])) == [False, False, True, False, True, False, False, True, False, True, False, True]
    assert np.isnan(ez[0, [3, 4, 8, 9]]).all()
    ec = D1.extend(D1.COS, z)  # the even extension copies: L = 8, the two ends have no mirror
    assert ec.shape == (1, 8) and T.mismatches(ec[:, 5:], np.ascontiguousarray(z[:, 3:0:-1])) == 0 and T.mismatches(ec[:, :5], z) == 0


def test_the_two_kernels_exist_and_do_not_spill(tmp_path, monkeypatch):
    """test_kernel_resources._metadata() on a copy of the library, as in test_spectral_cpu.py: its
    objcopy step, given no output name, writes its input file anew, and this process may have the
    library mapped by now"""
    if not os.path.exists(KR.LIB):
        pytest.skip("lib/libhsfft.so not built")
    copy = str(tmp_path / "libhsfft_copy.so")
    shutil.copyfile(KR.LIB, copy)
    monkeypatch.setattr(KR, "LIB", copy)
    kernels = KR._metadata()
    for name in ("k_dct1_pre", "k_dct1_post"):
        hits = {k: v for k, v in kernels.items() if re.match(r"^_ZN4dct1%d%sILb[01]EEE" % (len(name), name), k)}
        assert len(hits) == 2, (name, sorted(hits))  # the cosine and the sine form
        for k, res in hits.items():
            assert res.get("vgpr_spill_count", 0) == 0 and res.get("sgpr_spill_count", 0) == 0, (k, res)
