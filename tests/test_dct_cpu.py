"""CPU-only checks of the batched cosine and sine transforms (hsfft_dct_twiddles, hsfft_dct_batched of
include/hsfft_gpu.h):
  * the symbols are exported, declared and bound, and the Python callables exist;
  * hsfft_dct_twiddles equals the test library's libm table bit for bit;
  * every bad-argument case is rejected with HSFFT_ERR_ARG and a message before any device is
    touched (so it is testable here), and batch == 0 returns 0;
  * the Python conveniences reject bad shapes before loading anything;
  * the yardstick of test_gpu_dct.py -- the expectation composed in hsfft_dct_testlib from the
    reference's own r2c / c2r -- computes scipy's four transforms (long-double direct sums),
    inverts itself as accurately as the reference's own r2c -> c2r round trip, and satisfies the
    identities that tie the sine transforms to the cosine ones;
  * the four kernels are in the gfx950 code object and do not spill.

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

import hsfft_dct_testlib as D
import hsfft_testlib as T
import test_kernel_resources as KR

import hsfft

NAMES = ("hsfft_dct_twiddles", "hsfft_dct_batched")
TABLE_LENGTHS = (2, 6, 100, 4096, 12600, 65536)

# The library is loaded in a child process, as in test_stft_cpu.py.  The valid call is 3 rows of
# 100 doubles: 2400 bytes in and out.
CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import hsfft
L = hsfft.lib()
X, O = 0x100000, 0x300000  # distinct non-NULL "device pointers" (never dereferenced)
def call(kind=0, type=2, x=X, o=O, n=100, b=3):
    return (kind, type, x, o, n, b)
BIG = 1 << 30
bad = [("kind 2", call(kind=2)), ("kind -1", call(kind=-1)), ("type 1", call(type=1)), ("type 4", call(type=4)),
       ("type 0", call(type=0)), ("n odd", call(n=101)), ("n 1", call(n=1)), ("n 0", call(n=0)), ("n -2", call(n=-2)),
       ("n above 2^30", call(n=BIG + 2)), ("negative batch", call(b=-1)),
       ("n x batch above 2^40", call(n=BIG, b=1025)),
       ("NULL in", call(x=None)), ("NULL out", call(o=None)), ("in == out", call(o=X)),
       ("out starts in the input's last 8 bytes", call(o=X + 2400 - 8)),
       ("in starts in the output's last 8 bytes", call(x=O + 2400 - 8)),
       ("out overlaps the input only at batch 3", call(o=X + 2 * 800))]
out = {"exported": {n: hasattr(L, n) for n in ("hsfft_dct_twiddles", "hsfft_dct_batched")}}
out["bad"] = [(what, [L.hsfft_dct_batched(*call(kind=kd, type=tp)[:2], *a[2:]) if what[:4] not in ("kind", "type")
                      else L.hsfft_dct_batched(*a) for kd in (0, 1) for tp in (2, 3)],
               L.hsfft_last_error().decode()) for what, a in bad]
out["zero"] = [L.hsfft_dct_batched(*call(kind=kd, type=tp, b=0)) for kd in (0, 1) for tp in (2, 3)]
out["zero"].append(L.hsfft_dct_batched(*call(b=0, n=BIG)))
t = np.zeros(4, dtype=np.complex128)
out["bad_tw"] = [(what, L.hsfft_dct_twiddles(n, p), L.hsfft_last_error().decode())
                 for what, n, p in [("n odd", 7, t.ctypes.data), ("n 0", 0, t.ctypes.data), ("n 1", 1, t.ctypes.data),
                                    ("n -4", -4, t.ctypes.data), ("n above 2^30", BIG + 2, t.ctypes.data),
                                    ("NULL table", 6, None)]]
out["tw_untouched"] = bool((t == 0).all())
class Ptr:
    ptr = X
out["raised"] = {}
for what, fn in [("dct_batched", lambda: hsfft.dct_batched(0, 2, Ptr, Ptr, 100, 3)),
                 ("dct_twiddles", lambda: hsfft.dct_twiddles(7))]:
    try:
        fn()
        out["raised"][what] = None
    except hsfft.HsfftError as e:
        out["raised"][what] = str(e)
for n in json.loads(sys.argv[2]):
    hsfft.dct_twiddles(n).view(np.float64).tofile(sys.argv[3] + ".%d" % n)
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """what a fresh process saw: no call in it has valid arguments and a non-zero batch, so nothing
    is launched wherever it runs; the tables it wrote come back as arrays"""
    base = str(tmp_path_factory.mktemp("dct") / "table")
    res = subprocess.run([sys.executable, "-c", CHILD, T.PKG_DIR, json.dumps(TABLE_LENGTHS), base], capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    out["tables"] = {n: np.fromfile(base + ".%d" % n, dtype=np.complex128) for n in TABLE_LENGTHS}
    return out


def test_symbols_exported_and_declared(child):
    assert os.path.exists(hsfft.LIB_PATH)
    header = open(os.path.join(T.REPO, "include", "hsfft_gpu.h")).read()
    for name in NAMES:
        assert child["exported"][name], name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in hsfft.SIGNATURES, name
    for name in ("dct_twiddles", "dct_batched", "dct", "dst", "idct", "idst"):
        assert callable(getattr(hsfft, name, None)), name
    assert re.search(r"#define\s+HSFFT_KIND_COS\s+0\b", header) and re.search(r"#define\s+HSFFT_KIND_SIN\s+1\b", header)
    assert (hsfft.KIND_COS, hsfft.KIND_SIN) == (D.COS, D.SIN) == (0, 1)
    # the chunk rule the GPU test relies on and the knob's place in the scratch comment are documented
    assert re.search(r"HSFFT_DCT_CHUNK_MB / \(N x 8 \+ \(N/2\+1\) x 16\) rows", header)
    scratch_comment = header[header.index("Frees the library's scratch pool"):header.index("int hsfft_release_scratch")]
    assert "HSFFT_DCT_CHUNK_MB" in scratch_comment
    assert "real plan needs an even" in header  # odd lengths are out of scope, and the header says why


@pytest.mark.parametrize("n", TABLE_LENGTHS)
def test_twiddles_are_libm_sincos_bit_for_bit(child, n):
    got, want = child["tables"][n], D.table(n)
    assert got.shape == want.shape == (n // 2 + 1,)
    assert T.mismatches(got, want) == 0, (n, T.first_diff(got, want))
    assert got[0] == 1.0 + 0.0j  # k = 0: (cos 0, sin 0)
    assert abs(got[-1].real - got[-1].imag) < 1e-15 and abs(got[-1].real - np.sqrt(0.5)) < 1e-15  # k = n/2: pi / 4


def test_bad_arguments_are_rejected(child):
    """HSFFT_ERR_ARG and a message for every bad-argument case with every (kind, type), before any
    device is touched; batch == 0 returns 0"""
    assert len(child["bad"]) == 18
    for what, rcs, msg in child["bad"]:
        assert rcs == [hsfft.HSFFT_ERR_ARG] * 4, (what, rcs, msg)
        assert msg, what
    assert child["zero"] == [0] * 5
    for what, rc, msg in child["bad_tw"]:
        assert rc == hsfft.HSFFT_ERR_ARG and msg, (what, rc, msg)
    assert len(child["bad_tw"]) == 6 and child["tw_untouched"]


def test_bad_arguments_raise_in_python(child):
    assert set(child["raised"]) == {"dct_batched", "dct_twiddles"}
    assert "overlaps" in child["raised"]["dct_batched"]
    assert "odd" in child["raised"]["dct_twiddles"]


def test_conveniences_reject_bad_shapes_before_loading_anything():
    z = np.zeros
    for fn in (hsfft.dct, hsfft.dst, hsfft.idct, hsfft.idst):
        for x, kw in [(z((2, 3, 64)), {}), (z(()), {}), (z(7), {}), (z((3, 7)), {}), (z(1), {}), (z(0), {}), (z((2, 0)), {}),
                      (z(64), {"type": 1}), (z(64), {"type": 4})]:
            with pytest.raises(ValueError):
                fn(x, **kw)
        assert fn(z((0, 64))).shape == (0, 64)
        assert fn(z((0, 64)), type=3).dtype == np.float64


# ---------------------------------------------------------------- the yardstick, pinned
NAMES_OF = {(D.COS, 2): "DCT-II", (D.COS, 3): "DCT-III", (D.SIN, 2): "DST-II", (D.SIN, 3): "DST-III"}
KINDS_TYPES = sorted(NAMES_OF)


@pytest.mark.parametrize("kind,type", KINDS_TYPES, ids=[NAMES_OF[k] for k in KINDS_TYPES])
def test_expectation_is_scipys_transform(kind, type):
    """the composed expectation against a long-double direct sum of scipy's definition (norm=None),
    the angle reduced exactly by the integer k (2n+1) mod 4N, for every power of two from 2 to
    4096 on a uniform [-1, 1) row: the normwise error is within the suite's bound of 4 for
    oracle-against-numpy comparisons.  Powers of two only: the reference's radix-3 quirk and its
    radix-5 accuracy put other lengths at 1e4 or more in these units for its r2c alone.  A wrong
    index, sign or rotation gives an error of the order of the data, 1e15 in these units."""
    worst = 0.0
    for p in range(1, 13):
        N = 1 << p
        x = D.rows(N, 1, salt=0xB0 + 4 * kind + type)
        got, want = D.oracle(kind, type, x)[0], D.direct(kind, type, x[0])
        err = T.normwise_err(got.astype(np.longdouble), want)
        print(NAMES_OF[(kind, type)], "N", N, "normwise error", err)
        worst = max(worst, err)
        assert err <= 4, (kind, type, N, err)
    print(NAMES_OF[(kind, type)], "largest", worst)


@pytest.mark.parametrize("N", [64, 256, 4096])
def test_round_trip_is_as_accurate_as_the_reference(N):
    """dct3(dct2(x)) / 2N against x: within 4 x the error of the reference's own r2c -> c2r -> / N
    round trip on the permuted row (the margin covers the two extra rotations, four multiplies and
    two adds per word each)"""
    _, err, ref = D.round_trip_errors(N)
    print("N", N, "round trip error", err, "reference r2c -> c2r round trip error", ref, "ratio", err / ref if ref else np.inf)
    assert ref > 0
    assert err <= 4 * ref, (N, err, ref)


@pytest.mark.parametrize("N", [2, 6, 64, 1000])
def test_sine_transforms_are_variants_of_the_cosine_ones(N):
    """dst2(x) == dct2(x')[::-1] and dst3(X) == s . dct3(X[::-1]) in bits, with x' and s . the sign
    bit of the odd samples flipped, built here with np.copysign instead of the library's bit view"""
    x = D.rows(N, 3, salt=0xB9)
    odd = np.arange(N) % 2 == 1
    flipped = lambda a: np.copysign(a, np.where(np.signbit(a), 1.0, -1.0))
    xs = np.where(odd, flipped(x), x)
    assert T.mismatches(xs, D.flip_odd(x)) == 0
    assert T.mismatches(D.oracle_dct2(x, D.SIN), np.ascontiguousarray(D.oracle_dct2(xs)[:, ::-1])) == 0
    y = D.oracle_dct3(np.ascontiguousarray(x[:, ::-1]))
    assert T.mismatches(D.oracle_dct3(x, D.SIN), np.where(odd, flipped(y), y)) == 0
    z = np.array([[0.0, 0.0, -0.0, -0.0, np.nan, np.nan]])
    f = D.flip_odd(z)
    assert list(np.signbit(f[0])) == [False, True, True, False, False, True] and np.isnan(f[0, 4:]).all()


def test_the_four_kernels_exist_and_do_not_spill():
    kernels = KR._metadata()
    for name in ("k_dct2_pre", "k_dct2_post", "k_dct3_pre", "k_dct3_post"):
        hits = {k: v for k, v in kernels.items() if re.match(r"^_ZN3dct%d%sILb[01]EEE" % (len(name), name), k)}
        assert len(hits) == 2, (name, sorted(hits))  # the cosine and the sine form
        for k, res in hits.items():
            assert res.get("vgpr_spill_count", 0) == 0, (k, res)
