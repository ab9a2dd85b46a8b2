"""CPU-only checks of the batched chirp-z transform (hsfft_czt_shape, hsfft_czt_tables,
hsfft_czt_batched, hsfft_czt_real_batched of include/hsfft_gpu.h):
  * the symbols are exported, declared and bound, and the Python callables exist;
  * hsfft_czt_tables equals the test library's tables -- the exact phase reduction in rationals,
    libm's sincos -- bit for bit, where a plain-double phase is already wrong too;
  * every bad-argument case is rejected with HSFFT_ERR_ARG and a message before any device is
    touched (so it is testable here), and batch == 0 returns 0;
  * the yardstick of test_gpu_czt.py -- the composition in hsfft_czt_testlib around the reference's
    own c2c -- computes the definition: against a long-double direct sum it is within 4 x the error
    of the same composition around numpy.fft (the margin of the type-IV round-trip test, for the
    same reason: the two implementations round differently), it is the forward DFT at f0 = 0, df =
    1/n, and it is closer to the direct sum than scipy.signal.czt;
  * the three kernels are in the gfx950 code object and do not spill.

No call made here has valid arguments and a non-zero batch: nothing is ever launched, the
pointers are never dereferenced.
"""
import json
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import hsfft_czt_testlib as C
import hsfft_testlib as T
import test_kernel_resources as KR

import hsfft

NAMES = ("hsfft_czt_shape", "hsfft_czt_tables", "hsfft_czt_batched", "hsfft_czt_real_batched")
# (n, m, f0, df): negative df, df == 0, f0 == 0 (pre == chirp), m > n, one word, and j up to 65999
# at df = 1 / (3 x 65536), where j*j*df in plain double has lost its low bits
TABLE_CASES = ((7, 5, 0.1, 0.013), (100, 37, -0.31, -0.0021), (33, 64, 0.25, 0.0), (64, 33, 0.0, 1.0 / 64), (1, 1, 1.0, -1.0),
               (66000, 3, 0.3, 1.0 / (3 * 65536.0)))
ACCURACY_SIZES = ((1, 1), (2, 1), (1, 5), (7, 5), (33, 64), (100, 37), (1000, 300))
F0, DF = 0.1, 0.013

# The library is loaded in a child process, as in test_dct4_cpu.py.  The valid call: 3 rows of 100
# samples (2400 bytes real, 4800 complex) to 3 rows of 10 bins (480 bytes).
CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import hsfft
L = hsfft.lib()
X, O = 0x100000, 0x300000  # distinct non-NULL "device pointers" (never dereferenced)
BIG = 1 << 26
nan, inf = float("nan"), float("inf")
def err(rc):
    return (rc, L.hsfft_last_error().decode())
out = {"exported": {n: hasattr(L, n) for n in json.loads(sys.argv[3])}}
def czt(real, x=X, n=100, o=O, m=10, f0=0.1, df=0.01, b=3):
    fn = L.hsfft_czt_real_batched if real else L.hsfft_czt_batched
    return err(fn(x, n, o, m, f0, df, b))
out["czt"] = [(what, [czt(r, **kw) for r in (0, 1)]) for what, kw in [
    ("n 0", dict(n=0)), ("n -1", dict(n=-1)), ("m 0", dict(m=0)), ("m -3", dict(m=-3)),
    ("n + m - 1 above 2^26", dict(n=BIG, m=2)), ("n + m - 1 above 2^26, m large", dict(n=2, m=BIG)),
    ("n + m - 1 overflows an int", dict(n=0x7fffffff, m=0x7fffffff)),
    ("f0 NaN", dict(f0=nan)), ("f0 Inf", dict(f0=inf)), ("f0 -Inf", dict(f0=-inf)), ("f0 1.5", dict(f0=1.5)),
    ("f0 just below -1", dict(f0=-1.0000000000000002)), ("df NaN", dict(df=nan)), ("df Inf", dict(df=inf)),
    ("df 2", dict(df=2.0)), ("df just above 1", dict(df=1.0000000000000002)),
    ("NULL in", dict(x=None)), ("NULL out", dict(o=None)), ("negative batch", dict(b=-1)),
    ("n x batch above 2^40", dict(n=1 << 25, m=1, b=(1 << 15) + 1)),
    ("m x batch above 2^40", dict(n=1, m=1 << 25, b=(1 << 15) + 1)),
    ("L x batch above 2^40 alone", dict(n=(1 << 24) + 1, m=1, b=(1 << 15) + 1)),
    ("in == out", dict(o=X)), ("in starts in the output's last 8 bytes", dict(x=O + 480 - 8))]]
out["czt"] += [("out starts in the input's last 8 bytes", [czt(0, o=X + 4800 - 8), czt(1, o=X + 2400 - 8)])]
out["zero"] = [czt(0, b=0)[0], czt(1, b=0)[0], czt(0, b=0, o=X)[0], czt(1, b=0, n=BIG, m=1)[0]]
t = np.zeros(8, dtype=np.complex128)
p = t.ctypes.data
out["bad_tables"] = [(what,) + err(L.hsfft_czt_tables(n, m, f0, df, p, p + 64))
                     for what, n, m, f0, df in [("n 0", 0, 3, 0.1, 0.1), ("m 0", 3, 0, 0.1, 0.1), ("n -1", -1, 3, 0.1, 0.1),
                                                ("n + m - 1 above 2^26", BIG, 2, 0.1, 0.1), ("f0 NaN", 3, 3, nan, 0.1),
                                                ("f0 -1.5", 3, 3, -1.5, 0.1), ("df Inf", 3, 3, 0.1, inf), ("df NaN", 3, 3, 0.1, nan),
                                                ("df -2", 3, 3, 0.1, -2.0)]]
out["tables_untouched"] = bool((t == 0).all())
out["tables_null"] = [L.hsfft_czt_tables(4, 3, 0.1, 0.2, None, None), L.hsfft_czt_tables(4, 3, 0.1, 0.2, p, None),
                      L.hsfft_czt_tables(4, 3, 0.1, 0.2, None, p + 64)]
out["tables_null_wrote"] = [bool((t[:4] != 0).all()), bool((t[4:] != 0).all())]
Lv = ctypes.c_int(-7)
out["bad_shape"] = [(what,) + err(L.hsfft_czt_shape(n, m, ctypes.byref(Lv)))
                    for what, n, m in [("n 0", 0, 1), ("m 0", 1, 0), ("n -5", -5, 9), ("sum above 2^26", BIG, 2),
                                       ("sum overflows", 0x7fffffff, 0x7fffffff)]]
out["shape_untouched"] = Lv.value == -7
out["shapes"] = []
for n, m in [(1, 1), (2, 1), (1, 2), (2, 2), (40, 25), (40, 26), (33, 32), (BIG, 1), (1, BIG), (BIG // 2, BIG // 2 + 1)]:
    rc = L.hsfft_czt_shape(n, m, ctypes.byref(Lv))
    out["shapes"].append((n, m, rc, Lv.value))
out["shape_null_output"] = L.hsfft_czt_shape(40, 25, None)
class Ptr:
    ptr = X
out["raised"] = {}
for what, fn in [("czt_batched", lambda: hsfft.czt_batched(Ptr, False, 100, Ptr, 10, 0.1, 0.01, 3)),
                 ("czt_real_batched", lambda: hsfft.czt_batched(Ptr, True, 100, Ptr, 10, 0.1, 0.01, 3)),
                 ("czt_tables", lambda: hsfft.czt_tables(3, 3, 0.1, float("nan"))),
                 ("czt_shape", lambda: hsfft.czt_shape(0, 3))]:
    try:
        fn()
        out["raised"][what] = None
    except hsfft.HsfftError as e:
        out["raised"][what] = str(e)
for i, (n, m, f0, df) in enumerate(json.loads(sys.argv[2])):
    pre, chirp = hsfft.czt_tables(n, m, f0, df)
    pre.view(np.float64).tofile(sys.argv[4] + ".pre%d" % i)
    chirp.view(np.float64).tofile(sys.argv[4] + ".chirp%d" % i)
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """what a fresh process saw: no call in it has valid arguments and a non-zero batch, so nothing
    is launched wherever it runs; the tables it wrote come back as arrays"""
    base = str(tmp_path_factory.mktemp("czt") / "table")
    res = subprocess.run([sys.executable, "-c", CHILD, T.PKG_DIR, json.dumps(TABLE_CASES), json.dumps(NAMES), base],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    out["tables"] = [(np.fromfile(base + ".pre%d" % i, dtype=np.complex128), np.fromfile(base + ".chirp%d" % i, dtype=np.complex128))
                     for i in range(len(TABLE_CASES))]
    return out


def test_symbols_exported_and_declared(child):
    assert os.path.exists(hsfft.LIB_PATH)
    header = open(os.path.join(T.REPO, "include", "hsfft_gpu.h")).read()
    for name in NAMES:
        assert child["exported"][name], name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in hsfft.SIGNATURES, name
    for name in ("czt_shape", "czt_tables", "czt_batched", "czt", "zoom_fft"):
        assert callable(getattr(hsfft, name, None)), name
    # the chunk rule the GPU test relies on and the knob's place in the scratch comment are documented
    assert re.search(r"HSFFT_CZT_CHUNK_MB / \(2 x L x 16\) rows", header)
    scratch_comment = header[header.index("Frees the library's scratch pool"):header.index("int hsfft_release_scratch")]
    assert "HSFFT_CZT_CHUNK_MB" in scratch_comment and "hs_czt_release_device" in scratch_comment


@pytest.mark.parametrize("i", range(len(TABLE_CASES)), ids=["%d-%d" % c[:2] for c in TABLE_CASES])
def test_tables_are_the_reduced_phases_bit_for_bit(child, i):
    n, m, f0, df = TABLE_CASES[i]
    (pre, chirp), (wpre, wchirp) = child["tables"][i], C.tables(n, m, f0, df)
    assert pre.shape == wpre.shape == (n,) and chirp.shape == wchirp.shape == (max(n, m),)
    assert T.mismatches(chirp, wchirp) == 0, (TABLE_CASES[i], T.first_diff(chirp, wchirp))
    assert T.mismatches(pre, wpre) == 0, (TABLE_CASES[i], T.first_diff(pre, wpre))
    assert pre[0] == 1.0 and chirp[0] == 1.0
    if f0 == 0.0:
        assert T.mismatches(pre, chirp[:n]) == 0


def test_the_reduction_keeps_what_a_plain_double_phase_loses():
    """j = 65535, df = 1 / (3 x 65536): j*j*df mod 2 formed in plain double is 1.2e-12 half-turns off
    the exact value (and more at other j nearby); red() is within one rounding of it"""
    j, df = 65535.0, 1.0 / (3 * 65536.0)
    exact = Fraction(j * j) * Fraction(df) % 2
    plain = abs(Fraction(math.fmod(j * j * df, 2.0)) - exact)
    kept = abs(Fraction(C.red(j * j, df)) - exact)
    print("plain double phase error", float(plain), "reduced phase error", float(kept))
    assert float(plain) > 1e-12
    assert float(kept) <= 2.0 ** -52


def _all_rejected(cases, count):
    assert len(cases) == count
    for what, rc, msg in cases:
        assert rc == hsfft.HSFFT_ERR_ARG and msg, (what, rc, msg)


def test_bad_arguments_are_rejected(child):
    """HSFFT_ERR_ARG and a message for every bad-argument case of both entry points, before any device
    is touched; batch == 0 returns 0"""
    assert len(child["czt"]) == 25
    for what, both in child["czt"]:
        for rc, msg in both:
            assert rc == hsfft.HSFFT_ERR_ARG and msg, (what, rc, msg)
    assert child["zero"] == [0] * 4
    _all_rejected(child["bad_tables"], 9)
    assert child["tables_untouched"]
    assert child["tables_null"] == [0] * 3 and child["tables_null_wrote"] == [True, True]


def test_shape(child):
    _all_rejected(child["bad_shape"], 5)
    assert child["shape_untouched"] and child["shape_null_output"] == 0
    for n, m, rc, L in child["shapes"]:
        assert rc == 0 and L == C.shape_L(n, m), (n, m, rc, L)
    assert [s[3] for s in child["shapes"]] == [2, 2, 2, 4, 64, 128, 64, 1 << 26, 1 << 26, 1 << 26]


def test_bad_arguments_raise_in_python(child):
    assert set(child["raised"]) == {"czt_batched", "czt_real_batched", "czt_tables", "czt_shape"}
    assert "overlaps" in child["raised"]["czt_batched"] and "overlaps" in child["raised"]["czt_real_batched"]
    assert "finite" in child["raised"]["czt_tables"]
    assert "below 1" in child["raised"]["czt_shape"]


def test_conveniences_reject_bad_shapes_before_loading_anything():
    z = np.zeros
    for x, m, f0, df in [(z((2, 3, 8)), 4, 0.1, 0.1), (z(()), 4, 0.1, 0.1), (z(0), 4, 0.1, 0.1), (z(8), 0, 0.1, 0.1),
                         (z(8), 4, 1.5, 0.1), (z(8), 4, 0.1, float("nan")), (z(8), 4, float("inf"), 0.1), (z((2, 0)), 4, 0.1, 0.1)]:
        with pytest.raises(ValueError):
            hsfft.czt(x, m, f0, df)
    assert hsfft.czt(z((0, 8)), 5, 0.1, 0.1).shape == (0, 5) and hsfft.czt(z((0, 8)), 5, 0.1, 0.1).dtype == np.complex128
    for x, fn, kw in [(z((2, 3, 8)), 0.5, {}), (z(8), [0.1, 0.2, 0.3], {}), (z(8), 0.5, {"m": 0}), (z(8), [3.0, 9.0], {})]:
        with pytest.raises(ValueError):
            hsfft.zoom_fft(x, fn, **kw)
    assert hsfft.zoom_fft(z((0, 8)), [0.2, 0.5], m=3).shape == (0, 3)


# ---------------------------------------------------------------- the yardstick, pinned
_DIRECT = {}


def _accuracy(n, m, real):
    """(the row, the direct sum, the oracle composition's error, the numpy composition's error)"""
    key = (n, m, real)
    if key not in _DIRECT:
        x = C.real_rows(n, 1, salt=0xA1) if real else C.complex_rows(n, 1, salt=0xA1)
        want = C.direct_czt(x[0], m, F0, DF)
        _DIRECT[key] = (x, want, C.rel_err(C.oracle_czt(x, m, F0, DF)[0], want), C.rel_err(C.numpy_czt(x, m, F0, DF)[0], want))
    return _DIRECT[key]


@pytest.mark.parametrize("real", [True, False], ids=["real", "complex"])
@pytest.mark.parametrize("n,m", ACCURACY_SIZES)
def test_expectation_is_the_definition(n, m, real):
    """the composed expectation against the long-double direct sum, max |difference| / max |X|: within
    4 x the error of the same composition around numpy.fft on the same input (measured with this
    library at f0 = 0.1, df = 0.013: 0 for both at (1, 1); at most 1.06e-15 for the oracle, at (33, 64)
    real and (100, 37) complex, and 9.1e-16 for numpy; the largest ratio is 1.63, at (100, 37) complex)"""
    _, _, err, ref = _accuracy(n, m, real)
    print("n", n, "m", m, "real", real, "oracle composition", err, "numpy composition", ref)
    assert err <= 4 * ref, (n, m, real, err, ref)


def test_it_is_the_forward_transform_on_the_dft_grid():
    """n = m = 16, f0 = 0, df = 1/16: the composition against the reference's own forward c2c, within
    4 x the numpy composition's error against the direct sum there"""
    n = 16
    x = C.complex_rows(n, 1, salt=0xA2)
    want = C.direct_czt(x[0], n, 0.0, 1.0 / n)
    bound = 4 * C.rel_err(C.numpy_czt(x, n, 0.0, 1.0 / n)[0], want)
    got, dft = C.oracle_czt(x, n, 0.0, 1.0 / n)[0], T.oracle_c2c(x[0], 1)
    err = C.rel_err(got, dft)
    print("against the reference's c2c", err, "bound", bound)
    assert bound > 0 and err <= bound, (err, bound)


def test_it_is_closer_to_the_definition_than_scipy():
    """(1000, 300): scipy.signal.czt forms the chirp phase in plain double and loses bits as j grows"""
    signal = pytest.importorskip("scipy.signal")
    n, m = 1000, 300
    x, want, err, _ = _accuracy(n, m, False)
    theirs = C.rel_err(signal.czt(x[0], m, np.exp(-2j * np.pi * DF), np.exp(2j * np.pi * F0)), want)
    print("oracle composition", err, "scipy.signal.czt", theirs)
    assert err < theirs, (err, theirs)


def test_the_three_kernels_exist_and_do_not_spill():
    kernels = KR._metadata()
    for name, forms in (("k_czt_pre", 2), ("k_czt_mul", 1), ("k_czt_post", 1)):
        pat = r"^_ZN3czt%d%s%s" % (len(name), name, "ILb[01]EEE" if forms == 2 else "E")
        hits = {k: v for k, v in kernels.items() if re.match(pat, k)}
        assert len(hits) == forms, (name, sorted(hits))  # the complex and the real form
        for k, res in hits.items():
            assert res.get("vgpr_spill_count", 0) == 0, (k, res)
