"""CPU-only checks of the batched analytic signal and of Fourier resampling (hsfft_hilbert_batched,
hsfft_resample_batched, hsfft_spectral_chunk_rows of include/hsfft_gpu.h):
  * the symbols are exported, declared and bound, and the Python callables exist;
  * every bad-argument case is rejected with HSFFT_ERR_ARG and a message before any device is
    touched (so it is testable here), and batch == 0 returns 0;
  * hsfft_spectral_chunk_rows equals the documented rule, at the default knob and at others;
  * the yardstick of test_gpu_spectral.py -- the compositions in hsfft_spectral_testlib around the
    reference's own r2c, c2c and c2r -- computes the definitions: against long-double direct sums the
    error is at most max(1, 4 x the error of the same composition around numpy.fft) in T.normwise_err
    units, on powers of two only (test_dct_cpu.py gives the reason: the reference's radix-3 quirk and
    its radix-5 accuracy put other lengths far off for its r2c alone); the analytic signal's real
    part is the row; and both agree with scipy.signal where scipy is installed;
  * the two kernels are in the gfx950 code object and do not spill.

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

import hsfft_spectral_testlib as SP
import hsfft_testlib as T
import test_kernel_resources as KR

import hsfft

NAMES = ("hsfft_hilbert_batched", "hsfft_resample_batched", "hsfft_spectral_chunk_rows")
HILBERT_SIZES = tuple(1 << p for p in range(1, 12))  # 2 .. 2048
RESAMPLE_PAIRS = ((2, 2), (2, 4), (4, 2), (2, 64), (64, 2), (8, 32), (32, 8), (64, 64), (256, 128), (128, 256), (1024, 2048),
                  (2048, 512))
CHUNK_CASES = ((2, 0), (2, 2), (64, 0), (3000, 0), (3000, 2000), (2000, 3000), (65536, 0), (65536, 32768), (1 << 30, 0),
               (1 << 30, 1 << 30), (1 << 30, 2))

# The library is loaded in a child process, as in test_czt_cpu.py.  The valid calls: 3 rows of 100
# samples (2400 bytes) to 3 rows of 100 complex (4800 bytes) or of 60 reals (1440 bytes).
CHILD = r"""
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
import hsfft
L = hsfft.lib()
X, O = 0x100000, 0x300000  # distinct non-NULL, 16-byte aligned "device pointers" (never dereferenced)
BIG = 1 << 30
def err(rc):
    return (rc, L.hsfft_last_error().decode())
out = {"exported": {n: hasattr(L, n) for n in json.loads(sys.argv[2])}}
def hil(x=X, o=O, n=100, b=3):
    return err(L.hsfft_hilbert_batched(x, o, n, b))
def res(x=X, n=100, o=O, m=60, b=3):
    return err(L.hsfft_resample_batched(x, n, o, m, b))
out["hilbert"] = [(what,) + hil(**kw) for what, kw in [
    ("NULL in", dict(x=None)), ("NULL out", dict(o=None)), ("negative batch", dict(b=-1)),
    ("n odd", dict(n=101)), ("n 1", dict(n=1)), ("n 0", dict(n=0)), ("n -2", dict(n=-2)), ("n above 2^30", dict(n=BIG + 2)),
    ("n x batch above 2^40", dict(n=BIG, b=1025)),
    ("in 8-byte aligned", dict(x=X + 8)), ("out 8-byte aligned", dict(o=O + 8)), ("out 4-byte aligned", dict(o=O + 4)),
    ("in == out", dict(o=X)), ("out starts in the input's last 16 bytes", dict(o=X + 2400 - 16)),
    ("in starts in the output's last 16 bytes", dict(x=O + 4800 - 16)),
    ("out overlaps the input only at batch 3", dict(o=X + 2 * 800))]]
out["resample"] = [(what,) + res(**kw) for what, kw in [
    ("NULL in", dict(x=None)), ("NULL out", dict(o=None)), ("negative batch", dict(b=-1)),
    ("n odd", dict(n=101)), ("n 1", dict(n=1)), ("n 0", dict(n=0)), ("n -2", dict(n=-2)), ("n above 2^30", dict(n=BIG + 2)),
    ("m odd", dict(m=61)), ("m 1", dict(m=1)), ("m 0", dict(m=0)), ("m -2", dict(m=-2)), ("m above 2^30", dict(m=BIG + 2)),
    ("n x batch above 2^40", dict(n=BIG, m=2, b=1025)), ("m x batch above 2^40", dict(n=2, m=BIG, b=1025)),
    ("in 8-byte aligned", dict(x=X + 8)), ("out 8-byte aligned", dict(o=O + 8)), ("out 4-byte aligned", dict(o=O + 4)),
    ("in == out", dict(o=X)), ("out starts in the input's last 16 bytes", dict(o=X + 2400 - 16)),
    ("in starts in the output's last 16 bytes", dict(x=O + 1440 - 16)),
    ("out overlaps the input only at batch 3", dict(o=X + 2 * 800))]]
out["ok_neighbours"] = [hil(o=X + 2400, b=0)[0], res(o=X + 2400, b=0)[0]]
out["zero"] = [hil(b=0)[0], res(b=0)[0], hil(b=0, o=X)[0], res(b=0, o=X)[0], hil(b=0, n=BIG)[0], res(b=0, n=BIG, m=BIG)[0]]
rows = ctypes.c_longlong(-7)
out["bad_rows"] = [(what,) + err(L.hsfft_spectral_chunk_rows(n, m, ctypes.byref(rows)))
                   for what, n, m in [("n odd", 7, 0), ("n 0", 0, 0), ("n 0, m valid", 0, 4), ("n -2", -2, 0), ("n above 2^30", BIG + 2, 0),
                                      ("m odd", 8, 5), ("m 1", 8, 1), ("m -2", 8, -2), ("m above 2^30", 8, BIG + 2)]]
out["rows_untouched"] = rows.value == -7
out["rows_null"] = L.hsfft_spectral_chunk_rows(64, 0, None)
out["rows"] = {}
for knob in json.loads(sys.argv[4]):
    if knob is None:
        os.environ.pop("HSFFT_SPECTRAL_CHUNK_MB", None)
    else:
        os.environ["HSFFT_SPECTRAL_CHUNK_MB"] = knob
    got = []
    for n, m in json.loads(sys.argv[3]):
        rc = L.hsfft_spectral_chunk_rows(n, m, ctypes.byref(rows))
        got.append((rc, rows.value, hsfft.spectral_chunk_rows(n, m)))
    out["rows"][str(knob)] = got
os.environ.pop("HSFFT_SPECTRAL_CHUNK_MB", None)
class Ptr:
    ptr = X
class Odd:
    ptr = X + 8
out["raised"] = {}
for what, fn in [("hilbert_batched", lambda: hsfft.hilbert_batched(Ptr, Ptr, 100, 3)),
                 ("resample_batched", lambda: hsfft.resample_batched(Ptr, 100, Ptr, 60, 3)),
                 ("hilbert_batched aligned", lambda: hsfft.hilbert_batched(Odd, Ptr, 100, 3)),
                 ("resample_batched odd", lambda: hsfft.resample_batched(Ptr, 100, Ptr, 61, 3)),
                 ("spectral_chunk_rows", lambda: hsfft.spectral_chunk_rows(7))]:
    try:
        fn()
        out["raised"][what] = None
    except hsfft.HsfftError as e:
        out["raised"][what] = str(e)
print(json.dumps(out))
"""
KNOBS = (None, "1", "0.001", "64", "2.5")


@pytest.fixture(scope="module")
def child():
    """what a fresh process saw: no call in it has valid arguments and a non-zero batch, so nothing
    is launched wherever it runs"""
    res = subprocess.run([sys.executable, "-c", CHILD, T.PKG_DIR, json.dumps(NAMES), json.dumps(CHUNK_CASES), json.dumps(KNOBS)],
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
    for name in ("hilbert_batched", "resample_batched", "spectral_chunk_rows", "hilbert", "resample"):
        assert callable(getattr(hsfft, name, None)), name
    # the chunk rules the GPU test relies on, the knob's place in the scratch comment, the alignment
    # contract and the twiddle-mode caveat are documented
    assert re.search(r"HSFFT_SPECTRAL_CHUNK_MB / \(16 x \(n/2\+1\) \+ 16 x n\) rows", header)
    assert re.search(r"HSFFT_SPECTRAL_CHUNK_MB / \(16 x \(n/2\+1\) \+ 16 x \(m/2\+1\)\) rows", header)
    scratch_comment = header[header.index("Frees the library's scratch pool"):header.index("int hsfft_release_scratch")]
    assert "HSFFT_SPECTRAL_CHUNK_MB" in scratch_comment
    block = header[header.index("analytic signal (Hilbert)"):header.index("int hsfft_spectral_chunk_rows")]
    assert "16-byte aligned" in block and "twiddle mode" in block and "quirk" in block and "2^30" in block


def _all_rejected(cases, count, word=None):
    assert len(cases) == count
    for what, rc, msg in cases:
        assert rc == hsfft.HSFFT_ERR_ARG and msg, (what, rc, msg)
        if word:
            assert word in msg, (what, msg)


def test_bad_arguments_are_rejected(child):
    """HSFFT_ERR_ARG and the case's own message for every bad-argument case of both entry points, before
    any device is touched; batch == 0 returns 0"""
    for key, count in (("hilbert", 16), ("resample", 22)):
        cases = child[key]
        _all_rejected(cases, count)
        by = {what: msg for what, rc, msg in cases}
        for what, msg in by.items():
            assert msg.startswith("hsfft_%s_batched: " % key), (what, msg)
            if what.startswith("NULL") or what == "negative batch":
                assert "NULL pointer or negative batch" in msg, (what, msg)
            elif "batch above" in what:
                assert "more than the call can index" in msg, (what, msg)
            elif what[0] in "nm":
                assert "odd, below 2 or above 2^30" in msg, (what, msg)
            elif "aligned" in what:
                assert "16-byte aligned" in msg, (what, msg)
            else:
                assert "overlaps" in msg, (what, msg)
    assert child["zero"] == [0] * 6 and child["ok_neighbours"] == [0, 0]


def test_chunk_rows_is_the_documented_rule(child):
    _all_rejected(child["bad_rows"], 9, "odd, below 2 or above 2^30")
    assert child["rows_untouched"] and child["rows_null"] == 0
    for knob in KNOBS:
        mb = 1024.0 if knob is None else float(knob)
        nbytes = max(int(mb * (1 << 20)), 1 << 20)  # at least 1 MiB, fractions of a MiB kept
        for (n, m), (rc, rows, bound) in zip(CHUNK_CASES, child["rows"][str(knob)]):
            per = 16 * (n // 2 + 1) + (16 * (m // 2 + 1) if m else 16 * n)
            assert rc == 0 and rows == bound == max(1, nbytes // per), (knob, n, m, rc, rows, bound)
            if mb == int(mb):
                assert rows == SP.chunk_rows(n, m, int(mb)), (knob, n, m)
    one = dict(zip(CHUNK_CASES, child["rows"]["1"]))
    assert one[(3000, 0)][1] == 14 == 1048576 // 72016 and one[(3000, 2000)][1] == 26 == 1048576 // 40032


def test_bad_arguments_raise_in_python(child):
    assert set(child["raised"]) == {"hilbert_batched", "resample_batched", "hilbert_batched aligned", "resample_batched odd",
                                    "spectral_chunk_rows"}
    assert "overlaps" in child["raised"]["hilbert_batched"] and "overlaps" in child["raised"]["resample_batched"]
    assert "16-byte aligned" in child["raised"]["hilbert_batched aligned"]
    assert "odd" in child["raised"]["resample_batched odd"] and "odd" in child["raised"]["spectral_chunk_rows"]


def test_conveniences_reject_bad_shapes_before_loading_anything():
    z = np.zeros
    for x in (z((2, 3, 8)), z(()), z(7), z((3, 7)), z(1), z(0), z((2, 0))):
        with pytest.raises(ValueError):
            hsfft.hilbert(x)
        with pytest.raises(ValueError):
            hsfft.resample(x, 8)
    for num in (0, 1, 7, -2, (1 << 30) + 2):
        with pytest.raises(ValueError):
            hsfft.resample(z(8), num)
    assert hsfft.hilbert(z((0, 8))).shape == (0, 8) and hsfft.hilbert(z((0, 8))).dtype == np.complex128
    assert hsfft.resample(z((0, 8)), 6).shape == (0, 6) and hsfft.resample(z((0, 8)), 6).dtype == np.float64


# ---------------------------------------------------------------- the yardstick, pinned
_CASES = {}


def _hilbert_case(n):
    """(the row, the long-double sum, the oracle composition, its error, the numpy composition's error)"""
    if n not in _CASES:
        x = SP.rows(n, 1, salt=0xA1)
        want = SP.direct_hilbert(x[0])
        got = SP.oracle_hilbert(x)[0]
        _CASES[n] = (x, want, got, SP.err_units(got, want), SP.err_units(SP.numpy_hilbert(x)[0], want))
    return _CASES[n]


def _resample_case(n, m):
    if (n, m) not in _CASES:
        x = SP.rows(n, 1, salt=0xA2 + m)
        want = SP.direct_resample(x[0], m)
        got = SP.oracle_resample(x, m)[0]
        _CASES[(n, m)] = (x, want, got, SP.err_units(got, want), SP.err_units(SP.numpy_resample(x, m)[0], want))
    return _CASES[(n, m)]


def _bound(ref):
    """the suite's margin of 4 for oracle-against-numpy comparisons, with a floor of one unit: at n <= 4
    numpy is exact to 1e-4 units, and an index or sign mistake gives about 1e15"""
    return max(1.0, 4.0 * ref)


def test_hilbert_expectation_is_the_definition():
    """powers of two from 2 to 2048, in units of eps x max |want|.  Measured with this library: the
    largest error of the oracle composition is 2.97 units (n = 2048), of the numpy composition 1.78 (n =
    2048); from n = 8 up the ratio of the two lies between 0.61 and 1.81; at n = 4 the oracle
    composition is 0.18 units off where numpy is exact to 4e-4, which the floor of one unit covers"""
    worst = 0.0
    for n in HILBERT_SIZES:
        _, _, _, err, ref = _hilbert_case(n)
        print("hilbert n", n, "oracle composition", err, "numpy composition", ref)
        worst = max(worst, err)
        assert err <= _bound(ref), (n, err, ref)
    print("hilbert largest", worst)


def test_hilbert_real_part_is_the_row():
    for n in HILBERT_SIZES:
        x, want, got, _, ref = _hilbert_case(n)
        unit = np.finfo(np.float64).eps * np.abs(want).max()  # the same unit: eps x max |want|
        err = float(np.abs(got.real.astype(np.longdouble) - x[0].astype(np.longdouble)).max() / unit)
        print("hilbert n", n, "real part against the row", err)
        assert err <= _bound(ref), (n, err, ref)
        # and the definition's own real part is the row
        assert float(np.abs(want.real - x[0]).max()) < 1e-17 * n


@pytest.mark.parametrize("n,m", RESAMPLE_PAIRS)
def test_resample_expectation_is_the_definition(n, m):
    """measured with this library: the largest error of the oracle composition is 3.12 units, at (1024,
    2048), where the numpy composition has 1.95; numpy's own largest is 2.87, at (64, 2); above the floor
    of one unit the largest ratio of the two is 2.57, at (2, 64)"""
    _, _, _, err, ref = _resample_case(n, m)
    print("resample", n, m, "oracle composition", err, "numpy composition", ref)
    assert err <= _bound(ref), (n, m, err, ref)


def test_expectations_agree_with_scipy():
    """scipy.signal.hilbert and scipy.signal.resample within the same bound, in the same units"""
    signal = pytest.importorskip("scipy.signal")
    for n in HILBERT_SIZES:
        x, want, got, _, ref = _hilbert_case(n)
        err = float(np.abs(got - signal.hilbert(x[0])).max() / (np.finfo(np.float64).eps * float(np.abs(want).max())))
        print("hilbert n", n, "against scipy", err)
        assert err <= _bound(ref), (n, err, ref)
    for n, m in RESAMPLE_PAIRS:
        x, want, got, _, ref = _resample_case(n, m)
        err = float(np.abs(got - signal.resample(x[0], m)).max() / (np.finfo(np.float64).eps * float(np.abs(want).max())))
        print("resample", n, m, "against scipy", err)
        assert err <= _bound(ref), (n, m, err, ref)


def test_the_folded_bin_has_no_imaginary_part():
    """m < n: Y[K] = (q(2 Re S[K]), +0.0); the rule's three branches on one row, in bits"""
    S = np.array([[1.5 + 0.0j, -2.0 + 3.0j, 0.25 - 0.75j, 5.0 + 7.0j, -1.0 + 0.0j]])  # n = 8
    Y = SP.resample_spectrum(S, 8, 4)
    assert Y.shape == (1, 3) and Y[0, 2] == complex(0.25 * 2 / 8.0, 0.0) and not np.signbit(Y[0, 2].imag)
    assert Y[0, 1] == complex(-2.0 / 8.0, 3.0 / 8.0)
    Y = SP.resample_spectrum(S, 8, 12)
    assert Y.shape == (1, 7) and Y[0, 4] == complex(-0.5 / 8.0, 0.0) and T.zero_words(Y[0, 5:]) == 4
    Y = SP.resample_spectrum(S, 8, 8)
    assert T.mismatches(Y, S / 8.0) == 0
    Z = SP.hilbert_spectrum(S, 8)
    assert Z.shape == (1, 8) and Z[0, 0] == 1.5 / 8 and Z[0, 4] == -1.0 / 8 and Z[0, 1] == complex(-4.0 / 8, 6.0 / 8)
    assert T.zero_words(Z[0, 5:]) == 6 and not np.signbit(Z[0, 5:].view(np.float64)).any()


def test_the_two_kernels_exist_and_do_not_spill(tmp_path, monkeypatch):
    """test_kernel_resources._metadata() on a copy of the library: its objcopy step, given no output
    name, writes its input file anew, and this process may have the library mapped by now (the test
    files that load it in-process sort before this one)"""
    if not os.path.exists(KR.LIB):
        pytest.skip("lib/libhsfft.so not built")
    copy = str(tmp_path / "libhsfft_copy.so")
    shutil.copyfile(KR.LIB, copy)
    monkeypatch.setattr(KR, "LIB", copy)
    kernels = KR._metadata()
    for name in ("k_hilbert_spec", "k_resample_spec"):
        hits = {k: v for k, v in kernels.items() if re.match(r"^_ZN4spec%d%sE" % (len(name), name), k)}
        assert len(hits) == 1, (name, sorted(hits))
        for k, res in hits.items():
            assert res.get("vgpr_spill_count", 0) == 0, (k, res)
