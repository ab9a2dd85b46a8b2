"""CPU-only checks of the type-IV cosine and sine transforms and of the MDCT / IMDCT
(hsfft_dct4_twiddles, hsfft_dct4_batched, hsfft_mdct_shape, hsfft_mdct_batched, hsfft_imdct_batched of
include/hsfft_gpu.h):
  * the symbols are exported, declared and bound, and the Python callables exist;
  * hsfft_dct4_twiddles equals the test library's libm table bit for bit;
  * every bad-argument case of all five entry points is rejected with HSFFT_ERR_ARG and a message
    before any device is touched (so it is testable here), and batch == 0 returns 0;
  * the Python conveniences reject bad shapes before loading anything, and hsfft.dct and its kin
    keep rejecting type 4;
  * the yardstick of test_gpu_dct4.py and test_gpu_mdct.py -- the expectations composed in
    hsfft_dct4_testlib around the reference's own c2c -- computes scipy's type-IV transforms and the
    MDCT's definition (long-double direct sums), inverts itself as accurately as the reference's own
    c2c round trip, and reconstructs perfectly under a Princen-Bradley window;
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

import hsfft_dct4_testlib as F
import hsfft_testlib as T
import test_kernel_resources as KR

import hsfft

NAMES = ("hsfft_dct4_twiddles", "hsfft_dct4_batched", "hsfft_mdct_shape", "hsfft_mdct_batched", "hsfft_imdct_batched")
TABLE_LENGTHS = (2, 6, 100, 4096, 12600, 65536)

# The library is loaded in a child process, as in test_dct_cpu.py.  The valid calls: 3 rows of 100
# doubles (2400 bytes in and out); 3 rows of 800 at the hop 100, 7 frames each (19200 bytes of
# samples, 16800 of coefficients, a window of 1600).
CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import hsfft
L = hsfft.lib()
X, O, W = 0x100000, 0x300000, 0x500000  # distinct non-NULL "device pointers" (never dereferenced)
BIG = 1 << 30
def err(rc):
    return (rc, L.hsfft_last_error().decode())
def dct4(kind=0, x=X, o=O, n=100, b=3):
    return err(L.hsfft_dct4_batched(kind, x, o, n, b))
out = {"exported": {n: hasattr(L, n) for n in json.loads(sys.argv[4])}}
out["dct4"] = [(what, [dct4(kind=kd, **kw) for kd in (0, 1)]) for what, kw in [
    ("n odd", dict(n=101)), ("n 1", dict(n=1)), ("n 0", dict(n=0)), ("n -2", dict(n=-2)), ("n above 2^30", dict(n=BIG + 2)),
    ("negative batch", dict(b=-1)), ("n x batch above 2^40", dict(n=BIG, b=1025)), ("NULL in", dict(x=None)),
    ("NULL out", dict(o=None)), ("in == out", dict(o=X)), ("out starts in the input's last 8 bytes", dict(o=X + 2400 - 8)),
    ("in starts in the output's last 8 bytes", dict(x=O + 2400 - 8)),
    ("out overlaps the input only at batch 3", dict(o=X + 2 * 800))]]
out["dct4"] += [("kind 2", [dct4(kind=2)] * 2), ("kind -1", [dct4(kind=-1)] * 2)]
out["zero"] = [dct4(kind=0, b=0)[0], dct4(kind=1, b=0)[0], dct4(b=0, n=BIG)[0]]
t = np.zeros(4, dtype=np.complex128)
out["bad_tw"] = [(what,) + err(L.hsfft_dct4_twiddles(n, p))
                 for what, n, p in [("n odd", 7, t.ctypes.data), ("n 0", 0, t.ctypes.data), ("n 1", 1, t.ctypes.data),
                                    ("n -4", -4, t.ctypes.data), ("n above 2^30", BIG + 2, t.ctypes.data),
                                    ("NULL table", 6, None)]]
out["tw_untouched"] = bool((t == 0).all())
nf, lp = ctypes.c_int(-7), ctypes.c_int(-7)
def shape(n, N, pad):
    return err(L.hsfft_mdct_shape(n, N, pad, ctypes.byref(nf), ctypes.byref(lp)))
out["bad_shape"] = [(what,) + shape(*a) for what, a in [
    ("N odd", (800, 5, 0)), ("N 0", (800, 0, 0)), ("N -2", (800, -2, 0)), ("N above 2^30", (BIG, BIG + 2, 1)),
    ("n no multiple of N", (850, 100, 0)), ("one hop without pad", (100, 100, 0)), ("n 0 with pad", (0, 100, 1)),
    ("n -100", (-100, 100, 1)), ("n above 2^30", (BIG + 2, 2, 0)), ("pad 2", (800, 100, 2)), ("pad -1", (800, 100, -1))]]
out["shape_untouched"] = (nf.value, lp.value) == (-7, -7)
out["shapes"] = []
for a in [(800, 100, 0), (800, 100, 1), (200, 100, 0), (100, 100, 1), (4, 2, 0), (BIG, 2, 1)]:
    rc = L.hsfft_mdct_shape(*a, ctypes.byref(nf), ctypes.byref(lp))
    out["shapes"].append((list(a), rc, nf.value, lp.value))
out["shape_null_outputs"] = L.hsfft_mdct_shape(800, 100, 0, None, None)
def mdct(x=X, n=800, w=W, N=100, pad=0, o=O, b=3):
    return err(L.hsfft_mdct_batched(x, n, w, N, pad, o, b))
out["mdct"] = [(what,) + mdct(**kw) for what, kw in [
    ("N odd", dict(N=5)), ("N 0", dict(N=0)), ("n no multiple of N", dict(n=850)), ("one hop without pad", dict(n=100)),
    ("n 0 with pad", dict(n=0, pad=1)), ("pad 2", dict(pad=2)), ("NULL x", dict(x=None)), ("NULL out", dict(o=None)),
    ("negative batch", dict(b=-1)), ("frames x batch above 2^31 - 1", dict(n=BIG, N=2, b=5)),
    ("n x batch above 2^40", dict(n=BIG, N=1 << 29, b=1025)), ("out == x", dict(o=X)),
    ("out starts in x's last 8 bytes", dict(o=X + 19200 - 8)), ("x starts in the output's last 8 bytes", dict(x=O + 16800 - 8)),
    ("out starts in the window's last 8 bytes", dict(o=W + 1600 - 8)),
    ("the window starts in the output's last 8 bytes", dict(w=O + 16800 - 8))]]
out["mdct_zero"] = [mdct(b=0)[0], mdct(b=0, w=None, pad=1)[0], mdct(b=0, o=X)[0]]
def imdct(x=X, nf=7, w=W, N=100, pad=0, o=O, n=800, b=3):
    return err(L.hsfft_imdct_batched(x, nf, w, N, pad, o, n, b))
out["imdct"] = [(what,) + imdct(**kw) for what, kw in [
    ("N odd", dict(N=5, n=40)), ("N 0", dict(N=0)), ("no frame", dict(nf=0, n=100)), ("n is not (nframes + 1) N", dict(n=700)),
    ("n is not (nframes - 1) N with pad", dict(pad=1)), ("one frame with pad: n 0", dict(nf=1, pad=1, n=0)),
    ("pad 2", dict(pad=2)), ("NULL X", dict(x=None)), ("NULL out", dict(o=None)), ("negative batch", dict(b=-1)),
    ("n above 2^30", dict(nf=(1 << 29) + 1, N=2, n=BIG + 4, b=1)),
    ("frames x batch above 2^31 - 1", dict(nf=(1 << 29) - 1, N=2, n=BIG, b=5)),
    ("n x batch above 2^40", dict(nf=1, N=1 << 29, n=BIG, b=1025)), ("out == X", dict(o=X)),
    ("out starts in X's last 8 bytes", dict(o=X + 16800 - 8)), ("X starts in the output's last 8 bytes", dict(x=O + 19200 - 8)),
    ("out starts in the window's last 8 bytes", dict(o=W + 1600 - 8)),
    ("the window starts in the output's last 8 bytes", dict(w=O + 19200 - 8))]]
out["imdct_zero"] = [imdct(b=0)[0], imdct(b=0, w=None, pad=1, n=600)[0]]
class Ptr:
    ptr = X
out["raised"] = {}
for what, fn in [("dct4_batched", lambda: hsfft.dct4_batched(0, Ptr, Ptr, 100, 3)),
                 ("dct4_twiddles", lambda: hsfft.dct4_twiddles(7)),
                 ("mdct_shape", lambda: hsfft.mdct_shape(850, 100)),
                 ("mdct_batched", lambda: hsfft.mdct_batched(Ptr, 800, None, 100, False, Ptr, 3)),
                 ("imdct_batched", lambda: hsfft.imdct_batched(Ptr, 7, None, 100, False, Ptr, 800, 3))]:
    try:
        fn()
        out["raised"][what] = None
    except hsfft.HsfftError as e:
        out["raised"][what] = str(e)
for n in json.loads(sys.argv[2]):
    hsfft.dct4_twiddles(n).view(np.float64).tofile(sys.argv[3] + ".%d" % n)
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """what a fresh process saw: no call in it has valid arguments and a non-zero batch, so nothing
    is launched wherever it runs; the tables it wrote come back as arrays"""
    base = str(tmp_path_factory.mktemp("dct4") / "table")
    res = subprocess.run([sys.executable, "-c", CHILD, T.PKG_DIR, json.dumps(TABLE_LENGTHS), base, json.dumps(NAMES)],
                         capture_output=True, text=True, timeout=120)
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
    for name in ("dct4_twiddles", "dct4_batched", "mdct_shape", "mdct_batched", "imdct_batched", "dct4", "dst4", "mdct",
                 "imdct"):
        assert callable(getattr(hsfft, name, None)), name
    # the chunk rules the GPU tests rely on and the knob's place in the scratch comment are documented
    assert re.search(r"HSFFT_DCT_CHUNK_MB / \(N x 16\) rows", header)
    assert re.search(r"HSFFT_MDCT_CHUNK_MB / \(N x 8\)\s+\*?\s*frames", header)
    assert re.search(r"HSFFT_MDCT_CHUNK_MB / \(nframes x N\s+\*?\s*x 8\) rows", header)
    scratch_comment = header[header.index("Frees the library's scratch pool"):header.index("int hsfft_release_scratch")]
    assert "HSFFT_MDCT_CHUNK_MB" in scratch_comment
    # the existing transforms' block still says why odd lengths are out, and still names what it lacks
    assert "real plan needs an even" in header


@pytest.mark.parametrize("n", TABLE_LENGTHS)
def test_twiddles_are_libm_sincos_bit_for_bit(child, n):
    got, want = child["tables"][n], F.table(n)
    assert got.shape == want.shape == (n // 2,)
    assert T.mismatches(got, want) == 0, (n, T.first_diff(got, want))
    # j = 0: pi / 8n, and the last word's angle pi (4n - 7) / 8n lies below pi / 2
    assert abs(got[0].imag - np.sin(np.pi / (8 * n))) < 1e-15 and got[-1].real > 0 and got[-1].imag > 0


def _all_rejected(cases, count):
    assert len(cases) == count
    for what, rc, msg in cases:
        assert rc == hsfft.HSFFT_ERR_ARG and msg, (what, rc, msg)


def test_dct4_bad_arguments_are_rejected(child):
    """HSFFT_ERR_ARG and a message for every bad-argument case with both kinds, before any device is
    touched; batch == 0 returns 0"""
    assert len(child["dct4"]) == 15
    for what, both in child["dct4"]:
        for rc, msg in both:
            assert rc == hsfft.HSFFT_ERR_ARG and msg, (what, rc, msg)
    assert child["zero"] == [0] * 3
    _all_rejected(child["bad_tw"], 6)
    assert child["tw_untouched"]


def test_mdct_shape_and_bad_arguments(child):
    _all_rejected(child["bad_shape"], 11)
    assert child["shape_untouched"] and child["shape_null_outputs"] == 0
    for (n, N, pad), rc, nf, lpad in child["shapes"]:
        assert rc == 0 and nf == F.nframes_of(n, N, pad) and lpad == (N if pad else 0), (n, N, pad, rc, nf, lpad)
    assert [s[2] for s in child["shapes"]] == [7, 9, 1, 2, 1, (1 << 29) + 1]
    _all_rejected(child["mdct"], 16)
    _all_rejected(child["imdct"], 18)
    assert child["mdct_zero"] == [0] * 3 and child["imdct_zero"] == [0] * 2


def test_bad_arguments_raise_in_python(child):
    assert set(child["raised"]) == {"dct4_batched", "dct4_twiddles", "mdct_shape", "mdct_batched", "imdct_batched"}
    assert "overlaps" in child["raised"]["dct4_batched"]
    assert "odd" in child["raised"]["dct4_twiddles"]
    assert "multiple" in child["raised"]["mdct_shape"]
    assert "overlaps" in child["raised"]["mdct_batched"] and "overlaps" in child["raised"]["imdct_batched"]


def test_conveniences_reject_bad_shapes_before_loading_anything():
    z = np.zeros
    for fn in (hsfft.dct4, hsfft.dst4):
        for x in (z((2, 3, 64)), z(()), z(7), z((3, 7)), z(1), z(0), z((2, 0))):
            with pytest.raises(ValueError):
                fn(x)
        assert fn(z((0, 64))).shape == (0, 64) and fn(z((0, 64))).dtype == np.float64
    for x, N, kw in [(z((2, 3, 64)), 8, {}), (z(()), 8, {}), (z(64), 7, {}), (z(64), 0, {}), (z(60), 8, {}), (z(8), 8, {}),
                     (z(0), 8, {"pad": True}), (z(64), 8, {"window": z(8)}), (z(64), 8, {"window": z((2, 16))})]:
        with pytest.raises(ValueError):
            hsfft.mdct(x, N, **kw)
    assert hsfft.mdct(z((0, 64)), 8).shape == (0, 7, 8) and hsfft.mdct(z((0, 64)), 8, pad=True).shape == (0, 9, 8)
    for X, kw in [(z(8), {}), (z((2, 2, 3, 8)), {}), (z((3, 7)), {}), (z((0, 8)), {}), (z((1, 8)), {"pad": True}),
                  (z((3, 8)), {"window": z(8)})]:
        with pytest.raises(ValueError):
            hsfft.imdct(X, **kw)
    assert hsfft.imdct(z((0, 3, 8))).shape == (0, 32) and hsfft.imdct(z((0, 3, 8)), pad=True).shape == (0, 16)
    # type IV has entry points of its own: the type argument of the existing conveniences is still 2 or 3
    for fn in (hsfft.dct, hsfft.dst, hsfft.idct, hsfft.idst):
        with pytest.raises(ValueError):
            fn(z(64), type=4)


# ---------------------------------------------------------------- the yardstick, pinned
@pytest.mark.parametrize("kind", [F.COS, F.SIN], ids=["dct4", "dst4"])
def test_expectation_is_scipys_transform(kind):
    """the composed expectation against a long-double direct sum of scipy's definition (norm=None),
    the angle reduced exactly by the integer (2k+1)(2n+1) mod 8N, for every power of two from 2 to
    4096 on a uniform [-1, 1) row: the normwise error is within the suite's bound of 4 eps (2.07
    for the cosine and 2.59 for the sine form at most, as measured with this library).  Powers of
    two only: other inner lengths carry the reference's own twiddle defects, and there the GPU
    tests claim bit-equality alone.  A wrong index, sign or rotation gives an error of the order of
    the data, 1e15 in these units."""
    worst = 0.0
    for p in range(1, 13):
        N = 1 << p
        x = F.rows(N, 1, salt=0xB0 + kind)
        got, want = F.oracle_dct4(x, kind)[0], F.direct_dct4(kind, x[0])
        err = T.normwise_err(got.astype(np.longdouble), want)
        print("kind", kind, "N", N, "normwise error", err)
        worst = max(worst, err)
        assert err <= 4, (kind, N, err)
    print("kind", kind, "largest", worst)


@pytest.mark.parametrize("kind", [F.COS, F.SIN], ids=["dct4", "dst4"])
@pytest.mark.parametrize("N", [64, 256, 4096])
def test_round_trip_is_as_accurate_as_the_reference(N, kind):
    """dct4(dct4(x)) / 2N against x: within 4 x the error of the reference's own c2c forward ->
    inverse -> / h round trip at h = N/2 (the margin covers the four extra rotations, four multiplies
    and two adds per word each)"""
    _, err, ref = F.round_trip_errors(N, kind)
    print("N", N, "kind", kind, "round trip error", err, "reference c2c round trip error", ref, "ratio", err / ref if ref else np.inf)
    assert ref > 0
    assert err <= 4 * ref, (N, err, ref)


def test_sine_form_is_a_variant_of_the_cosine_form():
    """dst4(x) == s . dct4(x[::-1]) in bits, s . the sign bit of the odd outputs flipped, built here
    with np.copysign instead of the library's bit view"""
    for N in (2, 6, 64, 1000):
        x = F.rows(N, 3, salt=0xB9)
        y = F.oracle_dct4(np.ascontiguousarray(x[:, ::-1]))
        odd = np.arange(N) % 2 == 1
        want = np.where(odd, np.copysign(y, np.where(np.signbit(y), 1.0, -1.0)), y)
        assert T.mismatches(F.oracle_dct4(x, F.SIN), want) == 0, N


def test_mdct_expectations_are_the_definitions():
    """every frame of oracle_mdct against the long-double direct sum of the forward definition on the
    windowed frame, and oracle_imdct of three frames against the overlap-added direct sums of the
    backward definition over N/2: N = 2 to 256, with and without pad and window, within 4 eps
    normwise (2.24 forward and 1.58 backward at most, as measured with this library)"""
    worst_f = worst_b = 0.0
    for p in range(1, 9):
        N = 1 << p
        for pad in (False, True):
            for win in (None, F.sine_window(N)):
                x = F.rows(5 * N, 1, salt=0xC0 + pad)
                X = F.oracle_mdct(x, N, win, pad)
                fr = F.frames(x, N, pad)
                if win is not None:
                    fr = fr * win
                assert X.shape == (1, F.nframes_of(5 * N, N, pad), N)
                for f in range(X.shape[1]):
                    err = T.normwise_err(X[0, f].astype(np.longdouble), F.direct_mdct(fr[0, f]))
                    worst_f = max(worst_f, err)
                    assert err <= 4, ("forward", N, pad, win is not None, f, err)
                C = F.rows(3 * N, 1, salt=0xC7).reshape(1, 3, N)
                lpad = N if pad else 0
                acc = np.zeros(4 * N, dtype=np.longdouble)
                for f in range(3):
                    term = F.direct_imdct(C[0, f]) / np.longdouble(N // 2)
                    acc[f * N:(f + 2) * N] += term if win is None else term * win.astype(np.longdouble)
                y = F.oracle_imdct(C, win, pad)
                assert y.shape == (1, 4 * N - 2 * lpad)
                err = T.normwise_err(y[0].astype(np.longdouble), acc[lpad:4 * N - lpad])
                worst_b = max(worst_b, err)
                assert err <= 4, ("backward", N, pad, win is not None, err)
    print("largest normwise error: forward", worst_f, "backward", worst_b)


@pytest.mark.parametrize("pad", [False, True], ids=["nopad", "pad"])
def test_windowed_round_trip_reconstructs(pad):
    """sine window, N = 64, six frames: imdct(mdct(x)) against x on the samples two frames cover
    (all of them with pad), within 8 x the reference's c2c round-trip error at h = 32 -- two
    transforms of bound 4 x each; the samples one frame covers are not reconstructed"""
    N, nf = 64, 6
    n = (nf + 1) * N - (2 * N if pad else 0)
    x, w = F.rows(n, 1, salt=0xC9), F.sine_window(N)
    assert abs(w[:N] ** 2 + w[N:] ** 2 - 1).max() < 1e-15  # Princen-Bradley, up to the rounding of sin, squares and add
    X = F.oracle_mdct(x, N, w, pad)
    assert X.shape == (1, nf, N)
    back = F.oracle_imdct(X, w, pad)
    lo, hi = (0, n) if pad else (N, n - N)
    err, ref = float(np.abs(back - x)[0, lo:hi].max()), F.c2c_round_trip_error(N // 2)
    print("pad", pad, "round trip error", err, "reference c2c round trip error at 32", ref)
    assert ref > 0 and err <= 8 * ref, (err, ref)
    if not pad:
        assert np.abs(back - x)[0, :N].max() > 1e-3


def test_fold_and_unfold_on_an_index_ramp():
    """the two index maps on exact small integers, N = 6 (odd N/2): fold's signs and unfold's, and
    the sign of (-p) - p' on zeros"""
    p = np.arange(1.0, 13.0)
    assert F.fold(p).tolist() == [-9 - 10, -8 - 11, -7 - 12, 1 - 6, 2 - 5, 3 - 4]
    v = np.arange(1.0, 7.0)
    assert F.unfold(v).tolist() == [4, 5, 6, -6, -5, -4, -3, -2, -1, -1, -2, -3]
    z = F.fold(np.zeros(12))
    assert np.signbit(z[:3]).all() and not np.signbit(z[3:]).any()  # (-0) - 0 = -0, 0 - 0 = +0


def test_the_four_kernels_exist_and_do_not_spill():
    kernels = KR._metadata()
    for ns, name, forms in (("dct4", "k_dct4_pre", 2), ("dct4", "k_dct4_post", 2), ("mdct", "k_fold", 1),
                            ("mdct", "k_unfold_ola", 1)):
        pat = r"^_ZN%d%s%d%s%s" % (len(ns), ns, len(name), name, "ILb[01]EEE" if forms == 2 else "E")
        hits = {k: v for k, v in kernels.items() if re.match(pat, k)}
        assert len(hits) == forms, (name, sorted(hits))  # the cosine and the sine form
        for k, res in hits.items():
            assert res.get("vgpr_spill_count", 0) == 0, (k, res)

