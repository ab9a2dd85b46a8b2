"""Live pin of the oracle against the unmodified reference build (oracle/_ref/libhsref.so).
Skipped where the reference was not built (the GPU box relies on test_oracle_golden)."""
import ctypes

import numpy as np
import pytest

import hsfft_testlib as T

ref = T.reference()
pytestmark = pytest.mark.skipif(ref is None, reason="reference build oracle/_ref absent")

ASIS_SIZES = [3, 4, 5, 7, 8, 9, 12, 15, 16, 20, 25, 27, 32, 36, 45, 49, 60, 64, 100, 125, 243,
              343, 256, 512, 4096, 12600, 11, 22, 121, 17, 92, 87, 31, 185, 41, 43, 47, 106, 88,
              19, 97, 1021, 5003]


@pytest.mark.parametrize("n", ASIS_SIZES)
def test_oracle_equals_reference_asis(n):
    rng = np.random.default_rng(n)
    for sgn in (1, -1):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        y = np.zeros(n, dtype=np.complex128)
        p = ref.fft_init(n, sgn)
        ref.fft_exec(p, T.ptr(x), T.ptr(y))
        ref.free_fft(p)
        assert T.bits_equal(T.oracle_c2c(x, sgn, T.ORC_LEAF2_ASIS), y)


def test_factors_and_dividebyN_exhaustive():
    lib = T.oracle()
    a = np.zeros(64, dtype=np.int32)
    b = np.zeros(64, dtype=np.int32)
    for n in range(1, 1 << 16):
        assert lib.orc_dividebyN(n) == ref.dividebyN(n), n
        ka = lib.orc_factors(n, T.ptr(a))
        kb = ref.factors(n, T.ptr(b))
        assert ka == kb and np.array_equal(a[:ka], b[:kb]), n


def test_twiddle_bytes_equal_reference_plan():
    for n in [12, 36, 1024, 12600, 99991, 1 << 16]:
        for sgn in (1, -1):
            p = ref.fft_init(n, sgn)
            hdr = (ctypes.c_int * 68).from_address(p)
            lf = hdr[66]
            m = int(np.prod([hdr[2 + i] for i in range(lf)]))
            rtw = np.frombuffer(bytes((ctypes.c_double * (2 * (m - 1))).from_address(p + 272)), dtype=np.complex128)
            ref.free_fft(p)
            tw, _, _, om = T.oracle_plan_twiddles(n, sgn, 0)
            assert om == m and T.bits_equal(tw, rtw)


# ---------------------------------------------------------------- special values
# The GPU tests of the value domain (test_gpu_values.py) compare with the
# oracle on zeros of either sign, subnormals, values near overflow and non-finite values; here
# the oracle is pinned to the reference on those inputs.
def _ref_c2c(x, sgn):
    y = np.zeros(x.size, dtype=np.complex128)
    p = ref.fft_init(x.size, sgn)
    ref.fft_exec(p, T.ptr(x), T.ptr(y))
    ref.free_fft(p)
    return y


def _nonfinite_rows(n, seed, real=False):
    """dense rows with +Inf at n//3 and with a NaN at index 1"""
    a = T.real_input(n, seed) if real else T.complex_input(n, seed)
    b = a.copy()
    a[n // 3] = np.inf if real else complex(np.inf, a[n // 3].imag)
    b[1 % n] = np.nan if real else complex(np.nan, b[1 % n].imag)
    return a, b


@pytest.mark.parametrize("n", ASIS_SIZES)
def test_oracle_equals_reference_special_values(n):
    """every special kind, both signs: bit-equal; +Inf at n//3 and a NaN at index 1: bit-equal
    outside NaN words, whose positions coincide"""
    for sgn in (1, -1):
        for kind in T.SPECIAL_KINDS:
            x = T.special_inputs(n, kind, T.seed_for(n))
            got, want = T.oracle_c2c(x, sgn, T.ORC_LEAF2_ASIS), _ref_c2c(x, sgn)
            assert T.bits_equal(got, want), (n, sgn, kind, T.mismatches(got, want), T.first_diff(got, want))
        for x in _nonfinite_rows(n, T.seed_for(n)):
            got, want = T.oracle_c2c(x, sgn, T.ORC_LEAF2_ASIS), _ref_c2c(x, sgn)
            assert T.same_bits_nan_aware(got, want), (n, sgn, "non-finite")


def _ref_real(n, sgn, x, inverse):
    rp = ref.fft_real_init(n, sgn)
    y = np.zeros(n, dtype=np.float64 if inverse else np.complex128)
    (ref.fft_c2r_exec if inverse else ref.fft_r2c_exec)(rp, T.ptr(x), T.ptr(y))
    ref.free_real_fft(rp)
    return y


# 12 and 100 are left out: their inner plans (6 = [3,2], 50 = [5,5,2]) end in the radix-2 leaf
# that reads its stale output slot (D1), and real.c:87-88 / :159-160 hand fft_exec a buffer
# straight from malloc, so the reference's result there is whatever the heap held -- for every
# kind, finite or not.  (The c2c test above zeroes the output itself and keeps those lengths.)
@pytest.mark.parametrize("n", [8, 512, 4096])
def test_oracle_real_equals_reference_special_values(n):
    """fft_r2c_exec (both plan signs) of the real special rows and fft_c2r_exec of their
    spectra; non-finite rows NaN-aware.  Lengths whose inner plan ends in a factor 2 are not
    here: the reference reads uninitialised memory on them (see above)."""
    rows = [(k, T.special_real(n, k, T.seed_for(n)), T.bits_equal) for k in T.SPECIAL_KINDS]
    rows += [("non-finite", x, T.same_bits_nan_aware) for x in _nonfinite_rows(n, T.seed_for(n), real=True)]
    for kind, x, same in rows:
        for sgn in (1, -1):
            got, want = T.oracle_r2c(x, sgn, T.ORC_LEAF2_ASIS), _ref_real(n, sgn, x, False)
            assert same(got, want), ("r2c", n, sgn, kind, T.mismatches(got, want))
        X = T.oracle_r2c(x, 1)
        got, want = T.oracle_c2r(X, n, -1, T.ORC_LEAF2_ASIS), _ref_real(n, -1, X, True)
        assert same(got, want), ("c2r", n, kind, T.mismatches(got, want))


@pytest.mark.parametrize("ct", [b"linear", b"circular"])
def test_oracle_convolve_equals_reference_special_values(ct):
    """fft_convolve full / linear and full / circular at (300, 17): the signal of every special
    kind against a dense kernel (so only one operand is scaled in the huge case, and the
    product stays finite), and the kernel of every kind against a dense signal"""
    n, m = 300, 17
    for kind in T.SPECIAL_KINDS:
        for a, b in ((T.special_real(n, kind, 5), T.real_input(m, 6)), (T.real_input(n, 5), T.special_real(m, kind, 6))):
            got = T.oracle_convolve(b"full", ct, a, b)
            assert np.isfinite(got).all(), (ct, kind)
            o = np.zeros(4 * (n + m) + 8)
            ln = ref.fft_convolve(b"full", ct, T.ptr(a), n, T.ptr(b), m, T.ptr(o))
            assert ln == got.size and T.bits_equal(got, o[:ln]), (ct, kind, T.mismatches(got, o[:ln]))
    for a in _nonfinite_rows(n, 5, real=True):
        b = T.real_input(m, 6)
        got = T.oracle_convolve(b"full", ct, a, b)
        o = np.zeros(4 * (n + m) + 8)
        ln = ref.fft_convolve(b"full", ct, T.ptr(a), n, T.ptr(b), m, T.ptr(o))
        assert ln == got.size and T.same_bits_nan_aware(got, o[:ln]), (ct, "non-finite")
