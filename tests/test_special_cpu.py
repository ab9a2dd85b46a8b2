"""CPU: the conditions under which the special-value GPU tests (test_gpu_values.py) assert
something, pinned from the oracle alone so that they are checked wherever the suite runs.

A test on structured inputs is vacuous if the oracle's output does not contain what the input
was chosen for: exact zeros (constant, alternating and comb rows), negative zeros (the field of
random signed zeros through Bluestein), non-zero subnormal / small results (tiny), finite ones
(huge), and a partial mix of NaN words (one infinite element)."""
import numpy as np
import pytest

import hsfft_testlib as T


def test_helpers_construct_what_they_name():
    n = 12
    neg = np.signbit
    x = T.special_inputs(n, "alt", 1)
    assert x[0] == 1 and x[1] == -1 and not neg(x[0].imag) and neg(x[1].imag) and x[1].imag == 0
    x = T.special_inputs(n, "comb4", 1)
    assert x[0] == 0.75 - 0.25j and x[4] == x[0] and neg(x[1].real) and not neg(x[1].imag) and x[1] == 0
    assert np.flatnonzero(T.special_inputs(15, "comb4", 1)).tolist() == [0, 3, 6, 9, 12]
    assert np.flatnonzero(T.special_inputs(35, "comb4", 1)).tolist() == [0, 5, 10, 15, 20, 25, 30]
    w = T.special_inputs(n, "negzero", 1).view(np.uint64)
    assert (w == np.uint64(1 << 63)).all()
    z = T.special_inputs(4096, "zfield", 7).view(np.float64)
    assert (z == 0).all() and 0.4 < neg(z).mean() < 0.6
    x = T.special_inputs(n, "impulse", 1)
    assert x[1] == -1 and x[n - 1] == 1j and np.count_nonzero(x) == 2 and not neg(x.view(np.float64)[[0, 1, 3]]).any()
    x = T.special_inputs(n, "realonly", 3)
    assert T.bits_equal(x.real, T.complex_input(n, 3).real)
    assert neg(x.imag).tolist() == [j % 3 == 0 for j in range(n)] and (x.imag == 0).all()
    t = T.special_inputs(n, "tiny", 3).view(np.float64)
    assert (t != 0).all() and (np.abs(t) < np.finfo(np.float64).tiny).all()  # subnormal inputs
    assert np.abs(T.special_inputs(n, "huge", 3)).max() > 2.0 ** 999
    for k in T.SPECIAL_KINDS:
        assert T.bits_equal(T.special_real(n, k, 3), T.special_inputs(n, k, 3).real.copy()), k
        assert np.isfinite(T.special_inputs(n, k, 3).view(np.float64)).all(), k


def test_same_bits_nan_aware():
    a = np.array([1.0, -0.0, np.inf, np.nan, 2.0])
    b = a.copy()
    b.view(np.uint64)[3] ^= np.uint64((1 << 63) | 5)  # another NaN: sign and payload differ
    assert T.nan_words(b).tolist() == [False, False, False, True, False]
    assert T.same_bits_nan_aware(a, b) and not T.bits_equal(a, b)
    for i, v in ((1, 0.0), (2, -np.inf), (4, np.nan), (3, np.inf), (0, np.nextafter(1.0, 2.0))):
        c = b.copy()
        c[i] = v
        assert not T.same_bits_nan_aware(a, c), (i, v)
    assert not T.same_bits_nan_aware(a, b[:4])


def test_oracle_keeps_subnormals():
    x = np.zeros(8, dtype=np.complex128)
    x[0] = 5e-324
    assert np.count_nonzero(T.oracle_c2c(x, 1)) == 8


@pytest.mark.parametrize("n", T.ZERO_RICH_SIZES)
def test_structured_rows_give_exact_positive_zeros(n):
    """const, alt and comb4: at least half of the output words are exact zeros, all of them +0
    (so one flipped subtraction shows in thousands of words)"""
    for kind in ("const", "alt", "comb4"):
        for sgn in (1, -1):
            y = T.oracle_c2c(T.special_inputs(n, kind, T.seed_for(n)), sgn).view(np.float64)
            assert T.zero_words(y) >= n, (n, kind, sgn, T.zero_words(y))
            assert not np.signbit(y[y == 0]).any(), (n, kind, sgn)


@pytest.mark.parametrize("n", [97, 5003])
def test_signed_zero_field_through_bluestein_gives_negative_zeros(n):
    y = T.oracle_c2c(T.special_inputs(n, "zfield", T.seed_for(n)), 1).view(np.float64)
    negz = int(np.count_nonzero(np.signbit(y) & (y == 0)))
    assert T.zero_words(y) >= n and 0 < negz < T.zero_words(y), (n, T.zero_words(y), negz)


@pytest.mark.parametrize("n", [8, 97, 1000, 5003, 12600, 65536, 99991])
def test_tiny_has_no_zero_and_huge_is_finite(n):
    for sgn in (1, -1):
        y = T.oracle_c2c(T.special_inputs(n, "tiny", T.seed_for(n)), sgn)
        assert T.zero_words(y) == 0, (n, sgn)
        y = T.oracle_c2c(T.special_inputs(n, "huge", T.seed_for(n)), sgn)
        assert np.isfinite(y.view(np.float64)).all(), (n, sgn)


def _partial(n, idx):
    x = T.nonfinite_rows(n, idx, T.seed_for(n))
    return all(0.01 <= T.nan_fraction(T.oracle_c2c(x[r], sgn)) <= 0.99 for r in (0, 1) for sgn in (1, -1))


def test_nonfinite_index_table():
    """every entry of NONFINITE_INDEX is the first candidate index at which one infinite element
    gives a partial mix of NaN words; the lengths left out have no such candidate; the finite
    row of nonfinite_rows stays finite"""
    for n, idx in T.NONFINITE_INDEX.items():
        good = [i for i in T.nonfinite_candidates(n) if _partial(n, i)]
        assert good and good[0] == idx, (n, idx, good)
        assert np.isfinite(T.oracle_c2c(T.nonfinite_rows(n, idx, T.seed_for(n))[2], 1).view(np.float64)).all()
    for n in T.NONFINITE_LEFT_OUT:
        assert not any(_partial(n, i) for i in T.nonfinite_candidates(n)), n


def test_skip_probe_index():
    """the probe index of the plans the non-finite GPU test adds for it, and its condition: the
    oracle's rows keep infinite words (at least 8) that a wrongly multiplied k = 0 twiddle would
    turn into NaN"""
    want = {12: 1, 20: 1, 28: 1, 60: 6, 100: 6, 500: 31, 1000: 48, 1372: 57, 3000: 248, 5000: 248, 12600: 344,
            64: 0, 512: 0, 97: 0, 5003: 0}
    for n, idx in want.items():
        assert T.skip_probe_index(n) == idx, (n, T.skip_probe_index(n))
        if idx:
            x = T.nonfinite_rows(n, idx, T.seed_for(n) ^ 1)
            for sgn in (1, -1):
                for r in (0, 1):
                    y = T.oracle_c2c(x[r], sgn)
                    assert T.inf_words(y) >= 8 and T.nan_fraction(y) < 1, (n, sgn, r, T.inf_words(y))
