"""Expected values of the batched chirp-z transform (hsfft_czt_shape, hsfft_czt_tables,
hsfft_czt_batched, hsfft_czt_real_batched), from libm, the pinned 1D oracle and numpy alone -- never
from the code under test.

The two phase tables follow the header's reduction: red(a, b) = fmod(p, 2.0) + e with p = a * b
rounded and e the product's exact error.  Python 3.10 has no math.fma, so e is formed in rationals,
Fraction(a) * Fraction(b) - Fraction(p), and converted to a float, and the conversion is asserted to
be exact.  Every word is one libm sincos called through ctypes, as in hsfft_dct_testlib, computed at
test time.  The transforms in the middle are T.oracle_c2c(., 1) and T.oracle_c2c(., -1) at the
padded length L -- the reference's fft_exec -- and every other operation is one numpy float64 ufunc,
so each is rounded on its own; the sign flip acts on the sign bit of a uint64 view.
test_czt_cpu.py checks the composition against the long-double direct sum of the definition that
stands at the end of this file."""
import ctypes
import math
from fractions import Fraction

import numpy as np

import hsfft_dct4_testlib as F4
import hsfft_dct_testlib as D
import hsfft_testlib as T

PI2 = D.PI2
MAX_SUM = 1 << 26


def shape_L(n, m):
    """max(2, the power of two >= n + m - 1)"""
    L = 2
    while L < n + m - 1:
        L *= 2
    return L


def red(a, b):
    """a b mod 2 in half-turns, as the header defines it; a, b floats"""
    p = a * b
    e = Fraction(a) * Fraction(b) - Fraction(p)
    ef = float(e)
    assert Fraction(ef) == e, (a, b)
    return math.fmod(p, 2.0) + ef


_TABLES = {}


def tables(n, m, f0, df):
    """(pre, chirp) as complex128, c + i s: n and max(n, m) words; cached, read-only"""
    key = (n, m, float(f0).hex(), float(df).hex())
    if key not in _TABLES:
        f, s, c = D._sincos(), ctypes.c_double(), ctypes.c_double()
        K = max(n, m)
        pre, chirp = np.empty(n, dtype=np.complex128), np.empty(K, dtype=np.complex128)
        for j in range(K):
            ph = red(float(j) * float(j), df)
            f(PI2 * (0.5 * ph), ctypes.byref(s), ctypes.byref(c))
            chirp[j] = complex(c.value, s.value)
            if j < n:
                f(PI2 * (0.5 * (red(float(2 * j), f0) + ph)), ctypes.byref(s), ctypes.byref(c))
                pre[j] = complex(c.value, s.value)
        pre.setflags(write=False)
        chirp.setflags(write=False)
        _TABLES[key] = (pre, chirp)
    return _TABLES[key]


def compose(x, m, f0, df, fwd, inv):
    """the header's composition on the rows x (batch, n), float64 or complex128, around the given
    forward and unnormalised inverse transforms of rows of L: (batch, m) complex128"""
    x = np.ascontiguousarray(x)
    assert x.ndim == 2 and x.dtype in (np.float64, np.complex128)
    batch, n = x.shape
    L = shape_L(n, m)
    pre, chirp = tables(n, m, f0, df)
    u = np.zeros((batch, L), dtype=np.complex128)
    v = np.zeros(L, dtype=np.complex128)
    v[:m] = chirp[:m]
    if n > 1:
        v[L - n + 1:] = chirp[1:n][::-1]  # v[L-j] = chirp[j]
    with np.errstate(all="ignore"):
        c, s = pre.real[None, :], pre.imag[None, :]
        if x.dtype == np.float64:
            u.real[:, :n] = x * c
            u.imag[:, :n] = F4.flip(x * s)
        else:
            u.real[:, :n] = x.real * c + x.imag * s
            u.imag[:, :n] = x.imag * c - x.real * s
        V = fwd(v)[None, :]
        U = fwd(u)
        P = np.empty_like(U)
        P.real = U.real * V.real - U.imag * V.imag
        P.imag = U.real * V.imag + U.imag * V.real
        y = inv(P)
        dre, dim = y.real[:, :m] / float(L), y.imag[:, :m] / float(L)
        c, s = chirp.real[None, :m], chirp.imag[None, :m]
        X = np.empty((batch, m), dtype=np.complex128)
        X.real = dre * c + dim * s
        X.imag = dim * c - dre * s
    return X


def oracle_czt(x, m, f0, df, flags=0):
    """expected hsfft_czt_batched / hsfft_czt_real_batched (by the dtype) of the rows x (batch, n)"""
    return compose(x, m, f0, df, lambda a: T.oracle_c2c(a, 1, flags), lambda a: T.oracle_c2c(a, -1, flags))


def numpy_czt(x, m, f0, df):
    """the same composition with numpy.fft in place of the oracle's transforms"""
    return compose(x, m, f0, df, lambda a: np.fft.fft(a, axis=-1), lambda a: np.fft.ifft(a, axis=-1, norm="forward"))


def real_rows(n, batch, salt=0):
    """batch dense real rows (batch, n), uniform in [-1, 1), from the suite's generator"""
    return T.real_input(n, T.seed_for(n) ^ salt ^ 0xC27, batch=batch).reshape(batch, n)


def complex_rows(n, batch, salt=0):
    return T.complex_input(n, T.seed_for(n) ^ salt ^ 0xC27C, batch=batch).reshape(batch, n)


# ---------------------------------------------------------------- direct sum in long double
def _ld(t):
    """the rational t as a long double: its double rounding plus the double rounding of the rest"""
    hi = float(t)
    return np.longdouble(hi) + np.longdouble(float(t - Fraction(hi)))


def direct_czt(x, m, f0, df):
    """X[k] = sum_j x[j] exp(-2 pi i j (f0 + k df)) of one row in long double; every angle j (f0 + k
    df) mod 1 is formed exactly in rationals before the long-double cos and sin"""
    x = np.asarray(x)
    n = x.size
    xr, xi = x.real.astype(np.longdouble), x.imag.astype(np.longdouble)
    F0, DF = Fraction(float(f0)), Fraction(float(df))
    out = np.empty(m, dtype=np.clongdouble)
    for k in range(m):
        fk = (F0 + k * DF) % 1
        ang = 2 * F4._PI_LD * np.array([_ld((j * fk) % 1) for j in range(n)], dtype=np.longdouble)
        c, s = np.cos(ang), np.sin(ang)
        out[k] = np.sum(xr * c + xi * s) + 1j * np.sum(xi * c - xr * s)
    return out


def rel_err(got, want):
    """max |got - want| / max |want| in long double, as a float"""
    want = np.asarray(want, dtype=np.clongdouble)
    den = np.abs(want).max()
    return float(np.abs(np.asarray(got).astype(np.clongdouble) - want).max() / den)
