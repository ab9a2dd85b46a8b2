"""Expected values of the batched cosine and sine transforms (hsfft_dct_twiddles, hsfft_dct_batched),
from libm, the pinned 1D oracle and numpy alone -- never from the code under test.

The rotation table is libm's sincos called through ctypes with the header's angle formula, PI2 *
float(k) / (4.0 * float(N)); it is computed at test time, not stored, because glibc selects
CPU-specific variants.  The transforms are T.oracle_r2c -- the reference's fft_r2c_exec -- and the
oracle's c2r as hsfft_stft_testlib.oracle_c2r_frames uses it.  Permutations are numpy indexing, the
rotations numpy float64 multiplies, adds and subtracts (one ufunc each, so each is rounded on its
own), and the sign flips act on the sign bit of a uint64 view.  test_dct_cpu.py checks the
composition against long-double direct sums of scipy's definitions."""
import ctypes
import ctypes.util

import numpy as np

import hsfft_stft_testlib as S
import hsfft_testlib as T

PI2 = float("6.28318530717958647692528676655900577")  # include/highspeedFFT.h
COS, SIN = 0, 1
MAX_LEN = 1 << 30
_SIGN = np.uint64(1 << 63)

_libm = None


def _sincos():
    global _libm
    if _libm is None:
        lib = ctypes.CDLL(ctypes.util.find_library("m"))
        lib.sincos.restype = None
        lib.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        _libm = lib
    return _libm.sincos


_TABLES = {}


def table(N):
    """t[k] = c_k + i s_k for 0 <= k <= N/2, one libm sincos per word; cached, read-only"""
    if N not in _TABLES:
        f, s, c = _sincos(), ctypes.c_double(), ctypes.c_double()
        t = np.empty(N // 2 + 1, dtype=np.complex128)
        for k in range(N // 2 + 1):
            f(PI2 * float(k) / (4.0 * float(N)), ctypes.byref(s), ctypes.byref(c))
            t[k] = complex(c.value, s.value)
        t.setflags(write=False)
        _TABLES[N] = t
    return _TABLES[N]


def flip_odd(x):
    """a copy of x (..., N) with the sign bit of every odd-indexed word flipped, zeros and NaNs included"""
    y = np.array(x, dtype=np.float64)
    w = y.view(np.uint64)
    w[..., 1::2] ^= _SIGN
    return y


def permute(x):
    """v[j] = x[2j], v[N-1-j] = x[2j+1]"""
    h = x.shape[-1] // 2
    v = np.empty_like(x)
    v[..., :h] = x[..., 0::2]
    v[..., h:] = x[..., 1::2][..., ::-1]
    return v


def unpermute(y):
    """out[2j] = y[j], out[2j+1] = y[N-1-j]"""
    h = y.shape[-1] // 2
    out = np.empty_like(y)
    out[..., 0::2] = y[..., :h]
    out[..., 1::2] = y[..., h:][..., ::-1]
    return out


def oracle_dct2(x, kind=COS):
    """expected DCT-II (DST-II) of the rows x (batch, N)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.ndim == 2
    N = x.shape[1]
    h, t = N // 2, table(N)
    if kind == SIN:
        x = flip_odd(x)
    V = T.oracle_r2c(np.ascontiguousarray(permute(x)))[:, :h + 1]
    c, s = t.real[None, :], t.imag[None, :]
    with np.errstate(all="ignore"):
        re = V.real * c + V.imag * s
        im = V.imag * c - V.real * s
        out = np.empty_like(x)
        out[:, :h + 1] = 2.0 * re
        out[:, h + 1:] = (-2.0 * im[:, 1:h])[:, ::-1]
    return np.ascontiguousarray(out[:, ::-1]) if kind == SIN else out


def oracle_dct3(X, kind=COS):
    """expected DCT-III (DST-III) of the rows X (batch, N)"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    assert X.ndim == 2
    N = X.shape[1]
    h, t = N // 2, table(N)
    if kind == SIN:
        X = np.ascontiguousarray(X[:, ::-1])
    c, s = t.real[None, 1:], t.imag[None, 1:]
    a, b = X[:, 1:h + 1], X[:, N - 1:h - 1:-1]  # X[k] and X[N-k] for k = 1..h
    V = np.empty((X.shape[0], h + 1), dtype=np.complex128)
    V.real[:, 0], V.imag[:, 0] = X[:, 0], 0.0
    with np.errstate(all="ignore"):
        V.real[:, 1:] = a * c + b * s
        V.imag[:, 1:] = a * s - b * c
    out = unpermute(S.oracle_c2r_frames(V, N))
    return flip_odd(out) if kind == SIN else out


def oracle(kind, type, x):
    return (oracle_dct2 if type == 2 else oracle_dct3)(x, kind)


def rows(N, batch, salt=0):
    """batch dense real rows (batch, N), uniform in [-1, 1), from the suite's generator"""
    return T.real_input(N, T.seed_for(N) ^ salt ^ 0xDC7, batch=batch).reshape(batch, N)


# ---------------------------------------------------------------- direct sums in long double
_PI_LD = np.longdouble("3.14159265358979323846264338327950288")


def direct(kind, type, x):
    """scipy's definition (norm=None) of the transform of one row x by a long-double direct sum, the
    angle reduced exactly by integers: pi m / 2N with m = k (2n+1) mod 4N (k + 1 for the sines)"""
    x = np.asarray(x, dtype=np.longdouble)
    N = x.size
    ang = _PI_LD * np.arange(4 * N, dtype=np.longdouble) / np.longdouble(2 * N)
    tab = np.sin(ang) if kind == SIN else np.cos(ang)
    odd = 2 * np.arange(N, dtype=np.int64) + 1
    out = np.empty(N, dtype=np.longdouble)
    if type == 2:
        for k in range(N):
            out[k] = 2 * np.sum(x * tab[((k + kind) * odd) % (4 * N)])
    else:
        w = np.full(N, 2, dtype=np.longdouble)
        w[N - 1 if kind == SIN else 0] = 1
        kk = np.arange(N, dtype=np.int64) + kind
        xw = x * w
        for n in range(N):
            out[n] = np.sum(xw * tab[(kk * (2 * n + 1)) % (4 * N)])
    return out


def round_trip_errors(N):
    """(x, largest error of oracle_dct3(oracle_dct2(x)) / 2N against x, largest error of the
    reference's own r2c -> c2r -> / N round trip on the permuted row)"""
    x = rows(N, 1, salt=0xA1)
    back = oracle_dct3(oracle_dct2(x)) / (2.0 * N)
    v = np.ascontiguousarray(permute(x))
    rt = S.oracle_c2r_frames(np.ascontiguousarray(T.oracle_r2c(v)[:, :N // 2 + 1]), N) / float(N)
    return x[0], float(np.abs(back - x).max()), float(np.abs(rt - v).max())
