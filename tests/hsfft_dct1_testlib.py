"""Expected values of the batched type-I cosine and sine transforms (hsfft_dct1_batched,
hsfft_dct1_2d_batched), from numpy and the pinned 1D oracle alone -- never from the code under test.

The symmetric extension is numpy indexing, with np.negative for the sign of the odd extension (a
sign-bit flip: zeros and NaNs flip too); the transform is T.oracle_r2c -- the reference's
fft_r2c_exec -- on the extended row; the output is a slice of .real (cosine) or of -.imag (sine).
There is no table and no arithmetic beside the transform's own.  test_dct1_cpu.py checks the
composition against long-double direct sums of scipy's definitions."""
import numpy as np

import hsfft_stft_testlib as S
import hsfft_testlib as T

COS, SIN = 0, 1
MAX_LEN = 1 << 30  # of the extended row


def ext_len(kind, n):
    """L = 2(n-1) for the cosine transform, 2(n+1) for the sine transform"""
    return 2 * (n + 1) if kind == SIN else 2 * (n - 1)


def factor(kind, n):
    """T(T(x)) = factor x"""
    return float(ext_len(kind, n))


def extend(kind, x):
    """the even (cosine) or odd (sine) extension of the rows x (batch, n): rows of L"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    batch, n = x.shape
    L = ext_len(kind, n)
    e = np.empty((batch, L), dtype=np.float64)
    if kind == SIN:
        e[:, 0] = 0.0
        e[:, n + 1] = 0.0
        e[:, 1:n + 1] = x
        e[:, n + 2:] = np.negative(x[:, ::-1])  # e[L-1-j] = -x[j]
    else:
        e[:, :n] = x
        e[:, n:] = x[:, n - 2:0:-1]  # e[L-t] = x[t] for 1 <= t <= n-2
    return e


def chunk_rows(kind, n, chunk_mb=1024):
    """the documented chunk rule: bytes / (L x 8 + (L/2+1) x 16) rows"""
    L = ext_len(kind, n)
    return T.rows_per_chunk(chunk_mb, L * 8 + (L // 2 + 1) * 16, elem=1)


def oracle(kind, x, flags=0):
    """expected DCT-I (DST-I) of the rows x (batch, n)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.ndim == 2
    n = x.shape[1]
    with np.errstate(all="ignore"):
        Sp = T.oracle_r2c(extend(kind, x), flags=flags)
    if kind == SIN:
        return np.ascontiguousarray(np.negative(Sp.imag[:, 1:n + 1]))
    return np.ascontiguousarray(Sp.real[:, :n])


def oracle_2d(kind0, kind1, x, flags=0):
    """expected 2D transform of the images x (batch, n0, n1): the 1D expectation on every row, then on
    every column of that result"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    batch, n0, n1 = x.shape
    r = oracle(kind1, x.reshape(batch * n0, n1), flags).reshape(batch, n0, n1)
    c = oracle(kind0, np.ascontiguousarray(r.transpose(0, 2, 1)).reshape(batch * n1, n0), flags).reshape(batch, n1, n0)
    return np.ascontiguousarray(c.transpose(0, 2, 1))


def rows(n, batch, salt=0):
    """batch dense real rows (batch, n), uniform in [-1, 1), from the suite's generator"""
    return T.real_input(n, T.seed_for(n) ^ salt ^ 0xDC1, batch=batch).reshape(batch, n)


# ---------------------------------------------------------------- direct sums in long double
_PI_LD = np.longdouble("3.14159265358979323846264338327950288")


def direct(kind, x):
    """scipy's definition (norm=None) of the transform of one row x by a long-double direct sum, the
    angle reduced exactly by integers: 2 pi m / L with m = j k mod L (cosine, L = 2(n-1)) or
    (j+1)(k+1) mod L (sine, L = 2(n+1))"""
    x = np.asarray(x, dtype=np.longdouble)
    n = x.size
    L = ext_len(kind, n)
    ang = 2 * _PI_LD * np.arange(L, dtype=np.longdouble) / np.longdouble(L)
    out = np.empty(n, dtype=np.longdouble)
    if kind == SIN:
        tab, j1 = np.sin(ang), np.arange(1, n + 1, dtype=np.int64)
        for k in range(n):
            out[k] = 2 * np.sum(x * tab[(j1 * (k + 1)) % L])
    else:
        tab, j = np.cos(ang), np.arange(1, n - 1, dtype=np.int64)
        for k in range(n):
            out[k] = x[0] + (-1) ** k * x[n - 1] + 2 * np.sum(x[1:n - 1] * tab[(j * k) % L])
    return out


def round_trip_errors(kind, n):
    """(x, largest error of oracle(oracle(x)) / factor against x, largest error of the reference's own
    r2c -> c2r -> / L round trip on the extended row)"""
    x = rows(n, 1, salt=0xA1)
    L = ext_len(kind, n)
    back = oracle(kind, oracle(kind, x)) / factor(kind, n)
    e = extend(kind, x)
    rt = S.oracle_c2r_frames(np.ascontiguousarray(T.oracle_r2c(e)[:, :L // 2 + 1]), L) / float(L)
    return x[0], float(np.abs(back - x).max()), float(np.abs(rt - e).max())
