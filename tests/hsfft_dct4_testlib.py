"""Expected values of the type-IV cosine and sine transforms and of the MDCT / IMDCT built on them
(hsfft_dct4_twiddles, hsfft_dct4_batched, hsfft_mdct_batched, hsfft_imdct_batched), from libm, the
pinned 1D oracle and numpy alone -- never from the code under test.

The rotation table is libm's sincos called through ctypes with the header's angle formula, PI2 *
float(8 j + 1) / (16.0 * float(N)), computed at test time as in hsfft_dct_testlib.  The transform in
the middle is T.oracle_c2c(z, 1) -- the reference's fft_exec of fft_init(N/2, 1).  Pairings, folds
and unfolds are numpy indexing, the rotations, window products, divisions and overlap-adds numpy
float64 ufuncs (one per operation, so each is rounded on its own), and the sign flips act on the
sign bit of a uint64 view.  test_dct4_cpu.py checks the compositions against long-double direct
sums of the definitions."""
import ctypes

import numpy as np

import hsfft_dct_testlib as D
import hsfft_testlib as T

PI2 = D.PI2
COS, SIN = D.COS, D.SIN
MAX_LEN = 1 << 30
_SIGN = np.uint64(1 << 63)

_TABLES = {}


def table(N):
    """t[j] = c_j + i s_j for 0 <= j < N/2, one libm sincos per word; cached, read-only"""
    if N not in _TABLES:
        f, s, c = D._sincos(), ctypes.c_double(), ctypes.c_double()
        t = np.empty(N // 2, dtype=np.complex128)
        for j in range(N // 2):
            f(PI2 * float(8 * j + 1) / (16.0 * float(N)), ctypes.byref(s), ctypes.byref(c))
            t[j] = complex(c.value, s.value)
        t.setflags(write=False)
        _TABLES[N] = t
    return _TABLES[N]


def flip(x):
    """a copy of x with every sign bit flipped, zeros and NaNs included"""
    y = np.array(x, dtype=np.float64)
    y.view(np.uint64)[...] ^= _SIGN
    return y


def oracle_dct4(x, kind=COS, g=2.0):
    """expected DCT-IV (DST-IV) of the rows x (batch, N) with the gain g"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.ndim == 2 and x.shape[1] % 2 == 0
    N = x.shape[1]
    h, t = N // 2, table(N)
    if kind == SIN:
        x = np.ascontiguousarray(x[:, ::-1])
    a, b = x[:, 0::2], x[:, ::-1][:, 0::2]  # x[2j] and x[N-1-2j]
    c, s = t.real[None, :], t.imag[None, :]
    z = np.empty((x.shape[0], h), dtype=np.complex128)
    with np.errstate(all="ignore"):
        z.real = a * c + b * s
        z.imag = b * c - a * s
        Z = T.oracle_c2c(z, 1)
        re = Z.real * c + Z.imag * s
        im = Z.imag * c - Z.real * s
        out = np.empty_like(x)
        out[:, 0::2] = g * re
        out[:, 1::2] = ((-g) * im)[:, ::-1]  # out[N-1-2k]
    return D.flip_odd(out) if kind == SIN else out


def rows(N, batch, salt=0):
    """batch dense real rows (batch, N), uniform in [-1, 1), from the suite's generator"""
    return T.real_input(N, T.seed_for(N) ^ salt ^ 0xDC74, batch=batch).reshape(batch, N)


# ---------------------------------------------------------------- MDCT / IMDCT
def sine_window(N):
    """w[m] = sin(pi (m + 1/2) / 2N), m < 2N: w[m]^2 + w[m+N]^2 = 1 (Princen-Bradley)"""
    return np.sin(np.pi * (np.arange(2 * N) + 0.5) / (2 * N))


def nframes_of(n, N, pad):
    return n // N + 1 if pad else n // N - 1


def fold(p):
    """u[i] = (-p[3q-1-i]) - p[3q+i] for i < q, p[i-q] - p[3q-1-i] for q <= i < N; p (..., 2N), q = N/2"""
    q = p.shape[-1] // 4
    u = np.empty(p.shape[:-1] + (2 * q,), dtype=np.float64)
    with np.errstate(all="ignore"):
        u[..., :q] = flip(p[..., 2 * q:3 * q][..., ::-1]) - p[..., 3 * q:]
        u[..., q:] = p[..., :q] - p[..., q:2 * q][..., ::-1]
    return u


def unfold(v):
    """y[m] = v[m+q] for m < q, -v[3q-1-m] for q <= m < 3q, -v[m-3q] for 3q <= m < 2N; v (..., N)"""
    q = v.shape[-1] // 2
    y = np.empty(v.shape[:-1] + (4 * q,), dtype=np.float64)
    y[..., :q] = v[..., q:]
    y[..., q:3 * q] = flip(v[..., ::-1])
    y[..., 3 * q:] = flip(v[..., :q])
    return y


def frames(x, N, pad):
    """the frames of 2N samples, N apart, of the rows x (batch, n): (batch, nframes, 2N), zeros outside"""
    batch, n = x.shape
    lpad = N if pad else 0
    xp = np.zeros((batch, n + 2 * lpad))
    xp[:, lpad:lpad + n] = x
    nf = nframes_of(n, N, pad)
    return np.stack([xp[:, f * N:f * N + 2 * N] for f in range(nf)], axis=1)


def oracle_mdct(x, N, window=None, pad=False):
    """expected hsfft_mdct_batched of the rows x (batch, n): (batch, nframes, N)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    p = frames(x, N, pad)
    with np.errstate(all="ignore"):
        if window is not None:
            p = p * window[None, None, :]
        u = fold(p)
    return oracle_dct4(u.reshape(-1, N), COS, 1.0).reshape(u.shape)


def oracle_imdct(X, window=None, pad=False):
    """expected hsfft_imdct_batched of the coefficients X (batch, nframes, N): (batch, n)"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    batch, nf, N = X.shape
    lpad = N if pad else 0
    n = (nf + 1) * N - 2 * lpad
    v = oracle_dct4(X.reshape(-1, N), COS, 1.0).reshape(X.shape)
    with np.errstate(all="ignore"):
        t = unfold(v) / float(N // 2)
        if window is not None:
            t = t * window[None, None, :]
        full = np.empty((batch, nf + 1, N))
        full[:, 0] = t[:, 0, :N]  # a single covering frame gives its term alone
        full[:, nf] = t[:, nf - 1, N:]
        full[:, 1:nf] = t[:, :nf - 1, N:] + t[:, 1:, :N]  # the earlier frame's term, then the later one's
    return np.ascontiguousarray(full.reshape(batch, (nf + 1) * N)[:, lpad:lpad + n])


# ---------------------------------------------------------------- direct sums in long double
_PI_LD = np.longdouble("3.14159265358979323846264338327950288")


def _tab(N, kind=COS):
    """cos (sin) of pi m / 4N for 0 <= m < 8N: the angles reduced exactly by integers index it"""
    ang = _PI_LD * np.arange(8 * N, dtype=np.longdouble) / np.longdouble(4 * N)
    return np.sin(ang) if kind == SIN else np.cos(ang)


def direct_dct4(kind, x):
    """scipy's type-IV definition (norm=None) of one row: X[k] = 2 sum_n x[n] cos(pi (2k+1)(2n+1) / 4N),
    the angle index (2k+1)(2n+1) mod 8N"""
    x = np.asarray(x, dtype=np.longdouble)
    N = x.size
    tab, odd = _tab(N, kind), 2 * np.arange(N, dtype=np.int64) + 1
    return np.array([2 * np.sum(x * tab[((2 * k + 1) * odd) % (8 * N)]) for k in range(N)], dtype=np.longdouble)


def direct_mdct(u):
    """X[k] = sum_{m<2N} u[m] cos(pi/N (m + 1/2 + N/2)(k + 1/2)) of one frame u of 2N samples: the
    angle is pi (2m+1+N)(2k+1) / 4N"""
    u = np.asarray(u, dtype=np.longdouble)
    N = u.size // 2
    tab, mm = _tab(N), 2 * np.arange(2 * N, dtype=np.int64) + 1 + N
    return np.array([np.sum(u * tab[(mm * (2 * k + 1)) % (8 * N)]) for k in range(N)], dtype=np.longdouble)


def direct_imdct(X):
    """y[m] = sum_{k<N} X[k] cos(pi/N (m + 1/2 + N/2)(k + 1/2)) for m < 2N of one frame's coefficients"""
    X = np.asarray(X, dtype=np.longdouble)
    N = X.size
    tab, kk = _tab(N), 2 * np.arange(N, dtype=np.int64) + 1
    return np.array([np.sum(X * tab[((2 * m + 1 + N) * kk) % (8 * N)]) for m in range(2 * N)], dtype=np.longdouble)


def c2c_round_trip_error(h):
    """largest error of the reference's own c2c forward -> inverse -> / h round trip at length h"""
    z = T.complex_input(h, T.seed_for(h) ^ 0xA14)
    back = T.oracle_c2c(T.oracle_c2c(z, 1), -1) / float(h)
    return float(np.abs(back - z).max())


def round_trip_errors(N, kind=COS):
    """(x, largest error of oracle_dct4(oracle_dct4(x)) / 2N against x, the c2c round-trip error at N/2)"""
    x = rows(N, 1, salt=0xA1)
    back = oracle_dct4(oracle_dct4(x, kind), kind) / (2.0 * N)
    return x[0], float(np.abs(back - x).max()), c2c_round_trip_error(N // 2)
