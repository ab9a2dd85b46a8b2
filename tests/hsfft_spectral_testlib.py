"""Expected values of the batched analytic signal and of Fourier resampling (hsfft_hilbert_batched,
hsfft_resample_batched, hsfft_spectral_chunk_rows), from the pinned 1D oracle and numpy alone -- never
from the code under test.

The header's composition: S = the first n/2+1 bins of T.oracle_r2c -- the reference's fft_r2c_exec --
then the edit of the spectrum, every operation one numpy float64 ufunc on the real or on the imaginary
parts (so each add, halving and division is rounded on its own, and the division is the IEEE
quotient), then T.oracle_c2c(., -1) -- the reference's fft_exec of the inverse plan -- for the analytic
signal, or T.oracle_c2r row by row -- the reference's fft_c2r_exec -- for resampling.  The same
compositions stand here around numpy.fft, and at the end of the file the long-double direct sums of
the definitions that test_spectral_cpu.py holds both against."""
import numpy as np

import hsfft_dct_testlib as D
import hsfft_testlib as T

MAX_LEN = 1 << 30
MAX_WORDS = 1 << 40


def chunk_rows(n, m=0, chunk_mb=1024):
    """the documented chunk rule, before the clamp to the batch: the knob's bytes over a row's scratch
    bytes, 16 (n/2+1) + 16 n (the analytic signal, m == 0) or 16 (n/2+1) + 16 (m/2+1), at least 1"""
    per = 16 * (n // 2 + 1) + (16 * (m // 2 + 1) if m else 16 * n)
    return max(1, (max(chunk_mb, 1) << 20) // per)


# ---------------------------------------------------------------- the edit of the spectrum
def hilbert_spectrum(S, n):
    """Z (batch, n) from the compact bins S (batch, n/2+1): q(S[0]), q(S + S) below n/2, q(S[n/2]), +0.0 above"""
    h = n // 2
    assert S.shape[-1] == h + 1
    Z = np.zeros(S.shape[:-1] + (n,), dtype=np.complex128)
    re, im = S.real.copy(), S.imag.copy()
    with np.errstate(all="ignore"):
        re[..., 1:h] = re[..., 1:h] + re[..., 1:h]
        im[..., 1:h] = im[..., 1:h] + im[..., 1:h]
        Z.real[..., :h + 1] = re / float(n)
        Z.imag[..., :h + 1] = im / float(n)
    return Z


def resample_spectrum(S, n, m):
    """Y (batch, m/2+1) from the compact bins S (batch, n/2+1) by the header's rule"""
    assert S.shape[-1] == n // 2 + 1
    K = min(n, m) // 2
    Y = np.zeros(S.shape[:-1] + (m // 2 + 1,), dtype=np.complex128)
    re, im = S.real[..., :K + 1].copy(), S.imag[..., :K + 1].copy()
    with np.errstate(all="ignore"):
        if m > n:
            re[..., K] = 0.5 * re[..., K]
            im[..., K] = 0.5 * im[..., K]
        elif m < n:
            re[..., K] = re[..., K] + re[..., K]
        Y.real[..., :K + 1] = re / float(n)
        Y.imag[..., :K + 1] = im / float(n)
        if m < n:
            Y.imag[..., K] = 0.0  # +0.0, not a copy and not a quotient
    return Y


def _rows(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.ndim == 2 and x.shape[1] >= 2 and x.shape[1] % 2 == 0
    return x


def oracle_hilbert(x, flags=0):
    """expected hsfft_hilbert_batched of the rows x (batch, n): (batch, n) complex128"""
    x = _rows(x)
    n = x.shape[1]
    S = T.oracle_r2c(x, 1, flags)[:, :n // 2 + 1]
    return T.oracle_c2c(hilbert_spectrum(S, n), -1, flags)


def oracle_resample(x, m, flags=0):
    """expected hsfft_resample_batched of the rows x (batch, n): (batch, m) float64"""
    x = _rows(x)
    n = x.shape[1]
    Y = resample_spectrum(T.oracle_r2c(x, 1, flags)[:, :n // 2 + 1], n, m)
    bins = np.zeros(m, dtype=np.complex128)  # the oracle's c2r takes a row of m words and reads m/2+1
    out = np.empty((x.shape[0], m))
    for b in range(x.shape[0]):
        bins[:m // 2 + 1] = Y[b]
        out[b] = T.oracle_c2r(bins, m, -1, flags)
    return out


def numpy_hilbert(x):
    """the same composition around numpy.fft"""
    x = _rows(x)
    n = x.shape[1]
    return np.fft.ifft(hilbert_spectrum(np.fft.rfft(x, axis=-1), n), axis=-1, norm="forward")


def numpy_resample(x, m):
    x = _rows(x)
    n = x.shape[1]
    return np.fft.irfft(resample_spectrum(np.fft.rfft(x, axis=-1), n, m), n=m, axis=-1, norm="forward")


def rows(n, batch, salt=0):
    """batch dense real rows (batch, n), uniform in [-1, 1), from the suite's generator"""
    return T.real_input(n, T.seed_for(n) ^ salt ^ 0x5BEC, batch=batch).reshape(batch, n)


# ---------------------------------------------------------------- direct sums in long double
def _unit(n):
    """cos and sin of 2 pi t / n for t < n in long double"""
    ang = 2 * D._PI_LD * np.arange(n, dtype=np.longdouble) / np.longdouble(n)
    return np.cos(ang), np.sin(ang)


def _forward_bins(x, count):
    """X[k] = sum_j x[j] exp(-2 pi i k j / n) for k < count, the angle reduced exactly by k j mod n"""
    n = x.size
    c, s = _unit(n)
    j = np.arange(n, dtype=np.int64)
    X = np.empty(count, dtype=np.clongdouble)
    for k in range(count):
        t = (k * j) % n
        X[k] = np.sum(x * c[t]) - 1j * np.sum(x * s[t])
    return X


def direct_hilbert(x):
    """the analytic signal of one row by its definition, z[j] = (1/n) sum_k g_k X[k] exp(+2 pi i j k / n)
    with g = 1 at k = 0 and k = n/2, 2 between and 0 above, in long double"""
    x = np.asarray(x, dtype=np.longdouble)
    n = x.size
    h = n // 2
    X = _forward_bins(x, h + 1)
    g = np.full(h + 1, 2, dtype=np.longdouble)
    g[0] = g[h] = 1
    G = X * g
    c, s = _unit(n)
    k = np.arange(h + 1, dtype=np.int64)
    z = np.empty(n, dtype=np.clongdouble)
    for j in range(n):
        t = (j * k) % n
        z[j] = np.sum(G * (c[t] + 1j * s[t]))
    return z / np.longdouble(n)


def direct_resample(x, m):
    """scipy.signal.resample(x, m) of one real row by its definition in long double: the bins below K =
    min(n, m)/2 kept, the bin K kept (m == n), halved (m > n) or folded with its mirror into the new
    Nyquist bin, 2 Re X[K] (m < n); y[j] = (1/n) (Y[0] + 2 sum_{0<k<m/2} Re(Y[k] w^jk) + Y[m/2] (-1)^j)"""
    x = np.asarray(x, dtype=np.longdouble)
    n = x.size
    K, hm = min(n, m) // 2, m // 2
    Y = np.zeros(hm + 1, dtype=np.clongdouble)
    Y[:K + 1] = _forward_bins(x, K + 1)
    if m > n:
        Y[K] = Y[K] / 2
    elif m < n:
        Y[K] = 2 * Y[K].real
    w = np.full(hm + 1, 2, dtype=np.longdouble)
    w[0] = w[hm] = 1
    yr, yi = Y.real * w, Y.imag * w
    yi[0] = yi[hm] = 0  # a real row has no use for them
    c, s = _unit(m)
    k = np.arange(hm + 1, dtype=np.int64)
    y = np.empty(m, dtype=np.longdouble)
    for j in range(m):
        t = (j * k) % m
        y[j] = np.sum(yr * c[t] - yi * s[t])
    return y / np.longdouble(n)


def err_units(got, want):
    """T.normwise_err of got against the long-double `want`: max |got - want| / (eps max |want|)"""
    want = np.asarray(want)
    kind = np.clongdouble if np.iscomplexobj(want) else np.longdouble
    return T.normwise_err(np.asarray(got).astype(kind), want)
