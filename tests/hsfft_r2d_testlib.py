"""Expected values of the 2D real transforms (hsfft_r2c_2d, hsfft_r2c_2d_full, hsfft_c2r_2d),
composed from the pinned 1D oracle alone: the oracle's r2c / c2r on the rows
(hsfft_testlib.oracle_r2c / oracle_c2r) and its c2c on the n1/2+1 columns of the half spectrum
(hsfft_2d_testlib.oracle_columns).  The transposes in between are pure copies and the full
layout's mirror half is a copy with the sign bit of the imaginary part flipped, so the GPU result
must equal these word for word.  test_r2d_cpu.py checks the builders against numpy on the CPU."""
import numpy as np

import hsfft_2d_testlib as D
import hsfft_testlib as T


def oracle_r2c_2d(x, s0, s1, flags=0):
    """half spectra (b, n0, n1/2+1) of the real images x (b, n0, n1): bins 0..n1/2 of the oracle's
    r2c (sign s1) on every row, then its c2c (sign s0) on every column of that"""
    b, n0, n1 = x.shape
    w = n1 // 2 + 1
    rows = T.oracle_r2c(np.ascontiguousarray(x, dtype=np.float64).reshape(b * n0, n1), s1, flags)[:, :w]
    return D.oracle_columns(np.ascontiguousarray(rows).reshape(b, n0, w), s0, flags)


def complete_full(half, n1):
    """the full layout (b, n0, n1) of half spectra (b, n0, n1/2+1), completed by indexing: column
    k1 > n1/2 of row k0 is column n1-k1 of row (n0-k0) % n0 with the sign bit of the imaginary
    part flipped (a negation of the float64 word, not a complex conjugate: zeros and NaNs flip too)"""
    b, n0, w = half.shape
    h = n1 // 2
    assert w == h + 1
    full = np.empty((b, n0, n1), dtype=np.complex128)
    full[:, :, :w] = half
    k0 = (n0 - np.arange(n0)) % n0
    k1 = n1 - np.arange(w, n1)
    full[:, :, w:] = half[:, k0][:, :, k1]
    f64 = full.view(np.float64).reshape(b, n0, n1, 2)
    f64[:, :, w:, 1] = -f64[:, :, w:, 1]
    return full


def oracle_r2c_2d_full(x, s0, s1, flags=0):
    """the full-layout spectrum (b, n0, n1) of the real images x"""
    return complete_full(oracle_r2c_2d(x, s0, s1, flags), x.shape[2])


def oracle_c2r_2d(X, n1, s0, s1, flags=0):
    """real images (b, n0, n1) of the half spectra X (b, n0, n1/2+1): the oracle's c2c (sign s0) on
    every column, then its c2r (sign s1) on every row.  The oracle's 1D c2r takes a row in the
    reference layout (n1 bins) and reads bins 0..n1/2 of it, so each row is zero-padded to n1 bins."""
    b, n0, w = X.shape
    assert w == n1 // 2 + 1
    cols = D.oracle_columns(np.ascontiguousarray(X, dtype=np.complex128), s0, flags).reshape(b * n0, w)
    padded = np.zeros((b * n0, n1), dtype=np.complex128)
    padded[:, :w] = cols
    lib = T.oracle()
    rp = lib.orc_real_create(n1, s1, flags)  # T.oracle_c2r row by row, on one plan
    out = np.zeros((b * n0, n1), dtype=np.float64)
    for r in range(b * n0):
        lib.orc_c2r(rp, T.ptr(padded[r]), T.ptr(out[r]))
    lib.orc_real_destroy(rp)
    return out.reshape(b, n0, n1)


def real_images(n0, n1, batch, salt=0):
    """batch dense real images of n0 x n1 from the suite's generator"""
    n = n0 * n1
    return T.real_input(n, T.seed_for(n) ^ salt, batch=batch).reshape(batch, n0, n1)
