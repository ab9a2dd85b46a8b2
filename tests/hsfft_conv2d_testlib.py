"""Expected values of the batched 2D convolution (hsfft_convolve_2d_shape,
hsfft_convolve_2d_batched), composed from hsfft_r2d_testlib.oracle_r2c_2d / oracle_c2r_2d -- the
pinned 1D oracle on rows and columns -- and numpy alone: np.zeros padding, the spectral product on
separate float64 arrays so that every numpy operation rounds once (not numpy's complex multiply),
one division by float(P0 * P1) and a per-axis window restated from the 1D rule.  The transposes
the library skips are pure copies, so the GPU result must equal these word for word.
test_conv2d_cpu.py pins the builder to the reference's own 1D fft_convolve (a_rows = b_rows = 1)
and checks it against a direct 2D convolution."""
import numpy as np

import hsfft_r2d_testlib as R
import hsfft_testlib as T

TYPES = ("full", "same", "valid")
CONV_TYPES = ("linear", "circular")


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def axis_rule(typ, ct, n, m):
    """(P, start, length) of one axis: the reference's 1D rule (convolve.c:84-101, :163-195)"""
    assert typ in TYPES and ct in CONV_TYPES and n >= 1 and m >= 1
    if ct == "circular":
        P = next_pow2(max(n, m))
        return P, 0, P
    clen = n + m - 1
    P = next_pow2(clen)
    if typ == "full":
        return P, 0, clen
    if typ == "same":
        return P, (clen - max(n, m)) // 2, max(n, m)
    return P, min(n, m) - 1, max(n, m) - min(n, m) + 1


def shape_rule(typ, ct, a_rows, a_cols, b_rows, b_cols):
    """(out_rows, out_cols, pad_rows, pad_cols)"""
    P0, _, l0 = axis_rule(typ, ct, a_rows, b_rows)
    P1, _, l1 = axis_rule(typ, ct, a_cols, b_cols)
    return l0, l1, P0, P1


def pad(x, P0, P1):
    """(b, n0, n1) -> (b, P0, P1), the images at the top-left of +0.0"""
    b, n0, n1 = x.shape
    out = np.zeros((b, P0, P1), dtype=np.float64)
    out[:, :n0, :n1] = x
    return out


def oracle_padded(a, b, P0, P1):
    """the unwindowed result (batch, P0, P1) of a (batch, n0, n1) and b (batch or 1, m0, m1): the
    contract of include/hsfft_gpu.h step by step"""
    A = R.oracle_r2c_2d(pad(a, P0, P1), 1, 1)
    B = R.oracle_r2c_2d(pad(b, P0, P1), 1, 1)  # a shared kernel broadcasts over the batch below
    ar, ai = np.ascontiguousarray(A.real), np.ascontiguousarray(A.imag)
    br, bi = np.ascontiguousarray(B.real), np.ascontiguousarray(B.imag)
    t1, t2 = ar * br, ai * bi
    re = t1 - t2
    t3, t4 = ar * bi, ai * br
    im = t3 + t4
    C = np.empty(A.shape, dtype=np.complex128)
    C.real, C.imag = re, im
    y = R.oracle_c2r_2d(C, P1, -1, -1)
    return y / float(P0 * P1)


def window(y, typ, ct, a_shape, b_shape):
    """the output images cut from the unwindowed result"""
    _, s0, l0 = axis_rule(typ, ct, a_shape[0], b_shape[0])
    _, s1, l1 = axis_rule(typ, ct, a_shape[1], b_shape[1])
    return np.ascontiguousarray(y[:, s0:s0 + l0, s1:s1 + l1])


def oracle_convolve_2d(typ, ct, a, b):
    """expected output (batch, out_rows, out_cols) of a (batch, n0, n1) and b (batch or 1, m0, m1)"""
    P0 = axis_rule(typ, ct, a.shape[1], b.shape[1])[0]
    P1 = axis_rule(typ, ct, a.shape[2], b.shape[2])[0]
    return window(oracle_padded(a, b, P0, P1), typ, ct, a.shape[1:], b.shape[1:])


def images(n0, n1, batch, salt=0):
    """batch dense real images (batch, n0, n1) from the suite's generator"""
    n = n0 * n1
    return T.real_input(n, T.seed_for(n) ^ salt, batch=batch).reshape(batch, n0, n1)


def direct_convolve_2d(ct, a, b, P0, P1):
    """one pair by numpy.fft on the padded size, float64: the linear result at P >= clen on both
    axes, else the circular one (both operands zero-padded to P0 x P1, periodic)"""
    return np.fft.irfft2(np.fft.rfft2(a, s=(P0, P1)) * np.fft.rfft2(b, s=(P0, P1)), s=(P0, P1))
