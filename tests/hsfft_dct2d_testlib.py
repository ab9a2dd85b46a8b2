"""Expected values of the batched 2D cosine and sine transforms (hsfft_dct_2d_batched), composed from
hsfft_dct_testlib's 1D expectation alone: a transpose is a pure copy, so the call must equal, word
for word, that expectation applied to every row and then to every column of that result -- rows
first, then columns, for both types.  test_dct2d_cpu.py checks this builder against long-double
separable direct sums of scipy's definitions on the CPU."""
import numpy as np

import hsfft_dct_testlib as D
import hsfft_testlib as T

COS, SIN = D.COS, D.SIN
KIND_PAIRS = [(COS, COS), (COS, SIN), (SIN, COS), (SIN, SIN)]
COMBOS = [(k0, k1, t) for k0, k1 in KIND_PAIRS for t in (2, 3)]  # all eight (kind0, kind1, type)


def combo_id(c):
    return "%s%s_t%d" % ("cs"[c[0]], "cs"[c[1]], c[2])


def oracle_2d(kind0, kind1, type, x):
    """expected output for x (batch, n0, n1): kind1 along the rows, a numpy transpose, kind0 along the
    columns, a transpose back"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.ndim == 3
    b, n0, n1 = x.shape
    r = D.oracle(kind1, type, x.reshape(b * n0, n1)).reshape(b, n0, n1)
    cols = np.ascontiguousarray(r.transpose(0, 2, 1)).reshape(b * n1, n0)
    c = D.oracle(kind0, type, cols).reshape(b, n1, n0)
    return np.ascontiguousarray(c.transpose(0, 2, 1))


def direct_2d(kind0, kind1, type, x):
    """scipy's definition (norm=None) of the transform of one image x (n0, n1) as long double: the
    separable direct sum, hsfft_dct_testlib.direct on every row, then on every column"""
    x = np.asarray(x, dtype=np.longdouble)
    n0, n1 = x.shape
    r = np.stack([D.direct(kind1, type, x[i]) for i in range(n0)])
    return np.stack([D.direct(kind0, type, r[:, j]) for j in range(n1)], axis=1)


def frobenius_err(y, ref):
    """||y - ref||_F / (eps ||ref||_F), in long double"""
    y, ref = np.asarray(y, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    den = np.sqrt(np.sum(ref * ref))
    return float(np.sqrt(np.sum((y - ref) ** 2)) / (np.finfo(np.float64).eps * den))


def images(n0, n1, batch, salt=0):
    """batch dense real images (batch, n0, n1), uniform in [-1, 1), from the suite's generator"""
    n = n0 * n1
    return T.real_input(n, T.seed_for(n) ^ salt ^ 0xDC2D, batch=batch).reshape(batch, n0, n1)


def round_trip_error(kind0, kind1, n0, n1):
    """largest error of oracle_2d(type 3) of oracle_2d(type 2) of x, divided by 4 n0 n1, against x"""
    x = images(n0, n1, 1, salt=0xA2)
    back = oracle_2d(kind0, kind1, 3, oracle_2d(kind0, kind1, 2, x)) / (4.0 * n0 * n1)
    return float(np.abs(back - x).max())
