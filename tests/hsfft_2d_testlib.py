"""Expected values of the 2D and column transforms, composed from the pinned 1D oracle alone
(hsfft_testlib.oracle_c2c): a transpose is a pure copy, so hsfft_exec_2d must equal, word for
word, the oracle applied to every row and then to every column of that result.
test_2d_cpu.py checks this builder against numpy on the CPU."""
import numpy as np

import hsfft_testlib as T


def oracle_columns(x, s0, flags=0):
    """the oracle's transform of sign s0 along axis 1 of x (b, n0, n1): every column of every image"""
    b, n0, n1 = x.shape
    cols = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(b * n1, n0)
    return np.ascontiguousarray(T.oracle_c2c(cols, s0, flags).reshape(b, n1, n0).transpose(0, 2, 1))


def oracle_2d(x, s0, s1, flags=0):
    """rows (sign s1) then columns (sign s0) of x (b, n0, n1); flags: the oracle's flavour (0 is
    the reference as it is, which every GPU comparison uses)"""
    b, n0, n1 = x.shape
    exp = T.oracle_c2c(np.ascontiguousarray(x).reshape(b * n0, n1), s1, flags).reshape(b, n0, n1)
    return oracle_columns(exp, s0, flags)


def images(n0, n1, batch, salt=0):
    """batch dense images of n0 x n1 from the suite's generator"""
    n = n0 * n1
    return T.complex_input(n, T.seed_for(n) ^ salt, batch=batch).reshape(batch, n0, n1)
