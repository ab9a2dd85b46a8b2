"""Expected values of the batched overlap-add filter (hsfft_filter_shape, hsfft_filter_batched),
from the pinned 1D oracle and numpy alone: every block goes through T.oracle_convolve -- the
reference's own fft_convolve("full", "linear") of the block and the kernel -- and the blocks are
joined by the full[g] formula of include/hsfft_gpu.h in float64 with one add per word, then cut by
the restated window rule.  test_filter_cpu.py checks that this composition is the linear
convolution and, with one block, the reference's one-shot result word for word."""
import numpy as np

import hsfft_testlib as T

TYPES = ("full", "same", "valid")

# (n, m, P): the cases of test_filter_cpu.py's yardstick check
CASES = [(9, 4, 8), (9, 1, 4), (100, 2, 2), (1000, 33, 64), (40000, 33, 4096), (40000, 1025, 4096),
         (30000, 200, 16384), (8128, 33, 4096), (8129, 33, 4096)]


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def window_rule(typ, n, m):
    """(start, length) of the output window in the full result of n + m - 1 samples"""
    assert typ in TYPES and n >= 1 and m >= 1
    clen = n + m - 1
    if typ == "full":
        return 0, clen
    if typ == "same":
        return (clen - max(n, m)) // 2, max(n, m)
    return min(n, m) - 1, max(n, m) - min(n, m) + 1


def shape_rule(typ, n, m, block=0, floor=4096):
    """(out_len, P, L, nseg), or None where the library must reject the call; `floor` is
    HSFFT_FILTER_BLOCK_MIN"""
    if typ not in TYPES or n < 1 or m < 1 or n + m - 1 > 1 << 30:
        return None
    Q = max(2, next_pow2(n + m - 1))
    if block == 0:
        P = min(max(floor, next_pow2(4 * m)), Q)
    else:
        if block < 2 or block & (block - 1) or block < m:
            return None
        P = block
    L = P - m + 1
    nseg = -(-n // L)
    if nseg > 1 and L < m - 1:
        return None
    return window_rule(typ, n, m)[1], P, L, nseg


def oracle_full(x, h, P):
    """the overlap-added full result (n + m - 1 words) of one row x and the kernel h with blocks
    padded to P"""
    n, m = x.size, h.size
    L = P - m + 1
    nseg = -(-n // L)
    assert L >= 1 and (nseg == 1 or L >= m - 1)
    v = []
    for s in range(nseg):
        u = np.zeros(L)
        seg = x[s * L:(s + 1) * L]
        u[:seg.size] = seg
        vs = T.oracle_convolve(b"full", b"linear", u, h)
        assert vs.size == P, (vs.size, P)
        v.append(vs)
    full = np.empty(n + m - 1)
    for s in range(nseg):
        last = s == nseg - 1
        own = n + m - 1 - s * L if last else L  # the last block also owns the tail behind nseg * L
        full[s * L:s * L + own] = v[s][:own]
        if s > 0 and m > 1:
            k = min(m - 1, own)
            full[s * L:s * L + k] = v[s][:k] + v[s - 1][L:L + k]
    return full


def oracle_full_rows(x, h, P):
    """oracle_full of every row of x (batch, n): (batch, n + m - 1)"""
    return np.stack([oracle_full(r, h, P) for r in x])


def window(full, typ, n, m):
    """the output rows cut from full results of shape (..., n + m - 1)"""
    start, ln = window_rule(typ, n, m)
    return np.ascontiguousarray(full[..., start:start + ln])


def oracle_filter(typ, x, h, P):
    """expected output of x, of shape (n,) or (batch, n), and the kernel h with blocks padded to P"""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    full = oracle_full(x, h, P) if x.ndim == 1 else oracle_full_rows(x, h, P)
    return window(full, typ, x.shape[-1], h.size)


def rows(n, batch, salt=0):
    """batch dense real rows (batch, n) from the suite's generator"""
    return T.real_input(n, T.seed_for(n) ^ salt, batch=batch).reshape(batch, n)


def kernel(m, salt=0):
    return T.real_input(m, T.seed_for(m) ^ salt ^ 0x4B)
