"""GPU: the batched MDCT and IMDCT of real rows, hsfft_mdct_batched and hsfft_imdct_batched
(hsfft_dct4.h).

Tolerance: BIT-EXACT, as everywhere in the suite.  Expected values come from hsfft_dct4_testlib alone
-- numpy's frame gather, window products, folds, unfolds and overlap-adds around its type-IV
expectation (checked against long-double direct sums of the definitions in test_dct4_cpu.py) --
never from the code under test.  Every output buffer is filled with NaN before the call and lies
between sentinel words that must come back unchanged; the inputs are read back unchanged.
"""
import numpy as np
import pytest

import hsfft_dct4_testlib as F
import hsfft_testlib as T
from test_gpu_dct import Out, _assert_bits, _assert_bits_nan_aware, _upload

import hsfft

pytestmark = pytest.mark.gpu

HOPS = [2, 4, 6, 8, 12, 64, 256, 1024]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if hsfft.device_count() < 1:
        pytest.skip("no GPU")
    hsfft.lib().hsfft_set_device(0)
    yield
    hsfft.synchronize()


def _window(N, windowed):
    return F.sine_window(N) if windowed else None


def _shapes(pad):
    """frame counts: one frame needs pad == 0 (with pad a row of one hop already has two)"""
    return (2, 5) if pad else (1, 2, 5)


def _forward(x, N, w, pad, want, what, lead_in=0, lead_out=0, compare=_assert_bits):
    """one hsfft_mdct_batched call on fresh buffers, checked against `want` (batch, nframes, N)"""
    x = np.ascontiguousarray(x)
    batch, n = x.shape
    xbuf, dx = _upload(x, lead_in)
    wbuf = hsfft.DeviceBuffer.from_array(w) if w is not None else None
    out = Out(want.size, lead=lead_out)
    hsfft.mdct_batched(dx, n, wbuf, N, pad, out, batch)
    hsfft.synchronize()
    y, guard = out.read()
    xin = xbuf.to_array(np.float64, offset_bytes=lead_in * 8).reshape(x.shape)
    xbuf.free()
    out.free()
    if wbuf is not None:
        _assert_bits(wbuf.to_array(np.float64), w, (what, "the window changed"))
        wbuf.free()
    y = y.reshape(want.shape)
    compare(y, want, what)
    assert guard == 0, (what, "sentinel words changed", guard)
    compare(xin, x, (what, "the input changed"))
    return y


def _backward(X, w, pad, want, what, lead_in=0, lead_out=0, compare=_assert_bits):
    """one hsfft_imdct_batched call on fresh buffers, checked against `want` (batch, n)"""
    X = np.ascontiguousarray(X)
    batch, nf, N = X.shape
    xbuf, dx = _upload(X, lead_in)
    wbuf = hsfft.DeviceBuffer.from_array(w) if w is not None else None
    out = Out(want.size, lead=lead_out)
    hsfft.imdct_batched(dx, nf, wbuf, N, pad, out, want.shape[1], batch)
    hsfft.synchronize()
    y, guard = out.read()
    xin = xbuf.to_array(np.float64, offset_bytes=lead_in * 8).reshape(X.shape)
    xbuf.free()
    out.free()
    if wbuf is not None:
        wbuf.free()
    y = y.reshape(want.shape)
    compare(y, want, what)
    assert guard == 0, (what, "sentinel words changed", guard)
    compare(xin, X, (what, "the input changed"))
    return y


@pytest.mark.parametrize("N", HOPS)
def test_forward(N):
    """pad x window x frame counts, batch 3: hops with odd and even N/2, one-point to 512-point inner
    transforms, rows that end inside the last frame's reach (pad)"""
    for pad in (False, True):
        for nf in _shapes(pad):
            n = (nf + 1) * N - (2 * N if pad else 0)
            assert hsfft.mdct_shape(n, N, pad) == (nf, N if pad else 0)
            x = F.rows(n, 3, salt=0x3D ^ nf)
            for windowed in (False, True):
                w = _window(N, windowed)
                _forward(x, N, w, pad, F.oracle_mdct(x, N, w, pad), ("mdct", N, pad, nf, windowed))


@pytest.mark.parametrize("N", HOPS)
def test_backward(N):
    """pad x window x frame counts, batch 3; without pad the first and the last N samples of a row
    are covered by one frame and take its term alone"""
    for pad in (False, True):
        for nf in _shapes(pad):
            X = F.rows(nf * N, 3, salt=0x1D ^ nf).reshape(3, nf, N)
            for windowed in (False, True):
                w = _window(N, windowed)
                want = F.oracle_imdct(X, w, pad)
                assert want.shape == (3, (nf + 1) * N - (2 * N if pad else 0))
                _backward(X, w, pad, want, ("imdct", N, pad, nf, windowed))


@pytest.mark.parametrize("N", [6, 64])
def test_on_8_byte_aligned_buffers(N):
    """samples, coefficients and outputs each behind an odd number of doubles, in all four
    combinations, with the window 8-byte aligned as well"""
    x = F.rows(6 * N, 3, salt=0x8A)
    wsrc = np.concatenate([[0.0], F.sine_window(N)])
    wbuf = hsfft.DeviceBuffer.from_array(wsrc)
    w = wsrc[1:]
    wv = hsfft.DeviceView(wbuf, 8)
    want = F.oracle_mdct(x, N, w, False)
    back = F.oracle_imdct(want, w, False)
    for lead_in, lead_out in [(0, 0), (1, 0), (0, 3), (1, 3)]:
        _forward(x, N, None, False, F.oracle_mdct(x, N, None, False), ("mdct", N, lead_in, lead_out), lead_in, lead_out)
        _backward(want, None, False, F.oracle_imdct(want, None, False), ("imdct", N, lead_in, lead_out), lead_in, lead_out)
        xbuf, dx = _upload(x, lead_in)
        out = Out(want.size, lead=lead_out)
        hsfft.mdct_batched(dx, 6 * N, wv, N, False, out, 3)
        hsfft.synchronize()
        y, guard = out.read()
        _assert_bits(y.reshape(want.shape), want, ("mdct, 8-byte aligned window", N, lead_in, lead_out))
        assert guard == 0
        out.free()
        xbuf.free()
        cbuf, dc = _upload(want, lead_in)
        out = Out(back.size, lead=lead_out)
        hsfft.imdct_batched(dc, want.shape[1], wv, N, False, out, back.shape[1], 3)
        hsfft.synchronize()
        y, guard = out.read()
        _assert_bits(y.reshape(back.shape), back, ("imdct, 8-byte aligned window", N, lead_in, lead_out))
        assert guard == 0
        out.free()
        cbuf.free()
    wbuf.free()


def test_chunk_walk(monkeypatch):
    """HSFFT_MDCT_CHUNK_MB=1, N = 1024, 60 rows of 5 frames.  Forward: bytes / (N x 8) gives 128
    frames per chunk, so chunks of 128, 128 and 44 frames, whose edges fall inside rows.  Backward:
    bytes / (nframes x N x 8) gives 25 whole rows per chunk, so 25, 25 and 10.  Either result equals
    the default knob's word for word and equals the oracle"""
    N, nf, batch = 1024, 5, 60
    assert T.rows_per_chunk(1, N * 8, elem=1) == 128 and 128 % nf and T.rows_per_chunk(1, nf * N * 8, elem=1) == 25
    n, w = (nf + 1) * N, F.sine_window(N)
    x = F.rows(n, batch, salt=0xC4)
    X = F.oracle_mdct(x, N, w, False)
    back = F.oracle_imdct(X, w, False)
    dx, dX, dw = (hsfft.DeviceBuffer.from_array(a) for a in (x, X, w))
    for what, call, want in (("mdct", lambda o: hsfft.mdct_batched(dx, n, dw, N, False, o, batch), X),
                             ("imdct", lambda o: hsfft.imdct_batched(dX, nf, dw, N, False, o, n, batch), back)):
        o1, o2 = Out(want.size), Out(want.size)
        monkeypatch.setenv("HSFFT_MDCT_CHUNK_MB", "1")
        call(o1)
        monkeypatch.delenv("HSFFT_MDCT_CHUNK_MB")
        call(o2)
        hsfft.synchronize()
        diff = hsfft.count_diff_words(o1, o2, want.nbytes)
        got = [o.read() for o in (o1, o2)]
        o1.free()
        o2.free()
        assert diff == 0, ("chunked differs from one chunk", what, diff)
        for (y, guard), how in zip(got, ("chunked", "one chunk")):
            _assert_bits(y.reshape(want.shape), want, (what, how))
            assert guard == 0, (what, how)
    for d in (dx, dX, dw):
        d.free()


def test_row_ends_take_one_term_alone():
    """without pad one frame covers the first and the last N samples.  Coefficients that are all
    +0.0 give -0.0 at the odd places of every frame's transform, so the row ends hold -0.0 words:
    a kernel that added the single term to 0.0 would turn them into +0.0"""
    N, nf = 8, 3
    X = np.zeros((2, nf, N))
    want = F.oracle_imdct(X, None, False)
    assert T.zero_words(want) == want.size
    assert np.signbit(want[:, :N]).any() and np.signbit(want[:, -N:]).any()
    _backward(X, None, False, want, "zeros, no window")
    w = F.sine_window(N)
    _backward(X, w, False, F.oracle_imdct(X, w, False), "zeros, sine window")


def _special_rows(n, salt):
    """seven rows of n: zeros of mixed signs, subnormals, values near overflow, +Inf first, -Inf last,
    one NaN, and a dense finite row"""
    x = F.rows(n, 7, salt=salt).copy()
    x[0] = np.where(np.arange(n) % 3 == 0, -0.0, 0.0)
    x[1] = x[1] * 1e-310
    x[1, 3], x[1, 4] = 5e-324, -5e-324
    x[2] = x[2] * 1e300
    x[2, 5], x[2, 6] = 1.7e308, -1.7e308
    x[3, 0] = np.inf
    x[4, n - 1] = -np.inf
    x[5, n // 2 + 1] = np.nan
    assert np.isfinite(x[6]).all()
    return x


@pytest.mark.parametrize("pad", [False, True], ids=["nopad", "pad"])
def test_special_values(pad):
    """rows of zeros of mixed signs (the sign of (-p) - p' and of p - p' on zeros), subnormals, values
    near overflow, infinities and a NaN through the fold, the window product on the padding's +0.0
    and the unfold: the words equal the oracle's, NaN positions compared as NaN"""
    N, nf = 16, 4
    x = _special_rows((nf + 1) * N - (2 * N if pad else 0), 0xE9)
    X = _special_rows(nf * N, 0xEA).reshape(7, nf, N)
    wneg = F.sine_window(N) * np.where(np.arange(2 * N) % 5 == 0, -1.0, 1.0)  # a negative weight on the padding: -0.0
    for w in (None, F.sine_window(N), wneg):
        want = F.oracle_mdct(x, N, w, pad)
        assert T.zero_words(want[0]) == want[0].size and np.signbit(want[0]).any() and not np.signbit(want[0]).all()
        assert np.isfinite(want[6]).all() and np.isfinite(want[1]).all() and T.nan_words(want[5]).any()
        y = _forward(x, N, w, pad, want, ("mdct special values", pad, w is not None), compare=_assert_bits_nan_aware)
        assert np.isfinite(y[6]).all()
        _backward(X, w, pad, F.oracle_imdct(X, w, pad), ("imdct special values", pad, w is not None),
                  compare=_assert_bits_nan_aware)


def test_conveniences_and_round_trip():
    N, nf = 64, 6
    w = F.sine_window(N)
    for pad in (False, True):
        n = (nf + 1) * N - (2 * N if pad else 0)
        x = F.rows(n, 3, salt=0xC9)
        want = F.oracle_mdct(x, N, w, pad)
        X = hsfft.mdct(x, N, window=w, pad=pad)
        assert X.shape == (3, nf, N) and X.dtype == np.float64
        _assert_bits(X, want, ("mdct", pad, "2-D input"))
        X1 = hsfft.mdct(x[1], N, window=w, pad=pad)
        assert X1.shape == (nf, N)
        _assert_bits(X1, want[1], ("mdct", pad, "1-D input drops the batch axis"))
        _assert_bits(hsfft.mdct(x, N, pad=pad), F.oracle_mdct(x, N, None, pad), ("mdct", pad, "no window"))
        back = hsfft.imdct(X, window=w, pad=pad)
        assert back.shape == (3, n) and back.dtype == np.float64
        _assert_bits(back, F.oracle_imdct(want, w, pad), ("imdct", pad, "3-D input"))
        b1 = hsfft.imdct(X1, window=w, pad=pad)
        assert b1.shape == (n,)
        _assert_bits(b1, back[1], ("imdct", pad, "2-D input drops the batch axis"))
        _assert_bits(hsfft.imdct(X, pad=pad), F.oracle_imdct(want, None, pad), ("imdct", pad, "no window"))
        # perfect reconstruction of the samples two frames cover, within the CPU test's bound
        lo, hi = (0, n) if pad else (N, n - N)
        err, ref = float(np.abs(back - x)[:, lo:hi].max()), F.c2c_round_trip_error(N // 2)
        print("pad", pad, "round trip error on the GPU", err, "reference c2c round trip error at 32", ref)
        assert err <= 8 * ref, (pad, err, ref)
