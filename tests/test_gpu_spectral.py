"""GPU: the batched analytic signal and Fourier resampling, hsfft_hilbert_batched and
hsfft_resample_batched (hsfft_spectral.h).

Tolerance: BIT-EXACT, as everywhere in the suite.  Expected values come from hsfft_spectral_testlib
alone -- numpy's float64 adds, halvings and divisions on the compact bins of the reference's r2c,
between it and the reference's inverse c2c or c2r of the pinned oracle (checked against long-double
direct sums of the definitions in test_spectral_cpu.py) -- never from the code under test.  Every
output buffer is filled with NaN before the call, so a word that was never written shows, and lies
in front of sentinel words that must come back unchanged; the inputs are read back unchanged.  All
buffers are 16-byte aligned: the calls reject others (test_spectral_cpu.py).
"""
import numpy as np
import pytest

import hsfft_czt_testlib as C
import hsfft_spectral_testlib as SP
import hsfft_testlib as T
from test_gpu_dct import Out, _assert_bits, _assert_bits_nan_aware, _upload

import hsfft

pytestmark = pytest.mark.gpu

HILBERT_SIZES = (2, 4, 6, 8, 10, 12, 30, 32, 34, 62, 64, 66, 126, 128, 130, 254, 256, 258, 510, 512, 514)
RESAMPLE_SIZES = (2, 4, 6, 10, 16, 30, 32, 34, 64, 66, 250, 256)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if hsfft.device_count() < 1:
        pytest.skip("no GPU")
    hsfft.lib().hsfft_set_device(0)
    yield
    hsfft.synchronize()
    _ORACLE.clear()


_ORACLE = {}


def _case(n, m, batch, salt=0, flags=0):
    """the rows x (batch, n) and the expected output -- the analytic signal (batch, n) for m == 0, else
    the resampled rows (batch, m) -- computed once per module and kept read-only"""
    key = (n, m, batch, salt, flags)
    if key not in _ORACLE:
        x = SP.rows(n, batch, salt=0xD0 ^ salt)
        val = (x, SP.oracle_resample(x, m, flags) if m else SP.oracle_hilbert(x, flags))
        for a in val:
            a.setflags(write=False)
        _ORACLE[key] = val
    return _ORACLE[key]


def _run(x, m, want, what, compare=_assert_bits):
    """one call on fresh buffers, checked against `want`: the analytic signal for m == 0, else resampling to m"""
    x = np.ascontiguousarray(x)
    batch, n = x.shape
    xbuf, dx = _upload(x, 0)
    out = Out(batch * m if m else 2 * batch * n)
    assert dx.ptr % 16 == 0 and out.ptr % 16 == 0
    if m:
        hsfft.resample_batched(dx, n, out, m, batch)
    else:
        hsfft.hilbert_batched(dx, out, n, batch)
    hsfft.synchronize()
    y, guard = out.read()
    xin = xbuf.to_array(np.float64).reshape(x.shape)
    xbuf.free()
    out.free()
    y = (y if m else y.view(np.complex128)).reshape(want.shape)
    compare(y, want, what)
    assert guard == 0, (what, "sentinel words changed", guard)
    _assert_bits_nan_aware(xin, x, (what, "the input changed"))
    return y


@pytest.mark.parametrize("n", HILBERT_SIZES)
def test_small_hilbert_lengths(n):
    """batch 3, dense rows that all differ: n == 2 (no doubled bin), both sides of every block edge of n up
    to 512, lengths with the factors 3, 5 and 7 in the default twiddle mode"""
    x, want = _case(n, 0, 3)
    assert not np.array_equal(x[0], x[1]) and not np.array_equal(x[1], x[2])
    _run(x, 0, want, ("hilbert", n))


@pytest.mark.parametrize("n", RESAMPLE_SIZES)
def test_resample_pairs(n):
    """every m of the list for this n, batch 3: m < n, m == n and m > n, the folded bin at K = 1, and both
    sides of every block edge of m/2+1"""
    for m in RESAMPLE_SIZES:
        x, want = _case(n, m, 3)
        assert not np.array_equal(x[0], x[1]) and not np.array_equal(x[1], x[2])
        _run(x, m, want, ("resample", n, m))


@pytest.mark.parametrize("n,m", [(4096, 0), (4096, 3000), (3000, 4096), (131072, 0), (131072, 65536), (96000, 88200),
                                 (2062, 0), (2062, 4096), (4096, 2062)],
                         ids=lambda v: str(v))
def test_long_rows(n, m):
    """two rows each: several blocks per row (4096, 3000), a two-pass inner transform (131072, 96000 ->
    88200), and 2062 = 2 x 1031 with its large prime factor on whatever path its plans take"""
    x, want = _case(n, m, 2)
    _run(x, m, want, ("long rows", n, m))


def test_chunk_walk(monkeypatch):
    """HSFFT_SPECTRAL_CHUNK_MB=1: the analytic signal at n = 3000 on 33 rows walks chunks of 14, 14 and 5
    (1048576 / 72016 = 14), resampling (3000, 2000) on 60 rows chunks of 26, 26 and 8 (1048576 / 40032 =
    26); the result equals the default knob's word for word and equals the oracle"""
    for n, m, batch, per_chunk in ((3000, 0, 33, 14), (3000, 2000, 60, 26)):
        x, want = _case(n, m, batch)
        words = batch * m if m else 2 * batch * n
        dx = hsfft.DeviceBuffer.from_array(x)
        o1, o2 = Out(words), Out(words)
        call = (lambda o: hsfft.resample_batched(dx, n, o, m, batch)) if m else (lambda o: hsfft.hilbert_batched(dx, o, n, batch))
        monkeypatch.setenv("HSFFT_SPECTRAL_CHUNK_MB", "1")
        assert hsfft.spectral_chunk_rows(n, m) == per_chunk == SP.chunk_rows(n, m, 1) < batch
        call(o1)
        monkeypatch.delenv("HSFFT_SPECTRAL_CHUNK_MB")
        assert hsfft.spectral_chunk_rows(n, m) == SP.chunk_rows(n, m) >= batch
        call(o2)
        hsfft.synchronize()
        diff = hsfft.count_diff_words(o1, o2, 8 * words)
        got = [o.read() for o in (o1, o2)]
        o1.free()
        o2.free()
        dx.free()
        assert diff == 0, ("chunked differs from one chunk", n, m, diff)
        for (y, guard), what in zip(got, ("chunked", "one chunk")):
            _assert_bits((y if m else y.view(np.complex128)).reshape(want.shape), want, (what, n, m))
            assert guard == 0, (what, n, m)


def test_dirty_scratch():
    """a chirp-z call at L = 4096 leaves non-zero words in both pool buffers the calls share with it;
    then the analytic signal at 64, resampling (64, 256), whose upper three quarters of Y are zeros, and
    the analytic signal at 66; then hsfft_release_scratch and the first call again.  A zero-fill skipped
    in the upper half of Z or of Y shows here"""
    f0, df = 0.1, 0.013
    xc = C.real_rows(3000, 3, salt=0xD5)
    dxc = hsfft.DeviceBuffer.from_array(xc)
    oc = Out(2 * 3 * 1000)
    hsfft.czt_batched(dxc, True, 3000, oc, 1000, f0, df, 3)
    hsfft.synchronize()
    yc, guard = oc.read()
    oc.free()
    dxc.free()
    assert guard == 0 and np.count_nonzero(yc) == yc.size
    for n, m in ((64, 0), (64, 256), (66, 0)):
        x, want = _case(n, m, 3)
        _run(x, m, want, ("after czt", n, m))
    hsfft.check(hsfft.lib().hsfft_release_scratch(), "release_scratch")
    x, want = _case(64, 0, 3)
    _run(x, 0, want, "after release_scratch")


def _special_rows(n):
    """+0.0, -0.0, subnormals, values near DBL_MAX, one Inf, one NaN, a dense row, values near DBL_MAX again"""
    x = SP.rows(n, 8, salt=0xE7).copy()
    x[0] = 0.0
    x[1] = -0.0
    x[2] = x[2] * 1e-310
    x[2, 3], x[2, 4] = 5e-324, -5e-324
    # near DBL_MAX.  The reference's r2c forms the doubled sums itself before it halves them, so a finite
    # bin whose doubling overflows does not exist: a tone whose bin would be 1.2e308 gives an infinite S
    # from finite samples (row 3), and the largest doubling that can be met is a finite one (row 7)
    x[3] = np.cos(2 * np.pi * np.arange(n) / 8) * (1.2e308 / (n // 2))
    x[4, 5] = np.inf
    x[5, n // 2 + 1] = np.nan
    x[7] = np.array([1.0, 0.0, -1.0, 0.0] * (n // 4)) * (0.85e308 / (n // 2))  # S[n/4] = 0.85e308, the folded bin of n -> n/2
    return x


@pytest.mark.parametrize("n,m", [(64, 0), (64, 32), (32, 64)], ids=["hilbert64", "resample64-32", "resample32-64"])
def test_special_values(n, m):
    """rows of +0.0, of -0.0, of subnormals (q and the halving round them), of values near DBL_MAX (an
    infinite bin from finite samples; a bin of 0.85e308 whose doubling is the largest that stays finite),
    with one Inf and with one NaN, beside a dense row: the words equal the oracle's, NaN positions
    compared as NaN; an all-NaN output row is allowed only where the expectation is all NaN"""
    x = _special_rows(n)
    assert np.isfinite(x[6]).all() and np.signbit(x[1]).all() and not np.signbit(x[0]).any()
    want = SP.oracle_resample(x, m) if m else SP.oracle_hilbert(x)
    assert np.isfinite(want[6]).all() and np.isfinite(want[2]).all() and T.nan_words(want[5]).any()
    assert T.zero_words(want[0]) == want[0].view(np.float64).size and not np.isfinite(want[4].view(np.float64)).all()
    S = T.oracle_r2c(x[[3, 7]])[:, :n // 2 + 1]
    assert np.isfinite(x[3]).all() and np.isinf(S[0, n // 8].real) and not np.isfinite(want[3].view(np.float64)).all()
    assert np.isfinite(S[1].view(np.float64)).all() and S[1, n // 4].real > 0.8e308 and np.isfinite(want[7].view(np.float64)).all()
    y = _run(x, m, want, ("special values", n, m), compare=_assert_bits_nan_aware)
    for b in range(x.shape[0]):
        if T.nan_words(y[b]).all():
            assert T.nan_words(want[b]).all(), ("row", b, "is all NaN and its expectation is not")
    assert np.isfinite(y[6]).all()


def test_either_twiddle_mode_against_its_own_oracle():
    """the analytic signal at n = 250 and resampling (250, 66) in the reference mode, the exact mode and
    the reference mode again, each against the oracle with the matching flag: the plans follow the
    calling thread's mode.  At these two sizes the oracle's words happen to be the same in both modes (no
    plan in them meets the reference's quirk), so the analytic signal at 66 and resampling (250, 12) run
    as well: there the two oracles differ, and plans of the wrong mode would show"""
    differ = {}
    try:
        for n, m in ((250, 0), (250, 66), (66, 0), (250, 12)):
            for mode, flags in (("reference", 0), ("exact", T.ORC_EXACT), ("reference", 0)):
                hsfft.set_twiddle_mode(mode)
                x, want = _case(n, m, 3, flags=flags)
                _run(x, m, want, ("twiddle mode", mode, n, m))
            differ[(n, m)] = T.mismatches(_case(n, m, 3, flags=0)[1], _case(n, m, 3, flags=T.ORC_EXACT)[1]) > 0
    finally:
        hsfft.set_twiddle_mode("reference")
    print("the exact-twiddle oracle differs:", differ)
    assert differ[(66, 0)] and differ[(250, 12)]


def test_python_wrappers():
    """hsfft.hilbert and hsfft.resample on 2-D and 1-D input equal the low-level calls (the oracle's words)"""
    x, want = _case(256, 0, 3)
    y = hsfft.hilbert(x)
    assert y.shape == (3, 256) and y.dtype == np.complex128
    _assert_bits(y, want, "hilbert, 2-D input")
    y = hsfft.hilbert(x[1])
    assert y.shape == (256,) and y.dtype == np.complex128
    _assert_bits(y, want[1], "hilbert, 1-D input drops the batch axis")
    for m in (66, 256, 250):
        x, want = _case(256, m, 3)
        y = hsfft.resample(x, m)
        assert y.shape == (3, m) and y.dtype == np.float64
        _assert_bits(y, want, ("resample, 2-D input", m))
        y = hsfft.resample(x[2], m)
        assert y.shape == (m,) and y.dtype == np.float64
        _assert_bits(y, want[2], ("resample, 1-D input drops the batch axis", m))
    y = hsfft.resample(np.arange(8, dtype=np.int32), 4)  # any real dtype is converted
    assert y.dtype == np.float64 and y.shape == (4,)
    _assert_bits(y, SP.oracle_resample(np.arange(8.0)[None, :], 4)[0], "resample of an integer row")
