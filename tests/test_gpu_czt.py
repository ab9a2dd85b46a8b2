"""GPU: the batched chirp-z transform hsfft_czt_batched / hsfft_czt_real_batched (hsfft_czt.h).

Tolerance: BIT-EXACT, as everywhere in the suite.  Expected values come from hsfft_czt_testlib alone
-- the phase tables by the exact reduction in rationals and libm's sincos, numpy's float64
rotations, products and divisions around the reference's c2c of the pinned oracle at the padded
length (checked against long-double direct sums of the definition in test_czt_cpu.py) -- never from
the code under test.  Every output buffer is filled with NaN before the call, so a word that was
never written shows, and lies between sentinel words that must come back unchanged; the inputs are
read back unchanged.
"""
import numpy as np
import pytest

import hsfft_czt_testlib as C
import hsfft_testlib as T
from test_gpu_dct import Out, _assert_bits, _assert_bits_nan_aware, _upload

import hsfft

pytestmark = pytest.mark.gpu

PARAMS = [(0.1, 0.013), (-0.31, -0.0021)]
P_IDS = ["f0.1_df.013", "f-.31_df-.0021"]
REAL = [True, False]
R_IDS = ["real", "complex"]
SIZES = (1, 2, 3, 5, 8, 13, 31, 32, 33, 64)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if hsfft.device_count() < 1:
        pytest.skip("no GPU")
    hsfft.lib().hsfft_set_device(0)
    yield
    hsfft.synchronize()
    _ORACLE.clear()


_ORACLE = {}


def _case(real, n, m, f0, df, batch, salt=0, flags=0):
    """the rows x (batch, n) and the expected output (batch, m), computed once per module and kept read-only"""
    key = (real, n, m, f0, df, batch, salt, flags)
    if key not in _ORACLE:
        x = C.real_rows(n, batch, salt=0xD0 ^ salt) if real else C.complex_rows(n, batch, salt=0xD0 ^ salt)
        val = (x, C.oracle_czt(x, m, f0, df, flags))
        for a in val:
            a.setflags(write=False)
        _ORACLE[key] = val
    return _ORACLE[key]


def _run(x, m, f0, df, want, what, lead_in=0, lead_out=0, compare=_assert_bits):
    """one call on fresh buffers, checked against `want` (batch, m); lead_in / lead_out: doubles in
    front of the input and of the output"""
    x = np.ascontiguousarray(x)
    batch, n = x.shape
    real = x.dtype == np.float64
    xbuf, dx = _upload(x, lead_in)
    out = Out(2 * batch * m, lead=lead_out)
    hsfft.czt_batched(dx, real, n, out, m, f0, df, batch)
    hsfft.synchronize()
    y, guard = out.read()
    xin = xbuf.to_array(np.float64, offset_bytes=lead_in * 8).view(x.dtype).reshape(x.shape)
    xbuf.free()
    out.free()
    y = y.view(np.complex128).reshape(want.shape)
    compare(y, want, what)
    assert guard == 0, (what, "sentinel words changed", guard)
    _assert_bits_nan_aware(xin, x, (what, "the input changed"))
    return y


@pytest.mark.parametrize("real", REAL, ids=R_IDS)
@pytest.mark.parametrize("f0,df", PARAMS, ids=P_IDS)
def test_all_pairs_of_small_sizes(f0, df, real):
    """batch 3, dense rows that all differ: L = 2, both sides of every power-of-two boundary of n + m -
    1 up to 128, m > n as well as n > m, odd n (every other real row is only 8-byte aligned)"""
    for n in SIZES:
        for m in SIZES:
            assert hsfft.czt_shape(n, m) == C.shape_L(n, m)
            x, want = _case(real, n, m, f0, df, 3)
            assert n == 1 or not np.array_equal(x[0], x[1])
            _run(x, m, f0, df, want, (real, n, m, f0, df))


@pytest.mark.parametrize("real", REAL, ids=R_IDS)
def test_the_wrapped_chirp_just_fits(real):
    """(40, 25): n + m - 1 = 64 = L exactly, v's two halves touch; (40, 26): L = 128"""
    for n, m in ((40, 25), (40, 26)):
        assert hsfft.czt_shape(n, m) == (64 if m == 25 else 128)
        for f0, df in PARAMS:
            x, want = _case(real, n, m, f0, df, 3)
            _run(x, m, f0, df, want, (real, n, m, f0, df))


@pytest.mark.parametrize("real", REAL, ids=R_IDS)
@pytest.mark.parametrize("n,m", [(3000, 1000), (100000, 20000)], ids=["L4096", "L131072"])
def test_longer_rows(n, m, real):
    """two rows each: more than one block per row (L = 4096) and a two-pass inner transform (L = 131072)"""
    f0, df = PARAMS[0]
    x, want = _case(real, n, m, f0, df, 2)
    _run(x, m, f0, df, want, (real, n, m))


@pytest.mark.parametrize("real", REAL, ids=R_IDS)
@pytest.mark.parametrize("n,m", [(6, 5), (64, 64), (1000, 24)])
def test_on_8_byte_aligned_buffers(n, m, real):
    """input and output each behind an odd number of doubles, in all four combinations: caller
    buffers need the alignment of a double only, and the kernels fall back to 8-byte accesses on the
    side that is not 16-byte aligned; sentinels in front of the output as well"""
    f0, df = PARAMS[1]
    x, want = _case(real, n, m, f0, df, 3)
    for lead_in, lead_out in [(0, 0), (1, 0), (0, 3), (1, 3)]:
        _run(x, m, f0, df, want, (real, n, m, lead_in, lead_out), lead_in=lead_in, lead_out=lead_out)


def test_chunk_walk(monkeypatch):
    """HSFFT_CZT_CHUNK_MB=1, (3000, 1000), 19 rows: the documented rule, bytes / (2 x L x 16), gives 8
    rows per chunk, so chunks of 8, 8 and 3; the result equals the default knob's word for word and
    equals the oracle"""
    n, m, batch = 3000, 1000, 19
    f0, df = PARAMS[0]
    assert C.shape_L(n, m) == 4096 and T.rows_per_chunk(1, 2 * 4096) == 8
    for real in REAL:
        x, want = _case(real, n, m, f0, df, batch)
        dx = hsfft.DeviceBuffer.from_array(x)
        o1, o2 = Out(2 * batch * m), Out(2 * batch * m)
        monkeypatch.setenv("HSFFT_CZT_CHUNK_MB", "1")
        hsfft.czt_batched(dx, real, n, o1, m, f0, df, batch)
        monkeypatch.delenv("HSFFT_CZT_CHUNK_MB")
        hsfft.czt_batched(dx, real, n, o2, m, f0, df, batch)
        hsfft.synchronize()
        diff = hsfft.count_diff_words(o1, o2, 16 * batch * m)
        got = [o.read() for o in (o1, o2)]
        o1.free()
        o2.free()
        dx.free()
        assert diff == 0, ("chunked differs from one chunk", real, diff)
        for (y, guard), what in zip(got, ("chunked", "one chunk")):
            _assert_bits(y.view(np.complex128).reshape(batch, m), want, (what, real))
            assert guard == 0, (what, real)


@pytest.mark.parametrize("real", REAL, ids=R_IDS)
def test_more_than_65535_rows_in_one_call(real):
    """(1, 1), 70000 rows: one chunk, more than one launch's 65535 grid rows"""
    f0, df = PARAMS[0]
    x, want = _case(real, 1, 1, f0, df, 70000)
    _run(x, 1, f0, df, want, (real, "70000 rows of 1"))


def test_cache_eviction_release_and_finalize():
    """five keys through the four-entry cache, then the first again (it was evicted); the same sizes
    with another df and with another f0 must not reuse tables; then hsfft_release_scratch, a run,
    hsfft_finalize and a run: every result is bit-exact"""
    keys = [(8, 5, 0.1, 0.013), (16, 7, 0.1, 0.013), (5, 12, 0.2, 0.01), (31, 31, -0.4, 0.002), (64, 3, 0.0, 0.001),
            (8, 5, 0.1, 0.013), (8, 5, 0.1, 0.014), (8, 5, 0.11, 0.014), (8, 5, 0.1, 0.013)]
    for n, m, f0, df in keys:
        for real in REAL:
            x, want = _case(real, n, m, f0, df, 3)
            _run(x, m, f0, df, want, ("cache", real, n, m, f0, df))
    wants = [_case(True, 8, 5, 0.1, d, 3)[1] for d in (0.013, 0.014)] + [_case(True, 8, 5, 0.11, 0.014, 3)[1]]
    assert T.mismatches(wants[0], wants[1]) and T.mismatches(wants[1], wants[2])  # reused tables would show
    n, m, f0, df = 40, 25, 0.1, 0.013
    hsfft.check(hsfft.lib().hsfft_release_scratch(), "release_scratch")
    for real in REAL:
        x, want = _case(real, n, m, f0, df, 3)
        _run(x, m, f0, df, want, ("after release_scratch", real))
    hsfft.finalize()
    hsfft.lib().hsfft_set_device(0)
    for real in REAL:
        x, want = _case(real, n, m, f0, df, 3)
        _run(x, m, f0, df, want, ("after finalize", real))


def test_either_twiddle_mode_against_its_own_oracle():
    """one run per twiddle mode at L = 64, 512 and 4096, each against the oracle with the matching
    flag: the plans and the cached spectrum V follow the calling thread's mode, so where the oracle's
    exact-twiddle flag gives other words, an entry shared between the modes would show"""
    f0, df = PARAMS[0]
    differ = []
    try:
        for n, m in ((40, 25), (300, 213), (3000, 1000)):
            for mode, flags in (("reference", 0), ("exact", T.ORC_EXACT), ("reference", 0)):
                hsfft.set_twiddle_mode(mode)
                x, want = _case(True, n, m, f0, df, 2, flags=flags)
                _run(x, m, f0, df, want, ("twiddle mode", mode, n, m))
            differ.append(T.mismatches(_case(True, n, m, f0, df, 2, flags=0)[1], _case(True, n, m, f0, df, 2, flags=T.ORC_EXACT)[1]) > 0)
    finally:
        hsfft.set_twiddle_mode("reference")
    print("the exact-twiddle oracle differs at L = 64, 512, 4096:", differ)


def _special_rows(n, real):
    x = C.real_rows(n, 8, salt=0xE7).copy() if real else C.complex_rows(n, 8, salt=0xE7).copy()
    x[0] = np.where(np.arange(n) % 3 == 0, -0.0, 0.0)
    if not real:
        x[0] = x[0].real + 1j * np.where(np.arange(n) % 2 == 0, -0.0, 0.0)
    x[1] = x[1] * 1e-310
    x[1, 3], x[1, 4] = 5e-324, -5e-324
    x[2] = x[2] * 1e300
    x[2, 5], x[2, 6] = 1.7e308, -1.7e308
    x[3, 0] = np.inf
    x[4, 5] = np.inf if real else complex(0.5, np.inf)
    x[5, n - 1] = np.inf
    x[6, n // 2 + 1] = np.nan
    return x


@pytest.mark.parametrize("real", REAL, ids=R_IDS)
@pytest.mark.parametrize("n,m", [(16, 16), (64, 24)])
def test_special_values(n, m, real):
    """rows of signed zeros, subnormals, values near overflow, one +Inf at index 0, at an odd index
    and at the last index, and one NaN, beside a dense row: the words equal the oracle's, NaN
    positions compared as NaN"""
    f0, df = PARAMS[0]
    x = _special_rows(n, real)
    assert np.isfinite(x[7]).all()
    want = C.oracle_czt(x, m, f0, df)
    assert np.isfinite(want[7]).all() and T.nan_words(want[6]).all() and not np.isfinite(want[3]).all()
    assert not np.isfinite(want[4]).all() and not np.isfinite(want[5]).all()
    assert np.isfinite(want[1]).all() and T.zero_words(want[0]) == 2 * m
    y = _run(x, m, f0, df, want, ("special values", real, n, m), compare=_assert_bits_nan_aware)
    assert np.isfinite(y[7]).all()


def test_conveniences():
    f0, df = PARAMS[0]
    for real in REAL:
        x, want = _case(real, 100, 37, f0, df, 3)
        y = hsfft.czt(x, 37, f0, df)
        assert y.shape == (3, 37) and y.dtype == np.complex128
        _assert_bits(y, want, ("czt", real, "2-D input"))
        y = hsfft.czt(x[1], 37, f0, df)
        assert y.shape == (37,) and y.dtype == np.complex128
        _assert_bits(y, want[1], ("czt", real, "1-D input drops the batch axis"))
        zf0, zdf = 0.2 / 2.0, (0.5 - 0.2) / (64 * 2.0)
        y = hsfft.zoom_fft(x, [0.2, 0.5], m=64)
        assert y.shape == (3, 64)
        _assert_bits(y, hsfft.czt(x, 64, zf0, zdf), ("zoom_fft", real, "czt with the derived f0 and df"))
        _assert_bits(y, C.oracle_czt(x, 64, zf0, zdf), ("zoom_fft", real))
    # on the DFT grid it is the forward transform, as accurately as test_czt_cpu.py asks of the expectation
    n = 256
    x = C.complex_rows(n, 1, salt=0xA3)
    direct = C.direct_czt(x[0], n, 0.0, 1.0 / n)
    bound = 4 * C.rel_err(C.numpy_czt(x, n, 0.0, 1.0 / n)[0], direct)
    p = hsfft.Plan(n)
    dft = p.exec(x[0])
    p.close()
    err = C.rel_err(hsfft.czt(x[0], n, 0.0, 1.0 / n), dft)
    print("czt on the DFT grid against Plan(256).exec", err, "bound", bound)
    assert bound > 0 and err <= bound, (err, bound)
