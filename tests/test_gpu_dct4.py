"""GPU: the batched type-IV cosine and sine transforms hsfft_dct4_batched (hsfft_dct4.h).

Tolerance: BIT-EXACT, as everywhere in the suite.  Expected values come from hsfft_dct4_testlib alone
-- libm's sincos table, numpy's pairings, float64 rotations and sign-bit flips around the reference's
c2c of the pinned oracle (checked against long-double direct sums of scipy's definitions in
test_dct4_cpu.py) -- never from the code under test.  Every output buffer is filled with NaN before
the call, so a word that was never written shows, and lies between sentinel words that must come
back unchanged; the inputs are read back unchanged.
"""
import numpy as np
import pytest

import hsfft_dct4_testlib as F
import hsfft_testlib as T
from test_gpu_dct import Out, _assert_bits, _assert_bits_nan_aware, _upload

import hsfft

pytestmark = pytest.mark.gpu

KINDS = [F.COS, F.SIN]
K_IDS = ["dct4", "dst4"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if hsfft.device_count() < 1:
        pytest.skip("no GPU")
    hsfft.lib().hsfft_set_device(0)
    yield
    hsfft.synchronize()
    _ORACLE.clear()


_ORACLE = {}


def _case(N, batch, salt=0):
    """the rows x (batch, N) and both expected outputs, computed once per module and kept read-only"""
    key = (N, batch, salt)
    if key not in _ORACLE:
        x = F.rows(N, batch, salt=0xD0 ^ salt)
        val = {"x": x, F.COS: F.oracle_dct4(x, F.COS), F.SIN: F.oracle_dct4(x, F.SIN)}
        for a in val.values():
            a.setflags(write=False)
        _ORACLE[key] = val
    return _ORACLE[key]


def _run(kind, x, want, what, lead_in=0, lead_out=0, compare=_assert_bits):
    """one call on fresh buffers, checked against `want`; lead_in / lead_out: doubles in front of the
    input and of the output"""
    x = np.ascontiguousarray(x)
    batch, N = x.shape
    xbuf, dx = _upload(x, lead_in)
    out = Out(x.size, lead=lead_out)
    hsfft.dct4_batched(kind, dx, out, N, batch)
    hsfft.synchronize()
    y, guard = out.read()
    xin = xbuf.to_array(np.float64, offset_bytes=lead_in * 8).reshape(x.shape)
    xbuf.free()
    out.free()
    y = y.reshape(want.shape)
    compare(y, want, what)
    assert guard == 0, (what, "sentinel words changed", guard)
    compare(xin, x, (what, "the input changed"))
    return y


@pytest.mark.parametrize("kind", KINDS, ids=K_IDS)
def test_every_even_length_to_128(kind):
    """batch 3, dense rows that all differ: h = 1 (N = 2: the c2c is a copy), odd h and its middle
    lane, even h and its mirrored pairs, mixed-radix and Bluestein inner lengths"""
    for N in range(2, 130, 2):
        c = _case(N, 3)
        assert not np.array_equal(c["x"][0], c["x"][1])
        _run(kind, c["x"], c[kind], (kind, N))


@pytest.mark.parametrize("kind", KINDS, ids=K_IDS)
@pytest.mark.parametrize("N", [4096, 10006, 25200, 131072], ids=["4096", "bluestein_10006", "25200", "131072"])
def test_longer_rows(N, kind):
    """two rows each: more than one block per row, a Bluestein inner length (h = 5003), the 12600
    whole-row schedule (h = 12600) and a two-pass inner transform (h = 65536)"""
    c = _case(N, 2)
    _run(kind, c["x"], c[kind], (kind, N))


@pytest.mark.parametrize("kind", KINDS, ids=K_IDS)
@pytest.mark.parametrize("N", [6, 64, 1000])
def test_on_8_byte_aligned_buffers(N, kind):
    """input and output each behind an odd number of doubles, in all four combinations: caller
    buffers need the alignment of a double only, and the kernels fall back to 8-byte accesses on the
    side that is not 16-byte aligned; sentinels in front of the output as well"""
    c = _case(N, 3)
    for lead_in, lead_out in [(0, 0), (1, 0), (0, 3), (1, 3)]:
        _run(kind, c["x"], c[kind], (kind, N, lead_in, lead_out), lead_in=lead_in, lead_out=lead_out)


def test_chunk_walk(monkeypatch):
    """HSFFT_DCT_CHUNK_MB=1, N = 4096, 37 rows: the documented rule, bytes / (N x 16), gives 16 rows
    per chunk, so chunks of 16, 16 and 5; the result equals the default knob's word for word and
    equals the oracle"""
    N, batch = 4096, 37
    assert T.rows_per_chunk(1, N * 16, elem=1) == 16
    c = _case(N, batch)
    dx = hsfft.DeviceBuffer.from_array(c["x"])
    for kind in KINDS:
        o1, o2 = Out(c["x"].size), Out(c["x"].size)
        monkeypatch.setenv("HSFFT_DCT_CHUNK_MB", "1")
        hsfft.dct4_batched(kind, dx, o1, N, batch)
        monkeypatch.delenv("HSFFT_DCT_CHUNK_MB")
        hsfft.dct4_batched(kind, dx, o2, N, batch)
        hsfft.synchronize()
        diff = hsfft.count_diff_words(o1, o2, c["x"].nbytes)
        got = [o.read() for o in (o1, o2)]
        o1.free()
        o2.free()
        assert diff == 0, ("chunked differs from one chunk", kind, diff)
        for (y, guard), what in zip(got, ("chunked", "one chunk")):
            _assert_bits(y.reshape(batch, N), c[kind], (what, kind))
            assert guard == 0, (what, kind)
    dx.free()


@pytest.mark.parametrize("kind", KINDS, ids=K_IDS)
def test_more_than_65535_rows_in_one_call(kind):
    """N = 2, 70000 rows: one chunk, more than one launch's 65535 grid rows"""
    c = _case(2, 70000)
    _run(kind, c["x"], c[kind], (kind, "70000 rows of 2"))


def test_table_cache_eviction_release_and_finalize():
    """five lengths through the four-entry table cache, then the first again (it was evicted); then
    hsfft_release_scratch, a run, hsfft_finalize and a run: every result is bit-exact"""
    for N in (8, 16, 32, 64, 128, 8):
        c = _case(N, 3)
        _run(F.COS, c["x"], c[F.COS], ("cache", N))
        _run(F.SIN, c["x"], c[F.SIN], ("cache, dst4", N))
    c = _case(64, 3)
    hsfft.check(hsfft.lib().hsfft_release_scratch(), "release_scratch")
    _run(F.COS, c["x"], c[F.COS], "after release_scratch")
    _run(F.SIN, c["x"], c[F.SIN], "after release_scratch, dst4")
    hsfft.finalize()
    hsfft.lib().hsfft_set_device(0)
    _run(F.COS, c["x"], c[F.COS], "after finalize")
    _run(F.SIN, c["x"], c[F.SIN], "after finalize, dst4")


@pytest.mark.parametrize("N", [16, 64])
def test_special_values(N):
    """rows of signed zeros, subnormals, values near overflow, one +Inf at index 0, at an odd index
    and at the last index, and one NaN, beside a dense row: the words equal the oracle's, NaN
    positions compared as NaN"""
    x = F.rows(N, 8, salt=0xE7).copy()
    x[0] = np.where(np.arange(N) % 3 == 0, -0.0, 0.0)
    x[1] = x[1] * 1e-310
    x[1, 3], x[1, 4] = 5e-324, -5e-324
    x[2] = x[2] * 1e300
    x[2, 5], x[2, 6] = 1.7e308, -1.7e308
    x[3, 0] = np.inf
    x[4, 5] = np.inf
    x[5, N - 1] = np.inf
    x[6, N // 2 + 1] = np.nan
    assert np.isfinite(x[7]).all()
    for kind in KINDS:
        want = F.oracle_dct4(x, kind)
        assert np.isfinite(want[7]).all() and T.nan_words(want[6]).all() and not np.isfinite(want[3]).all()
        assert np.isfinite(want[1]).all() and T.zero_words(want[0]) == N
        # zeros of both signs come out of the cosine form; the sine form's flip of the odd outputs makes all +0.0
        assert np.signbit(want[0]).any() == (kind == F.COS) and not np.signbit(want[0]).all()
        y = _run(kind, x, want, ("special values", kind, N), compare=_assert_bits_nan_aware)
        assert np.isfinite(y[7]).all()


def test_conveniences():
    N = 256
    c = _case(N, 3)
    for fn, kind in ((hsfft.dct4, F.COS), (hsfft.dst4, F.SIN)):
        y = fn(c["x"])
        assert y.shape == (3, N) and y.dtype == np.float64
        _assert_bits(y, c[kind], (fn.__name__, "2-D input"))
        y = fn(c["x"][1])
        assert y.shape == (N,)
        _assert_bits(y, c[kind][1], (fn.__name__, "1-D input drops the batch axis"))
    x, err_oracle, ref = F.round_trip_errors(N)
    for fn in (hsfft.dct4, hsfft.dst4):
        back = fn(fn(x)) / (2.0 * N)  # either transform is its own inverse up to 2N
        err = float(np.abs(back - x).max())
        print(fn.__name__, "round trip error on the GPU", err, "of the expectation", err_oracle, "reference c2c round trip", ref)
        assert err <= 4 * ref, (fn.__name__, err, ref)
