"""GPU: the batched cosine and sine transforms hsfft_dct_batched (hsfft_dct.h).

Tolerance: BIT-EXACT, as everywhere in the suite.  Expected values come from hsfft_dct_testlib alone
-- libm's sincos table, numpy's permutations, float64 rotations and sign-bit flips around the
reference's r2c / c2r of the pinned oracle (checked against long-double direct sums of scipy's
definitions in test_dct_cpu.py) -- never from the code under test.  Every output buffer is filled
with NaN before the call, so a word that was never written shows, and lies between sentinel words
that must come back unchanged; the inputs are read back unchanged.
"""
import threading

import numpy as np
import pytest

import hsfft_dct_testlib as D
import hsfft_testlib as T

import hsfft

pytestmark = pytest.mark.gpu

SENTINEL = -12345.6789
TAIL = 4096  # sentinel doubles behind every output

KINDS_TYPES = [(D.COS, 2), (D.COS, 3), (D.SIN, 2), (D.SIN, 3)]
KT_IDS = ["dct2", "dct3", "dst2", "dst3"]


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
    """the rows x (batch, N) and the four expected outputs, computed once per module and kept read-only"""
    key = (N, batch, salt)
    if key not in _ORACLE:
        x = D.rows(N, batch, salt=0xD0 ^ salt)
        val = {"x": x}
        for kind, type in KINDS_TYPES:
            val[(kind, type)] = D.oracle(kind, type, x)
        for a in val.values():
            a.setflags(write=False)
        _ORACLE[key] = val
    return _ORACLE[key]


class Out:
    """an output buffer of `count` doubles filled with NaN, between `lead` sentinel doubles in front
    (an odd lead makes the output only 8-byte aligned) and TAIL behind"""

    def __init__(self, count, lead=0):
        self.lead, self.count = lead, count
        img = np.full(lead + count + TAIL, SENTINEL)
        img[lead:lead + count] = np.nan
        self.buf = hsfft.DeviceBuffer.from_array(img)
        self.ptr = self.buf.ptr + 8 * lead
        self.nbytes = 8 * count

    def read(self):
        """(the output words, the number of sentinel words that changed)"""
        img = self.buf.to_array(np.float64)
        guard = np.concatenate([img[:self.lead], img[self.lead + self.count:]])
        return img[self.lead:self.lead + self.count].copy(), int(np.count_nonzero(guard != SENTINEL))

    def free(self):
        self.buf.free()


def _assert_bits(y, want, what):
    bad = T.mismatches(y, want)
    assert bad == 0, (what, "mismatching words", bad, "first at", T.first_diff(y, want),
                      "NaN words left", int(T.nan_words(y).sum()))


def _assert_bits_nan_aware(y, want, what):
    assert T.same_bits_nan_aware(y, want), (what, "NaN words", int(T.nan_words(y).sum()), "expected",
                                            int(T.nan_words(want).sum()))


def _upload(a, lead):
    """a on the device behind `lead` doubles: (owning buffer, the view that starts at a)"""
    buf = hsfft.DeviceBuffer(lead * 8 + a.nbytes)
    view = hsfft.DeviceView(buf, lead * 8)
    hsfft.check(hsfft.lib().hsfft_memcpy_h2d(view.ptr, a.ctypes.data, a.nbytes), "h2d")
    return buf, view


def _run(kind, type, x, want, what, lead_in=0, lead_out=0, compare=_assert_bits):
    """one call on fresh buffers, checked against `want`; lead_in / lead_out: doubles in front of the
    input and of the output"""
    x = np.ascontiguousarray(x)
    batch, N = x.shape
    xbuf, dx = _upload(x, lead_in)
    out = Out(x.size, lead=lead_out)
    hsfft.dct_batched(kind, type, dx, out, N, batch)
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


@pytest.mark.parametrize("kind,type", KINDS_TYPES, ids=KT_IDS)
def test_every_even_length_to_128(kind, type):
    """batch 3, dense rows that all differ: h = 1 (N = 2, no mirrored output), k == h, odd and even h,
    one-point to 64-point inner transforms, mixed-radix and Bluestein inner lengths"""
    for N in range(2, 130, 2):
        c = _case(N, 3)
        assert not np.array_equal(c["x"][0], c["x"][1])
        _run(kind, type, c["x"], c[(kind, type)], (kind, type, N))


@pytest.mark.parametrize("kind,type", KINDS_TYPES, ids=KT_IDS)
@pytest.mark.parametrize("N,batch", [(1000, 3), (4096, 3), (12600, 3), (65536, 2), (10006, 2)],
                         ids=["1000", "4096", "12600", "65536", "bluestein_10006"])
def test_longer_rows(N, batch, kind, type):
    """more than one block per row, a non-power-of-two mixed-radix length, the 12600 row kernel's
    length, two-pass inner transforms, and a Bluestein inner length (10006 = 2 x 5003)"""
    c = _case(N, batch)
    _run(kind, type, c["x"], c[(kind, type)], (kind, type, N, batch))


@pytest.mark.parametrize("kind,type", KINDS_TYPES, ids=KT_IDS)
@pytest.mark.parametrize("N", [6, 64])
def test_on_8_byte_aligned_buffers(N, kind, type):
    """input and output each behind an odd number of doubles, in all four combinations: caller
    buffers need the alignment of a double only; sentinels in front of the output as well"""
    c = _case(N, 3)
    for lead_in, lead_out in [(0, 0), (1, 0), (0, 3), (1, 3)]:
        _run(kind, type, c["x"], c[(kind, type)], (kind, type, N, lead_in, lead_out), lead_in=lead_in, lead_out=lead_out)


def test_chunk_walk(monkeypatch):
    """HSFFT_DCT_CHUNK_MB=1, N = 4096, 37 rows: the documented rule, bytes / (N x 8 + (N/2+1) x 16),
    gives 15 rows per chunk, so chunks of 15, 15 and 7; the result equals the default knob's word
    for word and equals the oracle"""
    N, batch = 4096, 37
    assert T.rows_per_chunk(1, N * 8 + (N // 2 + 1) * 16, elem=1) == 15
    c = _case(N, batch)
    dx = hsfft.DeviceBuffer.from_array(c["x"])
    for kind, type in KINDS_TYPES:
        o1, o2 = Out(c["x"].size), Out(c["x"].size)
        monkeypatch.setenv("HSFFT_DCT_CHUNK_MB", "1")
        hsfft.dct_batched(kind, type, dx, o1, N, batch)
        monkeypatch.delenv("HSFFT_DCT_CHUNK_MB")
        hsfft.dct_batched(kind, type, dx, o2, N, batch)
        hsfft.synchronize()
        diff = hsfft.count_diff_words(o1, o2, c["x"].nbytes)
        got = [o.read() for o in (o1, o2)]
        o1.free()
        o2.free()
        assert diff == 0, ("chunked differs from one chunk", kind, type, diff)
        for (y, guard), what in zip(got, ("chunked", "one chunk")):
            _assert_bits(y.reshape(batch, N), c[(kind, type)], (what, kind, type))
            assert guard == 0, (what, kind, type)
    dx.free()


@pytest.mark.parametrize("kind,type", KINDS_TYPES, ids=KT_IDS)
def test_more_than_65535_rows_in_one_call(kind, type):
    """N = 2, 70000 rows: one chunk, more than one launch's 65535 grid rows"""
    c = _case(2, 70000)
    _run(kind, type, c["x"], c[(kind, type)], (kind, type, "70000 rows of 2"))


def test_table_cache_eviction_release_and_finalize():
    """five lengths through the four-entry table cache, then the first again (it was evicted); then
    hsfft_release_scratch, a run, hsfft_finalize and a run: every result is bit-exact"""
    kind, type = D.COS, 2
    for N in (8, 16, 32, 64, 128, 8):
        c = _case(N, 3)
        _run(kind, type, c["x"], c[(kind, type)], ("cache", N))
        _run(D.SIN, 3, c["x"], c[(D.SIN, 3)], ("cache, dst3", N))
    c = _case(64, 3)
    hsfft.check(hsfft.lib().hsfft_release_scratch(), "release_scratch")
    _run(kind, type, c["x"], c[(kind, type)], "after release_scratch")
    _run(D.COS, 3, c["x"], c[(D.COS, 3)], "after release_scratch, dct3")
    hsfft.finalize()
    hsfft.lib().hsfft_set_device(0)
    _run(kind, type, c["x"], c[(kind, type)], "after finalize")
    _run(D.SIN, 2, c["x"], c[(D.SIN, 2)], "after finalize, dst2")


@pytest.mark.parametrize("N", [16, 64])
def test_special_values(N):
    """rows of signed zeros, subnormals, values near overflow, one +Inf at index 0, at an odd index
    and at the last index, and one NaN, beside a dense row: the words equal the oracle's, NaN
    positions compared as NaN"""
    x = D.rows(N, 8, salt=0xE7).copy()
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
    for kind, type in KINDS_TYPES:
        want = D.oracle(kind, type, x)
        assert np.isfinite(want[7]).all() and T.nan_words(want[6]).all() and not np.isfinite(want[3]).all()
        assert np.isfinite(want[1]).all() and T.zero_words(want[0]) == N
        y = _run(kind, type, x, want, ("special values", kind, type, N), compare=_assert_bits_nan_aware)
        assert np.isfinite(y[7]).all()
    # type 3 takes V[0] over without arithmetic: an infinite X[0] (X[N-1] for the sine transform) leaves
    # infinite words in half of the row, where a rotation of V[0] would have made every word NaN
    for kind, row in ((D.COS, 3), (D.SIN, 5)):
        want = D.oracle(kind, 3, x[row:row + 1])
        assert T.inf_words(want) == N // 2 and int(T.nan_words(want).sum()) == N // 2


def test_conveniences():
    N = 256
    c = _case(N, 3)
    for fn, kind in ((hsfft.dct, D.COS), (hsfft.dst, D.SIN)):
        for type in (2, 3):
            y = fn(c["x"], type=type)
            assert y.shape == (3, N) and y.dtype == np.float64
            _assert_bits(y, c[(kind, type)], (fn.__name__, type, "2-D input"))
            y = fn(c["x"][1], type=type)
            assert y.shape == (N,)
            _assert_bits(y, c[(kind, type)][1], (fn.__name__, type, "1-D input drops the batch axis"))
    _assert_bits(hsfft.dct(c["x"]), c[(D.COS, 2)], "type defaults to 2")
    # the inverse is the other type and one division by 2.0 * n per word
    _assert_bits(hsfft.idct(c["x"], type=2), c[(D.COS, 3)] / (2.0 * N), "idct")
    _assert_bits(hsfft.idst(c["x"], type=3), c[(D.SIN, 2)] / (2.0 * N), "idst")
    x, err_oracle, ref = D.round_trip_errors(N)
    for fwd, inv in ((hsfft.dct, hsfft.idct), (hsfft.dst, hsfft.idst)):
        back = inv(fwd(x))
        assert back.shape == (N,)
        err = float(np.abs(back - x).max())
        print(fwd.__name__, "round trip error on the GPU", err, "of the expectation", err_oracle, "reference round trip", ref)
        assert err <= 4 * ref, (fwd.__name__, err, ref)


def test_two_threads_with_different_lengths():
    """two host threads on one device call different lengths and transforms at once: the device lock
    serialises the calls, the scratch and the table cache, and both get the oracle's bits"""
    jobs = [(1000, [(D.COS, 2), (D.SIN, 3)]), (4096, [(D.COS, 3), (D.SIN, 2)])]
    cases = [_case(N, 3) for N, _ in jobs]
    errors, start = [], threading.Barrier(2)

    def work(N, kts, c):
        try:
            hsfft.lib().hsfft_set_device(0)
            start.wait(timeout=60)
            for rep in range(4):
                for kind, type in kts:
                    _run(kind, type, c["x"], c[(kind, type)], ("thread", N, kind, type, rep))
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((N, repr(e)))

    threads = [threading.Thread(target=work, args=(N, kts, c)) for (N, kts), c in zip(jobs, cases)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    assert not errors, errors
