"""GPU: the batched type-I cosine and sine transforms hsfft_dct1_batched and hsfft_dct1_2d_batched
(hsfft_dct1.h).

Tolerance: BIT-EXACT, as everywhere in the suite.  Expected values come from hsfft_dct1_testlib alone
-- numpy's symmetric extension around the reference's r2c of the pinned oracle, a slice of .real or
of -.imag (checked against long-double direct sums of scipy's definitions in test_dct1_cpu.py) --
never from the code under test.  Every output buffer is filled with NaN before the call, so a word
that was never written shows, and lies between sentinel words that must come back unchanged; the
inputs are read back unchanged.
"""
import threading

import numpy as np
import pytest

import hsfft_dct1_testlib as D1
import hsfft_testlib as T
from test_gpu_dct import Out, _assert_bits, _assert_bits_nan_aware, _upload

import hsfft

pytestmark = pytest.mark.gpu

KINDS = [D1.COS, D1.SIN]
K_IDS = ["dct1", "dst1"]
PAIRS = [(D1.COS, D1.COS), (D1.COS, D1.SIN), (D1.SIN, D1.COS), (D1.SIN, D1.SIN)]
P_IDS = ["cos_cos", "cos_sin", "sin_cos", "sin_sin"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if hsfft.device_count() < 1:
        pytest.skip("no GPU")
    hsfft.lib().hsfft_set_device(0)
    yield
    hsfft.synchronize()
    _ORACLE.clear()


_ORACLE = {}


def _case(kind, n, batch, salt=0, flags=0):
    """the rows x (batch, n) and the expected output, computed once per module and kept read-only"""
    key = (kind, n, batch, salt, flags)
    if key not in _ORACLE:
        x = D1.rows(n, batch, salt=0xD0 ^ salt)
        want = D1.oracle(kind, x, flags)
        x.setflags(write=False)
        want.setflags(write=False)
        _ORACLE[key] = (x, want)
    return _ORACLE[key]


def _case_2d(pair, n0, n1, batch):
    key = ("2d", pair, n0, n1, batch)
    if key not in _ORACLE:
        x = D1.rows(n0 * n1, batch, salt=0x2D).reshape(batch, n0, n1)
        want = D1.oracle_2d(pair[0], pair[1], x)
        x.setflags(write=False)
        want.setflags(write=False)
        _ORACLE[key] = (x, want)
    return _ORACLE[key]


def _run(kind, x, want, what, lead_in=0, lead_out=0, compare=_assert_bits, pair=None):
    """one call on fresh buffers, checked against `want`; lead_in / lead_out: doubles in front of the
    input and of the output; pair: (kind0, kind1) of a 2D call on x (batch, n0, n1)"""
    x = np.ascontiguousarray(x)
    xbuf, dx = _upload(x, lead_in)
    out = Out(x.size, lead=lead_out)
    if pair is None:
        hsfft.dct1_batched(kind, dx, out, x.shape[1], x.shape[0])
    else:
        hsfft.dct1_2d_batched(pair[0], pair[1], dx, out, x.shape[1], x.shape[2], x.shape[0])
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
def test_every_length_to_130(kind):
    """batch 3, dense rows that all differ, every n from 2 (cosine) or 1 (sine) to 130: both parities,
    the rows with no mirrored word (cosine n = 2: L = 2; sine n = 1: L = 4), and power-of-two,
    mixed-radix and Bluestein inner lengths"""
    for n in range(1 if kind == D1.SIN else 2, 131):
        x, want = _case(kind, n, 3)
        assert not np.array_equal(x[0], x[1])
        _run(kind, x, want, (kind, n))


@pytest.mark.parametrize("kind", KINDS, ids=K_IDS)
@pytest.mark.parametrize("n_cos,n_sin,batch", [(1025, 1025, 3), (4097, 4097, 3), (12601, 12599, 3), (32769, 32767, 2), (5004, 5002, 2)],
                         ids=["1025", "4097", "L25200", "L65536", "bluestein_L10006"])
def test_longer_rows(n_cos, n_sin, batch, kind):
    """more than one block per row; L = 25200, whose inner transform is the 12600-point row kernel;
    L = 65536, a two-pass inner transform; L = 10006 = 2 x 5003, a Bluestein inner length"""
    n = n_sin if kind == D1.SIN else n_cos
    x, want = _case(kind, n, batch)
    _run(kind, x, want, (kind, n, batch))


@pytest.mark.parametrize("kind", KINDS, ids=K_IDS)
@pytest.mark.parametrize("n", [7, 64])
def test_on_8_byte_aligned_buffers(n, kind):
    """input and output each behind an odd number of doubles, in all four combinations: caller
    buffers need the alignment of a double only; sentinels in front of the output as well"""
    x, want = _case(kind, n, 3)
    for lead_in, lead_out in [(0, 0), (1, 0), (0, 3), (1, 3)]:
        _run(kind, x, want, (kind, n, lead_in, lead_out), lead_in=lead_in, lead_out=lead_out)


@pytest.mark.parametrize("kind,n", [(D1.COS, 2049), (D1.SIN, 2047)], ids=K_IDS)
def test_chunk_walk(monkeypatch, kind, n):
    """HSFFT_DCT_CHUNK_MB=1, L = 4096, 37 rows: the documented rule, bytes / (L x 8 + (L/2+1) x 16),
    gives 15 rows per chunk, so chunks of 15, 15 and 7; the result equals the default knob's word
    for word and equals the oracle"""
    batch = 37
    assert hsfft.dct1_shape(kind, n) == (4096, 2049)
    assert D1.chunk_rows(kind, n, 1) == 15 == (1 << 20) // (4096 * 8 + 2049 * 16)
    x, want = _case(kind, n, batch)
    dx = hsfft.DeviceBuffer.from_array(x)
    o1, o2 = Out(x.size), Out(x.size)
    monkeypatch.setenv("HSFFT_DCT_CHUNK_MB", "1")
    hsfft.dct1_batched(kind, dx, o1, n, batch)
    monkeypatch.delenv("HSFFT_DCT_CHUNK_MB")
    hsfft.dct1_batched(kind, dx, o2, n, batch)
    hsfft.synchronize()
    diff = hsfft.count_diff_words(o1, o2, x.nbytes)
    got = [o.read() for o in (o1, o2)]
    for d in (o1, o2, dx):
        d.free()
    assert diff == 0, ("chunked differs from one chunk", kind, diff)
    for (y, guard), what in zip(got, ("chunked", "one chunk")):
        _assert_bits(y.reshape(batch, n), want, (what, kind))
        assert guard == 0, (what, kind)


@pytest.mark.parametrize("kind", KINDS, ids=K_IDS)
def test_more_than_65535_rows_in_one_call(kind):
    """n = 2, 70000 rows: one chunk, more than one launch's 65535 grid rows"""
    x, want = _case(kind, 2, 70000)
    _run(kind, x, want, (kind, "70000 rows of 2"))


def test_dirty_scratch_release_and_finalize():
    """a longer call leaves its words in both pool buffers; the shorter calls after it get the oracle's
    bits all the same -- the sine rows rely on the two +0.0 words the kernel stores itself, and on every
    other word of the extension being written.  Then hsfft_release_scratch and again, hsfft_finalize
    and again."""
    def both(what):
        for kind, n in ((D1.COS, 1000), (D1.SIN, 15), (D1.SIN, 1), (D1.COS, 2), (D1.SIN, 100), (D1.COS, 17)):
            x, want = _case(kind, n, 5)
            _run(kind, x, want, (what, kind, n))
    big = np.arange(4 * 4097, dtype=np.float64).reshape(4, 4097) + 1.0  # no zero word anywhere
    _run(D1.COS, big, D1.oracle(D1.COS, big), "the longer call first")
    both("after a longer call")
    hsfft.check(hsfft.lib().hsfft_release_scratch(), "release_scratch")
    both("after release_scratch")
    hsfft.finalize()
    hsfft.lib().hsfft_set_device(0)
    both("after finalize")


@pytest.mark.parametrize("kind,n", [(D1.COS, 17), (D1.SIN, 15)], ids=K_IDS)
def test_special_values(kind, n):
    """L = 32.  Rows of signed zeros, subnormals, values near overflow, one +Inf at index 0, at an odd
    index and at the last index, and one NaN, beside a dense row: the words equal the oracle's, NaN
    positions compared as NaN"""
    x = D1.rows(n, 8, salt=0xE7).copy()
    x[0] = np.where(np.arange(n) % 3 == 0, -0.0, 0.0)
    x[1] = x[1] * 1e-310
    x[1, 3], x[1, 4] = 5e-324, -5e-324
    x[2] = x[2] * 1e300
    x[2, 5], x[2, 6] = 1.7e308, -1.7e308
    x[3, 0] = np.inf
    x[4, 5] = np.inf
    x[5, n - 1] = np.inf
    x[6, n // 2 + 1] = np.nan
    assert np.isfinite(x[7]).all()
    want = D1.oracle(kind, x)
    assert np.isfinite(want[7]).all() and T.nan_words(want[6]).all() and not np.isfinite(want[3]).all()
    assert np.isfinite(want[1]).all() and T.zero_words(want[0]) == n
    y = _run(kind, x, want, ("special values", kind, n), compare=_assert_bits_nan_aware)
    assert np.isfinite(y[7]).all()


def test_either_twiddle_mode_against_its_own_oracle():
    """n = 7 and 13 in the reference mode, the exact mode and the reference mode again, each against the
    oracle with the matching flag: the plan follows the calling thread's mode.  The cosine extensions
    (L = 12 and 24) meet the reference's quirk, so there the two oracles differ and a plan of the wrong
    mode would show; the sine extension of 7 (L = 16) is a power of two and the same in both"""
    differ = {}
    try:
        for kind in KINDS:
            for n in (7, 13):
                for mode, flags in (("reference", 0), ("exact", T.ORC_EXACT), ("reference", 0)):
                    hsfft.set_twiddle_mode(mode)
                    x, want = _case(kind, n, 3, flags=flags)
                    _run(kind, x, want, ("twiddle mode", mode, kind, n))
                differ[(kind, n)] = T.mismatches(_case(kind, n, 3, flags=0)[1], _case(kind, n, 3, flags=T.ORC_EXACT)[1]) > 0
    finally:
        hsfft.set_twiddle_mode("reference")
    print("the exact-twiddle oracle differs:", differ)
    assert differ[(D1.COS, 7)] and differ[(D1.COS, 13)]


@pytest.mark.parametrize("pair", PAIRS, ids=P_IDS)
@pytest.mark.parametrize("n0,n1", [(3, 5), (9, 8), (33, 17), (65, 64)])
def test_2d_images(n0, n1, pair):
    """3 images: odd and even axes, odd images (an odd number of doubles per image, so the second image
    is only 8-byte aligned), more than one transpose tile; against the 1D expectation on every row and
    then on every column of that result"""
    x, want = _case_2d(pair, n0, n1, 3)
    _run(None, x, want, (pair, n0, n1), pair=pair)
    _run(None, x, want, (pair, n0, n1, "8-byte aligned"), lead_in=1, lead_out=3, pair=pair)


def test_2d_is_rows_then_columns_of_the_1d_call():
    """word for word hsfft_dct1_batched on every row, the transpose, hsfft_dct1_batched on every column,
    the transpose: 33 x 17, cosine columns and sine rows"""
    pair, n0, n1, batch = (D1.COS, D1.SIN), 33, 17, 3
    x, want = _case_2d(pair, n0, n1, batch)
    dx = hsfft.DeviceBuffer.from_array(x)
    o, a, b, c = (Out(x.size) for _ in range(4))
    hsfft.dct1_2d_batched(pair[0], pair[1], dx, o, n0, n1, batch)
    hsfft.dct1_batched(pair[1], dx, a, n1, batch * n0)
    hsfft.transpose_real_batched(a, b, n0, n1, batch)
    hsfft.dct1_batched(pair[0], b, a, n0, batch * n1)
    hsfft.transpose_real_batched(a, c, n1, n0, batch)
    hsfft.synchronize()
    diff = hsfft.count_diff_words(o, c, x.nbytes)
    y, guard = o.read()
    for d in (dx, a, b, c, o):
        d.free()
    assert diff == 0 and guard == 0
    _assert_bits(y.reshape(x.shape), want, pair)


def test_2d_chunk_walk(monkeypatch):
    """HSFFT_2D_CHUNK_MB=1, 33 x 17 images of 561 doubles: the documented rule counts 16-byte words, so
    bytes / (16 x ceil(561 / 2)) gives 233 images per chunk, and batch 500 walks chunks of 233, 233 and
    34, the second of which starts at an odd double; the result equals the default knob's word for
    word and equals the oracle.  Once more with HSFFT_DCT_CHUNK_MB=1 as well: the row transforms then
    walk each chunk's 7689 and 3961 rows in chunks of their own"""
    pair, n0, n1, batch = (D1.SIN, D1.COS), 33, 17, 500
    assert T.rows_per_chunk(1, 16 * ((n0 * n1 + 1) // 2), elem=1) == 233
    assert D1.chunk_rows(pair[1], n1, 1) < 233 * n0 and D1.chunk_rows(pair[0], n0, 1) < 233 * n1
    x, want = _case_2d(pair, n0, n1, batch)
    dx = hsfft.DeviceBuffer.from_array(x)
    outs = [Out(x.size) for _ in range(3)]
    monkeypatch.setenv("HSFFT_2D_CHUNK_MB", "1")
    hsfft.dct1_2d_batched(pair[0], pair[1], dx, outs[0], n0, n1, batch)
    monkeypatch.setenv("HSFFT_DCT_CHUNK_MB", "1")
    hsfft.dct1_2d_batched(pair[0], pair[1], dx, outs[1], n0, n1, batch)
    monkeypatch.delenv("HSFFT_2D_CHUNK_MB")
    monkeypatch.delenv("HSFFT_DCT_CHUNK_MB")
    hsfft.dct1_2d_batched(pair[0], pair[1], dx, outs[2], n0, n1, batch)
    hsfft.synchronize()
    diffs = [hsfft.count_diff_words(o, outs[2], x.nbytes) for o in outs[:2]]
    got = [o.read() for o in outs]
    for d in outs + [dx]:
        d.free()
    assert diffs == [0, 0], ("chunked differs from one chunk", diffs)
    for (y, guard), what in zip(got, ("chunked", "chunked, nested", "one chunk")):
        _assert_bits(y.reshape(x.shape), want, what)
        assert guard == 0, what


def test_python_wrappers():
    for fn, inv, kind, n in ((hsfft.dct1, hsfft.idct1, D1.COS, 257), (hsfft.dst1, hsfft.idst1, D1.SIN, 255)):
        x, want = _case(kind, n, 3)
        y = fn(x)
        assert y.shape == (3, n) and y.dtype == np.float64
        _assert_bits(y, want, (fn.__name__, "2-D input"))
        y = fn(x[1])
        assert y.shape == (n,)
        _assert_bits(y, want[1], (fn.__name__, "1-D input drops the batch axis"))
        # the inverse is the same transform and one division per word
        _assert_bits(inv(x), want / D1.factor(kind, n), inv.__name__)
        _, err_oracle, ref = D1.round_trip_errors(kind, n)
        x1 = D1.rows(n, 1, salt=0xA1)[0]
        back = inv(fn(x1))
        assert back.shape == (n,)
        err = float(np.abs(back - x1).max())
        print(fn.__name__, "round trip error on the GPU", err, "of the expectation", err_oracle, "reference round trip", ref)
        assert err <= 4 * ref, (fn.__name__, err, ref)
    y = hsfft.dst1(np.arange(1, 6, dtype=np.int32))  # any real dtype is converted; an odd length
    _assert_bits(y, D1.oracle(D1.SIN, np.arange(1.0, 6.0)[None, :])[0], "dst1 of an integer row")
    for fn, inv, kind in ((hsfft.dct1n, hsfft.idct1n, D1.COS), (hsfft.dst1n, hsfft.idst1n, D1.SIN)):
        x, want = _case_2d((kind, kind), 9, 8, 3)
        y = fn(x)
        assert y.shape == (3, 9, 8) and y.dtype == np.float64
        _assert_bits(y, want, (fn.__name__, "3-D input"))
        y = fn(x[2])
        assert y.shape == (9, 8)
        _assert_bits(y, want[2], (fn.__name__, "2-D input drops the batch axis"))
        y = fn(x.reshape(1, 3, 9, 8))
        _assert_bits(y, want.reshape(1, 3, 9, 8), (fn.__name__, "leading axes are the batch"))
        _assert_bits(inv(x), want / (D1.factor(kind, 9) * D1.factor(kind, 8)), inv.__name__)


def test_two_threads_with_different_lengths():
    """two host threads on one device call different lengths and kinds at once: the device lock
    serialises the calls and the scratch, and both get the oracle's bits"""
    jobs = [(1001, [D1.COS, D1.SIN]), (4097, [D1.SIN, D1.COS])]
    cases = [{kind: _case(kind, n, 3) for kind in kinds} for n, kinds in jobs]
    errors, start = [], threading.Barrier(2)

    def work(n, kinds, c):
        try:
            hsfft.lib().hsfft_set_device(0)
            start.wait(timeout=60)
            for rep in range(4):
                for kind in kinds:
                    _run(kind, c[kind][0], c[kind][1], ("thread", n, kind, rep))
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((n, repr(e)))

    threads = [threading.Thread(target=work, args=(n, kinds, c)) for (n, kinds), c in zip(jobs, cases)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    assert not errors, errors
