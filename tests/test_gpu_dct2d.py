"""GPU: the batched 2D cosine and sine transforms hsfft_dct_2d_batched (hsfft_dct2d.h) and the transpose
of 8-byte elements hsfft_transpose_real_batched (tr2d::k_transpose8, hsfft_2d.h).

Tolerance: BIT-EXACT, as everywhere in the suite.  Expected values come from numpy's transpose and
from hsfft_dct2d_testlib.oracle_2d -- hsfft_dct_testlib's 1D expectation on the rows and then on the
columns, checked against long-double direct sums in test_dct2d_cpu.py -- never from the code under
test.  Every output buffer is filled with NaN before the call, so a word that was never written
shows, and lies between sentinel words that must come back unchanged; the inputs are read back
unchanged.
"""
import threading

import numpy as np
import pytest

import hsfft_dct2d_testlib as D2
import hsfft_dct_testlib as D
import hsfft_testlib as T
from test_gpu_dct import Out, _assert_bits, _assert_bits_nan_aware, _upload

import hsfft

pytestmark = pytest.mark.gpu

EDGES = (1, 2, 3, 63, 64, 65, 127, 128, 129)  # around the 64 x 64 tile, on both sides
SMALL = (2, 4, 6, 10, 16, 30, 62, 64, 66)
LEADS = [(0, 0), (1, 0), (0, 3), (1, 3)]       # doubles in front of the input and of the output


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if hsfft.device_count() < 1:
        pytest.skip("no GPU")
    hsfft.lib().hsfft_set_device(0)
    yield
    hsfft.synchronize()
    _IMAGES.clear()
    _ORACLE.clear()


_IMAGES, _ORACLE = {}, {}


def _images(n0, n1, batch, salt=0):
    key = (n0, n1, batch, salt)
    if key not in _IMAGES:
        x = D2.images(n0, n1, batch, salt=0xD0 ^ salt)
        x.setflags(write=False)
        _IMAGES[key] = x
    return _IMAGES[key]


def _want(combo, n0, n1, batch, salt=0):
    """the expected output of `combo` for _images(...), computed once per module and kept read-only"""
    key = (combo, n0, n1, batch, salt)
    if key not in _ORACLE:
        y = D2.oracle_2d(*combo, _images(n0, n1, batch, salt))
        y.setflags(write=False)
        _ORACLE[key] = y
    return _ORACLE[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _transpose(x, what, lead_in=0, lead_out=0):
    """one hsfft_transpose_real_batched of x (batch, rows, cols) on fresh buffers, compared as 8-byte
    words with numpy's transpose"""
    x = np.ascontiguousarray(x)
    batch, rows, cols = x.shape
    xbuf, dx = _upload(x, lead_in)
    out = Out(x.size, lead=lead_out)
    hsfft.transpose_real_batched(dx, out, rows, cols, batch)
    hsfft.synchronize()
    y, guard = out.read()
    xin = xbuf.to_array(np.float64, offset_bytes=lead_in * 8).reshape(x.shape)
    xbuf.free()
    out.free()
    want = np.ascontiguousarray(x.transpose(0, 2, 1))
    bad = int(np.count_nonzero(_bits(y.reshape(want.shape)) != _bits(want)))
    assert bad == 0, (what, "mismatching words", bad, "NaN words left", int(T.nan_words(y).sum()))
    assert guard == 0, (what, "sentinel words changed", guard)
    assert np.array_equal(_bits(xin), _bits(x)), (what, "the input changed")


def _coded(batch, rows, cols):
    """every word distinct, encoding (b, r, c)"""
    b, r, c = np.meshgrid(np.arange(batch), np.arange(rows), np.arange(cols), indexing="ij")
    return ((b * 100000.0 + r) * 100000.0 + c + 0.25).astype(np.float64)


@pytest.mark.parametrize("rows", EDGES)
def test_transpose_tile_edges(rows):
    """tile edges on both sides, partial tiles, single-row and single-column matrices; batch 3"""
    for cols in EDGES:
        x = _coded(3, rows, cols)
        assert np.unique(x).size == x.size
        _transpose(x, ("transpose", rows, cols))


@pytest.mark.parametrize("rows,cols", [(1, 70000), (70000, 1)])
def test_transpose_long_thin_matrices(rows, cols):
    """1094 tiles along one axis, one along the other; batch 2"""
    _transpose(_coded(2, rows, cols), ("transpose", rows, cols))


def test_transpose_on_8_byte_aligned_buffers():
    """input and output each behind an odd number of doubles, in all four combinations"""
    x = _coded(2, 65, 63)
    for lead_in, lead_out in LEADS:
        _transpose(x, ("transpose", lead_in, lead_out), lead_in=lead_in, lead_out=lead_out)


def test_transpose_copies_special_values_verbatim():
    """NaNs with distinct payloads (quiet and signalling, both signs), signed zeros and subnormals come
    back bit for bit: the kernel does no arithmetic"""
    rows, cols = 66, 70
    i = np.arange(rows * cols, dtype=np.uint64)
    w = np.uint64(0x7FF0000000000001) + i * np.uint64(0x0000000100000001)  # NaN: exponent ones, mantissa != 0
    w[1::4] |= np.uint64(1 << 63)
    w[2::8] = np.where(i[2::8] % 16 == 2, np.uint64(0), np.uint64(1 << 63))  # +0.0 and -0.0
    w[3::8] = i[3::8] + np.uint64(1)                                           # subnormals
    w[7::8] = (i[7::8] + np.uint64(1)) | np.uint64(1 << 63)
    nan = T.nan_words(w.view(np.float64))
    assert nan.sum() > w.size // 2 and np.unique(w[nan]).size == nan.sum()
    _transpose(w.view(np.float64).reshape(1, rows, cols), "special values")


# ---------------------------------------------------------------- the 2D transforms
def _run(combo, x, want, what, lead_in=0, lead_out=0, compare=_assert_bits):
    """one hsfft_dct_2d_batched on fresh buffers, checked against `want`"""
    x = np.ascontiguousarray(x)
    batch, n0, n1 = x.shape
    xbuf, dx = _upload(x, lead_in)
    out = Out(x.size, lead=lead_out)
    hsfft.dct_2d_batched(combo[0], combo[1], combo[2], dx, out, n0, n1, batch)
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


def test_the_oracle_tells_swapped_kinds_apart():
    """(COS, SIN) differs from (SIN, COS) on the same non-square input, so the tests below can see a
    swap of kind0 and kind1 or of the axes"""
    x = _images(6, 10, 3)
    for type in (2, 3):
        assert T.mismatches(_want((D.COS, D.SIN, type), 6, 10, 3), _want((D.SIN, D.COS, type), 6, 10, 3)) > 0
    assert not np.array_equal(x[0], x[1])


@pytest.mark.parametrize("combo", D2.COMBOS, ids=D2.combo_id)
def test_small_shapes(combo):
    """n0, n1 each in SMALL, batch 3, images that all differ: one- and two-tile transposes with tile
    edges on either side, h = 1, mixed-radix and Bluestein inner lengths, square and non-square"""
    for n0 in SMALL:
        for n1 in SMALL:
            _run(combo, _images(n0, n1, 3), _want(combo, n0, n1, 3), (combo, n0, n1))


@pytest.mark.parametrize("combo", D2.COMBOS, ids=D2.combo_id)
@pytest.mark.parametrize("n0,n1", [(128, 1000), (1000, 130), (4, 4096), (10006, 4)],
                         ids=["128x1000", "1000x130", "4x4096", "bluestein_10006x4"])
def test_longer_shapes(n0, n1, combo):
    """non-power-of-two mixed-radix lengths on either axis, a long row, and a Bluestein inner length
    (10006 = 2 x 5003) along axis 0; batch 2"""
    _run(combo, _images(n0, n1, 2), _want(combo, n0, n1, 2), (combo, n0, n1))


@pytest.mark.parametrize("combo", D2.COMBOS, ids=D2.combo_id)
def test_equals_the_public_1d_composition_on_the_gpu(combo):
    """hsfft_dct_batched -> hsfft_transpose_real_batched -> hsfft_dct_batched ->
    hsfft_transpose_real_batched gives the same words: hsfft_count_diff_words is 0"""
    kind0, kind1, type = combo
    n0, n1, batch = 62, 130, 5
    x = _images(n0, n1, batch)
    dx = hsfft.DeviceBuffer.from_array(x)
    a, b, c, o = (Out(x.size) for _ in range(4))
    hsfft.dct_2d_batched(kind0, kind1, type, dx, o, n0, n1, batch)
    hsfft.dct_batched(kind1, type, dx, a, n1, batch * n0)
    hsfft.transpose_real_batched(a, b, n0, n1, batch)
    hsfft.dct_batched(kind0, type, b, a, n0, batch * n1)
    hsfft.transpose_real_batched(a, c, n1, n0, batch)
    hsfft.synchronize()
    diff = hsfft.count_diff_words(o, c, x.nbytes)
    y, guard = o.read()
    for d in (dx, a, b, c, o):
        d.free()
    assert diff == 0, (combo, diff)
    _assert_bits(y.reshape(x.shape), _want(combo, n0, n1, batch), combo)
    assert guard == 0


def test_chunk_walk(monkeypatch):
    """HSFFT_2D_CHUNK_MB=1, 64 x 128 images of 64 KiB: the documented rule, bytes / (n0 x n1 x 8), gives
    16 images per chunk, so batch 37 walks chunks of 16, 16 and 5; the result equals the default
    knob's word for word and equals the oracle.  Once more with HSFFT_DCT_CHUNK_MB=1 as well: the row
    transforms then walk each chunk's 1024 and 2048 rows in chunks of their own (508 and 1008 rows)"""
    n0, n1, batch = 64, 128, 37
    assert T.rows_per_chunk(1, n0 * n1 * 8, elem=1) == 16
    assert T.rows_per_chunk(1, n1 * 8 + (n1 // 2 + 1) * 16, elem=1) == 508 < 16 * n0
    assert T.rows_per_chunk(1, n0 * 8 + (n0 // 2 + 1) * 16, elem=1) == 1008 < 16 * n1
    x = _images(n0, n1, batch)
    dx = hsfft.DeviceBuffer.from_array(x)
    for combo in D2.COMBOS:
        outs = [Out(x.size) for _ in range(3)]
        monkeypatch.setenv("HSFFT_2D_CHUNK_MB", "1")
        hsfft.dct_2d_batched(*combo, dx, outs[0], n0, n1, batch)
        monkeypatch.setenv("HSFFT_DCT_CHUNK_MB", "1")
        hsfft.dct_2d_batched(*combo, dx, outs[1], n0, n1, batch)
        monkeypatch.delenv("HSFFT_2D_CHUNK_MB")
        monkeypatch.delenv("HSFFT_DCT_CHUNK_MB")
        hsfft.dct_2d_batched(*combo, dx, outs[2], n0, n1, batch)
        hsfft.synchronize()
        diffs = [hsfft.count_diff_words(o, outs[2], x.nbytes) for o in outs[:2]]
        got = [o.read() for o in outs]
        for o in outs:
            o.free()
        assert diffs == [0, 0], ("chunked differs from one chunk", combo, diffs)
        for (y, guard), what in zip(got, ("chunked", "chunked, nested", "one chunk")):
            _assert_bits(y.reshape(x.shape), _want(combo, n0, n1, batch), (what, combo))
            assert guard == 0, (what, combo)
    dx.free()


@pytest.mark.parametrize("combo", D2.COMBOS, ids=D2.combo_id)
@pytest.mark.parametrize("n0,n1", [(6, 4), (64, 66)])
def test_on_8_byte_aligned_buffers(n0, n1, combo):
    """input and output each behind an odd number of doubles, in all four combinations: caller
    buffers need the alignment of a double only; sentinels in front of the output as well"""
    for lead_in, lead_out in LEADS:
        _run(combo, _images(n0, n1, 3), _want(combo, n0, n1, 3), (combo, n0, n1, lead_in, lead_out), lead_in=lead_in,
             lead_out=lead_out)


def test_special_values():
    """16 x 16 images of signed zeros, subnormals, values near overflow, one +Inf and one NaN, beside a
    dense image: the words equal the oracle's, NaN positions compared as NaN"""
    n = 16
    x = D2.images(n, n, 6, salt=0xE7).copy()
    x[0] = np.where(np.arange(n * n).reshape(n, n) % 3 == 0, -0.0, 0.0)
    x[1] = x[1] * 1e-310
    x[1, 3, 3], x[1, 4, 5] = 5e-324, -5e-324
    x[2] = x[2] * 1e300
    x[2, 5, 6], x[2, 6, 5] = 1.7e308, -1.7e308
    x[3, 2, 5] = np.inf
    x[4, n // 2 + 1, 3] = np.nan
    assert np.isfinite(x[5]).all()
    for combo in D2.COMBOS:
        want = D2.oracle_2d(*combo, x)
        assert np.isfinite(want[5]).all() and np.isfinite(want[1]).all() and T.zero_words(want[0]) == n * n
        assert T.nan_words(want[4]).all() and not np.isfinite(want[3]).all()
        y = _run(combo, x, want, ("special values", combo), compare=_assert_bits_nan_aware)
        assert np.isfinite(y[5]).all()


def test_release_scratch_and_finalize():
    """hsfft_release_scratch, then a call; hsfft_finalize, then hsfft_set_device and a call"""
    n0, n1 = 30, 64
    c1, c2 = (D.COS, D.SIN, 2), (D.SIN, D.COS, 3)
    _run(c1, _images(n0, n1, 3), _want(c1, n0, n1, 3), "before")
    hsfft.check(hsfft.lib().hsfft_release_scratch(), "release_scratch")
    _run(c1, _images(n0, n1, 3), _want(c1, n0, n1, 3), "after release_scratch")
    _run(c2, _images(n0, n1, 3), _want(c2, n0, n1, 3), "after release_scratch, type 3")
    hsfft.finalize()
    hsfft.lib().hsfft_set_device(0)
    _run(c1, _images(n0, n1, 3), _want(c1, n0, n1, 3), "after finalize")
    _run(c2, _images(n0, n1, 3), _want(c2, n0, n1, 3), "after finalize, type 3")


def test_two_threads_with_different_shapes():
    """two host threads on one device call different shapes and transforms at once, each four times:
    the device lock serialises the calls, the scratch and both caches, and both get the oracle's bits"""
    jobs = [((30, 64), [(D.COS, D.COS, 2), (D.SIN, D.COS, 3)]), ((64, 1000), [(D.COS, D.SIN, 3), (D.SIN, D.SIN, 2)])]
    for (n0, n1), combos in jobs:  # the expectations, before the threads start
        for combo in combos:
            _want(combo, n0, n1, 3)
    errors, start = [], threading.Barrier(2)

    def work(shape, combos):
        try:
            hsfft.lib().hsfft_set_device(0)
            start.wait(timeout=60)
            for rep in range(4):
                for combo in combos:
                    _run(combo, _images(*shape, 3), _want(combo, *shape, 3), ("thread", shape, combo, rep))
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((shape, repr(e)))

    threads = [threading.Thread(target=work, args=job) for job in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    assert not errors, errors


def test_conveniences():
    n0, n1 = 32, 64
    x = _images(n0, n1, 3)
    for fn, kind in ((hsfft.dctn, D.COS), (hsfft.dstn, D.SIN)):
        for type in (2, 3):
            want = _want((kind, kind, type), n0, n1, 3)
            y = fn(x, type=type)
            assert y.shape == (3, n0, n1) and y.dtype == np.float64
            _assert_bits(y, want, (fn.__name__, type, "3-D input"))
            y = fn(x[1], type=type)
            assert y.shape == (n0, n1) and y.dtype == np.float64
            _assert_bits(y, want[1], (fn.__name__, type, "a plain 2-D array"))
    _assert_bits(hsfft.dctn(x), _want((D.COS, D.COS, 2), n0, n1, 3), "type defaults to 2")
    y = hsfft.dstn(x.reshape(1, 3, n0, n1))
    assert y.shape == (1, 3, n0, n1)
    _assert_bits(y[0], _want((D.SIN, D.SIN, 2), n0, n1, 3), "leading axes are the batch")
    # the inverse is the other type and one division by 4.0 * n0 * n1 per word
    _assert_bits(hsfft.idctn(x, type=2), _want((D.COS, D.COS, 3), n0, n1, 3) / (4.0 * n0 * n1), "idctn")
    _assert_bits(hsfft.idstn(x, type=3), _want((D.SIN, D.SIN, 2), n0, n1, 3) / (4.0 * n0 * n1), "idstn")
    _, _, ref = D.round_trip_errors(n1)
    for fwd, inv in ((hsfft.dctn, hsfft.idctn), (hsfft.dstn, hsfft.idstn)):
        back = inv(fwd(x[0]))
        assert back.shape == (n0, n1)
        err = float(np.abs(back - x[0]).max())
        print(fwd.__name__, "round trip error on the GPU", err, "reference 1D round trip at N = 64", ref, "ratio", err / ref)
        assert err <= 8 * ref, (fwd.__name__, err, ref)
