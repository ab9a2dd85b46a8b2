"""GPU: the batched overlap-add filter hsfft_filter_batched (hsfft_filter.h).

Tolerance: BIT-EXACT, as everywhere in the suite.  Expected values come from hsfft_filter_testlib
alone -- the reference's fft_convolve of every block through the pinned oracle, joined by the
full[g] formula with one float64 add per overlapped word and cut by the restated window rule
(checked against a long-double direct convolution and pinned to the one-shot reference result in
test_filter_cpu.py) -- never from the code under test.  Every output buffer is filled with NaN
before the call, so a word that was never written shows, and lies between sentinel words that
must come back unchanged; both inputs are read back unchanged.
"""
import numpy as np
import pytest

import hsfft_filter_testlib as F
import hsfft_testlib as T

import hsfft

pytestmark = pytest.mark.gpu

SENTINEL = -12345.6789
TAIL = 4096  # sentinel doubles behind every output


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if hsfft.device_count() < 1:
        pytest.skip("no GPU")
    hsfft.lib().hsfft_set_device(0)
    yield
    hsfft.synchronize()
    _ORACLE.clear()


_ORACLE = {}


def _cached(key, make):
    """expected values computed once per module and kept read-only"""
    if key not in _ORACLE:
        val = make()
        for a in val if isinstance(val, tuple) else (val,):
            a.setflags(write=False)
        _ORACLE[key] = val
    return _ORACLE[key]


def _block(n, m, block):
    """the padded block length of a case (block 0: what the library's automatic rule gives)"""
    P = hsfft.filter_shape("full", n, m, block)[1]
    assert block == 0 or P == block
    return P


def _case(n, m, block, batch=3, salt=0):
    """(x (batch, n) dense, h (m,), the overlap-added full results (batch, n + m - 1)): one oracle
    run per case serves every window and every smaller batch (rows are independent)"""
    def make():
        x, h = F.rows(n, batch, salt=0xF5 ^ salt), F.kernel(m, salt=0xF5 ^ salt)
        return x, h, F.oracle_full_rows(x, h, _block(n, m, block))
    return _cached((n, m, block, batch, salt), make)


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
        return img[self.lead:self.lead + self.count], int(np.count_nonzero(guard != SENTINEL))

    def free(self):
        self.buf.free()


def _assert_bits(y, want, what):
    bad = T.mismatches(y, want)
    assert bad == 0, (what, "mismatching words", bad, "first at", T.first_diff(y, want),
                      "NaN words left", int(T.nan_words(y).sum()))


def _upload(x, lead):
    """x on the device behind `lead` doubles: (owning buffer, the view that starts at x)"""
    buf = hsfft.DeviceBuffer(lead * 8 + x.nbytes)
    view = hsfft.DeviceView(buf, lead * 8)
    hsfft.check(hsfft.lib().hsfft_memcpy_h2d(view.ptr, x.ctypes.data, x.nbytes), "h2d")
    return buf, view


def _run(typ, x, h, block, want, what, lead=0, compare=_assert_bits):
    """one call on fresh buffers, checked against `want`; lead: doubles in front of every buffer"""
    x, h = np.ascontiguousarray(x), np.ascontiguousarray(h)
    batch, n = x.shape
    (xbuf, dx), (hbuf, dh) = _upload(x, lead), _upload(h, lead)
    out = Out(want.size, lead=lead)
    hsfft.filter_batched(typ, dx, n, dh, h.size, block, out, batch)
    hsfft.synchronize()
    y, guard = out.read()
    xin = xbuf.to_array(np.float64, offset_bytes=lead * 8).reshape(x.shape)
    hin = hbuf.to_array(np.float64, offset_bytes=lead * 8)
    for d in (xbuf, hbuf, out):
        d.free()
    compare(y.reshape(want.shape), want, what)
    assert guard == 0, (what, "sentinel words changed", guard)
    _assert_bits(xin, x, (what, "x changed"))
    _assert_bits(hin, h, (what, "h changed"))
    return y.reshape(want.shape)


# the smallest shapes at which each piece can go wrong
SWEEP = [
    (9, 4, 8),             # L = 5: the last block is short and the tail runs past the last block
    (9, 1, 4),             # no overlap at all
    (100, 2, 2),           # L = 1 = m - 1, one hundred blocks, inner c2c of one point
    (1000, 33, 64),        # every sL odd or even in turn
    (8128, 33, 4096),      # n an exact multiple of L
    (8129, 33, 4096),      # and one more
    (40000, 1025, 4096),
    (30000, 200, 16384),   # inner c2c of 8192 points, the whole-row kernel
    (70000, 33, 32768),    # inner c2c of 16384 points, two passes
    (40000, 33, 0),        # the automatic block
    (4, 9, 16),            # a kernel longer than the row: one block, the valid window starts at n - 1
]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n,m,block", SWEEP, ids=["%dx%d@%d" % c for c in SWEEP])
def test_filter(n, m, block, batch):
    """full, same and valid; with batch 3 the rows are dense and all different, so a gather that
    reads into the neighbouring row, or a block scattered into the wrong row, shows"""
    x, h, full = _case(n, m, block)
    assert not np.array_equal(x[0], x[1]) and not np.array_equal(x[1], x[2])
    for typ in F.TYPES:
        want = F.window(full[:batch], typ, n, m)
        olen, P, L, nseg = hsfft.filter_shape(typ, n, m, block)
        assert want.shape == (batch, olen)
        _run(typ, x[:batch], h, block, want, (n, m, block, batch, typ))


def test_more_than_65535_blocks_in_one_call():
    """3 rows of 150000 with 3 taps at P = 8: L = 6, 25000 blocks per row, 75000 in one call and one
    chunk, more than one launch's 65535 rows; the second launch starts inside the last row"""
    n, m, block, batch = 150000, 3, 8, 3
    assert hsfft.filter_shape("full", n, m, block) == (n + m - 1, 8, 6, 25000)
    x, h, full = _case(n, m, block)
    for typ in ("full", "same"):
        _run(typ, x, h, block, F.window(full, typ, n, m), (n, m, block, batch, typ))


def test_filter_in_chunks(monkeypatch):
    """5 rows of 40000 with 33 taps at P = 4096: L = 4064, 10 blocks per row, 50 in all.  Under
    HSFFT_FILTER_CHUNK_MB=1 the documented rule (bytes / (P x 8 + (P/2+1) x 16)) gives 15 blocks
    per chunk: chunks of 15, 15, 15 and 5 that cross row boundaries (block 10 is row 1's first) and
    split overlapping neighbours of one row (blocks 14 | 15, 29 | 30, 44 | 45)"""
    n, m, block, batch, mb = 40000, 33, 4096, 5, 1
    assert hsfft.filter_shape("full", n, m, block)[2:] == (4064, 10)
    per = T.rows_per_chunk(mb, 1, elem=4096 * 8 + 2049 * 16)
    assert per == 15
    x, h, full = _case(n, m, block, batch=batch)
    want = F.window(full, "full", n, m)
    dx, dh = hsfft.DeviceBuffer.from_array(x), hsfft.DeviceBuffer.from_array(h)
    o1, o2 = Out(want.size), Out(want.size)
    monkeypatch.setenv("HSFFT_FILTER_CHUNK_MB", str(mb))
    hsfft.filter_batched("full", dx, n, dh, m, block, o1, batch)
    monkeypatch.delenv("HSFFT_FILTER_CHUNK_MB")
    hsfft.filter_batched("full", dx, n, dh, m, block, o2, batch)
    hsfft.synchronize()
    diff = hsfft.count_diff_words(o1, o2, want.size * 8)
    (y1, g1), (y2, g2) = o1.read(), o2.read()
    for d in (dx, dh, o1, o2):
        d.free()
    assert diff == 0, ("chunked differs from one chunk", diff)
    _assert_bits(y2.reshape(want.shape), want, "one chunk")
    _assert_bits(y1.reshape(want.shape), want, "chunked")
    assert (g1, g2) == (0, 0)


@pytest.mark.parametrize("typ", F.TYPES)
def test_one_block_equals_the_one_shot_path(typ):
    """(1000, 33) at block 2048 = next_power_of_two(1032): one block, and the words are those of
    hsfft_convolve_batched on the same rows with the kernel replicated per row"""
    n, m, block, batch = 1000, 33, 2048, 3
    assert hsfft.filter_shape(typ, n, m, block)[1:] == (2048, 2016, 1)
    x, h = F.rows(n, batch, salt=0xF6), F.kernel(m, salt=0xF6)
    want = np.stack([T.oracle_convolve(typ.encode(), b"linear", r, h) for r in x])
    y = _run(typ, x, h, block, want, ("one block", typ))
    dx, dh = hsfft.DeviceBuffer.from_array(x), hsfft.DeviceBuffer.from_array(np.tile(h, (batch, 1)))
    out = Out(want.size)
    ln = hsfft.lib().hsfft_convolve_batched(typ.encode(), b"linear", dx.ptr, n, dh.ptr, m, out.ptr, batch)
    hsfft.synchronize()
    one, guard = out.read()
    for d in (dx, dh, out):
        d.free()
    assert ln == want.shape[1] and guard == 0
    _assert_bits(y, one.reshape(want.shape), ("against hsfft_convolve_batched", typ))


@pytest.mark.parametrize("n,m,block", [(1000, 33, 64), (9, 4, 8)], ids=["1000x33@64", "9x4@8"])
def test_filter_on_8_byte_aligned_buffers(n, m, block):
    """x, h and the output one double past a 16-byte boundary, with sentinels in front of the output
    as well as behind: caller buffers need the alignment of a double only"""
    x, h, full = _case(n, m, block)
    for typ in F.TYPES:
        _run(typ, x, h, block, F.window(full, typ, n, m), (n, m, block, typ, "lead 1"), lead=1)


def _assert_bits_nan_aware(y, want, what):
    assert T.same_bits_nan_aware(y, want), (what, "NaN words", int(T.nan_words(y).sum()), "expected",
                                            int(T.nan_words(want).sum()))


@pytest.mark.parametrize("typ", ["full", "same"])
def test_special_values(typ):
    """(1000, 33) at P = 64: L = 32, 32 blocks.  Block 10 of row 0 (samples 320..351) holds -0.0,
    subnormals, 1e300, an Inf and a NaN together; block 20 holds the finite kinds once more, where
    no NaN hides them; row 1 is dense.  The words equal the oracle's -- NaN positions compared as
    NaN, where two blocks add too -- and only the words block 10 reaches are not finite"""
    n, m, block = 1000, 33, 64
    x, h = F.rows(n, 2, salt=0xF7).copy(), F.kernel(m, salt=0xF7)
    for base in (320, 640):
        x[0, base + 3] = -0.0
        x[0, base + 4:base + 8] = np.array([5e-324, -3e-310, 1e-308, -2.0 ** -1040])
        x[0, base + 9] = 1e300
        x[0, base + 10] = -1e300
    x[0, 320 + 20] = np.inf
    x[0, 320 + 25] = np.nan
    full = F.oracle_full_rows(x, h, block)
    reach = np.zeros(full.shape, dtype=bool)
    reach[0, 320:320 + 64] = True  # block 10's P words start at 10 L
    assert np.isfinite(full[~reach]).all()  # blocks that are not block 10 stay finite in the oracle
    assert T.nan_words(full[reach]).any() and np.abs(full[0, 640:704]).max() > 1e299
    want = F.window(full, typ, n, m)
    y = _run(typ, x, h, block, want, ("special values", typ), compare=_assert_bits_nan_aware)
    start = F.window_rule(typ, n, m)[0]
    finite = np.isfinite(y)
    assert finite[1].all() and finite[0, :320 - start].all() and finite[0, 384 - start:].all()


def test_back_to_back_calls_share_nothing_live():
    """three calls of different block lengths -- the second grows the scratch, the third runs in the
    front of it -- queued without a wait in between: scratch, the kernel's spectrum and the carry
    are reused in stream order"""
    c1, c2, c3 = (1000, 33, 64), (40000, 1025, 4096), (8129, 33, 4096)
    cases = [(c, "same" if i == 0 else "full") + _case(*c) for i, c in enumerate((c1, c2, c3))]
    wants = [F.window(full, typ, c[0], c[1]) for c, typ, _, _, full in cases]
    bufs = [(hsfft.DeviceBuffer.from_array(x), hsfft.DeviceBuffer.from_array(h)) for _, _, x, h, _ in cases]
    outs = [Out(w.size) for w in wants]
    for (c, typ, _, _, _), (dx, dh), out in zip(cases, bufs, outs):
        hsfft.filter_batched(typ, dx, c[0], dh, c[1], c[2], out, 3)
    hsfft.synchronize()
    got = [o.read() for o in outs]
    for d in [b for pair in bufs for b in pair] + outs:
        d.free()
    for (c, typ, _, _, _), w, (y, guard) in zip(cases, wants, got):
        _assert_bits(y.reshape(w.shape), w, (c, typ))
        assert guard == 0, c


def test_rejections_on_the_gpu_path():
    """real device buffers: an output that overlaps either input and a negative batch are refused,
    and batch == 0 returns 0 and writes nothing"""
    n, m, batch = 100, 7, 3
    x, h = F.rows(n, batch, salt=0xF8), F.kernel(m, salt=0xF8)
    dx, dh = hsfft.DeviceBuffer.from_array(x), hsfft.DeviceBuffer.from_array(np.concatenate([h, np.zeros(4096)]))
    out = Out(batch * (n + m - 1))
    L = hsfft.lib()
    for what, o in [("out overlaps x", hsfft.DeviceView(dx, 8 * (n - 1))), ("out == x", dx), ("out == h", dh),
                    ("out overlaps h", hsfft.DeviceView(dh, 8 * (m - 1)))]:
        with pytest.raises(hsfft.HsfftError, match="overlaps"):
            hsfft.filter_batched("valid", dx, n, dh, m, 0, o, batch)
    assert L.hsfft_filter_batched(b"full", dx.ptr, n, dh.ptr, m, 0, out.ptr, -1) == hsfft.HSFFT_ERR_ARG
    assert L.hsfft_last_error()
    assert L.hsfft_filter_batched(b"full", dx.ptr, n, dh.ptr, m, 0, out.ptr, 0) == 0
    hsfft.synchronize()
    y, guard = out.read()
    xin, hin = dx.to_array(np.float64), dh.to_array(np.float64, count=m)
    for d in (dx, dh, out):
        d.free()
    assert T.nan_words(y).all() and guard == 0  # nothing was written
    _assert_bits(xin.reshape(x.shape), x, "x changed")
    _assert_bits(hin, h, "h changed")


def test_oaconvolve_convenience():
    x, h, full = _case(1000, 33, 64)
    y = hsfft.oaconvolve(x[0], h, block=64)
    assert y.shape == (1032,) and y.dtype == np.float64
    _assert_bits(y, full[0], "1-D input")
    y = hsfft.oaconvolve(x, h, mode="same", block=64)
    assert y.shape == (3, 1000)
    _assert_bits(y, F.window(full, "same", 1000, 33), "2-D input")
    x, h, full = _case(40000, 33, 0)
    y = hsfft.oaconvolve(x, h, mode="valid")
    assert y.shape == (3, 40000 - 32)
    _assert_bits(y, F.window(full, "valid", 40000, 33), "automatic block")
