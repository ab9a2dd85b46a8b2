"""GPU: the batched 2D convolution hsfft_convolve_2d_batched (hsfft_conv2d.h).

Tolerance: BIT-EXACT, as everywhere in the suite.  Expected values come from
hsfft_conv2d_testlib alone -- zero padding, the composed 2D oracle of hsfft_r2d_testlib, the
spectral product with one rounding per numpy operation, one division and the restated window rule
(pinned to the reference's fft_convolve and checked against a direct sum in test_conv2d_cpu.py) --
never from the code under test.  Every output buffer holds stale data before the call and carries
a sentinel tail of 64 x max(out_rows, out_cols) elements beyond its exact size that must come
back unchanged, and both inputs are read back unchanged.
"""
import numpy as np
import pytest

import hsfft_conv2d_testlib as C
import hsfft_testlib as T

import hsfft

pytestmark = pytest.mark.gpu


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


def _operands(ash, bsh, batch, b_batch):
    def make():
        return C.images(*ash, batch, salt=0xC2), C.images(*bsh, b_batch, salt=0xD2)
    return _cached(("in", ash, bsh, batch, b_batch), make)


def _padded(ash, bsh, batch, b_batch, ct):
    """(a, b, the unwindowed expectation): one oracle run per operands and padded size serves
    every window, and linear and circular too where they pad alike"""
    a, b = _operands(ash, bsh, batch, b_batch)
    P0, P1 = C.shape_rule("full", ct, *ash, *bsh)[2:]
    return a, b, _cached(("y", ash, bsh, batch, b_batch, P0, P1), lambda: C.oracle_padded(a, b, P0, P1))


class Out:
    """an output buffer of `count` doubles filled with stale words, plus a sentinel tail of `tail`
    doubles behind it and `lead` doubles in front (an odd lead makes the output only 8-byte
    aligned); tail_diffs() compares the sentinels on the device against the words the fill put there"""

    def __init__(self, count, tail, seed=0x57A1E, lead=0):
        self.lead_bytes, self.nbytes, self.tail_bytes, self.seed = lead * 8, count * 8, tail * 8, seed
        self.buf = hsfft.DeviceBuffer(self.lead_bytes + self.nbytes + self.tail_bytes)
        hsfft.fill_real(self.buf, self.buf.nbytes // 8, seed)
        self.ptr = self.buf.ptr + self.lead_bytes

    def array(self):
        return self.buf.to_array(np.float64, count=self.nbytes // 8, offset_bytes=self.lead_bytes)

    def tail_diffs(self):
        diff = 0
        for off, nbytes in ((0, self.lead_bytes), (self.lead_bytes + self.nbytes, self.tail_bytes)):
            if nbytes:
                ref = hsfft.DeviceBuffer(nbytes)
                hsfft.fill_real(ref, nbytes // 8, self.seed, offset=off // 8)
                diff += hsfft.count_diff_words(hsfft.DeviceView(self.buf, off), ref, nbytes)
                ref.free()
        return diff

    def free(self):
        self.buf.free()


def _assert_bits(y, want, what):
    bad = T.mismatches(y, want)
    assert bad == 0, (what, "mismatching words", bad, "first at", T.first_diff(y, want))


def _upload(x, lead):
    """x on the device behind `lead` doubles: (owning buffer, the view that starts at x)"""
    buf = hsfft.DeviceBuffer(lead * 8 + x.nbytes)
    view = hsfft.DeviceView(buf, lead * 8)
    hsfft.check(hsfft.lib().hsfft_memcpy_h2d(view.ptr, x.ctypes.data, x.nbytes), "h2d")
    return buf, view


def _run(typ, ct, a, b, want, what, lead=0):
    """one call on fresh buffers, checked against `want`; lead: doubles in front of every buffer"""
    batch, b_batch = a.shape[0], b.shape[0]
    (abuf, da), (bbuf, db) = _upload(a, lead), _upload(b, lead)
    out = Out(want.size, 64 * max(want.shape[1:]), lead=lead)
    hsfft.convolve_2d_batched(typ, ct, da, a.shape[1], a.shape[2], db, b.shape[1], b.shape[2], b_batch, out, batch)
    hsfft.synchronize()
    y = out.array().reshape(want.shape)
    tail = out.tail_diffs()
    ain = abuf.to_array(np.float64, offset_bytes=lead * 8).reshape(a.shape)
    bin_ = bbuf.to_array(np.float64, offset_bytes=lead * 8).reshape(b.shape)
    for d in (abuf, bbuf, out):
        d.free()
    _assert_bits(y, want, what)
    assert tail == 0, (what, "sentinel words changed", tail)
    _assert_bits(ain, a, (what, "a changed"))
    _assert_bits(bin_, b, (what, "b changed"))


SHAPES = [
    ((2, 1), (1, 2)),        # P0 = 2, P1 = 2, w = 2
    ((1, 5), (1, 3)),        # P0 = 1: the column transforms are copies; also against the 1D oracle
    ((5, 7), (3, 2)),        # odd widths: source rows of the padding and output rows only 8-byte aligned
    ((3, 9), (8, 2)),        # each operand the larger on one axis
    ((40, 70), (30, 60)),    # P = 128 x 256, w = 129: transpose tiles on both sides of 64
    ((33, 33), (32, 32)),    # P = 64 x 64, w = 33
]
BATCHES = [(1, 1), (3, 3), (3, 1)]  # (batch, b_batch)


@pytest.mark.parametrize("ct", C.CONV_TYPES)
@pytest.mark.parametrize("batch,b_batch", BATCHES, ids=["x1", "x3", "x3-shared"])
@pytest.mark.parametrize("ash,bsh", SHAPES, ids=[f"{a[0]}x{a[1]}*{b[0]}x{b[1]}" for a, b in SHAPES])
def test_convolve_2d(ash, bsh, batch, b_batch, ct):
    """full, same and valid (under circular the type is checked and not used: the whole padded image)"""
    a, b, y = _padded(ash, bsh, batch, b_batch, ct)
    for typ in C.TYPES:
        want = C.window(y, typ, ct, ash, bsh)
        assert want.shape[1:] == hsfft.convolve_2d_shape(typ, ct, *ash, *bsh)[:2]
        if ash[0] == 1 and bsh[0] == 1:  # the yardstick's pin, once more on the shapes used here
            for i in range(batch):
                one = T.oracle_convolve(typ.encode(), ct.encode(), a[i, 0], b[i % b_batch, 0])
                _assert_bits(want[i, 0], one, ("1D oracle", typ, ct, i))
        _run(typ, ct, a, b, want, (ash, bsh, batch, b_batch, typ, ct))


@pytest.mark.parametrize("ct", C.CONV_TYPES)
def test_convolve_2d_wide_rows(ct):
    """2 x 200000 with 1 x 60000: P1 = 2^18, so the inner real transform takes the two-pass path
    with the fused compact split, and the c2r reads rows at pitch w = 2^17 + 1.  One pair: the
    oracle runs six rows of 2^18 (linear and circular pad alike and share them)"""
    ash, bsh = (2, 200000), (1, 60000)
    assert C.shape_rule("full", ct, *ash, *bsh)[2:] == (2, 1 << 18)
    a, b, y = _padded(ash, bsh, 1, 1, ct)
    for typ in C.TYPES if ct == "linear" else ("full",):
        _run(typ, ct, a, b, C.window(y, typ, ct, ash, bsh), (ash, bsh, typ, ct))


@pytest.mark.parametrize("ash,bsh", [((5, 7), (3, 2)), ((5, 8), (3, 3)), ((40, 70), (30, 60))],
                         ids=["5x7*3x2", "5x8*3x3", "40x70*30x60"])
def test_convolve_2d_on_8_byte_aligned_buffers(ash, bsh):
    """both inputs and the output one double past a 16-byte boundary, with sentinels in front of the
    output as well as behind: caller buffers need the alignment of a double only (odd and even
    widths on either side)"""
    a, b, y = _padded(ash, bsh, 3, 3, "linear")
    for typ in C.TYPES:
        _run(typ, "linear", a, b, C.window(y, typ, "linear", ash, bsh), (ash, bsh, typ, "lead 1"), lead=1)


# ---------------------------------------------------------------- chunk loop
def _assert_chunked(per, batch, at_least):
    """stated conditions of the chunk test: `at_least` chunks or more, the last one ragged"""
    assert 1 <= per < batch and batch % per != 0, (per, batch)
    assert -(-batch // per) >= at_least, (per, batch)


@pytest.mark.parametrize("b_batch", [7, 1], ids=["per-image", "shared"])
def test_convolve_2d_in_chunks(b_batch, monkeypatch):
    """7 pairs of 100 x 200 with 29 x 57: P = 128 x 256, a half spectrum of 128 x 129 x 16 B = 258
    KiB.  Under HSFFT_2D_CHUNK_MB=2 the documented rule (bytes / (3 x P0 x w x 16)) gives two pairs
    per chunk, so chunks of 2, 2, 2 and 1; the shared kernel's extra image is not counted"""
    ash, bsh, batch, mb = (100, 200), (29, 57), 7, 2
    assert C.shape_rule("same", "linear", *ash, *bsh)[2:] == (128, 256)
    per = T.rows_per_chunk(mb, 3 * 128 * 129)
    assert per == 2
    _assert_chunked(per, batch, 3)
    a, b, y = _padded(ash, bsh, batch, b_batch, "linear")
    want = C.window(y, "same", "linear", ash, bsh)
    da, db = hsfft.DeviceBuffer.from_array(a), hsfft.DeviceBuffer.from_array(b)
    o1, o2 = Out(want.size, 64 * 200, 0x57A1E), Out(want.size, 64 * 200, 0x57A1F)

    def call(out):
        hsfft.convolve_2d_batched("same", "linear", da, *ash, db, *bsh, b_batch, out, batch)

    monkeypatch.setenv("HSFFT_2D_CHUNK_MB", str(mb))
    call(o1)
    monkeypatch.delenv("HSFFT_2D_CHUNK_MB")
    call(o2)
    hsfft.synchronize()
    diff = hsfft.count_diff_words(o1, o2, want.size * 8)
    y1, y2 = (o.array().reshape(want.shape) for o in (o1, o2))
    tails = o1.tail_diffs(), o2.tail_diffs()
    ain, bin_ = da.to_array(np.float64).reshape(a.shape), db.to_array(np.float64).reshape(b.shape)
    for d in (da, db, o1, o2):
        d.free()
    assert diff == 0, ("chunked differs from one chunk", diff)
    _assert_bits(y2, want, "one chunk")
    _assert_bits(y1, want, "chunked")
    assert tails == (0, 0), tails
    _assert_bits(ain, a, "a changed")
    _assert_bits(bin_, b, "b changed")


# ---------------------------------------------------------------- scratch and plan cache
def test_back_to_back_calls_share_nothing_live():
    """two calls of different padded sizes (128 x 256, then 64 x 64 in the same, already large
    enough scratch) and a 1D hsfft_convolve_batched queued without a wait in between: scratch and
    cached plans are not reused under queued work"""
    s1, s2 = ((40, 70), (30, 60)), ((33, 33), (32, 32))
    a1, b1, y1 = _padded(*s1, 3, 3, "linear")
    a2, b2, y2 = _padded(*s2, 3, 1, "linear")
    w1, w2 = C.window(y1, "full", "linear", *s1), C.window(y2, "valid", "linear", *s2)
    n, m = 1000, 25
    x = T.real_input(n, T.seed_for(n) ^ 0xC3, batch=3).reshape(3, n)
    k = T.real_input(m, T.seed_for(m) ^ 0xC3, batch=3).reshape(3, m)
    w3 = np.stack([T.oracle_convolve(b"same", b"linear", x[r], k[r]) for r in range(3)])
    bufs = [hsfft.DeviceBuffer.from_array(v) for v in (a1, b1, a2, b2, x, k)]
    o1, o2, o3 = Out(w1.size, 64 * 256, 0x57A20), Out(w2.size, 64 * 64, 0x57A21), Out(w3.size, 0, 0x57A22)
    hsfft.convolve_2d_batched("full", "linear", bufs[0], *s1[0], bufs[1], *s1[1], 3, o1, 3)
    hsfft.convolve_2d_batched("valid", "linear", bufs[2], *s2[0], bufs[3], *s2[1], 1, o2, 3)
    ln = hsfft.lib().hsfft_convolve_batched(b"same", b"linear", bufs[4].ptr, n, bufs[5].ptr, m, o3.ptr, 3)
    hsfft.synchronize()
    got = [o.array().reshape(w.shape) for o, w in ((o1, w1), (o2, w2), (o3, w3))]
    tails = o1.tail_diffs(), o2.tail_diffs()
    for d in bufs + [o1, o2, o3]:
        d.free()
    assert ln == n, (ln, hsfft.lib().hsfft_last_error())
    _assert_bits(got[0], w1, "first call, 128 x 256")
    _assert_bits(got[1], w2, "second call, 64 x 64")
    _assert_bits(got[2], w3, "1D convolution")
    assert tails == (0, 0), tails


# ---------------------------------------------------------------- special values
@pytest.mark.parametrize("typ", ["full", "same"])
def test_special_values(typ):
    """the recipe of test_convolve_special_values in 2D: five images of 12 x 16, one finite kind
    each (zeros of either sign, a zero field, an impulse, subnormals, values near overflow),
    against dense 3 x 4 kernels scaled by 2^-20 so that no product overflows"""
    kinds = ("negzero", "zfield", "impulse", "tiny", "huge")
    rows, cols = 12, 16
    a = np.stack([T.special_rows(cols, (k,) * rows, T.seed_for(cols) + 100 * i, real=True) for i, k in enumerate(kinds)])
    b = C.images(3, 4, len(kinds), salt=0x5C) * 2.0 ** -20
    want = C.oracle_convolve_2d(typ, "linear", a, b)
    assert np.isfinite(want).all()
    assert T.zero_words(want) > 0  # zeros whose sign the kernels must keep
    assert all(np.any(want[i] != 0) for i in (2, 4))  # and the impulse and the huge image are not lost
    _run(typ, "linear", a, b, want, ("special values", typ))


# ---------------------------------------------------------------- convolve2d
def test_convolve2d_convenience():
    a = C.images(5, 7, 6, salt=0xE1).reshape(2, 3, 5, 7)
    k = C.images(3, 2, 1, salt=0xE2)[0]
    want = C.oracle_convolve_2d("full", "linear", a.reshape(6, 5, 7), k.reshape(1, 3, 2))
    y = hsfft.convolve2d(a, k)
    assert y.shape == (2, 3, 7, 8) and y.dtype == np.float64
    _assert_bits(y.reshape(want.shape), want, "shared kernel, leading axes")
    kb = C.images(3, 2, 6, salt=0xE3)
    want = C.oracle_convolve_2d("same", "linear", a.reshape(6, 5, 7), kb)
    y = hsfft.convolve2d(a, kb.reshape(2, 3, 3, 2), mode="same")
    assert y.shape == (2, 3, 5, 7)
    _assert_bits(y.reshape(want.shape), want, "one kernel per image")
    y = hsfft.convolve2d(a[0, 0], k, mode="valid")
    assert y.shape == (3, 6)
    _assert_bits(y, C.oracle_convolve_2d("valid", "linear", a[0, :1], k.reshape(1, 3, 2))[0], "a single image")
    y = hsfft.convolve2d(a, k, boundary="circular")
    assert y.shape == (2, 3, 8, 8)
    _assert_bits(y.reshape(6, 8, 8), C.oracle_convolve_2d("full", "circular", a.reshape(6, 5, 7), k.reshape(1, 3, 2)),
                 "circular")
