"""GPU: the 2D real transforms hsfft_r2c_2d, hsfft_r2c_2d_full and hsfft_c2r_2d (hsfft_2d.h).

Tolerance: BIT-EXACT, as everywhere in the suite (the one round-trip test says so where it is
not).  Expected values come from hsfft_r2d_testlib alone -- the pinned 1D oracle applied to the
rows and to the n1/2+1 columns, the mirror half by indexing with the sign bit of im flipped
(checked against numpy in test_r2d_cpu.py) -- never from the code under test.  Every output
buffer holds stale data before the call and carries a sentinel tail of 64 x max(n0, n1) elements
beyond its exact size that must come back unchanged (the pitched and mirrored stores are where an
edge guard can go wrong), and every input is read back unchanged.
"""
import numpy as np
import pytest

import hsfft_2d_testlib as D
import hsfft_r2d_testlib as R
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


def _want_half(n0, n1, batch, s0, s1):
    """real images and their composed-oracle half spectra"""
    def make():
        x = R.real_images(n0, n1, batch)
        return x, R.oracle_r2c_2d(x, s0, s1)
    return _cached(("half", n0, n1, batch, s0, s1), make)


def _want_c2r(n0, n1, batch):
    """the oracle half spectrum (forward plans) of the real images, and its composed-oracle c2r (inverse plans)"""
    def make():
        X = _want_half(n0, n1, batch, 1, 1)[1]
        return X, R.oracle_c2r_2d(X, n1, -1, -1)
    return _cached(("c2r", n0, n1, batch), make)


class Out:
    """an output buffer of `count` elements of `esize` bytes filled with stale words, plus a
    sentinel tail of `tail` elements; tail_diffs() compares the tail on the device against the
    words the fill put there"""

    def __init__(self, count, esize, tail, seed=0x57A1E):
        self.nbytes, self.tail_bytes, self.seed = count * esize, tail * esize, seed
        self.buf = hsfft.DeviceBuffer(self.nbytes + self.tail_bytes)
        hsfft.fill_real(self.buf, (self.nbytes + self.tail_bytes) // 8, seed)
        self.ptr = self.buf.ptr

    def array(self, dtype):
        return self.buf.to_array(dtype, count=self.nbytes // np.dtype(dtype).itemsize)

    def tail_diffs(self):
        ref = hsfft.DeviceBuffer(self.tail_bytes)
        hsfft.fill_real(ref, self.tail_bytes // 8, self.seed, offset=self.nbytes // 8)
        diff = hsfft.count_diff_words(hsfft.DeviceView(self.buf, self.nbytes), ref, self.tail_bytes)
        ref.free()
        return diff

    def free(self):
        self.buf.free()


def _assert_bits(y, want, what):
    bad = T.mismatches(y, want)
    assert bad == 0, (what, "mismatching words", bad, "first at", T.first_diff(y, want))


def _plans(n0, n1, s0, s1):
    return hsfft.Plan(n0, s0), hsfft.RealPlan(n1, s1)


def _run_r2c(n0, n1, batch, s0, s1, full, want=None, x=None):
    """one r2c_2d / r2c_2d_full call on fresh buffers, checked against the oracle"""
    if want is None:
        x, want = _want_half(n0, n1, batch, s0, s1)
    if full:
        want = R.complete_full(want, n1)
    p0, r1 = _plans(n0, n1, s0, s1)
    din = hsfft.DeviceBuffer.from_array(x)
    out = Out(want.size, 16, 64 * max(n0, n1))
    (hsfft.r2c_2d_full if full else hsfft.r2c_2d)(p0, r1, din, out, batch)
    hsfft.synchronize()
    y = out.array(np.complex128).reshape(want.shape)
    tail = out.tail_diffs()
    xin = din.to_array(np.float64).reshape(x.shape)
    din.free()
    out.free()
    p0.close()
    r1.close()
    what = ("r2c_2d_full" if full else "r2c_2d", n0, n1, batch, s0, s1)
    _assert_bits(y, want, what)
    assert tail == 0, (what, "sentinel tail words changed", tail)
    _assert_bits(xin, x, (what, "input changed"))


def _run_c2r(n0, n1, batch, X, want, s0=-1, s1=-1):
    p0, r1 = _plans(n0, n1, s0, s1)
    din = hsfft.DeviceBuffer.from_array(X)
    out = Out(want.size, 8, 64 * max(n0, n1))
    hsfft.c2r_2d(p0, r1, din, out, batch)
    hsfft.synchronize()
    y = out.array(np.float64).reshape(want.shape)
    tail = out.tail_diffs()
    xin = din.to_array(np.complex128).reshape(X.shape)
    din.free()
    out.free()
    p0.close()
    r1.close()
    what = ("c2r_2d", n0, n1, batch, s0, s1)
    _assert_bits(y, want, what)
    assert tail == 0, (what, "sentinel tail words changed", tail)
    _assert_bits(xin, X, (what, "input changed"))


SHAPES = [
    (1, 2), (2, 2), (3, 4), (5, 6), (8, 8), (16, 12),  # leaf plans, w = 2..7, no mirror at n1 = 2
    (64, 194), (97, 64),                               # Bluestein on the inner real plan / on the columns
    (100, 60),                                         # mixed radix
    (8, 1798),                                         # inner 899 = 29 x 31, generic odd radix
    (63, 126), (64, 128), (65, 130), (130, 134),       # w and n0 on either side of the 64 tile
    (512, 4096),                                       # multi-tile
    (4, 262144),                                       # inner 2^17: the two-pass path and the fused compact split
    (65536, 4),                                        # two-pass columns, w = 3 transposes
    (12600, 8),                                        # the mr row kernel fed from a transpose
]
CASES = [(n0, n1, 1) for n0, n1 in SHAPES] + [(8, 8, 3), (100, 60, 3), (97, 64, 3), (65, 130, 3)]
CASE_IDS = [f"{a}x{b}-x{c}" for a, b, c in CASES]


@pytest.mark.parametrize("sgn", [1, -1])
@pytest.mark.parametrize("n0,n1,batch", CASES, ids=CASE_IDS)
def test_r2c_2d(n0, n1, batch, sgn):
    _run_r2c(n0, n1, batch, sgn, sgn, full=False)


@pytest.mark.parametrize("sgn", [1, -1])
@pytest.mark.parametrize("n0,n1,batch", CASES, ids=CASE_IDS)
def test_r2c_2d_full(n0, n1, batch, sgn):
    _run_r2c(n0, n1, batch, sgn, sgn, full=True)


@pytest.mark.parametrize("full", [False, True], ids=["half", "full"])
def test_r2c_2d_mixed_signs(full):
    """each plan is applied as planned: the rows with r1's sign, the columns with p0's"""
    _run_r2c(100, 60, 1, -1, 1, full=full)


@pytest.mark.parametrize("n0,n1,batch", CASES, ids=CASE_IDS)
def test_c2r_2d(n0, n1, batch):
    X, want = _want_c2r(n0, n1, batch)
    _run_c2r(n0, n1, batch, X, want)


def test_c2r_2d_of_a_non_hermitian_spectrum():
    """the contract is compositional: dense complex words in every bin, the DC and Nyquist columns
    included, none of the symmetries a real image's spectrum has"""
    n0, n1, batch = 100, 60, 1
    X = D.images(n0, n1 // 2 + 1, batch, salt=0xA5)
    _run_c2r(n0, n1, batch, X, R.oracle_c2r_2d(X, n1, -1, -1))


@pytest.mark.parametrize("n0,n1", [(64, 128), (97, 64)])
def test_round_trip(n0, n1):
    """NOT bit-exact: c2r_2d(r2c_2d(x)) / (n0 n1) returns x to 1e-12 where the reference's
    transforms are true DFTs (powers of two and Bluestein: no D2 twiddle quirk), the bound
    test_c2r_batched_matches_oracle uses for the 1D pair"""
    batch = 2
    x = R.real_images(n0, n1, batch, salt=0x77)
    w = n1 // 2 + 1
    pf, rf = _plans(n0, n1, 1, 1)
    pi, ri = _plans(n0, n1, -1, -1)
    din = hsfft.DeviceBuffer.from_array(x)
    mid = Out(batch * n0 * w, 16, 64 * max(n0, n1))
    out = Out(x.size, 8, 64 * max(n0, n1))
    hsfft.r2c_2d(pf, rf, din, mid, batch)
    hsfft.c2r_2d(pi, ri, mid, out, batch)
    hsfft.synchronize()
    y = out.array(np.float64).reshape(x.shape)
    tails = mid.tail_diffs(), out.tail_diffs()
    din.free()
    mid.free()
    out.free()
    for p in (pf, rf, pi, ri):
        p.close()
    err = float(np.max(np.abs(y / (n0 * n1) - x)))
    print("round trip", n0, n1, "max abs error", err)
    assert err < 1e-12, (n0, n1, err)
    assert tails == (0, 0), tails


# ---------------------------------------------------------------- the other tile size
@pytest.mark.parametrize("n0,n1", [(63, 126), (65, 130), (130, 134)])
def test_r2c_2d_full_tile32(n0, n1, monkeypatch):
    """HSFFT_TR_TILE=32 selects k_transpose_herm<32> (and k_transpose<32>)"""
    monkeypatch.setenv("HSFFT_TR_TILE", "32")
    x = R.real_images(n0, n1, 3, salt=0x32)
    _run_r2c(n0, n1, 3, 1, 1, full=True, want=R.oracle_r2c_2d(x, 1, 1), x=x)


# ---------------------------------------------------------------- the mirrored transpose alone
@pytest.mark.parametrize("tile", ["64", "32"])
@pytest.mark.parametrize("n0,n1", [(1, 2), (1, 4), (3, 4), (63, 126), (64, 128), (65, 130), (130, 134), (200, 62)])
def test_mirrored_transpose_copies_words(n0, n1, tile, monkeypatch):
    """hsfft_bench_transpose_herm runs the kernel alone: random 64-bit patterns (NaN payloads,
    infinities, zeros of either sign) arrive verbatim in columns 0..h and with only the sign bit
    of im flipped in the mirror half, and nothing lands past the end"""
    monkeypatch.setenv("HSFFT_TR_TILE", tile)
    batch, w = 3, n1 // 2 + 1
    words = np.random.default_rng(0x4E4D + 1000 * n0 + n1).integers(0, 1 << 64, size=2 * batch * w * n0, dtype=np.uint64)
    src = words.view(np.complex128).reshape(batch, w, n0)  # transposed half spectra [k1][k0]
    want = R.complete_full(np.ascontiguousarray(src.transpose(0, 2, 1)), n1)
    din = hsfft.DeviceBuffer.from_array(src)
    out = Out(want.size, 16, 64 * max(n0, n1))
    hsfft.bench_transpose_herm(din, out, n0, n1, batch, 1)
    y = out.array(np.complex128).reshape(want.shape)
    tail = out.tail_diffs()
    xin = din.to_array(np.complex128).reshape(src.shape)
    din.free()
    out.free()
    _assert_bits(y, want, ("mirrored transpose", n0, n1, tile))
    assert tail == 0, ("sentinel tail words changed", n0, n1, tile, tail)
    _assert_bits(xin, src, "input changed")


# ---------------------------------------------------------------- chunk loop
def _assert_chunked(per, batch, at_least):
    """stated conditions of the chunk tests: `at_least` chunks or more, the last one ragged"""
    assert 1 <= per < batch and batch % per != 0, (per, batch)
    assert -(-batch // per) >= at_least, (per, batch)


def _chunked_and_not(call, mb, monkeypatch, count, esize, tail):
    """call(out) under HSFFT_2D_CHUNK_MB = mb and with the knob unset, each into its own stale buffer"""
    o1, o2 = Out(count, esize, tail, 0x57A1E), Out(count, esize, tail, 0x57A1F)
    monkeypatch.setenv("HSFFT_2D_CHUNK_MB", str(mb))
    call(o1)
    monkeypatch.delenv("HSFFT_2D_CHUNK_MB")
    call(o2)
    hsfft.synchronize()
    return o1, o2, hsfft.count_diff_words(o1, o2, count * esize)


CHUNK_N0, CHUNK_N1, CHUNK_BATCH = 192, 510, 7  # w = 256: a half spectrum is 192 x 256 x 16 B = 768 KiB


@pytest.mark.parametrize("full", [False, True], ids=["half", "full"])
def test_r2c_2d_in_chunks(full, monkeypatch):
    """7 images of 192 x 510 under HSFFT_2D_CHUNK_MB=2.5: three half spectra per chunk by the
    documented rule (bytes / (copies x n0 x w x 16), one copy), so chunks of 3, 3 and 1"""
    n0, n1, batch, mb = CHUNK_N0, CHUNK_N1, CHUNK_BATCH, 2.5
    w = n1 // 2 + 1
    per = T.rows_per_chunk(mb, n0 * w)
    assert per == 3
    _assert_chunked(per, batch, 3)
    x, want = _want_half(n0, n1, batch, 1, -1)
    if full:
        want = R.complete_full(want, n1)
    p0, r1 = _plans(n0, n1, 1, -1)
    din = hsfft.DeviceBuffer.from_array(x)
    fn = hsfft.r2c_2d_full if full else hsfft.r2c_2d
    o1, o2, diff = _chunked_and_not(lambda out: fn(p0, r1, din, out, batch), mb, monkeypatch, want.size, 16, 64 * n1)
    y1, y2 = (o.array(np.complex128).reshape(want.shape) for o in (o1, o2))
    tails = o1.tail_diffs(), o2.tail_diffs()
    xin = din.to_array(np.float64).reshape(x.shape)
    din.free()
    o1.free()
    o2.free()
    p0.close()
    r1.close()
    assert diff == 0, ("chunked differs from one chunk", diff)
    _assert_bits(y2, want, "one chunk")
    _assert_bits(y1, want, "chunked")
    assert tails == (0, 0), tails
    _assert_bits(xin, x, "input changed")


def test_c2r_2d_in_chunks(monkeypatch):
    """c2r_2d holds two copies of a chunk: 7 half spectra of 768 KiB under HSFFT_2D_CHUNK_MB=4 go
    two per chunk (4 MiB / (2 x 768 KiB)), so chunks of 2, 2, 2 and 1"""
    n0, n1, batch, mb = CHUNK_N0, CHUNK_N1, CHUNK_BATCH, 4
    w = n1 // 2 + 1
    per = T.rows_per_chunk(mb, 2 * n0 * w)
    assert per == 2
    _assert_chunked(per, batch, 3)
    X, want = _want_c2r(n0, n1, batch)
    p0, r1 = _plans(n0, n1, -1, -1)
    din = hsfft.DeviceBuffer.from_array(X)
    o1, o2, diff = _chunked_and_not(lambda out: hsfft.c2r_2d(p0, r1, din, out, batch), mb, monkeypatch, want.size, 8,
                                    64 * n1)
    y1, y2 = (o.array(np.float64).reshape(want.shape) for o in (o1, o2))
    tails = o1.tail_diffs(), o2.tail_diffs()
    xin = din.to_array(np.complex128).reshape(X.shape)
    din.free()
    o1.free()
    o2.free()
    p0.close()
    r1.close()
    assert diff == 0, ("chunked differs from one chunk", diff)
    _assert_bits(y2, want, "one chunk")
    _assert_bits(y1, want, "chunked")
    assert tails == (0, 0), tails
    _assert_bits(xin, X, "input changed")


# ---------------------------------------------------------------- scratch independence
def test_scratch_is_not_shared_with_1d_paths():
    """an r2c_2d call (HS_SCR_2D and, inside its r2c rows, HS_SCR_REAL_Z) followed at once,
    without a wait, by a 1D r2c of n = 65536 (HS_SCR_REAL_Z again) and a c2c of N = 5003
    (Bluestein scratch): the queued work must not see its scratch reused"""
    n0, n1 = 97, 64
    x2, want2 = _want_half(n0, n1, 1, 1, 1)
    p0, r1 = _plans(n0, n1, 1, 1)
    rows = 3
    xr = T.real_input(65536, T.seed_for(65536) ^ 0x2D, batch=rows).reshape(rows, 65536)
    xb = T.complex_input(5003, T.seed_for(5003) ^ 0x2D, batch=rows).reshape(rows, 5003)
    rr, pb = hsfft.RealPlan(65536, 1), hsfft.Plan(5003, 1)
    d2, dr, db = (hsfft.DeviceBuffer.from_array(a) for a in (x2, xr, xb))
    o2 = Out(want2.size, 16, 64 * max(n0, n1))
    orr, ob = Out(rows * 65536, 16, 0, 0x57A20), Out(xb.size, 16, 0, 0x57A21)
    hsfft.r2c_2d(p0, r1, d2, o2, 1)
    hsfft.r2c_batched(rr, dr, orr, rows)
    hsfft.exec_batched(pb, db, ob, rows)
    hsfft.synchronize()
    y2 = o2.array(np.complex128).reshape(want2.shape)
    yr = orr.array(np.complex128).reshape(rows, 65536)
    yb = ob.array(np.complex128).reshape(xb.shape)
    for b in (d2, dr, db, o2, orr, ob):
        b.free()
    for p in (p0, r1, rr, pb):
        p.close()
    _assert_bits(y2, want2, "r2c_2d 97x64")
    _assert_bits(yr, T.oracle_r2c(xr, 1), "r2c_batched 65536")
    _assert_bits(yb, T.oracle_c2c(xb, 1), "exec_batched 5003")


# ---------------------------------------------------------------- special values
def test_special_values():
    """signed zeros, a zero field, an impulse, subnormals and values near overflow (all finite),
    one kind per row, the five kinds repeated down the 64 x 64 real image: r2c_2d_full pins the
    sign of mirrored zeros, c2r_2d runs on the resulting half spectrum"""
    n = 64
    kinds = ("negzero", "zfield", "impulse", "tiny", "huge")
    five = T.special_rows(n, kinds, T.seed_for(n), real=True)
    x = np.ascontiguousarray(np.stack([five[r % len(kinds)] for r in range(n)]).reshape(1, n, n))
    for sgn in (1, -1):
        half = R.oracle_r2c_2d(x, sgn, sgn)
        assert np.isfinite(half.view(np.float64)).all()
        assert T.zero_words(half) > 0  # there are zeros whose sign the mirror must flip
        _run_r2c(n, n, 1, sgn, sgn, full=True, want=half, x=x)
    X = R.oracle_r2c_2d(x, 1, 1)
    want = R.oracle_c2r_2d(X, n, -1, -1)
    assert np.isfinite(want).all() and np.isfinite(X.view(np.float64)).all()
    _run_c2r(n, n, 1, X, want)


# ---------------------------------------------------------------- rfft2 / irfft2
def test_rfft2_irfft2_conveniences():
    x = R.real_images(16, 12, 2, salt=0xF2)
    half = R.oracle_r2c_2d(x, 1, 1)
    y = hsfft.rfft2(x)
    assert y.shape == (2, 16, 7) and y.dtype == np.complex128
    _assert_bits(y, half, "rfft2")
    yf = hsfft.rfft2(x, full=True)
    assert yf.shape == (2, 16, 12)
    _assert_bits(yf, R.complete_full(half, 12), "rfft2 full")
    _assert_bits(hsfft.rfft2(x, sgn=-1), R.oracle_r2c_2d(x, -1, -1), "rfft2 sgn=-1")
    z = hsfft.irfft2(half, 12)
    assert z.shape == x.shape and z.dtype == np.float64
    _assert_bits(z, R.oracle_c2r_2d(half, 12, -1, -1), "irfft2")
    lead = hsfft.rfft2(x.reshape(2, 1, 16, 12))
    assert lead.shape == (2, 1, 16, 7)
    _assert_bits(lead.reshape(half.shape), half, "rfft2 with leading axes")
    lead = hsfft.irfft2(half.reshape(2, 1, 16, 7), 12)
    assert lead.shape == (2, 1, 16, 12)
    _assert_bits(lead.reshape(x.shape), R.oracle_c2r_2d(half, 12, -1, -1), "irfft2 with leading axes")
