"""GPU: the batched transpose, the 2D transform and the column transform (hsfft_2d.h).

Tolerance: BIT-EXACT, as everywhere in the suite.  A transpose is a pure copy, so its output
must carry every 64-bit word of the input (random bit patterns here: NaN payloads, infinities
and subnormals included), and hsfft_exec_2d / hsfft_exec_columns must equal, word for word, the
1D oracle applied to every row and then to every column (hsfft_2d_testlib, checked against
numpy in test_2d_cpu.py).  Expected values never come from the code under test.  Every output
buffer holds stale data before the call and every input is read back unchanged.
"""
import numpy as np
import pytest

import hsfft_2d_testlib as D
import hsfft_testlib as T

import hsfft

pytestmark = pytest.mark.gpu

TILE = 64  # default tile of tr2d::k_transpose (HSFFT_TR_TILE=32 selects the other)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if hsfft.device_count() < 1:
        pytest.skip("no GPU")
    hsfft.lib().hsfft_set_device(0)
    yield
    hsfft.synchronize()
    _ORACLE.clear()


_ORACLE = {}


def _want_2d(n0, n1, batch, s0, s1):
    """input and composed-oracle output of one case, computed once per module and read-only"""
    key = (n0, n1, batch, s0, s1)
    if key not in _ORACLE:
        x = D.images(n0, n1, batch)
        y = D.oracle_2d(x, s0, s1)
        x.setflags(write=False)
        y.setflags(write=False)
        _ORACLE[key] = (x, y)
    return _ORACLE[key]


def _stale(count, seed=0x57A1E):
    d = hsfft.DeviceBuffer(count * 16)
    hsfft.fill_complex(d, count, seed)
    return d


def _free(*bufs):
    for b in bufs:
        b.free()


def _assert_bits(y, want, what):
    bad = T.mismatches(y, want)
    assert bad == 0, (what, "mismatching words", bad, "first at", T.first_diff(y, want))


# ---------------------------------------------------------------- transpose
T_SHAPES = [(1, 1), (1, 7), (7, 1), (31, 33), (32, 32), (33, 31), (64, 64), (70, 45), (129, 257), (130, 67)]


def _bit_patterns(count, seed):
    """random 64-bit patterns viewed as complex128: every class of double, NaN payloads included"""
    w = np.random.default_rng(seed).integers(0, 1 << 64, size=2 * count, dtype=np.uint64)
    return w.view(np.complex128)


def _check_transpose(rows, cols, batch):
    n = rows * cols * batch
    tail = TILE * max(rows, cols)  # at least one tile row of either side
    x = _bit_patterns(n, 0x7A5 + rows * 1000 + cols).reshape(batch, rows, cols)
    sentinel = _bit_patterns(n + tail, 0x5E47)
    din, dout = hsfft.DeviceBuffer.from_array(x), hsfft.DeviceBuffer.from_array(sentinel)
    hsfft.transpose_batched(din, dout, rows, cols, batch)
    hsfft.synchronize()
    got = dout.to_array(np.complex128)
    xin = din.to_array(np.complex128)
    _free(din, dout)
    _assert_bits(got[:n].reshape(batch, cols, rows), x.transpose(0, 2, 1), ("transpose", rows, cols, batch))
    _assert_bits(got[n:], sentinel[n:], ("tail written", rows, cols, batch))
    _assert_bits(xin, x.reshape(-1), ("input changed", rows, cols, batch))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("rows,cols", T_SHAPES, ids=[f"{r}x{c}" for r, c in T_SHAPES])
def test_transpose(rows, cols, batch):
    _check_transpose(rows, cols, batch)


@pytest.mark.parametrize("env", [{"HSFFT_TR_TILE": "32"}, {"HSFFT_TR_DIAG": "1"}, {"HSFFT_TR_TILE": "32", "HSFFT_TR_DIAG": "1"}],
                         ids=["tile32", "diagonal", "tile32-diagonal"])
def test_transpose_variants(env, monkeypatch):
    """the other tile size and the rotated tile order (the variants of DESIGN.md §8's table)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for rows, cols in [(1, 7), (63, 65), (64, 64), (70, 45), (129, 257)]:
        _check_transpose(rows, cols, 3)


# ---------------------------------------------------------------- exec_2d
def _run_2d(n0, n1, batch, s0, s1):
    x, want = _want_2d(n0, n1, batch, s0, s1)
    p0 = hsfft.Plan(n0, s0)
    p1 = p0 if (n1, s1) == (n0, s0) else hsfft.Plan(n1, s1)
    din, dout = hsfft.DeviceBuffer.from_array(x), _stale(x.size)
    hsfft.exec_2d(p0, p1, din, dout, batch)
    hsfft.synchronize()
    y = dout.to_array(np.complex128).reshape(x.shape)
    xin = din.to_array(np.complex128).reshape(x.shape)
    _free(din, dout)
    p0.close()
    p1.close()
    _assert_bits(y, want, ("exec_2d", n0, n1, batch, s0, s1))
    _assert_bits(xin, x, ("input changed", n0, n1, batch, s0, s1))


SHAPES_2D = [
    (2, 2), (3, 5), (8, 8), (16, 12),  # leaf-only plans
    (64, 97), (97, 64),                # Bluestein on either axis
    (100, 60),                         # mixed radix
    (29 * 31, 8),                      # generic odd radix
    (512, 4096),                       # whole-row kernels, multi-tile transposes
    (4, 65536), (65536, 4),            # the two-pass pf path on either axis, degenerate-aspect transposes
    (12600, 8),                        # the mr row kernel fed from a transpose
]
CASES_2D = [(n0, n1, 1) for n0, n1 in SHAPES_2D] + [(8, 8, 3), (100, 60, 3), (97, 64, 3)]


@pytest.mark.parametrize("sgn", [1, -1])
@pytest.mark.parametrize("n0,n1,batch", CASES_2D, ids=[f"{a}x{b}-x{c}" for a, b, c in CASES_2D])
def test_exec_2d(n0, n1, batch, sgn):
    _run_2d(n0, n1, batch, sgn, sgn)


@pytest.mark.parametrize("n0,n1,batch,s0,s1", [(100, 60, 3, -1, 1), (97, 64, 1, 1, -1)], ids=["100x60", "97x64"])
def test_exec_2d_mixed_signs(n0, n1, batch, s0, s1):
    """each plan is applied as planned: the rows with p1's sign, the columns with p0's"""
    _run_2d(n0, n1, batch, s0, s1)


# ---------------------------------------------------------------- exec_columns
@pytest.mark.parametrize("n,ncols", [(8, 5), (100, 33), (97, 7), (4096, 40)])
def test_exec_columns(n, ncols):
    batch = 2
    x = D.images(n, ncols, batch, salt=0xC0)
    for sgn in (1, -1):
        want = D.oracle_columns(x, sgn)
        p = hsfft.Plan(n, sgn)
        din, dout = hsfft.DeviceBuffer.from_array(x), _stale(x.size)
        hsfft.exec_columns(p, din, dout, ncols, batch)
        hsfft.synchronize()
        y = dout.to_array(np.complex128).reshape(x.shape)
        xin = din.to_array(np.complex128).reshape(x.shape)
        _free(din, dout)
        p.close()
        _assert_bits(y, want, ("exec_columns", n, ncols, sgn))
        _assert_bits(xin, x, ("input changed", n, ncols, sgn))


# ---------------------------------------------------------------- chunk loop
def _assert_chunked(per, batch, at_least):
    """stated conditions of the chunk tests: `at_least` chunks or more, the last one ragged"""
    assert 1 <= per < batch and batch % per != 0, (per, batch)
    assert -(-batch // per) >= at_least, (per, batch)


def _chunked_and_not(call, mb, monkeypatch, count):
    """call(out) under HSFFT_2D_CHUNK_MB = mb and with the knob unset, each into its own stale buffer"""
    d1, d2 = _stale(count, 0x57A1E), _stale(count, 0x57A1F)
    monkeypatch.setenv("HSFFT_2D_CHUNK_MB", str(mb))
    call(d1)
    monkeypatch.delenv("HSFFT_2D_CHUNK_MB")
    call(d2)
    hsfft.synchronize()
    return d1, d2, hsfft.count_diff_words(d1, d2, count * 16)


def test_exec_2d_in_chunks(monkeypatch):
    """7 images of 256 x 192 (768 KiB each) under HSFFT_2D_CHUNK_MB=2.5: three images per chunk by
    the documented rule (bytes / image bytes, hsfft_gpu.h), so chunks of 3, 3 and 1"""
    n0, n1, batch, mb = 256, 192, 7, 2.5
    per = T.rows_per_chunk(mb, n0 * n1)
    assert per == 3
    _assert_chunked(per, batch, 3)
    x, want = _want_2d(n0, n1, batch, 1, -1)
    p0, p1 = hsfft.Plan(n0, 1), hsfft.Plan(n1, -1)
    din = hsfft.DeviceBuffer.from_array(x)
    d1, d2, diff = _chunked_and_not(lambda out: hsfft.exec_2d(p0, p1, din, out, batch), mb, monkeypatch, x.size)
    y1, y2 = (d.to_array(np.complex128).reshape(x.shape) for d in (d1, d2))
    xin = din.to_array(np.complex128).reshape(x.shape)
    _free(din, d1, d2)
    p0.close()
    p1.close()
    assert diff == 0, ("chunked differs from one chunk", diff)
    _assert_bits(y2, want, "one chunk")
    _assert_bits(y1, want, "chunked")
    _assert_bits(xin, x, "input changed")


def test_exec_columns_in_chunks(monkeypatch):
    """the column path holds two copies of a chunk: 7 matrices of 256 x 192 under
    HSFFT_2D_CHUNK_MB=4 go two per chunk (4 MiB / (2 x 768 KiB)), so chunks of 2, 2, 2 and 1"""
    n, ncols, batch, mb = 256, 192, 7, 4
    per = T.rows_per_chunk(mb, 2 * n * ncols)
    assert per == 2
    _assert_chunked(per, batch, 3)
    x = D.images(n, ncols, batch, salt=0xC1)
    want = D.oracle_columns(x, 1)
    p = hsfft.Plan(n, 1)
    din = hsfft.DeviceBuffer.from_array(x)
    d1, d2, diff = _chunked_and_not(lambda out: hsfft.exec_columns(p, din, out, ncols, batch), mb, monkeypatch, x.size)
    y1, y2 = (d.to_array(np.complex128).reshape(x.shape) for d in (d1, d2))
    xin = din.to_array(np.complex128).reshape(x.shape)
    _free(din, d1, d2)
    p.close()
    assert diff == 0, ("chunked differs from one chunk", diff)
    _assert_bits(y2, want, "one chunk")
    _assert_bits(y1, want, "chunked")
    _assert_bits(xin, x, "input changed")


# ---------------------------------------------------------------- scratch independence
def test_scratch_is_not_shared_with_1d_paths():
    """a 2D call followed at once, without a wait, by 1D calls of N = 5003 (Bluestein: the
    M-point intermediate and, for the chain that stores through the chirp, the chain scratch) and
    N = 65536: the queued 2D work must not see its scratch reused, nor they the 2D call's"""
    x2, want2 = _want_2d(97, 64, 1, 1, 1)
    p0, p1 = hsfft.Plan(97, 1), hsfft.Plan(64, 1)
    rows = 3
    xb, xc = (T.complex_input(n, T.seed_for(n) ^ 0x2D, batch=rows).reshape(rows, n) for n in (5003, 65536))
    pb, pc = hsfft.Plan(5003, 1), hsfft.Plan(65536, 1)
    d2, db, dc = (hsfft.DeviceBuffer.from_array(a) for a in (x2, xb, xc))
    o2, ob, oc = _stale(x2.size), _stale(xb.size, 0x57A20), _stale(xc.size, 0x57A21)
    hsfft.exec_2d(p0, p1, d2, o2, 1)
    hsfft.exec_batched(pb, db, ob, rows)
    hsfft.exec_batched(pc, dc, oc, rows)
    hsfft.synchronize()
    y2 = o2.to_array(np.complex128).reshape(x2.shape)
    yb = ob.to_array(np.complex128).reshape(xb.shape)
    yc = oc.to_array(np.complex128).reshape(xc.shape)
    _free(d2, db, dc, o2, ob, oc)
    for p in (p0, p1, pb, pc):
        p.close()
    _assert_bits(y2, want2, "exec_2d 97x64")
    _assert_bits(yb, T.oracle_c2c(xb, 1), "exec_batched 5003")
    _assert_bits(yc, T.oracle_c2c(xc, 1), "exec_batched 65536")


# ---------------------------------------------------------------- special values
def test_exec_2d_special_values():
    """signed zeros, fields of zeros, impulses, subnormals and values near overflow (all finite),
    one kind per row, the five kinds repeated down the 64 x 64 image"""
    n = 64
    kinds = ("negzero", "zfield", "impulse", "tiny", "huge")
    five = T.special_rows(n, kinds, T.seed_for(n))
    x = np.ascontiguousarray(np.stack([five[r % len(kinds)] for r in range(n)]).reshape(1, n, n))
    for sgn in (1, -1):
        want = D.oracle_2d(x, sgn, sgn)
        assert np.isfinite(want.view(np.float64)).all()
        p = hsfft.Plan(n, sgn)
        din, dout = hsfft.DeviceBuffer.from_array(x), _stale(x.size)
        hsfft.exec_2d(p, p, din, dout, 1)
        hsfft.synchronize()
        y = dout.to_array(np.complex128).reshape(x.shape)
        _free(din, dout)
        p.close()
        _assert_bits(y, want, ("special values", sgn))


# ---------------------------------------------------------------- fft2
def test_fft2_convenience():
    x = D.images(16, 12, 2, salt=0xF2)
    for sgn in (1, -1):
        y = hsfft.fft2(x, sgn)
        assert y.shape == x.shape and y.dtype == np.complex128
        _assert_bits(y, D.oracle_2d(x, sgn, sgn), ("fft2", sgn))
    lead = hsfft.fft2(x.reshape(2, 1, 16, 12))
    assert lead.shape == (2, 1, 16, 12)
    _assert_bits(lead.reshape(x.shape), D.oracle_2d(x, 1, 1), "fft2 with leading axes")
