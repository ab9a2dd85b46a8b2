"""GPU: the loops that walk a batch in chunks, and the schedules that only knobs reach.

run_chain (hsfft_exec.c) advances its input and output by c0 rows per chunk and alternates two
scratch buffers between the passes of a chain; run_bluestein walks its M-point intermediates
in chunks of its own, around run_chain's; r2c_rows / hs_c2r_rows (hsfft_real.c) advance through
the reference layout (c0*N), the compact layout (c0*(N/2+1)) and the convolution's two compact
spectra.  At the default chunk sizes (256 MiB, 4 GiB, 16 GiB) every other test of the suite is
one chunk, so here the chunk knobs are set small enough that the batch takes several chunks
with a ragged last one -- a condition each test computes from the library's own formula
(hsfft_testlib.rows_per_chunk) and asserts.  The forced schedules come from the shared table
hsfft_testlib.FORCED_PLANS, which test_product_cpu.py pins on the CPU.

Tolerance: BIT-EXACT (0 ulp) against the oracle, as everywhere in the suite.  Every output
buffer holds stale data before the call, every input buffer is read back afterwards and must
be unchanged, and every chunked call is also compared word for word on the device with the same
call in one chunk (knob unset), so a wrong chunk boundary shows as a chunk bug and not as a
kernel bug.  When the batch does not divide into whole chunks the last chunk is ragged; with
one row per chunk there is no ragged chunk to have.
"""
import ctypes

import numpy as np
import pytest

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


def _id(fp):
    return "-".join([str(fp.n)] + [f"{k[6:]}={v}" for k, v in sorted(fp.env.items())])


def _stale_complex(count, seed):
    d = hsfft.DeviceBuffer(count * 16)
    hsfft.fill_complex(d, count, seed)
    return d


def _stale_real(count, seed):
    d = hsfft.DeviceBuffer(count * 8)
    hsfft.fill_real(d, count, seed)
    return d


def _assert_chunked(per, batch):
    """the chunking is a stated condition of the test: several chunks, the last one ragged
    (one row per chunk leaves nothing to be ragged)"""
    assert 1 <= per < batch, (per, batch)
    assert batch % per != 0 or per == 1, (per, batch)


def _free(*bufs):
    for b in bufs:
        b.free()


def _inner_passes(rp):
    """pass count of a real plan's inner N/2-point complex plan (its first member)"""
    return hsfft.check(hsfft.lib().hsfft_plan_num_passes(ctypes.c_void_p.from_address(rp.ptr).value), "num_passes")


def _twice(call, knobs, monkeypatch, make_out, nbytes):
    """call(out) with the chunk knobs set, then with them unset (one chunk), each into its own
    stale buffer: returns the two buffers and the number of 8-byte words in which they differ"""
    d1, d2 = make_out(0x57A1E), make_out(0x57A1F)
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    call(d1)
    for k in knobs:
        monkeypatch.delenv(k)
    call(d2)
    hsfft.synchronize()
    return d1, d2, hsfft.count_diff_words(d1, d2, nbytes)


# ---------------------------------------------------------------- a. c2c chains in chunks
CHUNKED = [(fp, mb, batch) for fp in T.FORCED_PLANS for mb, batch in fp.chunks]


@pytest.mark.parametrize("fp,mb,batch", CHUNKED, ids=[f"{_id(fp)}-{mb}MiB-x{b}" for fp, mb, b in CHUNKED])
def test_c2c_chain_in_chunks(fp, mb, batch, monkeypatch):
    """chains of three and more passes (the intermediates in one or both scratch buffers, the
    last pass in place on the output) over a batch of several chunks: the register-kernel
    chains [r0,8][8,8][8,8], the generic kernel with one power-of-two radix per pass, mixed
    radix lists in three, five and six generic passes.  Both signs."""
    n = fp.n
    assert len(fp.passes) >= 3
    _assert_chunked(T.rows_per_chunk(mb, n), batch)
    for k, v in fp.env.items():
        monkeypatch.setenv(k, v)
    x = T.complex_input(n, T.seed_for(n) ^ 0xC4, batch=batch).reshape(batch, n)
    for sgn in (1, -1):
        p = hsfft.Plan(n, sgn)
        assert p.num_passes() == len(fp.passes)
        din = hsfft.DeviceBuffer.from_array(x)
        d1, d2, diff = _twice(lambda out: hsfft.exec_batched(p, din, out, batch), {"HSFFT_CHUNK_MB": mb}, monkeypatch,
                              lambda seed: _stale_complex(batch * n, seed), x.nbytes)
        y1, y2 = (d.to_array(np.complex128).reshape(batch, n) for d in (d1, d2))
        want = T.oracle_c2c(x, sgn)
        assert diff == 0, ("chunked differs from one chunk", n, sgn, diff)
        assert T.bits_equal(y2, want), ("one chunk", n, sgn, T.mismatches(y2, want))
        assert T.bits_equal(y1, want), ("chunked", n, sgn, T.mismatches(y1, want))
        assert T.bits_equal(din.to_array(np.complex128).reshape(batch, n), x), ("input changed", n, sgn)
        _free(din, d1, d2)
        p.close()


# ---------------------------------------------------------------- b. forced schedules, one chunk
UNCHUNKED = [fp for fp in T.FORCED_PLANS if not fp.chunks]


@pytest.mark.parametrize("fp", UNCHUNKED, ids=[_id(fp) for fp in UNCHUNKED])
def test_forced_schedule(fp, monkeypatch):
    """the remaining forced schedules -- the G1 = 4 first-pass tile, the G2 = 4 / 16 last-pass
    tiles (with HSFFT_PF=0 the register kernel that has those tiles, without it the pipelined
    kernel that overrides them), the two-pass schedules of 4096 and 8192, five generic radix-8
    passes -- 3 rows, both signs"""
    n, rows = fp.n, 3
    for k, v in fp.env.items():
        monkeypatch.setenv(k, v)
    x = T.complex_input(n, T.seed_for(n) ^ 0xF5, batch=rows).reshape(rows, n)
    for sgn in (1, -1):
        p = hsfft.Plan(n, sgn)
        assert p.num_passes() == len(fp.passes)
        din = hsfft.DeviceBuffer.from_array(x)
        dout = _stale_complex(rows * n, 0x57A1E)
        hsfft.exec_batched(p, din, dout, rows)
        hsfft.synchronize()
        y = dout.to_array(np.complex128).reshape(rows, n)
        want = T.oracle_c2c(x, sgn)
        assert T.bits_equal(y, want), (n, sgn, fp.env, T.mismatches(y, want))
        assert T.bits_equal(din.to_array(np.complex128).reshape(rows, n), x), ("input changed", n, sgn)
        _free(din, dout)
        p.close()


# ---------------------------------------------------------------- c. Bluestein in chunks
BLUE = [(fp, bmb, cmb, batch) for fp in T.BLUESTEIN_PLANS for bmb, cmb, batch in fp.chunks]


@pytest.mark.parametrize("fp,blue_mb,chain_mb,batch", BLUE, ids=[f"{fp.n}-x{b}" for fp, _, _, b in BLUE])
def test_bluestein_in_chunks(fp, blue_mb, chain_mb, batch, monkeypatch):
    """run_bluestein's chunk loop.  M = 2^14 (N = 5003) and 2^17 (N = 40009): two chains per
    outer chunk; the inverse chain stores through the chirp, cannot end in place and takes
    scratch, so HSFFT_CHUNK_MB splits every outer chunk again.  M = 2^18 (N = 99991) with
    HSFFT_BLUE_XCD=0: the three launches per chunk over both M-point intermediates.  Both signs."""
    n, M = fp.n, T.BLUESTEIN_M[fp.n]
    per = T.rows_per_chunk(blue_mb, M)
    _assert_chunked(per, batch)
    knobs = {"HSFFT_BLUE_CHUNK_MB": blue_mb}
    if chain_mb is None:
        assert M == 1 << 18
        monkeypatch.setenv("HSFFT_BLUE_XCD", "0")  # not the persistent launch: the three-launch path
    else:
        inner = T.rows_per_chunk(chain_mb, M)
        assert 1 <= inner < per, (inner, per)  # the inverse chain splits a full outer chunk again
        knobs["HSFFT_CHUNK_MB"] = chain_mb
    x = T.complex_input(n, T.seed_for(n) ^ 0xB1, batch=batch).reshape(batch, n)
    for sgn in (1, -1):
        p = hsfft.Plan(n, sgn)
        assert p.header()["lt"] == 1 and p.num_passes() == len(fp.passes)
        din = hsfft.DeviceBuffer.from_array(x)
        d1, d2, diff = _twice(lambda out: hsfft.exec_batched(p, din, out, batch), knobs, monkeypatch,
                              lambda seed: _stale_complex(batch * n, seed), x.nbytes)
        y1, y2 = (d.to_array(np.complex128).reshape(batch, n) for d in (d1, d2))
        want = T.oracle_c2c(x, sgn)
        assert diff == 0, ("chunked differs from one chunk", n, sgn, diff)
        assert T.bits_equal(y2, want), ("one chunk", n, sgn, T.mismatches(y2, want))
        assert T.bits_equal(y1, want), ("chunked", n, sgn, T.mismatches(y1, want))
        assert T.bits_equal(din.to_array(np.complex128).reshape(batch, n), x), ("input changed", n, sgn)
        _free(din, d1, d2)
        p.close()


# ---------------------------------------------------------------- d. real paths in chunks
@pytest.mark.parametrize("n,batch", [(32768, 11), (131072, 3)])
def test_real_in_chunks(n, batch, monkeypatch):
    """HSFFT_REAL_CHUNK_MB=1: r2c in the reference layout (rows c0*N) and the compact layout
    (rows c0*(N/2+1)), both plan signs, and c2r, four rows per chunk (N = 32768) and one
    (N = 131072)"""
    h = n // 2
    _assert_chunked(T.rows_per_chunk(1, h), batch)
    knobs = {"HSFFT_REAL_CHUNK_MB": 1}
    x = T.real_input(n, T.seed_for(n) ^ 0xD4, batch=batch).reshape(batch, n)
    din = hsfft.DeviceBuffer.from_array(x)
    for sgn in (1, -1):
        rp = hsfft.RealPlan(n, sgn)
        want = T.oracle_r2c(x, sgn)
        for compact, cols in ((0, n), (1, h + 1)):
            fn = hsfft.r2c_batched_compact if compact else hsfft.r2c_batched
            d1, d2, diff = _twice(lambda out: fn(rp, din, out, batch), knobs, monkeypatch,
                                  lambda seed: _stale_complex(batch * cols, seed), batch * cols * 16)
            y1, y2 = (d.to_array(np.complex128).reshape(batch, cols) for d in (d1, d2))
            w = np.ascontiguousarray(want[:, :cols])
            assert diff == 0, ("r2c chunked differs from one chunk", n, sgn, compact, diff)
            assert T.bits_equal(y2, w), ("r2c one chunk", n, sgn, compact, T.mismatches(y2, w))
            assert T.bits_equal(y1, w), ("r2c chunked", n, sgn, compact, T.mismatches(y1, w))
            _free(d1, d2)
        rp.close()
    assert T.bits_equal(din.to_array(np.float64).reshape(batch, n), x), ("r2c input changed", n)
    X = T.oracle_r2c(x, 1)
    dX = hsfft.DeviceBuffer.from_array(X)
    ip = hsfft.RealPlan(n, -1)
    d1, d2, diff = _twice(lambda out: hsfft.c2r_batched(ip, dX, out, batch), knobs, monkeypatch,
                          lambda seed: _stale_real(batch * n, seed), batch * n * 8)
    y1, y2 = (d.to_array(np.float64).reshape(batch, n) for d in (d1, d2))
    want = np.stack([T.oracle_c2r(X[b], n, -1) for b in range(batch)])
    assert diff == 0, ("c2r chunked differs from one chunk", n, diff)
    assert T.bits_equal(y2, want), ("c2r one chunk", n, T.mismatches(y2, want))
    assert T.bits_equal(y1, want), ("c2r chunked", n, T.mismatches(y1, want))
    assert T.bits_equal(dX.to_array(np.complex128).reshape(batch, n), X), ("c2r input changed", n)
    assert np.max(np.abs(y1 / n - x)) < 1e-12  # powers of two: no D2 twiddle quirk
    _free(din, dX, d1, d2)
    ip.close()


@pytest.mark.parametrize("typ", [b"full", b"valid"])
def test_convolve_in_chunks(typ, monkeypatch):
    """hsfft_convolve_batched with HSFFT_REAL_CHUNK_MB=1: n = 5000, m = 300 gives P = 8192
    (inner length 4096, 16 rows per chunk), 37 rows in chunks of 16, 16 and 5 -- two compact r2c
    and hs_c2r_rows over the two compact spectra (d_a + c0*xdist, d_b + c0*xdist)"""
    L, lib = hsfft.lib(), T.oracle()
    n, m, rows = 5000, 300, 37
    P = L.next_power_of_two(n + m - 1)
    assert P == 8192
    _assert_chunked(T.rows_per_chunk(1, P // 2), rows)
    a = T.real_input(n, 0xC0A, batch=rows).reshape(rows, n)
    b = T.real_input(m, 0xC0B, batch=rows).reshape(rows, m)
    da, db = hsfft.DeviceBuffer.from_array(a), hsfft.DeviceBuffer.from_array(b)
    ln = n + m - 1 if typ == b"full" else n - m + 1

    def call(out):
        assert L.hsfft_convolve_batched(typ, b"linear", da.ptr, n, db.ptr, m, out.ptr, rows) == ln, L.hsfft_last_error()

    d1, d2, diff = _twice(call, {"HSFFT_REAL_CHUNK_MB": 1}, monkeypatch, lambda seed: _stale_real(rows * ln, seed),
                          rows * ln * 8)
    y1, y2 = (d.to_array(np.float64).reshape(rows, ln) for d in (d1, d2))
    want = np.empty((rows, ln))
    for r in range(rows):
        o = np.zeros(2 * (n + m) + 8)
        assert lib.orc_convolve(typ, b"linear", T.ptr(np.ascontiguousarray(a[r])), n,
                                T.ptr(np.ascontiguousarray(b[r])), m, T.ptr(o), 0) == ln
        want[r] = o[:ln]
    assert diff == 0, ("chunked differs from one chunk", typ, diff)
    assert T.bits_equal(y2, want), ("one chunk", typ, T.mismatches(y2, want))
    assert T.bits_equal(y1, want), ("chunked", typ, T.mismatches(y1, want))
    assert T.bits_equal(da.to_array(np.float64).reshape(rows, n), a), ("input a changed", typ)
    assert T.bits_equal(db.to_array(np.float64).reshape(rows, m), b), ("input b changed", typ)
    _free(da, db, d1, d2)


# ---------------------------------------------------------------- e. short split walks
@pytest.mark.parametrize("wt", [None, "1"])
@pytest.mark.parametrize("n,whole", [(16384, "0"), (32768, None), (65536, None)])
def test_r2c_short_walks_all_rotation_classes(n, whole, wt, monkeypatch):
    """pf::k_r2c_walk1 starts row b at rotation class b % 8 of its walk: 11 rows meet classes
    0..7 and the wrap, at the lengths whose walk is shorter than 8 tiles -- last pass
    B = 16 (N = 2^14 under HSFFT_WHOLE=0), 32 (2^15) and 64 (2^16) -- with the default walk
    length and with walks of one tile (HSFFT_R2C_WT=1).  Reference layout, both plan signs."""
    if whole is not None:
        monkeypatch.setenv("HSFFT_WHOLE", whole)
    if wt is not None:
        monkeypatch.setenv("HSFFT_R2C_WT", wt)
    batch = 11
    x = T.real_input(n, T.seed_for(n) ^ 0xE5, batch=batch).reshape(batch, n)
    din = hsfft.DeviceBuffer.from_array(x)
    for sgn in (1, -1):
        rp = hsfft.RealPlan(n, sgn)
        assert _inner_passes(rp) == 2  # [..][8,8,8] with B = n / 1024: the fused split walk
        dout = _stale_complex(batch * n, 0x57A1E)
        hsfft.r2c_batched(rp, din, dout, batch)
        hsfft.synchronize()
        y = dout.to_array(np.complex128).reshape(batch, n)
        want = T.oracle_r2c(x, sgn)
        bad = [b for b in range(batch) if not T.bits_equal(y[b], want[b])]
        assert not bad, (n, sgn, wt, "rows", bad, T.mismatches(y, want))
        _free(dout)
        rp.close()
    assert T.bits_equal(din.to_array(np.float64).reshape(batch, n), x), ("input changed", n)
    _free(din)


# ---------------------------------------------------------------- f. c2r across inner schedules
C2R_CASES = [
    # N, knobs, passes of the inner N/2-point plan (None: Bluestein, its M-point passes)
    (8192, {}, 1),                       # inner 4096: one whole-row radix-8 pass
    (16384, {}, 1),                      # inner 8192: one whole-row pass [2,8,8,8,8]
    (16384, {"HSFFT_WHOLE": "0"}, 2),    # inner 8192 as [2,8][8,8,8]
    (25200, {}, 1),                      # inner 12600: the row kernel
    (25200, {"HSFFT_MR_ROW": "0"}, 2),   # inner 12600 as two mixed-radix passes
    (6000, {}, 1),                       # inner 3000: one whole generic pass
    (20000, {}, 2),                      # inner 10000: two mixed passes
    (10006, {}, 2),                      # inner 5003: Bluestein, M = 16384
]


@pytest.mark.parametrize("n,env,inner", C2R_CASES, ids=[f"{n}" + "".join(f"-{k[6:]}={v}" for k, v in e.items())
                                                        for n, e, _ in C2R_CASES])
def test_c2r_inner_schedule_classes(n, env, inner, monkeypatch):
    """c2r (pre-twiddle + the inverse N/2-point c2c) with the inner transform in every schedule
    class: whole-row passes, their two-pass forms, the 12600 row kernel, a whole generic pass,
    two mixed passes and a small Bluestein length; 3 rows from the oracle's r2c.  Powers of two
    (no D2 twiddle quirk) also return N * x to 1e-12."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rows = 3
    x = T.real_input(n, T.seed_for(n) ^ 0xF6, batch=rows).reshape(rows, n)
    X = T.oracle_r2c(x, 1)
    rp = hsfft.RealPlan(n, -1)
    assert _inner_passes(rp) == inner
    dX = hsfft.DeviceBuffer.from_array(X)
    dout = _stale_real(rows * n, 0x57A1E)
    hsfft.c2r_batched(rp, dX, dout, rows)
    hsfft.synchronize()
    y = dout.to_array(np.float64).reshape(rows, n)
    want = np.stack([T.oracle_c2r(X[b], n, -1) for b in range(rows)])
    assert T.bits_equal(y, want), (n, env, T.mismatches(y, want))
    assert T.bits_equal(dX.to_array(np.complex128).reshape(rows, n), X), ("input changed", n)
    if n & (n - 1) == 0:
        assert np.max(np.abs(y / n - x)) < 1e-12
    _free(dX, dout)
    rp.close()
