"""GPU parity: libhsfft on the MI355X against the oracle (CPU restatement pinned to the
reference) and the golden fixtures generated from the reference itself.

Tolerance: BIT-EXACT (0 ulp) for every comparison against the oracle / fixtures -- the GPU
path keeps the reference's twiddle tables, operand order and separate roundings.  The suite's
one comparison against the oracle that is not bitwise is the NaN-class one of the non-finite
inputs (test_gpu_values.py, hsfft_testlib.same_bits_nan_aware): x86 and the GPU give a default
NaN different sign and payload bits, so NaN words must coincide by class and every other word,
signed zeros and infinities included, is bit-equal.  The only other non-bit-exact checks are
against numpy (independent truth), at 4*eps*max|X| for the full-precision radix-2/4/8 sizes and
1e-10 relative where the reference's 11-digit radix-3/5/7 constants limit accuracy.

Reference defects and the policy here: D1 (radix-2 leaf reads its
stale output slot) is NOT reproduced -- D1 sizes compare against the reference's "fixed"
flavour; D2 (twiddle-table quirk) IS reproduced in the default twiddle mode; D3 (radix 13),
D5 (N=2^k+1 Bluestein) and D6 (N=1) compute the correct transform where the reference crashes
or reads out of bounds.
"""
import numpy as np
import pytest

import hsfft_testlib as T

import hsfft

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if hsfft.device_count() < 1:
        pytest.skip("no GPU")
    hsfft.lib().hsfft_set_device(0)
    yield
    hsfft.synchronize()


def gpu_c2c_batched(n, sgn, x):
    """device-resident batched path"""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    batch = x.shape[0] if x.ndim == 2 else 1
    p = hsfft.Plan(n, sgn)
    din = hsfft.DeviceBuffer.from_array(x)
    dout = hsfft.DeviceBuffer(x.nbytes)
    hsfft.exec_batched(p, din, dout, batch)
    hsfft.synchronize()
    y = dout.to_array(np.complex128).reshape(x.shape)
    din.free()
    dout.free()
    p.close()
    return y


def oracle_rows(x, sgn, flags=0):
    return T.oracle_c2c(x, sgn, flags)


# every golden c2c size; D1 sizes are compared against the fixed flavour (oracle flags 0)
C2C_SIZES = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15, 16, 17, 19, 20, 22, 25, 27, 32, 36, 45, 49, 60, 64,
             97, 100, 121, 125, 128, 243, 256, 343, 512, 1021, 1024, 4096, 5003, 12600, 65536]


@pytest.mark.parametrize("whole", ["1", "0"])
@pytest.mark.parametrize("n", [2048, 4096, 8192, 16384])
def test_pow2_whole_row_single_pass(n, whole, monkeypatch):
    """powers of two that fit one workgroup (4096 = [8,8,8,8], 8192 = [2,8,8,8,8]) run as ONE
    pass (one HBM round trip); HSFFT_WHOLE=0 keeps the two-pass schedule.  Bit-exact both ways,
    both signs, ragged batch."""
    monkeypatch.setenv("HSFFT_WHOLE", whole)
    rows = 5
    x = T.complex_input(n, 0x5150 ^ n, batch=rows).reshape(rows, n)
    for sgn in (1, -1):
        p = hsfft.Plan(n, sgn)
        single = n <= 2048 or (whole == "1" and n <= 8192)
        assert p.num_passes() == (1 if single else 2), (n, whole)
        din = hsfft.DeviceBuffer.from_array(x)
        dout = hsfft.DeviceBuffer(x.nbytes)
        hsfft.exec_batched(p, din, dout, rows)
        y = dout.to_array(np.complex128).reshape(rows, n)
        assert T.bits_equal(y, oracle_rows(x, sgn)), (n, sgn, whole)
        din.free()
        dout.free()
        p.close()


@pytest.mark.parametrize("whole", ["1", "0"])
@pytest.mark.parametrize("n", [1000, 2000, 3000, 5000, 5120, 243, 625, 1001, 2 * 3 * 5 * 7 * 8, 11 * 13 * 8, 4913])
def test_mixed_whole_row_single_pass(n, whole, monkeypatch):
    """mixed / odd sizes up to 5120 points: ONE generic LDS pass per row (HSFFT_WHOLE=1,
    default) or passes of <= 512 points; bit-exact both ways, both signs."""
    monkeypatch.setenv("HSFFT_WHOLE", whole)
    rows = 3
    x = T.complex_input(n, 0x3A3A ^ n, batch=rows).reshape(rows, n)
    for sgn in (1, -1):
        p = hsfft.Plan(n, sgn)
        din = hsfft.DeviceBuffer.from_array(x)
        dout = hsfft.DeviceBuffer(x.nbytes)
        hsfft.exec_batched(p, din, dout, rows)
        y = dout.to_array(np.complex128).reshape(rows, n)
        assert T.bits_equal(y, oracle_rows(x, sgn)), (n, sgn, whole, p.num_passes())
        din.free()
        dout.free()
        p.close()


@pytest.mark.parametrize("n", C2C_SIZES)
def test_c2c_dropin_host_pointers_bit_exact(n):
    """fft_exec with host buffers (the reference's own calling convention)."""
    for sgn in (1, -1):
        x = T.complex_input(n, T.seed_for(n))
        y = hsfft.Plan(n, sgn).exec(x)
        assert T.bits_equal(y, oracle_rows(x, sgn)), (n, sgn, T.mismatches(y, oracle_rows(x, sgn)))


def _dropin_call(fn, plan_ptr, x, out_dtype, in_dev, out_dev, alias=False):
    """One drop-in call fn(plan, in, out) with each buffer in host or device memory (alias: one
    buffer for both).  The output buffer holds stale data before the call.  Returns the output
    and the input buffer's content after the call."""
    n = x.size
    xin = x.copy()
    stale = np.full(n, -7.25, dtype=out_dtype)
    bufs = []
    if in_dev:
        bufs.append(hsfft.DeviceBuffer.from_array(xin))
        pin = bufs[-1].ptr
    else:
        pin = xin.ctypes.data
    if alias:
        pout = pin
    elif out_dev:
        bufs.append(hsfft.DeviceBuffer.from_array(stale))
        pout = bufs[-1].ptr
    else:
        pout = stale.ctypes.data
    fn(plan_ptr, hsfft.VP(pin), hsfft.VP(pout))
    after = bufs[0].to_array(x.dtype) if in_dev else xin
    y = after if alias else bufs[-1].to_array(out_dtype) if out_dev else stale
    for b in bufs:
        b.free()
    return y, after


def test_dropin_pointer_combinations():
    """fft_exec, fft_r2c_exec and fft_c2r_exec with every placement of their two buffers -- host /
    host, device / device, device / host, host / device -- and fft_exec with inp == oup in host
    and in device memory (the library stages aliased buffers, so the result is the out-of-place
    one): bit-exact vs the oracle, stale output buffers, inputs left untouched.  fft_exec at
    N = 1024 (one pass: the small path), 65536 (two passes, the last in place) and 97 (Bluestein);
    the real pair at N = 4096 and 2^17."""
    L = hsfft.lib()
    pairs = [(0, 0), (1, 1), (1, 0), (0, 1)]
    for n in (1024, 65536, 97):
        x = T.complex_input(n, T.seed_for(n) ^ 0xD1)
        want = oracle_rows(x, 1)
        p = hsfft.Plan(n, 1)
        for in_dev, out_dev in pairs:
            y, after = _dropin_call(L.fft_exec, p.ptr, x, np.complex128, in_dev, out_dev)
            assert T.bits_equal(y, want), ("fft_exec", n, in_dev, out_dev, T.mismatches(y, want))
            assert T.bits_equal(after, x), ("fft_exec input", n, in_dev, out_dev)
        for dev in (0, 1):
            y, _ = _dropin_call(L.fft_exec, p.ptr, x, np.complex128, dev, dev, alias=True)
            assert T.bits_equal(y, want), ("fft_exec aliased", n, dev, T.mismatches(y, want))
        p.close()
    for n in (4096, 1 << 17):
        x = T.real_input(n, T.seed_for(n) ^ 0xD2)
        X = T.oracle_r2c(x, 1)
        back = T.oracle_c2r(X, n, -1)
        f, iv = hsfft.RealPlan(n, 1), hsfft.RealPlan(n, -1)
        for in_dev, out_dev in pairs:
            y, after = _dropin_call(L.fft_r2c_exec, f.ptr, x, np.complex128, in_dev, out_dev)
            assert T.bits_equal(y, X), ("fft_r2c_exec", n, in_dev, out_dev, T.mismatches(y, X))
            assert T.bits_equal(after, x), ("fft_r2c_exec input", n, in_dev, out_dev)
            y, after = _dropin_call(L.fft_c2r_exec, iv.ptr, X, np.float64, in_dev, out_dev)
            assert T.bits_equal(y, back), ("fft_c2r_exec", n, in_dev, out_dev, T.mismatches(y, back))
            assert T.bits_equal(after, X), ("fft_c2r_exec input", n, in_dev, out_dev)
        f.close()
        iv.close()


@pytest.mark.parametrize("n", C2C_SIZES)
def test_c2c_batched_device_bit_exact(n):
    rows = 3 if n <= 65536 else 1
    for sgn in (1, -1):
        x = T.complex_input(n, T.seed_for(n) ^ 0x77, batch=rows).reshape(rows, n)
        y = gpu_c2c_batched(n, sgn, x)
        assert T.bits_equal(y, oracle_rows(x, sgn)), (n, sgn)


def test_c2c_every_length_2_to_8192():
    """every transform length 2..8192, both signs, 2 device-resident rows each, bit-exact vs
    the oracle: every factorisation the reference planner produces in that range (radix 2..8,
    the generic odd radices 11..53, Bluestein for the larger prime factors) goes through the
    kernel selection (highSpeedFFT.c:1-120 planner, :1735-1907 Bluestein).  The same sweep to
    16384 passed once in 58 s; the suite keeps 8192 for its run time."""
    bad = []
    for n in range(2, 8193):
        x = T.complex_input(n, T.seed_for(n) ^ 0x5151, batch=2).reshape(2, n)
        for sgn in (1, -1):
            y = gpu_c2c_batched(n, sgn, x)
            if not T.bits_equal(y, oracle_rows(x, sgn)):
                bad.append((n, sgn))
    assert not bad, bad[:20]


def test_c2c_exact_twiddle_mode_every_length_2_to_8192():
    """the reference's USE_TWIDDLE_TABLES-off build (every stage twiddle from sincos;
    hsfft_set_twiddle_mode("exact")) for every length 2..8192, alternating signs, 2 rows,
    bit-exact vs the oracle with ORC_TWIDDLE_EXACT."""
    bad = []
    hsfft.set_twiddle_mode("exact")
    try:
        for n in range(2, 8193):
            sgn = 1 if n % 2 else -1
            x = T.complex_input(n, T.seed_for(n) ^ 0x4E4E, batch=2).reshape(2, n)
            y = gpu_c2c_batched(n, sgn, x)
            if not T.bits_equal(y, oracle_rows(x, sgn, flags=1)):
                bad.append((n, sgn))
    finally:
        hsfft.set_twiddle_mode("reference")
    assert not bad, bad[:20]


@pytest.mark.gpu
@pytest.mark.parametrize("flag", ["2", "1", "0"])
def test_c2c_dropin_repeated_calls_completion_word(flag, monkeypatch):
    """back-to-back drop-in fft_exec calls on host buffers whose input changes every call, each
    output checked bit-exact: the host reads the page-locked output slot as soon as the
    completion word arrives (HSFFT_SMALL_FLAG=2: stored by the one-workgroup kernel itself
    after every thread's system-scope release; 1: written by the command processor after the
    kernel; 0: the stream wait) -- a word that overtook the data would show the PREVIOUS
    call's output here.  Lengths whose pass is one workgroup (1024, 4096, 512) and one that is
    not (12600: command-processor word)."""
    monkeypatch.setenv("HSFFT_SMALL_FLAG", flag)
    for n, calls in ((1024, 400), (4096, 150), (512, 300), (12600, 60)):
        p = hsfft.Plan(n, 1)
        xs = [T.complex_input(n, T.seed_for(n) ^ (0x5151 + c)) for c in range(calls)]
        ys = [p.exec(x) for x in xs]
        p.close()
        ref = T.oracle_c2c(np.stack(xs), 1)
        bad = [c for c in range(calls) if not T.bits_equal(ys[c], ref[c])]
        assert not bad, (n, bad[:10])


@pytest.mark.parametrize("concurrent", ["1", "0"])
def test_c2c_dropin_every_length_2_to_4096(concurrent, monkeypatch):
    """the drop-in fft_exec on host buffers (one-pass plans take the page-locked zero-copy
    path -- on this thread's own stream without the device lock by default, under the device
    lock on the library stream with HSFFT_SMALL_CONCURRENT=0 -- the others the staged path)
    for every length 2..4096 (every 7th with the locked path), alternating signs, bit-exact vs
    the oracle (highSpeedFFT.c:1920-1942 fft_exec)."""
    monkeypatch.setenv("HSFFT_SMALL_CONCURRENT", concurrent)
    bad = []
    for n in range(2, 4097, 1 if concurrent == "1" else 7):
        sgn = 1 if n % 2 else -1
        x = T.complex_input(n, T.seed_for(n) ^ 0x6161)
        p = hsfft.Plan(n, sgn)
        y = p.exec(x)
        p.close()
        if not T.bits_equal(y, oracle_rows(x, sgn)):
            bad.append((n, sgn))
    assert not bad, bad[:20]


def test_c2c_matches_reference_fixtures(golden):
    """Golden outputs of the reference itself.  'asis' cases whose factor list ends in 2 are
    D1-affected (their output depends on the caller's buffer) and are covered by the 'fixed'
    flavour, which is compared in exact-twiddle mode."""
    meta, data = golden
    checked = 0
    for key, ent in sorted(meta["cases"].items()):
        if ent.get("kind") != "c2c" or not ent.get("full", False):
            continue
        n, sgn = ent["n"], ent["sgn"]
        if ent["flavour"] == "asis" and ent["plan"]["factors"][-1:] == [2]:
            continue
        hsfft.set_twiddle_mode("exact" if ent["flavour"] == "fixed" else "reference")
        try:
            y = hsfft.Plan(n, sgn).exec(T.complex_input(n, ent["seed"]))
        finally:
            hsfft.set_twiddle_mode("reference")
        assert T.bits_equal(y, data[key]), (key, T.mismatches(y, data[key]))
        checked += 1
    assert checked >= 60


def test_config1_n1024_fixed_flavour(golden):
    """BASELINE config 1 (N=1024, single transform): the reference's radix-2 leaf reads its
    stale output slot (D1); with that neutralised its output is exactly ours."""
    meta, data = golden
    x = T.complex_input(1024, T.SEEDS[1])
    hsfft.set_twiddle_mode("exact")  # 1024 = [8,8,8,2]: exact == reference twiddles here
    try:
        y = hsfft.Plan(1024, 1).exec(x)
    finally:
        hsfft.set_twiddle_mode("reference")
    assert T.bits_equal(y, data["c2c_fixed_1024_p"])
    y2 = hsfft.Plan(1024, 1).exec(x)
    assert T.bits_equal(y2, data["c2c_fixed_1024_p"])
    X = np.fft.fft(x)
    assert np.abs(y - X).max() <= 4 * EPS * np.abs(X).max()


def test_config2_2pow20_rows_and_fixture(golden):
    meta, data = golden
    n = 1 << 20
    x = T.complex_input(n, T.SEEDS[2], batch=2).reshape(2, n)
    y = gpu_c2c_batched(n, 1, x)
    assert T.bits_equal(y, oracle_rows(x, 1))
    key = "c2c_asis_1048576_p"
    assert T.bits_equal(y[0][data[key + "__idx"]], data[key + "__val"])
    assert T.sha256(y[0]) == meta["cases"][key]["sha256"]
    X = np.fft.fft(x[1])
    assert np.abs(y[1] - X).max() <= 4 * EPS * np.abs(X).max()


def test_config3_12600_reference_mode_and_exact_mode(golden):
    meta, data = golden
    n = 12600
    x = T.complex_input(n, T.SEEDS[3], batch=16).reshape(16, n)
    y = gpu_c2c_batched(n, 1, x)
    assert T.bits_equal(y, oracle_rows(x, 1))  # reference mode reproduces the D2 quirk
    assert T.bits_equal(y[0], data["c2c_asis_12600_p"])
    hsfft.set_twiddle_mode("exact")
    try:
        ye = gpu_c2c_batched(n, 1, x)
    finally:
        hsfft.set_twiddle_mode("reference")
    assert T.bits_equal(ye, oracle_rows(x, 1, T.ORC_EXACT))
    assert T.bits_equal(ye[0], data["c2c_fixed_12600_p"])
    X = np.fft.fft(x, axis=1)
    assert np.abs(ye - X).max() / np.abs(X).max() < 1e-10  # 11-digit radix-3/5/7 constants


def test_config4_bluestein_99991(golden):
    meta, data = golden
    n = 99991
    for sgn in (1, -1):
        x = T.complex_input(n, T.SEEDS[4], batch=3).reshape(3, n)
        y = gpu_c2c_batched(n, sgn, x)
        assert T.bits_equal(y, oracle_rows(x, sgn)), sgn
        key = f"c2c_asis_99991_{'p' if sgn == 1 else 'm'}"
        assert T.bits_equal(y[0][data[key + "__idx"]], data[key + "__val"])
        assert T.sha256(y[0]) == meta["cases"][key]["sha256"]
    X = np.fft.fft(x[0])
    y = gpu_c2c_batched(n, 1, x[:1])[0]
    assert np.abs(y - X).max() <= 8 * EPS * np.abs(X).max()


def test_config5_r2c_2pow22(golden):
    meta, data = golden
    n = 1 << 22
    x = T.real_input(n, T.SEEDS[5], batch=2).reshape(2, n)
    rp = hsfft.RealPlan(n, 1)
    din = hsfft.DeviceBuffer.from_array(x)
    dout = hsfft.DeviceBuffer(2 * n * 16)
    hsfft.r2c_batched(rp, din, dout, 2)
    y = dout.to_array(np.complex128).reshape(2, n)
    ref = T.oracle_r2c(x, 1)
    assert T.bits_equal(y, ref)
    key = "r2c_4194304_p"
    assert T.bits_equal(y[0][data[key + "__idx"]], data[key + "__val"])
    assert T.sha256(y[0]) == meta["cases"][key]["sha256"]


def test_real_small_fixtures(golden):
    meta, data = golden
    for key, ent in sorted(meta["cases"].items()):
        if ent.get("kind") == "r2c" and ent["full"]:
            x = T.real_input(ent["n"], ent["seed"])
            y = hsfft.RealPlan(ent["n"], ent["sgn"]).r2c(x)
            assert T.bits_equal(y, data[key]), key
        if ent.get("kind") == "c2r":
            y = hsfft.RealPlan(ent["n"], ent["sgn"]).c2r(data[ent["input_key"]])
            assert T.bits_equal(y, data[key]), key


@pytest.mark.parametrize("n,rows", [(1 << 16, 3), (1 << 22, 2), (2 * 99991, 2), (12600, 5)])
def test_c2r_batched_matches_oracle(n, rows):
    """c2r (ref real.c:150-193) at scale: the inverse pre-twiddle kernel + the sgn=-1 c2c
    (paired-load first pass and k_b512 at 2^22, Bluestein at 2*99991, mixed radix at 12600),
    bit-exact; where the reference's transform is exact (no D2 twiddle quirk) the round trip
    r2c -> c2r also returns N * x to 1e-12"""
    x = T.real_input(n, 11, batch=rows).reshape(rows, n)
    X = T.oracle_r2c(x, 1)
    rp = hsfft.RealPlan(n, -1)
    din = hsfft.DeviceBuffer.from_array(X)
    dout = hsfft.DeviceBuffer(rows * n * 8)
    hsfft.c2r_batched(rp, din, dout, rows)
    y = dout.to_array(np.float64).reshape(rows, n)
    for b in range(rows):
        assert T.bits_equal(y[b], T.oracle_c2r(X[b], n, -1)), b
    if n != 12600:
        assert np.max(np.abs(y / n - x)) < 1e-12


def test_real_every_even_length_2_to_4096():
    """r2c (both plan signs, reference layout and the compact N/2+1-bin extension) and c2r of
    every even length 2..4096, 2 device-resident rows, bit-exact vs the oracle (ref
    real.c:80-193: the N/2-point inner c2c of every factorisation, then the split or the
    pre-twiddle)."""
    bad = []
    for n in range(2, 4097, 2):
        x = T.real_input(n, 0x7A7A ^ n, batch=2).reshape(2, n)
        din = hsfft.DeviceBuffer.from_array(x)
        dout = hsfft.DeviceBuffer(2 * n * 16)
        for sgn in (1, -1):
            rp = hsfft.RealPlan(n, sgn)
            hsfft.r2c_batched(rp, din, dout, 2)
            y = dout.to_array(np.complex128).reshape(2, n)
            want = T.oracle_r2c(x, sgn)
            if not T.bits_equal(y, want):
                bad.append(("r2c", n, sgn))
            h1 = n // 2 + 1  # compact extension: the first N/2+1 bins of the same rows
            hsfft.r2c_batched_compact(rp, din, dout, 2)
            yc = dout.to_array(np.complex128, 2 * h1).reshape(2, h1)
            if not T.bits_equal(yc, np.ascontiguousarray(want[:, :h1])):
                bad.append(("r2c compact", n, sgn))
            rp.close()
        X = T.oracle_r2c(x, 1)
        dX = hsfft.DeviceBuffer.from_array(X)
        dy = hsfft.DeviceBuffer(2 * n * 8)
        rp = hsfft.RealPlan(n, -1)
        hsfft.c2r_batched(rp, dX, dy, 2)
        y = dy.to_array(np.float64).reshape(2, n)
        for b in range(2):
            if not T.bits_equal(y[b], T.oracle_c2r(X[b], n, -1)):
                bad.append(("c2r", n, b))
        rp.close()
        for buf in (din, dout, dX, dy):
            buf.free()
    assert not bad, bad[:20]


def test_convolve_fixtures(golden):
    meta, data = golden
    L = hsfft.lib()
    for key, ent in sorted(meta["cases"].items()):
        if ent.get("kind") != "conv":
            continue
        a = T.real_input(ent["n"], ent["seed_a"])
        b = T.real_input(ent["m"], ent["seed_b"])
        o = np.zeros(4 * (ent["n"] + ent["m"]))
        ln = L.fft_convolve(ent["type"].encode(), ent["conv_type"].encode(), T.ptr(a), ent["n"], T.ptr(b), ent["m"],
                            T.ptr(o))
        assert ln == ent["len"], key
        assert T.bits_equal(o[:ln], data[key]), key


def test_convolve_batched_matches_oracle():
    L = hsfft.lib()
    n, m, rows = 300, 17, 4
    a = T.real_input(n, 5, batch=rows).reshape(rows, n)
    b = T.real_input(m, 6, batch=rows).reshape(rows, m)
    da, db = hsfft.DeviceBuffer.from_array(a), hsfft.DeviceBuffer.from_array(b)
    for typ in (b"full", b"same", b"valid"):
        dout = hsfft.DeviceBuffer(rows * (n + m) * 8)
        ln = L.hsfft_convolve_batched(typ, b"linear", da.ptr, n, db.ptr, m, dout.ptr, rows)
        assert ln > 0
        y = dout.to_array(np.float64, rows * ln).reshape(rows, ln)
        lib = T.oracle()
        for r in range(rows):
            o = np.zeros(2 * (n + m))
            assert lib.orc_convolve(typ, b"linear", T.ptr(np.ascontiguousarray(a[r])), n,
                                    T.ptr(np.ascontiguousarray(b[r])), m, T.ptr(o), 0) == ln
            assert T.bits_equal(y[r], o[:ln]), (typ, r)


def test_convolve_batched_sweep():
    """hsfft_convolve_batched over 47 signal lengths x 6 kernel lengths (either one the longer,
    P = 2 .. 2048), linear full / same / valid and circular, 2 rows each: bit-exact vs the
    oracle's convolve.c:20-214 (P = next power of two of the output length)."""
    L, lib = hsfft.lib(), T.oracle()
    rows, bad, calls = 2, [], 0
    for n in range(1, 600, 13):
        for m in (1, 2, 5, 64, 200, 511):
            a = T.real_input(n, 0x11 ^ n, batch=rows).reshape(rows, n)
            b = T.real_input(m, 0x22 ^ m, batch=rows).reshape(rows, m)
            da, db = hsfft.DeviceBuffer.from_array(a), hsfft.DeviceBuffer.from_array(b)
            dout = hsfft.DeviceBuffer(rows * 2 * (n + m) * 8)
            for typ, ct in ((b"full", b"linear"), (b"same", b"linear"), (b"valid", b"linear"),
                            (b"full", b"circular")):
                ln = L.hsfft_convolve_batched(typ, ct, da.ptr, n, db.ptr, m, dout.ptr, rows)
                calls += 1
                if n == m == 1:  # P = 1: the reference's length-1 real plan exits; an error here
                    if ln >= 0:
                        bad.append((n, m, typ, ct, "P=1 accepted"))
                    continue
                if ln <= 0:
                    bad.append((n, m, typ, ct, "rc", ln))
                    continue
                y = dout.to_array(np.float64, rows * ln).reshape(rows, ln)
                for r in range(rows):
                    o = np.zeros(4 * (n + m))
                    want = lib.orc_convolve(typ, ct, T.ptr(np.ascontiguousarray(a[r])), n,
                                            T.ptr(np.ascontiguousarray(b[r])), m, T.ptr(o), 0)
                    if want != ln or not T.bits_equal(y[r], o[:ln]):
                        bad.append((n, m, typ, ct, r))
            for buf in (da, db, dout):
                buf.free()
    assert calls == 47 * 6 * 4
    assert not bad, bad[:20]


@pytest.mark.parametrize("n,m,typ", [(1 << 16, 1000, b"full"), (70000, 70000, b"same"), (5000, 300, b"valid")])
def test_convolve_batched_at_scale(n, m, typ):
    """hsfft_convolve_batched with P = 2^17 .. 2^18 (two-pass inner c2c, fused compact r2c
    split, compact spectral product): every row bit-exact vs the oracle's convolve.c"""
    L = hsfft.lib()
    rows = 3
    a = T.real_input(n, 15, batch=rows).reshape(rows, n)
    b = T.real_input(m, 16, batch=rows).reshape(rows, m)
    da, db = hsfft.DeviceBuffer.from_array(a), hsfft.DeviceBuffer.from_array(b)
    dout = hsfft.DeviceBuffer(rows * (n + m) * 8)
    ln = L.hsfft_convolve_batched(typ, b"linear", da.ptr, n, db.ptr, m, dout.ptr, rows)
    assert ln > 0
    y = dout.to_array(np.float64, rows * ln).reshape(rows, ln)
    lib = T.oracle()
    for r in range(rows):
        o = np.zeros(2 * (n + m) + 8)
        assert lib.orc_convolve(typ, b"linear", T.ptr(np.ascontiguousarray(a[r])), n,
                                T.ptr(np.ascontiguousarray(b[r])), m, T.ptr(o), 0) == ln
        assert T.bits_equal(y[r], o[:ln]), (typ, r)
    for d in (da, db, dout):
        d.free()


def test_divergences_d3_d5_d6():
    """radix 13 (reference segfaults, D3), N=2^k+1 Bluestein (reference reads past its
    twiddles, D5), N=1 (reference exits, D6): correct results here, bit-exact vs oracle."""
    for n in [13, 26, 169, 257, 1025, 1]:
        for sgn in (1, -1):
            x = T.complex_input(n, T.seed_for(n))
            y = hsfft.Plan(n, sgn).exec(x)
            assert T.bits_equal(y, oracle_rows(x, sgn)), (n, sgn)
            X = np.fft.fft(x) if sgn == 1 else np.fft.ifft(x) * n
            # 1025 = 5^2*41 is mixed radix with the reference's 11-digit radix-5 constants
            assert np.abs(y - X).max() <= 1e-10 * max(1.0, np.abs(X).max()), n


@pytest.mark.parametrize("runtime", ["0", "1"])
def test_generic_odd_radices(runtime, monkeypatch):
    """radices 11..53 (ref :1475-1628): one compile-time kernel per odd radix (registers, no
    scratch), passes holding two different odd radices (11*13*8, 17*19, 29*31) on the
    runtime-radix stage; HSFFT_ODD_RUNTIME=1 forces the runtime stage everywhere"""
    if runtime == "1":
        monkeypatch.setenv("HSFFT_ODD_RUNTIME", "1")
    for n in [11, 121, 17 * 8, 23 * 4, 29 * 3, 31, 37 * 5, 41, 43 * 2, 47, 53 * 8, 11 * 13 * 8, 17 * 19, 29 * 31,
              11 ** 4, 53 * 4096]:
        rows = 2 if n < 100000 else 1
        x = T.complex_input(n, 3, batch=rows).reshape(rows, n)
        for sgn in (1, -1):
            assert T.bits_equal(gpu_c2c_batched(n, sgn, x), oracle_rows(x, sgn)), (n, sgn)


@pytest.mark.parametrize("n", [64, 1000, 2 * 97])
def test_real_and_convolve_batches_beyond_65535_rows(n):
    """row helper kernels index rows by blockIdx.y (<= 65535 per launch): larger batches are
    sliced; r2c (split not fused for these sizes), c2r and batched convolution of 70000 short
    rows, sampled rows bit-exact vs the oracle"""
    rows = 70000
    x = T.real_input(n, 0xE0 ^ n, batch=rows).reshape(rows, n)
    rp, ip = hsfft.RealPlan(n, 1), hsfft.RealPlan(n, -1)
    din = hsfft.DeviceBuffer.from_array(x)
    dX = hsfft.DeviceBuffer(rows * n * 16)
    hsfft.r2c_batched(rp, din, dX, rows)
    dY = hsfft.DeviceBuffer(rows * n * 8)
    hsfft.c2r_batched(ip, dX, dY, rows)
    hsfft.synchronize()
    for r in (0, 65534, 65535, 65536, rows - 1):
        X = dX.to_array(np.complex128, n, r * n * 16)
        assert T.bits_equal(X, T.oracle_r2c(x[r], 1)), ("r2c", n, r)
        y = dY.to_array(np.float64, n, r * n * 8)
        assert T.bits_equal(y, T.oracle_c2r(X, n, -1)), ("c2r", n, r)
    L = hsfft.lib()
    m = 7
    b = T.real_input(m, 0xE1 ^ n, batch=rows).reshape(rows, m)
    db = hsfft.DeviceBuffer.from_array(b)
    dout = hsfft.DeviceBuffer(rows * (n + m) * 8)
    ln = L.hsfft_convolve_batched(b"full", b"linear", din.ptr, n, db.ptr, m, dout.ptr, rows)
    assert ln == n + m - 1, L.hsfft_last_error()
    for r in (0, 65535, rows - 1):
        y = dout.to_array(np.float64, ln, r * ln * 8)
        o = np.zeros(2 * (n + m) + 8)
        assert T.oracle().orc_convolve(b"full", b"linear", T.ptr(np.ascontiguousarray(x[r])), n,
                                       T.ptr(np.ascontiguousarray(b[r])), m, T.ptr(o), 0) == ln
        assert T.bits_equal(y, o[:ln]), ("conv", n, r)
    for d in (din, dX, dY, db, dout):
        d.free()


def test_batch_edge_cases():
    L = hsfft.lib()
    p = hsfft.Plan(64, 1)
    d = hsfft.DeviceBuffer(64 * 16)
    assert L.hsfft_exec_batched(p.ptr, d.ptr, d.ptr, 1) < 0      # in == out refused
    assert L.hsfft_exec_batched(p.ptr, d.ptr, hsfft.DeviceBuffer(16).ptr, 0) == 0  # empty batch
    assert L.hsfft_exec_batched(None, d.ptr, d.ptr, 1) < 0


def test_full_size_config2_properties():
    """BASELINE config 2 at full size (4096 x 2^20, 64 GiB in / 64 GiB out): sampled rows
    bit-exact vs the oracle and a forward/inverse round trip."""
    n, batch = 1 << 20, 4096
    p, pi = hsfft.Plan(n, 1), hsfft.Plan(n, -1)
    din = hsfft.DeviceBuffer(batch * n * 16)
    dout = hsfft.DeviceBuffer(batch * n * 16)
    hsfft.fill_complex(din, batch * n, T.SEEDS[2])
    hsfft.exec_batched(p, din, dout, batch)
    hsfft.synchronize()
    for row in (0, 1777, batch - 1):
        y = dout.to_array(np.complex128, n, row * n * 16)
        x = T.complex_input(n, T.SEEDS[2], batch=1, row0=row)
        assert T.bits_equal(y, oracle_rows(x, 1)), row
    # inverse of the first 8 rows back into din's head: round trip
    hsfft.exec_batched(pi, dout, din, 8)
    hsfft.synchronize()
    z = din.to_array(np.complex128, 8 * n).reshape(8, n) / n
    x = T.complex_input(n, T.SEEDS[2], batch=8).reshape(8, n)
    assert np.abs(z - x).max() < 1e-13
    din.free()
    dout.free()


def test_multi_device_api_single_gpu():
    L = hsfft.lib()
    n, batch = 4096, 8
    p = hsfft.Plan(n, 1)
    x = T.complex_input(n, 9, batch=batch).reshape(batch, n)
    din = hsfft.DeviceBuffer.from_array(x)
    dout = hsfft.DeviceBuffer(x.nbytes)
    import ctypes
    ins = (ctypes.c_void_p * 1)(din.ptr)
    outs = (ctypes.c_void_p * 1)(dout.ptr)
    assert L.hsfft_exec_multi(p.ptr, ins, outs, batch, 1) == 0
    assert T.bits_equal(dout.to_array(np.complex128).reshape(batch, n), oracle_rows(x, 1))

@pytest.mark.gpu
@pytest.mark.parametrize("k", list(range(12, 24)))
def test_power_of_two_sweep_both_signs(k):
    """every power of two 2^12 .. 2^23 (one- and two-pass plans: the pipelined / paired-load
    kernels' applicability conditions on A, B, P), 3 rows, both signs, bit-exact vs oracle"""
    n = 1 << k
    batch = 3 if k <= 21 else 1
    x = T.complex_input(n, 0x5EED ^ k, batch=batch).reshape(batch, n)
    for sgn in (1, -1):
        assert T.bits_equal(gpu_c2c_batched(n, sgn, x), oracle_rows(x, sgn)), (n, sgn)


@pytest.mark.gpu
@pytest.mark.parametrize("n,sgn", [(1 << 24, 1), (1 << 25, -1), (1 << 26, 1), (3 ** 14, -1), (5 ** 9, 1), (7 ** 8, 1),
                                   (2 ** 6 * 3 ** 3 * 5 ** 2 * 7 ** 2, -1), (1000003, 1), (4194301, -1)])
def test_largest_sizes_bit_exact(n, sgn):
    """the largest single transforms (one row each): powers of two to 2^26 (1 GiB rows, chains
    of three and more passes), long single-radix chains (3^14, 5^9, 7^8: the reference's D2
    table quirk makes 3^14 / 7^8 numerically wrong, and the GPU reproduces those bits), a
    2M-point mixed size, and Bluestein at M = 2^21 (prime 1000003) and M = 2^23 (prime 4194301,
    the largest below 2^22) -- bit-exact vs the oracle (highSpeedFFT.c:1920-1942, :1735-1907)."""
    x = T.complex_input(n, 0x1A7 ^ n)
    y = gpu_c2c_batched(n, sgn, x.reshape(1, n)).reshape(n)
    ref = oracle_rows(x, sgn)
    assert T.bits_equal(y, ref), (n, sgn, T.mismatches(y, ref))


@pytest.mark.gpu
@pytest.mark.parametrize("n,sgn", [(1 << 26, 1), (1 << 24, -1), (2 * 1000003, 1), (2 * 12600 * 81, -1)])
def test_largest_real_sizes_bit_exact(n, sgn):
    """r2c at the largest sizes (one row): 2^26 reals (inner 2^25 c2c), a Bluestein inner
    transform (N/2 = 1000003, M = 2^21) and a mixed-radix inner size -- bit-exact vs the oracle
    (real.c:78-136)."""
    x = T.real_input(n, 0x2B7 ^ n).reshape(1, n)
    rp = hsfft.RealPlan(n, sgn)
    din = hsfft.DeviceBuffer.from_array(x)
    dout = hsfft.DeviceBuffer(n * 16)
    hsfft.r2c_batched(rp, din, dout, 1)
    y = dout.to_array(np.complex128).reshape(1, n)
    ref = T.oracle_r2c(x, sgn)
    assert T.bits_equal(y, ref), (n, sgn, T.mismatches(y, ref))
    din.free()
    dout.free()
    rp.close()


def test_two_pass_2pow21_batched():
    """2^21 = [8,8,8,8] (4096-point first pass) + [8,8,8]: bit-exact vs the oracle."""
    n = 1 << 21
    x = T.complex_input(n, 21, batch=3).reshape(3, n)
    p = hsfft.Plan(n, 1)
    assert p.num_passes() == 2
    din = hsfft.DeviceBuffer.from_array(x)
    dout = hsfft.DeviceBuffer(x.nbytes)
    hsfft.exec_batched(p, din, dout, 3)
    y = dout.to_array(np.complex128).reshape(3, n)
    assert T.bits_equal(y, T.oracle_c2c(x, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("fuse", ["0", "1"])
@pytest.mark.parametrize("n,sgn", [(1 << 19, 1), (1 << 22, 1), (1 << 22, -1), (1 << 13, 1)])
def test_r2c_fused_split(n, sgn, fuse, monkeypatch):
    """the real.c split fused into the last c2c pass (HSFFT_R2C_FUSE=1, default: pf::k_r2c_walk1;
    0: separate split kernel), bit-exact, both plan signs, odd batch."""
    monkeypatch.setenv("HSFFT_R2C_FUSE", fuse)
    x = T.real_input(n, 23, batch=3).reshape(3, n)
    rp = hsfft.RealPlan(n, sgn)
    din = hsfft.DeviceBuffer.from_array(x)
    dout = hsfft.DeviceBuffer(3 * n * 16)
    hsfft.r2c_batched(rp, din, dout, 3)
    y = dout.to_array(np.complex128).reshape(3, n)
    assert T.bits_equal(y, T.oracle_r2c(x, sgn))


@pytest.mark.gpu
@pytest.mark.parametrize("wt", ["walk0", "32", "1", "5", "4096"])
@pytest.mark.parametrize("n,sgn", [(1 << 22, 1), (1 << 22, -1), (1 << 19, 1), (1 << 17, -1)])
def test_r2c_walk1(n, sgn, wt, monkeypatch):
    """pf::k_r2c_walk1 (the default split kernel of the reference-layout r2c: two 512-thread
    workgroups per CU, one tile buffer, stage-0/1 twiddles from global memory, 80 KiB of LDS,
    whole-line stores with the one-entry carry between tiles, 8 rotation classes, the next hi
    tile's rows loaded before the pairs phase's stores): walks of 32 tile pairs (default), 1
    (every tile a walk's first: partial first line, carry written at once), 5 (uneven walks, a
    short last walk), 4096 (one walk per row: the carry reaches column B/2); walk0: the
    one-tile-per-workgroup pf::k_r2c_fused (HSFFT_R2C_WALK=0).  Bit-exact vs the oracle, odd
    batch, stale output buffer."""
    if wt == "walk0":
        monkeypatch.setenv("HSFFT_R2C_WALK", "0")
    else:
        monkeypatch.setenv("HSFFT_R2C_WT", wt)
    x = T.real_input(n, 31, batch=3).reshape(3, n)
    rp = hsfft.RealPlan(n, sgn)
    din = hsfft.DeviceBuffer.from_array(x)
    dout = hsfft.DeviceBuffer(3 * n * 16)
    hsfft.fill_complex(dout, 3 * n, 1)  # stale data: every bin must be written
    hsfft.r2c_batched(rp, din, dout, 3)
    y = dout.to_array(np.complex128).reshape(3, n)
    assert T.bits_equal(y, T.oracle_r2c(x, sgn))


@pytest.mark.gpu
def test_12600_row_kernel_edited_twiddles_refresh(monkeypatch):
    """The row kernel reads the last stage's twiddles from a transposed copy that the device
    state builds beside the plan's table: after the caller edits the plan's public twiddle
    table (last-stage and stage-4 entries) and calls hsfft_plan_refresh, the default schedule
    must use the edited values -- bit-equal to the two mixed-radix passes (which read the table
    as laid out) and to the row kernel reading the table directly, and different from the
    unedited transform"""
    import ctypes
    n, rows = 12600, 40
    x = T.complex_input(n, 91, batch=rows).reshape(rows, n)
    p = hsfft.Plan(n, 1)
    din = hsfft.DeviceBuffer.from_array(x)
    d0, d1, d2, d3 = (hsfft.DeviceBuffer(x.nbytes) for _ in range(4))
    hsfft.exec_batched(p, din, d0, rows)  # unedited, device state built
    hsfft.synchronize()
    tw = (ctypes.c_double * (2 * (n - 1))).from_address(p.ptr + hsfft.STRUCT_TWIDDLE_OFFSET)
    L5, L4 = n // 8, n // 56
    for e in list(range(L5 - 1, L5 - 1 + 7 * 40)) + list(range(n - 200, n - 1)) + list(range(L4 - 1, L4 + 60)):
        tw[2 * e] *= 0.75      # real part
        tw[2 * e + 1] += 0.125  # imaginary part
    hsfft.check(hsfft.lib().hsfft_plan_refresh(hsfft.VP(p.ptr)), "refresh")
    hsfft.exec_batched(p, din, d1, rows)  # default: transposed copy of the edited table
    hsfft.synchronize()
    monkeypatch.setenv("HSFFT_MR_ROW", "0")
    hsfft.exec_batched(p, din, d2, rows)
    hsfft.synchronize()
    monkeypatch.delenv("HSFFT_MR_ROW")
    monkeypatch.setenv("HSFFT_ROW_TWN", "0")
    hsfft.exec_batched(p, din, d3, rows)
    hsfft.synchronize()
    monkeypatch.delenv("HSFFT_ROW_TWN")
    y0, y1, y2, y3 = (d.to_array(np.complex128).reshape(rows, n) for d in (d0, d1, d2, d3))
    assert T.bits_equal(y1, y2)
    assert T.bits_equal(y1, y3)
    assert not np.array_equal(y0, y1)
    assert T.bits_equal(y0, T.oracle_c2c(x, 1))
    for d in (din, d0, d1, d2, d3):
        d.free()
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"HSFFT_ROW_F23": "0"}, {"HSFFT_MR_ROW": "0"}, {"HSFFT_ROW_F45": "0"},
                                 {"HSFFT_ROW_TWN": "0"}])
@pytest.mark.parametrize("sgn", [1, -1])
@pytest.mark.parametrize("rows", [300, 64])
def test_12600_row_kernel_variants(env, sgn, rows, monkeypatch):
    """config 3's schedules, bit-exact vs the oracle, both signs: 300 rows leave the
    row-walking grid uneven (300 rows over 256 workgroups); 64 rows give every workgroup
    exactly ONE row, so no row can lean on an earlier row's barriers (the stage-1 twiddles of
    the fused first stages are read right after the per-workgroup LDS copy).  Schedules:
    mr::k_row2 (default: 512 threads, stages 0-1 and 2-3 fused in registers, stages 4-5 fused
    over thread pairs (F45) with the stage-5 twiddles from the plan's transposed copy of that
    stage's block, the next row's first input group prefetched into registers), the same with
    stages 4 and 5 apart, without the stage 2-3 fusion, with F45's stage-5 twiddles read from
    the table as laid out (HSFFT_ROW_TWN=0), and the two mixed-radix passes."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = 12600
    x = T.complex_input(n, 77, batch=rows).reshape(rows, n)
    p = hsfft.Plan(n, sgn)
    assert p.num_passes() == (2 if env.get("HSFFT_MR_ROW") == "0" else 1)
    din = hsfft.DeviceBuffer.from_array(x)
    dout = hsfft.DeviceBuffer(x.nbytes)
    hsfft.exec_batched(p, din, dout, rows)
    y = dout.to_array(np.complex128).reshape(rows, n)
    assert T.bits_equal(y, T.oracle_c2c(x, sgn))


def _full_size_c2c(n, batch, seed, rows, sgn=1, tol=1e-13, roundtrip=True, flags=0):
    """a BASELINE config at its full per-GPU batch: sampled rows bit-exact vs the oracle and
    a forward/inverse round trip of the first rows (size-independent properties)."""
    p, pi = hsfft.Plan(n, sgn), hsfft.Plan(n, -sgn)
    din = hsfft.DeviceBuffer(batch * n * 16)
    dout = hsfft.DeviceBuffer(batch * n * 16)
    hsfft.fill_complex(din, batch * n, seed)
    hsfft.exec_batched(p, din, dout, batch)
    hsfft.synchronize()
    for row in rows:
        y = dout.to_array(np.complex128, n, row * n * 16)
        x = T.complex_input(n, seed, batch=1, row0=row)
        assert T.bits_equal(y, oracle_rows(x, sgn, flags)), row
    if roundtrip:
        hsfft.exec_batched(pi, dout, din, 4)
        hsfft.synchronize()
        z = din.to_array(np.complex128, 4 * n).reshape(4, n) / n
        x = T.complex_input(n, seed, batch=4).reshape(4, n)
        assert np.abs(z - x).max() < tol
    din.free()
    dout.free()


def test_full_size_config3_12600_x_65536():
    """config 3 at full size (65536 rows, 13 GB each way), bit-exact in the reference twiddle
    mode (whose D2 tables are not an exact inverse pair, so the round trip is checked in
    exact mode, limited by the reference's 11-digit radix-3/5/7 constants)"""
    _full_size_c2c(12600, 65536, T.SEEDS[3], (0, 40000, 65535), roundtrip=False)
    hsfft.set_twiddle_mode("exact")
    try:
        _full_size_c2c(12600, 2048, T.SEEDS[3], (0, 2047), tol=1e-9, flags=T.ORC_EXACT)
    finally:
        hsfft.set_twiddle_mode("reference")


def test_full_size_config4_bluestein_99991_x_8192():
    _full_size_c2c(99991, 8192, T.SEEDS[4], (0, 5000, 8191), tol=1e-10)


def test_full_size_config5_r2c_2pow22_rows():
    """config 5's row length (2^22 reals) at 512 rows per call (one GPU's 4096-row shard runs
    in 8 such calls in bench.py): sampled rows bit-exact vs the oracle, Hermitian mirror"""
    n, batch = 1 << 22, 512
    rp = hsfft.RealPlan(n, 1)
    din = hsfft.DeviceBuffer(batch * n * 8)
    dout = hsfft.DeviceBuffer(batch * n * 16)
    hsfft.fill_real(din, batch * n, T.SEEDS[5])
    hsfft.r2c_batched(rp, din, dout, batch)
    hsfft.synchronize()
    for row in (0, 311, batch - 1):
        y = dout.to_array(np.complex128, n, row * n * 16)
        x = T.real_input(n, T.SEEDS[5], batch=1, row0=row)
        assert T.bits_equal(y, T.oracle_r2c(x.reshape(1, n), 1)[0]), row
        assert np.array_equal(y[1:n // 2], np.conj(y[n - 1:n // 2:-1]))
    din.free()
    dout.free()
