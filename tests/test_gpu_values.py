"""GPU: the value domain.  Every other GPU test feeds dense splitmix values in [-1, 1), on
which several arithmetic differences cannot show: x * (1, 0) and x have the same bits for
finite non-zero x, and so have a - b and -(b - a) for a non-zero result.  The reference skips
the k = 0 twiddle multiply for radix 4 / 5 / 7 and performs it for radix 2 / 8 and the odd
radices, and every kernel restates that rule; only exact zeros (-0 * 1 + x * 0 is +0) and
non-finite values (inf * 0 is NaN) tell a kernel that skips from one that multiplies.  Here
each kernel family runs on the rows of hsfft_testlib.special_inputs: constant, alternating and
comb rows (whose spectra are almost all exact +0), fields of signed zeros, impulses, real-only
rows with signed zero imaginary parts, subnormals (2^-1040) and values near overflow (2^1000).

Tolerance: BIT-EXACT against the oracle (which test_oracle_pin.py pins to the reference on the
same inputs) -- the sign of every zero counts.  The one exception is the non-finite test:
x86 and the GPU give a default NaN different sign and payload bits, so there NaN words must
coincide by class and every other word -- signed zeros and infinities included -- is bit-equal
(hsfft_testlib.same_bits_nan_aware).

Each case names the kernel family it is there for, sets the knob that forces it where one is
needed and asserts the plan's pass count (and Bluestein flag) as the tests that introduced
those knobs do, so a renamed knob fails the case instead of quietly running the default
schedule.  One call mixes kinds: each row of a batch is of another kind, and the kinds rotate
with the case so that every kind meets every case.  Cases of M >= 2^17 points (where the
oracle takes 0.1 s to 3 s per row) run one group of kinds instead of all nine; the group
rotates with the case.
"""
import collections
import ctypes

import numpy as np
import pytest

import hsfft_testlib as T

import hsfft

pytestmark = pytest.mark.gpu

KINDS = T.SPECIAL_KINDS


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if hsfft.device_count() < 1:
        pytest.skip("no GPU")
    hsfft.lib().hsfft_set_device(0)
    _preconditions()
    yield
    hsfft.synchronize()
    _ORACLE.clear()


# ---------------------------------------------------------------- shared oracle results
_ORACLE = {}


def _x(n, kind):
    return T.special_inputs(n, kind, T.seed_for(n))


def _want(n, kind, sgn, flags=0):
    """the oracle's transform of the row of this kind, computed once per module"""
    key = (n, kind, sgn, flags)
    if key not in _ORACLE:
        _ORACLE[key] = T.oracle_c2c(_x(n, kind), sgn, flags)
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]


def _preconditions():
    """what makes the comparisons below mean something (test_special_cpu.py pins the same from
    the oracle on every machine; here they are checked in the process that has the GPU library
    loaded, which must not have changed the host's floating-point mode)"""
    x = np.zeros(8, dtype=np.complex128)
    x[0] = 5e-324
    assert np.count_nonzero(T.oracle_c2c(x, 1)) == 8, "the host flushes subnormals to zero"
    for n in T.ZERO_RICH_SIZES:
        for kind in ("const", "alt", "comb4"):
            assert T.zero_words(_want(n, kind, 1)) >= n, (n, kind)
        assert T.zero_words(_want(n, "tiny", 1)) == 0, n
        assert np.isfinite(_want(n, "huge", 1).view(np.float64)).all(), n


def _groups(case_index, rows, ngroups):
    """the nine kinds rotated by the case index, in groups of `rows` (the last may be shorter)"""
    order = [KINDS[(case_index + i) % len(KINDS)] for i in range(len(KINDS))]
    groups = [order[i:i + rows] for i in range(0, len(order), rows)]
    return groups if ngroups is None else [groups[(case_index + g) % len(groups)] for g in range(ngroups)]


def _assert_rows(y, want, what):
    ok = T.bits_equal(y, want)
    if not ok:
        print(what, "mismatching words", T.mismatches(y, want), "first at", T.first_diff(y, want))
    assert ok, (what, T.mismatches(y, want), T.first_diff(y, want))


# ---------------------------------------------------------------- a. c2c by kernel family
Case = collections.namedtuple("Case", "family n env passes lt rows groups path")


def C(family, n, env=None, passes=1, lt=0, rows=3, groups=None, path="batched"):
    return Case(family, n, env or {}, passes, lt, rows, groups, path)


W0, W1 = {"HSFFT_WHOLE": "0"}, {"HSFFT_WHOLE": "1"}
C2C_CASES = (
    # the small drop-in path: fft_exec on host pointers, one page-locked zero-copy launch
    [C("dropin", n, path="host") for n in (8, 12, 60, 100, 512, 1024)] + [C("dropin", 97, lt=1, path="host")] +
    # radix-8 register kernels: one whole-row pass; 8192 = [2,8,8,8,8] whole and as [2,8][8,8,8]
    [C("r8-whole", 512), C("r8-whole", 2048), C("r8-whole", 4096), C("r8-whole", 8192, W1), C("r8-two", 8192, W0, 2)] +
    # two passes: [2,8,8] + pf::k_b512; 2^20 with the pipelined first pass and k_b512 (HSFFT_PF=3)
    # and with r8::k_pass for both (0); 2^21: the paired-load first pass [8,8,8,8]
    [C("r8-two", 65536, passes=2), C("pf", 1 << 20, {"HSFFT_PF": "3"}, 2, rows=2, groups=1),
     C("pf-off", 1 << 20, {"HSFFT_PF": "0"}, 2, rows=2, groups=1), C("paired", 1 << 21, passes=2, rows=1, groups=1)] +
    # the three-pass register chain [2,8][8,8][8,8]
    [C("r8-three", 65536, {"HSFFT_K1": "1"}, 3)] +
    # the generic LDS kernel: odd radices 7*11*13, 17^3, 8*11*13, one power-of-two radix per pass,
    # and the runtime-radix stage (17*19 is a Bluestein length -- 19 is missing from the
    # reference's dividebyN, D10 -- so 17*23 and 29*31 carry that knob to the generic kernel)
    [C("generic", 1001, passes=2), C("generic", 4913), C("generic", 11 * 13 * 8, passes=2),
     C("generic", 8192, {"HSFFT_GENERIC": "1", "HSFFT_PMAX": "8"}, 5),
     C("odd-runtime", 17 * 19, {"HSFFT_ODD_RUNTIME": "1"}, lt=1), C("odd-runtime", 17 * 23, {"HSFFT_ODD_RUNTIME": "1"}),
     C("odd-runtime", 29 * 31, {"HSFFT_ODD_RUNTIME": "1"}, 2)] +
    # mixed radix: one whole-row pass, and [5,5,5][8] / [3,5,5,5][8] / [5,5,5][5,8]
    [C("mixed", n, env, 1 if env is W1 else 2) for n in (1000, 3000, 5000) for env in (W1, W0)] +
    # the 12600 row kernel and its variants; the two mixed-radix register passes
    [C("row", 12600), C("row", 12600, {"HSFFT_ROW_F23": "0"}), C("row", 12600, {"HSFFT_ROW_F45": "0"}),
     C("row", 12600, {"HSFFT_ROW_TWN": "0"}), C("mr-two", 12600, {"HSFFT_MR_ROW": "0"}, 2)] +
    # the radix-4 combine (the reference skips its k = 0 twiddle) after every other radix
    [C("radix4", n) for n in (12, 20, 28, 36, 4 * 11, 4 * 125, 4 * 343, 4 * 8 * 8 * 3)] +
    # Bluestein: M = 256, 2^14, 2^17 chains; M = 2^18 persistent, three launches, and the
    # row-looped kernels off and on
    [C("bluestein", 97, lt=1), C("bluestein", 5003, passes=2, lt=1), C("bluestein", 40009, passes=2, lt=1, groups=1),
     C("bluestein", 99991, passes=2, lt=1, groups=1), C("bluestein", 99991, {"HSFFT_BLUE_XCD": "0"}, 2, 1, groups=1),
     C("bluestein", 65537, {"HSFFT_BLUE_PF": "0"}, 2, 1, groups=1),
     C("bluestein", 65537, {"HSFFT_BLUE_PF": "7"}, 2, 1, groups=1)]
)


def _case_id(c):
    return "-".join([c.family, str(c.n)] + [f"{k[6:]}={v}" for k, v in sorted(c.env.items())])


def _run_c2c(c, p, x, sgn):
    if c.path == "host":
        return np.stack([p.exec(row) for row in x])
    rows = x.shape[0]
    din = hsfft.DeviceBuffer.from_array(x)
    dout = hsfft.DeviceBuffer(x.nbytes)
    hsfft.exec_batched(p, din, dout, rows)
    hsfft.synchronize()
    y = dout.to_array(np.complex128).reshape(x.shape)
    din.free()
    dout.free()
    return y


@pytest.mark.parametrize("i,c", list(enumerate(C2C_CASES)), ids=[_case_id(c) for c in C2C_CASES])
def test_c2c_special_values(i, c, monkeypatch):
    """one kernel family per case, both signs, every kind (one kind per row), bit-exact"""
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    n = c.n
    for sgn in (1, -1):
        p = hsfft.Plan(n, sgn)
        assert p.num_passes() == c.passes and p.header()["lt"] == c.lt, (_case_id(c), p.num_passes(), p.header()["lt"])
        for kinds in _groups(i, c.rows, c.groups):
            x = np.stack([_x(n, k) for k in kinds])
            y = _run_c2c(c, p, x, sgn)
            for r, k in enumerate(kinds):
                _assert_rows(y[r], _want(n, k, sgn), (_case_id(c), sgn, k))
        p.close()


@pytest.mark.parametrize("n", [12600, 1000])
def test_c2c_special_values_exact_twiddle_mode(n):
    """the exact twiddle mode (every stage twiddle from sincos), against the oracle's"""
    hsfft.set_twiddle_mode("exact")
    try:
        for sgn in (1, -1):
            p = hsfft.Plan(n, sgn)
            assert p.num_passes() == 1
            for kinds in _groups(n, 3, None):
                y = _run_c2c(C("exact", n), p, np.stack([_x(n, k) for k in kinds]), sgn)
                for r, k in enumerate(kinds):
                    _assert_rows(y[r], _want(n, k, sgn, T.ORC_EXACT), ("exact", n, sgn, k))
            p.close()
    finally:
        hsfft.set_twiddle_mode("reference")


# ---------------------------------------------------------------- b. real transforms
def _inner(rp):
    """(pass count, Bluestein flag) of a real plan's inner N/2-point complex plan"""
    c = ctypes.c_void_p.from_address(rp.ptr).value
    return (hsfft.check(hsfft.lib().hsfft_plan_num_passes(c), "num_passes"), (ctypes.c_int * 68).from_address(c)[67])


_REAL = {}


def _real_rows(n, kinds):
    """the real special rows and, per plan sign, the oracle's r2c of them (once per module)"""
    for k in kinds:
        if (n, k) not in _REAL:
            x = T.special_real(n, k, T.seed_for(n))
            _REAL[(n, k)] = (x, {sgn: T.oracle_r2c(x, sgn) for sgn in (1, -1)})
    return np.stack([_REAL[(n, k)][0] for k in kinds]), {s: np.stack([_REAL[(n, k)][1][s] for k in kinds]) for s in (1, -1)}


R2C_CASES = [
    # N, knobs, passes of the inner N/2-point plan, its Bluestein flag
    (1 << 13, {"HSFFT_R2C_FUSE": "0"}, 1, 0), (1 << 13, {"HSFFT_R2C_FUSE": "1"}, 1, 0),  # inner 4096: one pass, split apart
    (1 << 17, {"HSFFT_R2C_FUSE": "0"}, 2, 0),  # the separate split kernel
    (1 << 17, {"HSFFT_R2C_FUSE": "1"}, 2, 0),  # pf::k_r2c_walk1 (compact: k_r2c_fused)
    (1 << 17, {"HSFFT_R2C_WALK": "0"}, 2, 0),  # pf::k_r2c_fused
    (1 << 17, {"HSFFT_R2C_WT": "1"}, 2, 0),    # walks of one tile
    (1000, {}, 1, 0),                          # inner 500 = [4,5,5,5]
    (2 * 5003, {}, 2, 1),                      # inner 5003: Bluestein
]


@pytest.mark.parametrize("i,case", list(enumerate(R2C_CASES)),
                         ids=[f"{n}" + "".join(f"-{k[6:]}={v}" for k, v in e.items()) for n, e, _, _ in R2C_CASES])
def test_r2c_special_values(i, case, monkeypatch):
    """r2c of the real special rows: both plan signs, the reference layout and the compact one,
    every kind"""
    n, env, passes, lt = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h1 = n // 2 + 1
    for kinds in _groups(i, 3, None):
        x, want = _real_rows(n, kinds)
        din = hsfft.DeviceBuffer.from_array(x)
        dout = hsfft.DeviceBuffer(3 * n * 16)
        for sgn in (1, -1):
            rp = hsfft.RealPlan(n, sgn)
            assert _inner(rp) == (passes, lt), (n, env, _inner(rp))
            hsfft.r2c_batched(rp, din, dout, 3)
            y = dout.to_array(np.complex128).reshape(3, n)
            hsfft.r2c_batched_compact(rp, din, dout, 3)
            yc = dout.to_array(np.complex128, 3 * h1).reshape(3, h1)
            for r, k in enumerate(kinds):
                _assert_rows(y[r], want[sgn][r], ("r2c", n, env, sgn, k))
                _assert_rows(yc[r], np.ascontiguousarray(want[sgn][r, :h1]), ("r2c compact", n, env, sgn, k))
            rp.close()
        din.free()
        dout.free()


@pytest.mark.parametrize("n,passes,lt", [(16, 1, 0), (1000, 1, 0), (1 << 16, 2, 0), (2 * 5003, 2, 1)])
def test_c2r_special_values(n, passes, lt):
    """c2r of the oracle's spectra of the real special rows, every kind"""
    rp = hsfft.RealPlan(n, -1)
    assert _inner(rp) == (passes, lt)
    for kinds in _groups(n, 3, None):
        X = _real_rows(n, kinds)[1][1]
        dX = hsfft.DeviceBuffer.from_array(X)
        dout = hsfft.DeviceBuffer(3 * n * 8)
        hsfft.c2r_batched(rp, dX, dout, 3)
        y = dout.to_array(np.float64).reshape(3, n)
        for r, k in enumerate(kinds):
            _assert_rows(y[r], T.oracle_c2r(X[r], n, -1), ("c2r", n, k))
        dX.free()
        dout.free()
    rp.close()


CONV_CASES = [(300, 17, b"full", b"linear"), (300, 17, b"same", b"linear"), (300, 17, b"valid", b"linear"),
              (300, 17, b"full", b"circular"), (5000, 300, b"full", b"linear")]


@pytest.mark.parametrize("i,case", list(enumerate(CONV_CASES)), ids=[f"{n}x{m}-{t.decode()}-{c.decode()}"
                                                                       for n, m, t, c in CONV_CASES])
def test_convolve_special_values(i, case):
    """hsfft_convolve_batched: signals of every kind against dense kernels (one operand scaled:
    the product of the huge row stays finite, which is asserted)"""
    n, m, typ, ct = case
    L = hsfft.lib()
    for kinds in _groups(i, 3, None):
        a = T.special_rows(n, kinds, T.seed_for(n), real=True)
        b = T.real_input(m, T.seed_for(m) ^ 0xC1, batch=3).reshape(3, m)
        want = [T.oracle_convolve(typ, ct, a[r], b[r]) for r in range(3)]
        assert all(np.isfinite(w).all() for w in want)
        ln = want[0].size
        da, db = hsfft.DeviceBuffer.from_array(a), hsfft.DeviceBuffer.from_array(b)
        dout = hsfft.DeviceBuffer(3 * ln * 8)
        assert L.hsfft_convolve_batched(typ, ct, da.ptr, n, db.ptr, m, dout.ptr, 3) == ln, L.hsfft_last_error()
        y = dout.to_array(np.float64).reshape(3, ln)
        for r, k in enumerate(kinds):
            _assert_rows(y[r], want[r], ("convolve", case, k))
        for d in (da, db, dout):
            d.free()


# ---------------------------------------------------------------- c. non-finite inputs
# N = 8 is not here: no candidate index gives a partial mix of NaN words (hsfft_testlib.py,
# NONFINITE_LEFT_OUT; pinned by test_special_cpu.py).  All-NaN outputs would assert nothing.
# Besides the index of the table, each mixed-radix length runs hsfft_testlib.skip_probe_index:
# the finite kinds and an Inf at an arbitrary index can hardly tell a late combine stage that
# multiplies at k = 0 from one that skips (its k = 0 inputs are sums of whole sub-sequences, +0
# for any field of mixed zeros, and an Inf elsewhere is NaN before it gets there), the probe
# brings a clean Inf to every skipped multiply.  Its condition is that the oracle's rows keep
# at least 8 infinite words.  The knob variants are there because each schedule of 12600 and
# the one- and two-pass forms of 1000, 3000 and 5000 restate the skip rule in code of their own.
NONFINITE_CASES = [(n, {}, None) for n in sorted(T.NONFINITE_INDEX)] + [
    (12600, {"HSFFT_ROW_F23": "0"}, 1), (12600, {"HSFFT_ROW_F45": "0"}, 1), (12600, {"HSFFT_ROW_TWN": "0"}, 1),
    (12600, {"HSFFT_MR_ROW": "0"}, 2), (12600, {"HSFFT_MR_ROW": "0", "HSFFT_WHOLE": "0", "HSFFT_PMAX": "64"}, 3),
    (1000, W0, 2), (100, {"HSFFT_GENERIC": "1"}, 1), (3000, W1, 1), (3000, W0, 2), (5000, W1, 1), (5000, W0, 2),
    (500, {}, 1), (1372, {}, 1)]


def _nonfinite_inputs(n):
    """(what, rows, lower and upper bound of the NaN fraction, least count of Inf words)"""
    sets = []
    if n in T.NONFINITE_INDEX:
        sets.append(("table", T.nonfinite_rows(n, T.NONFINITE_INDEX[n], T.seed_for(n)), 0.01, 0.99, 0))
    if T.skip_probe_index(n):
        sets.append(("probe", T.nonfinite_rows(n, T.skip_probe_index(n), T.seed_for(n) ^ 1), 0.0, 1.0 - 0.5 / n, 8))
    assert sets
    return sets


@pytest.mark.parametrize("n,env,passes", NONFINITE_CASES,
                         ids=[f"{n}" + "".join(f"-{k[6:]}={v}" for k, v in sorted(e.items())) for n, e, _ in NONFINITE_CASES])
def test_c2c_one_infinite_element(n, env, passes, monkeypatch):
    """one row with +Inf in the real part at one index, one with -Inf in the imaginary part
    there, one finite row: NaN words where the oracle has them -- a k = 0 twiddle multiplied
    where the reference skips it turns Inf into NaN (inf * 0) -- and every other word, the signs
    of Inf and of zero included, bit-equal.  Device-resident batch; up to 1024 points also
    through fft_exec on host pointers.  The conditions (1 % to 99 % NaN words in the oracle's
    rows for the table's index, infinite words left for the probe) are asserted from the oracle."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for what, x, lo, hi, infs in _nonfinite_inputs(n):
        for sgn in (1, -1):
            want = T.oracle_c2c(x, sgn)
            for r in (0, 1):
                assert lo <= T.nan_fraction(want[r]) <= hi, (n, what, sgn, r, T.nan_fraction(want[r]))
                assert T.inf_words(want[r]) >= infs, (n, what, sgn, r, T.inf_words(want[r]))
            p = hsfft.Plan(n, sgn)
            assert passes is None or p.num_passes() == passes, (n, env, p.num_passes())
            paths = [("batched", _run_c2c(C("nonfinite", n), p, x, sgn))]
            if n <= 1024:
                paths.append(("host", _run_c2c(C("nonfinite", n, path="host"), p, x, sgn)))
            for path, y in paths:
                for r in range(3):
                    same = T.same_bits_nan_aware(y[r], want[r])
                    if not same:
                        print(n, what, sgn, path, "row", r, "NaN words", int(T.nan_words(y[r]).sum()), "oracle",
                              int(T.nan_words(want[r]).sum()))
                    assert same, (n, what, sgn, path, r)
                assert T.bits_equal(y[2], want[2]), (n, what, sgn, path, "finite row")
            p.close()
