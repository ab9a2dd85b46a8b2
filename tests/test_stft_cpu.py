"""CPU-only checks of the batched STFT and its inverse (hsfft_stft_shape, hsfft_stft_batched,
hsfft_istft_batched of include/hsfft_gpu.h):
  * the symbols are exported, declared and bound, and the Python callables exist;
  * hsfft_stft_shape equals the restated rule over a grid of n, N, hop and center, rejects what the
    rule rejects with a message and then writes no result;
  * every bad-argument case of both calls is rejected with HSFFT_ERR_ARG and a message before any
    device is touched (so it is testable here), and batch == 0 returns 0;
  * the Python conveniences reject bad shapes before loading anything;
  * the yardstick of test_gpu_stft.py -- the expectation composed in hsfft_stft_testlib from the
    reference's own r2c / c2r per frame -- is the reference's r2c of the row cut into blocks where
    the frames do not overlap, agrees with numpy.fft.rfft of independently built frames, and
    inverts itself as accurately as the reference's own r2c -> c2r round trip.

No call made here has valid arguments and a non-zero batch: nothing is ever launched, the
pointers are never dereferenced.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hsfft_stft_testlib as S
import hsfft_testlib as T

import hsfft

NAMES = ("hsfft_stft_shape", "hsfft_stft_batched", "hsfft_istft_batched")

GRID_N, GRID_NFFT, GRID_HOP, GRID_CENTER = (1, 5, 8, 16, 21, 100, 1000), (2, 8, 16, 100, 7, 0), (1, 3, 8, 11, 0), (0, 1, 2)

# The library is loaded in a child process, as in test_filter_cpu.py.  Both plans have N = 8.
# Forward: x is 3 rows of 100 (2400 bytes), the window 8 doubles (64 bytes), hop 4, not centred: 24
# frames of 5 bins, so the spectra are 3 x 24 x 5 x 16 = 5760 bytes.  The inverse reads those and
# writes 3 rows of 100.
CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import hsfft
L = hsfft.lib()
X, W, O = 0x100000, 0x200000, 0x300000  # distinct non-NULL "device pointers" (never dereferenced)
rf, ri = hsfft.RealPlan(8, 1), hsfft.RealPlan(8, -1)
def fwd(r=rf.ptr, x=X, n=100, w=W, hop=4, c=0, o=O, b=3):
    return (r, x, n, w, hop, c, o, b)
def inv(r=ri.ptr, s=X, nf=24, w=W, hop=4, c=0, norm=1, o=O, n=100, b=3):
    return (r, s, nf, w, hop, c, norm, o, n, b)
BIG = 1 << 30
bad_fwd = [("NULL plan", fwd(r=None)), ("NULL x", fwd(x=None)), ("NULL out", fwd(o=None)), ("negative batch", fwd(b=-1)),
           ("hop 0", fwd(hop=0)), ("hop -1", fwd(hop=-1)), ("n 0", fwd(n=0)), ("n -3", fwd(n=-3)),
           ("n below N without center", fwd(n=7)), ("center 2", fwd(c=2)), ("center -1", fwd(c=-1)),
           ("n above 2^30", fwd(n=BIG + 1)),
           ("nframes x batch above 2^31 - 1", fwd(n=BIG, hop=1, b=3)),
           ("n x batch above 2^40", fwd(n=BIG, hop=BIG, c=1, b=2000)),
           ("out == x", fwd(o=X)), ("out == w", fwd(o=W)),
           ("out starts in x's last 8 bytes", fwd(o=X + 2400 - 8)),
           ("x starts in out's last 8 bytes", fwd(x=O + 5760 - 8)),
           ("out starts in w's last 8 bytes", fwd(o=W + 64 - 8)),
           ("w starts in out's last 8 bytes", fwd(w=O + 5760 - 8)),
           ("out overlaps x only at batch 3", fwd(o=X + 2 * 800))]
zero_fwd = [fwd(b=0), fwd(b=0, o=X), fwd(b=0, w=None), fwd(b=0, o=X + 2 * 800), fwd(b=0, c=1, n=5)]
bad_inv = [("NULL plan", inv(r=None)), ("NULL spec", inv(s=None)), ("NULL out", inv(o=None)), ("negative batch", inv(b=-1)),
           ("nframes 0", inv(nf=0)), ("nframes -1", inv(nf=-1)), ("hop 0", inv(hop=0)), ("hop -2", inv(hop=-2)),
           ("center 2", inv(c=2)), ("center -1", inv(c=-1)), ("n 0", inv(n=0)), ("n -1", inv(n=-1)),
           ("n above 2^30", inv(n=BIG + 1)),
           ("nframes x batch above 2^31 - 1", inv(nf=BIG, b=3)),
           ("n x batch above 2^40", inv(n=BIG, b=2000)),
           ("out == spec", inv(o=X)), ("out == w", inv(o=W)),
           ("out starts in spec's last 8 bytes", inv(o=X + 5760 - 8)),
           ("spec starts in out's last 8 bytes", inv(s=O + 2400 - 8)),
           ("out starts in w's last 8 bytes", inv(o=W + 64 - 8)),
           ("w starts in out's last 8 bytes", inv(w=O + 2400 - 8)),
           ("out overlaps spec only at batch 3", inv(o=X + 2 * 1920))]
zero_inv = [inv(b=0), inv(b=0, o=X), inv(b=0, w=None), inv(b=0, n=5), inv(b=0, norm=0, c=1, n=1)]
out = {"exported": {n: hasattr(L, n) for n in ("hsfft_stft_shape", "hsfft_stft_batched", "hsfft_istft_batched")}}
out["bad_fwd"] = [(what, L.hsfft_stft_batched(*a), L.hsfft_last_error().decode()) for what, a in bad_fwd]
out["zero_fwd"] = [L.hsfft_stft_batched(*a) for a in zero_fwd]
out["bad_inv"] = [(what, L.hsfft_istft_batched(*a), L.hsfft_last_error().decode()) for what, a in bad_inv]
out["zero_inv"] = [L.hsfft_istft_batched(*a) for a in zero_inv]
v = [ctypes.c_int(-7) for _ in range(3)]
refs = [ctypes.byref(x) for x in v]
def shape(n, N, hop, c):
    for x in v:
        x.value = -7
    rc = L.hsfft_stft_shape(n, N, hop, c, *refs)
    return rc, [x.value for x in v], L.hsfft_last_error().decode()
out["shape_big"] = [shape(BIG, 2, 1, 1), shape(BIG + 1, 2, 1, 1), shape(BIG, BIG, 1, 0), shape(BIG, BIG + 2, 1, 1)]
out["shape_null_results"] = L.hsfft_stft_shape(100, 8, 4, 0, None, None, None)
grid = json.loads(sys.argv[2])
out["grid"] = [((n, N, hop, c),) + shape(n, N, hop, c)
               for n in grid["n"] for N in grid["N"] for hop in grid["hop"] for c in grid["center"]]
class Ptr:
    ptr = X
out["raised"] = {}
for what, fn in [("stft_batched", lambda: hsfft.stft_batched(rf, Ptr, 100, Ptr, 4, 0, Ptr, 3)),
                 ("istft_batched", lambda: hsfft.istft_batched(ri, Ptr, 24, None, 4, 0, 1, Ptr, 100, 3)),
                 ("stft_shape", lambda: hsfft.stft_shape(7, 8, 4))]:
    try:
        fn()
        out["raised"][what] = None
    except hsfft.HsfftError as e:
        out["raised"][what] = str(e)
out["shape_py"] = [list(hsfft.stft_shape(100, 8, 4)), list(hsfft.stft_shape(100, 8, 4, center=True))]
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def child():
    """what a fresh process saw: no call in it has valid arguments and a non-zero batch, so
    nothing is launched wherever it runs"""
    grid = json.dumps({"n": GRID_N, "N": GRID_NFFT, "hop": GRID_HOP, "center": GRID_CENTER})
    res = subprocess.run([sys.executable, "-c", CHILD, T.PKG_DIR, grid], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_symbols_exported_and_declared(child):
    assert os.path.exists(hsfft.LIB_PATH)
    header = open(os.path.join(T.REPO, "include", "hsfft_gpu.h")).read()
    for name in NAMES:
        assert child["exported"][name], name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in hsfft.SIGNATURES, name
    for name in ("stft_shape", "stft_batched", "istft_batched", "stft", "istft"):
        assert callable(getattr(hsfft, name, None)), name
    # the chunk rules the GPU test relies on, the bounds and the knob's place in the scratch comment are documented
    assert re.search(r"HSFFT_STFT_CHUNK_MB / \(N x 8\) consecutive frames", header)
    assert re.search(r"HSFFT_STFT_CHUNK_MB /[\s*]*\(nframes x N x 8\) rows", header)
    assert re.search(r"One row larger than the knob still runs[\s*]*as one chunk", header)
    assert "n or N > 2^30" in header and "nframes x batch > 2^31 - 1" in header
    scratch_comment = header[header.index("Frees the library's scratch pool"):header.index("int hsfft_release_scratch")]
    assert "HSFFT_STFT_CHUNK_MB" in scratch_comment


def test_shape_matches_the_restated_rule(child):
    assert len(child["grid"]) == len(GRID_N) * len(GRID_NFFT) * len(GRID_HOP) * len(GRID_CENTER)
    accepted = 0
    for (n, N, hop, c), rc, got, msg in child["grid"]:
        want = S.shape_rule(n, N, hop, c)
        if want is None:
            assert rc == hsfft.HSFFT_ERR_ARG and msg, (n, N, hop, c, rc, got)
            assert got == [-7] * 3, (n, N, hop, c, got)  # a rejected call writes no result
        else:
            assert rc == 0 and tuple(got) == want, (n, N, hop, c, rc, got, want)
            accepted += 1
    assert accepted >= len(child["grid"]) // 4  # a fair share of the grid is valid calls
    grid = {tuple(k): (rc, v) for k, rc, v, _ in child["grid"]}
    # spot values, written out: (nframes, bins, lpad)
    assert grid[(21, 8, 3, 0)] == (0, [5, 5, 0])     # frames start at 0, 3, .., 12; sample 20 is not reached
    assert grid[(21, 8, 8, 0)] == (0, [2, 5, 0])
    assert grid[(8, 8, 3, 0)] == (0, [1, 5, 0])
    assert grid[(100, 16, 3, 1)] == (0, [34, 9, 8])
    assert grid[(5, 16, 3, 1)] == (0, [2, 9, 8])     # a centred row may be shorter than the frame
    assert grid[(5, 16, 3, 0)][0] == hsfft.HSFFT_ERR_ARG
    assert grid[(16, 2, 1, 0)] == (0, [15, 2, 0])
    assert grid[(1, 2, 11, 1)] == (0, [1, 2, 1])
    assert child["shape_null_results"] == 0
    assert child["shape_py"] == [[24, 5, 0], [26, 5, 4]]
    big = child["shape_big"]  # the bound on n and N is 2^30, inclusive
    assert big[0][:2] == [0, [(1 << 30) + 1, 2, 1]] and big[2][:2] == [0, [1, (1 << 29) + 1, 0]]
    for rc, got, msg in (big[1], big[3]):
        assert rc == hsfft.HSFFT_ERR_ARG and msg and got == [-7] * 3


@pytest.mark.parametrize("which", ["fwd", "inv"])
def test_bad_arguments_are_rejected(child, which):
    """HSFFT_ERR_ARG and a message for every bad-argument case, before any device is touched;
    batch == 0 returns 0 -- also with no window, and for the inverse with n below N"""
    assert len(child["bad_" + which]) >= 20
    for what, rc, msg in child["bad_" + which]:
        assert rc == hsfft.HSFFT_ERR_ARG, (which, what, rc, msg)
        assert msg, (which, what)
    assert child["zero_" + which] == [0] * 5


def test_bad_arguments_raise_in_python(child):
    assert set(child["raised"]) == {"stft_batched", "istft_batched", "stft_shape"}
    assert "overlaps" in child["raised"]["stft_batched"]
    assert "overlaps" in child["raised"]["istft_batched"]
    assert "shorter than the frame" in child["raised"]["stft_shape"]


def test_conveniences_reject_bad_shapes_before_loading_anything():
    z = np.zeros
    for x, n_fft, hop, kw in [(z((2, 3, 64)), 8, 4, {}), (z(()), 8, 4, {}), (z(64), 7, 4, {}), (z(64), 0, 4, {}),
                              (z(64), -8, 4, {}), (z(64), 8, 0, {}), (z(7), 8, 4, {}), (z(0), 8, 4, {"center": True}),
                              (z((2, 0)), 8, 4, {"center": True}), (z(64), 8, 4, {"window": z(7)}),
                              (z(64), 8, 4, {"window": z((1, 8))})]:
        with pytest.raises(ValueError):
            hsfft.stft(x, n_fft, hop, **kw)
    for s, hop, kw in [(z(5, dtype=complex), 4, {}), (z((2, 2, 3, 5), dtype=complex), 4, {}), (z((3, 1), dtype=complex), 4, {}),
                       (z((0, 5), dtype=complex), 4, {}), (z((3, 5), dtype=complex), 0, {}),
                       (z((3, 5), dtype=complex), 4, {"window": z(9)}), (z((3, 5), dtype=complex), 4, {"length": 0}),
                       (z((1, 5), dtype=complex), 4, {"center": True})]:  # one centred frame of 8 covers 0 samples
        with pytest.raises(ValueError):
            hsfft.istft(s, hop, **kw)
    assert hsfft.stft(z((0, 100)), 8, 4).shape == (0, 24, 5)
    assert hsfft.stft(z((0, 100)), 8, 4, center=True).shape == (0, 26, 5)
    assert hsfft.istft(z((0, 24, 5), dtype=complex), 4).shape == (0, 100)
    assert hsfft.istft(z((0, 26, 5), dtype=complex), 4, center=True).shape == (0, 100)
    assert hsfft.istft(z((0, 26, 5), dtype=complex), 4, center=True, length=77).shape == (0, 77)


# ---------------------------------------------------------------- the yardstick, pinned
def _frames_by_loops(x, N, hop, center):
    """the padded frames by the definition, with explicit loops (not the indexing of the test library)"""
    n, lpad = len(x), (N // 2 if center else 0)
    nframes = 1 + n // hop if center else 1 + (n - N) // hop
    u = np.zeros((nframes, N))
    for f in range(nframes):
        for j in range(N):
            p = f * hop - lpad + j
            if 0 <= p < n:
                u[f, j] = x[p]
    return u


@pytest.mark.parametrize("n,N", [(64, 8), (1000, 100), (776, 194), (35, 2)], ids=lambda v: str(v))
def test_frames_that_do_not_overlap_are_the_rows_of_the_reference(n, N):
    """w None, hop == N, not centred: the expectation is T.oracle_r2c of the row cut into N-blocks,
    word for word (mixed-radix inner 50, Bluestein inner 97 and the one-point inner transform too)"""
    x = S.rows(n, 1, salt=0xC1)[0]
    nframes = n // N
    got = S.oracle_stft(x, None, N, N, 0)
    want = T.oracle_r2c(x[:nframes * N].reshape(nframes, N))[:, :N // 2 + 1]
    assert got.shape == (nframes, N // 2 + 1)
    assert T.mismatches(got, np.ascontiguousarray(want)) == 0


@pytest.mark.parametrize("n,N,hop,center", [(1000, 64, 16, 1), (300, 64, 24, 0), (21, 8, 3, 0), (5, 16, 4, 1)],
                         ids=lambda v: str(v))
def test_frame_indexing_agrees_with_numpy(n, N, hop, center):
    """numpy.fft.rfft of the same windowed frames, built by explicit loops: the normwise error is
    within the suite's bound of 4 for oracle-against-numpy comparisons (inner lengths 32, 4 and 8
    have no radix-3 stage, so the reference as it is computes a DFT there).  A frame taken from the
    wrong place gives an error of the order of the data, 1e15 in these units."""
    x, w = S.rows(n, 1, salt=0xC2)[0], S.window(N, salt=0xC2)
    u = _frames_by_loops(x, N, hop, center)
    assert u.shape[0] == S.shape_rule(n, N, hop, center)[0]
    assert T.mismatches(S.frames_of(x, N, hop, center), u) == 0
    for win in (w, None):
        got = S.oracle_stft(x, win, N, hop, center)
        want = np.fft.rfft(u * win if win is not None else u, axis=1)
        err = T.normwise_err(got, want)
        print(n, N, hop, center, "window" if win is not None else "no window", "normwise error", err)
        assert err <= 4, (n, N, hop, center, err)
    # the inverse's indexing: numpy's irfft of Hermitian-consistent frames, overlap-added by explicit loops
    X = np.fft.rfft(u * w, axis=1)
    natural = S.natural_length(u.shape[0], N, hop, center)
    lpad = N // 2 if center else 0
    for nout in (natural, max(1, natural - 3), natural + N + 5):
        y = np.fft.irfft(X, n=N, axis=1) * w
        want = np.zeros(nout)
        for f in range(u.shape[0]):
            for j in range(N):
                i = f * hop - lpad + j
                if 0 <= i < nout:
                    want[i] += y[f, j]
        got = S.oracle_istft(X, w, N, hop, center, 0, nout)
        err = T.normwise_err(got, want)
        print(n, N, hop, center, "inverse, length", nout, "normwise error", err)
        assert err <= 4, (n, N, hop, center, nout, err)


def test_round_trip_is_as_accurate_as_the_reference():
    """Measured: STFT -> inverse STFT error 4.44e-16, the reference's own r2c -> c2r -> / N round
    trip on the unwindowed frames 5.55e-16 (ratio 0.8).  The bound is 4 x the second: the margin
    covers two window multiplies, up to four adds and one division per sample.  A misplaced frame
    or a wrong envelope gives an error of the order of the data, 1e15 times larger."""
    _, _, err, ref = S.round_trip_errors()
    print("round trip error", err, "reference r2c -> c2r round trip error", ref, "ratio", err / ref if ref else np.inf)
    assert ref > 0
    assert err <= 4 * ref, (err, ref)
