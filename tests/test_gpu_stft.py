"""GPU: the batched STFT hsfft_stft_batched and its inverse hsfft_istft_batched (hsfft_stft.h).

Tolerance: BIT-EXACT, as everywhere in the suite.  Expected values come from hsfft_stft_testlib
alone -- numpy's padded frames times the window, one float64 multiply per word, through the
reference's r2c of the pinned oracle; and for the inverse the reference's c2r of every frame, one
division, one multiply and the frames added per sample in increasing order, the first term stored
(checked against numpy.fft and as a round trip in test_stft_cpu.py) -- never from the code under
test.  Every output buffer is filled with NaN before the call, so a word that was never written
shows, and lies between sentinel words that must come back unchanged; the inputs are read back
unchanged.
"""
import numpy as np
import pytest

import hsfft_stft_testlib as S
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
    for p in _PLANS.values():
        p.close()
    _PLANS.clear()
    _ORACLE.clear()


_ORACLE, _PLANS = {}, {}


def _plan(N, sgn):
    if (N, sgn) not in _PLANS:
        _PLANS[(N, sgn)] = hsfft.RealPlan(N, sgn)
    return _PLANS[(N, sgn)]


def _cached(key, make):
    """expected values computed once per module and kept read-only"""
    if key not in _ORACLE:
        val = make()
        for a in val.values():
            if a is not None:
                a.setflags(write=False)
        _ORACLE[key] = val
    return _ORACLE[key]


def _case(n, N, hop, center, batch=3, salt=0):
    """one oracle run per case serves every mode, output length and smaller batch (rows are
    independent): x (batch, n) dense, the dense random window w, the expected spectra with and
    without it, dense random spectra `spec` for the inverse (not Hermitian-consistent: the contract
    is compositional) and their scaled frames v = c2r / N"""
    def make():
        x, w = S.rows(n, batch, salt=0xE5 ^ salt), S.window(N, salt=0xE5 ^ salt)
        nframes, bins, _ = S.shape_rule(n, N, hop, center)
        spec = S.spectra(batch, nframes, bins, salt=0xE5 ^ salt)
        return dict(x=x, w=w, fwd_w=S.oracle_stft(x, w, N, hop, center), fwd_0=S.oracle_stft(x, None, N, hop, center),
                    spec=spec, v=S.oracle_scaled_frames(spec, N))
    return _cached((n, N, hop, center, batch, salt), make)


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
        return img[self.lead:self.lead + self.count].copy(), int(np.count_nonzero(guard != SENTINEL))

    def free(self):
        self.buf.free()


def _assert_bits(y, want, what):
    bad = T.mismatches(y, want)
    assert bad == 0, (what, "mismatching words", bad, "first at", T.first_diff(y, want),
                      "NaN words left", int(T.nan_words(y).sum()))


def _assert_bits_nan_aware(y, want, what):
    assert T.same_bits_nan_aware(y, want), (what, "NaN words", int(T.nan_words(y).sum()), "expected",
                                            int(T.nan_words(want).sum()))


def _upload(a, lead):
    """a on the device behind `lead` doubles: (owning buffer, the view that starts at a)"""
    buf = hsfft.DeviceBuffer(lead * 8 + a.nbytes)
    view = hsfft.DeviceView(buf, lead * 8)
    hsfft.check(hsfft.lib().hsfft_memcpy_h2d(view.ptr, a.ctypes.data, a.nbytes), "h2d")
    return buf, view


def _back(buf, a, lead):
    return buf.to_array(a.dtype, offset_bytes=lead * 8).reshape(a.shape)


def _run(forward, a, w, N, hop, center, want, what, normalize=1, lead=0, compare=_assert_bits, sgn=None):
    """one call on fresh buffers, checked against `want`: forward on the rows a (batch, n), or the
    inverse on the spectra a (batch, nframes, N/2+1) into rows of want.shape[1] samples; lead:
    doubles in front of every buffer"""
    a = np.ascontiguousarray(a)
    w = None if w is None else np.ascontiguousarray(w)
    batch = a.shape[0]
    (abuf, da), (wbuf, dw) = _upload(a, lead), (_upload(w, lead) if w is not None else (None, None))
    out = Out(want.size * (2 if forward else 1), lead=lead)
    if forward:
        hsfft.stft_batched(_plan(N, sgn or 1), da, a.shape[1], dw, hop, center, out, batch)
    else:
        hsfft.istft_batched(_plan(N, sgn or -1), da, a.shape[1], dw, hop, center, normalize, out, want.shape[1], batch)
    hsfft.synchronize()
    y, guard = out.read()
    ain = _back(abuf, a, lead)
    win = _back(wbuf, w, lead) if w is not None else None
    for d in (abuf, wbuf, out):
        if d is not None:
            d.free()
    y = y.view(np.complex128 if forward else np.float64).reshape(want.shape)
    compare(y, want, what)
    assert guard == 0, (what, "sentinel words changed", guard)
    _assert_bits(ain, a, (what, "the input changed"))
    if w is not None:
        _assert_bits(win, w, (what, "the window changed"))
    return y


# the smallest shapes at which each piece can go wrong: (n, N, hop, center)
SWEEP = [
    (16, 2, 1, 0),             # inner c2c of one point
    (21, 8, 3, 0),             # odd hop: frame starts alternately 8- and 16-byte aligned; sample 20 is never reached
    (21, 8, 8, 0),             # no overlap, five samples left over
    (30, 8, 11, 0),            # hop > N: gaps between frames
    (8, 8, 4, 0),              # one frame
    (100, 16, 4, 1),           # centred: frames reach before the row and past its end
    (5, 16, 4, 1),             # a row shorter than the frame: a gather that reads the neighbour row shows
    (1000, 100, 25, 1),        # inner mixed-radix length 50
    (600, 194, 50, 0),         # inner Bluestein length 97
    (5000, 1024, 256, 1),      # the common small case
    (40000, 4096, 1024, 0),    # inner 2048
    (70000, 32768, 8192, 1),   # inner 16384, two passes
]
SWEEP_IDS = ["%d_N%d_hop%d_c%d" % c for c in SWEEP]


def _lengths(nframes, N, hop, center):
    """the natural output length, 3 shorter, and N + 5 longer"""
    natural = S.natural_length(nframes, N, hop, center)
    return [k for k in (natural, natural - 3, natural + N + 5) if k >= 1]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n,N,hop,center", SWEEP, ids=SWEEP_IDS)
def test_stft(n, N, hop, center, batch):
    """with a dense random window and with none; with batch 3 the rows are dense and all different,
    so a frame gathered from the neighbouring row shows"""
    c = _case(n, N, hop, center)
    assert not np.array_equal(c["x"][0], c["x"][1]) and not np.array_equal(c["x"][1], c["x"][2])
    nframes, bins, _ = hsfft.stft_shape(n, N, hop, center)
    assert c["fwd_w"].shape == (3, nframes, bins)
    _run(True, c["x"][:batch], c["w"], N, hop, center, c["fwd_w"][:batch], (n, N, hop, center, batch, "window"))
    _run(True, c["x"][:batch], None, N, hop, center, c["fwd_0"][:batch], (n, N, hop, center, batch, "no window"))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n,N,hop,center", SWEEP, ids=SWEEP_IDS)
def test_istft(n, N, hop, center, batch):
    """dense random spectra; normalised or not, with and without a window, into rows of the natural
    length, 3 shorter (a trim) and N + 5 longer (+0.0 beyond the last frame's reach)"""
    c = _case(n, N, hop, center)
    nframes = c["spec"].shape[1]
    lengths = _lengths(nframes, N, hop, center)
    assert len(lengths) >= 2
    for nout in lengths:
        for w in (c["w"], None):
            for normalize in (0, 1):
                want = S.oracle_istft_of_frames(c["v"][:batch], w, N, hop, center, normalize, nout)
                if nout > S.natural_length(nframes, N, hop, center):
                    assert T.zero_words(want[:, -5:]) == 5 * batch and not np.signbit(want[:, -5:]).any()
                _run(False, c["spec"][:batch], w, N, hop, center, want,
                     (n, N, hop, center, batch, nout, "window" if w is not None else "no window", normalize),
                     normalize=normalize)


def test_samples_between_frames_are_plus_zero():
    """(30, 8, 11, 0): frames cover 0..7, 11..18, 22..29; the samples in between are +0.0, normalised
    (no 0 / 0) or not"""
    n, N, hop = 30, 8, 11
    c = _case(n, N, hop, 0)
    assert c["spec"].shape[1] == 3
    for normalize in (0, 1):
        want = S.oracle_istft_of_frames(c["v"], c["w"], N, hop, 0, normalize, n)
        y = _run(False, c["spec"], c["w"], N, hop, 0, want, ("gaps", normalize), normalize=normalize)
        for lo, hi in ((8, 11), (19, 22)):
            assert T.zero_words(y[:, lo:hi]) == 3 * (hi - lo) and not np.signbit(y[:, lo:hi]).any()
        assert np.count_nonzero(y[:, :8]) == 3 * 8


def test_plans_are_applied_as_planned():
    """an inverse-sign plan forward and a forward-sign plan in the inverse: each is applied as it is"""
    n, N, hop, center = 100, 16, 4, 1
    c = _case(n, N, hop, center)
    _run(True, c["x"], c["w"], N, hop, center, S.oracle_stft(c["x"], c["w"], N, hop, center, sgn=-1), "sgn -1 forward", sgn=-1)
    want = S.oracle_istft(c["spec"], c["w"], N, hop, center, 1, n, sgn=1)
    _run(False, c["spec"], c["w"], N, hop, center, want, "sgn +1 inverse", sgn=1)


def test_more_than_65535_frames_in_one_call():
    """3 rows of (44000, 8, 2, 0): 21997 frames per row, 65991 in the call and in one chunk, more
    than one launch's 65535 grid rows; the forward's second launch starts inside the last row"""
    n, N, hop, batch = 44000, 8, 2, 3
    assert hsfft.stft_shape(n, N, hop, 0) == (21997, 5, 0)
    c = _case(n, N, hop, 0)
    _run(True, c["x"], c["w"], N, hop, 0, c["fwd_w"], "forward, 65991 frames")
    want = S.oracle_istft_of_frames(c["v"], c["w"], N, hop, 0, 1, n)
    _run(False, c["spec"], c["w"], N, hop, 0, want, "inverse, 65991 frames")


def test_stft_in_chunks(monkeypatch):
    """5 rows of (40000, 4096, 1024, 0): 36 frames per row, 180 in all.  Forward under
    HSFFT_STFT_CHUNK_MB=1 the documented rule (bytes / (N x 8)) gives 32 frames per chunk, which
    cross row boundaries; the inverse under HSFFT_STFT_CHUNK_MB=3 (bytes / (nframes x N x 8)) walks
    two rows per chunk: chunks of 2, 2 and 1 rows"""
    n, N, hop, batch = 40000, 4096, 1024, 5
    assert hsfft.stft_shape(n, N, hop, 0) == (36, 2049, 0)
    assert T.rows_per_chunk(1, N, elem=8) == 32 and 36 % 32 != 0
    assert T.rows_per_chunk(3, 36 * N, elem=8) == 2
    c = _case(n, N, hop, 0, batch=batch)
    rf, ri = _plan(N, 1), _plan(N, -1)
    dx, dw, ds = (hsfft.DeviceBuffer.from_array(c[k]) for k in ("x", "w", "spec"))
    want_f = c["fwd_w"]
    want_i = S.oracle_istft_of_frames(c["v"], c["w"], N, hop, 0, 1, n)
    f1, f2, i1, i2 = Out(want_f.size * 2), Out(want_f.size * 2), Out(want_i.size), Out(want_i.size)
    monkeypatch.setenv("HSFFT_STFT_CHUNK_MB", "1")
    hsfft.stft_batched(rf, dx, n, dw, hop, 0, f1, batch)
    monkeypatch.setenv("HSFFT_STFT_CHUNK_MB", "3")
    hsfft.istft_batched(ri, ds, 36, dw, hop, 0, 1, i1, n, batch)
    monkeypatch.delenv("HSFFT_STFT_CHUNK_MB")
    hsfft.stft_batched(rf, dx, n, dw, hop, 0, f2, batch)
    hsfft.istft_batched(ri, ds, 36, dw, hop, 0, 1, i2, n, batch)
    hsfft.synchronize()
    diff_f = hsfft.count_diff_words(f1, f2, want_f.size * 16)
    diff_i = hsfft.count_diff_words(i1, i2, want_i.size * 8)
    got = [o.read() for o in (f1, f2, i1, i2)]
    for d in (dx, dw, ds, f1, f2, i1, i2):
        d.free()
    assert (diff_f, diff_i) == (0, 0), ("chunked differs from one chunk", diff_f, diff_i)
    for (y, guard), want, what in zip(got, (want_f, want_f, want_i, want_i),
                                      ("forward chunked", "forward one chunk", "inverse chunked", "inverse one chunk")):
        _assert_bits(y.view(want.dtype).reshape(want.shape), want, what)
        assert guard == 0, what


@pytest.mark.parametrize("n,N,hop,center", [(21, 8, 3, 0), (100, 16, 4, 1)], ids=["21_N8_hop3_c0", "100_N16_hop4_c1"])
def test_stft_on_8_byte_aligned_buffers(n, N, hop, center):
    """signal, window, spectrum and output one double past a 16-byte boundary, with sentinels in
    front of the output as well as behind: caller buffers need the alignment of a double only"""
    c = _case(n, N, hop, center)
    _run(True, c["x"], c["w"], N, hop, center, c["fwd_w"], (n, N, hop, center, "forward, lead 1"), lead=1)
    _run(True, c["x"], None, N, hop, center, c["fwd_0"], (n, N, hop, center, "forward, no window, lead 1"), lead=1)
    for nout in _lengths(c["spec"].shape[1], N, hop, center):
        for normalize in (0, 1):
            want = S.oracle_istft_of_frames(c["v"], c["w"], N, hop, center, normalize, nout)
            _run(False, c["spec"], c["w"], N, hop, center, want, (n, N, hop, center, nout, normalize, "inverse, lead 1"),
                 normalize=normalize, lead=1)


def test_special_values():
    """(1000, 64, 16, 1).  Samples 320..335 of row 0 (one hop) hold -0.0, subnormals, +-1e300, an Inf
    and a NaN together; samples 640..655 hold the finite kinds once more, where no NaN hides them;
    row 1 is dense.  The window has a -0.0 tap, so padded positions give -0.0 there.  The words
    equal the oracle's -- NaN positions compared as NaN -- and only the four frames that cover
    samples 330 and 333 (19..22) are not finite.  The inverse likewise: a special word in frame
    20's spectrum of row 0 reaches samples 288..351 and nothing else"""
    n, N, hop, center = 1000, 64, 16, 1
    x, w = S.rows(n, 2, salt=0xE7).copy(), S.window(N, salt=0xE7).copy()
    w[5] = -0.0
    for base in (320, 640):
        x[0, base + 1] = -0.0
        x[0, base + 2:base + 6] = np.array([5e-324, -3e-310, 1e-308, -2.0 ** -1040])
        x[0, base + 7] = 1e300
        x[0, base + 8] = -1e300
    x[0, 330] = np.inf
    x[0, 333] = np.nan
    want = S.oracle_stft(x, w, N, hop, center)
    hit = np.zeros(want.shape, dtype=bool)
    hit[0, 19:23] = True
    assert np.isfinite(want[~hit]).all() and T.nan_words(want[hit]).any() and np.abs(want[0, 40]).max() > 1e299
    u0 = S.frames_of(x[0], N, hop, 1)[0] * w  # frame 0 starts 32 samples before the row
    assert u0[5] == 0 and np.signbit(u0[5])
    y = _run(True, x, w, N, hop, center, want, "special values, forward", compare=_assert_bits_nan_aware)
    assert np.isfinite(y[~hit]).all()
    _run(True, x, None, N, hop, center, S.oracle_stft(x, None, N, hop, center), "special values, forward, no window",
         compare=_assert_bits_nan_aware)

    spec = S.spectra(2, 63, 33, salt=0xE7).copy()
    spec[0, 40, 2] = complex(-0.0, 5e-324)
    spec[0, 40, 4] = complex(1e300, -3e-310)
    spec[0, 40, 6] = complex(1e-308, -1e300)
    spec[0, 20, 3] = complex(np.inf, spec[0, 20, 3].imag)
    spec[0, 20, 9] = complex(spec[0, 20, 9].real, np.nan)
    v = S.oracle_scaled_frames(spec, N)
    for normalize in (0, 1):
        want = S.oracle_istft_of_frames(v, w, N, hop, center, normalize, n)
        reach = np.zeros(want.shape, dtype=bool)
        reach[0, 288:352] = True
        assert np.isfinite(want[~reach]).all() and T.nan_words(want[reach]).any()
        assert np.abs(want[0, 608:672]).max() > 1e296
        y = _run(False, spec, w, N, hop, center, want, ("special values, inverse", normalize), normalize=normalize,
                 compare=_assert_bits_nan_aware)
        assert np.isfinite(y[~reach]).all()


def test_back_to_back_calls_share_nothing_live():
    """three calls of different N -- forward, inverse (it grows the scratch), forward -- queued
    without a wait in between: the scratch is reused in stream order"""
    c1, c2, c3 = (1000, 100, 25, 1), (40000, 4096, 1024, 0), (5000, 1024, 256, 1)
    k1, k2, k3 = (_case(*c) for c in (c1, c2, c3))
    want2 = S.oracle_istft_of_frames(k2["v"], k2["w"], c2[1], c2[2], c2[3], 1, c2[0])
    wants = [k1["fwd_w"], want2, k3["fwd_w"]]
    ins = [hsfft.DeviceBuffer.from_array(a) for a in (k1["x"], k2["spec"], k3["x"])]
    wins = [hsfft.DeviceBuffer.from_array(k["w"]) for k in (k1, k2, k3)]
    outs = [Out(wants[0].size * 2), Out(wants[1].size), Out(wants[2].size * 2)]
    hsfft.stft_batched(_plan(c1[1], 1), ins[0], c1[0], wins[0], c1[2], c1[3], outs[0], 3)
    hsfft.istft_batched(_plan(c2[1], -1), ins[1], k2["spec"].shape[1], wins[1], c2[2], c2[3], 1, outs[1], c2[0], 3)
    hsfft.stft_batched(_plan(c3[1], 1), ins[2], c3[0], wins[2], c3[2], c3[3], outs[2], 3)
    hsfft.synchronize()
    got = [o.read() for o in outs]
    for d in ins + wins + outs:
        d.free()
    for c, want, (y, guard) in zip((c1, c2, c3), wants, got):
        _assert_bits(y.view(want.dtype).reshape(want.shape), want, c)
        assert guard == 0, c


def test_rejections_on_the_gpu_path():
    """real device buffers: an output that overlaps the signal, the window or the spectrum and a
    negative batch are refused, and batch == 0 returns 0 and writes nothing"""
    n, N, hop, batch = 100, 8, 4, 3
    x, w = S.rows(n, batch, salt=0xE8), S.window(N, salt=0xE8)
    spec = S.spectra(batch, 24, 5, salt=0xE8)
    dx, ds = hsfft.DeviceBuffer.from_array(x), hsfft.DeviceBuffer.from_array(spec)
    dw = hsfft.DeviceBuffer.from_array(np.concatenate([w, np.zeros(4096)]))
    rf, ri = _plan(N, 1), _plan(N, -1)
    L = hsfft.lib()
    for what, o in [("out overlaps x", hsfft.DeviceView(dx, 8 * (batch * n - 1))), ("out == x", dx), ("out == w", dw),
                    ("out overlaps w", hsfft.DeviceView(dw, 8 * (N - 1)))]:
        with pytest.raises(hsfft.HsfftError, match="overlaps"):
            hsfft.stft_batched(rf, dx, n, dw, hop, 0, o, batch)
    for what, o in [("out overlaps spec", hsfft.DeviceView(ds, 16 * (batch * 24 * 5) - 8)), ("out == spec", ds),
                    ("out == w", dw), ("out overlaps w", hsfft.DeviceView(dw, 8 * (N - 1)))]:
        with pytest.raises(hsfft.HsfftError, match="overlaps"):
            hsfft.istft_batched(ri, ds, 24, dw, hop, 0, 1, o, n, batch)
    fo, io = Out(batch * 24 * 5 * 2), Out(batch * n)
    assert L.hsfft_stft_batched(rf.ptr, dx.ptr, n, dw.ptr, hop, 0, fo.ptr, -1) == hsfft.HSFFT_ERR_ARG
    assert L.hsfft_last_error()
    assert L.hsfft_istft_batched(ri.ptr, ds.ptr, 24, dw.ptr, hop, 0, 1, io.ptr, n, -1) == hsfft.HSFFT_ERR_ARG
    assert L.hsfft_last_error()
    assert L.hsfft_stft_batched(rf.ptr, dx.ptr, n, dw.ptr, hop, 0, fo.ptr, 0) == 0
    assert L.hsfft_istft_batched(ri.ptr, ds.ptr, 24, dw.ptr, hop, 0, 1, io.ptr, n, 0) == 0
    hsfft.synchronize()
    (yf, gf), (yi, gi) = fo.read(), io.read()
    xin, win, sin = dx.to_array(np.float64), dw.to_array(np.float64, count=N), ds.to_array(np.complex128)
    for d in (dx, dw, ds, fo, io):
        d.free()
    assert T.nan_words(yf).all() and T.nan_words(yi).all() and (gf, gi) == (0, 0)  # nothing was written
    _assert_bits(xin.reshape(x.shape), x, "x changed")
    _assert_bits(win, w, "w changed")
    _assert_bits(sin.reshape(spec.shape), spec, "spec changed")


def test_stft_conveniences():
    n, N, hop = 1000, 100, 25
    c = _case(n, N, hop, 1)
    y = hsfft.stft(c["x"][0], N, hop, window=c["w"], center=True)
    assert y.shape == (41, 51) and y.dtype == np.complex128
    _assert_bits(y, c["fwd_w"][0], "stft, 1-D input")
    y = hsfft.stft(c["x"], N, hop, center=True)
    assert y.shape == (3, 41, 51)
    _assert_bits(y, c["fwd_0"], "stft, 2-D input, no window")
    natural = S.natural_length(41, N, hop, 1)
    assert natural == n
    z = hsfft.istft(c["spec"][0], hop, window=c["w"], center=True)
    assert z.shape == (n,) and z.dtype == np.float64
    _assert_bits(z, S.oracle_istft_of_frames(c["v"][0], c["w"], N, hop, 1, 1, n), "istft, 1-D input")
    z = hsfft.istft(c["spec"], hop, center=True, normalize=False, length=n + 7)
    assert z.shape == (3, n + 7)
    _assert_bits(z, S.oracle_istft_of_frames(c["v"], None, N, hop, 1, 0, n + 7), "istft, 2-D input, no window, longer")
    c = _case(21, 8, 3, 0)
    z = hsfft.istft(c["spec"], 3, window=c["w"])
    assert z.shape == (3, 20)  # 5 frames: (5 - 1) x 3 + 8
    _assert_bits(z, S.oracle_istft_of_frames(c["v"], c["w"], 8, 3, 0, 1, 20), "istft, not centred")


def test_hann_round_trip_returns_the_signal():
    """periodic Hann, N 64, hop 16, centred, normalised, n 1000: the inverse of the forward returns
    x within 4 x the error of the reference's own r2c -> c2r -> / N round trip on the same frames,
    the bound test_stft_cpu.py measures the expectation against (measured there: 4.44e-16 against
    5.55e-16)"""
    x, w, err_oracle, ref = S.round_trip_errors()
    back = hsfft.istft(hsfft.stft(x, 64, 16, window=w, center=True), 16, window=w, center=True, length=1000)
    err = float(np.abs(back - x).max())
    print("round trip error on the GPU", err, "of the expectation", err_oracle, "reference round trip", ref)
    assert err <= 4 * ref, (err, ref)
