"""Expected values of the batched STFT and its inverse (hsfft_stft_shape, hsfft_stft_batched,
hsfft_istft_batched), from the pinned 1D oracle and numpy alone.  Forward: numpy builds the padded
frames and multiplies them by the window in float64 (one IEEE multiply per word, at padded
positions too), and every frame goes through T.oracle_r2c -- the reference's own fft_r2c_exec --
with bins 0..N/2 kept.  Inverse: every frame goes through the oracle's c2r -- the reference's
fft_c2r_exec, which reads bins 0..N/2 --, is divided by float(N) and multiplied by the window, and a
Python loop over the frames in increasing f adds each frame's terms to the samples it covers, the
first term of a sample stored, not added to 0.0; the envelope likewise.  test_stft_cpu.py checks
this composition against numpy.fft and as a round trip."""
import numpy as np

import hsfft_testlib as T

MAX_LEN = 1 << 30  # the header's bound on n and N


def shape_rule(n, N, hop, center):
    """(nframes, bins, lpad), or None where the library must reject the call"""
    if N < 2 or N % 2 or N > MAX_LEN or hop < 1 or n < 1 or n > MAX_LEN or center not in (0, 1):
        return None
    if not center and n < N:
        return None
    return (1 + n // hop if center else 1 + (n - N) // hop), N // 2 + 1, (N // 2 if center else 0)


def natural_length(nframes, N, hop, center):
    """the samples of the row that nframes frames cover: (nframes - 1) hop + N - 2 lpad"""
    return (nframes - 1) * hop + N - (N if center else 0)


def frames_of(x, N, hop, center):
    """the padded frames (nframes, N) of one row: position f hop - lpad + j, +0.0 outside [0, n)"""
    n = x.size
    nframes, _, lpad = shape_rule(n, N, hop, center)
    p = (np.arange(nframes, dtype=np.int64) * hop - lpad)[:, None] + np.arange(N, dtype=np.int64)[None, :]
    inside = (p >= 0) & (p < n)
    return np.where(inside, x[np.clip(p, 0, n - 1)], 0.0)


def oracle_stft(x, w, N, hop, center, sgn=1):
    """expected spectra of x, of shape (n,) or (batch, n): (nframes, N/2+1) or (batch, nframes, N/2+1)"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        return np.stack([oracle_stft(r, w, N, hop, center, sgn) for r in x])
    u = frames_of(x, N, hop, center)
    if w is not None:
        u = u * np.asarray(w, dtype=np.float64)[None, :]
    return np.ascontiguousarray(T.oracle_r2c(np.ascontiguousarray(u), sgn)[:, :N // 2 + 1])


def oracle_c2r_frames(S, N, sgn=-1):
    """the reference's c2r of every row of S (nframes, N/2+1): (nframes, N), unscaled"""
    lib = T.oracle()
    S = np.ascontiguousarray(S, dtype=np.complex128)
    X = np.zeros(N, dtype=np.complex128)
    y = np.zeros((S.shape[0], N))
    rp = lib.orc_real_create(N, sgn, 0)
    for f in range(S.shape[0]):
        X[:N // 2 + 1] = S[f]
        lib.orc_c2r(rp, T.ptr(X), T.ptr(y[f]))
    lib.orc_real_destroy(rp)
    return y


def overlap_add(t, e, N, hop, center, normalize, n):
    """the samples 0..n-1 from the frames' terms t (nframes, N) and envelope terms e (N,): frames in
    increasing f, a sample's first term stored and every later one added, one add each"""
    lpad = N // 2 if center else 0
    acc, env, seen = np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)
    for f in range(t.shape[0]):
        start = f * hop - lpad
        lo, hi = max(0, start), min(n, start + N)
        if lo >= hi:
            continue
        tt, ee, s = t[f, lo - start:hi - start], e[lo - start:hi - start], seen[lo:hi]
        acc[lo:hi] = np.where(s, acc[lo:hi] + tt, tt)
        env[lo:hi] = np.where(s, env[lo:hi] + ee, ee)
        seen[lo:hi] = True
    if normalize:
        with np.errstate(all="ignore"):
            acc = np.where(seen, acc / np.where(seen, env, 1.0), 0.0)
    return acc


def oracle_scaled_frames(S, N, sgn=-1):
    """v_f = the reference's c2r of every frame of S (..., nframes, N/2+1), divided by float(N):
    (..., nframes, N).  The costly half of the inverse, shared by every window, mode and length"""
    S = np.asarray(S, dtype=np.complex128)
    if S.ndim == 3:
        return np.stack([oracle_scaled_frames(r, N, sgn) for r in S])
    assert S.shape[1] == N // 2 + 1
    with np.errstate(all="ignore"):
        return oracle_c2r_frames(S, N, sgn) / float(N)


def oracle_istft_of_frames(v, w, N, hop, center, normalize, n):
    """expected rows of n samples from the scaled frames v (..., nframes, N): one multiply by the
    window, then the overlap-add"""
    if v.ndim == 3:
        return np.stack([oracle_istft_of_frames(r, w, N, hop, center, normalize, n) for r in v])
    with np.errstate(all="ignore"):
        if w is not None:
            w = np.asarray(w, dtype=np.float64)
            t, e = v * w[None, :], w * w
        else:
            t, e = v, np.ones(N)
        return overlap_add(t, e, N, hop, center, normalize, n)


def oracle_istft(S, w, N, hop, center, normalize, n, sgn=-1):
    """expected rows of n samples from S of shape (nframes, N/2+1) or (batch, nframes, N/2+1)"""
    return oracle_istft_of_frames(oracle_scaled_frames(S, N, sgn), w, N, hop, center, normalize, n)


def rows(n, batch, salt=0):
    """batch dense real rows (batch, n) from the suite's generator"""
    return T.real_input(n, T.seed_for(n) ^ salt ^ 0x57F7, batch=batch).reshape(batch, n)


def window(N, salt=0):
    """a dense random window: no tap is zero, so the envelope never vanishes where a frame covers"""
    return T.real_input(N, T.seed_for(N) ^ salt ^ 0x3D)


def hann(N):
    """the periodic Hann window"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)


def spectra(batch, nframes, bins, salt=0):
    """dense random spectra (batch, nframes, bins), not Hermitian-consistent"""
    return T.complex_input(nframes * bins, T.seed_for(nframes * bins) ^ salt ^ 0x1F7, batch=batch).reshape(batch, nframes, bins)


def round_trip_errors():
    """(x, w, largest error of oracle_istft(oracle_stft(x)) against x, largest error of the reference's own
    r2c -> c2r -> / N round trip on the same frames unwindowed) for the periodic Hann window, N 64,
    hop 16, centred, normalised, n 1000; test_gpu_stft.py bounds the conveniences' round trip by the
    same figures"""
    n, N, hop = 1000, 64, 16
    x, w = rows(n, 1, salt=0xC3)[0], hann(N)
    back = oracle_istft(oracle_stft(x, w, N, hop, 1), w, N, hop, 1, 1, n)
    u = frames_of(x, N, hop, 1)
    rt = oracle_c2r_frames(T.oracle_r2c(np.ascontiguousarray(u))[:, :N // 2 + 1], N) / float(N)
    return x, w, float(np.abs(back - x).max()), float(np.abs(rt - u).max())
