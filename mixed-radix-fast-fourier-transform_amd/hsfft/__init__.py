"""hsfft -- Python (ctypes) binding of libhsfft.so, the MI355X drop-in for highSpeedFFT.

The product is the C-ABI library lib/libhsfft.so (include/highspeedFFT.h, include/real.h,
include/hsfft_gpu.h).  This module only binds it for tests and bench.py; it contains no
compute.  Loading fails loudly if the library was not built (run __graft_entry__.build()
or `make -C mixed-radix-fast-fourier-transform_amd`).
"""
import ctypes
import os

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("HSFFT_LIB_PATH") or os.path.join(PKG_ROOT, "lib", "libhsfft.so")

VP = ctypes.c_void_p
CI = ctypes.c_int

# public symbols of include/*.h with their ctypes signatures (tests check every one exists)
SIGNATURES = {
    # highspeedFFT.h
    "fft_init": (VP, [CI, CI]),
    "fft_exec": (None, [VP, VP, VP]),
    "divideby": (CI, [CI, CI]),
    "dividebyN": (CI, [CI]),
    "factors": (CI, [CI, VP]),
    "twiddle": (None, [VP, CI, CI]),
    "longvectorN": (None, [VP, CI, VP, CI]),
    "free_fft": (None, [VP]),
    # real.h
    "fft_real_init": (VP, [CI, CI]),
    "fft_r2c_exec": (None, [VP, VP, VP]),
    "fft_c2r_exec": (None, [VP, VP, VP]),
    "free_real_fft": (None, [VP]),
    "fft_convolve": (CI, [ctypes.c_char_p, ctypes.c_char_p, VP, CI, VP, CI, VP]),
    "next_power_of_two": (CI, [CI]),
    "find_optimal_fft_length": (CI, [CI, ctypes.c_char_p, CI, CI]),
    # hsfft_gpu.h
    "hsfft_device_count": (CI, []),
    "hsfft_set_device": (CI, [CI]),
    "hsfft_get_device": (CI, []),
    "hsfft_malloc": (VP, [ctypes.c_size_t]),
    "hsfft_free": (CI, [VP]),
    "hsfft_memcpy_h2d": (CI, [VP, VP, ctypes.c_size_t]),
    "hsfft_memcpy_d2h": (CI, [VP, VP, ctypes.c_size_t]),
    "hsfft_memset": (CI, [VP, CI, ctypes.c_size_t]),
    "hsfft_synchronize": (CI, []),
    "hsfft_release_scratch": (CI, []),
    "hsfft_finalize": (CI, []),
    "hsfft_get_stream": (VP, []),
    "hsfft_last_error": (ctypes.c_char_p, []),
    "hsfft_set_twiddle_mode": (CI, [CI]),
    "hsfft_get_twiddle_mode": (CI, []),
    "hsfft_plan_refresh": (CI, [VP]),
    "hsfft_plan_num_passes": (CI, [VP]),
    "hsfft_digit_reverse_map": (CI, [VP, VP]),
    "hsfft_exec_batched": (CI, [VP, VP, VP, CI]),
    "hsfft_exec_batched_host": (CI, [VP, VP, VP, CI]),
    "hsfft_r2c_batched": (CI, [VP, VP, VP, CI]),
    "hsfft_r2c_batched_compact": (CI, [VP, VP, VP, CI]),
    "hsfft_c2r_batched": (CI, [VP, VP, VP, CI]),
    "hsfft_convolve_batched": (CI, [ctypes.c_char_p, ctypes.c_char_p, VP, CI, VP, CI, VP, CI]),
    "hsfft_transpose_batched": (CI, [VP, VP, CI, CI, CI]),
    "hsfft_exec_2d": (CI, [VP, VP, VP, VP, CI]),
    "hsfft_exec_columns": (CI, [VP, VP, VP, CI, CI]),
    "hsfft_r2c_2d": (CI, [VP, VP, VP, VP, CI]),
    "hsfft_r2c_2d_full": (CI, [VP, VP, VP, VP, CI]),
    "hsfft_c2r_2d": (CI, [VP, VP, VP, VP, CI]),
    "hsfft_convolve_2d_shape": (CI, [ctypes.c_char_p, ctypes.c_char_p, CI, CI, CI, CI, ctypes.POINTER(CI),
                                     ctypes.POINTER(CI), ctypes.POINTER(CI), ctypes.POINTER(CI)]),
    "hsfft_convolve_2d_batched": (CI, [ctypes.c_char_p, ctypes.c_char_p, VP, CI, CI, VP, CI, CI, CI, VP, CI]),
    "hsfft_filter_shape": (CI, [ctypes.c_char_p, CI, CI, CI, ctypes.POINTER(CI), ctypes.POINTER(CI), ctypes.POINTER(CI),
                                ctypes.POINTER(CI)]),
    "hsfft_filter_batched": (CI, [ctypes.c_char_p, VP, CI, VP, CI, CI, VP, CI]),
    "hsfft_stft_shape": (CI, [CI, CI, CI, CI, ctypes.POINTER(CI), ctypes.POINTER(CI), ctypes.POINTER(CI)]),
    "hsfft_stft_batched": (CI, [VP, VP, CI, VP, CI, CI, VP, CI]),
    "hsfft_istft_batched": (CI, [VP, VP, CI, VP, CI, CI, CI, VP, CI, CI]),
    "hsfft_dct_twiddles": (CI, [CI, VP]),
    "hsfft_dct_batched": (CI, [CI, CI, VP, VP, CI, CI]),
    "hsfft_transpose_real_batched": (CI, [VP, VP, CI, CI, CI]),
    "hsfft_dct_2d_batched": (CI, [CI, CI, CI, VP, VP, CI, CI, CI]),
    "hsfft_dct4_twiddles": (CI, [CI, VP]),
    "hsfft_dct4_batched": (CI, [CI, VP, VP, CI, CI]),
    "hsfft_dct1_shape": (CI, [CI, CI, ctypes.POINTER(CI), ctypes.POINTER(CI)]),
    "hsfft_dct1_batched": (CI, [CI, VP, VP, CI, CI]),
    "hsfft_dct1_2d_batched": (CI, [CI, CI, VP, VP, CI, CI, CI]),
    "hsfft_mdct_shape": (CI, [CI, CI, CI, ctypes.POINTER(CI), ctypes.POINTER(CI)]),
    "hsfft_mdct_batched": (CI, [VP, CI, VP, CI, CI, VP, CI]),
    "hsfft_imdct_batched": (CI, [VP, CI, VP, CI, CI, VP, CI, CI]),
    "hsfft_czt_shape": (CI, [CI, CI, ctypes.POINTER(CI)]),
    "hsfft_czt_tables": (CI, [CI, CI, ctypes.c_double, ctypes.c_double, VP, VP]),
    "hsfft_czt_batched": (CI, [VP, CI, VP, CI, ctypes.c_double, ctypes.c_double, CI]),
    "hsfft_czt_real_batched": (CI, [VP, CI, VP, CI, ctypes.c_double, ctypes.c_double, CI]),
    "hsfft_hilbert_batched": (CI, [VP, VP, CI, CI]),
    "hsfft_resample_batched": (CI, [VP, CI, VP, CI, CI]),
    "hsfft_spectral_chunk_rows": (CI, [CI, CI, ctypes.POINTER(ctypes.c_longlong)]),
    "hsfft_fill_complex": (CI, [VP, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64]),
    "hsfft_fill_real": (CI, [VP, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64]),
    "hsfft_time_batched": (CI, [VP, VP, VP, CI, CI, ctypes.POINTER(ctypes.c_float),
                                ctypes.POINTER(ctypes.c_float), CI]),
    "hsfft_time_r2c_batched": (CI, [VP, VP, VP, CI, CI, ctypes.POINTER(ctypes.c_float)]),
    "hsfft_time_exec_host": (CI, [VP, VP, VP, CI, CI, CI, ctypes.POINTER(ctypes.c_double)]),
    "hsfft_exec_multi": (CI, [VP, VP, VP, CI, CI]),
    "hsfft_bench_copy": (CI, [VP, VP, ctypes.c_size_t, CI, ctypes.POINTER(ctypes.c_float)]),
    "hsfft_bench_transpose_herm": (CI, [VP, VP, CI, CI, CI, CI, ctypes.POINTER(ctypes.c_float)]),
    "hsfft_bluestein_fallbacks": (ctypes.c_longlong, []),
    "hsfft_thread_streams_created": (ctypes.c_longlong, []),
    "hsfft_count_diff_words": (CI, [VP, VP, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]),
}

HSFFT_ERR_ARG, HSFFT_ERR_DEVICE, HSFFT_ERR_NOMEM = -1, -2, -3  # include/hsfft_gpu.h

STRUCT_TWIDDLE_OFFSET = 272  # offsetof(struct fft_set, twiddle), include/highspeedFFT.h

_lib = None


class HsfftError(RuntimeError):
    pass


def lib():
    """Load lib/libhsfft.so once and bind every public symbol."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HsfftError(f"{LIB_PATH} not built: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(VP) if isinstance(a, np.ndarray) else VP(a)


def check(rc, what="hsfft"):
    if rc < 0:
        raise HsfftError(f"{what} failed ({rc}): {lib().hsfft_last_error().decode()}")
    return rc


def device_count():
    return lib().hsfft_device_count()


class Plan:
    """fft_object wrapper (fft_init / free_fft)."""

    def __init__(self, n, sgn=1):
        self.n, self.sgn = n, sgn
        self.ptr = lib().fft_init(n, sgn)
        if not self.ptr:
            raise HsfftError(f"fft_init({n}, {sgn}) returned NULL")

    def header(self):
        hdr = (ctypes.c_int * 68).from_address(self.ptr)
        lf = hdr[66]
        return dict(N=hdr[0], sgn=hdr[1], factors=[hdr[2 + i] for i in range(lf)], lf=lf, lt=hdr[67])

    def twiddles(self):
        h = self.header()
        m = int(np.prod(h["factors"])) if h["factors"] else 1
        n = max(m - 1, 0)
        raw = (ctypes.c_double * (2 * n)).from_address(self.ptr + STRUCT_TWIDDLE_OFFSET)
        return np.frombuffer(bytes(raw), dtype=np.complex128).copy()

    def num_passes(self):
        return check(lib().hsfft_plan_num_passes(self.ptr), "num_passes")

    def exec(self, x, out=None):
        """drop-in fft_exec on host numpy arrays (staged through HBM)."""
        x = np.ascontiguousarray(x, dtype=np.complex128)
        y = np.zeros_like(x) if out is None else out
        lib().fft_exec(self.ptr, _ptr(x), _ptr(y))
        return y

    def close(self):
        if self.ptr:
            lib().free_fft(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RealPlan:
    def __init__(self, n, sgn=1):
        self.n, self.sgn = n, sgn
        self.ptr = lib().fft_real_init(n, sgn)
        if not self.ptr:
            raise HsfftError("fft_real_init failed")

    def r2c(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros(self.n, dtype=np.complex128)
        lib().fft_r2c_exec(self.ptr, _ptr(x), _ptr(y))
        return y

    def c2r(self, X):
        X = np.ascontiguousarray(X, dtype=np.complex128)
        y = np.zeros(self.n, dtype=np.float64)
        lib().fft_c2r_exec(self.ptr, _ptr(X), _ptr(y))
        return y

    def close(self):
        if self.ptr:
            lib().free_real_fft(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """HBM allocation through hsfft_malloc (no torch involved)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = lib().hsfft_malloc(self.nbytes)
        if not self.ptr:
            raise HsfftError(f"hsfft_malloc({self.nbytes}) failed: {lib().hsfft_last_error().decode()}")

    @classmethod
    def from_array(cls, a):
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        check(lib().hsfft_memcpy_h2d(b.ptr, _ptr(a), a.nbytes), "h2d")
        return b

    def to_array(self, dtype, count=None, offset_bytes=0):
        dt = np.dtype(dtype)
        count = (self.nbytes - offset_bytes) // dt.itemsize if count is None else count
        out = np.empty(count, dtype=dt)
        check(lib().hsfft_memcpy_d2h(_ptr(out), VP(self.ptr + offset_bytes), out.nbytes), "d2h")
        return out

    def fill_zero(self):
        check(lib().hsfft_memset(self.ptr, 0, self.nbytes), "memset")

    def free(self):
        if self.ptr:
            lib().hsfft_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceView:
    """a byte offset into a DeviceBuffer (not owning; never freed)"""

    def __init__(self, buf, offset_bytes):
        self.ptr = buf.ptr + int(offset_bytes)
        self.nbytes = buf.nbytes - int(offset_bytes)


def exec_batched(plan, d_in, d_out, batch):
    return check(lib().hsfft_exec_batched(plan.ptr, VP(d_in.ptr), VP(d_out.ptr), batch), "exec_batched")


def exec_batched_host(plan, x, out=None):
    """c2c of host rows x (batch, N) complex128 through hsfft_exec_batched_host"""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    out = np.empty_like(x) if out is None else out
    batch = x.shape[0] if x.ndim == 2 else 1
    check(lib().hsfft_exec_batched_host(plan.ptr, _ptr(x), _ptr(out), batch), "exec_batched_host")
    return out


def transpose_batched(d_in, d_out, rows, cols, batch):
    """out[b][c][r] = in[b][r][c] for batch matrices of rows x cols 16-byte elements"""
    return check(lib().hsfft_transpose_batched(VP(d_in.ptr), VP(d_out.ptr), rows, cols, batch), "transpose_batched")


def exec_2d(plan0, plan1, d_in, d_out, batch):
    """2D c2c of batch images of plan0.n rows x plan1.n columns: plan1 on the rows, then plan0 on the columns"""
    return check(lib().hsfft_exec_2d(plan0.ptr, plan1.ptr, VP(d_in.ptr), VP(d_out.ptr), batch), "exec_2d")


def exec_columns(plan, d_in, d_out, ncols, batch):
    """c2c along axis 0 of batch matrices of plan.n rows x ncols columns"""
    return check(lib().hsfft_exec_columns(plan.ptr, VP(d_in.ptr), VP(d_out.ptr), ncols, batch), "exec_columns")


def fft2(x, sgn=1):
    """2D c2c over the last two axes of a complex128 array of shape (..., n0, n1), unscaled:
    plans, uploads, runs hsfft_exec_2d and downloads"""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    if x.ndim < 2:
        raise ValueError("fft2 needs an array of at least two dimensions")
    n0, n1 = x.shape[-2:]
    if x.size == 0:
        return np.empty_like(x)
    batch = x.size // (n0 * n1)
    made = []
    try:
        p0 = Plan(n0, sgn)
        made.append(p0.close)
        p1 = p0 if n1 == n0 else Plan(n1, sgn)
        made.append(p1.close)
        d_in = DeviceBuffer.from_array(x)
        made.append(d_in.free)
        d_out = DeviceBuffer(x.nbytes)
        made.append(d_out.free)
        exec_2d(p0, p1, d_in, d_out, batch)
        synchronize()
        return d_out.to_array(np.complex128).reshape(x.shape)
    finally:
        for release in reversed(made):
            release()


def r2c_2d(plan0, rplan1, d_in, d_out, batch):
    """batch real images of plan0.n x rplan1.n -> half spectra of plan0.n x (rplan1.n/2+1): r2c of
    rplan1 on the rows, then plan0 on the columns"""
    return check(lib().hsfft_r2c_2d(plan0.ptr, rplan1.ptr, VP(d_in.ptr), VP(d_out.ptr), batch), "r2c_2d")


def r2c_2d_full(plan0, rplan1, d_in, d_out, batch):
    """the same transform in the full layout, plan0.n x rplan1.n complex per image (mirror half included)"""
    return check(lib().hsfft_r2c_2d_full(plan0.ptr, rplan1.ptr, VP(d_in.ptr), VP(d_out.ptr), batch), "r2c_2d_full")


def c2r_2d(plan0, rplan1, d_in, d_out, batch):
    """batch half spectra of plan0.n x (rplan1.n/2+1) -> real images of plan0.n x rplan1.n: plan0 on
    the columns, then c2r of rplan1 on the rows"""
    return check(lib().hsfft_c2r_2d(plan0.ptr, rplan1.ptr, VP(d_in.ptr), VP(d_out.ptr), batch), "c2r_2d")


def _real_2d(call, x, n0, n1, sgn, out_dtype, out_shape):
    """plan (n0, n1, sgn), upload x, run call(p0, r1, d_in, d_out, batch), download"""
    batch = x.size // (x.shape[-2] * x.shape[-1])
    out_bytes = int(np.prod(out_shape)) * np.dtype(out_dtype).itemsize
    made = []
    try:
        p0 = Plan(n0, sgn)
        made.append(p0.close)
        r1 = RealPlan(n1, sgn)
        made.append(r1.close)
        d_in = DeviceBuffer.from_array(x)
        made.append(d_in.free)
        d_out = DeviceBuffer(out_bytes)
        made.append(d_out.free)
        call(p0, r1, d_in, d_out, batch)
        synchronize()
        return d_out.to_array(out_dtype).reshape(out_shape)
    finally:
        for release in reversed(made):
            release()


def rfft2(x, sgn=1, full=False):
    """2D r2c over the last two axes of a float64 array of shape (..., n0, n1), n1 even, unscaled:
    the half spectrum (..., n0, n1/2+1), or with full=True the full layout (..., n0, n1); plans,
    uploads, runs hsfft_r2c_2d / hsfft_r2c_2d_full and downloads"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim < 2:
        raise ValueError("rfft2 needs an array of at least two dimensions")
    n0, n1 = x.shape[-2:]
    if n1 % 2:
        raise ValueError("rfft2 needs an even last axis")
    shape = x.shape[:-1] + (n1 if full else n1 // 2 + 1,)
    if x.size == 0:
        return np.empty(shape, dtype=np.complex128)
    return _real_2d(r2c_2d_full if full else r2c_2d, x, n0, n1, sgn, np.complex128, shape)


def irfft2(X, n1, sgn=-1):
    """2D c2r over the last two axes of a complex128 array of half spectra (..., n0, n1/2+1),
    unscaled: real images (..., n0, n1); plans, uploads, runs hsfft_c2r_2d and downloads"""
    X = np.ascontiguousarray(X, dtype=np.complex128)
    if X.ndim < 2:
        raise ValueError("irfft2 needs an array of at least two dimensions")
    if n1 < 2 or n1 % 2 or X.shape[-1] != n1 // 2 + 1:
        raise ValueError("irfft2 needs an even n1 and a last axis of n1/2+1 bins")
    shape = X.shape[:-1] + (n1,)
    if X.size == 0:
        return np.empty(shape, dtype=np.float64)
    return _real_2d(c2r_2d, X, X.shape[-2], n1, sgn, np.float64, shape)


def _name(s):
    return s.encode() if isinstance(s, str) else s


def convolve_2d_shape(mode, boundary, a_rows, a_cols, b_rows, b_cols):
    """(out_rows, out_cols, pad_rows, pad_cols) of hsfft_convolve_2d_batched: sizes only, no device touched"""
    v = [CI(0) for _ in range(4)]
    check(lib().hsfft_convolve_2d_shape(_name(mode), _name(boundary), a_rows, a_cols, b_rows, b_cols,
                                        *(ctypes.byref(x) for x in v)), "convolve_2d_shape")
    return tuple(x.value for x in v)


def convolve_2d_batched(mode, boundary, d_a, a_rows, a_cols, d_b, b_rows, b_cols, b_batch, d_out, batch):
    """batch real images a_rows x a_cols convolved with b_batch (batch or 1) images b_rows x b_cols
    into batch images of the size convolve_2d_shape gives; mode full | same | valid, boundary
    linear | circular"""
    return check(lib().hsfft_convolve_2d_batched(_name(mode), _name(boundary), VP(d_a.ptr), a_rows, a_cols, VP(d_b.ptr),
                                                 b_rows, b_cols, b_batch, VP(d_out.ptr), batch), "convolve_2d_batched")


_CONV_MODES, _CONV_BOUNDARIES = ("full", "same", "valid"), ("linear", "circular")


def _conv_axis(mode, boundary, n, m):
    """window length of one axis by the library's rule (hsfft_convolve_2d_shape), for shape checks
    that must not load the library"""
    if boundary == "circular":
        return 1 << (max(n, m) - 1).bit_length()
    return {"full": n + m - 1, "same": max(n, m), "valid": max(n, m) - min(n, m) + 1}[mode]


def convolve2d(a, b, mode="full", boundary="linear"):
    """2D convolution over the last two axes of float64 arrays: a of shape (..., rows, cols), b with
    the same leading shape or a single 2D kernel shared by every image; uploads, runs
    hsfft_convolve_2d_batched and downloads.  The output size follows the library's per-axis rule:
    full / same / valid windows for boundary="linear", the whole power-of-two padded image for
    "circular"."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if mode not in _CONV_MODES or boundary not in _CONV_BOUNDARIES:
        raise ValueError(f"convolve2d: mode is one of {_CONV_MODES}, boundary one of {_CONV_BOUNDARIES}")
    if a.ndim < 2 or b.ndim < 2:
        raise ValueError("convolve2d needs arrays of at least two dimensions")
    if b.ndim != 2 and b.shape[:-2] != a.shape[:-2]:
        raise ValueError("convolve2d: b is one 2D kernel or has a's leading shape")
    (ar, ac), (br, bc) = a.shape[-2:], b.shape[-2:]
    if min(ar, ac, br, bc) < 1:
        raise ValueError("convolve2d: empty image")
    if ac == 1 and bc == 1:
        raise ValueError("convolve2d: both widths are 1 (no real transform of length 1)")
    shape = a.shape[:-2] + (_conv_axis(mode, boundary, ar, br), _conv_axis(mode, boundary, ac, bc))
    if a.size == 0:
        return np.empty(shape, dtype=np.float64)
    batch = a.size // (ar * ac)
    b_batch = batch if b.ndim != 2 else 1
    if tuple(shape[-2:]) != convolve_2d_shape(mode, boundary, ar, ac, br, bc)[:2]:
        raise HsfftError("convolve2d: the library's output shape differs from the binding's")
    made = []
    try:
        d_a = DeviceBuffer.from_array(a)
        made.append(d_a.free)
        d_b = DeviceBuffer.from_array(b)
        made.append(d_b.free)
        d_out = DeviceBuffer(int(np.prod(shape)) * 8)
        made.append(d_out.free)
        convolve_2d_batched(mode, boundary, d_a, ar, ac, d_b, br, bc, b_batch, d_out, batch)
        synchronize()
        return d_out.to_array(np.float64).reshape(shape)
    finally:
        for release in reversed(made):
            release()


def filter_shape(mode, n, m, block=0):
    """(out_len, P, L, nseg) of hsfft_filter_batched: sizes only, no device touched; block 0 is automatic"""
    v = [CI(0) for _ in range(4)]
    check(lib().hsfft_filter_shape(_name(mode), n, m, block, *(ctypes.byref(x) for x in v)), "filter_shape")
    return tuple(x.value for x in v)


def filter_batched(mode, d_x, n, d_h, m, block, d_out, batch):
    """batch real rows of n samples filtered by one kernel of m taps, by overlap-add with blocks
    padded to `block` (0: automatic), into batch rows of the length filter_shape gives; mode
    full | same | valid"""
    return check(lib().hsfft_filter_batched(_name(mode), VP(d_x.ptr), n, VP(d_h.ptr), m, block, VP(d_out.ptr), batch),
                 "filter_batched")


def oaconvolve(x, h, mode="full", block=0):
    """linear convolution of the float64 rows x, of shape (n,) or (batch, n), with one 1-D kernel h
    by overlap-add: uploads, runs hsfft_filter_batched and downloads"""
    x, h = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(h, dtype=np.float64)
    if mode not in _CONV_MODES:
        raise ValueError(f"oaconvolve: mode is one of {_CONV_MODES}")
    if x.ndim not in (1, 2) or h.ndim != 1:
        raise ValueError("oaconvolve needs x of one or two dimensions and a one-dimensional kernel")
    n, m = x.shape[-1], h.shape[0]
    if n < 1 or m < 1:
        raise ValueError("oaconvolve: empty row or kernel")
    if block < 0 or (block and (block & (block - 1) or block < 2 or block < m)):
        raise ValueError("oaconvolve: block is 0 or a power of two >= 2 and >= the kernel length")
    shape = x.shape[:-1] + (_conv_axis(mode, "linear", n, m),)
    if x.size == 0:
        return np.empty(shape, dtype=np.float64)
    batch = x.size // n
    if shape[-1] != filter_shape(mode, n, m, block)[0]:
        raise HsfftError("oaconvolve: the library's output length differs from the binding's")
    made = []
    try:
        d_x = DeviceBuffer.from_array(x)
        made.append(d_x.free)
        d_h = DeviceBuffer.from_array(h)
        made.append(d_h.free)
        d_out = DeviceBuffer(int(np.prod(shape)) * 8)
        made.append(d_out.free)
        filter_batched(mode, d_x, n, d_h, m, block, d_out, batch)
        synchronize()
        return d_out.to_array(np.float64).reshape(shape)
    finally:
        for release in reversed(made):
            release()


def stft_shape(n, n_fft, hop, center=False):
    """(nframes, bins, lpad) of hsfft_stft_batched: sizes only, no device touched"""
    v = [CI(0) for _ in range(3)]
    check(lib().hsfft_stft_shape(n, n_fft, hop, int(center), *(ctypes.byref(x) for x in v)), "stft_shape")
    return tuple(x.value for x in v)


def _opt_ptr(d):
    return VP(d.ptr) if d is not None else None


def stft_batched(rplan, d_x, n, d_w, hop, center, d_out, batch):
    """batch real rows of n samples -> batch x nframes x (rplan.n/2+1) complex: frames of rplan.n
    samples `hop` apart, times the window d_w (None: no window), through the r2c of rplan"""
    return check(lib().hsfft_stft_batched(rplan.ptr, VP(d_x.ptr), n, _opt_ptr(d_w), hop, int(center), VP(d_out.ptr), batch),
                 "stft_batched")


def istft_batched(rplan, d_spec, nframes, d_w, hop, center, normalize, d_out, n, batch):
    """batch x nframes x (rplan.n/2+1) complex -> batch real rows of n samples: c2r of rplan on
    every frame, / rplan.n, times the window, overlap-added; normalize divides by the summed
    squared window"""
    return check(lib().hsfft_istft_batched(rplan.ptr, VP(d_spec.ptr), nframes, _opt_ptr(d_w), hop, int(center),
                                           int(normalize), VP(d_out.ptr), n, batch), "istft_batched")


def _stft_window(who, window, n_fft):
    if window is None:
        return None
    window = np.ascontiguousarray(window, dtype=np.float64)
    if window.shape != (n_fft,):
        raise ValueError(f"{who}: the window is one-dimensional, n_fft = {n_fft} long")
    return window


def _stft_run(call, plan_args, x, window, out_dtype, out_shape):
    """plan, upload x and the window, run call(plan, d_x, d_w, d_out), download"""
    made = []
    try:
        rp = RealPlan(*plan_args)
        made.append(rp.close)
        d_x = DeviceBuffer.from_array(x)
        made.append(d_x.free)
        d_w = None
        if window is not None:
            d_w = DeviceBuffer.from_array(window)
            made.append(d_w.free)
        d_out = DeviceBuffer(int(np.prod(out_shape)) * np.dtype(out_dtype).itemsize)
        made.append(d_out.free)
        call(rp, d_x, d_w, d_out)
        synchronize()
        return d_out.to_array(out_dtype).reshape(out_shape)
    finally:
        for release in reversed(made):
            release()


def stft(x, n_fft, hop, window=None, center=False):
    """short-time Fourier transform of the float64 rows x, of shape (n,) or (batch, n): complex128
    (batch, nframes, n_fft/2+1), without the batch axis for 1-D input; frames of n_fft samples `hop`
    apart times `window`, forward r2c, unscaled.  center=True puts sample f*hop in the middle of
    frame f, with zeros outside the row.  Plans, uploads, runs hsfft_stft_batched and downloads"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    center = bool(center)
    if x.ndim not in (1, 2):
        raise ValueError("stft needs x of one or two dimensions")
    if n_fft < 2 or n_fft % 2 or hop < 1:
        raise ValueError("stft: n_fft is even and >= 2, hop >= 1")
    n = x.shape[-1]
    if n < 1 or (not center and n < n_fft):
        raise ValueError("stft: a row is empty or, without center, shorter than n_fft")
    window = _stft_window("stft", window, n_fft)
    nframes = 1 + n // hop if center else 1 + (n - n_fft) // hop
    shape = x.shape[:-1] + (nframes, n_fft // 2 + 1)
    if x.size == 0:
        return np.empty(shape, dtype=np.complex128)
    batch = x.size // n
    if nframes != stft_shape(n, n_fft, hop, center)[0]:
        raise HsfftError("stft: the library's frame count differs from the binding's")
    return _stft_run(lambda rp, d_x, d_w, d_out: stft_batched(rp, d_x, n, d_w, hop, center, d_out, batch),
                     (n_fft, 1), x, window, np.complex128, shape)


def istft(S, hop, window=None, center=False, normalize=True, length=None):
    """inverse of stft for complex128 S of shape (nframes, bins) or (batch, nframes, bins), n_fft =
    2 (bins - 1): float64 rows of `length` samples (None: (nframes-1)*hop + n_fft - 2*lpad, what
    the frames cover of the row); normalize divides by the overlap-added squared window.  Plans,
    uploads, runs hsfft_istft_batched and downloads"""
    S = np.ascontiguousarray(S, dtype=np.complex128)
    center = bool(center)
    if S.ndim not in (2, 3):
        raise ValueError("istft needs S of two or three dimensions")
    nframes, bins = S.shape[-2:]
    if nframes < 1 or bins < 2 or hop < 1:
        raise ValueError("istft: at least one frame, at least two bins, hop >= 1")
    n_fft = 2 * (bins - 1)
    window = _stft_window("istft", window, n_fft)
    n = (nframes - 1) * hop + n_fft - (n_fft if center else 0) if length is None else length
    if n < 1:
        raise ValueError("istft: the output length is below 1")
    shape = S.shape[:-2] + (n,)
    if S.size == 0:
        return np.empty(shape, dtype=np.float64)
    batch = S.size // (nframes * bins)
    return _stft_run(lambda rp, d_s, d_w, d_out: istft_batched(rp, d_s, nframes, d_w, hop, center, normalize, d_out, n,
                                                               batch),
                     (n_fft, -1), S, window, np.float64, shape)


KIND_COS, KIND_SIN = 0, 1  # include/hsfft_gpu.h


def dct_twiddles(n):
    """the n/2+1 rotation words (cos, sin)(pi k / 2n) of hsfft_dct_batched as complex128: host only"""
    t = np.empty(max(int(n), 0) // 2 + 1, dtype=np.complex128)
    check(lib().hsfft_dct_twiddles(n, _ptr(t)), "dct_twiddles")
    return t


def dct_batched(kind, type, d_in, d_out, n, batch):
    """batch real rows of n samples -> batch rows of n: kind KIND_COS / KIND_SIN, type 2 or 3,
    scipy's conventions with norm=None"""
    return check(lib().hsfft_dct_batched(kind, type, VP(d_in.ptr), VP(d_out.ptr), n, batch), "dct_batched")


def _dct_run(who, kind, type, x, inverse):
    """check the shape, upload x, run hsfft_dct_batched and download; inverse: the other type, then
    one division by 2.0 * n per word"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if type not in (2, 3):
        raise ValueError(f"{who}: type is 2 or 3")
    if x.ndim not in (1, 2):
        raise ValueError(f"{who} needs x of one or two dimensions")
    n = x.shape[-1]
    if n < 2 or n % 2:
        raise ValueError(f"{who}: the row length is even and >= 2")
    if x.size == 0:
        return np.empty(x.shape, dtype=np.float64)
    made = []
    try:
        d_in = DeviceBuffer.from_array(x)
        made.append(d_in.free)
        d_out = DeviceBuffer(x.nbytes)
        made.append(d_out.free)
        dct_batched(kind, 5 - type if inverse else type, d_in, d_out, n, x.size // n)
        synchronize()
        y = d_out.to_array(np.float64).reshape(x.shape)
    finally:
        for release in reversed(made):
            release()
    return y / (2.0 * n) if inverse else y


def dct(x, type=2):
    """DCT-II or DCT-III (scipy.fft.dct, norm=None) of the float64 rows x, of shape (n,) or
    (batch, n), n even: uploads, runs hsfft_dct_batched and downloads"""
    return _dct_run("dct", KIND_COS, type, x, False)


def dst(x, type=2):
    """DST-II or DST-III (scipy.fft.dst, norm=None) of the float64 rows x, of shape (n,) or (batch, n)"""
    return _dct_run("dst", KIND_SIN, type, x, False)


def idct(x, type=2):
    """inverse of dct(., type): the other type, divided by 2.0 * n in numpy (scipy.fft.idct, norm=None)"""
    return _dct_run("idct", KIND_COS, type, x, True)


def idst(x, type=2):
    """inverse of dst(., type): the other type, divided by 2.0 * n in numpy (scipy.fft.idst, norm=None)"""
    return _dct_run("idst", KIND_SIN, type, x, True)


def transpose_real_batched(d_in, d_out, rows, cols, batch):
    """out[b][c][r] = in[b][r][c] for batch matrices of rows x cols doubles"""
    return check(lib().hsfft_transpose_real_batched(VP(d_in.ptr), VP(d_out.ptr), rows, cols, batch),
                 "transpose_real_batched")


def dct_2d_batched(kind0, kind1, type, d_in, d_out, n0, n1, batch):
    """batch real images of n0 x n1 -> batch images of n0 x n1: kind1 along the rows, then kind0 along
    the columns (KIND_COS / KIND_SIN each), one type, 2 or 3, scipy's conventions with norm=None"""
    return check(lib().hsfft_dct_2d_batched(kind0, kind1, type, VP(d_in.ptr), VP(d_out.ptr), n0, n1, batch),
                 "dct_2d_batched")


def _dctn_run(who, kind, type, x, inverse):
    """check the shape, upload x, run hsfft_dct_2d_batched with `kind` on both axes and download;
    inverse: the other type, then one division by 4.0 * n0 * n1 per word"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if type not in (2, 3):
        raise ValueError(f"{who}: type is 2 or 3")
    if x.ndim < 2:
        raise ValueError(f"{who} needs an array of at least two dimensions")
    n0, n1 = x.shape[-2:]
    if n0 < 2 or n0 % 2 or n1 < 2 or n1 % 2:
        raise ValueError(f"{who}: the last two axes are even and >= 2 long")
    if x.size == 0:
        return np.empty(x.shape, dtype=np.float64)
    made = []
    try:
        d_in = DeviceBuffer.from_array(x)
        made.append(d_in.free)
        d_out = DeviceBuffer(x.nbytes)
        made.append(d_out.free)
        dct_2d_batched(kind, kind, 5 - type if inverse else type, d_in, d_out, n0, n1, x.size // (n0 * n1))
        synchronize()
        y = d_out.to_array(np.float64).reshape(x.shape)
    finally:
        for release in reversed(made):
            release()
    return y / (4.0 * n0 * n1) if inverse else y


def dctn(x, type=2):
    """2D DCT-II or DCT-III (scipy.fft.dctn, norm=None) over the last two axes of a float64 array of
    shape (..., n0, n1), both even: uploads, runs hsfft_dct_2d_batched and downloads"""
    return _dctn_run("dctn", KIND_COS, type, x, False)


def dstn(x, type=2):
    """2D DST-II or DST-III (scipy.fft.dstn, norm=None) over the last two axes of a float64 array"""
    return _dctn_run("dstn", KIND_SIN, type, x, False)


def idctn(x, type=2):
    """inverse of dctn(., type): the other type, divided by 4.0 * n0 * n1 in numpy (scipy.fft.idctn, norm=None)"""
    return _dctn_run("idctn", KIND_COS, type, x, True)


def idstn(x, type=2):
    """inverse of dstn(., type): the other type, divided by 4.0 * n0 * n1 in numpy (scipy.fft.idstn, norm=None)"""
    return _dctn_run("idstn", KIND_SIN, type, x, True)


def dct4_twiddles(n):
    """the n/2 rotation words (cos, sin)(pi (8j+1) / 8n) of hsfft_dct4_batched as complex128: host only"""
    t = np.empty(max(int(n), 0) // 2, dtype=np.complex128)
    check(lib().hsfft_dct4_twiddles(n, _ptr(t)), "dct4_twiddles")
    return t


def dct4_batched(kind, d_in, d_out, n, batch):
    """batch real rows of n samples -> batch rows of n: DCT-IV (KIND_COS) or DST-IV (KIND_SIN),
    scipy's conventions with norm=None"""
    return check(lib().hsfft_dct4_batched(kind, VP(d_in.ptr), VP(d_out.ptr), n, batch), "dct4_batched")


def mdct_shape(n, N, pad=False):
    """(nframes, lpad) of hsfft_mdct_batched: sizes only, no device touched"""
    v = [CI(0) for _ in range(2)]
    check(lib().hsfft_mdct_shape(n, N, int(pad), *(ctypes.byref(x) for x in v)), "mdct_shape")
    return tuple(x.value for x in v)


def mdct_batched(d_x, n, d_w, N, pad, d_out, batch):
    """batch real rows of n samples -> batch x nframes x N coefficients: frames of 2N samples N
    apart, times the window d_w of 2N (None: no window)"""
    return check(lib().hsfft_mdct_batched(VP(d_x.ptr), n, _opt_ptr(d_w), N, int(pad), VP(d_out.ptr), batch), "mdct_batched")


def imdct_batched(d_X, nframes, d_w, N, pad, d_out, n, batch):
    """batch x nframes x N coefficients -> batch real rows of n = (nframes + 1) N - 2 lpad samples:
    every frame's 2N samples / (N/2), times the window, overlap-added"""
    return check(lib().hsfft_imdct_batched(VP(d_X.ptr), nframes, _opt_ptr(d_w), N, int(pad), VP(d_out.ptr), n, batch),
                 "imdct_batched")


def _device_run(call, x, window, out_shape):
    """upload x and the window, run call(d_x, d_w, d_out), download float64 of out_shape"""
    made = []
    try:
        d_x = DeviceBuffer.from_array(x)
        made.append(d_x.free)
        d_w = None
        if window is not None:
            d_w = DeviceBuffer.from_array(window)
            made.append(d_w.free)
        d_out = DeviceBuffer(int(np.prod(out_shape)) * 8)
        made.append(d_out.free)
        call(d_x, d_w, d_out)
        synchronize()
        return d_out.to_array(np.float64).reshape(out_shape)
    finally:
        for release in reversed(made):
            release()


def _mdct_window(who, window, N):
    if window is None:
        return None
    window = np.ascontiguousarray(window, dtype=np.float64)
    if window.shape != (2 * N,):
        raise ValueError(f"{who}: the window is one-dimensional, 2 N = {2 * N} long")
    return window


def _dct4_run(who, kind, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim not in (1, 2):
        raise ValueError(f"{who} needs x of one or two dimensions")
    n = x.shape[-1]
    if n < 2 or n % 2:
        raise ValueError(f"{who}: the row length is even and >= 2")
    if x.size == 0:
        return np.empty(x.shape, dtype=np.float64)
    return _device_run(lambda d_x, d_w, d_out: dct4_batched(kind, d_x, d_out, n, x.size // n), x, None, x.shape)


def dct4(x):
    """DCT-IV (scipy.fft.dct(x, type=4), norm=None) of the float64 rows x, of shape (n,) or (batch, n),
    n even; its own inverse up to 2n: uploads, runs hsfft_dct4_batched and downloads"""
    return _dct4_run("dct4", KIND_COS, x)


def dst4(x):
    """DST-IV (scipy.fft.dst(x, type=4), norm=None) of the float64 rows x, of shape (n,) or (batch, n)"""
    return _dct4_run("dst4", KIND_SIN, x)


def dct1_shape(kind, n):
    """(L, bins) of hsfft_dct1_batched: the extended length 2(n-1) (KIND_COS) or 2(n+1) (KIND_SIN) and
    its L/2+1 compact bins; sizes only, no device touched"""
    v = [CI(0) for _ in range(2)]
    check(lib().hsfft_dct1_shape(kind, n, *(ctypes.byref(x) for x in v)), "dct1_shape")
    return tuple(x.value for x in v)


def dct1_batched(kind, d_in, d_out, n, batch):
    """batch real rows of n samples -> batch rows of n: DCT-I (KIND_COS, n >= 2) or DST-I (KIND_SIN,
    n >= 1), scipy's conventions with norm=None; every length, odd ones included"""
    return check(lib().hsfft_dct1_batched(kind, VP(d_in.ptr), VP(d_out.ptr), n, batch), "dct1_batched")


def dct1_2d_batched(kind0, kind1, d_in, d_out, n0, n1, batch):
    """batch real images of n0 x n1 -> batch images of n0 x n1: type I of kind1 along the rows, then of
    kind0 along the columns (KIND_COS / KIND_SIN each), scipy's conventions with norm=None"""
    return check(lib().hsfft_dct1_2d_batched(kind0, kind1, VP(d_in.ptr), VP(d_out.ptr), n0, n1, batch), "dct1_2d_batched")


def _dct1_factor(kind, n):
    """T(T(x)) = factor x: 2(n-1) for DCT-I, 2(n+1) for DST-I"""
    return 2.0 * (n + 1) if kind == KIND_SIN else 2.0 * (n - 1)


def _dct1_run(who, kind, x, inverse):
    """check the shape, upload x, run hsfft_dct1_batched and download; inverse: the same transform,
    then one division by 2.0 * (n-1) or 2.0 * (n+1) per word"""
    x = np.asarray(x, dtype=np.float64)  # a scalar keeps its zero dimensions here and is rejected
    if x.ndim not in (1, 2):
        raise ValueError(f"{who} needs x of one or two dimensions")
    x = np.ascontiguousarray(x)
    n = x.shape[-1]
    if n < (1 if kind == KIND_SIN else 2):
        raise ValueError(f"{who}: the row length is at least {1 if kind == KIND_SIN else 2}")
    if x.size == 0:
        return np.empty(x.shape, dtype=np.float64)
    y = _device_run(lambda d_x, d_w, d_out: dct1_batched(kind, d_x, d_out, n, x.size // n), x, None, x.shape)
    return y / _dct1_factor(kind, n) if inverse else y


def dct1(x):
    """DCT-I (scipy.fft.dct(x, type=1), norm=None) of the float64 rows x, of shape (n,) or (batch, n),
    n >= 2, odd or even: uploads, runs hsfft_dct1_batched and downloads"""
    return _dct1_run("dct1", KIND_COS, x, False)


def dst1(x):
    """DST-I (scipy.fft.dst(x, type=1), norm=None) of the float64 rows x, of shape (n,) or (batch, n), n >= 1"""
    return _dct1_run("dst1", KIND_SIN, x, False)


def idct1(x):
    """inverse of dct1: dct1 divided by 2.0 * (n-1) in numpy (scipy.fft.idct(x, type=1), norm=None)"""
    return _dct1_run("idct1", KIND_COS, x, True)


def idst1(x):
    """inverse of dst1: dst1 divided by 2.0 * (n+1) in numpy (scipy.fft.idst(x, type=1), norm=None)"""
    return _dct1_run("idst1", KIND_SIN, x, True)


def _dct1n_run(who, kind, x, inverse):
    """check the shape, upload x, run hsfft_dct1_2d_batched with `kind` on both axes and download;
    inverse: the same transform, then one division by the product of the two axes' factors per word"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim < 2:
        raise ValueError(f"{who} needs an array of at least two dimensions")
    n0, n1 = x.shape[-2:]
    least = 1 if kind == KIND_SIN else 2
    if n0 < least or n1 < least:
        raise ValueError(f"{who}: the last two axes are at least {least} long")
    if x.size == 0:
        return np.empty(x.shape, dtype=np.float64)
    y = _device_run(lambda d_x, d_w, d_out: dct1_2d_batched(kind, kind, d_x, d_out, n0, n1, x.size // (n0 * n1)), x, None,
                    x.shape)
    return y / (_dct1_factor(kind, n0) * _dct1_factor(kind, n1)) if inverse else y


def dct1n(x):
    """2D DCT-I (scipy.fft.dctn(x, type=1), norm=None) over the last two axes of a float64 array of
    shape (..., n0, n1), both >= 2: uploads, runs hsfft_dct1_2d_batched and downloads"""
    return _dct1n_run("dct1n", KIND_COS, x, False)


def dst1n(x):
    """2D DST-I (scipy.fft.dstn(x, type=1), norm=None) over the last two axes of a float64 array"""
    return _dct1n_run("dst1n", KIND_SIN, x, False)


def idct1n(x):
    """inverse of dct1n: dct1n divided by 2.0 * (n0-1) * (2.0 * (n1-1)) in numpy"""
    return _dct1n_run("idct1n", KIND_COS, x, True)


def idst1n(x):
    """inverse of dst1n: dst1n divided by 2.0 * (n0+1) * (2.0 * (n1+1)) in numpy"""
    return _dct1n_run("idst1n", KIND_SIN, x, True)


def mdct(x, N, window=None, pad=False):
    """MDCT of the float64 rows x, of shape (n,) or (batch, n), n a multiple of the hop N (even):
    float64 (batch, nframes, N), without the batch axis for 1-D input; frames of 2N samples N apart
    times `window` (2N long).  pad=True adds one frame at either end, so that every sample lies in
    two frames.  Uploads, runs hsfft_mdct_batched and downloads"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    pad = bool(pad)
    if x.ndim not in (1, 2):
        raise ValueError("mdct needs x of one or two dimensions")
    if N < 2 or N % 2:
        raise ValueError("mdct: the hop N is even and >= 2")
    n = x.shape[-1]
    if n % N or n < (N if pad else 2 * N):
        raise ValueError("mdct: a row is a multiple of N long and holds at least one frame of 2N (N with pad)")
    window = _mdct_window("mdct", window, N)
    nframes = n // N + 1 if pad else n // N - 1
    shape = x.shape[:-1] + (nframes, N)
    if x.size == 0:
        return np.empty(shape, dtype=np.float64)
    if nframes != mdct_shape(n, N, pad)[0]:
        raise HsfftError("mdct: the library's frame count differs from the binding's")
    return _device_run(lambda d_x, d_w, d_out: mdct_batched(d_x, n, d_w, N, pad, d_out, x.size // n), x, window, shape)


def imdct(X, window=None, pad=False):
    """inverse of mdct for float64 X of shape (nframes, N) or (batch, nframes, N): rows of (nframes +
    1) N samples, 2N fewer with pad; with a window whose squares N apart add up to one, imdct(mdct(x))
    is x on every sample that two frames cover.  Uploads, runs hsfft_imdct_batched and downloads"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    pad = bool(pad)
    if X.ndim not in (2, 3):
        raise ValueError("imdct needs X of two or three dimensions")
    nframes, N = X.shape[-2:]
    if N < 2 or N % 2 or nframes < (2 if pad else 1):
        raise ValueError("imdct: N is even and >= 2, and there is at least one frame (two with pad)")
    window = _mdct_window("imdct", window, N)
    n = (nframes + 1) * N - (2 * N if pad else 0)
    shape = X.shape[:-2] + (n,)
    if X.size == 0:
        return np.empty(shape, dtype=np.float64)
    batch = X.size // (nframes * N)
    return _device_run(lambda d_X, d_w, d_out: imdct_batched(d_X, nframes, d_w, N, pad, d_out, n, batch), X, window, shape)


def czt_shape(n, m):
    """the padded power-of-two length L = max(2, next power of two >= n + m - 1) of the chirp-z
    calls: sizes only, no device touched"""
    L = CI(0)
    check(lib().hsfft_czt_shape(n, m, ctypes.byref(L)), "czt_shape")
    return L.value


def czt_tables(n, m, f0, df):
    """(pre, chirp) of hsfft_czt_batched as complex128 (cos + i sin): the n input-rotation words and
    the max(n, m) chirp words, phases reduced exactly: host only"""
    n, m = int(n), int(m)
    pre = np.empty(max(n, 0), dtype=np.complex128)
    chirp = np.empty(max(n, m, 0), dtype=np.complex128)
    check(lib().hsfft_czt_tables(n, m, f0, df, _ptr(pre), _ptr(chirp)), "czt_tables")
    return pre, chirp


def czt_batched(d_in, real, n, d_out, m, f0, df, batch):
    """batch rows of n samples, float64 (real true) or complex128 -> batch rows of m complex:
    X[k] = sum_j x[j] exp(-2 pi i j (f0 + k df)), f0 and df in cycles per sample"""
    fn = lib().hsfft_czt_real_batched if real else lib().hsfft_czt_batched
    return check(fn(VP(d_in.ptr), n, VP(d_out.ptr), m, f0, df, batch), "czt_real_batched" if real else "czt_batched")


def czt(x, m, f0, df):
    """chirp-z transform on the unit circle of the rows x, float64 or complex128 of shape (n,) or
    (batch, n): complex128 (batch, m), without the batch axis for 1-D input, X[k] = sum_j x[j]
    exp(-2 pi i j (f0 + k df)).  scipy.signal.czt(x, m, w, a) with w = exp(-2 pi i df), a = exp(2 pi i
    f0).  Uploads, runs hsfft_czt_batched or hsfft_czt_real_batched (picked by the dtype) and downloads"""
    x = np.asarray(x)
    if x.ndim not in (1, 2):
        raise ValueError("czt needs x of one or two dimensions")
    real = not np.iscomplexobj(x)
    x = np.ascontiguousarray(x, dtype=np.float64 if real else np.complex128)
    n, m = x.shape[-1], int(m)
    if n < 1 or m < 1 or n + m - 1 > 1 << 26:
        raise ValueError("czt: n and m are at least 1 and n + m - 1 is at most 2^26")
    f0, df = float(f0), float(df)
    if not (abs(f0) <= 1.0 and abs(df) <= 1.0):
        raise ValueError("czt: f0 and df are finite and at most 1 in magnitude (frequencies are periodic: reduce them)")
    shape = x.shape[:-1] + (m,)
    if x.size == 0:
        return np.empty(shape, dtype=np.complex128)
    made = []
    try:
        d_x = DeviceBuffer.from_array(x)
        made.append(d_x.free)
        d_out = DeviceBuffer(int(np.prod(shape)) * 16)
        made.append(d_out.free)
        czt_batched(d_x, real, n, d_out, m, f0, df, x.size // n)
        synchronize()
        return d_out.to_array(np.complex128).reshape(shape)
    finally:
        for release in reversed(made):
            release()


def zoom_fft(x, fn, m=None, fs=2.0, endpoint=False):
    """scipy.signal.zoom_fft: m bins of the rows x from f1 to f2 (fn = [f1, f2], or a scalar f2 with f1 =
    0) at the sampling frequency fs; m defaults to the row length, and endpoint=True includes f2.  It is
    czt(x, m, f1 / fs, (f2 - f1) / (d fs)) with d = m - 1 for endpoint, else m"""
    x = np.asarray(x)
    if x.ndim not in (1, 2):
        raise ValueError("zoom_fft needs x of one or two dimensions")
    m = x.shape[-1] if m is None else int(m)
    if m < 1:
        raise ValueError("zoom_fft: m is at least 1")
    fn = np.atleast_1d(np.asarray(fn, dtype=np.float64))
    if fn.shape == (1,):
        f1, f2 = 0.0, float(fn[0])
    elif fn.shape == (2,):
        f1, f2 = float(fn[0]), float(fn[1])
    else:
        raise ValueError("zoom_fft: fn is a scalar or holds two frequencies")
    d = m - 1 if endpoint else m
    return czt(x, m, f1 / fs, (f2 - f1) / (d * fs) if d else 0.0)


def spectral_chunk_rows(n, m=0):
    """the rows of one chunk of hilbert_batched (m == 0) or resample_batched by the documented rule,
    HSFFT_SPECTRAL_CHUNK_MB over a row's scratch bytes, before the clamp to the batch: host only"""
    rows = ctypes.c_longlong(0)
    check(lib().hsfft_spectral_chunk_rows(n, m, ctypes.byref(rows)), "spectral_chunk_rows")
    return rows.value


def hilbert_batched(d_in, d_out, n, batch):
    """batch real rows of n samples (n even) -> batch rows of n complex: the analytic signal x + i H[x]
    of scipy.signal.hilbert.  Both buffers 16-byte aligned.  Results follow the thread's twiddle mode:
    full accuracy on powers of two, about 1e-11 in the exact mode on lengths with factors 3, 5 or 7,
    and the reference's quirk results in the default mode on lengths such as 6 and 12"""
    return check(lib().hsfft_hilbert_batched(VP(d_in.ptr), VP(d_out.ptr), n, batch), "hilbert_batched")


def resample_batched(d_in, n, d_out, m, batch):
    """batch real rows of n samples -> batch real rows of m samples (both even): scipy.signal.resample(x,
    m), the spectrum truncated or zero-extended.  Both buffers 16-byte aligned.  Accuracy and twiddle
    mode as for hilbert_batched, by both lengths"""
    return check(lib().hsfft_resample_batched(VP(d_in.ptr), n, VP(d_out.ptr), m, batch), "resample_batched")


def _spectral_rows(who, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim not in (1, 2):
        raise ValueError(f"{who} needs x of one or two dimensions")
    n = x.shape[-1]
    if n < 2 or n % 2 or n > 1 << 30:
        raise ValueError(f"{who}: the row length is even, at least 2 and at most 2^30")
    return x, n


def hilbert(x):
    """analytic signal (scipy.signal.hilbert) of the float64 rows x, of shape (n,) or (batch, n), n even:
    complex128 of the same shape, real part x, imaginary part its Hilbert transform.  Uploads, runs
    hsfft_hilbert_batched and downloads.  Accuracy follows the thread's twiddle mode (hilbert_batched)"""
    x, n = _spectral_rows("hilbert", x)
    if x.size == 0:
        return np.empty(x.shape, dtype=np.complex128)
    made = []
    try:
        d_x = DeviceBuffer.from_array(x)
        made.append(d_x.free)
        d_out = DeviceBuffer(x.size * 16)
        made.append(d_out.free)
        hilbert_batched(d_x, d_out, n, x.size // n)
        synchronize()
        return d_out.to_array(np.complex128).reshape(x.shape)
    finally:
        for release in reversed(made):
            release()


def resample(x, num):
    """Fourier resampling (scipy.signal.resample(x, num)) of the float64 rows x, of shape (n,) or (batch,
    n), to num samples per row, n and num even: float64.  Uploads, runs hsfft_resample_batched and
    downloads.  Accuracy follows the thread's twiddle mode (hilbert_batched)"""
    x, n = _spectral_rows("resample", x)
    num = int(num)
    if num < 2 or num % 2 or num > 1 << 30:
        raise ValueError("resample: num is even, at least 2 and at most 2^30")
    shape = x.shape[:-1] + (num,)
    if x.size == 0:
        return np.empty(shape, dtype=np.float64)
    return _device_run(lambda d_x, d_w, d_out: resample_batched(d_x, n, d_out, num, x.size // n), x, None, shape)


def r2c_batched(rplan, d_in, d_out, batch):
    return check(lib().hsfft_r2c_batched(rplan.ptr, VP(d_in.ptr), VP(d_out.ptr), batch), "r2c_batched")


def r2c_batched_compact(rplan, d_in, d_out, batch):
    return check(lib().hsfft_r2c_batched_compact(rplan.ptr, VP(d_in.ptr), VP(d_out.ptr), batch),
                 "r2c_batched_compact")


def c2r_batched(rplan, d_in, d_out, batch):
    return check(lib().hsfft_c2r_batched(rplan.ptr, VP(d_in.ptr), VP(d_out.ptr), batch), "c2r_batched")


def fill_complex(d, count, seed, offset=0):
    return check(lib().hsfft_fill_complex(VP(d.ptr), count, seed, offset), "fill_complex")


def fill_real(d, count, seed, offset=0):
    return check(lib().hsfft_fill_real(VP(d.ptr), count, seed, offset), "fill_real")


def synchronize():
    return check(lib().hsfft_synchronize(), "synchronize")


def finalize():
    """hsfft_finalize(): release every device object the library holds (before process exit)"""
    return check(lib().hsfft_finalize(), "finalize")


def set_twiddle_mode(mode):
    return check(lib().hsfft_set_twiddle_mode({"reference": 0, "exact": 1}.get(mode, mode)), "twiddle_mode")


def time_batched(plan, d_in, d_out, batch, iters, max_pass=16):
    ms = ctypes.c_float(0.0)
    pms = (ctypes.c_float * max_pass)()
    check(lib().hsfft_time_batched(plan.ptr, VP(d_in.ptr), VP(d_out.ptr), batch, iters, ctypes.byref(ms), pms,
                                   max_pass), "time_batched")
    return ms.value, [pms[i] for i in range(max_pass)]


def bench_copy(d_src, d_dst, nbytes, iters):
    ms = ctypes.c_float(0.0)
    check(lib().hsfft_bench_copy(VP(d_src.ptr), VP(d_dst.ptr), nbytes, iters, ctypes.byref(ms)), "bench_copy")
    return ms.value


def bench_transpose_herm(d_in, d_out, n0, n1, batch, iters):
    """milliseconds of `iters` mirrored transposes (the last step of r2c_2d_full), event-timed"""
    ms = ctypes.c_float(0.0)
    check(lib().hsfft_bench_transpose_herm(VP(d_in.ptr), VP(d_out.ptr), n0, n1, batch, iters, ctypes.byref(ms)),
          "bench_transpose_herm")
    return ms.value


def count_diff_words(d_a, d_b, nbytes):
    """8-byte words that differ between two device buffers (on the GPU)"""
    c = ctypes.c_uint64(0)
    check(lib().hsfft_count_diff_words(VP(d_a.ptr), VP(d_b.ptr), nbytes, ctypes.byref(c)), "count_diff_words")
    return c.value


def time_r2c_batched(rplan, d_in, d_out, batch, iters):
    ms = ctypes.c_float(0.0)
    check(lib().hsfft_time_r2c_batched(rplan.ptr, VP(d_in.ptr), VP(d_out.ptr), batch, iters, ctypes.byref(ms)),
          "time_r2c_batched")
    return ms.value
