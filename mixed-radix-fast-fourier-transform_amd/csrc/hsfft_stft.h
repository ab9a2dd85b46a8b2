/*
 * hsfft_stft.h -- batched short-time Fourier transform of real rows and its inverse
 * (hsfft_stft_shape, hsfft_stft_batched, hsfft_istft_batched of include/hsfft_gpu.h; the
 * reference has whole-row transforms only).  Included at the end of hsfft_device.hip after
 * hsfft_filter.h: the drivers launch their two kernels directly, so no host C file needs a new
 * device-layer symbol.
 *
 * Forward: the overlapping frames of every row are gathered, multiplied by the window, into a
 * scratch of contiguous rows of N, and hs_r2c_rows() unchanged writes their compact spectra
 * straight into the caller's output.  Inverse: hs_c2r_rows() unchanged turns every frame's
 * N/2+1 bins into N reals in the scratch, and one kernel divides, windows and adds the frames
 * that cover each output sample, in increasing frame order.  The scratch is
 * bounded by HSFFT_STFT_CHUNK_MB, not by the job.
 */
#include "hsfft_gpu.h"
#include "hsfft_host.h"

namespace stft {

/* Frame gather with the window: frame yi of the launch is frame q = q0 + yi of the call, frame
 * f = q % nframes of row b = q / nframes; dst[yi][j] = xpad[start + j] * w[j] with start = f hop -
 * lpad, xpad = x[b] inside [0, n) and +0.0 outside (the product is computed there too: +0.0 *
 * w[j]), and no multiply at all where w == NULL.  Nothing is read outside row b.  One lane writes
 * 16 bytes (destination rows are N x 8 bytes, N even, so every pair is aligned); the source
 * offset b n + start can be odd, so the pair is one 16-byte load where the frame's first sample
 * is 16-byte aligned and both words lie inside the row, and 8-byte loads elsewhere.  The window
 * is N doubles read by every frame: it stays in L2.  q is uniform over the workgroup: the
 * division runs once on the scalar unit. */
__global__ __launch_bounds__(256) void k_stft_frames(const double *__restrict__ x, const double *__restrict__ w,
                                                     long long n, long long N, long long hop, long long lpad,
                                                     long long nframes, long long q0, double *__restrict__ dst)
{
    const long long yi = blockIdx.y, q = q0 + yi, b = q / nframes, f = q - b * nframes;
    const long long start = f * hop - lpad;
    const double *xrow = x + b * n;
    v2d *row = (v2d *)(dst + yi * N);
    const bool al = (((uintptr_t)xrow + 8 * (uintptr_t)start) & 15) == 0;
    const bool wal = ((uintptr_t)w & 15) == 0;
    const long long pairs = N / 2;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < pairs; i += (long long)gridDim.x * blockDim.x) {
        const long long j = 2 * i, p = start + j;
        const bool in0 = p >= 0 && p < n, in1 = p + 1 >= 0 && p + 1 < n;
        v2d v = {0.0, 0.0};
        if (in0 && in1 && al) v = *(const v2d *)(xrow + p);
        else {
            if (in0) v.x = xrow[p];
            if (in1) v.y = xrow[p + 1];
        }
        if (w) {
            v2d c;
            if (wal) c = *(const v2d *)(w + j);
            else {
                c.x = w[j];
                c.y = w[j + 1];
            }
            v.x = v.x * c.x;
            v.y = v.y * c.y;
        }
        row[i] = v;
    }
}

struct ola_args {
    const double *Y; /* the chunk's unscaled frames, rows of N: frame f of the chunk's row r at (r nframes + f) N */
    const double *w; /* the window, or NULL */
    double *out;     /* the chunk's first output row */
    long long r0;    /* the chunk's row index of the launch's row 0 */
    long long n, N, hop, lpad, nframes;
    int normalize;
    double div;
};

/* one output sample: the frames f in [0, nframes) with 0 <= i + lpad - f hop < N, in increasing
 * f.  Each term is y / N, then times w[j], each rounded on its own; the accumulator starts as the
 * first term and every later term is one add.  The envelope is built the same way from w[j] w[j]
 * (1.0 per frame without a window) and divides the sum once, whatever it is.  A sample that no
 * frame covers is +0.0. */
__device__ __forceinline__ double ola_word(const ola_args &a, const double *yrow, long long i)
{
    /* n, N <= 2^30 and hop, nframes < 2^31: t, the frame numbers and j fit 32 bits, and the
     * divisions are 32-bit ones */
    const unsigned t = (unsigned)(i + a.lpad), N = (unsigned)a.N, hop = (unsigned)a.hop;
    unsigned f = t >= N ? (t - N) / hop + 1 : 0, fhi = t / hop;
    if (fhi > (unsigned)a.nframes - 1) fhi = (unsigned)a.nframes - 1;
    if (f > fhi) return 0.0;
    double acc = 0.0, env = 0.0;
    bool first = true;
    for (; f <= fhi; f++) {
        const unsigned j = t - f * hop;
        double v = yrow[(long long)f * a.N + j] / a.div, e = 1.0;
        if (a.w) {
            const double c = a.w[j];
            v = v * c;
            e = c * c;
        }
        acc = first ? v : acc + v;
        env = first ? e : env + e;
        first = false;
    }
    return a.normalize ? acc / env : acc;
}

/* Windowed overlap-add: row yi of the launch is row r = r0 + yi of the chunk.  A lane owns two
 * neighbouring output samples, paired so that their address is 16-byte aligned whatever the
 * alignment of the row (the pair index is shifted by the row's misalignment; the row's first or
 * last sample can be a pair of one), computes both in registers and stores once: 16 bytes where
 * both samples exist, 8 otherwise.  Neighbouring lanes read neighbouring words of the same frame.
 * No output word is read and there are no atomics: the order of the adds is the contract.
 * Compiled under the file's -ffp-contract=off. */
__global__ __launch_bounds__(256) void k_istft_ola(ola_args a)
{
    const long long r = a.r0 + blockIdx.y;
    const double *yrow = a.Y + r * a.nframes * a.N;
    double *orow = a.out + r * a.n;
    const long long mis = ((uintptr_t)orow >> 3) & 1, pairs = (a.n + mis + 1) / 2;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < pairs; k += (long long)gridDim.x * blockDim.x) {
        const long long i = 2 * k - mis;
        const bool in0 = i >= 0, in1 = i + 1 < a.n;
        v2d v;
        if (in0) v.x = ola_word(a, yrow, i);
        if (in1) v.y = ola_word(a, yrow, i + 1);
        if (in0 && in1) *(v2d *)(orow + i) = v;
        else if (in0) orow[i] = v.x;
        else if (in1) orow[i + 1] = v.y;
    }
}

constexpr int MAX_LEN = 1 << 30;          /* n and N */
constexpr long long MAX_WORDS = 1LL << 40; /* n x batch and nframes x batch x N */

/* the part of the shape rule both directions share: 0, or HSFFT_ERR_ARG with the message set */
static int check_sizes(const char *who, int n, int N, int hop, int center)
{
    if (N < 2 || (N & 1) || N > MAX_LEN || hop < 1 || n < 1 || n > MAX_LEN ||
        (center != 0 && center != 1)) {
        hs_seterr("%s: n %d, frame length %d, hop %d or center %d is out of range", who, n, N, hop, center);
        return HSFFT_ERR_ARG;
    }
    return 0;
}

/* 0 with *nframes set, or HSFFT_ERR_ARG with the message set */
static int get_shape(const char *who, int n, int N, int hop, int center, int *nframes)
{
    const int rc = check_sizes(who, n, N, hop, center);
    if (rc) return rc;
    if (!center && n < N) {
        hs_seterr("%s: a row of %d samples is shorter than the frame of %d (center == 0)", who, n, N);
        return HSFFT_ERR_ARG;
    }
    *nframes = center ? 1 + n / hop : 1 + (n - N) / hop;
    return 0;
}

/* the frame length of a real plan, or 0 where there is no plan or 2 x its inner length is out of range */
static int plan_len(fft_real_object r)
{
    return r && r->cobj && r->cobj->N >= 1 && r->cobj->N <= MAX_LEN / 2 ? 2 * r->cobj->N : 0;
}

/* the bounds on a call's totals: 0, or HSFFT_ERR_ARG with the message set */
static int check_totals(const char *who, int n, int N, int nframes, int batch)
{
    const long long total = (long long)nframes * batch;
    if (total > 0x7fffffffLL || total * N > MAX_WORDS || (long long)n * batch > MAX_WORDS) {
        hs_seterr("%s: %d frames of %d in each of %d rows of %d are more than the call can index", who, nframes, N,
                  batch, n);
        return HSFFT_ERR_ARG;
    }
    return 0;
}

static int dev_rc(int rc, const char *what)
{
    if (rc) hs_seterr("%s: %s", what, hsd_errstr());
    return rc ? HSFFT_ERR_DEVICE : 0;
}

static int frames(const fft_type *x, const fft_type *w, long long n, long long N, long long hop, long long lpad,
                  long long nframes, long long q0, double *R, long long cb)
{
    for (long long b0 = 0; b0 < cb; b0 += Y_MAX) {
        const int nb = (int)(cb - b0 < Y_MAX ? cb - b0 : Y_MAX);
        hipLaunchKernelGGL(k_stft_frames, dim3(grid_for(N / 2, 256), nb), dim3(256), 0, stream(), x, w, n, N, hop, lpad,
                           nframes, q0 + b0, R + b0 * N);
        HCHK(hipGetLastError());
    }
    return 0;
}

static int ola(ola_args a, long long rows)
{
    for (long long b0 = 0; b0 < rows; b0 += Y_MAX) {
        const int nb = (int)(rows - b0 < Y_MAX ? rows - b0 : Y_MAX);
        a.r0 = b0;
        hipLaunchKernelGGL(k_istft_ola, dim3(grid_for((a.n + 2) / 2, 256), nb), dim3(256), 0, stream(), a);
        HCHK(hipGetLastError());
    }
    return 0;
}

/* (device lock held) the forward call.  Frames are numbered q = b nframes + f and walked in
 * chunks of `c` consecutive q, which may cross row boundaries, with one pool buffer R (c x N
 * doubles).  Per chunk: gather and window x -> R, r2c-compact rows R -> the caller's output. */
static int run_forward(fft_real_object r, const fft_type *d_x, int n, const fft_type *d_w, int hop, int lpad,
                       int nframes, fft_data *d_out, int batch)
{
    const long long N = 2LL * r->cobj->N, total = (long long)batch * nframes;
    long long c = (long long)(hs_env_mb("HSFFT_STFT_CHUNK_MB", 1024.0) / (sizeof(double) * (size_t)N));
    if (c > total) c = total;
    if (c < 1) c = 1;
    double *R;
    for (;;) {
        R = (double *)hs_scratch(HS_SCR_STFT, sizeof(double) * (size_t)N * (size_t)c);
        if (R || c == 1) break;
        c = (c + 1) / 2;
    }
    if (!R) {
        hs_seterr("hsfft_stft_batched: scratch allocation failed (%lld frames of %lld)", c, N);
        return HSFFT_ERR_NOMEM;
    }
    int rc = 0;
    for (long long q0 = 0; q0 < total && !rc; q0 += c) {
        const long long cb = total - q0 < c ? total - q0 : c;
        rc = dev_rc(frames(d_x, d_w, n, N, hop, lpad, nframes, q0, R, cb), "stft frame gather");
        if (!rc) rc = hs_r2c_rows(r, R, d_out + q0 * (N / 2 + 1), (int)cb, 1);
    }
    return rc;
}

/* (device lock held) the inverse call.  Whole rows are walked in chunks of `c` rows with one pool
 * buffer Y (c x nframes x N doubles): a row's frames never straddle a chunk, so nothing is
 * carried.  Per chunk: c2r rows spec -> Y at the pitch N/2+1, overlap-add Y -> out. */
static int run_inverse(fft_real_object ri, const fft_data *d_spec, int nframes, const fft_type *d_w, int hop, int lpad,
                       int normalize, fft_type *d_out, int n, int batch)
{
    const long long N = 2LL * ri->cobj->N, bins = N / 2 + 1;
    const size_t per = sizeof(double) * (size_t)N * (size_t)nframes;
    long long c = (long long)(hs_env_mb("HSFFT_STFT_CHUNK_MB", 1024.0) / per);
    if (c > batch) c = batch;
    if (c < 1) c = 1;
    double *Y;
    for (;;) {
        Y = (double *)hs_scratch(HS_SCR_STFT, per * (size_t)c);
        if (Y || c == 1) break;
        c = (c + 1) / 2;
    }
    if (!Y) {
        hs_seterr("hsfft_istft_batched: scratch allocation failed (%lld rows of %d frames of %lld)", c, nframes, N);
        return HSFFT_ERR_NOMEM;
    }
    ola_args a;
    a.Y = Y;
    a.w = d_w;
    a.r0 = 0;
    a.n = n;
    a.N = N;
    a.hop = hop;
    a.lpad = lpad;
    a.nframes = nframes;
    a.normalize = normalize;
    a.div = (double)N;
    int rc = 0;
    for (long long b0 = 0; b0 < batch && !rc; b0 += c) {
        const long long rows = batch - b0 < c ? batch - b0 : c;
        rc = hs_c2r_rows(ri, d_spec + b0 * nframes * bins, NULL, bins, Y, (int)(rows * nframes));
        a.out = d_out + b0 * n;
        if (!rc) rc = dev_rc(ola(a, rows), "istft overlap-add");
    }
    return rc;
}

}  // namespace stft

extern "C" {

int hsfft_stft_shape(int n, int N, int hop, int center, int *nframes, int *bins, int *lpad)
{
    hs_seterr("%s", "");
    int nf;
    const int rc = stft::get_shape("hsfft_stft_shape", n, N, hop, center, &nf);
    if (rc) return rc;
    if (nframes) *nframes = nf;
    if (bins) *bins = N / 2 + 1;
    if (lpad) *lpad = center ? N / 2 : 0;
    return 0;
}

int hsfft_stft_batched(fft_real_object r, const fft_type *d_x, int n, const fft_type *d_w, int hop, int center,
                       fft_data *d_out, int batch)
{
    hs_seterr("%s", "");
    const int N = stft::plan_len(r);
    if (!N || !d_x || !d_out || batch < 0) {
        hs_seterr("hsfft_stft_batched: invalid arguments");
        return HSFFT_ERR_ARG;
    }
    int nframes;
    int rc = stft::get_shape("hsfft_stft_batched", n, N, hop, center, &nframes);
    if (!rc) rc = stft::check_totals("hsfft_stft_batched", n, N, nframes, batch);
    if (rc) return rc;
    const uintptr_t nb = (uintptr_t)batch;
    const uintptr_t out_bytes = sizeof(fft_data) * (uintptr_t)nframes * (uintptr_t)(N / 2 + 1) * nb;
    if (tr2d::overlap_bytes(d_out, out_bytes, d_x, sizeof(fft_type) * (uintptr_t)n * nb) ||
        (d_w && tr2d::overlap_bytes(d_out, out_bytes, d_w, batch ? sizeof(fft_type) * (uintptr_t)N : 0))) {
        hs_seterr("hsfft_stft_batched: the output overlaps an input");
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    rc = hs_require_gpu();
    if (rc) return rc;
    const int d = hs_lock_device();
    rc = stft::run_forward(r, d_x, n, d_w, hop, center ? N / 2 : 0, nframes, d_out, batch);
    hs_unlock_device(d);
    return rc;
}

int hsfft_istft_batched(fft_real_object ri, const fft_data *d_spec, int nframes, const fft_type *d_w, int hop,
                        int center, int normalize, fft_type *d_out, int n, int batch)
{
    hs_seterr("%s", "");
    const int N = stft::plan_len(ri);
    if (!N || !d_spec || !d_out || batch < 0) {
        hs_seterr("hsfft_istft_batched: invalid arguments");
        return HSFFT_ERR_ARG;
    }
    int rc = stft::check_sizes("hsfft_istft_batched", n, N, hop, center);
    if (rc) return rc;
    if (nframes < 1) {
        hs_seterr("hsfft_istft_batched: %d frames", nframes);
        return HSFFT_ERR_ARG;
    }
    rc = stft::check_totals("hsfft_istft_batched", n, N, nframes, batch);
    if (rc) return rc;
    const uintptr_t nb = (uintptr_t)batch;
    const uintptr_t out_bytes = sizeof(fft_type) * (uintptr_t)n * nb;
    if (tr2d::overlap_bytes(d_out, out_bytes, d_spec, sizeof(fft_data) * (uintptr_t)nframes * (uintptr_t)(N / 2 + 1) * nb) ||
        (d_w && tr2d::overlap_bytes(d_out, out_bytes, d_w, batch ? sizeof(fft_type) * (uintptr_t)N : 0))) {
        hs_seterr("hsfft_istft_batched: the output overlaps an input");
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    rc = hs_require_gpu();
    if (rc) return rc;
    const int d = hs_lock_device();
    rc = stft::run_inverse(ri, d_spec, nframes, d_w, hop, center ? N / 2 : 0, normalize != 0, d_out, n, batch);
    hs_unlock_device(d);
    return rc;
}

}  // extern "C"
