/*
 * hsfft_dct.h -- batched DCT-II / DCT-III and DST-II / DST-III of real rows (hsfft_dct_batched of
 * include/hsfft_gpu.h; the reference has no cosine or sine transform).
 * Included at the end of hsfft_device.hip after hsfft_stft.h: the driver launches its kernels
 * directly, so no host C file needs a new device-layer symbol.
 *
 * Makhoul's N-point algorithm around the unchanged row transforms.  Type 2: one kernel permutes
 * every row (even samples ascending, odd samples descending) into a scratch of rows of N,
 * hs_r2c_rows() writes their compact spectra into a second scratch, and one kernel rotates bin k
 * by the table's (cos, sin)(pi k / 2N) and writes the two outputs it gives.  Type 3 runs the same
 * steps backwards: rotate pairs of inputs into N/2+1 bins, hs_c2r_rows(), undo the permutation.
 * The sine transforms are index and sign variants inside the same kernels.  Both
 * scratch buffers are bounded by HSFFT_DCT_CHUNK_MB, not by the job.  The table and the cache of
 * its device copies are host C on the device layer's interface: hsfft_dct.c.
 */
#include "hsfft_gpu.h"
#include "hsfft_host.h"

namespace dct {

/* the sign bit flipped, of zeros and NaNs too: no arithmetic */
__device__ __forceinline__ double flip(double x)
{
    return __longlong_as_double(__double_as_longlong(x) ^ (long long)0x8000000000000000ULL);
}

/* Type 2, before the r2c: v[j] = x[2j], v[N-1-j] = x[2j+1] for j < h = N/2; SIN flips the sign
 * bit of the odd samples.  Row yi of the launch.  A lane owns the source pair: one 16-byte load
 * where the row is 16-byte aligned (rows are N x 8 bytes, N even, so all rows are or none is), two
 * 8-byte loads otherwise.  The stores are 8 bytes each; both streams, ascending from v and
 * descending from v + N - 1, are contiguous across the wave. */
template <bool SIN>
__global__ __launch_bounds__(256) void k_dct2_pre(const double *__restrict__ x, double *__restrict__ v, long long N)
{
    const long long h = N / 2;
    const double *xrow = x + blockIdx.y * N;
    double *vrow = v + blockIdx.y * N;
    const bool al = ((uintptr_t)xrow & 15) == 0;
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < h; j += (long long)gridDim.x * blockDim.x) {
        v2d p;
        if (al) p = *(const v2d *)(xrow + 2 * j);
        else {
            p.x = xrow[2 * j];
            p.y = xrow[2 * j + 1];
        }
        vrow[j] = p.x;
        vrow[N - 1 - j] = SIN ? flip(p.y) : p.y;
    }
}

/* Type 2, after the r2c: a lane owns bin k <= h of row yi.  With V = S[yi][k] and (c, s) = t[k]:
 * re = V.re c + V.im s, im = V.im c - V.re s, every operation rounded on its own (the file's
 * -ffp-contract=off) and computed for every k, k = 0 and k = h included.  2 re goes to out[k] and,
 * for 1 <= k < h, -2 im to out[N-k]; SIN reverses the row: out[N-1-k] and out[k-1].  16-byte loads
 * of the bin and of the table word; 8-byte stores, because the caller's rows need the alignment
 * of a double only and the two destinations are N - 2k words apart.  Both store streams are
 * contiguous across the wave. */
template <bool SIN>
__global__ __launch_bounds__(256) void k_dct2_post(const v2d *__restrict__ S, const v2d *__restrict__ t,
                                                   double *__restrict__ out, long long N)
{
    const long long h = N / 2;
    const v2d *srow = S + blockIdx.y * (h + 1);
    double *orow = out + blockIdx.y * N;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k <= h; k += (long long)gridDim.x * blockDim.x) {
        const v2d V = srow[k], w = t[k];
        const double re = V.x * w.x + V.y * w.y;
        const double im = V.y * w.x - V.x * w.y;
        orow[SIN ? N - 1 - k : k] = 2.0 * re;
        if (k >= 1 && k < h) orow[SIN ? k - 1 : N - k] = -2.0 * im;
    }
}

/* Type 3, before the c2r: a lane owns bin k <= h of row yi.  V[0] = (X[0], +0.0) with no
 * arithmetic; for k >= 1, with a = X[k], b = X[N-k] and (c, s) = t[k]: V[k] = (a c + b s, a s - b c),
 * every operation rounded on its own.  SIN reads the row reversed: X[N-1], and a = X[N-1-k], b =
 * X[k-1].  8-byte loads (two streams, contiguous across the wave), one 16-byte store. */
template <bool SIN>
__global__ __launch_bounds__(256) void k_dct3_pre(const double *__restrict__ X, const v2d *__restrict__ t,
                                                  v2d *__restrict__ S, long long N)
{
    const long long h = N / 2;
    const double *xrow = X + blockIdx.y * N;
    v2d *srow = S + blockIdx.y * (h + 1);
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k <= h; k += (long long)gridDim.x * blockDim.x) {
        v2d V;
        if (k == 0) {
            V.x = xrow[SIN ? N - 1 : 0];
            V.y = 0.0;
        } else {
            const double a = xrow[SIN ? N - 1 - k : k], b = xrow[SIN ? k - 1 : N - k];
            const v2d w = t[k];
            V.x = a * w.x + b * w.y;
            V.y = a * w.y - b * w.x;
        }
        srow[k] = V;
    }
}

/* Type 3, after the c2r: out[2j] = y[j], out[2j+1] = y[N-1-j] for j < h; SIN flips the sign bit
 * of the odd samples.  A lane owns the destination pair: one 16-byte store where the caller's row
 * is 16-byte aligned, two 8-byte stores otherwise. */
template <bool SIN>
__global__ __launch_bounds__(256) void k_dct3_post(const double *__restrict__ y, double *__restrict__ out, long long N)
{
    const long long h = N / 2;
    const double *yrow = y + blockIdx.y * N;
    double *orow = out + blockIdx.y * N;
    const bool al = ((uintptr_t)orow & 15) == 0;
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < h; j += (long long)gridDim.x * blockDim.x) {
        v2d p;
        p.x = yrow[j];
        p.y = SIN ? flip(yrow[N - 1 - j]) : yrow[N - 1 - j];
        if (al) *(v2d *)(orow + 2 * j) = p;
        else {
            orow[2 * j] = p.x;
            orow[2 * j + 1] = p.y;
        }
    }
}

constexpr long long MAX_WORDS = 1LL << 40; /* n x batch */

static int dev_rc(int rc, const char *what)
{
    if (rc) hs_seterr("%s: %s", what, hsd_errstr());
    return rc ? HSFFT_ERR_DEVICE : 0;
}

/* one of the four kernels on `rows` rows, in slices of Y_MAX rows; a, b: the kernel's input and
 * output, rows of `apitch` and `bpitch` words of their own type */
template <typename KA, typename KB, typename F>
static int launch(F fn, const KA *a, long long apitch, KB *b, long long bpitch, long long items, long long rows)
{
    for (long long b0 = 0; b0 < rows; b0 += Y_MAX) {
        const int nb = (int)(rows - b0 < Y_MAX ? rows - b0 : Y_MAX);
        fn(dim3(grid_for(items, 256), nb), a + b0 * apitch, b + b0 * bpitch);
        HCHK(hipGetLastError());
    }
    return 0;
}

static int pre2(int sin, const double *x, double *v, long long N, long long rows)
{
    return launch([=](dim3 g, const double *a, double *b) {
        if (sin) hipLaunchKernelGGL(k_dct2_pre<true>, g, dim3(256), 0, stream(), a, b, N);
        else hipLaunchKernelGGL(k_dct2_pre<false>, g, dim3(256), 0, stream(), a, b, N);
    }, x, N, v, N, N / 2, rows);
}

static int post2(int sin, const v2d *S, const v2d *t, double *out, long long N, long long rows)
{
    return launch([=](dim3 g, const v2d *a, double *b) {
        if (sin) hipLaunchKernelGGL(k_dct2_post<true>, g, dim3(256), 0, stream(), a, t, b, N);
        else hipLaunchKernelGGL(k_dct2_post<false>, g, dim3(256), 0, stream(), a, t, b, N);
    }, S, N / 2 + 1, out, N, N / 2 + 1, rows);
}

static int pre3(int sin, const double *X, const v2d *t, v2d *S, long long N, long long rows)
{
    return launch([=](dim3 g, const double *a, v2d *b) {
        if (sin) hipLaunchKernelGGL(k_dct3_pre<true>, g, dim3(256), 0, stream(), a, t, b, N);
        else hipLaunchKernelGGL(k_dct3_pre<false>, g, dim3(256), 0, stream(), a, t, b, N);
    }, X, N, S, N / 2 + 1, N / 2 + 1, rows);
}

static int post3(int sin, const double *y, double *out, long long N, long long rows)
{
    return launch([=](dim3 g, const double *a, double *b) {
        if (sin) hipLaunchKernelGGL(k_dct3_post<true>, g, dim3(256), 0, stream(), a, b, N);
        else hipLaunchKernelGGL(k_dct3_post<false>, g, dim3(256), 0, stream(), a, b, N);
    }, y, N, out, N, N / 2, rows);
}

/* (device lock held) the call.  Rows are walked in chunks of `c` with two pool buffers, R (c x N
 * doubles: the permuted rows, or the c2r's output) and S (c x (N/2+1) complex: the compact
 * spectra).  Per chunk, type 2: permute x -> R, r2c-compact R -> S, rotate S -> out; type 3: rotate
 * X -> S, c2r S -> R at the pitch N/2+1, permute R -> out. */
static int run(int dev, int sin, int type, fft_real_object f, fft_real_object g, const fft_type *d_in, fft_type *d_out,
               int n, int batch)
{
    const long long N = n, bins = N / 2 + 1;
    const size_t per = sizeof(double) * (size_t)N + sizeof(fft_data) * (size_t)bins;
    long long c = (long long)(hs_env_mb("HSFFT_DCT_CHUNK_MB", 1024.0) / per);
    if (c > batch) c = batch;
    if (c < 1) c = 1;
    double *R;
    fft_data *S;
    for (;;) {
        R = (double *)hs_scratch(HS_SCR_DCT, sizeof(double) * (size_t)N * (size_t)c);
        S = R ? (fft_data *)hs_scratch(HS_SCR_DCT_SPEC, sizeof(fft_data) * (size_t)bins * (size_t)c) : NULL;
        if (S || c == 1) break;
        c = (c + 1) / 2;
    }
    if (!S) {
        hs_seterr("hsfft_dct_batched: scratch allocation failed (%lld rows of %lld)", c, N);
        return HSFFT_ERR_NOMEM;
    }
    const v2d *t = (const v2d *)hs_dct_table(dev, n);
    if (!t) return HSFFT_ERR_DEVICE;
    int rc = 0;
    for (long long b0 = 0; b0 < batch && !rc; b0 += c) {
        const long long rows = batch - b0 < c ? batch - b0 : c;
        const double *in = d_in + b0 * N;
        double *out = d_out + b0 * N;
        if (type == 2) {
            rc = dev_rc(pre2(sin, in, R, N, rows), "dct permutation");
            if (!rc) rc = hs_r2c_rows(f, R, S, (int)rows, 1);
            if (!rc) rc = dev_rc(post2(sin, (const v2d *)S, t, out, N, rows), "dct rotation");
        } else {
            rc = dev_rc(pre3(sin, in, t, (v2d *)S, N, rows), "dct rotation");
            if (!rc) rc = hs_c2r_rows(g, S, NULL, bins, R, (int)rows);
            if (!rc) rc = dev_rc(post3(sin, R, out, N, rows), "dct permutation");
        }
    }
    return rc;
}

}  // namespace dct

extern "C" {

int hsfft_dct_batched(int kind, int type, const fft_type *d_in, fft_type *d_out, int n, int batch)
{
    hs_seterr("%s", "");
    if ((kind != HSFFT_KIND_COS && kind != HSFFT_KIND_SIN) || (type != 2 && type != 3)) {
        hs_seterr("hsfft_dct_batched: kind %d is not 0 (cosine) or 1 (sine), or type %d is not 2 or 3", kind, type);
        return HSFFT_ERR_ARG;
    }
    if (n < 2 || (n & 1) || n > HS_DCT_MAX_LEN) {
        hs_seterr("hsfft_dct_batched: the length %d is odd, below 2 or above 2^30", n);
        return HSFFT_ERR_ARG;
    }
    if (!d_in || !d_out || batch < 0) {
        hs_seterr("hsfft_dct_batched: NULL pointer or negative batch");
        return HSFFT_ERR_ARG;
    }
    if ((long long)n * batch > dct::MAX_WORDS) {
        hs_seterr("hsfft_dct_batched: %d rows of %d are more than the call can index", batch, n);
        return HSFFT_ERR_ARG;
    }
    const uintptr_t bytes = sizeof(fft_type) * (uintptr_t)n * (uintptr_t)batch;
    if (batch && (d_in == d_out || tr2d::overlap_bytes(d_out, bytes, d_in, bytes))) {
        hs_seterr("hsfft_dct_batched: the output overlaps the input");
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    int rc = hs_require_gpu();
    if (rc) return rc;
    const hs_conv_pair rp = hs_conv_plans(n);
    if (!rp.f || !rp.i) {
        hs_seterr("hsfft_dct_batched: planning the length %d failed", n);
        rc = HSFFT_ERR_NOMEM;
    } else {
        const int d = hs_lock_device();
        rc = dct::run(d, kind == HSFFT_KIND_SIN, type, rp.f, rp.i, d_in, d_out, n, batch);
        hs_unlock_device(d);
    }
    hs_conv_plans_done(rp);
    return rc;
}

}  // extern "C"
