/*
 * hsfft_czt.h -- batched chirp-z transform (zoom FFT) of real and complex rows on the unit circle
 * (hsfft_czt_batched, hsfft_czt_real_batched of include/hsfft_gpu.h; the reference has none).
 * Included at the end of hsfft_device.hip after hsfft_dct4.h: the drivers launch their kernels
 * directly, so no host C file needs a new device-layer symbol.
 *
 * Bluestein's algorithm around the unchanged power-of-two row transforms: j k = (j^2 + k^2 - (k-j)^2)
 * / 2 turns the m sums over n samples into one circular convolution of length L >= n + m - 1 with a
 * chirp.  One kernel rotates every sample by the table `pre` and zero-fills up to L, hs_c2c_rows()
 * transforms the rows, one kernel multiplies them by the chirp's spectrum V (one row, shared by all,
 * transformed once per cache entry), hs_c2c_rows() transforms back, and one kernel scales the first
 * m words by 1/L, rotates them by the table `chirp` and writes the caller's rows.
 * Nothing is fused into a transform pass.  The scratch buffers are bounded by HSFFT_CZT_CHUNK_MB,
 * not by the job.  The tables, their exact phase reduction and the cache of device copies are host
 * C: hsfft_czt.c.
 */
#include "hsfft_gpu.h"
#include "hsfft_host.h"

namespace czt {

using dct::flip;

/* Before the forward transform: u[j] = rot_in(x[j].re, x[j].im, pre[j]) for j < n and (+0.0, +0.0)
 * for n <= j < L, into row yi of the scratch.  A real sample gives (x c, -(x s)): two multiplies
 * and a flip of the sign bit, no add.
 * Complex rows: a lane owns word j; the caller's sample is one 16-byte load where the rows are
 * 16-byte aligned (they are n x 16 bytes, so all are or none is) and 8 + 8 otherwise.
 * Real rows: a lane loads the samples 2p and 2p+1 -- 16 bytes where that address is 16-byte
 * aligned (rows are n x 8 bytes: with an odd n every other row is) and 8 + 8 otherwise -- and the
 * wave's 128 samples are then dealt out across its lanes, so that lane l stores the words W + l and
 * W + 64 + l: two store streams and two table streams, each contiguous across the wave, where a
 * lane that kept its own two samples would store 16 bytes at a stride of 32.  The loop bound is
 * uniform over a wave (256 threads = 4 whole waves), as the exchange needs. */
template <bool REAL>
__global__ __launch_bounds__(256) void k_czt_pre(const double *__restrict__ x, const v2d *__restrict__ pre,
                                                 v2d *__restrict__ z, long long n, long long L)
{
    v2d *zrow = z + blockIdx.y * L;
    if (REAL) {
        const double *xrow = x + blockIdx.y * n;
        const bool al = ((uintptr_t)xrow & 15) == 0;
        const int lane = threadIdx.x & 63;
        const long long half = L / 2;
        for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p - lane < half;
             p += (long long)gridDim.x * blockDim.x) {
            v2d a;
            a.x = 0.0;
            a.y = 0.0;
            if (2 * p + 1 < n) {
                if (al) a = *(const v2d *)(xrow + 2 * p);
                else {
                    a.x = xrow[2 * p];
                    a.y = xrow[2 * p + 1];
                }
            } else if (2 * p < n) a.x = xrow[2 * p];
            /* both table words are requested before the exchange waits for the samples */
            const long long j0 = 2 * (p - lane) + lane, j1 = j0 + 64;
            v2d w[2];
            w[0].x = w[0].y = w[1].x = w[1].y = 0.0;
            if (j0 < n) w[0] = pre[j0];
            if (j1 < n) w[1] = pre[j1];
#pragma unroll
            for (int hh = 0; hh < 2; hh++) {
                const int src = 32 * hh + (lane >> 1);
                const double ex = __shfl(a.x, src, 64), ey = __shfl(a.y, src, 64);
                const double xv = (lane & 1) ? ey : ex;
                const long long j = hh ? j1 : j0;
                v2d u;
                u.x = j < n ? xv * w[hh].x : 0.0;
                u.y = j < n ? flip(xv * w[hh].y) : 0.0;
                if (j < L) zrow[j] = u;
            }
        }
    } else {
        const double *xrow = x + blockIdx.y * 2 * n;
        const bool al = ((uintptr_t)xrow & 15) == 0;
        for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < L; j += (long long)gridDim.x * blockDim.x) {
            v2d u;
            u.x = 0.0;
            u.y = 0.0;
            if (j < n) {
                v2d a;
                if (al) a = *(const v2d *)(xrow + 2 * j);
                else {
                    a.x = xrow[2 * j];
                    a.y = xrow[2 * j + 1];
                }
                u = dct4::rot_in(a.x, a.y, pre[j]);
            }
            zrow[j] = u;
        }
    }
}

/* Between the transforms: P[i] = cmul1(U[i], V[i]) in place on the chunk's spectra, the row's
 * spectrum as the left operand.  V is L x 16 bytes read by every row: it is served from L2 or the
 * Infinity Cache, so the kernel's HBM traffic is the rows', once in and once out.  (A form whose
 * lanes kept V[i] in registers across four rows was measured and was no faster: DESIGN.md §16.) */
__global__ __launch_bounds__(256) void k_czt_mul(v2d *__restrict__ U, const v2d *__restrict__ V, long long L)
{
    v2d *urow = U + blockIdx.y * L;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < L; i += (long long)gridDim.x * blockDim.x) {
        const v2d a = urow[i], c = V[i];
        v2d p;
        p.x = a.x * c.x - a.y * c.y;
        p.y = a.x * c.y + a.y * c.x;
        urow[i] = p;
    }
}

/* After the inverse transform: d = y[k] / L per component, X[k] = rot_in(d.re, d.im, chirp[k]) for k <
 * m of row yi; the words m .. L-1 of the row are not read.  L is a power of two up to 2^26, so its
 * reciprocal `inv` is exact and d = y * inv is the correctly rounded quotient, bit for bit, of
 * zeros, subnormals, infinities and NaNs too: one multiply where the division would expand into a
 * sequence with fused operations.  The caller's word is one 16-byte store where the rows are 16-byte
 * aligned (m x 16 bytes each: all are or none is) and 8 + 8 otherwise. */
__global__ __launch_bounds__(256) void k_czt_post(const v2d *__restrict__ y, const v2d *__restrict__ chirp,
                                                  double *__restrict__ out, long long m, long long L, double inv)
{
    const v2d *yrow = y + blockIdx.y * L;
    double *orow = out + blockIdx.y * 2 * m;
    const bool al = ((uintptr_t)orow & 15) == 0;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < m; k += (long long)gridDim.x * blockDim.x) {
        const v2d v = yrow[k];
        const v2d X = dct4::rot_in(v.x * inv, v.y * inv, chirp[k]);
        if (al) *(v2d *)(orow + 2 * k) = X;
        else {
            orow[2 * k] = X.x;
            orow[2 * k + 1] = X.y;
        }
    }
}

template <bool REAL>
static int pre(const double *x, const v2d *t, v2d *z, long long n, long long L, long long rows)
{
    return dct::launch([=](dim3 g, const double *a, v2d *b) {
        hipLaunchKernelGGL(k_czt_pre<REAL>, g, dim3(256), 0, stream(), a, t, b, n, L);
    }, x, REAL ? n : 2 * n, z, L, REAL ? L / 2 : L, rows);
}

static int mul(v2d *U, const v2d *V, long long L, long long rows)
{
    return dct::launch([=](dim3 g, const v2d *, v2d *b) {
        hipLaunchKernelGGL(k_czt_mul, g, dim3(256), 0, stream(), b, V, L);
    }, (const v2d *)U, L, U, L, L, rows);
}

static int post(const v2d *y, const v2d *t, double *out, long long m, long long L, long long rows)
{
    return dct::launch([=](dim3 g, const v2d *a, double *b) {
        hipLaunchKernelGGL(k_czt_post, g, dim3(256), 0, stream(), a, t, b, m, L, 1.0 / (double)L);
    }, y, L, out, 2 * m, m, rows);
}

/* (device lock held) `batch` rows of n: ef and eg are the forward and the inverse c2c plan of length
 * L.  Rows are walked in chunks of `c` with two pool buffers of c x L complex each, z (u, then y) and
 * Z (U, then P).  A cache entry that is new first has its v transformed into its V.  Per chunk:
 * rotate and zero-fill in -> z, rows z -> Z, Z *= V, rows Z -> z, scale and rotate z -> out. */
template <bool REAL>
static int run(const char *who, int dev, hs_entry *ef, hs_entry *eg, const double *d_in, fft_data *d_out, int n, int m, int L,
               double f0, double df, long long batch)
{
    const size_t row = sizeof(fft_data) * (size_t)L;
    long long c = (long long)(hs_env_mb("HSFFT_CZT_CHUNK_MB", 1024.0) / (2 * row));
    if (c > batch) c = batch;
    if (c < 1) c = 1;
    fft_data *z, *Z;
    for (;;) {
        z = (fft_data *)hs_scratch(HS_SCR_CZT, row * (size_t)c);
        Z = z ? (fft_data *)hs_scratch(HS_SCR_CZT_SPEC, row * (size_t)c) : NULL;
        if (Z || c == 1) break;
        c = (c + 1) / 2;
    }
    if (!Z) {
        hs_seterr("%s: scratch allocation failed (%lld rows of %d)", who, c, L);
        return HSFFT_ERR_NOMEM;
    }
    hs_czt_data t;
    int rc = hs_czt_get(dev, n, m, L, f0, df, hsfft_get_twiddle_mode(), &t);
    if (rc) return rc;
    if (!t.ready) {
        rc = tr2d::rows(ef, t.v, t.V, 1);
        if (rc) return rc;
        hs_czt_set_ready(dev, t.slot);
    }
    for (long long b0 = 0; b0 < batch && !rc; b0 += c) {
        const long long rows = batch - b0 < c ? batch - b0 : c;
        rc = dct::dev_rc(pre<REAL>(d_in + b0 * (REAL ? n : 2LL * n), (const v2d *)t.pre, (v2d *)z, n, L, rows),
                         "czt input rotation");
        if (!rc) rc = tr2d::rows(ef, z, Z, rows);
        if (!rc) rc = dct::dev_rc(mul((v2d *)Z, (const v2d *)t.V, L, rows), "czt spectral product");
        if (!rc) rc = tr2d::rows(eg, Z, z, rows);
        if (!rc) rc = dct::dev_rc(post((const v2d *)z, (const v2d *)t.chirp, (double *)(d_out + b0 * m), m, L, rows),
                                  "czt output rotation");
    }
    return rc;
}

/* both entry points: the argument checks, then the GPU, the plan pair of length L from the
 * convolution plan cache (it follows the calling thread's twiddle mode, and a repeated length
 * builds nothing) and the device lock around run() */
template <bool REAL>
static int call(const char *who, const void *d_in, int n, fft_data *d_out, int m, double f0, double df, int batch)
{
    hs_seterr("%s", "");
    if (!d_in || !d_out || batch < 0) {
        hs_seterr("%s: NULL pointer or negative batch", who);
        return HSFFT_ERR_ARG;
    }
    int L;
    int rc = hs_czt_sizes(who, n, m, &L);
    if (!rc) rc = hs_czt_freqs(who, f0, df);
    if (rc) return rc;
    if ((long long)n * batch > dct::MAX_WORDS || (long long)m * batch > dct::MAX_WORDS || (long long)L * batch > dct::MAX_WORDS) {
        hs_seterr("%s: %d rows of %d, %d or the padded %d are more than the call can index", who, batch, n, m, L);
        return HSFFT_ERR_ARG;
    }
    const uintptr_t nb = (uintptr_t)batch;
    if (tr2d::overlap_bytes(d_out, sizeof(fft_data) * (uintptr_t)m * nb, d_in,
                            (REAL ? sizeof(fft_type) : sizeof(fft_data)) * (uintptr_t)n * nb)) {
        hs_seterr("%s: the output overlaps the input", who);
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    rc = hs_require_gpu();
    if (rc) return rc;
    const hs_conv_cpair cp = hs_conv_cplans(L);
    if (!cp.f || !cp.i) {
        hs_seterr("%s: planning the length %d failed", who, L);
        rc = HSFFT_ERR_NOMEM;
    } else {
        const int d = hs_lock_device();
        hs_entry *ef = hs_entry_get(cp.f), *eg = hs_entry_get(cp.i);
        rc = ef && eg ? run<REAL>(who, d, ef, eg, (const double *)d_in, d_out, n, m, L, f0, df, batch) : HSFFT_ERR_ARG;
        hs_entry_put(eg);
        hs_entry_put(ef);
        hs_unlock_device(d);
    }
    hs_conv_cplans_done(cp);
    return rc;
}

}  // namespace czt

extern "C" {

int hsfft_czt_batched(const fft_data *d_in, int n, fft_data *d_out, int m, double f0, double df, int batch)
{
    return czt::call<false>("hsfft_czt_batched", d_in, n, d_out, m, f0, df, batch);
}

int hsfft_czt_real_batched(const fft_type *d_in, int n, fft_data *d_out, int m, double f0, double df, int batch)
{
    return czt::call<true>("hsfft_czt_real_batched", d_in, n, d_out, m, f0, df, batch);
}

}  // extern "C"
