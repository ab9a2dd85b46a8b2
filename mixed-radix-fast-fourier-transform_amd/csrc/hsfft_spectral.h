/*
 * hsfft_spectral.h -- batched analytic signal (scipy.signal.hilbert) and Fourier resampling
 * (scipy.signal.resample) of real rows (hsfft_hilbert_batched, hsfft_resample_batched of
 * include/hsfft_gpu.h; the reference has neither).
 * Included at the end of hsfft_device.hip after hsfft_czt.h: the drivers launch their kernels
 * directly, so no host C file needs a new device-layer symbol.
 *
 * Both are r2c, an edit of the compact spectrum, and an inverse transform, around the unchanged row
 * transforms: hs_r2c_rows() writes a chunk's compact spectra S into one pool buffer, one kernel
 * writes the edited spectra -- scaled by 1 / n with a true division -- into a second, and the
 * inverse row transform (c2c of n words for the analytic signal, c2r of m reals for resampling)
 * writes from there straight into the caller's rows: there is no pass after it.
 * Nothing is fused into a transform pass.  Both scratch buffers are bounded by
 * HSFFT_SPECTRAL_CHUNK_MB, not by the job.  The argument rules and the chunk rule are host C:
 * hsfft_spectral.c.
 */
#include "hsfft_gpu.h"
#include "hsfft_host.h"

namespace spec {

static_assert(HS_SPECTRAL_MAX_WORDS == dct::MAX_WORDS, "the host file's bound on the totals is dct::MAX_WORDS");

/* The analytic signal's spectrum: a lane owns the word k < n of row yi of Z.  For k <= n/2 one
 * 16-byte load of S[k]; the gain of the bins 0 < k < n/2 is the add S + S (exact unless it
 * overflows), then the two divisions by dn = (double)n; the words above n/2 are stored as (+0.0,
 * +0.0) and load nothing.  One 16-byte store per word, contiguous across the wave.  Both sides are
 * pool scratch: 16-byte aligned, row pitches of n/2+1 and n words of 16 bytes.  The division is the
 * IEEE quotient, as in k_istft_ola: a multiply by the rounded reciprocal would differ wherever n is
 * no power of two.  Compiled under the file's -ffp-contract=off. */
__global__ __launch_bounds__(256) void k_hilbert_spec(const v2d *__restrict__ S, v2d *__restrict__ Z, long long n, double dn)
{
    const long long h = n / 2;
    const v2d *srow = S + blockIdx.y * (h + 1);
    v2d *zrow = Z + blockIdx.y * n;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
        v2d z;
        z.x = 0.0;
        z.y = 0.0;
        if (k <= h) {
            v2d a = srow[k];
            if (k > 0 && k < h) {
                a.x = a.x + a.x;
                a.y = a.y + a.y;
            }
            z.x = a.x / dn;
            z.y = a.y / dn;
        }
        zrow[k] = z;
    }
}

/* The resampled row's spectrum: a lane owns the word k <= m/2 of row yi of Y.  With K = min(n, m) / 2:
 * S[k] / dn below K; at K the bin itself (m == n), half of it (m > n: the bin is shared with its
 * mirror, which the longer spectrum holds apart) or twice its real part with the imaginary part
 * +0.0 (m < n: the bin and its mirror fold onto the new Nyquist bin, and the c2r reads that word's
 * imaginary part); (+0.0, +0.0) above K.  One 16-byte load where k <= K, one 16-byte store.  The
 * halving is exact unless it underflows and the doubling unless it overflows; the division is the
 * IEEE quotient by dn = (double)n. */
__global__ __launch_bounds__(256) void k_resample_spec(const v2d *__restrict__ S, v2d *__restrict__ Y, long long n, long long m,
                                                       double dn)
{
    const long long hm = m / 2, K = (n < m ? n : m) / 2;
    const v2d *srow = S + blockIdx.y * (n / 2 + 1);
    v2d *yrow = Y + blockIdx.y * (hm + 1);
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k <= hm; k += (long long)gridDim.x * blockDim.x) {
        v2d y;
        y.x = 0.0;
        y.y = 0.0;
        if (k <= K) {
            v2d a = srow[k];
            if (k < K || m == n) {
                y.x = a.x / dn;
                y.y = a.y / dn;
            } else if (m > n) {
                y.x = (0.5 * a.x) / dn;
                y.y = (0.5 * a.y) / dn;
            } else y.x = (a.x + a.x) / dn;
        }
        yrow[k] = y;
    }
}

static int hilbert_spec(const v2d *S, v2d *Z, long long n, long long rows)
{
    return dct::launch([=](dim3 g, const v2d *a, v2d *b) {
        hipLaunchKernelGGL(k_hilbert_spec, g, dim3(256), 0, stream(), a, b, n, (double)n);
    }, S, n / 2 + 1, Z, n, n, rows);
}

static int resample_spec(const v2d *S, v2d *Y, long long n, long long m, long long rows)
{
    return dct::launch([=](dim3 g, const v2d *a, v2d *b) {
        hipLaunchKernelGGL(k_resample_spec, g, dim3(256), 0, stream(), a, b, n, m, (double)n);
    }, S, n / 2 + 1, Y, m / 2 + 1, m / 2 + 1, rows);
}

/* (device lock held) `batch` rows of n.  f: the forward real plan of n.  ei != NULL: the analytic
 * signal, ei the inverse c2c plan of n and d_out rows of n complex; else resampling, g the inverse
 * real plan of m and d_out rows of m reals.  Rows are walked in chunks of `c` with two pool buffers,
 * S (c x (n/2+1) complex) and E (c x n complex, or c x (m/2+1)).  Per chunk: r2c-compact in -> S,
 * edit S -> E, inverse rows E -> out. */
static int run(const char *who, fft_real_object f, hs_entry *ei, fft_real_object g, const fft_type *d_in, void *d_out, int n,
               int m, long long batch)
{
    const size_t sw = (size_t)n / 2 + 1, ew = ei ? (size_t)n : (size_t)m / 2 + 1;
    long long c = hs_spectral_rows(n, ei ? 0 : m);
    if (c > batch) c = batch;
    fft_data *S, *E;
    for (;;) {
        S = (fft_data *)hs_scratch(HS_SCR_SPECTRAL, sizeof(fft_data) * sw * (size_t)c);
        E = S ? (fft_data *)hs_scratch(HS_SCR_SPECTRAL_SPEC, sizeof(fft_data) * ew * (size_t)c) : NULL;
        if (E || c == 1) break;
        c = (c + 1) / 2;
    }
    if (!E) {
        hs_seterr("%s: scratch allocation failed (%lld rows of %d)", who, c, n);
        return HSFFT_ERR_NOMEM;
    }
    int rc = 0;
    for (long long b0 = 0; b0 < batch && !rc; b0 += c) {
        const long long rows = batch - b0 < c ? batch - b0 : c;
        rc = hs_r2c_rows(f, d_in + b0 * n, S, (int)rows, 1);
        if (rc) break;
        if (ei) {
            rc = dct::dev_rc(hilbert_spec((const v2d *)S, (v2d *)E, n, rows), "analytic-signal spectrum");
            if (!rc) rc = tr2d::rows(ei, E, (fft_data *)d_out + b0 * n, rows);
        } else {
            rc = dct::dev_rc(resample_spec((const v2d *)S, (v2d *)E, n, m, rows), "resampled spectrum");
            if (!rc) rc = hs_c2r_rows(g, E, NULL, (long long)ew, (fft_type *)d_out + b0 * m, (int)rows);
        }
    }
    return rc;
}

}  // namespace spec

extern "C" {

int hsfft_hilbert_batched(const fft_type *d_in, fft_data *d_out, int n, int batch)
{
    const char *who = "hsfft_hilbert_batched";
    hs_seterr("%s", "");
    int rc = hs_spectral_args(who, d_in, n, d_out, 0, batch, 1);
    if (rc || batch == 0) return rc;
    rc = hs_require_gpu();
    if (rc) return rc;
    const hs_conv_pair rp = hs_conv_plans(n);
    const hs_conv_cpair cp = hs_conv_cplans(n);
    if (!rp.f || !cp.i) {
        hs_seterr("%s: planning the length %d failed", who, n);
        rc = HSFFT_ERR_NOMEM;
    } else {
        const int d = hs_lock_device();
        hs_entry *ei = hs_entry_get(cp.i);
        rc = ei ? spec::run(who, rp.f, ei, NULL, d_in, d_out, n, 0, batch) : HSFFT_ERR_ARG;
        hs_entry_put(ei);
        hs_unlock_device(d);
    }
    hs_conv_cplans_done(cp);
    hs_conv_plans_done(rp);
    return rc;
}

int hsfft_resample_batched(const fft_type *d_in, int n, fft_type *d_out, int m, int batch)
{
    const char *who = "hsfft_resample_batched";
    hs_seterr("%s", "");
    int rc = hs_spectral_args(who, d_in, n, d_out, m, batch, 0);
    if (rc || batch == 0) return rc;
    rc = hs_require_gpu();
    if (rc) return rc;
    const hs_conv_pair rn = hs_conv_plans(n), rm = hs_conv_plans(m);
    if (!rn.f || !rm.i) {
        hs_seterr("%s: planning the lengths %d and %d failed", who, n, m);
        rc = HSFFT_ERR_NOMEM;
    } else {
        const int d = hs_lock_device();
        rc = spec::run(who, rn.f, NULL, rm.i, d_in, d_out, n, m, batch);
        hs_unlock_device(d);
    }
    hs_conv_plans_done(rm);
    hs_conv_plans_done(rn);
    return rc;
}

}  // extern "C"
