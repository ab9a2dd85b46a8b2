/*
 * hsfft_dct1.h -- batched DCT-I / DST-I of real rows and of real images (hsfft_dct1_batched,
 * hsfft_dct1_2d_batched of include/hsfft_gpu.h; the reference has no cosine or sine transform).
 * Included at the end of hsfft_device.hip after hsfft_spectral.h: the drivers launch their kernels
 * directly, so no host C file needs a new device-layer symbol.
 *
 * Symmetric extension around the unchanged r2c row transform (FFTW's reodft00e-r2hc-pad, pocketfft):
 * one kernel writes every row's even (cosine, L = 2(n-1)) or odd (sine, L = 2(n+1)) extension into a
 * scratch of rows of L, hs_r2c_rows() writes their compact spectra into a second scratch, and one
 * kernel copies the real parts of the bins 0..n-1 (cosine) or the sign-flipped imaginary parts of
 * the bins 1..n (sine) into the caller's rows.  L is even for every n, so this
 * family has no evenness rule.  Neither kernel does arithmetic; nothing is fused into a transform
 * pass; there is no table.  Both scratch buffers are bounded by HSFFT_DCT_CHUNK_MB, not by the job.
 * The argument rules, the shape helper and the chunk rule are host C: hsfft_dct1.c.
 */
#include "hsfft_gpu.h"
#include "hsfft_host.h"

namespace dct1 {

static_assert(HS_DCT1_MAX_WORDS == dct::MAX_WORDS, "the host file's bound on the totals is dct::MAX_WORDS");

/* Before the r2c: a lane owns the source sample j < n of row yi.  One 8-byte load from the caller's
 * row -- rows of odd n alternate between 8- and 16-byte alignment, so nothing wider -- and two
 * 8-byte stores into the scratch row e of L doubles, the ascending copy and the mirrored one; both
 * store streams are contiguous across the wave.
 *   cosine, L = 2(n-1): e[j] = x[j]; e[L-j] = x[j] for 1 <= j <= n-2 (the two ends have no mirror)
 *   sine,   L = 2(n+1): e[j+1] = x[j]; e[L-1-j] = x[j] with the sign bit flipped (dct::flip: zeros
 *                       and NaNs too); the lane of j == 0 also stores e[0] = e[n+1] = +0.0
 * Every word of the scratch row is written: the pool class holds other calls' leftovers. */
template <bool SIN>
__global__ __launch_bounds__(256) void k_dct1_pre(const double *__restrict__ x, double *__restrict__ e, long long n, long long L)
{
    const double *xrow = x + blockIdx.y * n;
    double *erow = e + blockIdx.y * L;
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x) {
        const double v = xrow[j];
        if (SIN) {
            erow[j + 1] = v;
            erow[L - 1 - j] = dct::flip(v);
            if (j == 0) {
                erow[0] = 0.0;
                erow[n + 1] = 0.0;
            }
        } else {
            erow[j] = v;
            if (j >= 1 && j <= n - 2) erow[L - j] = v;
        }
    }
}

/* After the r2c: a lane owns the output k < n of row yi.  One 16-byte load of its bin from the
 * scratch row of L/2+1 bins (16-byte aligned) and one 8-byte store of the kept component to the
 * caller's row: Re S[k] (cosine), or Im S[k+1] with the sign bit flipped (sine; S[0] and S[n+1] are
 * not read).  No arithmetic. */
template <bool SIN>
__global__ __launch_bounds__(256) void k_dct1_post(const v2d *__restrict__ S, double *__restrict__ out, long long n, long long bins)
{
    const v2d *srow = S + blockIdx.y * bins;
    double *orow = out + blockIdx.y * n;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
        const v2d V = srow[SIN ? k + 1 : k];
        orow[k] = SIN ? dct::flip(V.y) : V.x;
    }
}

static int pre(int sin, const double *x, double *e, long long n, long long L, long long rows)
{
    return dct::launch([=](dim3 g, const double *a, double *b) {
        if (sin) hipLaunchKernelGGL(k_dct1_pre<true>, g, dim3(256), 0, stream(), a, b, n, L);
        else hipLaunchKernelGGL(k_dct1_pre<false>, g, dim3(256), 0, stream(), a, b, n, L);
    }, x, n, e, L, n, rows);
}

static int post(int sin, const v2d *S, double *out, long long n, long long bins, long long rows)
{
    return dct::launch([=](dim3 g, const v2d *a, double *b) {
        if (sin) hipLaunchKernelGGL(k_dct1_post<true>, g, dim3(256), 0, stream(), a, b, n, bins);
        else hipLaunchKernelGGL(k_dct1_post<false>, g, dim3(256), 0, stream(), a, b, n, bins);
    }, S, bins, out, n, n, rows);
}

/* (device lock held) `batch` rows of n.  f: the forward real plan of Lext.  Rows are walked in chunks
 * of `c` with two pool buffers, R (c x L doubles: the extended rows) and S (c x (L/2+1) complex: the
 * compact spectra).  Per chunk: extend x -> R, r2c-compact R -> S, pick S -> out. */
static int run(const char *who, int sin, fft_real_object f, const fft_type *d_in, fft_type *d_out, int n, int Lext, int batch)
{
    const long long N = n, L = Lext, bins = L / 2 + 1;
    long long c = hs_dct1_rows(Lext);
    if (c > batch) c = batch;
    double *R;
    fft_data *S;
    for (;;) {
        R = (double *)hs_scratch(HS_SCR_DCT, sizeof(double) * (size_t)L * (size_t)c);
        S = R ? (fft_data *)hs_scratch(HS_SCR_DCT_SPEC, sizeof(fft_data) * (size_t)bins * (size_t)c) : NULL;
        if (S || c == 1) break;
        c = (c + 1) / 2;
    }
    if (!S) {
        hs_seterr("%s: scratch allocation failed (%lld rows of %lld)", who, c, L);
        return HSFFT_ERR_NOMEM;
    }
    int rc = 0;
    for (long long b0 = 0; b0 < batch && !rc; b0 += c) {
        const long long rows = batch - b0 < c ? batch - b0 : c;
        rc = dct::dev_rc(pre(sin, d_in + b0 * N, R, N, L, rows), "type-I extension");
        if (!rc) rc = hs_r2c_rows(f, R, S, (int)rows, 1);
        if (!rc) rc = dct::dev_rc(post(sin, (const v2d *)S, d_out + b0 * N, N, bins, rows), "type-I output");
    }
    return rc;
}

/* (device lock held) rows of (sin1, n1) then columns of (sin0, n0) of `batch` n0 x n1 images, per
 * chunk with one scratch copy T of the chunk in HS_SCR_2D -- the shape of dct2d::run: rows in -> T,
 * transpose T -> out, rows out -> T (the columns, now contiguous), transpose T -> out.  d_in is only
 * read.  An image may hold an odd number of doubles: tr2d::chunk_scratch counts 16-byte elements, so
 * it is given the image rounded up to a whole one, ceil(n0 n1 / 2); the chunk then has at least the
 * ci x n0 x n1 doubles that the images, packed without gaps, take. */
static int run_2d(const char *who, int sin0, int sin1, fft_real_object f0, fft_real_object f1, const fft_type *in, fft_type *out,
                  int n0, int L0, int n1, int L1, int batch)
{
    const long long img = (long long)n0 * n1;
    long long ci;
    fft_type *T = (fft_type *)tr2d::chunk_scratch((img + 1) / 2, n0 > n1 ? n0 : n1, 1, batch, &ci);
    if (!T) return HSFFT_ERR_NOMEM;
    for (long long b0 = 0; b0 < batch; b0 += ci) {
        const long long cb = batch - b0 < ci ? batch - b0 : ci;
        const fft_type *ib = in + b0 * img;
        fft_type *ob = out + b0 * img;
        int rc = run(who, sin1, f1, ib, T, n1, L1, (int)(cb * n0));
        if (!rc) rc = tr2d::transpose8(T, ob, n0, n1, cb);
        if (!rc) rc = run(who, sin0, f0, ob, T, n0, L0, (int)(cb * n1));
        if (!rc) rc = tr2d::transpose8(T, ob, n1, n0, cb);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace dct1

extern "C" {

int hsfft_dct1_batched(int kind, const fft_type *d_in, fft_type *d_out, int n, int batch)
{
    const char *who = "hsfft_dct1_batched";
    hs_seterr("%s", "");
    int L;
    int rc = hs_dct1_args(who, kind, d_in, d_out, n, batch, &L);
    if (rc || batch == 0) return rc;
    rc = hs_require_gpu();
    if (rc) return rc;
    const hs_conv_pair rp = hs_conv_plans(L);
    if (!rp.f) {
        hs_seterr("%s: planning the length %d failed", who, L);
        rc = HSFFT_ERR_NOMEM;
    } else {
        const int d = hs_lock_device();
        rc = dct1::run(who, kind == HSFFT_KIND_SIN, rp.f, d_in, d_out, n, L, batch);
        hs_unlock_device(d);
    }
    hs_conv_plans_done(rp);
    return rc;
}

int hsfft_dct1_2d_batched(int kind0, int kind1, const fft_type *d_in, fft_type *d_out, int n0, int n1, int batch)
{
    const char *who = "hsfft_dct1_2d_batched";
    hs_seterr("%s", "");
    int L0, L1;
    int rc = hs_dct1_args_2d(who, kind0, kind1, d_in, d_out, n0, n1, batch, &L0, &L1);
    if (rc || batch == 0) return rc;
    rc = hs_require_gpu();
    if (rc) return rc;
    const hs_conv_pair p1 = hs_conv_plans(L1), p0 = hs_conv_plans(L0);
    if (!p0.f || !p1.f) {
        hs_seterr("%s: planning the lengths %d and %d failed", who, L0, L1);
        rc = HSFFT_ERR_NOMEM;
    } else {
        const int d = hs_lock_device();
        rc = dct1::run_2d(who, kind0 == HSFFT_KIND_SIN, kind1 == HSFFT_KIND_SIN, p0.f, p1.f, d_in, d_out, n0, L0, n1, L1, batch);
        hs_unlock_device(d);
    }
    hs_conv_plans_done(p0);
    hs_conv_plans_done(p1);
    return rc;
}

}  // extern "C"
