/*
 * hsfft_dct4.h -- batched DCT-IV / DST-IV of real rows, and the MDCT / IMDCT of real rows built on
 * them (hsfft_dct4_batched, hsfft_mdct_shape, hsfft_mdct_batched, hsfft_imdct_batched of
 * include/hsfft_gpu.h; the reference has no cosine, sine or lapped transform).  Included at the end
 * of hsfft_device.hip after hsfft_dct2d.h: the drivers launch their kernels directly, so no host C
 * file needs a new device-layer symbol.
 *
 * Type IV by a complex transform of half the length: one kernel pairs x[2j] with x[N-1-2j] and
 * rotates the pair by the table's (cos, sin)(pi (8j+1) / 8N) into a scratch of rows of N/2 complex,
 * hs_c2c_rows() unchanged transforms them into a second scratch, and one kernel rotates bin k by the
 * same table and writes the two outputs it gives.  There is no split pass, as the r2c of the types
 * II and III has.  The sine form is an index and sign variant inside the same two kernels.  The MDCT
 * folds every frame of 2N samples into N (one kernel) and runs the type-IV driver on the folded
 * rows; the IMDCT runs the driver on the coefficients and unfolds, windows and overlap-adds (one
 * kernel).  The scratch buffers are bounded by HSFFT_DCT_CHUNK_MB and
 * HSFFT_MDCT_CHUNK_MB, not by the job.  The table and the cache of its device copies are host C:
 * hsfft_dct4.c.
 */
#include "hsfft_gpu.h"
#include "hsfft_host.h"

namespace dct4 {

using dct::flip;

/* z = (a c + b s, b c - a s), every operation rounded on its own (the file's -ffp-contract=off) */
__device__ __forceinline__ v2d rot_in(double a, double b, v2d w)
{
    v2d z;
    z.x = a * w.x + b * w.y;
    z.y = b * w.x - a * w.y;
    return z;
}

/* Before the c2c: z[j] = rot_in(x[2j], x[N-1-2j], t[j]) for j < h = N/2; SIN reads the row
 * reversed, which swaps the two samples: rot_in(x[N-1-2j], x[2j], t[j]).  Row yi of the launch.  A
 * lane indexed by j alone would use half of each 16 bytes it touches at both ends of the row, so a
 * lane owns the mirrored pair p and p' = h-1-p: it loads (x[2p], x[2p+1]) and (x[2p'], x[2p'+1]),
 * 16 bytes each where the row is 16-byte aligned (rows are N x 8 bytes, N even, so all rows are or
 * none is) and 8 + 8 otherwise, and two table words; z[p] takes x[2p] and x[2p'+1], z[p'] takes
 * x[2p'] and x[2p+1].  Two 16-byte stores, one stream ascending from z and one descending from
 * z + h - 1, both contiguous across the wave.  The middle lane of an odd h has p == p' and works
 * once. */
template <bool SIN>
__global__ __launch_bounds__(256) void k_dct4_pre(const double *__restrict__ x, const v2d *__restrict__ t,
                                                  v2d *__restrict__ z, long long N)
{
    const long long h = N / 2, lanes = (h + 1) / 2;
    const double *xrow = x + blockIdx.y * N;
    v2d *zrow = z + blockIdx.y * h;
    const bool al = ((uintptr_t)xrow & 15) == 0;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < lanes; p += (long long)gridDim.x * blockDim.x) {
        const long long q = h - 1 - p;
        v2d lo, hi;
        if (al) {
            lo = *(const v2d *)(xrow + 2 * p);
            hi = *(const v2d *)(xrow + 2 * q);
        } else {
            lo.x = xrow[2 * p];
            lo.y = xrow[2 * p + 1];
            hi.x = xrow[2 * q];
            hi.y = xrow[2 * q + 1];
        }
        zrow[p] = SIN ? rot_in(hi.y, lo.x, t[p]) : rot_in(lo.x, hi.y, t[p]);
        if (q != p) zrow[q] = SIN ? rot_in(lo.y, hi.x, t[q]) : rot_in(hi.x, lo.y, t[q]);
    }
}

/* After the c2c: with V = Z[yi][k] and (c, s) = t[k], re_k = V.re c + V.im s and im_k = V.im c -
 * V.re s, each operation rounded on its own and computed for every k; out[2k] = g re_k and
 * out[N-1-2k] = (-g) im_k, and SIN flips the sign bit of the odd outputs.  A lane owns the mirrored
 * pair k and k' = h-1-k: it loads Z[k], Z[k'], t[k], t[k'] and stores (out[2k], out[2k+1]) = (g
 * re_k, -g im_k') and (out[2k'], out[2k'+1]) = (g re_k', -g im_k), 16 bytes each where the caller's
 * row is 16-byte aligned and 8 + 8 otherwise.  g: 2.0 for the transforms, 1.0 for the MDCT. */
template <bool SIN>
__global__ __launch_bounds__(256) void k_dct4_post(const v2d *__restrict__ Z, const v2d *__restrict__ t,
                                                   double *__restrict__ out, long long N, double g)
{
    const long long h = N / 2, lanes = (h + 1) / 2;
    const v2d *zrow = Z + blockIdx.y * h;
    double *orow = out + blockIdx.y * N;
    const bool al = ((uintptr_t)orow & 15) == 0;
    const double ng = -g;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < lanes; k += (long long)gridDim.x * blockDim.x) {
        const long long q = h - 1 - k;
        const v2d V = zrow[k], w = t[k], U = zrow[q], u = t[q];
        const double re_k = V.x * w.x + V.y * w.y, im_k = V.y * w.x - V.x * w.y;
        const double re_q = U.x * u.x + U.y * u.y, im_q = U.y * u.x - U.x * u.y;
        v2d lo, hi;
        lo.x = g * re_k;
        lo.y = SIN ? flip(ng * im_q) : ng * im_q;
        hi.x = g * re_q;
        hi.y = SIN ? flip(ng * im_k) : ng * im_k;
        if (al) {
            *(v2d *)(orow + 2 * k) = lo;
            if (q != k) *(v2d *)(orow + 2 * q) = hi;
        } else {
            orow[2 * k] = lo.x;
            orow[2 * k + 1] = lo.y;
            if (q != k) {
                orow[2 * q] = hi.x;
                orow[2 * q + 1] = hi.y;
            }
        }
    }
}

static int pre(int sin, const double *x, const v2d *t, v2d *z, long long N, long long rows)
{
    return dct::launch([=](dim3 g, const double *a, v2d *b) {
        if (sin) hipLaunchKernelGGL(k_dct4_pre<true>, g, dim3(256), 0, stream(), a, t, b, N);
        else hipLaunchKernelGGL(k_dct4_pre<false>, g, dim3(256), 0, stream(), a, t, b, N);
    }, x, N, z, N / 2, (N / 2 + 1) / 2, rows);
}

static int post(int sin, const v2d *Z, const v2d *t, double *out, long long N, double gain, long long rows)
{
    return dct::launch([=](dim3 g, const v2d *a, double *b) {
        if (sin) hipLaunchKernelGGL(k_dct4_post<true>, g, dim3(256), 0, stream(), a, t, b, N, gain);
        else hipLaunchKernelGGL(k_dct4_post<false>, g, dim3(256), 0, stream(), a, t, b, N, gain);
    }, Z, N / 2, out, N, (N / 2 + 1) / 2, rows);
}

/* (device lock held) `batch` rows of n: e is the forward c2c plan of length n/2.  Rows are walked
 * in chunks of `c` with two pool buffers of c x n/2 complex each, z (the rotated pairs) and Z (their
 * transforms).  Per chunk: rotate in -> z, c2c rows z -> Z (one copy where n/2 == 1), rotate Z ->
 * out.  `who` names the public call in messages. */
static int run(const char *who, int dev, int sin, double gain, hs_entry *e, const fft_type *d_in, fft_type *d_out, int n,
               long long batch)
{
    const long long N = n, h = N / 2;
    const size_t half = sizeof(fft_data) * (size_t)h;
    long long c = (long long)(hs_env_mb("HSFFT_DCT_CHUNK_MB", 1024.0) / (2 * half));
    if (c > batch) c = batch;
    if (c < 1) c = 1;
    fft_data *z, *Z;
    for (;;) {
        z = (fft_data *)hs_scratch(HS_SCR_DCT, half * (size_t)c);
        Z = z ? (fft_data *)hs_scratch(HS_SCR_DCT_SPEC, half * (size_t)c) : NULL;
        if (Z || c == 1) break;
        c = (c + 1) / 2;
    }
    if (!Z) {
        hs_seterr("%s: scratch allocation failed (%lld rows of %lld)", who, c, N);
        return HSFFT_ERR_NOMEM;
    }
    const v2d *t = (const v2d *)hs_dct4_table(dev, n);
    if (!t) return HSFFT_ERR_DEVICE;
    int rc = 0;
    for (long long b0 = 0; b0 < batch && !rc; b0 += c) {
        const long long rows = batch - b0 < c ? batch - b0 : c;
        rc = dct::dev_rc(pre(sin, d_in + b0 * N, t, (v2d *)z, N, rows), "dct4 input rotation");
        if (!rc) rc = tr2d::rows(e, z, Z, rows);
        if (!rc) rc = dct::dev_rc(post(sin, (const v2d *)Z, t, d_out + b0 * N, N, gain, rows), "dct4 output rotation");
    }
    return rc;
}

/* the GPU, the forward c2c plan of length h from the convolution plan cache (it follows the calling
 * thread's twiddle mode, and a repeated length builds nothing) and the device lock around
 * body(dev, e) */
template <typename F>
static int with_plan(const char *who, int h, F body)
{
    int rc = hs_require_gpu();
    if (rc) return rc;
    const hs_conv_cpair cp = hs_conv_cplans(h);
    if (!cp.f || !cp.i) {
        hs_seterr("%s: planning the length %d failed", who, h);
        rc = HSFFT_ERR_NOMEM;
    } else {
        const int d = hs_lock_device();
        hs_entry *e = hs_entry_get(cp.f);
        rc = e ? body(d, e) : HSFFT_ERR_ARG;
        hs_entry_put(e);
        hs_unlock_device(d);
    }
    hs_conv_cplans_done(cp);
    return rc;
}

}  // namespace dct4

namespace mdct {

using dct::flip;

/* one windowed sample of a frame: xpad[start + m] * w[m], xpad = the row inside [0, n) and +0.0
 * outside (the product is computed there too), and no multiply at all where w == NULL */
__device__ __forceinline__ double sample(const double *xrow, const double *w, long long n, long long start, long long m)
{
    const long long s = start + m;
    const double v = s >= 0 && s < n ? xrow[s] : 0.0;
    return w ? v * w[m] : v;
}

/* Gather, window and fold: frame yi of the launch is frame f = q % nframes of row b = q / nframes,
 * q = q0 + yi, and starts at f N - lpad.  With p[m] its 2N windowed samples and hq = N/2:
 *   u[i] = (-p[3hq-1-i]) - p[3hq+i] for i < hq,   u[i] = p[i-hq] - p[3hq-1-i] for hq <= i < N,
 * the unary minus a flip of the sign bit.  Lane i writes u[i]: its first source walks down from
 * p[3hq-1] and its second walks up, from p[3hq] for i < hq and from p[0] after that, so every
 * stream is contiguous across the wave; 8-byte accesses, because hq may be odd and the source row
 * needs the alignment of a double only.  Nothing is read outside row b.  The window is 2N doubles
 * read by every frame: it stays in L2.  q is uniform over the workgroup. */
__global__ __launch_bounds__(256) void k_fold(const double *__restrict__ x, const double *__restrict__ w, long long n,
                                              long long N, long long lpad, long long nframes, long long q0,
                                              double *__restrict__ dst)
{
    const long long yi = blockIdx.y, q = q0 + yi, b = q / nframes, f = q - b * nframes;
    const long long start = f * N - lpad, hq = N / 2;
    const double *xrow = x + b * n;
    double *row = dst + yi * N;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const double down = sample(xrow, w, n, start, 3 * hq - 1 - i);
        row[i] = i < hq ? flip(down) - sample(xrow, w, n, start, 3 * hq + i) : sample(xrow, w, n, start, i - hq) - down;
    }
}

struct ola_args {
    const double *V; /* the chunk's type-IV outputs, rows of N: frame f of the chunk's row r at (r nframes + f) N */
    const double *w; /* the window of 2N, or NULL */
    double *out;     /* the chunk's first output row */
    long long r0;    /* the chunk's row index of the launch's row 0 */
    long long n, N, lpad, nframes;
    double div;      /* (double)(N/2) */
};

/* sample m < 2N of one frame's term: the unfolded v -- v[m+hq] for m < hq, -v[3hq-1-m] for hq <= m <
 * 3hq, -v[m-3hq] after that, the minus a flip of the sign bit -- divided by hq, then times w[m],
 * each rounded on its own */
__device__ __forceinline__ double term(const ola_args &a, const double *v, long long m)
{
    const long long hq = a.N / 2;
    const double y = m < hq ? v[m + hq] : flip(m < 3 * hq ? v[3 * hq - 1 - m] : v[m - 3 * hq]);
    const double d = y / a.div;
    return a.w ? d * a.w[m] : d;
}

/* one output sample: position P = i + lpad is covered by frame P/N - 1 (its second half) and by
 * frame P/N (its first half), where they exist, and at least one does.  The earlier frame's term
 * first, the later one's added to it; a single frame gives its term alone. */
__device__ __forceinline__ double ola_word(const ola_args &a, const double *vrow, long long i)
{
    /* n, N, lpad <= 2^30: P fits 32 bits, and the division is a 32-bit one */
    const unsigned P = (unsigned)(i + a.lpad);
    const long long f1 = P / (unsigned)a.N, m = P - (unsigned)f1 * (unsigned)a.N;
    if (f1 == 0) return term(a, vrow, m);
    const double t0 = term(a, vrow + (f1 - 1) * a.N, m + a.N);
    return f1 < a.nframes ? t0 + term(a, vrow + f1 * a.N, m) : t0;
}

/* Unfold, window and overlap-add: row yi of the launch is row r = r0 + yi of the chunk.  A lane owns
 * the output samples 2k and 2k+1 (n is even), reads the two v rows that cover them and stores once:
 * 16 bytes where the caller's row is 16-byte aligned (rows are n x 8 bytes, so all are or none is),
 * 8 + 8 otherwise.  Every output word is written exactly once, none is read, and there are no
 * atomics: the order of the add is the contract. */
__global__ __launch_bounds__(256) void k_unfold_ola(ola_args a)
{
    const long long r = a.r0 + blockIdx.y;
    const double *vrow = a.V + r * a.nframes * a.N;
    double *orow = a.out + r * a.n;
    const bool al = ((uintptr_t)orow & 15) == 0;
    const long long pairs = a.n / 2;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < pairs; k += (long long)gridDim.x * blockDim.x) {
        v2d v;
        v.x = ola_word(a, vrow, 2 * k);
        v.y = ola_word(a, vrow, 2 * k + 1);
        if (al) *(v2d *)(orow + 2 * k) = v;
        else {
            orow[2 * k] = v.x;
            orow[2 * k + 1] = v.y;
        }
    }
}

/* the ranges both directions share: 0, or HSFFT_ERR_ARG with the message set */
static int check_sizes(const char *who, int n, int N, int pad)
{
    if (N < 2 || (N & 1) || N > stft::MAX_LEN || n < 1 || n > stft::MAX_LEN || (pad != 0 && pad != 1)) {
        hs_seterr("%s: n %d, hop %d or pad %d is out of range (the hop is even, 2 to 2^30)", who, n, N, pad);
        return HSFFT_ERR_ARG;
    }
    return 0;
}

/* 0 with *nframes set, or HSFFT_ERR_ARG with the message set */
static int get_shape(const char *who, int n, int N, int pad, int *nframes)
{
    const int rc = check_sizes(who, n, N, pad);
    if (rc) return rc;
    if (n % N || (!pad && n < 2 * N)) {
        hs_seterr("%s: a row of %d samples is no multiple of the hop %d, or shorter than one frame of 2 x %d (pad == 0)", who,
                  n, N, N);
        return HSFFT_ERR_ARG;
    }
    *nframes = pad ? n / N + 1 : n / N - 1;
    return 0;
}

static int fold(const fft_type *x, const fft_type *w, long long n, long long N, long long lpad, long long nframes,
                long long q0, double *U, long long cb)
{
    for (long long b0 = 0; b0 < cb; b0 += Y_MAX) {
        const int nb = (int)(cb - b0 < Y_MAX ? cb - b0 : Y_MAX);
        hipLaunchKernelGGL(k_fold, dim3(grid_for(N, 256), nb), dim3(256), 0, stream(), x, w, n, N, lpad, nframes, q0 + b0,
                           U + b0 * N);
        HCHK(hipGetLastError());
    }
    return 0;
}

static int ola(ola_args a, long long rows)
{
    for (long long b0 = 0; b0 < rows; b0 += Y_MAX) {
        const int nb = (int)(rows - b0 < Y_MAX ? rows - b0 : Y_MAX);
        a.r0 = b0;
        hipLaunchKernelGGL(k_unfold_ola, dim3(grid_for(a.n / 2, 256), nb), dim3(256), 0, stream(), a);
        HCHK(hipGetLastError());
    }
    return 0;
}

/* `rows` (frames, or rows of frames) per chunk of HSFFT_MDCT_CHUNK_MB, at least one and at most
 * `most`, and the chunk in HS_SCR_MDCT: halved while the allocation fails; NULL with the message set */
static double *chunk_scratch(const char *who, size_t row_bytes, long long most, long long *per_chunk)
{
    long long c = (long long)(hs_env_mb("HSFFT_MDCT_CHUNK_MB", 1024.0) / row_bytes);
    if (c > most) c = most;
    if (c < 1) c = 1;
    double *S;
    for (;;) {
        S = (double *)hs_scratch(HS_SCR_MDCT, row_bytes * (size_t)c);
        if (S || c == 1) break;
        c = (c + 1) / 2;
    }
    if (!S) hs_seterr("%s: scratch allocation failed (%lld rows of %lld bytes)", who, c, (long long)row_bytes);
    *per_chunk = c;
    return S;
}

/* (device lock held) the forward call.  Frames are numbered q = b nframes + f and walked in chunks
 * of consecutive q, which may cross row boundaries, with one pool buffer U (c x N doubles).  Per
 * chunk: gather, window and fold x -> U, type IV with gain 1.0 U -> the caller's output. */
static int run_forward(int dev, hs_entry *e, const fft_type *d_x, int n, const fft_type *d_w, int N, int lpad, int nframes,
                       fft_type *d_out, int batch)
{
    const char *who = "hsfft_mdct_batched";
    const long long total = (long long)batch * nframes;
    long long c;
    double *U = chunk_scratch(who, sizeof(double) * (size_t)N, total, &c);
    if (!U) return HSFFT_ERR_NOMEM;
    int rc = 0;
    for (long long q0 = 0; q0 < total && !rc; q0 += c) {
        const long long cb = total - q0 < c ? total - q0 : c;
        rc = dct::dev_rc(fold(d_x, d_w, n, N, lpad, nframes, q0, U, cb), "mdct fold");
        if (!rc) rc = dct4::run(who, dev, 0, 1.0, e, U, d_out + q0 * N, N, cb);
    }
    return rc;
}

/* (device lock held) the backward call.  Whole rows are walked in chunks of `c` rows with one pool
 * buffer V (c x nframes x N doubles): a row's frames never straddle a chunk, so nothing is carried.
 * Per chunk: type IV with gain 1.0 coefficients -> V, unfold and overlap-add V -> out. */
static int run_backward(int dev, hs_entry *e, const fft_type *d_X, int nframes, const fft_type *d_w, int N, int lpad,
                        fft_type *d_out, int n, int batch)
{
    const char *who = "hsfft_imdct_batched";
    const size_t per = sizeof(double) * (size_t)N * (size_t)nframes;
    long long c;
    double *V = chunk_scratch(who, per, batch, &c);
    if (!V) return HSFFT_ERR_NOMEM;
    ola_args a;
    a.V = V;
    a.w = d_w;
    a.n = n;
    a.N = N;
    a.lpad = lpad;
    a.nframes = nframes;
    a.div = (double)(N / 2);
    int rc = 0;
    for (long long b0 = 0; b0 < batch && !rc; b0 += c) {
        const long long rows = batch - b0 < c ? batch - b0 : c;
        rc = dct4::run(who, dev, 0, 1.0, e, d_X + b0 * nframes * N, V, N, rows * nframes);
        a.out = d_out + b0 * n;
        if (!rc) rc = dct::dev_rc(ola(a, rows), "imdct overlap-add");
    }
    return rc;
}

}  // namespace mdct

extern "C" {

int hsfft_dct4_batched(int kind, const fft_type *d_in, fft_type *d_out, int n, int batch)
{
    const char *who = "hsfft_dct4_batched";
    hs_seterr("%s", "");
    if (kind != HSFFT_KIND_COS && kind != HSFFT_KIND_SIN) {
        hs_seterr("%s: kind %d is not 0 (cosine) or 1 (sine)", who, kind);
        return HSFFT_ERR_ARG;
    }
    if (n < 2 || (n & 1) || n > HS_DCT_MAX_LEN) {
        hs_seterr("%s: the length %d is odd, below 2 or above 2^30", who, n);
        return HSFFT_ERR_ARG;
    }
    if (!d_in || !d_out || batch < 0) {
        hs_seterr("%s: NULL pointer or negative batch", who);
        return HSFFT_ERR_ARG;
    }
    if ((long long)n * batch > dct::MAX_WORDS) {
        hs_seterr("%s: %d rows of %d are more than the call can index", who, batch, n);
        return HSFFT_ERR_ARG;
    }
    const uintptr_t bytes = sizeof(fft_type) * (uintptr_t)n * (uintptr_t)batch;
    if (batch && (d_in == d_out || tr2d::overlap_bytes(d_out, bytes, d_in, bytes))) {
        hs_seterr("%s: the output overlaps the input", who);
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    return dct4::with_plan(who, n / 2, [=](int dev, hs_entry *e) {
        return dct4::run(who, dev, kind == HSFFT_KIND_SIN, 2.0, e, d_in, d_out, n, batch);
    });
}

int hsfft_mdct_shape(int n, int N, int pad, int *nframes, int *lpad)
{
    hs_seterr("%s", "");
    int nf;
    const int rc = mdct::get_shape("hsfft_mdct_shape", n, N, pad, &nf);
    if (rc) return rc;
    if (nframes) *nframes = nf;
    if (lpad) *lpad = pad ? N : 0;
    return 0;
}

int hsfft_mdct_batched(const fft_type *d_x, int n, const fft_type *d_w, int N, int pad, fft_type *d_out, int batch)
{
    const char *who = "hsfft_mdct_batched";
    hs_seterr("%s", "");
    if (!d_x || !d_out || batch < 0) {
        hs_seterr("%s: NULL pointer or negative batch", who);
        return HSFFT_ERR_ARG;
    }
    int nframes;
    int rc = mdct::get_shape(who, n, N, pad, &nframes);
    if (!rc) rc = stft::check_totals(who, n, N, nframes, batch);
    if (rc) return rc;
    const uintptr_t nb = (uintptr_t)batch, esz = sizeof(fft_type);
    const uintptr_t out_bytes = esz * (uintptr_t)nframes * (uintptr_t)N * nb;
    if (tr2d::overlap_bytes(d_out, out_bytes, d_x, esz * (uintptr_t)n * nb) ||
        (d_w && tr2d::overlap_bytes(d_out, out_bytes, d_w, batch ? esz * 2 * (uintptr_t)N : 0))) {
        hs_seterr("%s: the output overlaps an input", who);
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    return dct4::with_plan(who, N / 2, [=](int dev, hs_entry *e) {
        return mdct::run_forward(dev, e, d_x, n, d_w, N, pad ? N : 0, nframes, d_out, batch);
    });
}

int hsfft_imdct_batched(const fft_type *d_X, int nframes, const fft_type *d_w, int N, int pad, fft_type *d_out, int n,
                        int batch)
{
    const char *who = "hsfft_imdct_batched";
    hs_seterr("%s", "");
    if (!d_X || !d_out || batch < 0) {
        hs_seterr("%s: NULL pointer or negative batch", who);
        return HSFFT_ERR_ARG;
    }
    int rc = mdct::check_sizes(who, n, N, pad);
    if (rc) return rc;
    if (nframes < 1 || ((long long)nframes + 1) * N - (pad ? 2LL * N : 0) != n) {
        hs_seterr("%s: %d frames at the hop %d with pad %d do not give rows of %d samples", who, nframes, N, pad, n);
        return HSFFT_ERR_ARG;
    }
    rc = stft::check_totals(who, n, N, nframes, batch);
    if (rc) return rc;
    const uintptr_t nb = (uintptr_t)batch, esz = sizeof(fft_type);
    const uintptr_t out_bytes = esz * (uintptr_t)n * nb;
    if (tr2d::overlap_bytes(d_out, out_bytes, d_X, esz * (uintptr_t)nframes * (uintptr_t)N * nb) ||
        (d_w && tr2d::overlap_bytes(d_out, out_bytes, d_w, batch ? esz * 2 * (uintptr_t)N : 0))) {
        hs_seterr("%s: the output overlaps an input", who);
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    return dct4::with_plan(who, N / 2, [=](int dev, hs_entry *e) {
        return mdct::run_backward(dev, e, d_X, nframes, d_w, N, pad ? N : 0, d_out, n, batch);
    });
}

}  // extern "C"
