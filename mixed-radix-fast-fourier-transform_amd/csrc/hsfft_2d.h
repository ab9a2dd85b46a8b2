/*
 * hsfft_2d.h -- batched transpose of 16-byte elements and the 2D / column c2c drivers built on it
 * (hsfft_transpose_batched, hsfft_exec_2d, hsfft_exec_columns of include/hsfft_gpu.h; the
 * reference has no counterpart).  Included at the end of hsfft_device.hip: the drivers launch
 * the transpose directly, so no host C file needs a new device-layer symbol.
 *
 * The 1D transforms are hs_c2c_rows() unchanged -- every planned length over contiguous rows --
 * and a transpose is a pure copy, so a 2D result is, word for word, the reference's fft_exec
 * applied to every row and then to every column of that result.
 *
 * The real 2D transforms (hsfft_r2c_2d, hsfft_r2c_2d_full, hsfft_c2r_2d) are built
 * the same way from hs_r2c_rows() / hs_c2r_rows(), hs_c2c_rows() over the n1/2+1 columns of the
 * half spectrum and the transposes; the full layout's mirror half is written by the one kernel
 * they add, k_transpose_herm.
 *
 * k_transpose8 is the same transpose for 8-byte elements (hsfft_transpose_real_batched); the 2D
 * cosine and sine transforms of hsfft_dct2d.h run it between the row transforms of hsfft_dct.h
 * (DESIGN.md §14).
 */
#include "hsfft_gpu.h"
#include "hsfft_host.h"

namespace tr2d {

/* out[b][c][r] = in[b][r][c] for one TS x TS tile per workgroup of 256 threads.
 *
 * Both global sides are 16 B per lane with lanes on consecutive elements of the side's fastest
 * axis: TS = 32 gives two 512-B runs per wave-instruction, TS = 64 one 1-KiB run.  The tile is
 * staged through LDS with a row pitch of TS + 1 elements.  The row-wise stores (ds_write_b128,
 * 8 contiguous lanes per group, banks modulo 32 dwords) cover 128 contiguous bytes per group:
 * conflict-free at any pitch.  The column-wise loads (ds_read_b128, banks modulo 64 dwords = 16
 * slots of 16 B, groups of 16 lanes {0-3,12-15,20-27}, ...) put lane l at slot (l * (TS + 1) +
 * const) mod 16 = (l + const) mod 16, and every group holds 16 distinct l mod 16: conflict-free.
 * At pitch TS the 16 lanes of a group would all sit on one slot (16-way).
 *
 * The batch is flattened into the 1D grid (tile index = (b * ntr + tr) * ntc + tc, 64-bit
 * arithmetic throughout); DIAG rotates the tile column by the tile row, so that workgroups that
 * run together differ in both coordinates and neither side walks one power-of-two stride
 * (+7 % on 32768 x 512, -11 % on square images; off by default).
 * No arithmetic on the data: plain 16-B vector loads and stores, every word copied verbatim. */
template <int TS, bool DIAG>
__global__ __launch_bounds__(256) void k_transpose(const v2d *__restrict__ in, v2d *__restrict__ out, long long rows,
                                                   long long cols, long long ntr, long long ntc, long long tile0)
{
    extern __shared__ v2d tr_tile[];
    constexpr int P = TS + 1, RY = 256 / TS, NK = TS / RY;
    const long long t = tile0 + blockIdx.x, per = ntr * ntc;
    const long long b = t / per, rem = t - b * per;
    const long long tr = rem / ntc;
    long long tc = rem - tr * ntc;
    if (DIAG) {
        tc += tr % ntc;
        if (tc >= ntc) tc -= ntc;
    }
    const int tx = threadIdx.x % TS, ty = threadIdx.x / TS;
    const long long r0 = tr * TS, c0 = tc * TS;
    const v2d *src = in + b * rows * cols;
    v2d *dst = out + b * rows * cols;
    v2d v[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const long long r = r0 + ty + k * RY, c = c0 + tx;
        if (r < rows && c < cols) v[k] = src[r * cols + c];
    }
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const long long r = r0 + ty + k * RY, c = c0 + tx;
        if (r < rows && c < cols) tr_tile[(ty + k * RY) * P + tx] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const long long c = c0 + ty + k * RY, r = r0 + tx; /* output row c, output column r */
        if (c < cols && r < rows) dst[c * rows + r] = tr_tile[tx * P + ty + k * RY];
    }
}

/* tiles per launch: the grid's x dimension is 32-bit */
constexpr long long MAX_GRID = 1LL << 30;

/* (device lock held by the caller) queue the transposes of `batch` images on the selected stream */
static int launch(const void *in, void *out, long long rows, long long cols, long long batch)
{
    typedef void (*kfn)(const v2d *, v2d *, long long, long long, long long, long long, long long);
    /* HSFFT_TR_TILE (64 | 32) and HSFFT_TR_DIAG (0 | 1): measurement knobs, the four variants of
     * DESIGN.md §8's table (tools/bench_2d.py --variants); the defaults are the fastest there */
    const int ts = hs_env_int("HSFFT_TR_TILE", 64) == 32 ? 32 : 64;
    const int diag = hs_env_int("HSFFT_TR_DIAG", 0) != 0;
    const kfn fn = ts == 64 ? (diag ? k_transpose<64, true> : k_transpose<64, false>)
                            : (diag ? k_transpose<32, true> : k_transpose<32, false>);
    const size_t lds = (size_t)ts * (ts + 1) * sizeof(v2d);
    const long long ntr = (rows + ts - 1) / ts, ntc = (cols + ts - 1) / ts;
    if (ntr > MAX_GRID / ntc) {
        snprintf(g_err, sizeof g_err, "transpose: %lld x %lld tiles per image", ntr, ntc);
        return -1;
    }
    if (lds > 65536) { /* once per device and kernel (callers hold the device lock) */
        static bool lds_set[HS_MAX_DEV][2];
        bool &done = lds_set[cur_dev()][diag];
        if (!done) HCHK(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        done = true;
    }
    const long long total = batch * ntr * ntc;
    for (long long t0 = 0; t0 < total; t0 += MAX_GRID) {
        const long long g = total - t0 < MAX_GRID ? total - t0 : MAX_GRID;
        hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(256), lds, stream(), (const v2d *)in, (v2d *)out, rows, cols, ntr,
                           ntc, t0);
        HCHK(hipGetLastError());
    }
    return 0;
}

static int transpose(const void *in, void *out, long long rows, long long cols, long long batch)
{
    const int rc = launch(in, out, rows, cols, batch);
    if (rc) hs_seterr("transpose: %s", g_err);
    return rc ? HSFFT_ERR_DEVICE : 0;
}

/* out[b][c][r] = in[b][r][c] for 8-byte elements (hsfft_transpose_real_batched and the 2D cosine and
 * sine transforms, hsfft_dct2d.h): one TS x TS tile of doubles per workgroup of 256 threads, the
 * skeleton of k_transpose.
 *
 * Both global sides are 8 B per lane -- caller buffers need the alignment of a double only -- with
 * lanes on consecutive elements of the side's fastest axis: at TS = 64 a wave-instruction covers
 * one 512-B run.  The tile is staged through LDS with a row pitch of TS + 1 doubles = 130 dwords.
 * The row-wise stores (ds_write_b64, banks modulo 32 dwords, groups of 16 contiguous lanes) cover
 * 128 contiguous bytes = 32 consecutive dwords per group: conflict-free at any pitch.  The
 * column-wise loads (ds_read_b64, banks modulo 64 dwords = 32 slots of 8 B, the two 32-lane halves
 * as groups) put lane l at dword 130 l + const, that is at slot (65 l + const) mod 32 = (l + const)
 * mod 32, and a half holds 32 distinct l mod 32: conflict-free.  At pitch TS every lane of a half
 * would sit on one slot (32-way).  Every LDS address is a multiple of 8 bytes.
 *
 * The batch is flattened into the 1D grid as in k_transpose, 64-bit arithmetic throughout, edge
 * guards on both sides.  No arithmetic on the data: plain 8-B loads and stores, every word -- NaN
 * payloads, signed zeros, subnormals -- copied verbatim. */
template <int TS>
__global__ __launch_bounds__(256) void k_transpose8(const double *__restrict__ in, double *__restrict__ out,
                                                    long long rows, long long cols, long long ntr, long long ntc,
                                                    long long tile0)
{
    constexpr int P = TS + 1, RY = 256 / TS, NK = TS / RY;
    __shared__ double tile[TS * P];
    const long long t = tile0 + blockIdx.x, per = ntr * ntc;
    const long long b = t / per, rem = t - b * per;
    const long long tr = rem / ntc, tc = rem - tr * ntc;
    const int tx = threadIdx.x % TS, ty = threadIdx.x / TS;
    const long long r0 = tr * TS, c0 = tc * TS;
    const double *src = in + b * rows * cols;
    double *dst = out + b * rows * cols;
    double v[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const long long r = r0 + ty + k * RY, c = c0 + tx;
        if (r < rows && c < cols) v[k] = src[r * cols + c];
    }
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const long long r = r0 + ty + k * RY, c = c0 + tx;
        if (r < rows && c < cols) tile[(ty + k * RY) * P + tx] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const long long c = c0 + ty + k * RY, r = r0 + tx; /* output row c, output column r */
        if (c < cols && r < rows) dst[c * rows + r] = tile[tx * P + ty + k * RY];
    }
}

/* (device lock held by the caller) queue the 8-byte transposes of `batch` matrices on the selected
 * stream; the tile is 64 x 65 x 8 = 33280 bytes of static LDS */
static int launch8(const double *in, double *out, long long rows, long long cols, long long batch)
{
    constexpr int ts = 64;
    const long long ntr = (rows + ts - 1) / ts, ntc = (cols + ts - 1) / ts;
    if (ntr > MAX_GRID / ntc) {
        snprintf(g_err, sizeof g_err, "transpose: %lld x %lld tiles per matrix", ntr, ntc);
        return -1;
    }
    const long long total = batch * ntr * ntc;
    for (long long t0 = 0; t0 < total; t0 += MAX_GRID) {
        const long long g = total - t0 < MAX_GRID ? total - t0 : MAX_GRID;
        hipLaunchKernelGGL(k_transpose8<ts>, dim3((unsigned)g), dim3(256), 0, stream(), in, out, rows, cols, ntr, ntc, t0);
        HCHK(hipGetLastError());
    }
    return 0;
}

static int transpose8(const double *in, double *out, long long rows, long long cols, long long batch)
{
    const int rc = launch8(in, out, rows, cols, batch);
    if (rc) hs_seterr("transpose of 8-byte elements: %s", g_err);
    return rc ? HSFFT_ERR_DEVICE : 0;
}

/* The last transpose of hsfft_r2c_2d_full: the transposed half spectrum in[b][k1][k0] (w = n1/2 + 1
 * rows of n0) goes to the full layout out[b][k0][k1] (n0 rows of n1), and every element with
 * 1 <= k1 <= n1/2 - 1 is stored a second time, imaginary part negated, at the mirrored index
 * out[b][(n0 - k0) % n0][n1 - k1].  Together the two stores write each of the n0 x n1 outputs
 * exactly once: the primary covers the columns 0..n1/2, the mirror the columns n1/2+1..n1-1.
 *
 * Staging as in k_transpose: 256 threads, one TS x TS tile of the source, LDS pitch TS + 1, edge
 * guards on both sides, 64-bit indices, the batch flattened into the 1D grid.  A wave-instruction
 * of the primary store covers one run of consecutive k1 of one output row; its mirror store
 * covers the same run of another row with the lane order reversed, so it coalesces the same way.
 * The negation is a sign-bit flip (zeros and NaNs included); no other arithmetic on the data. */
template <int TS>
__global__ __launch_bounds__(256) void k_transpose_herm(const v2d *__restrict__ in, v2d *__restrict__ out, long long n0,
                                                        long long n1, long long ntr, long long ntc, long long tile0)
{
    extern __shared__ v2d tr_tile[];
    constexpr int P = TS + 1, RY = 256 / TS, NK = TS / RY;
    const long long h = n1 / 2, w = h + 1;
    const long long t = tile0 + blockIdx.x, per = ntr * ntc;
    const long long b = t / per, rem = t - b * per;
    const long long tr = rem / ntc, tc = rem - tr * ntc;
    const int tx = threadIdx.x % TS, ty = threadIdx.x / TS;
    const long long r0 = tr * TS, c0 = tc * TS; /* source row = k1, source column = k0 */
    const v2d *src = in + b * w * n0;
    v2d *dst = out + b * n0 * n1;
    v2d v[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const long long r = r0 + ty + k * RY, c = c0 + tx;
        if (r < w && c < n0) v[k] = src[r * n0 + c];
    }
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const long long r = r0 + ty + k * RY, c = c0 + tx;
        if (r < w && c < n0) tr_tile[(ty + k * RY) * P + tx] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const long long k0 = c0 + ty + k * RY, k1 = r0 + tx;
        if (k0 < n0 && k1 < w) {
            v2d e = tr_tile[tx * P + ty + k * RY];
            dst[k0 * n1 + k1] = e;
            if (k1 >= 1 && k1 < h) {
                e.y = -e.y;
                dst[(k0 ? n0 - k0 : 0) * n1 + (n1 - k1)] = e;
            }
        }
    }
}

/* (device lock held by the caller) queue the mirrored transposes of `batch` images */
static int launch_herm(const void *in, void *out, long long n0, long long n1, long long batch)
{
    typedef void (*kfn)(const v2d *, v2d *, long long, long long, long long, long long, long long);
    const int ts = hs_env_int("HSFFT_TR_TILE", 64) == 32 ? 32 : 64; /* the knob of launch() */
    const kfn fn = ts == 64 ? k_transpose_herm<64> : k_transpose_herm<32>;
    const size_t lds = (size_t)ts * (ts + 1) * sizeof(v2d);
    const long long ntr = (n1 / 2 + 1 + ts - 1) / ts, ntc = (n0 + ts - 1) / ts;
    if (ntr > MAX_GRID / ntc) {
        snprintf(g_err, sizeof g_err, "mirrored transpose: %lld x %lld tiles per image", ntr, ntc);
        return -1;
    }
    if (lds > 65536) { /* once per device (callers hold the device lock) */
        static bool lds_set[HS_MAX_DEV];
        bool &done = lds_set[cur_dev()];
        if (!done) HCHK(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        done = true;
    }
    const long long total = batch * ntr * ntc;
    for (long long t0 = 0; t0 < total; t0 += MAX_GRID) {
        const long long g = total - t0 < MAX_GRID ? total - t0 : MAX_GRID;
        hipLaunchKernelGGL(fn, dim3((unsigned)g), dim3(256), lds, stream(), (const v2d *)in, (v2d *)out, n0, n1, ntr, ntc,
                           t0);
        HCHK(hipGetLastError());
    }
    return 0;
}

static int transpose_herm(const void *in, void *out, long long n0, long long n1, long long batch)
{
    const int rc = launch_herm(in, out, n0, n1, batch);
    if (rc) hs_seterr("mirrored transpose: %s", g_err);
    return rc ? HSFFT_ERR_DEVICE : 0;
}

/* Scratch of the 2D paths (HS_SCR_2D): HSFFT_2D_CHUNK_MB (default 1024) bounds it.  A call walks
 * its batch in chunks of whole images: bytes / (copies * image bytes) images, at least one, at
 * most the batch and at most what keeps a chunk's row count an int; halved while the allocation
 * fails; the last chunk may be ragged.  hsfft_exec_2d needs one copy of the chunk and
 * hsfft_exec_columns two; for the real 2D transforms the image is the half spectrum, n0 x
 * (n1/2+1) elements: hsfft_r2c_2d and hsfft_r2c_2d_full need one copy, hsfft_c2r_2d two.
 * Images are counted in 16-byte elements: hsfft_dct_2d_batched (hsfft_dct2d.h) passes n0 x n1 / 2
 * for its real images of n0 x n1 doubles, both even, and holds one copy.
 * `extra_elems` more elements are allocated behind the chunk copies without counting towards the
 * rule (the 2D convolution's shared kernel spectrum, hsfft_conv2d.h). */
static void *chunk_scratch(long long img_elems, int max_dim, int copies, int batch, long long *per_chunk,
                           long long extra_elems = 0)
{
    const size_t img_bytes = sizeof(fft_data) * (size_t)img_elems;
    long long ci = (long long)(hs_env_mb("HSFFT_2D_CHUNK_MB", 1024.0) / ((size_t)copies * img_bytes));
    if (ci > batch) ci = batch;
    if (ci > 0x7fffffffLL / max_dim) ci = 0x7fffffffLL / max_dim;
    if (ci < 1) ci = 1;
    void *S;
    for (;;) {
        S = hs_scratch(HS_SCR_2D, (size_t)copies * img_bytes * (size_t)ci + sizeof(fft_data) * (size_t)extra_elems);
        if (S || ci == 1) break;
        ci = (ci + 1) / 2;
    }
    if (!S) hs_seterr("2D scratch allocation of %lld bytes failed", (long long)copies * (long long)img_bytes * ci);
    *per_chunk = ci;
    return S;
}

/* `count` contiguous rows of e's length; a length-1 transform is a copy (ref :332-342), queued
 * here as one copy instead of hs_c2c_rows' one per row */
static int rows(hs_entry *e, const fft_data *in, fft_data *out, long long count)
{
    if (e->N > 1) return hs_c2c_rows(e, in, e->N, out, e->N, (int)count);
    if (hsd_d2d_async(out, in, sizeof(fft_data) * (size_t)count)) {
        hs_seterr("2D copy: %s", hsd_errstr());
        return HSFFT_ERR_DEVICE;
    }
    return 0;
}

/* (device lock held) rows of p1 then columns of p0 of `batch` n0 x n1 images, per chunk:
 * rows in -> S, transpose S -> out, rows out -> S (the columns, now contiguous), transpose
 * S -> out.  d_in is only read. */
static int exec_2d(hs_entry *e0, hs_entry *e1, const fft_data *in, fft_data *out, int batch)
{
    const long long n0 = e0->N, n1 = e1->N, img = n0 * n1;
    if (img > (1LL << 40)) {
        hs_seterr("hsfft_exec_2d: image of %lld x %lld samples is too large", n0, n1);
        return HSFFT_ERR_ARG;
    }
    long long ci;
    fft_data *S = (fft_data *)chunk_scratch(img, (int)(n0 > n1 ? n0 : n1), 1, batch, &ci);
    if (!S) return HSFFT_ERR_NOMEM;
    for (long long b0 = 0; b0 < batch; b0 += ci) {
        const long long cb = batch - b0 < ci ? batch - b0 : ci;
        const fft_data *ib = in + b0 * img;
        fft_data *ob = out + b0 * img;
        int rc = rows(e1, ib, S, cb * n0);
        if (!rc) rc = transpose(S, ob, n0, n1, cb);
        if (!rc) rc = rows(e0, ob, S, cb * n1);
        if (!rc) rc = transpose(S, ob, n1, n0, cb);
        if (rc) return rc;
    }
    return 0;
}

/* (device lock held) the transform of p along axis 0 of `batch` n x ncols matrices, per chunk:
 * transpose in -> S0, rows S0 -> S1, transpose S1 -> out.  Three trips through HBM with two
 * chunk-sized halves of the scratch; with one half the second transpose would have to land in
 * the scratch again (its source is the output buffer) and a fourth trip, a copy, would follow. */
static int exec_columns(hs_entry *e, const fft_data *in, fft_data *out, int ncols, int batch)
{
    const long long n = e->N, img = n * (long long)ncols;
    if (img > (1LL << 40)) {
        hs_seterr("hsfft_exec_columns: matrix of %lld x %d samples is too large", n, ncols);
        return HSFFT_ERR_ARG;
    }
    long long ci;
    fft_data *S0 = (fft_data *)chunk_scratch(img, (int)(n > ncols ? n : ncols), 2, batch, &ci);
    if (!S0) return HSFFT_ERR_NOMEM;
    fft_data *S1 = S0 + ci * img;
    for (long long b0 = 0; b0 < batch; b0 += ci) {
        const long long cb = batch - b0 < ci ? batch - b0 : ci;
        int rc = transpose(in + b0 * img, S0, n, ncols, cb);
        if (!rc) rc = rows(e, S0, S1, cb * ncols);
        if (!rc) rc = transpose(S1, out + b0 * img, ncols, n, cb);
        if (rc) return rc;
    }
    return 0;
}

/* the half spectrum of the real 2D transforms: n0 rows of w = n1/2 + 1 bins; 0 (message set) if
 * it is too large */
static long long half_image(const char *who, long long n0, long long w)
{
    if (n0 * w <= (1LL << 40)) return n0 * w;
    hs_seterr("%s: half spectrum of %lld x %lld bins is too large", who, n0, w);
    return 0;
}

/* (device lock held) r2c of r1 on the rows, then e0 on the w = n1/2 + 1 columns of `batch` real
 * n0 x n1 images, per chunk with one scratch copy S of the chunk's half spectra: r2c-compact rows
 * in -> S (n0 x w), transpose S -> T, rows T -> S (the columns, now contiguous: w x n0), and the
 * last transpose S -> out.  full 0: out holds n0 x w per image, T is the output chunk itself and
 * the last transpose is the plain one.  full 1: out holds n0 x n1 per image, T is the front of
 * the (no smaller) output chunk and the last transpose also writes the mirror half. */
static int r2c_2d(hs_entry *e0, fft_real_object r1, const fft_type *in, fft_data *out, int batch, int full)
{
    const long long n0 = e0->N, h = r1->cobj->N, n1 = 2 * h, w = h + 1;
    const long long img = half_image(full ? "hsfft_r2c_2d_full" : "hsfft_r2c_2d", n0, w), oimg = full ? n0 * n1 : img;
    if (!img) return HSFFT_ERR_ARG;
    long long ci;
    fft_data *S = (fft_data *)chunk_scratch(img, (int)(n0 > w ? n0 : w), 1, batch, &ci);
    if (!S) return HSFFT_ERR_NOMEM;
    for (long long b0 = 0; b0 < batch; b0 += ci) {
        const long long cb = batch - b0 < ci ? batch - b0 : ci;
        fft_data *ob = out + b0 * oimg;
        int rc = hs_r2c_rows(r1, in + b0 * n0 * n1, S, (int)(cb * n0), 1);
        if (!rc) rc = transpose(S, ob, n0, w, cb);
        if (!rc) rc = rows(e0, ob, S, cb * w);
        if (!rc) rc = full ? transpose_herm(S, ob, n0, n1, cb) : transpose(S, ob, w, n0, cb);
        if (rc) return rc;
    }
    return 0;
}

/* (device lock held) e0 on the w columns of `batch` half spectra of n0 x w, then c2r of r1 on
 * every row, per chunk with two scratch copies (the real output is smaller than a half spectrum,
 * so it cannot hold an intermediate): transpose in -> S0, rows S0 -> S1, transpose S1 -> S0, c2r
 * rows S0 (pitch w) -> out. */
static int c2r_2d(hs_entry *e0, fft_real_object r1, const fft_data *in, fft_type *out, int batch)
{
    const long long n0 = e0->N, h = r1->cobj->N, n1 = 2 * h, w = h + 1;
    const long long img = half_image("hsfft_c2r_2d", n0, w);
    if (!img) return HSFFT_ERR_ARG;
    long long ci;
    fft_data *S0 = (fft_data *)chunk_scratch(img, (int)(n0 > w ? n0 : w), 2, batch, &ci);
    if (!S0) return HSFFT_ERR_NOMEM;
    fft_data *S1 = S0 + ci * img;
    for (long long b0 = 0; b0 < batch; b0 += ci) {
        const long long cb = batch - b0 < ci ? batch - b0 : ci;
        int rc = transpose(in + b0 * img, S0, n0, w, cb);
        if (!rc) rc = rows(e0, S0, S1, cb * w);
        if (!rc) rc = transpose(S1, S0, w, n0, cb);
        if (!rc) rc = hs_c2r_rows(r1, S0, NULL, w, out + b0 * n0 * n1, (int)(cb * n0));
        if (rc) return rc;
    }
    return 0;
}

/* the byte ranges [a, a + na) and [b, b + nb) share a byte */
static bool overlap_bytes(const void *a, uintptr_t na, const void *b, uintptr_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb ? pb - pa < na : pa - pb < nb;
}

/* the byte ranges [a, a + n) and [b, b + n) share a byte */
static bool overlap(const void *a, const void *b, long long elems)
{
    const uintptr_t n = (uintptr_t)elems * sizeof(fft_data);
    return overlap_bytes(a, n, b, n);
}

/* argument check of the three real 2D entry points; the real side holds n0 x n1 doubles per
 * image and the complex side `cplx_cols` bins per row.  0, or HSFFT_ERR_ARG with the message set */
static int real_2d_args(const char *who, fft_object p0, fft_real_object r1, const void *d_real, const void *d_cplx,
                        int full, int batch)
{
    bool bad = !p0 || !r1 || !r1->cobj || !d_real || !d_cplx || d_real == d_cplx || batch < 0 || p0->N < 1 ||
               r1->cobj->N < 1;
    if (!bad) {
        const uintptr_t n0 = (uintptr_t)p0->N, h = (uintptr_t)r1->cobj->N, cols = full ? 2 * h : h + 1;
        bad = overlap_bytes(d_real, sizeof(fft_type) * n0 * 2 * h * (uintptr_t)batch, d_cplx,
                            sizeof(fft_data) * n0 * cols * (uintptr_t)batch);
    }
    if (bad) hs_seterr("%s: invalid arguments", who);
    return bad ? HSFFT_ERR_ARG : 0;
}

}  // namespace tr2d

extern "C" {

int hsfft_transpose_batched(const fft_data *d_in, fft_data *d_out, int rows, int cols, int batch)
{
    hs_seterr("%s", "");
    if (!d_in || !d_out || d_in == d_out || batch < 0 || rows < 1 || cols < 1 ||
        tr2d::overlap(d_in, d_out, (long long)rows * cols * batch)) {
        hs_seterr("hsfft_transpose_batched: invalid arguments");
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    int rc = hs_require_gpu();
    if (rc) return rc;
    const int d = hs_lock_device();
    rc = tr2d::transpose(d_in, d_out, rows, cols, batch);
    hs_unlock_device(d);
    return rc;
}

int hsfft_transpose_real_batched(const fft_type *d_in, fft_type *d_out, int rows, int cols, int batch)
{
    hs_seterr("%s", "");
    bool bad = !d_in || !d_out || d_in == d_out || batch < 0 || rows < 1 || cols < 1;
    if (!bad) {
        const uintptr_t bytes = sizeof(fft_type) * (uintptr_t)rows * (uintptr_t)cols * (uintptr_t)batch;
        bad = tr2d::overlap_bytes(d_in, bytes, d_out, bytes);
    }
    if (bad) {
        hs_seterr("hsfft_transpose_real_batched: invalid arguments");
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    int rc = hs_require_gpu();
    if (rc) return rc;
    const int d = hs_lock_device();
    rc = tr2d::transpose8(d_in, d_out, rows, cols, batch);
    hs_unlock_device(d);
    return rc;
}

int hsfft_exec_2d(fft_object p0, fft_object p1, const fft_data *d_in, fft_data *d_out, int batch)
{
    hs_seterr("%s", "");
    if (!p0 || !p1 || !d_in || !d_out || d_in == d_out || batch < 0 || p0->N < 1 || p1->N < 1 ||
        tr2d::overlap(d_in, d_out, (long long)p0->N * p1->N * batch)) {
        hs_seterr("hsfft_exec_2d: invalid arguments");
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    int rc = hs_require_gpu();
    if (rc) return rc;
    const int d = hs_lock_device();
    hs_entry *e0 = hs_entry_get(p0), *e1 = hs_entry_get(p1);
    rc = e0 && e1 ? tr2d::exec_2d(e0, e1, d_in, d_out, batch) : HSFFT_ERR_ARG;
    hs_entry_put(e1);
    hs_entry_put(e0);
    hs_unlock_device(d);
    return rc;
}

int hsfft_exec_columns(fft_object p, const fft_data *d_in, fft_data *d_out, int ncols, int batch)
{
    hs_seterr("%s", "");
    if (!p || !d_in || !d_out || d_in == d_out || batch < 0 || ncols < 1 || p->N < 1 ||
        tr2d::overlap(d_in, d_out, (long long)p->N * ncols * batch)) {
        hs_seterr("hsfft_exec_columns: invalid arguments");
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    int rc = hs_require_gpu();
    if (rc) return rc;
    const int d = hs_lock_device();
    hs_entry *e = hs_entry_get(p);
    rc = e ? tr2d::exec_columns(e, d_in, d_out, ncols, batch) : HSFFT_ERR_ARG;
    hs_entry_put(e);
    hs_unlock_device(d);
    return rc;
}

/* the three real 2D entry points: mode 0 hsfft_r2c_2d, 1 hsfft_r2c_2d_full, 2 hsfft_c2r_2d */
static int real_2d(const char *who, int mode, fft_object p0, fft_real_object r1, const void *d_in, void *d_out,
                   int batch)
{
    hs_seterr("%s", "");
    int rc = tr2d::real_2d_args(who, p0, r1, mode == 2 ? d_out : d_in, mode == 2 ? d_in : d_out, mode == 1, batch);
    if (rc || batch == 0) return rc;
    rc = hs_require_gpu();
    if (rc) return rc;
    const int d = hs_lock_device();
    hs_entry *e0 = hs_entry_get(p0);
    rc = !e0         ? HSFFT_ERR_ARG
         : mode == 2 ? tr2d::c2r_2d(e0, r1, (const fft_data *)d_in, (fft_type *)d_out, batch)
                     : tr2d::r2c_2d(e0, r1, (const fft_type *)d_in, (fft_data *)d_out, batch, mode);
    hs_entry_put(e0);
    hs_unlock_device(d);
    return rc;
}

int hsfft_r2c_2d(fft_object p0, fft_real_object r1, const fft_type *d_in, fft_data *d_out, int batch)
{
    return real_2d("hsfft_r2c_2d", 0, p0, r1, d_in, d_out, batch);
}

int hsfft_r2c_2d_full(fft_object p0, fft_real_object r1, const fft_type *d_in, fft_data *d_out, int batch)
{
    return real_2d("hsfft_r2c_2d_full", 1, p0, r1, d_in, d_out, batch);
}

int hsfft_c2r_2d(fft_object p0, fft_real_object r1, const fft_data *d_in, fft_type *d_out, int batch)
{
    return real_2d("hsfft_c2r_2d", 2, p0, r1, d_in, d_out, batch);
}

int hsfft_bench_transpose_herm(const fft_data *d_in, fft_data *d_out, int n0, int n1, int batch, int iters, float *ms)
{
    hs_seterr("%s", "");
    if (!d_in || !d_out || !ms || iters < 1 || batch < 1 || n0 < 1 || n1 < 2 || n1 % 2 ||
        tr2d::overlap_bytes(d_in, sizeof(fft_data) * (uintptr_t)n0 * (n1 / 2 + 1) * batch, d_out,
                            sizeof(fft_data) * (uintptr_t)n0 * n1 * batch)) {
        hs_seterr("hsfft_bench_transpose_herm: invalid arguments");
        return HSFFT_ERR_ARG;
    }
    int rc = hs_require_gpu();
    if (rc) return rc;
    const int d = hs_lock_device();
    rc = tr2d::transpose_herm(d_in, d_out, n0, n1, batch); /* warm-up, outside the timing */
    if (!rc && hsd_timer_start()) rc = HSFFT_ERR_DEVICE;
    for (int i = 0; i < iters && !rc; i++) rc = tr2d::transpose_herm(d_in, d_out, n0, n1, batch);
    if (!rc && hsd_timer_stop(ms)) rc = HSFFT_ERR_DEVICE;
    hs_unlock_device(d);
    return rc;
}

}  // extern "C"
