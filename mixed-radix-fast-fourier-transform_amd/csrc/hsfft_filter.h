/*
 * hsfft_filter.h -- batched overlap-add filtering of long real rows by one shared kernel
 * (hsfft_filter_shape, hsfft_filter_batched of include/hsfft_gpu.h; the reference has the one-shot
 * fft_convolve only).  Included at the end of hsfft_device.hip after hsfft_conv2d.h: the driver
 * launches its three kernels directly, so no host C file needs a new device-layer symbol.
 *
 * Each row is cut into blocks of L = P - m + 1 samples; every block is convolved with the kernel
 * at the padded length P by hs_r2c_rows() and hs_c2c_rows() unchanged, and the m - 1 samples by
 * which neighbouring blocks overlap are added.  A block's unscaled result is, word for word, what
 * hsfft_convolve_batched computes for that block and the kernel, so the output is the sum of
 * reference fft_convolve results stated in the header.  The kernel is transformed
 * once per call and the scratch is bounded by HSFFT_FILTER_CHUNK_MB, not by the job.
 */
#include "hsfft_gpu.h"
#include "hsfft_host.h"

namespace oafilt {

/* Block gather: block yi of the launch is block q = q0 + yi of the call, samples [sL, sL + L) of
 * row b = q / nseg with s = q % nseg; dst[yi][j] = x[b][sL + j] for j < min(L, n - sL), else +0.0,
 * for every j < P.  The last block of a row is shorter, and nothing is read past the end of its
 * row.  One lane writes 16 bytes (destination rows are P x 8 bytes, P even, so every pair is
 * aligned); the source offset b n + sL can be odd, so the pair is one 16-byte load where the
 * block's first sample is 16-byte aligned and two 8-byte loads elsewhere.  q is uniform over the
 * workgroup: the division runs once on the scalar unit. */
__global__ __launch_bounds__(256) void k_filter_gather(const double *__restrict__ x, long long n, long long L,
                                                       long long nseg, long long P, long long q0,
                                                       double *__restrict__ dst)
{
    const long long yi = blockIdx.y, q = q0 + yi, b = q / nseg, s = q - b * nseg;
    long long cnt = n - s * L;
    if (cnt > L) cnt = L;
    const double *src = x + b * n + s * L;
    v2d *row = (v2d *)(dst + yi * P);
    const bool al = ((uintptr_t)src & 15) == 0;
    const long long pairs = P / 2;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < pairs; i += (long long)gridDim.x * blockDim.x) {
        const long long j = 2 * i;
        v2d v = {0.0, 0.0};
        if (j + 1 < cnt) {
            if (al) v = *(const v2d *)(src + j);
            else {
                v.x = src[j];
                v.y = src[j + 1];
            }
        } else if (j < cnt)
            v.x = src[j];
        row[i] = v;
    }
}

/* k_c2r_pre_mul with the second operand at row distance 0: the product of every block's spectrum
 * with the one kernel spectrum Hs (bins 0..h), fed to real.c:169-179's inverse pre-twiddle.  Same
 * cmul1 expression with the block's spectrum as the left operand and the same t1, t2 lines, so the
 * words of Zi equal k_c2r_pre_mul's on a replicated Hs.  Hs is (h + 1) x 16 bytes, read by every
 * block of the launch: it stays in L2. */
__global__ void k_c2r_pre_mul_shared(const double2 *A, const double2 *Hs, const double2 *w2, double2 *Zi, int h,
                                     long long xdist, long long zdist)
{
    const int b = blockIdx.y;
    const double2 *x = A + b * xdist;
    double2 *z = Zi + b * zdist;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < h; k += gridDim.x * blockDim.x) {
        const double2 a = cmul1(x[k], Hs[k]), c = cmul1(x[h - k], Hs[h - k]), w = w2[k];
        const double t1 = -a.y - c.y, t2 = -c.x + a.x;
        z[k] = make_double2(a.x + c.x + (t1 * w.x) - (t2 * w.y), a.y - c.y + (t2 * w.x) + (t1 * w.y));
    }
}

struct scatter_args {
    const double *Y;     /* the chunk's unscaled block results, rows of P */
    const double *carry; /* words L..P-1 of the block before the chunk's first one */
    double *out;
    long long q0;        /* the call's block index of the launch's block 0 */
    long long y0;        /* the chunk's block index of the launch's block 0 */
    long long P, L, m, nseg, clen, start, olen;
    double div;
};

/* one word of the overlap-added full result: v_s[j] = y_s[j] / P, plus v_{s-1}[L + j] where the
 * previous block of the row reaches (s > 0 and j < m - 1), in this order, each division before
 * the add.  The previous block is the row of Y above, or the carry for the chunk's first block. */
__device__ __forceinline__ double oa_word(const scatter_args &a, const double *yrow, long long yc, long long s,
                                          long long j, double y)
{
    double v = y / a.div;
    if (s > 0 && j < a.m - 1) {
        const double p = yc > 0 ? yrow[j + a.L - a.P] : a.carry[j];
        v = v + p / a.div;
    }
    return v;
}

/* Overlap-add scatter: block s of a row owns the words g = sL + j of the row's full result with
 * j < L, and the row's last block also owns the tail up to clen, so every word of the full result
 * has one owner and the thread that owns it computes it and stores it once, where it lies inside
 * the window: out[b][g - start] for start <= g < start + olen.  No output word is read.  A lane
 * owns the pair j, j + 1 (Y rows are 16-byte aligned; one 16-byte load) and stores 16 bytes where
 * both words are inside the window and their address is aligned, else word by word.  Compiled
 * under the file's -ffp-contract=off. */
__global__ __launch_bounds__(256) void k_filter_scatter(scatter_args a)
{
    const long long yi = blockIdx.y, q = a.q0 + yi, b = q / a.nseg, s = q - b * a.nseg, yc = a.y0 + yi;
    const long long own = s == a.nseg - 1 ? a.clen - s * a.L : a.L;
    const double *yrow = a.Y + yc * a.P;
    double *orow = a.out + b * a.olen;
    const long long pairs = (own + 1) / 2;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < pairs; i += (long long)gridDim.x * blockDim.x) {
        const long long j = 2 * i, t = s * a.L + j - a.start;
        const v2d y = *(const v2d *)(yrow + j);
        const bool in0 = t >= 0 && t < a.olen, in1 = j + 1 < own && t + 1 >= 0 && t + 1 < a.olen;
        if (!in0 && !in1) continue;
        v2d v;
        if (in0) v.x = oa_word(a, yrow, yc, s, j, y.x);
        if (in1) v.y = oa_word(a, yrow, yc, s, j + 1, y.y);
        if (in0 && in1 && ((uintptr_t)(orow + t) & 15) == 0) *(v2d *)(orow + t) = v;
        else {
            if (in0) orow[t] = v.x;
            if (in1) orow[t + 1] = v.y;
        }
    }
}

/* sizes of one call */
struct shape {
    int olen, start, P, L, nseg, clen;
};

/* 0, or HSFFT_ERR_ARG with the message set */
static int get_shape(const char *type, int n, int m, int block, shape *s)
{
    if (n < 1 || m < 1 || (long long)n + m - 1 > (1LL << 30)) {
        hs_seterr("hsfft_filter: lengths %d and %d are out of range", n, m);
        return HSFFT_ERR_ARG;
    }
    const int clen = n + m - 1, big = n > m ? n : m, sm = n < m ? n : m;
    if (type == NULL || strcmp(type, "full") == 0) {
        s->start = 0;
        s->olen = clen;
    } else if (strcmp(type, "same") == 0) {
        s->start = (clen - big) / 2;
        s->olen = big;
    } else if (strcmp(type, "valid") == 0) {
        s->start = sm - 1;
        s->olen = big - sm + 1;
    } else {
        hs_seterr("hsfft_filter: output type '%s' is not 'full', 'same' or 'valid'", type);
        return HSFFT_ERR_ARG;
    }
    const int np = next_power_of_two(clen), Q = np > 2 ? np : 2;
    int P = block;
    if (block == 0) { /* automatic: four kernel lengths or the floor, whichever is larger, capped at one block */
        long long a = HSFFT_FILTER_BLOCK_MIN;
        while (a < 4LL * m) a *= 2;
        P = a < Q ? (int)a : Q;
    } else if (block < 2 || (block & (block - 1)) || block < m) {
        hs_seterr("hsfft_filter: block %d is not a power of two >= 2 and >= the kernel length %d", block, m);
        return HSFFT_ERR_ARG;
    }
    const int L = P - m + 1, nseg = (int)(((long long)n + L - 1) / L);
    if (nseg > 1 && L < m - 1) {
        hs_seterr("hsfft_filter: block %d leaves segments of %d samples, fewer than the %d a kernel of %d overlaps", P, L,
                  m - 1, m);
        return HSFFT_ERR_ARG;
    }
    s->P = P;
    s->L = L;
    s->nseg = nseg;
    s->clen = clen;
    return 0;
}

/* the device layer's status of a launch as this layer's code, message set */
static int dev_rc(int rc, const char *what)
{
    if (rc) hs_seterr("%s: %s", what, hsd_errstr());
    return rc ? HSFFT_ERR_DEVICE : 0;
}

static int gather(const fft_type *x, const shape &sh, long long n, long long q0, double *R, long long cb)
{
    for (long long b0 = 0; b0 < cb; b0 += Y_MAX) {
        const int nb = (int)(cb - b0 < Y_MAX ? cb - b0 : Y_MAX);
        hipLaunchKernelGGL(k_filter_gather, dim3(grid_for(sh.P / 2, 256), nb), dim3(256), 0, stream(), x, n, (long long)sh.L,
                           (long long)sh.nseg, (long long)sh.P, q0 + b0, R + b0 * sh.P);
        HCHK(hipGetLastError());
    }
    return 0;
}

static int pre_mul_shared(const fft_data *S, const fft_data *H, const void *tw2, fft_data *Z, int h, long long cb)
{
    for (long long b0 = 0; b0 < cb; b0 += Y_MAX) {
        const int nb = (int)(cb - b0 < Y_MAX ? cb - b0 : Y_MAX);
        hipLaunchKernelGGL(k_c2r_pre_mul_shared, dim3(grid_for(h, 256), nb), dim3(256), 0, stream(),
                           (const double2 *)S + b0 * (h + 1), (const double2 *)H, (const double2 *)tw2,
                           (double2 *)Z + b0 * h, h, (long long)h + 1, (long long)h);
        HCHK(hipGetLastError());
    }
    return 0;
}

static int scatter(const double *Y, const double *carry, fft_type *out, const shape &sh, long long m, long long q0,
                   long long cb)
{
    scatter_args a;
    a.Y = Y;
    a.carry = carry;
    a.out = out;
    a.P = sh.P;
    a.L = sh.L;
    a.m = m;
    a.nseg = sh.nseg;
    a.clen = sh.clen;
    a.start = sh.start;
    a.olen = sh.olen;
    a.div = (double)sh.P;
    for (long long b0 = 0; b0 < cb; b0 += Y_MAX) {
        const int nb = (int)(cb - b0 < Y_MAX ? cb - b0 : Y_MAX);
        a.q0 = q0 + b0;
        a.y0 = b0;
        hipLaunchKernelGGL(k_filter_scatter, dim3(grid_for(sh.P / 2, 256), nb), dim3(256), 0, stream(), a);
        HCHK(hipGetLastError());
    }
    return 0;
}

/* (device lock held) the whole call.  Blocks are numbered q = b nseg + s and walked in chunks of
 * `c` consecutive q, which may cross row boundaries, with two pool buffers: R (c x P doubles) and S
 * (c x (P/2+1) complex).  Per chunk: gather x -> R, r2c-compact rows R -> S, product with the
 * kernel's spectrum and pre-twiddle S, H -> Z (in R, dead by then), rows of the inverse plan's
 * inner c2c Z -> Y (in S, dead by then: c x P/2 complex fit), overlap-add scatter Y -> out.  Behind
 * S lie H (the kernel's P/2+1 bins, transformed once per call through R) and the carry: words
 * L..P-1 of a chunk's last block, copied there after the chunk's scatter when the next chunk
 * starts inside the same row, for that chunk's first block to add. */
static int run(fft_real_object f, fft_real_object iv, const shape &sh, const fft_type *d_x, int n, const fft_type *d_h,
               int m, fft_type *d_out, int batch)
{
    const long long P = sh.P, h = P / 2, w = h + 1, total = (long long)batch * sh.nseg;
    const size_t per = sizeof(double) * (size_t)P + sizeof(fft_data) * (size_t)w;
    long long c = (long long)(hs_env_mb("HSFFT_FILTER_CHUNK_MB", 1024.0) / per);
    if (c > total) c = total;
    if (c > 0x7fffffffLL) c = 0x7fffffffLL;
    if (c < 1) c = 1;
    double *R;
    fft_data *S;
    for (;;) {
        R = (double *)hs_scratch(HS_SCR_FILTER, sizeof(double) * (size_t)P * (size_t)c);
        S = R ? (fft_data *)hs_scratch(HS_SCR_CONV_SPEC,
                                       sizeof(fft_data) * (size_t)w * (size_t)(c + 1) + sizeof(double) * (size_t)m)
              : NULL;
        if (S || c == 1) break;
        c = (c + 1) / 2;
    }
    if (!S) {
        hs_seterr("hsfft_filter_batched: scratch allocation failed (%lld blocks of P = %lld)", c, P);
        return HSFFT_ERR_NOMEM;
    }
    fft_data *H = S + c * w;
    double *carry = (double *)(H + w);
    hs_entry *e_inv = hs_entry_get(iv->cobj);
    void *tw2 = e_inv ? hs_real_tw2_device(iv) : NULL;
    int rc = !e_inv ? HSFFT_ERR_ARG : !tw2 ? HSFFT_ERR_DEVICE : 0;
    if (!rc) rc = dev_rc(hsd_copy_rows(d_h, m, 0, m, R, P, P, 1), "filter kernel padding");
    if (!rc) rc = hs_r2c_rows(f, R, H, 1, 1);
    for (long long q0 = 0; q0 < total && !rc; q0 += c) {
        const long long cb = total - q0 < c ? total - q0 : c;
        rc = dev_rc(gather(d_x, sh, n, q0, R, cb), "filter block gather");
        if (!rc) rc = hs_r2c_rows(f, R, S, (int)cb, 1);
        if (!rc) rc = dev_rc(pre_mul_shared(S, H, tw2, (fft_data *)R, (int)h, cb), "filter product");
        if (!rc) rc = tr2d::rows(e_inv, (const fft_data *)R, S, cb);
        if (!rc) rc = dev_rc(scatter((const double *)S, carry, d_out, sh, m, q0, cb), "filter overlap-add");
        if (!rc && m > 1 && q0 + cb < total && (q0 + cb) % sh.nseg != 0)
            rc = dev_rc(hsd_d2d_async(carry, (const double *)S + (cb - 1) * P + sh.L, sizeof(double) * (size_t)(m - 1)),
                        "filter carry");
    }
    hs_entry_put(e_inv);
    return rc;
}

}  // namespace oafilt

extern "C" {

int hsfft_filter_shape(const char *type, int n, int m, int block, int *out_len, int *P, int *L, int *nseg)
{
    hs_seterr("%s", "");
    oafilt::shape sh;
    const int rc = oafilt::get_shape(type, n, m, block, &sh);
    if (rc) return rc;
    if (out_len) *out_len = sh.olen;
    if (P) *P = sh.P;
    if (L) *L = sh.L;
    if (nseg) *nseg = sh.nseg;
    return 0;
}

int hsfft_filter_batched(const char *type, const fft_type *d_x, int n, const fft_type *d_h, int m, int block,
                         fft_type *d_out, int batch)
{
    hs_seterr("%s", "");
    if (!d_x || !d_h || !d_out || batch < 0) {
        hs_seterr("hsfft_filter_batched: invalid arguments");
        return HSFFT_ERR_ARG;
    }
    oafilt::shape sh;
    int rc = oafilt::get_shape(type, n, m, block, &sh);
    if (rc) return rc;
    const uintptr_t nb = (uintptr_t)batch, esz = sizeof(fft_type);
    const uintptr_t out_bytes = esz * (uintptr_t)sh.olen * nb;
    if (tr2d::overlap_bytes(d_out, out_bytes, d_x, esz * (uintptr_t)n * nb) ||
        tr2d::overlap_bytes(d_out, out_bytes, d_h, batch ? esz * (uintptr_t)m : 0)) {
        hs_seterr("hsfft_filter_batched: the output overlaps an input");
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    rc = hs_require_gpu();
    if (rc) return rc;
    const hs_conv_pair rp = hs_conv_plans(sh.P);
    if (!rp.f || !rp.i) {
        hs_seterr("hsfft_filter_batched: planning the block length %d failed", sh.P);
        rc = HSFFT_ERR_NOMEM;
    } else {
        const int d = hs_lock_device();
        rc = oafilt::run(rp.f, rp.i, sh, d_x, n, d_h, m, d_out, batch);
        hs_unlock_device(d);
    }
    hs_conv_plans_done(rp);
    return rc;
}

}  // extern "C"
