/*
 * hsfft_conv2d.h -- batched 2D convolution of real images (hsfft_convolve_2d_shape,
 * hsfft_convolve_2d_batched of include/hsfft_gpu.h; the reference has the 1D fft_convolve only).
 * Included at the end of hsfft_device.hip after hsfft_2d.h: the driver uses the tr2d helpers and
 * the device layer's existing convolution helpers (hsd_copy_rows, hsd_cmul, hsd_copy_rows_div), so
 * no host C file needs a new device-layer symbol and no kernel is added.
 *
 * The transforms are hs_r2c_rows() / hs_c2r_rows() / hs_c2c_rows() unchanged and the transposes
 * are pure copies, so a result is, word for word, hsfft_c2r_2d of the elementwise product of two
 * hsfft_r2c_2d spectra of the zero-padded images, divided once and windowed.  The
 * product runs on the transposed half spectra [k1][k0]: it is elementwise, so the last transpose
 * of each forward transform and the first of the inverse, which cancel, are never run.
 */
#include "hsfft_gpu.h"
#include "hsfft_host.h"

namespace conv2d {

/* the device layer's status of a copy / product launch as this layer's code, message set */
static int dev_rc(int rc, const char *what)
{
    if (rc) hs_seterr("%s: %s", what, hsd_errstr());
    return rc ? HSFFT_ERR_DEVICE : 0;
}

/* Zero padding with the 1D convolution's row copy (hsd_copy_rows: dst[i] = i < ncopy ? src[i] :
 * +0.0, every word of the destination rows written): `cb` images of n0 x n1 doubles go to the
 * top-left of images of P0 x P1 doubles in `dst`.  First the columns -- the cb x n0 rows of n1
 * become rows of P1 -- then the rows, with each image as one "row" of n0 x P1 words that becomes one
 * of P0 x P1.  The second step needs `tmp` (cb x n0 x P1 doubles) and is skipped where n0 == P0. */
static int pad(const fft_type *in, long long n0, long long n1, long long P0, long long P1, double *tmp, double *dst,
               long long cb)
{
    double *cols = n0 == P0 ? dst : tmp;
    int rc = hsd_copy_rows(in, n1, 0, n1, cols, P1, P1, (int)(cb * n0));
    if (!rc && n0 != P0) rc = hsd_copy_rows(tmp, n0 * P1, 0, n0 * P1, dst, P0 * P1, P0 * P1, (int)cb);
    return dev_rc(rc, "2D convolution padding");
}

/* Window and scale with the 1D convolution's copies: the orows x ocols window at (s0, s1) of each
 * of `cb` images of P0 x P1 doubles in `src`, divided once per element, goes to contiguous images
 * in `out`.  First the rows -- each image as one "row", orows x P1 words from s0 x P1 on, into `tmp`;
 * skipped where the window has every row -- then the columns with the division
 * (hsd_copy_rows_div), which writes the batch x orows x ocols outputs and nothing else. */
static int window(const double *src, long long P0, long long P1, long long s0, long long s1, long long orows,
                  long long ocols, double *tmp, fft_type *out, long long cb, double div)
{
    int rc = 0;
    if (orows != P0) {
        rc = hsd_copy_rows(src, P0 * P1, s0 * P1, orows * P1, tmp, orows * P1, orows * P1, (int)cb);
        src = tmp;
    }
    if (!rc) rc = hsd_copy_rows_div(src, P1, s1, out, ocols, ocols, (int)(cb * orows), div);
    return dev_rc(rc, "2D convolution window");
}

/* Spectral product in place, x[b][i] = x[b][i] * y[b][i] over `cb` images of `img` elements, by
 * the 1D convolution's k_cmul (hsd_cmul: re = x.re y.re - x.im y.im, im = x.re y.im + x.im y.re,
 * the operand order of convolve.c:149-150, compiled under -ffp-contract=off).  It is elementwise,
 * so it does not care that both operands are transposed half spectra. */
static int product(fft_data *x, const fft_data *y, long long img, long long cb)
{
    return dev_rc(hsd_cmul(x, y, x, img, (int)cb, img), "2D convolution product");
}

/* sizes of one call, from the per-axis rule of the 1D convolution (hs_conv_axis) */
struct shape {
    int P0, P1, s0, s1, orows, ocols;
};

/* 0, or HSFFT_ERR_ARG with the message set */
static int get_shape(const char *type, const char *conv_type, int a_rows, int a_cols, int b_rows, int b_cols, shape *s)
{
    if (!conv_type) {
        hs_seterr("2D convolution: NULL convolution type");
        return HSFFT_ERR_ARG;
    }
    s->orows = hs_conv_axis(type, conv_type, a_rows, b_rows, &s->P0, &s->s0);
    if (s->orows < 0) return HSFFT_ERR_ARG;
    s->ocols = hs_conv_axis(type, conv_type, a_cols, b_cols, &s->P1, &s->s1);
    if (s->ocols < 0) return HSFFT_ERR_ARG;
    if (s->P1 < 2) { /* both widths 1: the reference's real plan of length 1 exits (real.c:26-31) */
        hs_seterr("2D convolution of two images of width 1: transform length %d is not even", s->P1);
        return HSFFT_ERR_ARG;
    }
    if (s->orows < 1 || s->ocols < 1) {
        hs_seterr("2D convolution: empty output window of %d x %d", s->orows, s->ocols);
        return HSFFT_ERR_ARG;
    }
    return 0;
}

/* forward transform of `cb` zero-padded images into the transposed half spectra T ([k1][k0], w
 * rows of P0): pad -> S0 (P0 x P1 reals, through X), r2c-compact rows S0 -> X, transpose X -> S0,
 * rows of e0 S0 -> T.  X may be T. */
static int forward(hs_entry *e0, fft_real_object r1, const fft_type *in, int n0, int n1, long long P0, long long P1,
                   fft_data *S0, fft_data *X, fft_data *T, long long cb)
{
    const long long w = P1 / 2 + 1;
    int rc = pad(in, n0, n1, P0, P1, (double *)X, (double *)S0, cb);
    if (!rc) rc = hs_r2c_rows(r1, (const fft_type *)S0, X, (int)(cb * P0), 1);
    if (!rc) rc = tr2d::transpose(X, S0, P0, w, cb);
    if (!rc) rc = tr2d::rows(e0, S0, T, cb * w);
    return rc;
}

/* (device lock held) the whole call, per chunk of `ci` image pairs with three chunk-sized slots
 * S0, S1, S2 of the HS_SCR_2D buffer (an image is the half spectrum, P0 x w elements; the padded
 * real image is smaller and fits a slot): A^T into S1 and B^T into S2 by forward(), product S1 .*
 * S2 -> S1, rows of the inverse column plan S1 -> S2, transpose S2 -> S0 (P0 x w), c2r rows S0
 * (pitch w) -> S1 as P0 x P1 reals, window / divide S1 -> out (through S0).  A shared kernel
 * (b_batch 1) is transformed once per call into one more image behind the three slots and copied
 * into every image of S2 per chunk (a row copy with source stride 0). */
static int run(hs_entry *e_p0, hs_entry *e_q0, fft_real_object r1, fft_real_object s1, const shape &sh,
               const fft_type *d_a, int a_rows, int a_cols, const fft_type *d_b, int b_rows, int b_cols, int shared,
               fft_type *d_out, int batch)
{
    const long long P0 = sh.P0, P1 = sh.P1, w = P1 / 2 + 1;
    const long long img = tr2d::half_image("hsfft_convolve_2d_batched", P0, w);
    if (!img) return HSFFT_ERR_ARG;
    long long ci;
    fft_data *S0 = (fft_data *)tr2d::chunk_scratch(img, (int)(P0 > w ? P0 : w), 3, batch, &ci, shared ? img : 0);
    if (!S0) return HSFFT_ERR_NOMEM;
    fft_data *S1 = S0 + ci * img, *S2 = S1 + ci * img, *BT = S2 + ci * img;
    const long long oimg = (long long)sh.orows * sh.ocols;
    const double div = (double)(P0 * P1);
    int rc = 0;
    if (shared) rc = forward(e_p0, r1, d_b, b_rows, b_cols, P0, P1, S0, S2, BT, 1);
    for (long long b0 = 0; b0 < batch && !rc; b0 += ci) {
        const long long cb = batch - b0 < ci ? batch - b0 : ci;
        rc = forward(e_p0, r1, d_a + b0 * a_rows * a_cols, a_rows, a_cols, P0, P1, S0, S1, S1, cb);
        if (!rc && !shared) rc = forward(e_p0, r1, d_b + b0 * b_rows * b_cols, b_rows, b_cols, P0, P1, S0, S2, S2, cb);
        if (!rc && shared) /* every image of S2 <- the one spectrum, as rows of 2 x img doubles */
            rc = dev_rc(hsd_copy_rows(BT, 0, 0, 2 * img, S2, 2 * img, 2 * img, (int)cb), "2D convolution kernel copy");
        if (!rc) rc = product(S1, S2, img, cb);
        if (!rc) rc = tr2d::rows(e_q0, S1, S2, cb * w);
        if (!rc) rc = tr2d::transpose(S2, S0, w, P0, cb);
        if (!rc) rc = hs_c2r_rows(s1, S0, NULL, w, (fft_type *)S1, (int)(cb * P0));
        if (!rc)
            rc = window((const double *)S1, P0, P1, sh.s0, sh.s1, sh.orows, sh.ocols, (double *)S0, d_out + b0 * oimg, cb,
                        div);
    }
    return rc;
}

}  // namespace conv2d

extern "C" {

int hsfft_convolve_2d_shape(const char *type, const char *conv_type, int a_rows, int a_cols, int b_rows, int b_cols,
                            int *out_rows, int *out_cols, int *pad_rows, int *pad_cols)
{
    hs_seterr("%s", "");
    conv2d::shape sh;
    const int rc = conv2d::get_shape(type, conv_type, a_rows, a_cols, b_rows, b_cols, &sh);
    if (rc) return rc;
    if (out_rows) *out_rows = sh.orows;
    if (out_cols) *out_cols = sh.ocols;
    if (pad_rows) *pad_rows = sh.P0;
    if (pad_cols) *pad_cols = sh.P1;
    return 0;
}

int hsfft_convolve_2d_batched(const char *type, const char *conv_type, const fft_type *d_a, int a_rows, int a_cols,
                              const fft_type *d_b, int b_rows, int b_cols, int b_batch, fft_type *d_out, int batch)
{
    hs_seterr("%s", "");
    if (!d_a || !d_b || !d_out || batch < 0 || (batch > 0 && b_batch != 1 && b_batch != batch)) {
        hs_seterr("hsfft_convolve_2d_batched: invalid arguments");
        return HSFFT_ERR_ARG;
    }
    conv2d::shape sh;
    int rc = conv2d::get_shape(type, conv_type, a_rows, a_cols, b_rows, b_cols, &sh);
    if (rc) return rc;
    const uintptr_t nb = (uintptr_t)batch, esz = sizeof(fft_type);
    const uintptr_t out_bytes = esz * (uintptr_t)sh.orows * (uintptr_t)sh.ocols * nb;
    if (tr2d::overlap_bytes(d_out, out_bytes, d_a, esz * (uintptr_t)a_rows * (uintptr_t)a_cols * nb) ||
        tr2d::overlap_bytes(d_out, out_bytes, d_b, esz * (uintptr_t)b_rows * (uintptr_t)b_cols * (batch ? b_batch : 0))) {
        hs_seterr("hsfft_convolve_2d_batched: the output overlaps an input");
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    rc = hs_require_gpu();
    if (rc) return rc;
    const hs_conv_pair rp = hs_conv_plans(sh.P1);
    const hs_conv_cpair cp = hs_conv_cplans(sh.P0);
    if (!rp.f || !rp.i || !cp.f || !cp.i) {
        hs_seterr("hsfft_convolve_2d_batched: planning the padded size %d x %d failed", sh.P0, sh.P1);
        rc = HSFFT_ERR_NOMEM;
    } else {
        const int d = hs_lock_device();
        hs_entry *e_p0 = hs_entry_get(cp.f), *e_q0 = hs_entry_get(cp.i);
        rc = e_p0 && e_q0 ? conv2d::run(e_p0, e_q0, rp.f, rp.i, sh, d_a, a_rows, a_cols, d_b, b_rows, b_cols,
                                        b_batch == 1 && batch > 1 ? 1 : 0, d_out, batch)
                          : HSFFT_ERR_ARG;
        hs_entry_put(e_q0);
        hs_entry_put(e_p0);
        hs_unlock_device(d);
    }
    hs_conv_cplans_done(cp);
    hs_conv_plans_done(rp);
    return rc;
}

}  // extern "C"
