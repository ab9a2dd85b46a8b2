/*
 * hsfft_dct2d.h -- batched 2D DCT-II / DCT-III and DST-II / DST-III of real images
 * (hsfft_dct_2d_batched of include/hsfft_gpu.h; the reference has no cosine or sine transform).
 * Included at the end of hsfft_device.hip after hsfft_dct.h: the driver calls dct::run and launches
 * the transpose directly, so no host C file needs a new device-layer symbol.
 *
 * The row transforms are dct::run unchanged and tr2d::k_transpose8 is a pure copy, so a 2D result
 * is, word for word, hsfft_dct_batched applied to every row and then to every column of that
 * result -- the shape of tr2d::exec_2d with 8-byte elements.
 */
#include "hsfft_gpu.h"
#include "hsfft_host.h"

namespace dct2d {

/* (device lock held) rows of (sin1, n1) then columns of (sin0, n0) of `batch` n0 x n1 images, per
 * chunk with one scratch copy T of the chunk in HS_SCR_2D: rows in -> T, transpose T -> out, rows
 * out -> T (the columns, now contiguous), transpose T -> out.  d_in is only read.  dct::run keeps
 * its own buffers (HS_SCR_DCT, HS_SCR_DCT_SPEC) and its own inner chunk walk; both rotation tables
 * stay in the four-entry cache while the two lengths alternate. */
static int run(int dev, int sin0, int sin1, int type, hs_conv_pair p0, hs_conv_pair p1, const fft_type *in, fft_type *out,
               int n0, int n1, int batch)
{
    const long long img = (long long)n0 * n1; /* even: counted in 16-byte elements by chunk_scratch */
    long long ci;
    fft_type *T = (fft_type *)tr2d::chunk_scratch(img / 2, n0 > n1 ? n0 : n1, 1, batch, &ci);
    if (!T) return HSFFT_ERR_NOMEM;
    for (long long b0 = 0; b0 < batch; b0 += ci) {
        const long long cb = batch - b0 < ci ? batch - b0 : ci;
        const fft_type *ib = in + b0 * img;
        fft_type *ob = out + b0 * img;
        int rc = dct::run(dev, sin1, type, p1.f, p1.i, ib, T, n1, (int)(cb * n0));
        if (!rc) rc = tr2d::transpose8(T, ob, n0, n1, cb);
        if (!rc) rc = dct::run(dev, sin0, type, p0.f, p0.i, ob, T, n0, (int)(cb * n1));
        if (!rc) rc = tr2d::transpose8(T, ob, n1, n0, cb);
        if (rc) return rc;
    }
    return 0;
}

static bool bad_len(int n) { return n < 2 || (n & 1) || n > HS_DCT_MAX_LEN; }

}  // namespace dct2d

extern "C" {

int hsfft_dct_2d_batched(int kind0, int kind1, int type, const fft_type *d_in, fft_type *d_out, int n0, int n1, int batch)
{
    hs_seterr("%s", "");
    if ((kind0 != HSFFT_KIND_COS && kind0 != HSFFT_KIND_SIN) || (kind1 != HSFFT_KIND_COS && kind1 != HSFFT_KIND_SIN) ||
        (type != 2 && type != 3)) {
        hs_seterr("hsfft_dct_2d_batched: kind %d or %d is not 0 (cosine) or 1 (sine), or type %d is not 2 or 3", kind0, kind1,
                  type);
        return HSFFT_ERR_ARG;
    }
    if (dct2d::bad_len(n0) || dct2d::bad_len(n1)) {
        hs_seterr("hsfft_dct_2d_batched: the image of %d x %d has an axis that is odd, below 2 or above 2^30", n0, n1);
        return HSFFT_ERR_ARG;
    }
    if (!d_in || !d_out || batch < 0) {
        hs_seterr("hsfft_dct_2d_batched: NULL pointer or negative batch");
        return HSFFT_ERR_ARG;
    }
    const long long img = (long long)n0 * n1;
    if (batch && (img > dct::MAX_WORDS || batch > dct::MAX_WORDS / img)) {
        hs_seterr("hsfft_dct_2d_batched: %d images of %d x %d are more than the call can index", batch, n0, n1);
        return HSFFT_ERR_ARG;
    }
    const uintptr_t bytes = sizeof(fft_type) * (uintptr_t)img * (uintptr_t)batch;
    if (batch && (d_in == d_out || tr2d::overlap_bytes(d_out, bytes, d_in, bytes))) {
        hs_seterr("hsfft_dct_2d_batched: the output overlaps the input");
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 0;
    int rc = hs_require_gpu();
    if (rc) return rc;
    const hs_conv_pair p1 = hs_conv_plans(n1), p0 = hs_conv_plans(n0);
    if (!p0.f || !p0.i || !p1.f || !p1.i) {
        hs_seterr("hsfft_dct_2d_batched: planning the lengths %d and %d failed", n0, n1);
        rc = HSFFT_ERR_NOMEM;
    } else {
        const int d = hs_lock_device();
        rc = dct2d::run(d, kind0 == HSFFT_KIND_SIN, kind1 == HSFFT_KIND_SIN, type, p0, p1, d_in, d_out, n0, n1, batch);
        hs_unlock_device(d);
    }
    hs_conv_plans_done(p0);
    hs_conv_plans_done(p1);
    return rc;
}

}  // extern "C"
