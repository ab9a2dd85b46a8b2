/*
 * hsfft_dct1.c -- host side of the type-I cosine and sine transforms (hsfft_dct1.h holds the two
 * kernels and the drivers): the extended length and its limits, hsfft_dct1_shape, the chunk rule,
 * and the whole argument check of hsfft_dct1_batched and hsfft_dct1_2d_batched.  Host C on no device
 * symbol at all, like hsfft_spectral.c: every rejection is reached in any build of the host code,
 * with or without the HIP translation unit.
 */
#include <stdint.h>

#include "hsfft_gpu.h"
#include "hsfft_host.h"

/* 0 with *L = 2(n-1) (cosine, n >= 2) or 2(n+1) (sine, n >= 1), or HSFFT_ERR_ARG with the message
 * set: a kind other than 0 or 1, n below that, or L above 2^30.  L may be NULL. */
int hs_dct1_sizes(const char *who, int kind, int n, int *L)
{
    if (kind != HSFFT_KIND_COS && kind != HSFFT_KIND_SIN) {
        hs_seterr("%s: kind %d is not 0 (cosine) or 1 (sine)", who, kind);
        return HSFFT_ERR_ARG;
    }
    const long long ext = kind == HSFFT_KIND_SIN ? 2 * ((long long)n + 1) : 2 * ((long long)n - 1);
    if (n < (kind == HSFFT_KIND_SIN ? 1 : 2) || ext > HS_DCT_MAX_LEN) {
        hs_seterr("%s: the length %d is below %d, or its extension of %s words is above 2^30", who, n,
                  kind == HSFFT_KIND_SIN ? 1 : 2, kind == HSFFT_KIND_SIN ? "2(n+1)" : "2(n-1)");
        return HSFFT_ERR_ARG;
    }
    if (L) *L = (int)ext;
    return 0;
}

int hsfft_dct1_shape(int kind, int n, int *L, int *bins)
{
    hs_seterr("%s", "");
    int ext;
    const int rc = hs_dct1_sizes("hsfft_dct1_shape", kind, n, &ext);
    if (rc) return rc;
    if (L) *L = ext;
    if (bins) *bins = ext / 2 + 1;
    return 0;
}

/* rows per chunk before the clamp to the batch: the knob's bytes over the scratch bytes of one
 * row -- L doubles and L/2+1 bins -- at least 1 */
long long hs_dct1_rows(int L)
{
    const size_t per = sizeof(fft_type) * (size_t)L + sizeof(fft_data) * ((size_t)L / 2 + 1);
    const long long c = (long long)(hs_env_mb("HSFFT_DCT_CHUNK_MB", 1024.0) / per);
    return c < 1 ? 1 : c;
}

/* the byte ranges [a, a + na) and [b, b + nb) share a byte */
static int overlap_bytes(const void *a, uintptr_t na, const void *b, uintptr_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb ? pb - pa < na : pa - pb < nb;
}

/* pointers, batch, the total of `words` per item, and overlap: the part both entry points share */
static int buffers(const char *who, const void *d_in, const void *d_out, long long words, int batch, const char *items)
{
    if (!d_in || !d_out || batch < 0) {
        hs_seterr("%s: NULL pointer or negative batch", who);
        return HSFFT_ERR_ARG;
    }
    if (batch && (words > HS_DCT1_MAX_WORDS || batch > HS_DCT1_MAX_WORDS / words)) {
        hs_seterr("%s: %d %s of %lld words are more than the call can index", who, batch, items, words);
        return HSFFT_ERR_ARG;
    }
    const uintptr_t bytes = sizeof(fft_type) * (uintptr_t)words * (uintptr_t)batch;
    if (batch && (d_in == d_out || overlap_bytes(d_out, bytes, d_in, bytes))) {
        hs_seterr("%s: the output overlaps the input", who);
        return HSFFT_ERR_ARG;
    }
    return 0;
}

/* Every rejection of hsfft_dct1_batched, in the order of hsfft_dct_batched: kind, length, pointers
 * and batch, total, overlap.  0 with *L set, or HSFFT_ERR_ARG with the message set; no device is
 * touched. */
int hs_dct1_args(const char *who, int kind, const void *d_in, const void *d_out, int n, int batch, int *L)
{
    const int rc = hs_dct1_sizes(who, kind, n, L);
    return rc ? rc : buffers(who, d_in, d_out, n, batch, "rows");
}

/* the same for hsfft_dct1_2d_batched: kind0 and n0 along the columns, kind1 and n1 along the rows */
int hs_dct1_args_2d(const char *who, int kind0, int kind1, const void *d_in, const void *d_out, int n0, int n1, int batch,
                    int *L0, int *L1)
{
    int rc = hs_dct1_sizes(who, kind0, n0, L0);
    if (!rc) rc = hs_dct1_sizes(who, kind1, n1, L1);
    return rc ? rc : buffers(who, d_in, d_out, (long long)n0 * n1, batch, "images");
}
