/*
 * hsfft_spectral.c -- host side of the analytic signal and of Fourier resampling (hsfft_spectral.h
 * holds the two kernels and the driver): the size and limit rules, the chunk rule behind
 * hsfft_spectral_chunk_rows, and the whole argument check of hsfft_hilbert_batched and
 * hsfft_resample_batched.  Host C on no device symbol at all, like the size rules of hsfft_czt.c:
 * every rejection is reached in any build of the host code, with or without the HIP translation unit.
 */
#include <stdint.h>

#include "hsfft_gpu.h"
#include "hsfft_host.h"

static int bad_len(int n) { return n < 2 || (n & 1) || n > HS_SPECTRAL_MAX_LEN; }

/* 0, or HSFFT_ERR_ARG with the message set: n even in [2, 2^30]; m the same, or 0 (no second length:
 * the Hilbert call) where `hilbert` is set */
int hs_spectral_sizes(const char *who, int n, int m, int hilbert)
{
    if (bad_len(n) || (hilbert ? m != 0 : bad_len(m))) {
        if (hilbert) hs_seterr("%s: the length %d is odd, below 2 or above 2^30", who, n);
        else hs_seterr("%s: the length n %d or m %d is odd, below 2 or above 2^30", who, n, m);
        return HSFFT_ERR_ARG;
    }
    return 0;
}

/* the scratch bytes of one row: its n/2+1 compact bins and the edited spectrum behind them, n words
 * (Hilbert, m == 0) or m/2+1 (resample) */
static size_t row_bytes(int n, int m)
{
    const size_t bins = (size_t)n / 2 + 1;
    return sizeof(fft_data) * (bins + (m ? (size_t)m / 2 + 1 : (size_t)n));
}

/* rows per chunk before the clamp to the batch: the knob's bytes over a row's, at least 1 */
long long hs_spectral_rows(int n, int m)
{
    const long long c = (long long)(hs_env_mb("HSFFT_SPECTRAL_CHUNK_MB", 1024.0) / row_bytes(n, m));
    return c < 1 ? 1 : c;
}

int hsfft_spectral_chunk_rows(int n, int m, long long *rows)
{
    hs_seterr("%s", "");
    const int rc = hs_spectral_sizes("hsfft_spectral_chunk_rows", n, m, m == 0);
    if (rc) return rc;
    if (rows) *rows = hs_spectral_rows(n, m);
    return 0;
}

/* the byte ranges [a, a + na) and [b, b + nb) share a byte */
static int overlap_bytes(const void *a, uintptr_t na, const void *b, uintptr_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb ? pb - pa < na : pa - pb < nb;
}

/* Every rejection of the two entry points, in the order the header lists them; m == 0 with `hilbert`
 * set.  The input is n x 8 bytes per row, the output n x 16 (Hilbert) or m x 8 (resample).  0, or
 * HSFFT_ERR_ARG with the message set; no device is touched. */
int hs_spectral_args(const char *who, const void *d_in, int n, const void *d_out, int m, int batch, int hilbert)
{
    if (!d_in || !d_out || batch < 0) {
        hs_seterr("%s: NULL pointer or negative batch", who);
        return HSFFT_ERR_ARG;
    }
    const int rc = hs_spectral_sizes(who, n, m, hilbert);
    if (rc) return rc;
    if ((long long)n * batch > HS_SPECTRAL_MAX_WORDS || (long long)m * batch > HS_SPECTRAL_MAX_WORDS) {
        if (hilbert) hs_seterr("%s: %d rows of %d are more than the call can index", who, batch, n);
        else hs_seterr("%s: %d rows of %d or %d are more than the call can index", who, batch, n, m);
        return HSFFT_ERR_ARG;
    }
    /* the row transforms read d_in and write d_out in 16-byte words */
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 15) {
        hs_seterr("%s: d_in and d_out must be 16-byte aligned (the row transforms access them in 16-byte words)", who);
        return HSFFT_ERR_ARG;
    }
    const uintptr_t nb = (uintptr_t)batch;
    const uintptr_t out_bytes = hilbert ? sizeof(fft_data) * (uintptr_t)n * nb : sizeof(fft_type) * (uintptr_t)m * nb;
    if (overlap_bytes(d_out, out_bytes, d_in, sizeof(fft_type) * (uintptr_t)n * nb)) {
        hs_seterr("%s: the output overlaps the input", who);
        return HSFFT_ERR_ARG;
    }
    return 0;
}
