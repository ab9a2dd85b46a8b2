/*
 * hsfft_dct4.c -- host side of the type-IV cosine and sine transforms and of the MDCT built on
 * them (hsfft_dct4.h holds the kernels and the drivers): the rotation table t[j] = (cos, sin)(pi
 * (8j+1) / 8n), hsfft_dct4_twiddles, and the per-device cache of the table's device copies.  Host C
 * on the device layer's interface, like hsfft_dct.c, whose table and cache stay as they are:
 * hsfft_release_scratch and hsfft_finalize (hsfft_exec.c) reach hs_dct4_release_device in every
 * build of the host code, with or without the HIP translation unit.
 */
#define _GNU_SOURCE /* sincos */
#include <math.h>
#include <stdlib.h>

#include "hsfft_gpu.h"
#include "hsfft_host.h"

/* the contract's table: one libm sincos per word, the angle exactly as the header writes it */
static void fill_table(int n, fft_data *t)
{
    for (long long j = 0; j < n / 2; j++) {
        double s, c;
        sincos(PI2 * (double)(8 * j + 1) / (16.0 * (double)n), &s, &c);
        t[j].re = c;
        t[j].im = s;
    }
}

int hsfft_dct4_twiddles(int n, fft_data *h_tw)
{
    hs_seterr("%s", "");
    if (n < 2 || (n & 1) || n > HS_DCT_MAX_LEN) {
        hs_seterr("hsfft_dct4_twiddles: the length %d is odd, below 2 or above 2^30", n);
        return HSFFT_ERR_ARG;
    }
    if (!h_tw) {
        hs_seterr("hsfft_dct4_twiddles: NULL table");
        return HSFFT_ERR_ARG;
    }
    fill_table(n, h_tw);
    return 0;
}

/* Device copies of the table, per device: keyed by n, 4 entries, the least recently used one
 * replaced.  Touched only under the device lock of `dev`, so it needs no lock of its own. */
#define HS_DCT4_NTAB 4
static struct {
    int n;
    void *d;
    unsigned long long used;
} g_tab[HS_MAX_DEV][HS_DCT4_NTAB];
static unsigned long long g_tab_clock[HS_MAX_DEV];

const void *hs_dct4_table(int dev, int n)
{
    int slot = 0;
    for (int i = 0; i < HS_DCT4_NTAB; i++) {
        if (g_tab[dev][i].d && g_tab[dev][i].n == n) {
            g_tab[dev][i].used = ++g_tab_clock[dev];
            return g_tab[dev][i].d;
        }
        /* an empty slot before any used one, else the least recently used */
        if (g_tab[dev][slot].d && (!g_tab[dev][i].d || g_tab[dev][i].used < g_tab[dev][slot].used)) slot = i;
    }
    const size_t bytes = sizeof(fft_data) * ((size_t)n / 2);
    fft_data *h = malloc(bytes);
    if (!h) {
        hs_seterr("hsfft_dct4_batched: no host memory for the table of %d", n);
        return NULL;
    }
    fill_table(n, h);
    if (g_tab[dev][slot].d) { /* queued kernels may still read the table that goes */
        (void)hsd_sync();
        hsd_free(g_tab[dev][slot].d);
        g_tab[dev][slot].d = NULL;
    }
    void *d = hsd_malloc(bytes);
    if (d && hsd_h2d(d, h, bytes)) {
        hsd_free(d);
        d = NULL;
    }
    free(h);
    if (!d) {
        hs_seterr("hsfft_dct4_batched: uploading the table of %d failed: %s", n, hsd_errstr());
        return NULL;
    }
    g_tab[dev][slot].n = n;
    g_tab[dev][slot].d = d;
    g_tab[dev][slot].used = ++g_tab_clock[dev];
    return d;
}

void hs_dct4_release_device(int dev)
{
    if (dev < 0 || dev >= HS_MAX_DEV) return;
    for (int i = 0; i < HS_DCT4_NTAB; i++) {
        hsd_free(g_tab[dev][i].d);
        g_tab[dev][i].d = NULL;
        g_tab[dev][i].n = 0;
        g_tab[dev][i].used = 0;
    }
}
