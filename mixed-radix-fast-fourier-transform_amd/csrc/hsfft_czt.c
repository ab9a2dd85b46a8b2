/*
 * hsfft_czt.c -- host side of the chirp-z transform (hsfft_czt.h holds the kernels and the drivers):
 * hsfft_czt_shape, the two phase tables of hsfft_czt_tables with their exact phase reduction, and the
 * per-device cache of a transform's device data -- the input rotation, the chirp, the wrapped chirp
 * v and room for its spectrum V.  Host C on the device layer's interface, like hsfft_dct4.c:
 * hsfft_release_scratch and hsfft_finalize (hsfft_exec.c) reach hs_czt_release_device in every build
 * of the host code, with or without the HIP translation unit.
 */
#define _GNU_SOURCE /* sincos */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "hsfft_gpu.h"
#include "hsfft_host.h"

/* 0 with *L set, or HSFFT_ERR_ARG with the message set: n, m >= 1 and n + m - 1 <= 2^26 */
int hs_czt_sizes(const char *who, int n, int m, int *L)
{
    if (n < 1 || m < 1 || (long long)n + m - 1 > HS_CZT_MAX_SUM) {
        hs_seterr("%s: n %d or m %d is below 1, or n + m - 1 is above 2^26", who, n, m);
        return HSFFT_ERR_ARG;
    }
    int p = 2;
    while (p < n + m - 1) p *= 2;
    *L = p;
    return 0;
}

/* 0, or HSFFT_ERR_ARG with the message set: both finite and at most 1 in magnitude */
int hs_czt_freqs(const char *who, double f0, double df)
{
    if (!(fabs(f0) <= 1.0) || !(fabs(df) <= 1.0)) { /* a NaN fails both comparisons */
        hs_seterr("%s: f0 %g or df %g is not finite or above 1 in magnitude (frequencies are periodic: reduce them)", who, f0,
                  df);
        return HSFFT_ERR_ARG;
    }
    return 0;
}

int hsfft_czt_shape(int n, int m, int *L)
{
    hs_seterr("%s", "");
    int p;
    const int rc = hs_czt_sizes("hsfft_czt_shape", n, m, &p);
    if (rc) return rc;
    if (L) *L = p;
    return 0;
}

/* a b mod 2 in half-turns: the rounded product's residue (fmod is exact) plus the product's exact
 * error, one rounded add.  a is an integer below 2^53 and |b| <= 1, so nothing overflows. */
static double red(double a, double b)
{
    const double p = a * b;
    const double e = fma(a, b, -p);
    return fmod(p, 2.0) + e;
}

/* the contract's word: one libm sincos of the phase in half-turns */
static fft_data word(double ph)
{
    fft_data w;
    double s, c;
    sincos(PI2 * (0.5 * ph), &s, &c);
    w.re = c;
    w.im = s;
    return w;
}

static void fill_tables(int n, int m, double f0, double df, fft_data *pre, fft_data *chirp)
{
    const long long K = n > m ? n : m;
    for (long long j = 0; chirp && j < K; j++) chirp[j] = word(red((double)j * (double)j, df));
    for (long long j = 0; pre && j < n; j++) pre[j] = word(red((double)(2 * j), f0) + red((double)j * (double)j, df));
}

int hsfft_czt_tables(int n, int m, double f0, double df, fft_data *h_pre, fft_data *h_chirp)
{
    const char *who = "hsfft_czt_tables";
    hs_seterr("%s", "");
    int L;
    int rc = hs_czt_sizes(who, n, m, &L);
    if (!rc) rc = hs_czt_freqs(who, f0, df);
    if (rc) return rc;
    fill_tables(n, m, f0, df, h_pre, h_chirp);
    return 0;
}

/* Device data of a transform, per device: keyed by (n, m, the bits of f0 and df, twiddle mode), 4
 * entries, the least recently used one replaced.  One allocation per entry: pre (n words), chirp
 * (K), v (L) and V (L).  Touched only under the device lock of `dev`, so it needs no lock of its
 * own. */
#define HS_CZT_NTAB 4
static struct {
    int n, m, mode, ready;
    double f0, df; /* compared as bits */
    fft_data *d;
    unsigned long long used;
} g_tab[HS_MAX_DEV][HS_CZT_NTAB];
static unsigned long long g_tab_clock[HS_MAX_DEV];

static void fill_data(hs_czt_data *out, int dev, int slot, int L)
{
    const long long n = g_tab[dev][slot].n, m = g_tab[dev][slot].m, K = n > m ? n : m;
    out->pre = g_tab[dev][slot].d;
    out->chirp = g_tab[dev][slot].d + n;
    out->v = g_tab[dev][slot].d + n + K;
    out->V = g_tab[dev][slot].d + n + K + L;
    out->slot = slot;
    out->ready = g_tab[dev][slot].ready;
}

int hs_czt_get(int dev, int n, int m, int L, double f0, double df, int mode, hs_czt_data *out)
{
    int slot = 0;
    for (int i = 0; i < HS_CZT_NTAB; i++) {
        if (g_tab[dev][i].d && g_tab[dev][i].n == n && g_tab[dev][i].m == m && g_tab[dev][i].mode == mode &&
            memcmp(&g_tab[dev][i].f0, &f0, sizeof f0) == 0 && memcmp(&g_tab[dev][i].df, &df, sizeof df) == 0) {
            g_tab[dev][i].used = ++g_tab_clock[dev];
            fill_data(out, dev, i, L);
            return 0;
        }
        /* an empty slot before any used one, else the least recently used */
        if (g_tab[dev][slot].d && (!g_tab[dev][i].d || g_tab[dev][i].used < g_tab[dev][slot].used)) slot = i;
    }
    const size_t K = (size_t)(n > m ? n : m), host_words = (size_t)n + K + (size_t)L;
    fft_data *h = malloc(sizeof(fft_data) * host_words);
    if (!h) {
        hs_seterr("hsfft_czt_batched: no host memory for the tables of n %d, m %d", n, m);
        return HSFFT_ERR_NOMEM;
    }
    fft_data *chirp = h + n, *v = h + n + K;
    fill_tables(n, m, f0, df, h, chirp);
    /* v: the chirp at 0 .. m-1, its mirror at L-n+1 .. L-1, +0.0 between (L >= n + m - 1: no clash) */
    memset(v, 0, sizeof(fft_data) * (size_t)L);
    memcpy(v, chirp, sizeof(fft_data) * (size_t)m);
    for (long long j = 1; j < n; j++) v[L - j] = chirp[j];
    if (g_tab[dev][slot].d) { /* queued kernels may still read the entry that goes */
        (void)hsd_sync();
        hsd_free(g_tab[dev][slot].d);
        g_tab[dev][slot].d = NULL;
    }
    void *d = hsd_malloc(sizeof(fft_data) * (host_words + (size_t)L));
    if (d && hsd_h2d(d, h, sizeof(fft_data) * host_words)) {
        hsd_free(d);
        d = NULL;
    }
    free(h);
    if (!d) {
        hs_seterr("hsfft_czt_batched: uploading the tables of n %d, m %d failed: %s", n, m, hsd_errstr());
        return HSFFT_ERR_NOMEM;
    }
    g_tab[dev][slot].n = n;
    g_tab[dev][slot].m = m;
    g_tab[dev][slot].mode = mode;
    g_tab[dev][slot].ready = 0;
    g_tab[dev][slot].f0 = f0;
    g_tab[dev][slot].df = df;
    g_tab[dev][slot].d = d;
    g_tab[dev][slot].used = ++g_tab_clock[dev];
    fill_data(out, dev, slot, L);
    return 0;
}

void hs_czt_set_ready(int dev, int slot)
{
    if (dev >= 0 && dev < HS_MAX_DEV && slot >= 0 && slot < HS_CZT_NTAB && g_tab[dev][slot].d) g_tab[dev][slot].ready = 1;
}

void hs_czt_release_device(int dev)
{
    if (dev < 0 || dev >= HS_MAX_DEV) return;
    for (int i = 0; i < HS_CZT_NTAB; i++) {
        hsd_free(g_tab[dev][i].d);
        memset(&g_tab[dev][i], 0, sizeof g_tab[dev][i]);
    }
}
