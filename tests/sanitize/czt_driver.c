/*
 * czt_driver.c -- TEST INFRASTRUCTURE ONLY: the host side of the chirp-z transform (csrc/hsfft_czt.c:
 * hsfft_czt_shape, hsfft_czt_tables with its phase reduction, the per-device cache of device data
 * and its release) under -fsanitize=address,undefined against the null device (null_device.c, whose
 * "device memory" is host memory, so a cached entry can be read back).  Built and run by
 * tests/test_czt_sanitize_cpu.py.  Prints "czt sanitize: ok".
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hsfft_gpu.h"
#include "hsfft_host.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

typedef struct {
    int n, m;
    double f0, df;
} key;

/* the entry's pre, chirp and v equal hsfft_czt_tables and the wrap rule byte for byte; V (L words,
 * not yet written by anyone here) is writable to its last byte */
static int entry_is(const hs_czt_data *t, key k, int L)
{
    const size_t K = (size_t)(k.n > k.m ? k.n : k.m);
    fft_data *pre = malloc(sizeof(fft_data) * (size_t)k.n), *chirp = malloc(sizeof(fft_data) * K);
    fft_data *v = calloc((size_t)L, sizeof(fft_data));
    int ok = pre && chirp && v && hsfft_czt_tables(k.n, k.m, k.f0, k.df, pre, chirp) == 0;
    if (ok) {
        memcpy(v, chirp, sizeof(fft_data) * (size_t)k.m);
        for (int j = 1; j < k.n; j++) v[L - j] = chirp[j];
        ok = memcmp(t->pre, pre, sizeof(fft_data) * (size_t)k.n) == 0 && memcmp(t->chirp, chirp, sizeof(fft_data) * K) == 0 &&
             memcmp(t->v, v, sizeof(fft_data) * (size_t)L) == 0 && t->chirp == t->pre + k.n && t->v == t->chirp + K &&
             t->V == t->v + L;
        memset(t->V, 0, sizeof(fft_data) * (size_t)L);
    }
    free(pre);
    free(chirp);
    free(v);
    return ok;
}

static int get(int d, key k, hs_czt_data *t)
{
    int L;
    return hsfft_czt_shape(k.n, k.m, &L) == 0 && hs_czt_get(d, k.n, k.m, L, k.f0, k.df, 0, t) == 0 && entry_is(t, k, L);
}

int main(void)
{
    /* the shape and the tables: exactly n and max(n, m) words (the buffers have no spare byte) */
    int L = -7;
    CHECK(hsfft_czt_shape(40, 25, &L) == 0 && L == 64);
    CHECK(hsfft_czt_shape(40, 26, &L) == 0 && L == 128);
    CHECK(hsfft_czt_shape(1, 1, &L) == 0 && L == 2);
    CHECK(hsfft_czt_shape(1 << 25, (1 << 25) + 1, &L) == 0 && L == 1 << 26);
    CHECK(hsfft_czt_shape(7, 9, NULL) == 0);
    L = -7;
    CHECK(hsfft_czt_shape(0, 3, &L) == HSFFT_ERR_ARG && hsfft_last_error()[0] && L == -7);
    CHECK(hsfft_czt_shape(3, 0, &L) == HSFFT_ERR_ARG && hsfft_czt_shape(1 << 26, 2, &L) == HSFFT_ERR_ARG);
    CHECK(hsfft_czt_shape(0x7fffffff, 0x7fffffff, &L) == HSFFT_ERR_ARG && L == -7);
    const key sizes[] = {{1, 1, 0.5, -0.25}, {7, 5, 0.1, 0.013}, {5, 7, -0.31, -0.0021}, {1000, 3, 0.0, 1.0 / 3000.0},
                         {3, 66000, 1.0, 1.0 / (3 * 65536.0)}};
    for (size_t i = 0; i < sizeof sizes / sizeof sizes[0]; i++) {
        const key k = sizes[i];
        const int K = k.n > k.m ? k.n : k.m;
        fft_data *pre = malloc(sizeof(fft_data) * (size_t)k.n), *chirp = malloc(sizeof(fft_data) * (size_t)K);
        CHECK(pre && chirp && hsfft_czt_tables(k.n, k.m, k.f0, k.df, pre, chirp) == 0);
        CHECK(hsfft_czt_tables(k.n, k.m, k.f0, k.df, NULL, chirp) == 0 && hsfft_czt_tables(k.n, k.m, k.f0, k.df, pre, NULL) == 0);
        CHECK(hsfft_czt_tables(k.n, k.m, k.f0, k.df, NULL, NULL) == 0);
        for (int j = 0; j < K; j++) {
            CHECK(fabs(chirp[j].re * chirp[j].re + chirp[j].im * chirp[j].im - 1.0) < 1e-15);
            if (k.f0 == 0.0 && j < k.n) CHECK(memcmp(&pre[j], &chirp[j], sizeof pre[j]) == 0);
        }
        CHECK(pre[0].re == 1.0 && pre[0].im == 0.0 && chirp[0].re == 1.0 && chirp[0].im == 0.0);
        free(pre);
        free(chirp);
    }
    fft_data one[2] = {{-7.0, -7.0}, {-7.0, -7.0}};
    const double bad[] = {NAN, INFINITY, -INFINITY, 1.5, -1.0000000000000002};
    for (size_t i = 0; i < sizeof bad / sizeof bad[0]; i++) {
        CHECK(hsfft_czt_tables(1, 1, bad[i], 0.1, &one[0], &one[1]) == HSFFT_ERR_ARG && hsfft_last_error()[0]);
        CHECK(hsfft_czt_tables(1, 1, 0.1, bad[i], &one[0], &one[1]) == HSFFT_ERR_ARG && hsfft_last_error()[0]);
    }
    CHECK(hsfft_czt_tables(0, 1, 0.1, 0.1, &one[0], &one[1]) == HSFFT_ERR_ARG);
    CHECK(hsfft_czt_tables(1, -1, 0.1, 0.1, &one[0], &one[1]) == HSFFT_ERR_ARG);
    CHECK(hsfft_czt_tables(1 << 26, 2, 0.1, 0.1, &one[0], &one[1]) == HSFFT_ERR_ARG);
    CHECK(one[0].re == -7.0 && one[0].im == -7.0 && one[1].re == -7.0 && one[1].im == -7.0);

    /* the cache on two devices: five keys through the four entries, then the first again; keys that
     * differ only in df, only in f0 or only in the twiddle mode do not share an entry */
    const key k1 = {8, 5, 0.1, 0.013}, k2 = {8, 5, 0.1, 0.014}, k3 = {8, 5, 0.2, 0.013}, k4 = {40, 25, -0.3, 0.001},
              k5 = {40, 26, -0.3, 0.001};
    for (int dev = 0; dev < 2; dev++) {
        CHECK(hsfft_set_device(dev) == 0);
        const int d = hs_lock_device();
        CHECK(d == dev);
        hs_czt_data a, b, c, e, f, g;
        CHECK(get(d, k1, &a) && get(d, k2, &b) && get(d, k3, &c) && get(d, k4, &e));
        CHECK(!a.ready && !b.ready && !c.ready && !e.ready);
        CHECK(a.pre != b.pre && a.pre != c.pre && b.pre != c.pre && a.slot != b.slot && a.slot != c.slot && b.slot != c.slot);
        hs_czt_set_ready(d, a.slot);
        CHECK(get(d, k1, &g) && g.pre == a.pre && g.V == a.V && g.slot == a.slot && g.ready); /* a hit: k2 is now the oldest */
        CHECK(get(d, k5, &f) && f.slot == b.slot && !f.ready);                                /* replaces k2 */
        CHECK(get(d, k1, &g) && g.pre == a.pre && g.ready);
        CHECK(get(d, k3, &g) && g.pre == c.pre && get(d, k4, &g) && g.pre == e.pre);
        CHECK(get(d, k2, &g) && !g.ready && g.slot == f.slot);                                /* rebuilt: replaces k5, the oldest */
        hs_czt_data h;
        CHECK(hs_czt_get(d, k1.n, k1.m, 16, k1.f0, k1.df, 1, &h) == 0 && !h.ready && h.slot == a.slot); /* another mode: replaces k1 */
        CHECK(get(d, k1, &g) && !g.ready);                                                    /* k1 again, rebuilt, not ready */
        hs_czt_set_ready(d, -1);
        hs_czt_set_ready(d, 99);
        hs_czt_set_ready(-1, 0);
        hs_unlock_device(d);
    }
    CHECK(hsfft_set_device(0) == 0);
    CHECK(hsfft_release_scratch() == 0); /* device 0's entries go; a later request rebuilds */
    int d = hs_lock_device();
    hs_czt_data t;
    CHECK(get(d, k4, &t) && !t.ready);
    hs_unlock_device(d);
    CHECK(hsfft_finalize() == 0);        /* every device's: what is left would be a leak report */
    d = hs_lock_device();
    CHECK(get(d, k5, &t) && !t.ready);
    hs_czt_release_device(d);
    hs_czt_release_device(d);            /* idempotent */
    hs_czt_release_device(-1);
    hs_czt_release_device(HS_MAX_DEV);
    hs_unlock_device(d);
    CHECK(hsfft_finalize() == 0);
    printf("czt sanitize: ok\n");
    return 0;
}
