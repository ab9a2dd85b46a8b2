/*
 * dct4_driver.c -- TEST INFRASTRUCTURE ONLY: the host side of the type-IV cosine and sine transforms
 * (csrc/hsfft_dct4.c: the rotation table, hsfft_dct4_twiddles, the per-device cache of device
 * copies and its release) under -fsanitize=address,undefined against the null device
 * (null_device.c, whose "device memory" is host memory, so a cached table can be read back).
 * Built and run by tests/test_dct4_sanitize_cpu.py.  Prints "dct4 sanitize: ok".
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

/* the cached copy of n's table equals hsfft_dct4_twiddles(n) byte for byte */
static int table_is(const void *d, int n)
{
    const size_t bytes = sizeof(fft_data) * ((size_t)n / 2);
    fft_data *t = malloc(bytes);
    const int ok = t && hsfft_dct4_twiddles(n, t) == 0 && memcmp(t, d, bytes) == 0;
    free(t);
    return ok;
}

int main(void)
{
    /* the table: exactly n/2 words (the buffer has no spare byte), one sincos each */
    for (int n = 2; n <= 4098; n += n < 64 ? 2 : 1006) {
        fft_data *t = malloc(sizeof(fft_data) * ((size_t)n / 2));
        CHECK(t && hsfft_dct4_twiddles(n, t) == 0);
        for (int j = 0; j < n / 2; j++) {
            double s, c;
            sincos(PI2 * (double)(8 * j + 1) / (16.0 * (double)n), &s, &c);
            CHECK(memcmp(&t[j].re, &c, sizeof c) == 0 && memcmp(&t[j].im, &s, sizeof s) == 0);
            CHECK(c > 0.0 && s > 0.0); /* every angle lies inside (0, pi / 2) */
        }
        free(t);
    }
    fft_data one = {-7.0, -7.0};
    const int bad[] = {0, 1, -2, 7, (1 << 30) + 2};
    for (size_t i = 0; i < sizeof bad / sizeof bad[0]; i++) {
        CHECK(hsfft_dct4_twiddles(bad[i], &one) == HSFFT_ERR_ARG && hsfft_last_error()[0]);
        CHECK(one.re == -7.0 && one.im == -7.0);
    }
    CHECK(hsfft_dct4_twiddles(6, NULL) == HSFFT_ERR_ARG);

    /* the cache on two devices: four entries, least recently used replaced, release frees; the
     * types II / III cache beside it is another one */
    for (int dev = 0; dev < 2; dev++) {
        CHECK(hsfft_set_device(dev) == 0);
        const int d = hs_lock_device();
        CHECK(d == dev);
        const void *p8 = hs_dct4_table(d, 8), *p16 = hs_dct4_table(d, 16), *p32 = hs_dct4_table(d, 32),
                   *p64 = hs_dct4_table(d, 64);
        CHECK(p8 && p16 && p32 && p64);
        const void *o8 = hs_dct_table(d, 8);
        CHECK(o8 && o8 != p8);
        CHECK(hs_dct4_table(d, 8) == p8 && hs_dct4_table(d, 64) == p64); /* hits: 16 is now the oldest */
        const void *p128 = hs_dct4_table(d, 128);                        /* replaces 16 */
        CHECK(p128 && table_is(p128, 128));
        CHECK(hs_dct4_table(d, 8) == p8 && hs_dct4_table(d, 32) == p32 && hs_dct4_table(d, 64) == p64);
        CHECK(table_is(p8, 8) && table_is(p32, 32) && table_is(p64, 64));
        const void *q16 = hs_dct4_table(d, 16);                          /* rebuilt: replaces 128, the oldest */
        CHECK(q16 && table_is(q16, 16));
        CHECK(hs_dct4_table(d, 8) == p8 && hs_dct4_table(d, 32) == p32 && hs_dct4_table(d, 64) == p64);
        const void *big = hs_dct4_table(d, 1 << 16);                     /* replaces 16 */
        CHECK(big && table_is(big, 1 << 16));
        const void *two = hs_dct4_table(d, 2);                           /* one word; replaces 8 */
        CHECK(two && table_is(two, 2));
        CHECK(hs_dct_table(d, 8) == o8);                                 /* the other cache was not disturbed */
        hs_unlock_device(d);
    }
    CHECK(hsfft_set_device(0) == 0);
    CHECK(hsfft_release_scratch() == 0); /* device 0's tables go; a later request rebuilds */
    int d = hs_lock_device();
    const void *again = hs_dct4_table(d, 64);
    CHECK(again && table_is(again, 64));
    hs_unlock_device(d);
    CHECK(hsfft_finalize() == 0);        /* every device's: what is left would be a leak report */
    d = hs_lock_device();
    again = hs_dct4_table(d, 6);
    CHECK(again && table_is(again, 6));
    hs_dct4_release_device(d);
    hs_dct4_release_device(d);           /* idempotent */
    hs_dct4_release_device(-1);
    hs_dct4_release_device(HS_MAX_DEV);
    hs_unlock_device(d);
    CHECK(hsfft_finalize() == 0);
    printf("dct4 sanitize: ok\n");
    return 0;
}
