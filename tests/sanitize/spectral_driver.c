/*
 * spectral_driver.c -- TEST INFRASTRUCTURE ONLY: the host side of the analytic signal and of Fourier
 * resampling (csrc/hsfft_spectral.c: the length rule, the chunk rule of hsfft_spectral_chunk_rows and
 * the whole argument check of the two entry points) under -fsanitize=address,undefined against the
 * null device (null_device.c).  No pointer handed to a check is dereferenced by it, so the "device
 * pointers" here are plain numbers.  Built and run by tests/test_spectral_sanitize_cpu.py.  Prints
 * "spectral sanitize: ok".
 */
#define _GNU_SOURCE
#include <stdint.h>
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

#define BIG (1 << 30)
static const void *const X = (const void *)(uintptr_t)0x100000, *const O = (const void *)(uintptr_t)0x300000;
static const void *at(const void *p, long long off) { return (const void *)((uintptr_t)p + (uintptr_t)off); }

static int rejected(int rc, const char *word)
{
    return rc == HSFFT_ERR_ARG && strstr(hsfft_last_error(), word) != NULL;
}

/* the documented rule in plain integers */
static long long rule(long long bytes, long long n, long long m)
{
    const long long per = 16 * (n / 2 + 1) + (m ? 16 * (m / 2 + 1) : 16 * n), c = bytes / per;
    return c < 1 ? 1 : c;
}

int main(void)
{
    const char *h = "hsfft_hilbert_batched", *r = "hsfft_resample_batched";
    /* the valid calls: 3 rows of 100 samples to 3 rows of 100 complex or of 60 reals */
    CHECK(hs_spectral_args(h, X, 100, O, 0, 3, 1) == 0 && hs_spectral_args(r, X, 100, O, 60, 3, 0) == 0);
    CHECK(hs_spectral_args(r, X, 100, O, 100, 3, 0) == 0 && hs_spectral_args(r, X, 2, O, BIG, 1, 0) == 0);
    CHECK(hs_spectral_args(h, X, BIG, at(X, 8LL * BIG), 0, 1, 1) == 0); /* the largest row, the output right behind it */
    CHECK(hs_spectral_args(h, X, 100, X, 0, 0, 1) == 0 && hs_spectral_args(r, X, 100, X, 60, 0, 0) == 0); /* empty ranges */
    /* pointers and batch */
    CHECK(rejected(hs_spectral_args(h, NULL, 100, O, 0, 3, 1), "NULL") && rejected(hs_spectral_args(h, X, 100, NULL, 0, 3, 1), "NULL"));
    CHECK(rejected(hs_spectral_args(r, NULL, 100, O, 60, 3, 0), "NULL") && rejected(hs_spectral_args(r, X, 100, O, 60, -1, 0), "negative"));
    CHECK(rejected(hs_spectral_args(h, X, 100, O, 0, -2147483647 - 1, 1), "negative"));
    /* lengths: the message names the call */
    const int bad[] = {0, 1, -2, 3, 101, BIG + 2, 2147483647, -2147483647 - 1};
    for (size_t i = 0; i < sizeof bad / sizeof bad[0]; i++) {
        CHECK(rejected(hs_spectral_args(h, X, bad[i], O, 0, 3, 1), "odd, below 2 or above 2^30") && strstr(hsfft_last_error(), h));
        CHECK(rejected(hs_spectral_args(r, X, bad[i], O, 60, 3, 0), "odd, below 2 or above 2^30") && strstr(hsfft_last_error(), r));
        CHECK(rejected(hs_spectral_args(r, X, 100, O, bad[i], 3, 0), "odd, below 2 or above 2^30"));
        CHECK(hs_spectral_sizes(h, bad[i], 0, 1) == HSFFT_ERR_ARG && hs_spectral_sizes(r, 8, bad[i], 0) == HSFFT_ERR_ARG);
        long long rows = -7;
        CHECK(hsfft_spectral_chunk_rows(bad[i], 0, &rows) == HSFFT_ERR_ARG && rows == -7);
        if (bad[i]) CHECK(hsfft_spectral_chunk_rows(8, bad[i], &rows) == HSFFT_ERR_ARG && rows == -7);
    }
    CHECK(hs_spectral_sizes(h, 8, 8, 1) == HSFFT_ERR_ARG); /* the Hilbert call has no second length */
    CHECK(hs_spectral_sizes(h, 2, 0, 1) == 0 && hs_spectral_sizes(h, BIG, 0, 1) == 0 && hs_spectral_sizes(r, 2, BIG, 0) == 0);
    /* totals: 2^40 words pass, one row more does not; the products do not overflow */
    CHECK(hs_spectral_args(h, X, BIG, at(X, 1LL << 60), 0, 1024, 1) == 0);
    CHECK(rejected(hs_spectral_args(h, X, BIG, at(X, 1LL << 60), 0, 1025, 1), "more than the call can index"));
    CHECK(rejected(hs_spectral_args(r, X, BIG, at(X, 1LL << 60), 2, 1025, 0), "more than the call can index"));
    CHECK(rejected(hs_spectral_args(r, X, 2, at(X, 1LL << 60), BIG, 1025, 0), "more than the call can index"));
    CHECK(rejected(hs_spectral_args(r, X, BIG, at(X, 1LL << 60), BIG, 2147483647, 0), "more than the call can index"));
    /* alignment: 16 bytes on either side */
    const int off[] = {1, 4, 8, 12};
    for (size_t i = 0; i < sizeof off / sizeof off[0]; i++) {
        CHECK(rejected(hs_spectral_args(h, at(X, off[i]), 100, O, 0, 3, 1), "16-byte aligned"));
        CHECK(rejected(hs_spectral_args(h, X, 100, at(O, off[i]), 0, 3, 1), "16-byte aligned"));
        CHECK(rejected(hs_spectral_args(r, at(X, off[i]), 100, O, 60, 3, 0), "16-byte aligned"));
        CHECK(rejected(hs_spectral_args(r, X, 100, at(O, off[i]), 60, 3, 0), "16-byte aligned"));
    }
    /* overlap: any shared byte, each range with its own size; neighbours pass */
    CHECK(rejected(hs_spectral_args(h, X, 100, X, 0, 3, 1), "overlaps") && rejected(hs_spectral_args(r, X, 100, X, 60, 3, 0), "overlaps"));
    CHECK(rejected(hs_spectral_args(h, X, 100, at(X, 2400 - 16), 0, 3, 1), "overlaps") && hs_spectral_args(h, X, 100, at(X, 2400), 0, 3, 1) == 0);
    CHECK(rejected(hs_spectral_args(h, at(O, 4800 - 16), 100, O, 0, 3, 1), "overlaps") && hs_spectral_args(h, at(O, 4800), 100, O, 0, 3, 1) == 0);
    CHECK(rejected(hs_spectral_args(r, at(O, 1440 - 16), 100, O, 60, 3, 0), "overlaps") && hs_spectral_args(r, at(O, 1440), 100, O, 60, 3, 0) == 0);
    CHECK(rejected(hs_spectral_args(r, X, 100, at(X, 1600), 60, 3, 0), "overlaps") && hs_spectral_args(r, X, 100, at(X, 1600), 60, 2, 0) == 0);
    CHECK(rejected(hs_spectral_args(h, X, 100, at(X, 1600), 0, 3, 1), "overlaps") && hs_spectral_args(h, X, 100, at(X, 1600), 0, 2, 1) == 0);
    /* a range that ends at the top of the address space does not wrap into a false overlap */
    CHECK(hs_spectral_args(r, (const void *)(UINTPTR_MAX - 2400 + 1), 100, O, 60, 3, 0) == 0);

    /* the chunk rule, at the default knob and at others; the knob is read per call */
    const int sizes[][2] = {{2, 0}, {2, 2}, {64, 0}, {3000, 0}, {3000, 2000}, {2000, 3000}, {65536, 0}, {65536, 32768},
                            {BIG, 0}, {BIG, BIG}, {BIG, 2}, {2, BIG}};
    const struct {
        const char *knob;
        long long bytes;
    } knobs[] = {{NULL, 1024LL << 20}, {"1", 1 << 20}, {"0", 1 << 20}, {"0.001", 1 << 20}, {"64", 64 << 20},
                 {"2.5", 2621440}, {"junk", 1 << 20}, {"16384", 16384LL << 20}};
    for (size_t k = 0; k < sizeof knobs / sizeof knobs[0]; k++) {
        if (knobs[k].knob) CHECK(setenv("HSFFT_SPECTRAL_CHUNK_MB", knobs[k].knob, 1) == 0);
        else CHECK(unsetenv("HSFFT_SPECTRAL_CHUNK_MB") == 0);
        for (size_t i = 0; i < sizeof sizes / sizeof sizes[0]; i++) {
            const int n = sizes[i][0], m = sizes[i][1];
            long long rows = -7;
            CHECK(hsfft_spectral_chunk_rows(n, m, &rows) == 0 && rows == rule(knobs[k].bytes, n, m) && rows >= 1);
            CHECK(hs_spectral_rows(n, m) == rows && hsfft_spectral_chunk_rows(n, m, NULL) == 0);
        }
    }
    CHECK(setenv("HSFFT_SPECTRAL_CHUNK_MB", "1", 1) == 0);
    long long rows;
    CHECK(hsfft_spectral_chunk_rows(3000, 0, &rows) == 0 && rows == 14);
    CHECK(hsfft_spectral_chunk_rows(3000, 2000, &rows) == 0 && rows == 26);
    CHECK(unsetenv("HSFFT_SPECTRAL_CHUNK_MB") == 0);
    CHECK(hsfft_last_error()[0] == 0); /* a call that succeeds clears the message */
    CHECK(hsfft_finalize() == 0);
    printf("spectral sanitize: ok\n");
    return 0;
}
