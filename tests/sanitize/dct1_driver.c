/*
 * dct1_driver.c -- TEST INFRASTRUCTURE ONLY: the host side of the type-I cosine and sine transforms
 * (csrc/hsfft_dct1.c: the kind and length rule, hsfft_dct1_shape, the chunk rule and the whole
 * argument check of hsfft_dct1_batched and hsfft_dct1_2d_batched) under -fsanitize=address,undefined
 * against the null device (null_device.c).  No pointer handed to a check is dereferenced by it, so
 * the "device pointers" here are plain numbers.  Built and run by tests/test_dct1_sanitize_cpu.py.
 * Prints "dct1 sanitize: ok".
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

#define HALF (1 << 29)
#define INT_LO (-2147483647 - 1)
/* 8-byte aligned only: the calls need the alignment of a double */
static const void *const X = (const void *)(uintptr_t)0x100008, *const O = (const void *)(uintptr_t)0x300008;
static const void *at(const void *p, long long off) { return (const void *)((uintptr_t)p + (uintptr_t)off); }

static int rejected(int rc, const char *word)
{
    return rc == HSFFT_ERR_ARG && strstr(hsfft_last_error(), word) != NULL;
}

/* the documented rule in plain integers */
static long long rule(long long bytes, long long L)
{
    const long long c = bytes / (L * 8 + (L / 2 + 1) * 16);
    return c < 1 ? 1 : c;
}

int main(void)
{
    const char *w = "hsfft_dct1_batched", *w2 = "hsfft_dct1_2d_batched";
    const int C = HSFFT_KIND_COS, S = HSFFT_KIND_SIN;
    int L = -7, L0 = -7, L1 = -7, bins = -7;

    /* the length rule and the shape helper, at both ends of both kinds */
    CHECK(hs_dct1_sizes(w, C, 2, &L) == 0 && L == 2 && hs_dct1_sizes(w, S, 1, &L) == 0 && L == 4);
    CHECK(hs_dct1_sizes(w, C, HALF + 1, &L) == 0 && L == 1 << 30 && hs_dct1_sizes(w, S, HALF - 1, &L) == 0 && L == 1 << 30);
    CHECK(hs_dct1_sizes(w, C, 7, NULL) == 0 && hs_dct1_sizes(w, S, 7, &L) == 0 && L == 16);
    L = -7;
    const int badc[] = {1, 0, -1, -3, HALF + 2, 1 << 30, 2147483647, INT_LO};
    const int bads[] = {0, -1, -3, HALF, 1 << 30, 2147483647, INT_LO};
    for (size_t i = 0; i < sizeof badc / sizeof badc[0]; i++) {
        CHECK(rejected(hs_dct1_sizes(w, C, badc[i], &L), "is below 2") && strstr(hsfft_last_error(), w) && L == -7);
        CHECK(rejected(hsfft_dct1_shape(C, badc[i], &L, &bins), "above 2^30") && L == -7 && bins == -7);
        CHECK(rejected(hs_dct1_args(w, C, X, O, badc[i], 3, &L), "is below 2"));
        CHECK(rejected(hs_dct1_args_2d(w2, C, S, X, O, badc[i], 7, 3, &L0, &L1), "is below 2") && strstr(hsfft_last_error(), w2));
        CHECK(rejected(hs_dct1_args_2d(w2, S, C, X, O, 7, badc[i], 3, &L0, &L1), "is below 2"));
    }
    for (size_t i = 0; i < sizeof bads / sizeof bads[0]; i++) {
        CHECK(rejected(hs_dct1_sizes(w, S, bads[i], &L), "is below 1") && L == -7);
        CHECK(rejected(hsfft_dct1_shape(S, bads[i], &L, &bins), "above 2^30") && L == -7 && bins == -7);
        CHECK(rejected(hs_dct1_args(w, S, X, O, bads[i], 3, &L), "is below 1"));
        CHECK(rejected(hs_dct1_args_2d(w2, S, S, X, O, bads[i], 7, 3, &L0, &L1), "is below 1"));
    }
    const int badk[] = {2, -1, 3, 2147483647, INT_LO};
    for (size_t i = 0; i < sizeof badk / sizeof badk[0]; i++) {
        CHECK(rejected(hs_dct1_sizes(w, badk[i], 8, &L), "is not 0 (cosine) or 1 (sine)") && L == -7);
        CHECK(rejected(hsfft_dct1_shape(badk[i], 8, &L, &bins), "is not 0 (cosine) or 1 (sine)"));
        CHECK(rejected(hs_dct1_args(w, badk[i], X, O, 101, 3, &L), "is not 0"));
        CHECK(rejected(hs_dct1_args_2d(w2, badk[i], C, X, O, 5, 7, 3, &L0, &L1), "is not 0"));
        CHECK(rejected(hs_dct1_args_2d(w2, C, badk[i], X, O, 5, 7, 3, &L0, &L1), "is not 0"));
    }
    CHECK(hsfft_dct1_shape(C, 9, NULL, NULL) == 0 && hsfft_dct1_shape(C, 9, &L, &bins) == 0 && L == 16 && bins == 9);
    CHECK(hsfft_dct1_shape(S, 9, &L, NULL) == 0 && L == 20 && hsfft_dct1_shape(S, 1, NULL, &bins) == 0 && bins == 3);
    CHECK(hsfft_dct1_shape(C, 2, &L, &bins) == 0 && L == 2 && bins == 2);
    CHECK(hsfft_dct1_shape(C, HALF + 1, &L, &bins) == 0 && L == 1 << 30 && bins == HALF + 1);

    /* the valid calls: 3 rows of 101 doubles (2424 bytes), 3 images of 5 x 7 (840 bytes); empty ranges */
    CHECK(hs_dct1_args(w, C, X, O, 101, 3, &L) == 0 && L == 200 && hs_dct1_args(w, S, X, O, 101, 3, &L) == 0 && L == 204);
    CHECK(hs_dct1_args_2d(w2, C, S, X, O, 5, 7, 3, &L0, &L1) == 0 && L0 == 8 && L1 == 16);
    CHECK(hs_dct1_args_2d(w2, S, S, X, O, 1, 1, 3, &L0, &L1) == 0 && L0 == 4 && L1 == 4);
    CHECK(hs_dct1_args(w, C, X, X, 101, 0, &L) == 0 && hs_dct1_args_2d(w2, C, C, X, X, 5, 7, 0, &L0, &L1) == 0);
    /* pointers and batch */
    CHECK(rejected(hs_dct1_args(w, C, NULL, O, 101, 3, &L), "NULL") && rejected(hs_dct1_args(w, C, X, NULL, 101, 3, &L), "NULL"));
    CHECK(rejected(hs_dct1_args(w, S, X, O, 101, -1, &L), "negative") && rejected(hs_dct1_args(w, S, X, O, 101, INT_LO, &L), "negative"));
    CHECK(rejected(hs_dct1_args_2d(w2, C, C, NULL, O, 5, 7, 3, &L0, &L1), "NULL"));
    CHECK(rejected(hs_dct1_args_2d(w2, C, C, X, NULL, 5, 7, 3, &L0, &L1), "NULL"));
    CHECK(rejected(hs_dct1_args_2d(w2, C, C, X, O, 5, 7, -1, &L0, &L1), "negative"));
    /* totals: 2^40 words pass, more do not; the products do not overflow */
    const void *far = at(X, 1LL << 60);
    CHECK(hs_dct1_args(w, C, X, far, 1 << 29, 2048, &L) == 0);
    CHECK(rejected(hs_dct1_args(w, C, X, far, HALF + 1, 2048, &L), "more than the call can index"));
    CHECK(rejected(hs_dct1_args(w, S, X, far, HALF - 1, 2147483647, &L), "more than the call can index"));
    CHECK(hs_dct1_args_2d(w2, C, C, X, far, 1 << 20, 1 << 20, 1, &L0, &L1) == 0);
    CHECK(rejected(hs_dct1_args_2d(w2, C, C, X, far, 1 << 20, 1 << 20, 2, &L0, &L1), "more than the call can index"));
    CHECK(rejected(hs_dct1_args_2d(w2, C, C, X, far, 1 << 21, 1 << 20, 1, &L0, &L1), "more than the call can index"));
    CHECK(rejected(hs_dct1_args_2d(w2, C, S, X, far, HALF + 1, HALF - 1, 2147483647, &L0, &L1), "more than the call can index"));
    CHECK(hs_dct1_args_2d(w2, C, S, X, far, HALF + 1, HALF - 1, 0, &L0, &L1) == 0); /* an empty batch indexes nothing */
    /* overlap: any shared byte; neighbours pass; an odd row length keeps every pointer 8-byte aligned only */
    CHECK(rejected(hs_dct1_args(w, C, X, X, 101, 3, &L), "overlaps"));
    CHECK(rejected(hs_dct1_args(w, C, X, at(X, 2424 - 8), 101, 3, &L), "overlaps") && hs_dct1_args(w, C, X, at(X, 2424), 101, 3, &L) == 0);
    CHECK(rejected(hs_dct1_args(w, S, at(O, 2424 - 8), O, 101, 3, &L), "overlaps") && hs_dct1_args(w, S, at(O, 2424), O, 101, 3, &L) == 0);
    CHECK(rejected(hs_dct1_args(w, C, X, at(X, 1616), 101, 3, &L), "overlaps") && hs_dct1_args(w, C, X, at(X, 1616), 101, 2, &L) == 0);
    CHECK(rejected(hs_dct1_args_2d(w2, C, C, X, X, 5, 7, 3, &L0, &L1), "overlaps"));
    CHECK(rejected(hs_dct1_args_2d(w2, C, C, X, at(X, 840 - 8), 5, 7, 3, &L0, &L1), "overlaps"));
    CHECK(hs_dct1_args_2d(w2, C, C, X, at(X, 840), 5, 7, 3, &L0, &L1) == 0);
    CHECK(rejected(hs_dct1_args_2d(w2, S, C, at(O, 840 - 8), O, 5, 7, 3, &L0, &L1), "overlaps"));
    /* a range that ends at the top of the address space does not wrap into a false overlap */
    CHECK(hs_dct1_args(w, C, (const void *)(UINTPTR_MAX - 2424 + 1), O, 101, 3, &L) == 0);

    /* the chunk rule, at the default knob and at others; the knob is read per call */
    const int lens[] = {2, 4, 12, 200, 4096, 25200, 65536, 1 << 30};
    const struct {
        const char *knob;
        long long bytes;
    } knobs[] = {{NULL, 1024LL << 20}, {"1", 1 << 20}, {"0", 1 << 20}, {"0.001", 1 << 20}, {"64", 64 << 20},
                 {"2.5", 2621440}, {"junk", 1 << 20}, {"16384", 16384LL << 20}};
    for (size_t k = 0; k < sizeof knobs / sizeof knobs[0]; k++) {
        if (knobs[k].knob) CHECK(setenv("HSFFT_DCT_CHUNK_MB", knobs[k].knob, 1) == 0);
        else CHECK(unsetenv("HSFFT_DCT_CHUNK_MB") == 0);
        for (size_t i = 0; i < sizeof lens / sizeof lens[0]; i++)
            CHECK(hs_dct1_rows(lens[i]) == rule(knobs[k].bytes, lens[i]) && hs_dct1_rows(lens[i]) >= 1);
    }
    CHECK(setenv("HSFFT_DCT_CHUNK_MB", "1", 1) == 0);
    CHECK(hs_dct1_rows(4096) == 15 && 1048576 / 65552 == 15); /* n = 2049 (cosine) and 2047 (sine) */
    CHECK(unsetenv("HSFFT_DCT_CHUNK_MB") == 0);
    CHECK(hsfft_dct1_shape(C, 9, &L, &bins) == 0 && hsfft_last_error()[0] == 0); /* a call that succeeds clears the message */
    CHECK(hsfft_finalize() == 0);
    printf("dct1 sanitize: ok\n");
    return 0;
}
