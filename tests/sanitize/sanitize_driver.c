/*
 * sanitize_driver.c -- TEST INFRASTRUCTURE ONLY (tests/test_sanitize_cpu.py).
 *
 * Runs the host C of libhsfft.so (csrc/hsfft_plan.c, hsfft_schedule.c, hsfft_exec.c, hsfft_real.c,
 * hsfft_convolve.c, hsfft_measure.c, hsfft_crash.c) against the null device (null_device.c) under
 * -fsanitize=address,undefined:
 *   1. planner: fft_init's public fields and twiddle bytes equal the oracle's plan for every
 *      N <= PLAN_MAX and a list of larger sizes (ref highSpeedFFT.c:206-286, :1979-2313);
 *   2. registry + scheduler: every size through fft_exec, hsfft_exec_batched, the host
 *      pipeline, r2c / c2r (both layouts), convolution (every output type), a plan whose
 *      public fields are edited between calls (registry rebuild), hsfft_plan_refresh,
 *      hsfft_release_scratch -- the null device touches the first and last element of every
 *      row each launch would read or write;
 *   3. threads: 8 host threads creating / executing / freeing plans, sharing one plan, and
 *      cycling convolutions through more padded lengths than the plan cache holds;
 *   4. devices: hsfft_exec_multi over the 4 null devices the test asks for (HSFFT_NULL_NDEV):
 *      one host thread per device building its own device state, shards of uneven size, two
 *      callers at once, then free_fft releasing the state of every device.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "highspeedFFT.h"
#include "hsfft_gpu.h"
#include "real.h"
#include "../../oracle/hsfft_oracle.h"

#define PLAN_MAX 3000

static int fails;

#define CHECK(c, ...)                         \
    do {                                      \
        if (!(c)) {                           \
            fprintf(stderr, "FAIL: " __VA_ARGS__); \
            fprintf(stderr, "\n");            \
            fails++;                          \
        }                                     \
    } while (0)

static void check_plan(int n, int sgn)
{
    fft_object o = fft_init(n, sgn);
    orc_plan *r = orc_plan_create(n, sgn, 0);
    CHECK(o && r, "plan %d", n);
    if (!o || !r) return;
    int fac[64];
    const int lf = orc_plan_factors(r, fac);
    long long mplan = 1;
    for (int i = 0; i < o->lf; i++) mplan *= o->factors[i];
    if (o->lt == 1 && mplan != orc_plan_M(r)) { /* D5 (N = 2^k+1): the oracle keeps the exec-length table */
        orc_plan_destroy(r);
        free_fft(o);
        return;
    }
    CHECK(o->lf == lf && o->lt == orc_plan_lt(r) && o->N == n && o->sgn == sgn, "plan fields N=%d", n);
    for (int i = 0; i < lf && i < o->lf; i++) CHECK(o->factors[i] == fac[i], "factor %d of N=%d", i, n);
    const int M = orc_plan_M(r);
    if (M > 1) CHECK(!memcmp(o->twiddle, orc_plan_twiddles(r), sizeof(fft_data) * (size_t)(M - 1)), "twiddles N=%d", n);
    orc_plan_destroy(r);
    free_fft(o);
}

static fft_data *cbuf(long long n)
{
    fft_data *p = malloc(sizeof(fft_data) * (size_t)(n > 0 ? n : 1));
    for (long long i = 0; i < n; i++) p[i].re = p[i].im = (double)(i % 7);
    return p;
}

static void run_c2c(int n, int batch)
{
    for (int sgn = -1; sgn <= 1; sgn += 2) {
        fft_object o = fft_init(n, sgn);
        fft_data *x = cbuf((long long)n * batch), *y = cbuf((long long)n * batch);
        fft_exec(o, x, y);
        CHECK(hsfft_exec_batched(o, x, y, batch) == 0, "exec_batched N=%d: %s", n, hsfft_last_error());
        CHECK(hsfft_exec_batched_host(o, x, y, batch) == 0, "host N=%d", n);
        free(x);
        free(y);
        free_fft(o);
    }
}

static void *other_sync(void *rc)
{
    *(int *)rc = hsfft_synchronize();
    return NULL;
}

static void run_real(int n, int batch)
{
    fft_real_object f = fft_real_init(n, 1), iv = fft_real_init(n, -1);
    double *x = malloc(sizeof(double) * (size_t)n * batch);
    for (long long i = 0; i < (long long)n * batch; i++) x[i] = (double)(i % 5);
    fft_data *X = cbuf((long long)n * batch);
    fft_r2c_exec(f, x, X);
    fft_c2r_exec(iv, X, x);
    CHECK(hsfft_r2c_batched(f, x, X, batch) == 0, "r2c N=%d", n);
    CHECK(hsfft_r2c_batched_compact(f, x, X, batch) == 0, "r2c compact N=%d", n);
    CHECK(hsfft_c2r_batched(iv, X, x, batch) == 0, "c2r N=%d", n);
    free(x);
    free(X);
    free_real_fft(f);
    free_real_fft(iv);
}

static void run_conv(int n, int m)
{
    static const char *types[] = {"full", "same", "valid"}, *ctypes[] = {"linear", "circular"};
    double *a = calloc((size_t)n, sizeof(double)), *b = calloc((size_t)m, sizeof(double));
    double *o = calloc(4 * (size_t)(n + m) + 8, sizeof(double));
    for (int t = 0; t < 3; t++)
        for (int c = 0; c < 2; c++) {
            const int len = fft_convolve(types[t], ctypes[c], a, n, b, m, o);
            CHECK(len > 0, "convolve %s %s %d %d", types[t], ctypes[c], n, m);
        }
    const int rows = 3;
    double *ba = calloc((size_t)n * rows, sizeof(double)), *bb = calloc((size_t)m * rows, sizeof(double));
    double *bo = calloc((size_t)(n + m) * rows + 8, sizeof(double));
    CHECK(hsfft_convolve_batched("same", "linear", ba, n, bb, m, bo, rows) > 0, "convolve_batched %d %d", n, m);
    free(a);
    free(b);
    free(o);
    free(ba);
    free(bb);
    free(bo);
}

static fft_object g_shared;

/* 4. two callers running hsfft_exec_multi on one shared plan at once */
static fft_object g_multi;
static void *multi_caller(void *arg)
{
    const int ndev = hsfft_device_count(), n = 12600, rows = 5 + (int)(long)arg;
    const fft_data *ins[16];
    fft_data *outs[16];
    for (int g = 0; g < ndev; g++) {
        ins[g] = cbuf((long long)n * rows);
        outs[g] = cbuf((long long)n * rows);
    }
    for (int it = 0; it < 4; it++) CHECK(hsfft_exec_multi(g_multi, ins, outs, rows, ndev) == 0, "concurrent exec_multi");
    for (int g = 0; g < ndev; g++) {
        free((void *)ins[g]);
        free(outs[g]);
    }
    return NULL;
}

/* 5. the concurrent small fft_exec path (host buffers, outside the device lock) on a plan
 * that another thread refreshes: the refresh rebuilds the device state while a small call may
 * still be using the old one (it must be retired, not freed, until that call is
 * done); every thread's per-thread slots and stream are parked when it exits and adopted by
 * the next thread */
extern void null_mark_host(const void *p, int on);
static fft_object g_small;

static void *small_caller(void *arg)
{
    const int refresher = (int)(long)arg == 1, calls = (int)(long)arg >= 2 ? (int)(long)arg - 1 : 300;
    fft_data *x = cbuf(1024), *y = cbuf(1024);
    null_mark_host(x, 1);
    null_mark_host(y, 1);
    for (int it = 0; it < calls; it++) {
        if (refresher) CHECK(hsfft_plan_refresh(g_small) == 0, "refresh while small calls run");
        fft_exec(g_small, x, y);
    }
    null_mark_host(x, 0);
    null_mark_host(y, 0);
    free(x);
    free(y);
    return NULL;
}

static void *hammer(void *arg)
{
    const int t = (int)(long)arg;
    fft_data *x = cbuf(12600), *y = cbuf(12600);
    for (int it = 0; it < 40; it++) {
        fft_exec(g_shared, x, y);
        const int n = 8 + 37 * ((t * 40 + it) % 23);
        fft_object o = fft_init(n, it & 1 ? 1 : -1);
        fft_data *a = cbuf(n), *b = cbuf(n);
        fft_exec(o, a, b);
        free(a);
        free(b);
        free_fft(o);
        const int k = 5 + (t + it) % 10; /* ten padded lengths: more than the 8 cached pairs */
        const int len = (1 << k) / 2;
        double *ca = calloc((size_t)len, sizeof(double)), *cb = calloc((size_t)len, sizeof(double));
        double *co = calloc(2 * (size_t)len + 8, sizeof(double));
        CHECK(fft_convolve("full", "linear", ca, len, cb, len, co) == 2 * len - 1, "thread conv");
        free(ca);
        free(cb);
        free(co);
    }
    free(x);
    free(y);
    return NULL;
}

/* the small path's per-call snapshot of the HSFFT_* knobs (hs_getenv, round 6): inside a
 * snapshot scope every lookup equals getenv, after any setenv / unsetenv between scopes too */
#include "hsfft_internal.h"
static void check_env_snapshot(void)
{
    setenv("HSFFT_ZZ_A", "1", 1);
    unsetenv("HSFFT_ZZ_B");
    hs_env_begin();
    CHECK(hs_getenv("HSFFT_ZZ_A") && !strcmp(hs_getenv("HSFFT_ZZ_A"), "1"), "snapshot: set value");
    CHECK(hs_getenv("HSFFT_ZZ_B") == NULL && hs_getenv("HSFFT_ZZ") == NULL, "snapshot: absent / prefix");
    CHECK(hs_getenv("PATH") == NULL, "snapshot: only HSFFT_ knobs");
    hs_env_end();
    CHECK(hs_getenv("PATH") == getenv("PATH"), "outside a snapshot: getenv");
    for (int it = 0; it < 200; it++) {
        char v[16];
        snprintf(v, sizeof v, "%d", it % 3); /* values repeat: glibc may reuse a string */
        setenv("HSFFT_ZZ_A", v, 1);
        if (it % 5 == 0) setenv("HSFFT_ZZ_B", v, 1);
        if (it % 7 == 0) unsetenv("HSFFT_ZZ_B");
        hs_env_begin();
        const char *a = hs_getenv("HSFFT_ZZ_A"), *b = hs_getenv("HSFFT_ZZ_B"), *gb = getenv("HSFFT_ZZ_B");
        CHECK(a && !strcmp(a, v), "snapshot after setenv, round %d", it);
        CHECK((b == NULL) == (gb == NULL) && (!b || !strcmp(b, gb)), "snapshot after unsetenv, round %d", it);
        hs_env_end();
    }
    unsetenv("HSFFT_ZZ_A");
    unsetenv("HSFFT_ZZ_B");
}

int main(void)
{
    check_env_snapshot();
    for (int n = 1; n <= PLAN_MAX; n++) {
        check_plan(n, 1);
        if (n % 7 == 0) check_plan(n, -1);
    }
    const int big[] = {12600, 65536, 99991, 1 << 20, 65537, 169, 2 * 3 * 5 * 7 * 11 * 13};
    for (unsigned i = 0; i < sizeof big / sizeof big[0]; i++) check_plan(big[i], 1);

    const int sizes[] = {1, 2, 3, 7, 8, 12, 13, 16, 19, 97, 128, 1000, 1021, 1024, 4096, 12600, 65536, 1 << 18,
                         1 << 20, 99991, 257, 1025, 53 * 8};
    for (unsigned i = 0; i < sizeof sizes / sizeof sizes[0]; i++) run_c2c(sizes[i], sizes[i] > (1 << 17) ? 1 : 3);
    const int rsizes[] = {2, 8, 64, 1000, 8192, 1 << 16, 1 << 22, 2 * 99991, 12600};
    for (unsigned i = 0; i < sizeof rsizes / sizeof rsizes[0]; i++) run_real(rsizes[i], rsizes[i] > (1 << 20) ? 1 : 2);
    run_real(1 << 22, 3);
    run_conv(5, 3);
    run_conv(300, 17);
    run_conv(1000, 1000);
    run_conv(1 << 16, 1000);

    /* the persistent Bluestein launch times out (its workgroups were not all resident):
     * synchronous entry points (fft_exec, hsfft_exec_batched_host) re-run the rows on the
     * three-launch path and count the fallback; the asynchronous hsfft_exec_batched leaves the
     * error pending for ITS thread's next hsfft_synchronize(), which reports it exactly once --
     * a later call on another plan that grows the scratch pool and builds device state does not
     * consume it, and another thread's hsfft_synchronize() does not inherit it */
    {
        extern int null_bx_timeout;
        const long long fb0 = hsfft_bluestein_fallbacks();
        null_bx_timeout = 1;
        run_c2c(99991, 3);
        null_bx_timeout = 0;
        /* run_c2c: 2 signs x (fft_exec, hsfft_exec_batched_host) synchronous */
        const long long fb1 = hsfft_bluestein_fallbacks();
        CHECK(fb1 == fb0 + 4, "bluestein fallback count %lld", fb1 - fb0);
        {
            fft_object big = fft_init(1 << 20, 1), small = fft_init(1024, -1);
            fft_data *x = cbuf(3LL << 20), *y = cbuf(3LL << 20);
            CHECK(hsfft_release_scratch() == 0, "release_scratch keeps the pending error");
            CHECK(hsfft_exec_batched(big, x, y, 3) == 0, "another plan's call succeeds: %s", hsfft_last_error());
            fft_exec(small, x, y);
            pthread_t ot;
            int other_rc = 1;
            pthread_create(&ot, NULL, other_sync, &other_rc);
            pthread_join(ot, NULL);
            CHECK(other_rc == 0, "another thread's hsfft_synchronize() does not inherit the error");
            CHECK(hsfft_synchronize() == HSFFT_ERR_DEVICE, "the pending launch error is reported");
            CHECK(hsfft_synchronize() == 0, "the launch error is reported once");
            free(x);
            free(y);
            free_fft(big);
            free_fft(small);
        }
        run_c2c(99991, 2);
        CHECK(hsfft_bluestein_fallbacks() == fb1, "no fallback without a timeout");
        CHECK(hsfft_synchronize() == 0, "no error without a timeout");
        null_bx_timeout = 2; /* the grid refused as not co-resident: same three-launch path */
        run_c2c(99991, 3);
        null_bx_timeout = 0;
        CHECK(hsfft_bluestein_fallbacks() == fb1 + 6, "bluestein refusal count %lld", hsfft_bluestein_fallbacks() - fb1);
    }

    /* a caller edits the public fields between calls: the registry rebuilds its entry */
    fft_object e = fft_init(64, 1);
    fft_data *x = cbuf(64), *y = cbuf(64);
    fft_exec(e, x, y);
    e->sgn = -1;
    for (int i = 0; i < 63; i++) e->twiddle[i].im = -e->twiddle[i].im;
    fft_exec(e, x, y);
    CHECK(hsfft_plan_refresh(e) == 0, "refresh");
    fft_exec(e, x, y);
    free_fft(e);
    free(x);
    free(y);
    CHECK(hsfft_release_scratch() == 0, "release_scratch");

    /* 4. hsfft_exec_multi over every null device (rows split unevenly: 7 over 4 devices) */
    {
        const int ndev = hsfft_device_count();
        CHECK(ndev == 4, "null devices: %d (the test sets HSFFT_NULL_NDEV=4)", ndev);
        const int msz[] = {1024, 12600, 99991, 1 << 18};
        for (unsigned i = 0; i < sizeof msz / sizeof msz[0]; i++) {
            const int n = msz[i], rows = 7;
            fft_object o = fft_init(n, i & 1 ? -1 : 1);
            const fft_data *ins[16];
            fft_data *outs[16];
            for (int g = 0; g < ndev; g++) {
                const int r = rows * (g + 1) / ndev - rows * g / ndev;
                ins[g] = cbuf((size_t)n * (r > 0 ? r : 1));
                outs[g] = cbuf((size_t)n * (r > 0 ? r : 1));
            }
            CHECK(hsfft_exec_multi(o, ins, outs, rows, ndev) == 0, "exec_multi %d: %s", n, hsfft_last_error());
            CHECK(hsfft_exec_multi(o, ins, outs, 2, ndev) == 0, "exec_multi %d, 2 rows over %d devices", n, ndev);
            CHECK(hsfft_exec_multi(o, ins, outs, rows, ndev + 1) < 0, "exec_multi %d: more devices than exist", n);
            free_fft(o);
            for (int g = 0; g < ndev; g++) {
                free((void *)ins[g]);
                free(outs[g]);
            }
        }
        CHECK(hsfft_get_device() == 0, "exec_multi restores the caller's device");
        g_multi = fft_init(12600, -1);
        pthread_t mt[2];
        for (long t = 0; t < 2; t++) pthread_create(&mt[t], NULL, multi_caller, (void *)t);
        for (int t = 0; t < 2; t++) pthread_join(mt[t], NULL);
        free_fft(g_multi);
    }

    {
        /* 5a. a refresher and three small callers at once; at exit each parks its set */
        extern int null_parks, null_adopts, null_drained, null_host_allocs;
        g_small = fft_init(1024, 1);
        const int park0 = __atomic_load_n(&null_parks, __ATOMIC_RELAXED);
        pthread_t st[8];
        for (long t = 0; t < 4; t++) pthread_create(&st[t], NULL, small_caller, (void *)(t == 0 ? 1L : 0L));
        for (int t = 0; t < 4; t++) pthread_join(st[t], NULL);
        CHECK(__atomic_load_n(&null_parks, __ATOMIC_RELAXED) - park0 == 4, "sets parked at thread exit: %d of 4",
              __atomic_load_n(&null_parks, __ATOMIC_RELAXED) - park0);
        /* 5b. three generations of 8 threads: later threads adopt the parked sets, so no more
         * streams or page-locked blocks are created than threads were alive at once (VERDICT r5:
         * round 5 destroyed dead threads' objects on a new thread's path instead) */
        const long long str0 = hsfft_thread_streams_created();
        const int ad0 = __atomic_load_n(&null_adopts, __ATOMIC_RELAXED);
        int allocs_gen1 = 0;
        for (int gen = 0; gen < 3; gen++) {
            for (long t = 0; t < 8; t++) pthread_create(&st[t], NULL, small_caller, (void *)0L);
            for (int t = 0; t < 8; t++) pthread_join(st[t], NULL);
            if (gen == 0) allocs_gen1 = __atomic_load_n(&null_host_allocs, __ATOMIC_RELAXED);
        }
        /* 5b'. threads that make exactly ONE call, then threads that make two: a recycled
         * completion word continues its previous owner's sequence (a new owner restarting at 1
         * would find 1 already there and take it for its own kernel's completion) */
        for (int gen = 0; gen < 2; gen++) {
            for (long t = 0; t < 8; t++) pthread_create(&st[t], NULL, small_caller, (void *)(gen ? 3L : 2L));
            for (int t = 0; t < 8; t++) pthread_join(st[t], NULL);
        }
        const long long made = hsfft_thread_streams_created() - str0;
        CHECK(made <= 8 - 4 && made >= 0, "three generations of 8 threads created %lld streams (4 parked sets existed)", made);
        CHECK(__atomic_load_n(&null_adopts, __ATOMIC_RELAXED) - ad0 >= 16, "generations 2-3 adopt parked sets: %d",
              __atomic_load_n(&null_adopts, __ATOMIC_RELAXED) - ad0);
        CHECK(__atomic_load_n(&null_host_allocs, __ATOMIC_RELAXED) == allocs_gen1,
              "generations 2-3 allocate no page-locked memory: %d blocks",
              __atomic_load_n(&null_host_allocs, __ATOMIC_RELAXED) - allocs_gen1);
        free_fft(g_small);
        /* 5c. the pool is destroyed by hsfft_release_scratch (and hsfft_finalize), not before */
        const int dr0 = __atomic_load_n(&null_drained, __ATOMIC_RELAXED);
        CHECK(hsfft_release_scratch() == 0, "release_scratch drains the pool");
        const int dr = __atomic_load_n(&null_drained, __ATOMIC_RELAXED) - dr0;
        CHECK(dr >= 8, "parked sets destroyed by release_scratch: %d", dr);
    }

    { /* the C-loop drop-in timing (bench.py's c1): warm-up threads, then 4 timed threads */
        fft_object o = fft_init(1024, 1);
        fft_data *x = cbuf(1024), *y = cbuf(1024);
        double us[4] = {-1, -1, -1, -1};
        CHECK(hsfft_time_exec_host(o, x, y, 4, 20, 3, us) == 0, "time_exec_host: %s", hsfft_last_error());
        CHECK(us[0] >= 0 && us[1] <= us[0] && us[0] <= us[2] && us[3] > 0, "time_exec_host results");
        CHECK(hsfft_time_exec_host(o, x, y, 0, 20, 3, us) == HSFFT_ERR_ARG, "time_exec_host: 0 threads refused");
        free(x);
        free(y);
        free_fft(o);
    }

    g_shared = fft_init(12600, 1);
    pthread_t th[8];
    for (long t = 0; t < 8; t++) pthread_create(&th[t], NULL, hammer, (void *)t);
    for (int t = 0; t < 8; t++) pthread_join(th[t], NULL);
    free_fft(g_shared);
    CHECK(hsfft_release_scratch() == 0, "release_scratch 2");

    /* teardown: every device's objects released (each null device finalised once), the library
     * usable again afterwards */
    {
        extern int null_finalized;
        const int f0 = null_finalized;
        CHECK(hsfft_finalize() == 0, "finalize: %s", hsfft_last_error());
        CHECK(null_finalized - f0 == hsfft_device_count(), "finalize visits every device: %d", null_finalized - f0);
        run_c2c(12600, 2);
        run_real(1 << 16, 2);
        run_conv(300, 17);
        CHECK(hsfft_finalize() == 0, "finalize 2");
    }

    if (fails) {
        fprintf(stderr, "%d failures\n", fails);
        return 1;
    }
    printf("sanitize: ok\n");
    return 0;
}
