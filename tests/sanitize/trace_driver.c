/*
 * trace_driver.c -- TEST INFRASTRUCTURE ONLY (tests/test_sanitize_cpu.py).
 *
 * Runs a fixed list of calls into the host C of libhsfft.so against the null device with
 * HSFFT_NULL_TRACE set (null_device.c), single-threaded, on one null device.  The file the null
 * device writes -- one line per device-layer launch, copy and stream selection, no addresses --
 * is compared byte for byte with tests/golden/launch_trace.txt: the GPU suite proves outputs, this
 * pins the sequence of device-layer calls behind them (an extra trip through scratch, another
 * chunk size or another kernel choice changes the file).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "highspeedFFT.h"
#include "hsfft_gpu.h"
#include "real.h"

extern int null_bx_timeout;
void null_trace_note(const char *text);
void null_mark_host(const void *p, int on);

static void note(const char *fmt, int a, int b, int c)
{
    char buf[160];
    snprintf(buf, sizeof buf, fmt, a, b, c);
    null_trace_note(buf);
}

static void knob(const char *name, const char *value)
{
    char buf[160];
    snprintf(buf, sizeof buf, "knob %s=%s", name, value ? value : "(unset)");
    null_trace_note(buf);
    if (value) setenv(name, value, 1);
    else unsetenv(name);
}

/* zeroed "device" rows (never touched beyond the first and last element of a row) */
static void *rows(size_t elem, long long n) { return calloc((size_t)(n > 0 ? n : 1), elem); }

static void c2c_batched(int n, int batch)
{
    fft_object o = fft_init(n, 1);
    fft_data *x = rows(sizeof *x, (long long)n * batch), *y = rows(sizeof *y, (long long)n * batch);
    note("hsfft_exec_batched N=%d batch=%d", n, batch, 0);
    const int rc = hsfft_exec_batched(o, x, y, batch);
    note("rc=%d synchronize=%d", rc, hsfft_synchronize(), 0);
    free(x);
    free(y);
    free_fft(o);
}

static void c2c_host(int n, int batch)
{
    fft_object o = fft_init(n, 1);
    fft_data *x = rows(sizeof *x, (long long)n * batch), *y = rows(sizeof *y, (long long)n * batch);
    note("hsfft_exec_batched_host N=%d batch=%d", n, batch, 0);
    note("rc=%d", hsfft_exec_batched_host(o, x, y, batch), 0, 0);
    free(x);
    free(y);
    free_fft(o);
}

static void real_batched(int n, int batch)
{
    fft_real_object f = fft_real_init(n, 1), iv = fft_real_init(n, -1);
    double *x = rows(sizeof *x, (long long)n * batch);
    fft_data *X = rows(sizeof *X, (long long)n * batch);
    note("hsfft_r2c_batched N=%d batch=%d", n, batch, 0);
    note("rc=%d", hsfft_r2c_batched(f, x, X, batch), 0, 0);
    note("hsfft_r2c_batched_compact N=%d batch=%d", n, batch, 0);
    note("rc=%d", hsfft_r2c_batched_compact(f, x, X, batch), 0, 0);
    note("hsfft_c2r_batched N=%d batch=%d", n, batch, 0);
    const int rc = hsfft_c2r_batched(iv, X, x, batch);
    note("rc=%d synchronize=%d", rc, hsfft_synchronize(), 0);
    free(x);
    free(X);
    free_real_fft(f);
    free_real_fft(iv);
}

/* the drop-in entry points; host_in / host_out: which caller buffers are host memory */
static void dropin_c2c(int n, int host_in, int host_out, int alias)
{
    fft_object o = fft_init(n, 1);
    fft_data *x = rows(sizeof *x, n), *y = alias ? x : rows(sizeof *y, n);
    if (host_in) null_mark_host(x, 1);
    if (host_out && !alias) null_mark_host(y, 1);
    note(alias ? "fft_exec N=%d host=%d aliased" : "fft_exec N=%d host_in=%d host_out=%d", n, host_in, host_out);
    fft_exec(o, x, y);
    null_mark_host(x, 0);
    if (!alias) null_mark_host(y, 0);
    free(x);
    if (!alias) free(y);
    free_fft(o);
}

static void dropin_real(int n, int host_in, int host_out)
{
    fft_real_object f = fft_real_init(n, 1), iv = fft_real_init(n, -1);
    double *x = rows(sizeof *x, n);
    fft_data *X = rows(sizeof *X, n);
    if (host_in) null_mark_host(x, 1);
    if (host_out) null_mark_host(X, 1);
    note("fft_r2c_exec N=%d host_in=%d host_out=%d", n, host_in, host_out);
    fft_r2c_exec(f, x, X);
    null_mark_host(x, 0);
    null_mark_host(X, 0);
    if (host_in) null_mark_host(X, 1);
    if (host_out) null_mark_host(x, 1);
    note("fft_c2r_exec N=%d host_in=%d host_out=%d", n, host_in, host_out);
    fft_c2r_exec(iv, X, x);
    null_mark_host(x, 0);
    null_mark_host(X, 0);
    free(x);
    free(X);
    free_real_fft(f);
    free_real_fft(iv);
}

int main(void)
{
    if (!getenv("HSFFT_NULL_TRACE")) {
        fprintf(stderr, "trace_driver: set HSFFT_NULL_TRACE to the file to write\n");
        return 2;
    }
    static const int sizes[] = {8, 1024, 1 << 16, 1 << 20, 1 << 22, 12600, 100000};
    for (unsigned i = 0; i < sizeof sizes / sizeof sizes[0]; i++) c2c_batched(sizes[i], 5);
    knob("HSFFT_CHUNK_MB", "1");
    c2c_batched(1024, 5);
    c2c_batched(1 << 16, 2);
    c2c_batched(1 << 22, 2); /* a three-pass chain in chunks of one row */
    knob("HSFFT_CHUNK_MB", NULL);

    c2c_batched(97, 3);
    c2c_batched(99991, 3);
    knob("HSFFT_BLUE_XCD", "0");
    c2c_batched(99991, 3);
    knob("HSFFT_BLUE_XCD", NULL);
    knob("HSFFT_BLUE_NOFUSE", "1");
    c2c_batched(99991, 3);
    knob("HSFFT_BLUE_NOFUSE", NULL);
    for (null_bx_timeout = 1; null_bx_timeout <= 2; null_bx_timeout++) {
        note("null_bx_timeout=%d", null_bx_timeout, 0, 0);
        c2c_batched(99991, 3);
    }
    null_bx_timeout = 0;
    note("null_bx_timeout=%d", 0, 0, 0);

    real_batched(4096, 3);
    real_batched(1 << 20, 3);
    knob("HSFFT_R2C_FUSE", "0");
    real_batched(4096, 3);
    real_batched(1 << 20, 3);
    knob("HSFFT_R2C_FUSE", NULL);

    {
        const int n = 1000, m = 300, batch = 2;
        double *a = rows(sizeof *a, n * batch), *b = rows(sizeof *b, m * batch), *o = rows(sizeof *o, (n + m) * batch);
        note("hsfft_convolve_batched full linear %d %d batch=%d", n, m, batch);
        note("rc=%d", hsfft_convolve_batched("full", "linear", a, n, b, m, o, batch), 0, 0);
        note("fft_convolve full linear %d %d", n, m, 0);
        note("rc=%d", fft_convolve("full", "linear", a, n, b, m, o), 0, 0);
        free(a);
        free(b);
        free(o);
    }

    knob("HSFFT_HOST_CHUNK_MB", "1");
    c2c_host(4096, 7);
    c2c_host(4096, 40); /* three chunks: both staging slots are reused */
    knob("HSFFT_HOST_CHUNK_MB", NULL);

    knob("HSFFT_SMALL_CONCURRENT", "1");
    dropin_c2c(1024, 1, 1, 0);
    knob("HSFFT_SMALL_CONCURRENT", "0");
    dropin_c2c(1024, 1, 1, 0);
    knob("HSFFT_SMALL_CONCURRENT", NULL);
    dropin_c2c(1 << 16, 1, 1, 0);
    dropin_real(4096, 1, 1);

    /* the other pointer combinations of the drop-in entry points' staging rule */
    dropin_c2c(1 << 16, 0, 0, 0);
    dropin_c2c(1 << 16, 0, 1, 0);
    dropin_c2c(1 << 16, 1, 0, 0);
    dropin_c2c(1 << 16, 0, 0, 1);
    dropin_c2c(1 << 16, 1, 1, 1);
    dropin_c2c(1024, 0, 0, 1);
    dropin_real(4096, 0, 0);
    dropin_real(4096, 0, 1);
    dropin_real(4096, 1, 0);

    note("hsfft_finalize=%d", hsfft_finalize(), 0, 0);
    printf("trace: ok\n");
    return 0;
}
