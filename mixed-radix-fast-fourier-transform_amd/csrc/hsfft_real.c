/*
 * hsfft_real.c -- real-signal transforms of libhsfft.so (host C; compute on the GPU).
 *   fft_real_init  ref src/real.c:26-64    (inner N/2 complex plan + twiddle2)
 *   fft_r2c_exec   ref src/real.c:78-136   (pack = reinterpretation, c2c, split, mirror)
 *   fft_c2r_exec   ref src/real.c:150-193  (pre-twiddle, c2c, unpack = reinterpretation)
 *   free_real_fft  ref src/real.c:259-267  (also releases device state of both objects)
 */
#define _GNU_SOURCE
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hsfft_gpu.h"
#include "hsfft_host.h"

typedef struct hs_real_entry {
    const struct fft_real_set *key;
    void *d_tw2[HS_MAX_DEV];
    struct hs_real_entry *next;
} hs_real_entry;

static pthread_mutex_t g_rlock = PTHREAD_MUTEX_INITIALIZER;
static hs_real_entry *g_real;

fft_real_object fft_real_init(int N, int sgn)
{
    if (N <= 0 || N % 2 != 0) {
        fprintf(stderr, "Error: Signal length (%d) must be positive and even\n", N);
        exit(EXIT_FAILURE);
    }
    const int h = N / 2;
    fft_real_object r = (fft_real_object)malloc(sizeof(struct fft_real_set) + sizeof(fft_data) * (size_t)h);
    if (r == NULL) {
        fprintf(stderr, "Error: Memory allocation failed for real FFT object\n");
        exit(EXIT_FAILURE);
    }
    r->cobj = fft_init(h, sgn);
    if (r->cobj == NULL) {
        free(r);
        fprintf(stderr, "Error: Failed to initialize complex FFT object\n");
        exit(EXIT_FAILURE);
    }
    for (int k = 0; k < h; k++) {
        double sn, cs;
        sincos(PI2 * k / N, &sn, &cs);
        r->twiddle2[k].re = cs;
        r->twiddle2[k].im = sn;
    }
    return r;
}

void *hs_real_tw2_device(fft_real_object r)
{
    const int d = hsd_get_device();
    if (d < 0 || d >= HS_MAX_DEV) return NULL;
    pthread_mutex_lock(&g_rlock);
    hs_real_entry *e = g_real;
    while (e && e->key != r) e = e->next;
    if (!e) {
        e = calloc(1, sizeof *e);
        e->key = r;
        e->next = g_real;
        g_real = e;
    }
    if (!e->d_tw2[d]) {
        const size_t b = sizeof(fft_data) * (size_t)r->cobj->N;
        e->d_tw2[d] = hsd_malloc(b);
        if (e->d_tw2[d] && hsd_h2d(e->d_tw2[d], r->twiddle2, b)) {
            hsd_free(e->d_tw2[d]);
            e->d_tw2[d] = NULL;
        }
    }
    void *p = e->d_tw2[d];
    pthread_mutex_unlock(&g_rlock);
    return p;
}

void free_real_fft(fft_real_object r)
{
    if (r == NULL) return;
    pthread_mutex_lock(&g_rlock);
    for (hs_real_entry **pp = &g_real; *pp; pp = &(*pp)->next)
        if ((*pp)->key == r) {
            hs_real_entry *e = *pp;
            *pp = e->next;
            const int cur = hsd_get_device();
            for (int d = 0; d < HS_MAX_DEV; d++)
                if (e->d_tw2[d]) {
                    hsd_set_device(d);
                    hsd_free(e->d_tw2[d]);
                }
            if (cur >= 0) hsd_set_device(cur);
            free(e);
            break;
        }
    pthread_mutex_unlock(&g_rlock);
    free_fft(r->cobj);
    free(r);
}

/* (hsfft_finalize) drop every real plan's device twiddles on device `dev` (rebuilt on demand) */
void hs_real_release_device(int dev)
{
    pthread_mutex_lock(&g_rlock);
    for (hs_real_entry *e = g_real; e; e = e->next)
        if (e->d_tw2[dev]) {
            hsd_free(e->d_tw2[dev]);
            e->d_tw2[dev] = NULL;
        }
    pthread_mutex_unlock(&g_rlock);
}

/* row chunk for the inner c2c's intermediate Z (HS_SCR_REAL_Z): HSFFT_REAL_CHUNK_MB of Z per
 * chunk, default 16 GiB (measured, 4096 x 2^22 r2c, fused split: 2 GiB 91.7, 4 GiB 94.1,
 * 8 GiB 98.3, 16 GiB 99.9 GSamples/s -- longer launches fill the chip better); halved while
 * the allocation fails, so a device with less free HBM still runs, in smaller chunks */
static fft_data *real_chunk(int h, int batch, long long *chunk)
{
    const size_t bytes = hs_env_mb("HSFFT_REAL_CHUNK_MB", 16384.0);
    long long rows = (long long)(bytes / (sizeof(fft_data) * (size_t)h));
    if (rows < 1) rows = 1;
    if (rows > batch) rows = batch;
    for (;;) {
        fft_data *Z = hs_scratch(HS_SCR_REAL_Z, sizeof(fft_data) * (size_t)(rows * h));
        if (Z || rows == 1) {
            *chunk = rows;
            if (!Z) hs_seterr("scratch allocation of %lld bytes failed", (long long)(rows * h * 16));
            return Z;
        }
        rows = (rows + 1) / 2;
    }
}

/* (device lock held) r2c of `batch` rows.  compact 0: the reference's mirrored rows of N bins;
 * 1: bins 0..N/2 per row (rows of N/2+1 complex), the non-redundant half
 * -- 16 B written per real sample instead of 24 for the same values (bit-identical to bins
 * 0..N/2 of the mirrored rows) */
int hs_r2c_rows(fft_real_object r, const fft_type *d_in, fft_data *d_out, int batch, int compact)
{
    hs_entry *e = hs_entry_get(r->cobj);
    void *tw2 = e ? hs_real_tw2_device(r) : NULL;
    const int h = r->cobj->N, N = 2 * h;
    const long long xdist = compact ? h + 1 : N;
    long long chunk = 1;
    fft_data *Z = tw2 ? real_chunk(h, batch, &chunk) : NULL;
    int rc = !tw2 ? HSFFT_ERR_DEVICE : !Z ? HSFFT_ERR_NOMEM : 0;
    for (long long c0 = 0; c0 < batch && !rc; c0 += chunk) {
        const int cb = (int)(batch - c0 < chunk ? batch - c0 : chunk);
        fft_data *X = d_out + c0 * xdist;
        /* x[2k], x[2k+1] packed as complex = the same bytes (ref real.c:99-103) */
        rc = hs_r2c_fused(e, d_in + c0 * N, h, Z, X, xdist, tw2, cb, compact);
        if (rc == 1) {
            rc = hs_c2c_rows(e, d_in + c0 * N, h, Z, h, cb);
            if (!rc) rc = (compact ? hsd_r2c_post_compact : hsd_r2c_post)(Z, tw2, X, h, cb, h, xdist) ? HSFFT_ERR_DEVICE : 0;
        }
    }
    hs_entry_put(e);
    return rc;
}

/* (callers hold the device lock) c2r of rows xdist complex apart (the reference layout: N;
 * compact spectra: N/2+1 -- the pre-twiddle reads bins 0..N/2 only, ref real.c:169-179); with
 * d_b, of the product d_a .* d_b, multiplied inside the pre-twiddle */
int hs_c2r_rows(fft_real_object r, const fft_data *d_a, const fft_data *d_b, long long xdist, fft_type *d_out,
                int batch)
{
    hs_entry *e = hs_entry_get(r->cobj);
    void *tw2 = e ? hs_real_tw2_device(r) : NULL;
    const int h = r->cobj->N, N = 2 * h;
    long long chunk = 1;
    fft_data *Zi = tw2 ? real_chunk(h, batch, &chunk) : NULL;
    int rc = !tw2 ? HSFFT_ERR_DEVICE : !Zi ? HSFFT_ERR_NOMEM : 0;
    for (long long c0 = 0; c0 < batch && !rc; c0 += chunk) {
        const int cb = (int)(batch - c0 < chunk ? batch - c0 : chunk);
        rc = d_b ? hsd_c2r_pre_mul(d_a + c0 * xdist, d_b + c0 * xdist, tw2, Zi, h, cb, xdist, h)
                 : hsd_c2r_pre(d_a + c0 * xdist, tw2, Zi, h, cb, xdist, h);
        if (rc) rc = HSFFT_ERR_DEVICE;
        /* unpacking complex_output into interleaved reals is again a reinterpretation */
        if (!rc) rc = hs_c2c_rows(e, Zi, h, d_out + c0 * N, h, cb);
    }
    hs_entry_put(e);
    return rc;
}

/* argument and GPU check of the batched entry points, then the device lock: 0 with the device
 * locked (*dev), 1 for an empty batch (nothing to do, not locked), < 0 on error */
static int real_enter(const char *who, fft_real_object r, const void *d_in, const void *d_out, int batch, int *dev)
{
    if (!r || !r->cobj || !d_in || !d_out || batch < 0) {
        hs_seterr("%s: invalid arguments", who);
        return HSFFT_ERR_ARG;
    }
    if (batch == 0) return 1;
    const int rc = hs_require_gpu();
    if (rc) return rc;
    *dev = hs_lock_device();
    return 0;
}

int hsfft_r2c_batched(fft_real_object r, const fft_type *d_in, fft_data *d_out, int batch)
{
    int d, rc = real_enter("hsfft_r2c_batched", r, d_in, d_out, batch, &d);
    if (rc) return rc < 0 ? rc : 0;
    rc = hs_r2c_rows(r, d_in, d_out, batch, 0);
    hs_unlock_device(d);
    return rc;
}

int hsfft_r2c_batched_compact(fft_real_object r, const fft_type *d_in, fft_data *d_out, int batch)
{
    int d, rc = real_enter("hsfft_r2c_batched_compact", r, d_in, d_out, batch, &d);
    if (rc) return rc < 0 ? rc : 0;
    rc = hs_r2c_rows(r, d_in, d_out, batch, 1);
    hs_unlock_device(d);
    return rc;
}

int hsfft_c2r_batched(fft_real_object r, const fft_data *d_in, fft_type *d_out, int batch)
{
    int d, rc = real_enter("hsfft_c2r_batched", r, d_in, d_out, batch, &d);
    if (rc) return rc < 0 ? rc : 0;
    rc = hs_c2r_rows(r, d_in, NULL, 2LL * r->cobj->N, d_out, batch);
    hs_unlock_device(d);
    return rc;
}

int hsfft_time_r2c_batched(fft_real_object r, const fft_type *d_in, fft_data *d_out, int batch, int iters, float *ms)
{
    if (!r || iters < 1 || !ms) return HSFFT_ERR_ARG;
    int rc = hs_require_gpu();
    if (rc) return rc;
    const int d = hs_lock_device();
    rc = hsfft_r2c_batched(r, d_in, d_out, batch); /* device state outside the timing */
    if (!rc && hsd_timer_start()) rc = HSFFT_ERR_DEVICE;
    for (int i = 0; i < iters && !rc; i++) rc = hsfft_r2c_batched(r, d_in, d_out, batch);
    if (!rc && hsd_timer_stop(ms)) rc = HSFFT_ERR_DEVICE;
    hs_unlock_device(d);
    return rc;
}

static void real_fail(const char *who, const char *what)
{
    fprintf(stderr, "Error: %s%s (%s)\n", who, what, hsfft_last_error());
    exit(EXIT_FAILURE);
}

/* The drop-in pair: one row through the batched entry point, on the caller's buffers when both
 * are device pointers, else staged (hs_stage_in); synchronous.  c2r reads bins 0..N/2 only
 * (real.c:169-179), so h+1 bins are uploaded into a staging row N bins long. */
static void real_exec_locked(fft_real_object r, int inverse, void *inp, void *oup)
{
    const char *who = inverse ? "fft_c2r_exec" : "fft_r2c_exec";
    if (r == NULL || inp == NULL || oup == NULL) {
        fprintf(stderr, "Error: Invalid real FFT object or data pointers\n");
        exit(EXIT_FAILURE);
    }
    if (hs_require_gpu()) real_fail(who, " needs an MI355X");
    const int h = r->cobj->N, N = 2 * h;
    const size_t rbytes = sizeof(double) * (size_t)N, cbytes = sizeof(fft_data) * (size_t)N;
    const size_t in_bytes = inverse ? cbytes : rbytes, out_bytes = inverse ? rbytes : cbytes;
    const int din = hsd_is_device_ptr(inp), dout = hsd_is_device_ptr(oup);
    void *di = inp, *dq = oup;
    int rc = 0;
    if (!(din && dout)) {
        rc = hs_stage_in(inp, din, inverse ? sizeof(fft_data) * (size_t)(h + 1) : rbytes, in_bytes, out_bytes, &di, &dq);
        if (rc == 1) real_fail(who, ": staging allocation failed");
    }
    if (!rc) rc = inverse ? hsfft_c2r_batched(r, di, dq, 1) : hsfft_r2c_batched(r, di, dq, 1);
    if (!rc && dq != oup) rc = hs_stage_out(oup, dout, dq, out_bytes);
    if (!rc) rc = hsd_sync();
    if (rc) real_fail(who, " failed");
}

static void real_exec(fft_real_object r, int inverse, void *inp, void *oup)
{
    const int d = hs_lock_device();
    hs_sync_call(1); /* synchronous: a Bluestein inner plan re-runs timed-out rows itself */
    real_exec_locked(r, inverse, inp, oup);
    hs_sync_call(0);
    hs_unlock_device(d);
}

void fft_r2c_exec(fft_real_object r, fft_type *inp, fft_data *oup) { real_exec(r, 0, inp, oup); }
void fft_c2r_exec(fft_real_object r, fft_data *inp, fft_type *oup) { real_exec(r, 1, inp, oup); }
