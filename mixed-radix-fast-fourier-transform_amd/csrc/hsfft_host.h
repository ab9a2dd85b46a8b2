/*
 * hsfft_host.h -- host-side internals shared by the C translation units of libhsfft.so.
 */
#ifndef HSFFT_HOST_H_
#define HSFFT_HOST_H_

#include <stdlib.h>

#include "highspeedFFT.h"
#include "hsfft_internal.h"
#include "real.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-device state of one plan: device copies of what the plan needs */
typedef struct hs_devstate {
    void *d_tw;   /* M-1 (+1) complex twiddles, copied from the public struct; only the
                   * [3,3,5,5,7,8] whole-row schedule (N = 12600) also holds the last stage's block
                   * transposed at d_tw + M, and readers are told so by tw_t below */
    void *d_gcs;  /* odd-radix cos/sin constants */
    void *d_chirp;/* Bluestein chirp h(n), N complex */
    void *d_hk;   /* Bluestein spectrum of the scaled, mirrored chirp, M complex */
    int tw_t;     /* 1: d_tw + M holds the last stage's block transposed (the 12600 row kernel) */
    /* users outside the device lock (the concurrent small fft_exec path) pin the state for
     * their whole call: a rebuild (hsfft_plan_refresh) then retires it instead of freeing it,
     * and the last hs_devstate_put frees it.  Both fields change under the device lock. */
    int refs;
    int retired;
} hs_devstate;

/* schedule derived from the public plan fields (snapshot) */
typedef struct hs_entry {
    const struct fft_set *key;
    int N, sgn, lt, lf, M; /* M = length of the mixed-radix transform actually run */
    int factors[64];       /* snapshot of the public fields (edits trigger a rebuild) */
    int rlf, rfac[64];     /* factor list actually executed (differs only for D5) */
    int tw_from_struct;    /* 1: twiddles copied from the struct; 0: private table (D5) */
    fft_data *tw_private;  /* Bluestein plan/exec length mismatch (D5): own M_exec table */
    int nst;
    int stage_r[HS_MAX_STAGES];  /* innermost first */
    int first_leaf;
    int npass;
    hsd_pass pass[HS_MAX_PASSES];
    double *gcs;           /* host odd-radix constants */
    int ngcs;
    fft_data *chirp;       /* Bluestein chirp (host) */
    hs_devstate *ds[HS_MAX_DEV];
    int version;           /* bumped by hsfft_plan_refresh: device copies re-uploaded */
    int ds_version[HS_MAX_DEV];
    int refs;              /* users holding the entry (hs_entry_get .. hs_entry_put) */
    int dead;              /* unlinked (free_fft or a rebuild): freed by the last put */
    struct hs_entry *next;
} hs_entry;

/* planner (hsfft_plan.c) */
int hs_twiddle_mode(void);
void hs_longvector(fft_data *tw, int M, const int *fac, int lf, int exact);
int hs_bluestein_M_init(int N); /* fft_init sizing (log10), ref :242-252 */
int hs_bluestein_M_exec(int N); /* bluestein_fft sizing (log2), ref :1750-1751 */

/* a length the reference runs as one leaf butterfly (ref :332-713); every other radix uses
 * the odd-radix constants */
static inline int hs_is_leaf_radix(int r) { return r == 2 || r == 3 || r == 4 || r == 5 || r == 7 || r == 8; }
/* integer knob (hs_getenv: served from the small path's snapshot inside fft_exec) */
static inline int hs_env_int(const char *name, int dflt)
{
    const char *s = hs_getenv(name);
    return s ? atoi(s) : dflt;
}
/* pass schedule of e->M (hsfft_schedule.c): stages, passes with tiles and variants, odd-radix
 * constants; nonzero (hs_seterr set where there is something to say) if M cannot be scheduled */
int hs_build_schedule(hs_entry *e);
/* HSFFT_CRASH_TRACE=1 (hsfft_crash.c): install the crash-trace signal handlers */
void hs_crash_trace_install(void);

/* registry / execution (hsfft_exec.c).  hs_entry_get returns the entry with a
 * reference held; every successful get is paired with hs_entry_put. */
hs_entry *hs_entry_get(const struct fft_set *obj);
void hs_entry_put(hs_entry *e);
void hs_entry_release(const struct fft_set *obj);
/* Reentrancy: every public entry point that enqueues work or touches per-device state
 * (scratch pool, staging slots, streams, events, lazily built device state) runs under the
 * recursive lock of the calling thread's current device.  Host threads on different devices
 * run concurrently; threads sharing a device take turns per call. */
int hs_lock_device(void);
void hs_unlock_device(int dev);
int hs_require_gpu(void);
void hs_seterr(const char *fmt, ...);
int hs_c2c_rows(hs_entry *e, const void *in, long long idist, void *out, long long odist, int batch);
/* r2c with the split fused into the last c2c pass: returns 1 when the plan's schedule does
 * not allow it (caller falls back to c2c + split), 0 on success, < 0 on error */
int hs_r2c_fused(hs_entry *e, const void *in, long long idist, void *Z, void *X, long long xdist, const void *tw2,
                 int batch, int compact);
/* r2c of `batch` contiguous rows (hsfft_real.c; device lock held): compact 0 writes the
 * reference's mirrored rows of N bins, 1 rows of N/2+1 bins (bins 0..N/2, the same words) */
int hs_r2c_rows(fft_real_object r, const fft_type *d_in, fft_data *d_out, int batch, int compact);
/* c2r of rows xdist complex apart (hsfft_real.c); d_b != NULL: of the product d_a .* d_b */
int hs_c2r_rows(fft_real_object r, const fft_data *d_a, const fft_data *d_b, long long xdist, fft_type *d_out,
                int batch);
/* the device copy of r's twiddle2 table (N/2 complex) on the current device, uploaded on first use
 * and kept until free_real_fft / hsfft_finalize; NULL on failure (hsfft_real.c) */
void *hs_real_tw2_device(fft_real_object r);
/* Scratch buffers, one per class and device, grown on demand and used under the device lock.
 * Two names with one number share a buffer: their users are separate public entry points that
 * hold the device lock for their whole call, wait for the device before they return, and never
 * call each other, so the buffer is never live for both. */
enum {
    HS_SCR_CHAIN0 = 0,    /* intermediates of a pass chain, alternating */
    HS_SCR_CHAIN1 = 1,
    HS_SCR_FILTER = 2,    /* hsfft_filter_batched (hsfft_filter.h): a chunk's gathered blocks.  A class of
                           * its own, and its spectra in HS_SCR_CONV_SPEC, whose other user runs on the
                           * library stream too: the call is asynchronous, so it shares no buffer with
                           * an entry point that writes its scratch from another stream */
    HS_SCR_STFT = 2,      /* hsfft_stft_batched / hsfft_istft_batched (hsfft_stft.h): a chunk's windowed frames,
                           * or its frames after the c2r.  The filter's number under a second name although
                           * these calls are asynchronous too: all three run wholly on the library stream
                           * under the device lock and never call each other, so stream order keeps one
                           * call's kernels behind the previous call's, whichever of the three it was */
    HS_SCR_DCT = 2,       /* hsfft_dct_batched (hsfft_dct.h): a chunk's permuted rows, or its rows after the
                           * c2r.  A third name for the same number by the same argument: the call is
                           * asynchronous, runs wholly on the library stream under the device lock and
                           * calls neither the filter nor the STFT, so stream order separates the users */
    HS_SCR_CZT = 2,       /* hsfft_czt_batched / hsfft_czt_real_batched (hsfft_czt.h): a chunk's rotated, zero-filled
                           * rows, then its rows after the inverse transform.  A fourth name for the same
                           * number by the same argument: the call is asynchronous, runs wholly on the
                           * library stream under the device lock and calls neither the filter, the STFT
                           * nor a cosine or sine transform, so stream order separates the users */
    HS_SCR_SPECTRAL = 2,  /* hsfft_hilbert_batched / hsfft_resample_batched (hsfft_spectral.h): a chunk's compact
                           * spectra S.  A fifth name for the same number by the same argument: the calls
                           * are asynchronous, run wholly on the library stream under the device lock and
                           * call none of the other users, so stream order separates them; the row
                           * transforms in between use the chain, Bluestein and HS_SCR_REAL_Z classes */
    HS_SCR_BLUE_MID = 3,  /* Bluestein M-point intermediate, or the persistent launch's images */
    HS_SCR_REAL_Z = 4,    /* real transforms: the inner c2c's N/2-point rows */
    HS_SCR_STAGE_IN = 5,  /* drop-in fft_exec / fft_r2c_exec / fft_c2r_exec: staged input */
    HS_SCR_CONV_IN = 5,   /* drop-in fft_convolve: both uploaded signals (it runs the batched
                           * real transforms, never the drop-in ones) */
    HS_SCR_STAGE_OUT = 6, /* drop-in staged output */
    HS_SCR_HOST_IN = 7,   /* hsfft_exec_batched_host: two upload slots (it runs c2c rows only) */
    HS_SCR_CONV_PAD = 7,  /* convolution: both zero-padded signals (it runs real transforms only) */
    HS_SCR_BLUE_MID2 = 8, /* Bluestein second intermediate (fused middle kernel) */
    HS_SCR_HOST_OUT = 9,  /* hsfft_exec_batched_host: two download slots */
    HS_SCR_CONV_SPEC = 10,/* convolution: both compact spectra */
    HS_SCR_DCT_SPEC = 10, /* hsfft_dct_batched: a chunk's compact spectra, as the filter keeps its own in
                           * HS_SCR_CONV_SPEC; the convolution, the filter and this call all run on the
                           * library stream under the device lock and never call each other */
    HS_SCR_CZT_SPEC = 10, /* the chirp-z calls: a chunk's spectra, then their products with the chirp's, as
                           * hsfft_dct_batched keeps its spectra here: all users of the number run on the
                           * library stream under the device lock and never call each other */
    HS_SCR_SPECTRAL_SPEC = 10, /* the same two calls: a chunk's edited spectra, Z (rows of n words) or Y (rows
                           * of m/2+1), which the inverse transform reads; by the argument of
                           * HS_SCR_CZT_SPEC.  The class holds other calls' leftovers, so every word of
                           * Z and Y, the zero ones too, is written in every chunk */
    HS_SCR_2D = 11,       /* hsfft_exec_2d / hsfft_exec_columns / the 2D real transforms (hsfft_2d.h): the
                           * chunk between the row transforms and the transposes; a class of its own,
                           * because the row transforms in between use the chain, Bluestein and
                           * HS_SCR_REAL_Z classes.  hsfft_dct_2d_batched (hsfft_dct2d.h) keeps its chunk
                           * here too: the class is free there, because dct::run in between uses
                           * HS_SCR_DCT and HS_SCR_DCT_SPEC beside those and keeps its own inner chunk
                           * walk (HSFFT_DCT_CHUNK_MB) */
    HS_SCR_MDCT = 11,     /* hsfft_mdct_batched / hsfft_imdct_batched (hsfft_dct4.h): a chunk's folded frames,
                           * or its frames after the type-IV transform.  The 2D class under a second
                           * name by the argument of hsfft_dct_2d_batched: dct4::run in between uses
                           * HS_SCR_DCT and HS_SCR_DCT_SPEC beside the row kernels' classes and keeps its
                           * own inner chunk walk, and no 2D entry point is called from here */
    HS_NSCRATCH = 12
};
void *hs_scratch(int cls, size_t bytes);
/* Staging of the drop-in entry points (device lock held).  Caller buffers are used directly
 * only when BOTH are device pointers; otherwise both sides go through the staging slots.
 * hs_stage_in sizes both slots (*di, *dq) and copies copy_bytes of the caller's input into *di
 * -- d2d for a device pointer, h2d for a host one; returns 1 if a slot could not be allocated,
 * else the copy's result.  hs_stage_out copies the output slot to the caller's buffer. */
int hs_stage_in(const void *p, int on_device, size_t copy_bytes, size_t in_bytes, size_t out_bytes, void **di,
                void **dq);
int hs_stage_out(void *p, int on_device, const void *dq, size_t bytes);
/* brackets a synchronous entry point on this thread (1 enter, 0 leave): persistent Bluestein
 * launches inside it wait and re-run timed-out rows instead of reporting them later */
void hs_sync_call(int enter);
/* release this layer's device objects (hsfft_finalize): idle convolution plan pairs, real
 * plans' device twiddles on the current device */
void hs_conv_cache_release(void);
/* Cached plan pairs of the convolutions (hsfft_convolve.c), keyed by length and twiddle mode and
 * reference counted: the forward and inverse real plans of a padded length, and the forward and
 * inverse c2c plans of the 2D convolution's padded row count.  Every get is paired with its done;
 * slot < 0 marks a private pair (every slot busy) that done frees; f or i is NULL where a build
 * failed.  A repeated request for a cached length builds nothing. */
typedef struct {
    fft_real_object f, i;
    int slot;
} hs_conv_pair;
typedef struct {
    fft_object f, i;
    int slot;
} hs_conv_cpair;
hs_conv_pair hs_conv_plans(int P);
void hs_conv_plans_done(hs_conv_pair cp);
hs_conv_cpair hs_conv_cplans(int P);
void hs_conv_cplans_done(hs_conv_cpair cp);
/* one axis of the 2D convolution by the 1D rule: padded length, window start; returns the
 * window length or -1 (message set) */
int hs_conv_axis(const char *type, const char *conv_type, int n, int m, int *P, int *start);
void hs_real_release_device(int dev);
/* The cosine and sine transforms' rotation table (hsfft_dct.c), n/2+1 words (cos, sin)(pi k / 2n).
 * hs_dct_table (device lock of `dev` held, `dev` current): its copy on the device from a cache of
 * four lengths per device, the least recently used one replaced; a miss builds the table on the
 * host and uploads it synchronously; NULL with the message set on failure.  hs_dct_release_device
 * (the same lock held, the device's work waited for): frees the device's cached tables; they are
 * rebuilt on demand. */
#define HS_DCT_MAX_LEN (1 << 30)
const void *hs_dct_table(int dev, int n);
void hs_dct_release_device(int dev);
/* The type-IV transforms' rotation table (hsfft_dct4.c), n/2 words (cos, sin)(pi (8j+1) / 8n), with
 * a cache of its own under the same rules: four lengths per device, the least recently used one
 * replaced, freed by hs_dct4_release_device and rebuilt on demand. */
const void *hs_dct4_table(int dev, int n);
void hs_dct4_release_device(int dev);
/* The chirp-z transform's host side (hsfft_czt.c).  hs_czt_sizes and hs_czt_freqs: the argument
 * rules of hsfft_czt_shape and hsfft_czt_tables for the other entry points; 0, or HSFFT_ERR_ARG with
 * the message set.  hs_czt_get (device lock of `dev` held, `dev` current): the device data of one (n,
 * m, f0, df, twiddle mode) from a cache of four per device, the least recently used one replaced (it
 * is waited for before it is freed); a miss builds the two tables and the wrapped chirp v on the
 * host and uploads them synchronously, and leaves `ready` 0: the driver then transforms v into V
 * and calls hs_czt_set_ready.  0, or HSFFT_ERR_NOMEM with the message set.  hs_czt_release_device
 * (the same lock held, the device's work waited for): frees the device's entries. */
#define HS_CZT_MAX_SUM (1 << 26)
typedef struct {
    const fft_data *pre, *chirp, *v; /* n, max(n, m) and L words */
    fft_data *V;                     /* L words: the forward transform of v once `ready` */
    int slot, ready;
} hs_czt_data;
int hs_czt_sizes(const char *who, int n, int m, int *L);
int hs_czt_freqs(const char *who, double f0, double df);
int hs_czt_get(int dev, int n, int m, int L, double f0, double df, int mode, hs_czt_data *out);
void hs_czt_set_ready(int dev, int slot);
void hs_czt_release_device(int dev);
/* The analytic signal's and Fourier resampling's host side (hsfft_spectral.c); `hilbert` set means
 * there is no second length and m is 0.  hs_spectral_sizes: the length rule of both calls and of
 * hsfft_spectral_chunk_rows.  hs_spectral_rows: the rows of one chunk by the documented rule, before
 * the clamp to the batch (valid lengths only).  hs_spectral_args: every rejection of the two entry
 * points -- pointers, batch, lengths, totals, alignment, overlap.  0, or HSFFT_ERR_ARG with the
 * message set; none of them touches a device. */
#define HS_SPECTRAL_MAX_LEN HS_DCT_MAX_LEN
#define HS_SPECTRAL_MAX_WORDS (1LL << 40) /* n x batch and m x batch: dct::MAX_WORDS */
int hs_spectral_sizes(const char *who, int n, int m, int hilbert);
long long hs_spectral_rows(int n, int m);
int hs_spectral_args(const char *who, const void *d_in, int n, const void *d_out, int m, int batch, int hilbert);
/* The type-I cosine and sine transforms' host side (hsfft_dct1.c).  hs_dct1_sizes: the kind and
 * length rule of every type-I entry point, and the extended length L = 2(n-1) or 2(n+1) (L may be
 * NULL).  hs_dct1_rows: the rows of one chunk by the documented rule, before the clamp to the batch.
 * hs_dct1_args, hs_dct1_args_2d: every rejection of hsfft_dct1_batched and hsfft_dct1_2d_batched.  0,
 * or HSFFT_ERR_ARG with the message set; none of them touches a device.  The driver (hsfft_dct1.h)
 * keeps a chunk's extended rows in HS_SCR_DCT and their compact spectra in HS_SCR_DCT_SPEC, by the
 * argument of hsfft_dct_batched, which it never calls; hsfft_dct1_2d_batched keeps its chunk of
 * images in HS_SCR_2D as hsfft_dct_2d_batched does. */
#define HS_DCT1_MAX_WORDS (1LL << 40) /* n x batch, n0 x n1 x batch: dct::MAX_WORDS */
int hs_dct1_sizes(const char *who, int kind, int n, int *L);
long long hs_dct1_rows(int L);
int hs_dct1_args(const char *who, int kind, const void *d_in, const void *d_out, int n, int batch, int *L);
int hs_dct1_args_2d(const char *who, int kind0, int kind1, const void *d_in, const void *d_out, int n0, int n1, int batch,
                    int *L0, int *L1);
/* bytes from an environment knob given in MiB (default dflt_mb; at least 1 MiB) */
size_t hs_env_mb(const char *name, double dflt_mb);

#ifdef __cplusplus
}
#endif

#endif
