/*
 * hsfft_gpu.h -- MI355X extension API of libhsfft.so (no counterpart in the reference, which
 * has no batched or device-resident entry points).
 *
 * Conventions: plain pointers and sizes only.  "d_" pointers are device (HBM) pointers
 * obtained from hsfft_malloc (or any hipMalloc'd memory).  Batched transforms use contiguous
 * rows (row b starts at b*N samples).  Calls are asynchronous on the library stream of the
 * current device unless stated; hsfft_synchronize() waits.  Functions return 0 on success
 * and a negative code on error (message via hsfft_last_error()).
 */
#ifndef HSFFT_GPU_H_
#define HSFFT_GPU_H_

#include <stddef.h>
#include <stdint.h>

#include "highspeedFFT.h"
#include "real.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSFFT_OK 0
#define HSFFT_ERR_ARG -1
#define HSFFT_ERR_DEVICE -2
#define HSFFT_ERR_NOMEM -3
#define HSFFT_ERR_UNSUPPORTED -4

/* --- devices, memory, streams ---------------------------------------------------------- */
int hsfft_device_count(void);
int hsfft_set_device(int dev);          /* also selects the library stream of that device */
int hsfft_get_device(void);
void *hsfft_malloc(size_t bytes);        /* device memory on the current device, NULL on error */
int hsfft_free(void *d_ptr);
int hsfft_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes);  /* synchronous */
int hsfft_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes);  /* synchronous */
int hsfft_memset(void *d_ptr, int value, size_t bytes);
int hsfft_synchronize(void);
/* Frees the library's scratch pool on the current device (intermediates, staging slots,
 * convolution buffers) after waiting for queued work; the pool regrows on demand.  The pool
 * otherwise persists for the process: up to the largest chunk a call needed (c2c chains
 * HSFFT_CHUNK_MB, default 256 MiB x 2; Bluestein HSFFT_BLUE_CHUNK_MB, 4 GiB x 2; real paths
 * HSFFT_REAL_CHUNK_MB, 16 GiB; the 2D paths, complex and real, HSFFT_2D_CHUNK_MB, 1 GiB -- the
 * real 2D transforms hold that and the real paths' buffer together, the 2D cosine and sine
 * transforms that and the two buffers of HSFFT_DCT_CHUNK_MB; the overlap-add filter
 * HSFFT_FILTER_CHUNK_MB, 1 GiB; the STFT and its inverse HSFFT_STFT_CHUNK_MB, 1 GiB, in the
 * filter's first buffer; the cosine and sine transforms HSFFT_DCT_CHUNK_MB, 1 GiB, in the
 * filter's two buffers, the type-IV transforms too; the MDCT and its inverse HSFFT_MDCT_CHUNK_MB,
 * 1 GiB, in the 2D paths' buffer beside those two; the chirp-z transforms HSFFT_CZT_CHUNK_MB, 1 GiB,
 * in the cosine and sine transforms' two buffers; the analytic signal and Fourier resampling
 * HSFFT_SPECTRAL_CHUNK_MB, 1 GiB, in the same two buffers -- each halved while allocation fails).  Also
 * frees the current device's cached DCT rotation tables (at most four, rebuilt on demand), its
 * cached type-IV rotation tables (at most four more) and its cached chirp-z entries (at most four:
 * the tables, the wrapped chirp and its spectrum; hs_czt_release_device). */
int hsfft_release_scratch(void);
/* Teardown: waits for every device's work, then releases every device object the library
 * holds on every device -- scratch pool, page-locked staging slots, the device state of every
 * live plan (twiddles, odd-radix constants, Bluestein chirp / hk), real plans' device twiddles,
 * the cached DCT and type-IV rotation tables, the cached chirp-z entries (hs_czt_release_device), idle convolution plans, persistent-launch counters and the calling thread's error words (a
 * pending launch error of the calling thread is reported as by hsfft_synchronize), timing and
 * ordering events, the library streams.  Plans stay valid and everything is re-created on
 * demand, so the library remains usable.  Call it before process exit (bench.py and the test
 * session do), with no other library call running.  Returns 0 or a negative code. */
int hsfft_finalize(void);
void *hsfft_get_stream(void);            /* hipStream_t of the current device */
const char *hsfft_last_error(void);

/* --- plan options ---------------------------------------------------------------------- */
/* Twiddle mode for plans created afterwards by fft_init/fft_real_init on this thread:
 *   0 = reference (default): byte-identical to the reference planner, including its
 *       twiddle-table quirk;
 *   1 = exact: every stage twiddle from sincos (D2 fixed).
 * The environment variable HSFFT_TWIDDLE=exact sets the process default. */
int hsfft_set_twiddle_mode(int mode);
int hsfft_get_twiddle_mode(void);
/* Re-upload the plan's public twiddle array after the caller modified it in place. */
int hsfft_plan_refresh(fft_object obj);
/* Number of GPU passes (kernel launches per transform batch) the plan executes. */
int hsfft_plan_num_passes(fft_object obj);
/* Digit-reversal map of the reference recursion: output slot q holds input index map[q]
 * after the leaf stage (integer exact; N entries; mixed-radix plans only). */
int hsfft_digit_reverse_map(fft_object obj, int *map);

/* --- batched, device-resident execution ------------------------------------------------ */
/* c2c: d_in, d_out hold batch*N complex; d_in is not modified; d_in != d_out. */
int hsfft_exec_batched(fft_object obj, const fft_data *d_in, fft_data *d_out, int batch);
/* c2c on HOST-resident rows (the drop-in case of a caller that never touches HBM): rows are
 * streamed through HBM in chunks with upload / transform / download overlapped on three
 * streams; caller buffers are page-locked for the call where possible.  Synchronous. */
int hsfft_exec_batched_host(fft_object obj, const fft_data *h_in, fft_data *h_out, int batch);
/* r2c in the reference layout: batch rows of N reals -> batch rows of N complex (mirrored) */
int hsfft_r2c_batched(fft_real_object obj, const fft_type *d_in, fft_data *d_out, int batch);
/* r2c, compact layout: batch rows of N reals -> batch rows of N/2+1 complex (bins 0..N/2,
 * identical to the first N/2+1 bins of hsfft_r2c_batched; one third less HBM written) */
int hsfft_r2c_batched_compact(fft_real_object obj, const fft_type *d_in, fft_data *d_out, int batch);
/* c2r: batch rows of N complex (first N/2+1 read) -> batch rows of N reals */
int hsfft_c2r_batched(fft_real_object obj, const fft_data *d_in, fft_type *d_out, int batch);
/* batched linear/circular convolution of equal-length real rows (reference semantics of
 * fft_convolve, applied row-wise); returns the output length per row, or < 0 */
int hsfft_convolve_batched(const char *type, const char *conv_type, const fft_type *d_a,
                           int length1, const fft_type *d_b, int length2, fft_type *d_out,
                           int batch);

/* --- transforms along other axes: transpose, 2D, columns -------------------------------- */
/* All of these are asynchronous on the library stream and run under the device lock, like
 * hsfft_exec_batched; Bluestein lengths keep that call's error-word contract (below).  They
 * return HSFFT_ERR_ARG -- before any device is touched -- for NULL pointers, d_in == d_out or
 * input and output ranges that overlap, a negative batch or a dimension < 1; batch == 0 returns
 * 0.  d_in is never written.
 * hsfft_exec_2d and hsfft_exec_columns keep one scratch buffer in the library's pool (freed by
 * hsfft_release_scratch / hsfft_finalize): HSFFT_2D_CHUNK_MB (default 1024 MiB, at least 1)
 * bounds it, and a call walks its batch in chunks of whole images -- as many as fit, at least
 * one (hsfft_exec_columns holds two copies of a chunk, so half as many fit), halved while the
 * allocation fails. */
/* out[b][c][r] = in[b][r][c]; d_in != d_out, ranges must not overlap.  A pure copy of 16-byte
 * elements: every word, NaN payloads included, arrives unchanged. */
int hsfft_transpose_batched(const fft_data *d_in, fft_data *d_out, int rows, int cols, int batch);
/* The same transpose for batch matrices of rows x cols doubles, with the same contract and the same
 * rejections (the byte ranges are rows x cols x batch x 8 long): a pure copy of 8-byte elements,
 * every word -- NaN payloads, signed zeros, subnormals -- arrives unchanged.  The buffers need the
 * alignment of a double only.  The transpose between the row transforms of hsfft_dct_2d_batched. */
int hsfft_transpose_real_batched(const fft_type *d_in, fft_type *d_out, int rows, int cols, int batch);
/* 2D c2c of batch row-major images of p0->N rows by p1->N columns: the 1D transform of p1 on every
 * row, then the 1D transform of p0 on every column of that result (this order is part of the
 * contract: results are bit-identical to the reference's fft_exec applied that way). No scaling.
 * p0 and p1 may be one plan (square images) and may differ in sign: each is applied as planned.
 * Four trips through HBM per chunk: rows, transpose, rows (the columns), transpose. */
int hsfft_exec_2d(fft_object p0, fft_object p1, const fft_data *d_in, fft_data *d_out, int batch);
/* 1D c2c along axis 0 of batch row-major matrices of p->N rows by ncols columns (out[b][k][c] =
 * the transform over r of in[b][r][c]).  Three trips through HBM per chunk: transpose, rows,
 * transpose. */
int hsfft_exec_columns(fft_object p, const fft_data *d_in, fft_data *d_out, int ncols, int batch);
/* 2D transforms of real images.  In all three, r1 = fft_real_init(n1, s1) with n1 even is the real
 * plan of the rows, p0 (n0 = p0->N >= 1, any planned length) the plan of the columns, and a "half
 * spectrum" is n0 rows of n1/2+1 bins (row pitch n1/2+1).  Same conventions as above: asynchronous
 * under the device lock, the Bluestein error-word contract of hsfft_exec_batched, d_in never
 * written, no scaling.  HSFFT_ERR_ARG -- before any device is touched -- for NULL plans or
 * pointers, d_in == d_out or input and output byte ranges that overlap (each range with its own
 * element size and count), a negative batch; batch == 0 returns 0.  Scratch as above, with the
 * half spectrum as the image: a chunk is HSFFT_2D_CHUNK_MB / (copies x n0 x (n1/2+1) x 16) images,
 * at least one; hsfft_r2c_2d and hsfft_r2c_2d_full hold one copy of a chunk, hsfft_c2r_2d two. */
/* batch images of n0 x n1 reals -> batch half spectra of n0 x (n1/2+1) complex (row pitch n1/2+1):
 * bins 0..n1/2 of the reference's fft_r2c_exec(r1) on every row (what hsfft_r2c_batched_compact
 * writes), then the reference's fft_exec(p0) on each of the n1/2+1 columns of that result.  This
 * order is part of the contract: results are bit-identical to the reference applied that way. */
int hsfft_r2c_2d(fft_object p0, fft_real_object r1, const fft_type *d_in, fft_data *d_out, int batch);
/* same transform, reference-style full layout: n0 x n1 complex per image.  Columns k1 <= n1/2 hold
 * the words of hsfft_r2c_2d.  The mirror half, columns k1 = n1/2+1 .. n1-1, is a copy with a sign
 * flip, not a second column transform: out[k0][k1] = (re, -im) of out[(n0-k0) % n0][n1-k1], where
 * -im flips the sign bit (of zeros and NaNs too), as the reference builds the upper half of its
 * own 1D r2c rows.  With n1 == 2 there is no mirror column.  Every element is written once. */
int hsfft_r2c_2d_full(fft_object p0, fft_real_object r1, const fft_type *d_in, fft_data *d_out, int batch);
/* batch half spectra n0 x (n1/2+1) -> batch images of n0 x n1 reals: fft_exec(p0) on each of the
 * n1/2+1 columns of the input, then the reference's fft_c2r_exec(r1) on every row of that result
 * (it reads bins 0..n1/2, here at pitch n1/2+1).  Compositional: holds for any input words,
 * Hermitian-consistent or not. */
int hsfft_c2r_2d(fft_object p0, fft_real_object r1, const fft_data *d_in, fft_type *d_out, int batch);

/* --- batched 2D convolution of real images ---------------------------------------------- */
/* Sizes only, no device touched.  Each axis follows the 1D rule of fft_convolve / hsfft_convolve_batched
 * on its own, with n and m the two operands' lengths on that axis: "linear" has clen = n + m - 1,
 * "circular" clen = max(n, m); the padded transform size is P = next_power_of_two(clen).  Linear
 * returns the window `type` selects -- "full" (or NULL): clen samples from 0; "same": max(n, m)
 * samples from (clen - max(n, m)) / 2; "valid": max(n, m) - min(n, m) + 1 samples from
 * min(n, m) - 1 -- and circular returns all P samples (type is still checked, then not used).
 * Writes the output image's rows and columns and the padded sizes P0 = *pad_rows (from the row
 * counts) and P1 = *pad_cols (from the widths); a NULL result pointer is skipped.  Returns 0, or
 * HSFFT_ERR_ARG with a message for a NULL or unknown conv_type, an unknown type, a dimension
 * < 1, P1 < 2 (both widths 1: a real plan of length 1 does not exist) or an empty window. */
int hsfft_convolve_2d_shape(const char *type, const char *conv_type, int a_rows, int a_cols, int b_rows,
                            int b_cols, int *out_rows, int *out_cols, int *pad_rows, int *pad_cols);
/* d_a: batch contiguous row-major real images of a_rows x a_cols; d_b: b_batch images of b_rows x
 * b_cols, where b_batch is batch (one kernel per image) or 1 (one kernel shared by every image, the
 * filtering case); d_out: batch contiguous images of out_rows x out_cols (hsfft_convolve_2d_shape).
 * The contract is compositional.  With w = P1/2+1, p0 = fft_init(P0, 1), q0 = fft_init(P0, -1), r1 =
 * fft_real_init(P1, 1) and s1 = fft_real_init(P1, -1):
 *   A = what hsfft_r2c_2d(p0, r1) gives on a placed at the top-left of a P0 x P1 image of +0.0,
 *   B = the same for b,
 *   C[k] = (A.re*B.re - A.im*B.im, A.re*B.im + A.im*B.re), every multiply, subtract and add rounded
 *          on its own (the operand order of the reference's 1D product),
 *   y = what hsfft_c2r_2d(q0, s1) gives on C,
 *   out[r][c] = y[start0 + r][start1 + c] / (double)((long long)P0 * P1), one division per element.
 * No zero row or column is skipped.  Internally the product runs on the transposed half spectra
 * ([k1][k0]), so the last transpose of each forward transform and the first of the inverse are not
 * run; padding, product and window use the row-copy and product kernels of the 1D convolution; the
 * words are those of the composition above.  The four plans come from the library's convolution plan cache: a call
 * with padded sizes it has seen before builds no plan.
 * Asynchronous on the library stream under the device lock, like hsfft_exec_2d; the inputs are
 * never written; Bluestein lengths would keep the error-word contract of hsfft_exec_batched
 * (below), although power-of-two plans never take that path.  Returns 0 on success and for batch
 * == 0.  HSFFT_ERR_ARG with a message -- before any device is touched -- for what
 * hsfft_convolve_2d_shape rejects, NULL data pointers, batch < 0, b_batch not 1 or batch (when
 * batch > 0), and a d_out byte range that overlaps either input's (each range with its own size).
 * Scratch: the HSFFT_2D_CHUNK_MB buffer of the 2D transforms with the padded half spectrum as the
 * image.  A call walks its batch in chunks of HSFFT_2D_CHUNK_MB / (3 x P0 x (P1/2+1) x 16) image
 * pairs, at least one, halved while the allocation fails; a shared kernel's spectrum is one more
 * image in the same buffer that the rule does not count.  No allocation per call. */
int hsfft_convolve_2d_batched(const char *type, const char *conv_type, const fft_type *d_a, int a_rows,
                              int a_cols, const fft_type *d_b, int b_rows, int b_cols, int b_batch,
                              fft_type *d_out, int batch);

/* --- batched overlap-add filtering of long real rows by one shared kernel ---------------- */
/* Linear convolution of `batch` rows of n reals with ONE kernel of m reals, by overlap-add: each
 * row is cut into blocks of L samples, each block is convolved with the kernel at the padded
 * length P = L + m - 1, and the m - 1 samples by which neighbouring blocks overlap are added.  The
 * kernel is transformed once per call, the transforms have P points instead of
 * next_power_of_two(n + m - 1), and the scratch is bounded by a knob, not by the job. */
#define HSFFT_FILTER_BLOCK_MIN 8192 /* floor of the automatic block: the fastest measured block */
/* Sizes only, no device touched; a NULL result pointer is skipped.  clen = n + m - 1.  The window
 * is the 1D rule of fft_convolve / hsfft_convolve_batched: "full" (or NULL): clen samples from 0;
 * "same": max(n, m) samples from (clen - max(n, m)) / 2; "valid": max(n, m) - min(n, m) + 1
 * samples from min(n, m) - 1; its length goes to *out_len.  With Q = max(2,
 * next_power_of_two(clen)): block == 0 is automatic, P = min(max(HSFFT_FILTER_BLOCK_MIN,
 * next_power_of_two(4 m)), Q); otherwise P = block, which must be a power of two, >= 2 and >= m.
 * L = P - m + 1 and nseg = ceil(n / L) blocks per row.  With nseg > 1, L >= m - 1 is required, so
 * that at most two blocks meet at any output sample (the automatic rule always satisfies it).
 * Returns 0, or HSFFT_ERR_ARG with a message for n or m < 1, clen > 2^30, an unknown type, or a
 * block that breaks these rules. */
int hsfft_filter_shape(const char *type, int n, int m, int block, int *out_len, int *P, int *L, int *nseg);
/* d_x: batch contiguous rows of n reals; d_h: one kernel of m reals, shared by every row; d_out:
 * batch contiguous rows of out_len reals (hsfft_filter_shape).  The contract is compositional.
 * With f = fft_real_init(P, 1), g = fft_real_init(P, -1), for block s of row b:
 *   u_s = x[b][sL .. sL+L) at the start of P words of +0.0 (the last block is shorter; nothing is
 *         read past the end of row b),
 *   H   = bins 0..P/2 of the reference's fft_r2c_exec(f) on h at the start of P words of +0.0,
 *   U_s = the same transform of u_s,
 *   C_s[k] = (U.re*H.re - U.im*H.im, U.re*H.im + U.im*H.re), every operation rounded on its own,
 *          the block's spectrum as the left operand (the reference's 1D product),
 *   y_s = the reference's fft_c2r_exec(g) of C_s,  v_s[i] = y_s[i] / (double)P, one division each,
 *   full[g] for g = sL + j, 0 <= j < L, s < nseg:  v_s[j] when s == 0 or j >= m - 1, else
 *          v_s[j] + v_{s-1}[L + j], in this order;
 *   full[g] for g >= nseg L (the tail after the last block) = v_{nseg-1}[g - (nseg-1) L],
 *   out[b][t] = full[start + t].
 * v_s is, word for word, what the reference's fft_convolve("full", "linear", u_s[0..L), L, h, m, .)
 * returns, so the output is a sum of reference results; with P == Q there is one block and the
 * words are those of hsfft_convolve_batched on the same rows with the kernel replicated per row.
 * No block is skipped for being zero.  Where two blocks add and both terms are NaN, the payload is
 * not part of the contract; everything else is.
 * Asynchronous on the library stream under the device lock, like hsfft_exec_2d; the inputs are
 * never written; every output word is written exactly once and none is read.  Returns 0 on success
 * and for batch == 0.  HSFFT_ERR_ARG with a message -- before any device is touched -- for NULL
 * pointers, batch < 0, what hsfft_filter_shape rejects, and a d_out byte range that overlaps
 * d_x's or d_h's.  The two real plans come from the convolution plan cache.
 * Scratch: two pool buffers, no allocation per call.  Blocks are numbered q = b nseg + s and walked
 * in chunks of HSFFT_FILTER_CHUNK_MB / (P x 8 + (P/2+1) x 16) consecutive blocks
 * (HSFFT_FILTER_CHUNK_MB: default 1024 MiB, at least 1, read per call), at least one, halved while
 * the allocation fails; a chunk may cross row boundaries.  The kernel's spectrum and the m - 1
 * words a chunk hands to the next lie behind the second buffer, and the rule does not count them. */
int hsfft_filter_batched(const char *type, const fft_type *d_x, int n, const fft_type *d_h, int m, int block,
                         fft_type *d_out, int batch);

/* --- batched short-time Fourier transform of real rows, and its inverse ------------------ */
/* The frames of an STFT overlap: they start `hop` samples apart and are N long, each is multiplied
 * by a window of N reals and transformed by r2c.  The inverse runs c2r on every frame, windows it
 * again and adds the frames that cover each output sample.  Both compose the unchanged row
 * transforms with one new kernel each; the window and the framing are not fused into a transform
 * pass. */
/* Sizes only, no device touched; a NULL result pointer is skipped and a rejected call writes
 * nothing.  N is the frame length (even, >= 2; N = 2 * r->cobj->N for a real plan r), hop >= 1,
 * n >= 1 the row length, center 0 or 1.  *lpad = center ? N/2 : 0 and *bins = N/2 + 1.  Frame f
 * covers the positions p = f hop - lpad + j, 0 <= j < N, of its row; a position outside [0, n)
 * reads as +0.0.  center == 0 requires n >= N and gives *nframes = 1 + (n - N) / hop (trailing
 * samples that no frame reaches are not read); center == 1 gives *nframes = 1 + n / hop, the
 * frame count of the usual centred STFT, with zero instead of reflected padding.  Returns 0, or
 * HSFFT_ERR_ARG with a message for an odd N, N < 2, hop < 1, n < 1, a center other than 0 or 1,
 * n < N with center == 0, or n or N > 2^30. */
int hsfft_stft_shape(int n, int N, int hop, int center, int *nframes, int *bins, int *lpad);
/* d_x: batch contiguous rows of n reals; d_w: a window of N = 2 * r->cobj->N reals shared by every
 * frame, or NULL; d_out: batch x nframes x (N/2+1) complex, contiguous, frame-major.  The contract
 * is compositional.  For frame f of row b:
 *   u[j] = xpad[f hop - lpad + j] * w[j], one multiply rounded on its own, computed for every j: a
 *          padded position contributes +0.0 * w[j], whatever that is (-0.0 for a negative tap);
 *          with d_w == NULL there is no multiply, u[j] = xpad[f hop - lpad + j];
 *   out[b][f][0..N/2] = bins 0..N/2 of the reference's fft_r2c_exec(r) on u -- the words
 *          hsfft_r2c_batched_compact writes.
 * r is applied as planned: either sign, any even length a real plan supports (mixed-radix or
 * Bluestein inner lengths, N == 2); Bluestein inner lengths keep the error-word contract of
 * hsfft_exec_batched (below).  Nothing is read outside row b, and no frame is skipped for being
 * zero.
 * Asynchronous on the library stream under the device lock, like hsfft_filter_batched; the inputs
 * are never written; every output word is written exactly once and none is read.  Returns 0 on
 * success and for batch == 0.  HSFFT_ERR_ARG with a message -- before any device is touched -- for
 * a NULL plan, d_x or d_out, batch < 0, what hsfft_stft_shape rejects, nframes x batch > 2^31 - 1,
 * n x batch or nframes x batch x N > 2^40 (the byte counts of the call's buffers then fit 64 bits
 * with room to spare), and a d_out byte range that overlaps d_x's or d_w's.
 * Scratch: one pool buffer, no allocation per call.  Frames are numbered q = b nframes + f and
 * walked in chunks of HSFFT_STFT_CHUNK_MB / (N x 8) consecutive frames (HSFFT_STFT_CHUNK_MB:
 * default 1024 MiB, at least 1, read per call), at least one, halved while the allocation fails; a
 * chunk may cross row boundaries.  Per chunk the frames are gathered and windowed into the scratch
 * and transformed from there straight into d_out. */
int hsfft_stft_batched(fft_real_object r, const fft_type *d_x, int n, const fft_type *d_w, int hop,
                       int center, fft_data *d_out, int batch);
/* d_spec: batch x nframes x (N/2+1) complex with N = 2 * ri->cobj->N; d_w: a window of N reals or
 * NULL; d_out: batch contiguous rows of n reals.  The contract is compositional and holds for any
 * input words, Hermitian-consistent or not:
 *   y_f = the reference's fft_c2r_exec(ri) on frame f (it reads bins 0..N/2, here at pitch N/2+1),
 *   v_f[j] = y_f[j] / (double)N, one division,
 *   t_f[j] = v_f[j] * w[j], one multiply; v_f[j] itself with d_w == NULL.
 * For output sample i of row b let F(i) be the frames f in [0, nframes) with 0 <= i + lpad - f hop
 * < N, in increasing f.  acc starts as the first frame's term t_f[i + lpad - f hop], not as 0.0,
 * and each later term is added in that order, one rounded add each.  With normalize != 0, env is
 * built the same way from w[j] * w[j], each product rounded (from 1.0 per frame with d_w == NULL),
 * and out[b][i] = acc / env, one division; no threshold is applied, a zero envelope gives the IEEE
 * result.  With normalize == 0, out[b][i] = acc.  A sample that no frame covers (hop > N, or
 * beyond the last frame's reach) is +0.0 in both modes.  n >= 1 is otherwise free: it need not be
 * the length the frames came from, and a shorter n trims.  Where two or more NaN terms meet, the
 * payload is not part of the contract; everything else is.
 * Conventions and rejections as for hsfft_stft_batched, with hop >= 1, center 0 or 1, 1 <= n <=
 * 2^30 (n < N is allowed here), nframes >= 1, the same bounds on the totals, and a d_out range
 * that overlaps d_spec's or d_w's.
 * Scratch: the same pool buffer.  Whole rows are walked in chunks of HSFFT_STFT_CHUNK_MB /
 * (nframes x N x 8) rows, at least one, halved while the allocation fails down to one row, then
 * HSFFT_ERR_NOMEM; a row's frames never straddle a chunk.  One row larger than the knob still runs
 * as one chunk. */
int hsfft_istft_batched(fft_real_object ri, const fft_data *d_spec, int nframes, const fft_type *d_w,
                        int hop, int center, int normalize, fft_type *d_out, int n, int batch);

/* --- batched cosine and sine transforms (DCT-II / III, DST-II / III) of real rows --------- */
/* The conventions are scipy's with norm=None, unnormalised, for rows of N = n reals:
 *   DCT-II   X[k] = 2 sum_n x[n] cos(pi k (2n+1) / 2N)
 *   DCT-III  y[n] = X[0] + 2 sum_{k>=1} X[k] cos(pi k (2n+1) / 2N)
 *   DST-II   X[k] = 2 sum_n x[n] sin(pi (k+1) (2n+1) / 2N)
 *   DST-III  y[n] = (-1)^n X[N-1] + 2 sum_{k<N-1} X[k] sin(pi (k+1) (2n+1) / 2N)
 * so that type 3 of type 2 of x is 2N x.  Each is Makhoul's N-point algorithm: the unchanged r2c
 * or c2r row transform of length N with one new kernel before it and one after; the permutation
 * and the rotation are not fused into a transform pass.  Only even n: a real plan needs an even
 * length.  Odd lengths, types I and IV and orthonormal scaling are out of scope. */
#define HSFFT_KIND_COS 0
#define HSFFT_KIND_SIN 1
/* Host only, no device touched: the n/2+1 rotation words the calls below use, h_tw[k] = (c_k, s_k)
 * for 0 <= k <= n/2 from one libm sincos(PI2 * (double)k / (4.0 * (double)n), &s_k, &c_k) each (PI2
 * of highspeedFFT.h; the angle is pi k / 2n).  Returns 0, or HSFFT_ERR_ARG with a message for n
 * odd, n < 2, n > 2^30 or a NULL h_tw. */
int hsfft_dct_twiddles(int n, fft_data *h_tw);
/* kind: HSFFT_KIND_COS / HSFFT_KIND_SIN; type: 2 or 3; d_in, d_out: batch contiguous rows of n
 * reals.  The contract is compositional and bit-exact.  With N = n, h = N/2, f = fft_real_init(N, 1),
 * g = fft_real_init(N, -1) and t = the table of hsfft_dct_twiddles(N), per row:
 * DCT-II:
 *   v[j] = x[2j], v[N-1-j] = x[2j+1] for j < h,
 *   V = bins 0..h of the reference's fft_r2c_exec(f) on v -- the words hsfft_r2c_batched_compact
 *       writes,
 *   re_k = V.re*c_k + V.im*s_k, im_k = V.im*c_k - V.re*s_k, every multiply, add and subtract rounded
 *       on its own and computed for every k with no special case,
 *   out[k] = 2.0*re_k for 0 <= k <= h, out[N-k] = -2.0*im_k for 1 <= k < h.
 * DCT-III:
 *   V[0] = (X[0], +0.0) with no arithmetic (an infinite X[0] stays infinite),
 *   V[k] = (a*c_k + b*s_k, a*s_k - b*c_k) with a = X[k], b = X[N-k] for 1 <= k <= h, each operation
 *       rounded on its own,
 *   y = the reference's fft_c2r_exec(g) on V (it reads bins 0..h, here at pitch h+1), unscaled,
 *   out[2j] = y[j], out[2j+1] = y[N-1-j] for j < h.
 * DST-II is DCT-II of x' with x'[n] = x[n] for even n and the sign bit of x[n] flipped for odd n
 * (of zeros and NaNs too), written reversed: out[k] = X'[N-1-k].  DST-III is DCT-III of X'[k] =
 * X[N-1-k] with out[n] = y[n] for even n and the sign bit flipped for odd n.  Both are index and
 * sign variants inside the same two kernels, with no extra pass over memory.  Where two NaN terms
 * meet in one add, the payload is not part of the contract; everything else is.
 * The two plans come from the convolution plan cache: they follow the calling thread's twiddle
 * mode, and a repeated length builds nothing.  Any even length a real plan supports (mixed-radix
 * or Bluestein inner lengths, N == 2); Bluestein inner lengths keep the error-word contract of
 * hsfft_exec_batched (below).
 * Asynchronous on the library stream under the device lock, like hsfft_stft_batched; the input is
 * never written; every output word is written exactly once and none is read.  Returns 0 on
 * success and for batch == 0.  HSFFT_ERR_ARG with a message -- before any device is touched -- for
 * a kind other than 0 or 1, a type other than 2 or 3, n odd, n < 2 or n > 2^30, batch < 0,
 * n x batch > 2^40, NULL pointers, d_in == d_out or input and output byte ranges that overlap.
 * Scratch: two pool buffers (the filter's), no allocation per call.  Rows are walked in chunks of
 * HSFFT_DCT_CHUNK_MB / (N x 8 + (N/2+1) x 16) rows (HSFFT_DCT_CHUNK_MB: default 1024 MiB, at least
 * 1, read per call), at least one, halved while the allocation fails.  The table is cached on the
 * device, four lengths per device, the least recently used one replaced: a length not in the cache
 * builds its table on the host and uploads it synchronously. */
int hsfft_dct_batched(int kind, int type, const fft_type *d_in, fft_type *d_out, int n, int batch);

/* --- batched 2D cosine and sine transforms of real images -------------------------------- */
/* batch contiguous row-major real images of n0 rows by n1 columns -> batch images of the same
 * shape.  kind1 (HSFFT_KIND_COS / HSFFT_KIND_SIN) is the transform along the rows (axis 1), kind0
 * the transform along the columns (axis 0); one type, 2 or 3, for both axes, in the conventions
 * above (scipy's dctn / dstn with norm=None for equal kinds; mixed kinds are what a Poisson solver
 * with mixed boundaries needs).  Type 3 of type 2 of x is 4 n0 n1 x.
 * The contract is compositional and bit-exact: the result is, word for word, hsfft_dct_batched(kind1,
 * type) on every row and then hsfft_dct_batched(kind0, type) on every column of that result -- rows
 * first, then columns, for both types.  The row transforms are that call's kernels unchanged; in
 * between the images are transposed by the copy of hsfft_transpose_real_batched.  Per chunk: rows
 * d_in -> scratch, transpose scratch -> d_out, rows d_out -> scratch (the columns, now contiguous),
 * transpose scratch -> d_out; four trips through HBM beside the row transforms' own.
 * Everything else is hsfft_dct_batched's: both plan pairs come from the convolution plan cache and
 * both rotation tables from the four-entry cache (the two lengths alternate inside one call and
 * both stay cached), Bluestein inner lengths keep the error-word contract of hsfft_exec_batched,
 * the call is asynchronous on the library stream under the device lock, d_in is never written and
 * every output word is written.  Returns 0 on success and for batch == 0.  HSFFT_ERR_ARG with a
 * message -- before any device is touched -- for a kind other than 0 or 1, a type other than 2 or
 * 3, n0 or n1 odd, below 2 or above 2^30, batch < 0, n0 x n1 x batch > 2^40, NULL pointers,
 * d_in == d_out or input and output byte ranges that overlap.
 * Scratch: one copy of a chunk in the 2D transforms' pool buffer, beside the two buffers the row
 * transforms keep (and walk in chunks of their own, HSFFT_DCT_CHUNK_MB).  A call walks its batch in
 * chunks of HSFFT_2D_CHUNK_MB / (n0 x n1 x 8) images (default 1024 MiB), at least one, at most the
 * batch and at most what keeps a chunk's row count -- images x max(n0, n1) -- an int; halved while
 * the allocation fails; the last chunk may be ragged. */
int hsfft_dct_2d_batched(int kind0, int kind1, int type, const fft_type *d_in, fft_type *d_out, int n0, int n1,
                         int batch);

/* --- batched type-IV cosine and sine transforms (DCT-IV / DST-IV) of real rows ------------ */
/* scipy's conventions with norm=None, for rows of N = n reals:
 *   DCT-IV   X[k] = 2 sum_n x[n] cos(pi (2k+1) (2n+1) / 4N)
 *   DST-IV   X[k] = 2 sum_n x[n] sin(pi (2k+1) (2n+1) / 4N)
 * so that either one applied twice gives 2N x.  Each is the unchanged c2c row transform of length
 * N/2 with one new kernel before it and one after; there is no split pass, as the r2c of the
 * types II and III has.  Entry points of their own: hsfft_dct_batched keeps rejecting type 4.  Only
 * even n; type I, odd lengths, orthonormal scaling and a 2D type IV are out of scope.
 * Host only, no device touched: the n/2 rotation words the calls below use, h_tw[j] = (c_j, s_j)
 * for 0 <= j < n/2 from one libm sincos(PI2 * (double)(8*j + 1) / (16.0 * (double)n), &s_j, &c_j)
 * each (the angle is pi (8j+1) / 8n; one table serves both rotations).  Returns 0, or HSFFT_ERR_ARG
 * with a message for n odd, n < 2, n > 2^30 or a NULL h_tw. */
int hsfft_dct4_twiddles(int n, fft_data *h_tw);
/* kind: HSFFT_KIND_COS / HSFFT_KIND_SIN; d_in, d_out: batch contiguous rows of n reals.  The
 * contract is compositional and bit-exact.  With N = n, h = N/2, t = the table of
 * hsfft_dct4_twiddles(N) and a gain g = 2.0, per row (the cosine form):
 *   a_j = x[2j], b_j = x[N-1-2j], z[j] = (a_j*c_j + b_j*s_j, b_j*c_j - a_j*s_j) for j < h,
 *   Z = the reference's fft_exec of the forward plan fft_init(h, 1) on z (h == 1: a copy),
 *   re_k = Z[k].re*c_k + Z[k].im*s_k, im_k = Z[k].im*c_k - Z[k].re*s_k,
 *   out[2k] = g*re_k, out[N-1-2k] = (-g)*im_k for k < h,
 * every multiply, add and subtract rounded on its own and computed for every index with no
 * special case.  The sine form is the cosine form of the reversed row, x'[n] = x[N-1-n], with the
 * sign bit of the odd outputs flipped (of zeros and NaNs too): an index and sign variant inside the
 * same two kernels, with no extra pass over memory.  Where two NaN terms meet in one add, the
 * payload is not part of the contract; everything else is.
 * The plan comes from the convolution plan cache: it follows the calling thread's twiddle mode, and
 * a repeated length builds nothing.  Any even n (mixed-radix or Bluestein h, h == 1); Bluestein h
 * keep the error-word contract of hsfft_exec_batched (below).
 * Asynchronous on the library stream under the device lock; the input is never written; every
 * output word is written exactly once and none is read; caller rows need the alignment of a
 * double only.  Returns 0 on success and for batch == 0.  HSFFT_ERR_ARG with a message -- before any
 * device is touched -- for a kind other than 0 or 1, n odd, n < 2 or n > 2^30, batch < 0, n x batch >
 * 2^40, NULL pointers, d_in == d_out or input and output byte ranges that overlap.
 * Scratch: the two pool buffers of hsfft_dct_batched, N/2 complex per row each, no allocation per
 * call.  Rows are walked in chunks of HSFFT_DCT_CHUNK_MB / (N x 16) rows (default 1024 MiB, at
 * least 1, read per call), at least one, halved while the allocation fails.  The table is cached on
 * the device in a cache of its own, four lengths per device, the least recently used one replaced:
 * a length not in the cache builds its table on the host and uploads it synchronously. */
int hsfft_dct4_batched(int kind, const fft_type *d_in, fft_type *d_out, int n, int batch);

/* --- batched type-I cosine and sine transforms (DCT-I / DST-I) of real rows and images ----- */
/* scipy's conventions with norm=None, for rows of n reals -- the transforms of grids that include
 * their boundary points (DCT-I, Neumann) or exclude them (DST-I, Dirichlet):
 *   DCT-I, n >= 2   X[k] = x[0] + (-1)^k x[n-1] + 2 sum_{j=1..n-2} x[j] cos(pi j k / (n-1))
 *   DST-I, n >= 1   X[k] = 2 sum_{j=0..n-1} x[j] sin(pi (j+1) (k+1) / (n+1))
 * Each is its own inverse up to the factor 2(n-1) (DCT-I) or 2(n+1) (DST-I).  Each is the unchanged
 * r2c row transform of the symmetrically extended row -- length L = 2(n-1) or 2(n+1) -- with one new
 * kernel before it and one after, neither of which does arithmetic; nothing is fused into a
 * transform pass and there is no table.  L is even for every n, so these calls take every length,
 * odd ones included; types 2, 3 and 4 stay even-only.  Entry points of their own: hsfft_dct_batched
 * and hsfft_dct_2d_batched keep rejecting type 1.  An (n-1)-point fast algorithm and orthonormal
 * scaling are out of scope.
 * Host only, no device touched: the extended length into *L and its L/2+1 compact bins into *bins
 * (NULL is skipped).  Returns 0, or HSFFT_ERR_ARG with a message for exactly the kinds and lengths
 * that hsfft_dct1_batched rejects: a kind other than 0 or 1, n < 2 (cosine) or n < 1 (sine), or
 * L > 2^30. */
int hsfft_dct1_shape(int kind, int n, int *L, int *bins);
/* kind: HSFFT_KIND_COS / HSFFT_KIND_SIN; d_in, d_out: batch contiguous rows of n reals.  The
 * contract is compositional and bit-exact.  Per row x, with f = fft_real_init(L, 1):
 * cosine, L = 2(n-1):
 *   e[t] = x[t] for 0 <= t <= n-1, e[L-t] = x[t] for 1 <= t <= n-2,
 *   S = bins 0..L/2 of the reference's fft_r2c_exec(f) on e -- the words hsfft_r2c_batched_compact
 *       writes,
 *   out[k] = S[k].re for 0 <= k <= n-1: a copy.
 * sine, L = 2(n+1):
 *   e[0] = e[n+1] = +0.0, e[j+1] = x[j], e[L-1-j] = x[j] with its sign bit flipped (of zeros and NaNs
 *       too, no arithmetic) for 0 <= j <= n-1,
 *   S as above,
 *   out[k] = S[k+1].im with its sign bit flipped for 0 <= k <= n-1; S[0] and S[n+1] are not read.
 * Every output word is the named component of the reference's r2c of the extended row, so results
 * follow the calling thread's twiddle mode (the plan comes from the convolution plan cache; a
 * repeated length builds nothing): full accuracy where L is a power of two -- n = 2^p + 1 for the
 * cosine, n = 2^p - 1 for the sine -- about 1e-11 in the exact mode on L with factors 3, 5 or 7, and
 * in the default (reference) mode the reference's twiddle-quirk results on L such as 6 and 12
 * (hsfft_set_twiddle_mode above), which are far from the definition.  The bit-exact contract holds
 * at every length regardless.  Any L a real plan supports (mixed-radix or Bluestein inner lengths,
 * L == 2); Bluestein inner lengths keep the error-word contract of hsfft_exec_batched (below).
 * Asynchronous on the library stream under the device lock; the input is never written; every
 * output word is written exactly once and none is read; caller rows need the alignment of a
 * double only (rows of odd n alternate between 8- and 16-byte alignment anyway).  Returns 0 on
 * success and for batch == 0.  HSFFT_ERR_ARG with a message -- before any device is touched -- for a
 * kind other than 0 or 1, n < 2 (cosine) or n < 1 (sine), L > 2^30, batch < 0, n x batch > 2^40, NULL
 * pointers, d_in == d_out or input and output byte ranges that overlap.
 * Scratch: the two pool buffers of hsfft_dct_batched, no allocation per call: the extended rows and
 * their compact spectra.  Rows are walked in chunks of HSFFT_DCT_CHUNK_MB / (L x 8 + (L/2+1) x 16)
 * rows (HSFFT_DCT_CHUNK_MB: default 1024 MiB, at least 1, read per call), at least one and at most
 * the batch, halved while the allocation fails; HSFFT_ERR_NOMEM if one row still fails. */
int hsfft_dct1_batched(int kind, const fft_type *d_in, fft_type *d_out, int n, int batch);
/* batch contiguous row-major real images of n0 rows by n1 columns -> batch images of the same
 * shape.  kind1 is the transform along the rows (axis 1, length n1), kind0 the transform along the
 * columns (axis 0, length n0): scipy's dctn / dstn with type=1, norm=None for equal kinds; mixed
 * kinds are what a Poisson solver on a vertex grid with mixed boundaries needs.  Applied twice it
 * gives the image times the product of the two axes' factors.
 * The contract is compositional and bit-exact: the result is, word for word, hsfft_dct1_batched(kind1)
 * on every row and then hsfft_dct1_batched(kind0) on every column of that result.  The row
 * transforms are that call's kernels unchanged; in between the images are transposed by the copy of
 * hsfft_transpose_real_batched.  Per chunk: rows d_in -> scratch, transpose scratch -> d_out, rows
 * d_out -> scratch (the columns, now contiguous), transpose scratch -> d_out.
 * Everything else is hsfft_dct1_batched's, per axis: the length rule (either axis may be odd, and so
 * may n0 x n1), the twiddle mode, the alignment of a double, asynchronous on the library stream
 * under the device lock, d_in never written, every output word written.  Returns 0 on success and
 * for batch == 0.  HSFFT_ERR_ARG with a message -- before any device is touched -- for a kind other
 * than 0 or 1, an axis below 2 (cosine) or 1 (sine) or with L > 2^30, batch < 0, n0 x n1 x batch >
 * 2^40, NULL pointers, d_in == d_out or input and output byte ranges that overlap.
 * Scratch: one copy of a chunk in the 2D transforms' pool buffer, beside the two buffers the row
 * transforms keep (and walk in chunks of their own, HSFFT_DCT_CHUNK_MB).  A call walks its batch in
 * chunks of HSFFT_2D_CHUNK_MB / (16 x ceil(n0 x n1 / 2)) images (default 1024 MiB; the pool counts
 * 16-byte words, so an odd image is rounded up by one double), at least one, at most the batch and
 * at most what keeps a chunk's row count -- images x max(n0, n1) -- an int; halved while the
 * allocation fails; the last chunk may be ragged. */
int hsfft_dct1_2d_batched(int kind0, int kind1, const fft_type *d_in, fft_type *d_out, int n0, int n1, int batch);

/* --- batched MDCT and IMDCT of real rows -------------------------------------------------- */
/* The lapped transform of audio codecs: frames of 2N samples, N apart (N even, 2 to 2^30), N
 * coefficients per frame; a window d_w of 2N reals, or NULL for none.
 *   forward   X[k] = sum_{m<2N} u[m] cos(pi/N (m + 1/2 + N/2) (k + 1/2)),   u = frame x window
 *   backward  y[m] = the same sum over k < N
 * With pad == 0 frame f starts at sample f N; with pad == 1 at f N - N, so that the first and the
 * last N samples of a row lie in two frames as well; lpad = pad ? N : 0, and a position outside
 * [0, n) reads +0.0.
 * Sizes only, no device touched: n % N == 0 is required; pad == 0 needs n >= 2N and gives nframes =
 * n/N - 1, pad == 1 needs n >= N and gives nframes = n/N + 1.  nframes and lpad may be NULL.
 * HSFFT_ERR_ARG with a message for anything else, N odd, N < 2, N or n above 2^30, n < 1, or a pad
 * other than 0 or 1. */
int hsfft_mdct_shape(int n, int N, int pad, int *nframes, int *lpad);
/* d_x: batch rows of n reals; d_out: batch x nframes x N reals, frame-major.  Bit-exact contract,
 * frame f of row b, q = N/2:
 *   p[m] = xpad[f N - lpad + m] * w[m], one multiply (computed on the +0.0 outside the row too); no
 *       multiply for a NULL d_w,
 *   u[i] = (-p[3q-1-i]) - p[3q+i] for i < q, u[i] = p[i-q] - p[3q-1-i] for q <= i < N, the unary
 *       minus a flip of the sign bit,
 *   out[b][f][:] = the hsfft_dct4_batched contract (cosine) on u with the gain g = 1.0.
 * One kernel gathers, windows and folds into a scratch of rows of N; the type-IV driver runs from
 * there into d_out.  Asynchronous like hsfft_dct4_batched; inputs are never written.  Returns 0 on
 * success and for batch == 0.  HSFFT_ERR_ARG with a message -- before any device is touched -- for
 * what hsfft_mdct_shape rejects, NULL d_x or d_out, batch < 0, nframes x batch > 2^31 - 1, n x batch
 * or nframes x batch x N above 2^40, or a d_out range that overlaps d_x's or d_w's.
 * Scratch: the 2D transforms' pool buffer, beside the two of hsfft_dct4_batched (walked in chunks of
 * their own).  Consecutive frames b nframes + f are walked in chunks of HSFFT_MDCT_CHUNK_MB / (N x 8)
 * frames (default 1024 MiB, at least 1, read per call), at least one, halved while the allocation
 * fails; a chunk may cross rows. */
int hsfft_mdct_batched(const fft_type *d_x, int n, const fft_type *d_w, int N, int pad, fft_type *d_out, int batch);
/* d_X: batch x nframes x N coefficients; d_out: batch rows of n = (nframes + 1) N - 2 lpad reals,
 * n >= 1 (so pad == 1 needs nframes >= 2).  Bit-exact contract, q = N/2:
 *   v_f = the hsfft_dct4_batched contract (cosine) on frame f's coefficients with g = 1.0,
 *   y_f[m] = v_f[m+q] for m < q, -v_f[3q-1-m] for q <= m < 3q, -v_f[m-3q] for 3q <= m < 2N (sign-bit
 *       flips),
 *   t_f[m] = (y_f[m] / (double)q) * w[m]: one division and one multiply, the multiply absent for a
 *       NULL d_w,
 *   out[b][i], with P = i + lpad: the term t_f[P - f N] of the earlier covering frame f = P/N - 1 where
 *       that is >= 0, then the term of frame P/N added where that is < nframes; a single covering
 *       frame gives its term alone, not 0.0 + term.
 * With a Princen-Bradley window, w[m]^2 + w[m+N]^2 = 1, the division by N/2 makes imdct(mdct(x))
 * equal x on every sample that two frames cover.  One kernel reads the two v rows per sample and
 * writes every output word exactly once, with no atomics.  Conventions and rejections as for
 * hsfft_mdct_batched, with nframes >= 1 and n equal to the length above.
 * Scratch: the same buffers.  Whole rows are walked in chunks of HSFFT_MDCT_CHUNK_MB / (nframes x N
 * x 8) rows, at least one, halved while the allocation fails; one row larger than the knob still
 * runs as one chunk. */
int hsfft_imdct_batched(const fft_type *d_X, int nframes, const fft_type *d_w, int N, int pad, fft_type *d_out, int n,
                        int batch);

/* --- batched chirp-z transform (zoom FFT) of real and complex rows -------------------------- */
/* m bins at any spacing df, starting at any frequency f0 (doubles, in cycles per sample), of a row
 * x of n samples, real or complex:
 *   X[k] = sum_{j<n} x[j] exp(-2 pi i j (f0 + k df)),   0 <= k < m
 * scipy.signal.zoom_fft(x, [f1, f2], m, fs) is f0 = f1/fs, df = (f2-f1)/(m fs); scipy.signal.czt(x, m, w,
 * a) on the unit circle is w = exp(-2 pi i df), a = exp(2 pi i f0); n = m, f0 = 0, df = 1/n is the
 * forward DFT.  Bluestein's algorithm: the unchanged c2c row transforms of the power-of-two length L
 * with one new kernel before, one between and one after.  Spiral contours (|w| or |a| other than 1),
 * an inverse and 2D are out of scope.
 * Sizes only, no device touched: L = max(2, the power of two >= n + m - 1); L may be NULL.
 * HSFFT_ERR_ARG with a message unless n >= 1, m >= 1 and n + m - 1 <= 2^26 (every j < max(n, m) then
 * has j*j exact in a double). */
int hsfft_czt_shape(int n, int m, int *L);
/* Host only, no device touched: the K = max(n, m) chirp words and the n input-rotation words the
 * calls below use, each (c, s) from one libm sincos(PI2 * (0.5 * ph), &s, &c).  The phase ph, in
 * half-turns, comes from this reduction, which is part of the contract:
 *   red(a, b):  p = a*b (rounded);  e = fma(a, b, -p) (the product's exact error);
 *               return fmod(p, 2.0) + e          (fmod is exact; one rounded add)
 *   h_chirp[j]: ph = red((double)j*(double)j, df)                               0 <= j < K
 *   h_pre[j]:   ph = red((double)(2*j), f0) + red((double)j*(double)j, df)      0 <= j < n
 * so the phase j*j*df, which in plain double loses bits as j grows, keeps its full precision modulo
 * one turn; with f0 == 0, h_pre[j] equals h_chirp[j] bit for bit.  Either pointer may be NULL and is
 * then skipped.  HSFFT_ERR_ARG with a message for what hsfft_czt_shape rejects and for an f0 or df
 * that is not finite or above 1 in magnitude (frequencies are periodic: callers reduce them). */
int hsfft_czt_tables(int n, int m, double f0, double df, fft_data *h_pre, fft_data *h_chirp);
/* d_in: batch contiguous rows of n complex (hsfft_czt_batched) or n reals (hsfft_czt_real_batched);
 * d_out: batch rows of m complex.  The contract is compositional and bit-exact.  With f = fft_init(L,
 * 1) and g = fft_init(L, -1) from the convolution plan cache (they follow the calling thread's
 * twiddle mode) and (c, s) table words of hsfft_czt_tables, per row:
 *   u[j] = (x.re*c + x.im*s, x.im*c - x.re*s) with (c, s) = pre[j], j < n;  (+0.0, +0.0) for n <= j < L
 *          real input: u[j] = (x*c, -(x*s)), the minus a flip of the sign bit: two multiplies, no add
 *   v[i] = chirp[i] for i < m;  v[L-j] = chirp[j] for 1 <= j < n;  (+0.0, +0.0) elsewhere
 *   V    = the reference's fft_exec(f) on v -- once per (n, m, f0, df, twiddle mode), not per row
 *   U    = the reference's fft_exec(f) on u
 *   P[i] = (U.re*V.re - U.im*V.im, U.re*V.im + U.im*V.re)
 *   y    = the reference's fft_exec(g) on P
 *   d    = (y[k].re / (double)L, y[k].im / (double)L)
 *   X[k] = (d.re*c + d.im*s, d.im*c - d.re*s) with (c, s) = chirp[k],  k < m
 * every multiply, add, subtract and divide rounded on its own and computed for every index with no
 * special case.  Where two NaN terms meet in one add, the payload is not part of the contract;
 * everything else is.
 * Asynchronous on the library stream under the device lock; the input is never written; every
 * output word is written exactly once and none is read; caller rows need the alignment of a
 * double only.  Returns 0 on success and for batch == 0.  HSFFT_ERR_ARG with a message -- before any
 * device is touched -- for what hsfft_czt_shape or hsfft_czt_tables rejects, NULL pointers, batch < 0,
 * n x batch, m x batch or L x batch above 2^40, or input and output byte ranges that overlap (each
 * with its own element size).
 * Scratch: the two pool buffers of hsfft_dct_batched, L complex per row each, no allocation per
 * call.  Rows are walked in chunks of HSFFT_CZT_CHUNK_MB / (2 x L x 16) rows (default 1024 MiB, at
 * least 1, read per call), at least one, halved while the allocation fails; HSFFT_ERR_NOMEM if one
 * row still fails.  pre, chirp, v and V are cached on the device, four (n, m, f0, df, twiddle mode)
 * per device, the least recently used one replaced: a transform not in the cache builds its tables
 * on the host, uploads them synchronously and runs the one transform of v before the first row. */
int hsfft_czt_batched(const fft_data *d_in, int n, fft_data *d_out, int m, double f0, double df, int batch);
int hsfft_czt_real_batched(const fft_type *d_in, int n, fft_data *d_out, int m, double f0, double df, int batch);

/* --- batched analytic signal (Hilbert) and Fourier resampling of real rows ----------------- */
/* scipy.signal.hilbert(x) = x + i H[x], and scipy.signal.resample(x, m): the sample count of a row
 * changed from n to m by truncating or zero-extending its spectrum.  Both are the unchanged r2c row
 * transform of length n, one new kernel that edits the compact spectrum, and the unchanged inverse
 * row transform -- c2c of n words, or c2r of m reals -- which writes straight into d_out; the edit is
 * not fused into a transform pass.  n and m are even, from 2 to 2^30 (the limit of hsfft_dct_batched;
 * the row transforms have no lower one): a real plan needs an even length.  Odd lengths, a window
 * in the frequency domain, complex rows and other axes are out of scope.
 * The contract is compositional and bit-exact.  With f = fft_real_init(n, 1), S = the n/2+1 compact
 * bins of the reference's fft_r2c_exec(f) on the row -- the words hsfft_r2c_batched_compact writes --
 * and q(a) = a / (double)n applied per component, one correctly rounded IEEE division (not a
 * multiply by a reciprocal):
 * hsfft_hilbert_batched, d_in: batch rows of n reals, d_out: batch rows of n complex:
 *   Z[0] = q(S[0]);  Z[k] = q(S[k] + S[k]) for 0 < k < n/2 (the add per component, before the
 *   division);  Z[n/2] = q(S[n/2]);  Z[k] = (+0.0, +0.0) for n/2 < k < n;  with n == 2 there is no
 *   doubled bin,
 *   out = the reference's fft_exec(fft_init(n, -1)) on Z: n complex words, unnormalised -- the scale
 *   already sits in q.
 * hsfft_resample_batched, d_in: batch rows of n reals, d_out: batch rows of m reals, K = min(n, m)/2:
 *   Y[k] = q(S[k]) for k < K,
 *   Y[K] = q(S[K]) where m == n;  q(0.5 * S[K]) per component where m > n;  (q(S[K].re + S[K].re),
 *   +0.0) where m < n: the imaginary part of the folded bin is +0.0, not a copy -- the reference's
 *   c2r reads that word --
 *   Y[k] = (+0.0, +0.0) for K < k <= m/2,
 *   out = the reference's fft_c2r_exec(fft_real_init(m, -1)) on Y (it reads bins 0..m/2, here at
 *   pitch m/2+1): m reals.  This is scipy's resample(x, m); its factor m/n already sits in q.
 * Infinite and NaN bins propagate by the IEEE rules (the reference's r2c already returns an infinite
 * bin where S + S would overflow); 0.5 * S and q round subnormals; everything is computed for every
 * index with no special case.  Where a NaN meets arithmetic, its payload is not part of the contract.
 * The plans come from the convolution plan cache -- the real plan pairs of n and of m, the c2c pair
 * of n -- so results follow the calling thread's twiddle mode, and a repeated length builds nothing.
 * Accuracy is that of the row transforms: full on powers of two; about 1e-11 in the exact mode on
 * lengths with factors 3, 5 or 7; in the default (reference) mode lengths such as 6 and 12 give the
 * reference's twiddle-quirk results (hsfft_set_twiddle_mode above), which are far from the
 * definition.  The bit-exact contract holds at every even length regardless.  Bluestein inner
 * lengths keep the error-word contract of hsfft_exec_batched (below).
 * Alignment: the row transforms read d_in and write d_out directly, in 16-byte words, as
 * hsfft_r2c_batched_compact, hsfft_exec_batched and hsfft_c2r_batched do with their buffers (a real
 * row is read and written as n/2 complex words).  d_in and d_out must therefore be 16-byte aligned,
 * as every hsfft_malloc'd pointer is; rows are n x 8, n x 16 or m x 8 bytes with n and m even, so
 * every row then is.  A pointer that is not is rejected; there is no 8-byte path.
 * Asynchronous on the library stream under the device lock; the input is never written; every
 * output word is written exactly once.  Returns 0 on success and for batch == 0.  HSFFT_ERR_ARG
 * with a message -- before any device is touched -- for NULL pointers, batch < 0, n or m odd, below 2
 * or above 2^30, n x batch or m x batch above 2^40, a d_in or d_out that is not 16-byte aligned, or
 * input and output byte ranges that overlap at all (each with its own element size).
 * Scratch: the two pool buffers of hsfft_dct_batched, no allocation per call: the compact spectra,
 * and the edited spectra that the inverse transform reads.  Rows are walked in chunks of
 * HSFFT_SPECTRAL_CHUNK_MB / (16 x (n/2+1) + 16 x n) rows for hsfft_hilbert_batched and
 * HSFFT_SPECTRAL_CHUNK_MB / (16 x (n/2+1) + 16 x (m/2+1)) rows for hsfft_resample_batched
 * (HSFFT_SPECTRAL_CHUNK_MB: default 1024 MiB, at least 1, read per call), at least one and at most
 * the batch, halved while the allocation fails; HSFFT_ERR_NOMEM if one row still fails. */
int hsfft_hilbert_batched(const fft_type *d_in, fft_data *d_out, int n, int batch);
int hsfft_resample_batched(const fft_type *d_in, int n, fft_type *d_out, int m, int batch);
/* Host only, no device touched: the rows of one chunk by the rule above, before the clamp to the
 * batch, into *rows (NULL is skipped); m == 0 asks for hsfft_hilbert_batched.  HSFFT_ERR_ARG with a
 * message for an n or a non-zero m that is odd, below 2 or above 2^30. */
int hsfft_spectral_chunk_rows(int n, int m, long long *rows);

/* --- synthetic data and timing (benchmark support) ------------------------------------- */
/* x[j] = (u(2(offset+j)), u(2(offset+j)+1)), u(i) = splitmix64(seed ^ i) -> [-1, 1) */
int hsfft_fill_complex(fft_data *d_x, int64_t count, uint64_t seed, uint64_t offset);
int hsfft_fill_real(fft_type *d_x, int64_t count, uint64_t seed, uint64_t offset);
/* Runs hsfft_exec_batched `iters` times between HIP events on the library stream and
 * returns the total milliseconds in *ms; per-pass average kernel milliseconds (measured
 * with events around each pass, one extra instrumented iteration) go to pass_ms[0..npass) */
int hsfft_time_batched(fft_object obj, const fft_data *d_in, fft_data *d_out, int batch,
                       int iters, float *ms, float *pass_ms, int max_pass);
int hsfft_time_r2c_batched(fft_real_object obj, const fft_type *d_in, fft_data *d_out,
                           int batch, int iters, float *ms);
/* The drop-in fft_exec on HOST buffers timed in a C loop, as the reference is timed (BASELINE
 * config 1): `warmup` calls per thread in warm-up threads that then exit, then `nthreads`
 * (1..64) fresh threads start together and each make `iters` back-to-back fft_exec calls on
 * `obj` with a private copy of `in` (N complex).  us[0..2]: median, p10 and p90 of thread 0's
 * per-call latency (microseconds); us[3]: the timed region's wall time / (nthreads x iters),
 * i.e. microseconds per transform in aggregate.  `out` receives thread 0's last output. */
int hsfft_time_exec_host(fft_object obj, const fft_data *in, fft_data *out, int nthreads,
                         int iters, int warmup, double *us);

/* Number of 8-byte words that differ between two device buffers of `bytes` bytes (a multiple
 * of 8) into *count; synchronous.  For whole-output comparisons between schedules (tests). */
int hsfft_count_diff_words(const void *d_a, const void *d_b, size_t bytes, uint64_t *count);

/* Stream-copy reference: `iters` device copies of `bytes` (multiple of 16) from d_src to
 * d_dst, event-timed; the practical HBM ceiling reported next to the FFT numbers. */
int hsfft_bench_copy(const void *d_src, void *d_dst, size_t bytes, int iters, float *ms);
/* The last step of hsfft_r2c_2d_full alone, event-timed (`iters` launches after one warm-up, total
 * milliseconds in *ms): batch transposed half spectra d_in[b][k1][k0] ((n1/2+1) x n0) to the full
 * layout d_out[b][k0][k1] (n0 x n1), mirror half included.  n1 even, batch >= 1. */
int hsfft_bench_transpose_herm(const fft_data *d_in, fft_data *d_out, int n0, int n1, int batch, int iters, float *ms);
/* Bluestein M = 2^18 (e.g. N = 99991) runs as one persistent launch whose workgroups must all
 * be resident at once; the library checks that with the occupancy API before launching, and a
 * grid that cannot be co-resident runs on the three-launch path at once (same results, more
 * time).  Its in-launch waits keep a last-resort bound (~1.3 s without progress):
 *   - synchronous entry points (fft_exec, fft_r2c_exec / fft_c2r_exec, hsfft_exec_multi) wait
 *     for the launch and re-run the rows of a launch whose waits timed out on the three-launch
 *     path themselves; hsfft_exec_batched_host keeps its launches asynchronous (uploads overlap
 *     transforms), checks its own error word once at the end and then re-runs the whole batch
 *     on the three-launch path;
 *   - asynchronous device-buffer calls (hsfft_exec_batched, hsfft_r2c_batched, ...) record a
 *     timed-out wait in an error word of the CALLING THREAD; it is reported exactly once, as
 *     HSFFT_ERR_DEVICE, by that thread's next hsfft_synchronize() on that device (or its next
 *     timing call, hsfft_time_*), and it means that thread's Bluestein outputs since its previous
 *     hsfft_synchronize() are invalid.  No other call consumes it or reports it: not a later
 *     call on another plan, not a scratch-pool growth, not another thread's hsfft_synchronize().
 *   HSFFT_BX_SYNC=1 makes every Bluestein call synchronous.
 * Count of calls whose rows ran on the three-launch path (refused grid or timed-out waits). */
long long hsfft_bluestein_fallbacks(void);

/* --- threading -------------------------------------------------------------------------
 * Every entry point is safe to call from several host threads at once, on shared or
 * distinct plans (the reference's mixed-radix fft_exec is reentrant, highSpeedFFT.c:1920).
 * Calls that run on the same device are serialised per call by a device lock (they share
 * the device's stream and scratch pool); calls on different devices run concurrently.
 * Freeing a plan while another thread still executes it remains a caller error.
 * A thread's own objects (the small host-buffer path's page-locked slots, completion word and
 * stream, its Bluestein error words) are recycled when it exits: they are parked per device and
 * the next thread to use that device takes them over (an exited thread's pending Bluestein error
 * is discarded, never passed on).  Nothing is created or destroyed on the exiting thread, where
 * the HIP runtime's per-thread state may already be gone, nor on a new thread's path; the parked
 * sets are destroyed by hsfft_release_scratch() and hsfft_finalize(). */

/* Per-thread streams created by the process so far (diagnostics: with threads recycled through
 * the pool, at most the number of threads that ever used the library AT ONCE, per device). */
long long hsfft_thread_streams_created(void);

/* --- multi-device (single process; one host thread per device, no collective) --------- */
/* Shards the batch contiguously over devices 0..ndev-1: h-side arrays of per-device
 * pointers d_in[g], d_out[g] each hold rows [g*batch/ndev, (g+1)*batch/ndev). */
int hsfft_exec_multi(fft_object obj, const fft_data *const *d_in, fft_data *const *d_out,
                     int batch, int ndev);

#ifdef __cplusplus
}
#endif

#endif /* HSFFT_GPU_H_ */
