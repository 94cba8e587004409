/*
 * libtomo_cor.so -- the position of the rotation axis on the detector from a sinogram over [0, pi), by the Fourier-space metric of
 * Vo et al., Opt. Express 22 (2014) 19078 (gfx950): the device side of tomography_alignment_amd/rotation_axis.py.  A separate library
 * from libtomo_hip.so (include/tomo.h), like libtomo_fsc.so, so that the projector's kernel sources (and the hash that keys the
 * committed PMC counters) stay untouched; it links hipFFT and nothing of the package.  All work is enqueued on the caller-given stream
 * (in practice the tomo context's, tomo_ctx_stream); only the calls that hand values to the host (tomo_cor_metric, tomo_cor_debug_*)
 * wait for it.
 *
 * Definition (tests/cor_model.py is the same in numpy).  S[n][nx], float32: row i taken at phi0 + i pi / n.  A candidate is a real
 * column shift t; it stands for the axis offset t / 2 pixels from the detector centre (nx - 1) / 2.
 *   flip[i][j] = S[i][nx - 1 - j],  comp[i][j] = S[n - 1 - i][j].
 *   B_t[i][j]  = flip[i][j - t] for integer t (an exact copy); otherwise the cubic B-spline interpolant of the row flip[i] at
 *                x = j - t, coefficients from the mirror-boundary prefilter (pole sqrt(3) - 2, gain 6, the start of the causal
 *                recursion summed over the mirrored row), all in float64, rounded to float32 once.  Only the detector axis is filtered.
 *                The columns that wrapped -- j < ceil(t) for t >= 0, j >= nx + floor(t) for t < 0 -- are comp[i][j].
 *   M_t        = the rows of S, then the rows of B_t: R = 2 n rows of nx.
 *   mask       on the signed integer frequencies kv (rows) and ku (columns): w(kv) = ceil(|kv| dv / (radius du)),
 *                dv = (R - 1) / (2 pi R), du = 1 / nx, radius = 0.5 ratio nx;  W = 1 iff |ku| <= w(kv) and
 *                |kv| > min(drop, ceil(0.05 R)) and |ku| >= 2.  It is symmetric about DC, so the R2C half-spectrum suffices.
 *   m(t)       = sum W |FFT2(M_t)| / (R nx), on the half-spectrum with the Hermitian weight 2 (1 at ku = nx / 2 for even nx), float64.
 * The search over t (coarse integers, then a fine list about the coarse minimum) is the Python layer's; this library evaluates m for a
 * list of (slice, t) pairs.
 *
 * tomo_cor_load gathers the rows z of a device sinogram p[n_p][nx][nz] (z fastest) into contiguous S[slice][n][nx], angles first ..
 * first + n - 1, and computes the float64 spline coefficients of every flipped row once.  tomo_cor_metric builds M_t for a batch of
 * pairs straight into the padded in-place R2C buffer (rows of 2 (nx / 2 + 1) floats), transforms the batch with hipFFT and reduces
 * sum W |F| per pair: per-lane float64 sums, a fixed shuffle tree per work-group, and the work-groups' partial sums added in index order
 * -- no atomics, and a grid that depends on the shape only, so the same input gives the same bits.  A batch of b pairs needs
 * b 2 n (nx / 2 + 1) 8 bytes plus hipFFT's work area; b is the largest count for which both fit max_scratch_bytes (0: no limit; never
 * fewer than one pair).  Every pair is transformed on its own, so the result does not depend on b.  Plans are cached per (R, nx, b) and
 * share one work area, both owned by the handle, as are S, the coefficients and the batch buffer.
 *
 * TOMO_COR_ERR_UNSUPPORTED, before anything is allocated or launched: n < TOMO_COR_MIN_N, nx < TOMO_COR_MIN_NX,
 * nx > TOMO_COR_MAX_NX, 2 n > TOMO_COR_MAX_R, more than TOMO_COR_MAX_SLICES slices.
 *
 * A handle owns one device, its buffers and plans, and the last error; one handle is used by one thread at a time.  Every entry point
 * returns a tomo_cor_status and checks its arguments before it launches anything; on failure tomo_cor_last_error(h) says why (h may
 * be NULL for errors raised before a handle exists).
 */
#ifndef TOMO_COR_H
#define TOMO_COR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_COR_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_COR_MIN_N 8
#define TOMO_COR_MIN_NX 16
#define TOMO_COR_MAX_NX 8192     /* detector columns */
#define TOMO_COR_MAX_R 16384     /* rows of the stacked sinogram, 2 n */
#define TOMO_COR_MAX_SLICES 4096 /* detector rows of one load */

typedef enum {
    TOMO_COR_OK = 0,
    TOMO_COR_ERR_ARG = 1,          /* bad argument */
    TOMO_COR_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_COR_ERR_NODEV = 3,        /* no HIP device */
    TOMO_COR_ERR_UNSUPPORTED = 4,  /* a size the library does not handle */
    TOMO_COR_ERR_FFT = 5           /* a hipFFT call failed */
} tomo_cor_status;

/* indices of the pass_ms of tomo_cor_load and of tomo_cor_metric */
enum { TOMO_COR_MS_GATHER = 0, TOMO_COR_MS_PREFILTER = 1, TOMO_COR_LOAD_MS_N = 2 };
enum { TOMO_COR_MS_BUILD = 0, TOMO_COR_MS_R2C = 1, TOMO_COR_MS_REDUCE = 2, TOMO_COR_METRIC_MS_N = 3 };

typedef struct tomo_cor tomo_cor;

TOMO_API int tomo_cor_abi_version(void);
TOMO_API int tomo_cor_create(int device, tomo_cor **h);
TOMO_API int tomo_cor_destroy(tomo_cor *h);
TOMO_API const char *tomo_cor_last_error(tomo_cor *h);
/* TOMO_COR_ERR_UNSUPPORTED for a shape beyond the limits above; needs no handle or device. */
TOMO_API int tomo_cor_check_shape(int n, int nx, int nslices);
/* The mask as the reduction uses it, for the R = 2 n rows of the transform: hi[r] is the last column 2 <= ku <= hi[r] of the
 * half-spectrum that counts in row r (min(w(kv), nx / 2); 0 for a row that is cut).  Needs no handle or device. */
TOMO_API int tomo_cor_wedge(int n, int nx, double ratio, int drop, int *hi);
/* The pairs per batch under a scratch budget, before the work area is known (taken to be as large as the spectra; tomo_cor_metric
 * lowers the count if a plan asks for more).  Needs no handle or device. */
TOMO_API int tomo_cor_batch(int npairs, int n, int nx, size_t max_scratch_bytes, int *batch);
/* device bytes the handle holds between calls */
TOMO_API int tomo_cor_device_bytes(tomo_cor *h, int64_t *bytes);
/* host seconds spent making hipFFT plans since the handle was created */
TOMO_API int tomo_cor_plan_seconds(tomo_cor *h, double *seconds);
/* Gather + prefilter.  d_p: p[n_p][nx][nz] on the device; rows: nslices host ints in 0 .. nz - 1; the angles first .. first + n - 1
 * of p are taken.  pass_ms: NULL, or TOMO_COR_LOAD_MS_N floats (then the call waits for the stream).  Enqueues and returns. */
TOMO_API int tomo_cor_load(tomo_cor *h, void *stream, const float *d_p, int n_p, int nx, int nz, int first, int n, const int *rows,
                           int nslices, float *pass_ms);
/* m[k] = the metric of the pair (slice[k], t[k]), k < npairs, of the loaded sinograms; slice, t and m are host arrays.  Waits for the
 * stream.  pass_ms: NULL, or TOMO_COR_METRIC_MS_N floats, summed over the batches. */
TOMO_API int tomo_cor_metric(tomo_cor *h, void *stream, const int *slice, const double *t, int npairs, double ratio, int drop,
                             size_t max_scratch_bytes, double *m, float *pass_ms);
/* Debug entries for the tests: M_t of one pair as the build kernel writes it, without the row padding, into host out[2 n][nx]; the
 * gathered S[slice][n][nx] into host out[n][nx]; the spline coefficients of flip into host out[n][nx] doubles.  They wait. */
TOMO_API int tomo_cor_debug_build(tomo_cor *h, void *stream, int slice, double t, float *out);
TOMO_API int tomo_cor_debug_sinogram(tomo_cor *h, void *stream, int slice, float *out);
TOMO_API int tomo_cor_debug_coefficients(tomo_cor *h, void *stream, int slice, double *out);

#ifdef __cplusplus
}
#endif
#endif
