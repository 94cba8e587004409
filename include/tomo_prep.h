/*
 * libtomo_prep.so -- preprocessing of raw detector frames on the GPU (gfx950): the device side of tomography_alignment_amd/preprocess.py.
 * A separate library from libtomo_hip.so (include/tomo.h), so that the projector's kernel sources (and the hash that keys the committed
 * PMC counters) stay untouched; it does not link libtomo_hip.so.  Every operation is enqueued on a caller-given stream (in practice the
 * tomo context's, tomo_ctx_stream), so the sinogram it writes is ordered with the projector work that reads it.
 *
 * Layouts: raw frames, flats and darks are [n][rows = z][cols = x] (x fastest), uint16 or float32; the sinogram is float32
 * p[n_proj][ndx][ndz] (z, the rotation axis, fastest: include/tomo.h).
 *
 *   reference   one float32 frame from n frames: mean (float64 sum in frame order, / n, rounded once) or median (n <= 64; exact
 *               selection; for even n float32(0.5 * (double(a) + double(b))) of the two middle values).
 *   normalize   out[i][x - x0][z - z0] = f(raw[i][z][x]) over the window z0:z1, x0:x1, with
 *                   den = flat - dark;  den = den < 1e-6f ? 1e-6f : den;  r = (float(raw) - dark) / den   (IEEE division)
 *                   r = use_cutoff ? fminf(r, cutoff) : r;   out = minus_log ? -logf(fmaxf(r, min_ratio)) : r
 *   stripe      sorting-based stripe removal (Vo, Atwood & Drakopoulos 2018, algorithm 3): per detector row z, each column (x, z) is
 *               sorted along the angles by the key (orderable bits of v with -0 -> +0 and every NaN above +inf, angle index); the
 *               sorted rows are median-filtered along x at equal rank (odd window `size`, half-sample-symmetric reflection) and put back
 *               at the angles they came from.  n_proj <= TOMO_PREP_MAX_NPROJ, 3 <= size <= min(ndx, 63), size odd.  z is processed in
 *               chunks whose scratch (10 bytes per sinogram value of the chunk) fits max_scratch_bytes (0: no limit); the result does not
 *               depend on the chunking.  d_out may alias d_in; partial overlap is not allowed.
 *
 * A handle owns one device, the stripe scratch and the last error; one handle is used by one thread at a time.  Every entry point returns
 * a tomo_prep_status and checks its arguments before it launches anything; on failure tomo_prep_last_error(h) says why (h may be NULL
 * for errors raised before a handle exists).
 */
#ifndef TOMO_PREP_H
#define TOMO_PREP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_PREP_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_PREP_MAX_NPROJ 8192         /* one 64-bit sort key per angle in LDS */
#define TOMO_PREP_MAX_MEDIAN_FRAMES 64   /* reference frames by median */
#define TOMO_PREP_MAX_STRIPE_SIZE 63

typedef enum {
    TOMO_PREP_OK = 0,
    TOMO_PREP_ERR_ARG = 1,          /* bad argument (shape, dtype, NULL pointer, window) */
    TOMO_PREP_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_PREP_ERR_NODEV = 3,        /* no HIP device */
    TOMO_PREP_ERR_UNSUPPORTED = 4   /* n_proj > TOMO_PREP_MAX_NPROJ, or a median over more than 64 frames */
} tomo_prep_status;

typedef enum { TOMO_PREP_U16 = 0, TOMO_PREP_F32 = 1 } tomo_prep_dtype;
typedef enum { TOMO_PREP_MEAN = 0, TOMO_PREP_MEDIAN = 1 } tomo_prep_method;

typedef struct tomo_prep tomo_prep;

TOMO_API int tomo_prep_abi_version(void);
TOMO_API int tomo_prep_create(int device, tomo_prep **h);
TOMO_API int tomo_prep_destroy(tomo_prep *h);
TOMO_API const char *tomo_prep_last_error(tomo_prep *h);
/* d_out[rows][cols] = reduce(d_frames[n][rows][cols]) by `method`; n >= 1. */
TOMO_API int tomo_prep_reference(tomo_prep *h, void *stream, const void *d_frames, int dtype, int n, int rows, int cols, int method,
                                 float *d_out);
/* d_out[n][x1 - x0][z1 - z0] from d_raw[n][rows][cols] and the float32 reference frames d_flat, d_dark [rows][cols];
 * 0 <= z0 < z1 <= rows, 0 <= x0 < x1 <= cols. */
TOMO_API int tomo_prep_normalize(tomo_prep *h, void *stream, const void *d_raw, int dtype, int n, int rows, int cols, const float *d_flat,
                                 const float *d_dark, int z0, int z1, int x0, int x1, int use_cutoff, float cutoff, int minus_log,
                                 float min_ratio, float *d_out);
/* The z columns per chunk the stripe removal uses for this shape and budget (how tests and benchmarks see the chunking). */
TOMO_API int tomo_prep_stripe_chunk(int n_proj, int ndx, int ndz, size_t max_scratch_bytes, int *chunk_z);
/* Stripe removal of d_in[n_proj][ndx][ndz] into d_out.  pass_ms: NULL, or 3 floats that receive the device time of the sort, the median
 * and the scatter passes summed over the chunks -- the call then synchronises the stream (benchmarks only). */
TOMO_API int tomo_prep_stripe_sorting(tomo_prep *h, void *stream, const float *d_in, float *d_out, int n_proj, int ndx, int ndz, int size,
                                      size_t max_scratch_bytes, float *pass_ms);

#ifdef __cplusplus
}
#endif
#endif
