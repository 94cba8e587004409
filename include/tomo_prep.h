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
 *   detector    the stripe detector the next two share, one z row at a time, in float64: the float32 factors f[x] (NaN and +inf read as
 *               FLT_MAX, -inf as -FLT_MAX) are sorted descending into d; nd = ndx / 4; a least-squares line through (i, d[i]),
 *               nd <= i < ndx - nd - 1, by the closed form with centred abscissae (xm the mean index, ym = sum d / count, slope
 *               m = sum (i - xm)(d[i] - ym) / sum (i - xm)^2, each sum in ascending i, intercept c = ym - m xm); t1 = c + m (ndx - 1),
 *               noise = max(|t1 - c|, 1e-6), v1 = |d[0] - c| / noise, v2 = |d[ndx - 1] - t1| / noise.  v1 >= snr masks every x with
 *               f[x] > c + (0.5 snr) noise; v2 >= snr masks every x with f[x] <= t1 - (0.5 snr) noise; the mask is then dilated by one
 *               column on each side.  8 <= ndx <= 8192 (one row of factors is sorted in LDS).
 *   large       large-stripe removal (Vo algorithm 5): the columns are sorted along the angles and the sorted rows median-filtered
 *               along x (window `size`) exactly as in `stripe`; nd = int(0.5 clip(drop_ratio, 0, 0.8) n_proj); over the ranks
 *               nd <= r < n_proj - nd, l1[x] and l2[x] are the float64 sums, in rank order, of the sorted and of the smoothed values,
 *               each divided by the count, and f[x] = l2 != 0 ? float32(l1 / l2) : 1.  The detector masks columns.  If norm, every
 *               value becomes s[a][x] / f[x] (IEEE float32 division); in a masked column it becomes the smoothed value at the rank the
 *               angle had in the sort (the paper re-sorts the normalised column; the ranks are the same whenever f > 0 and the division
 *               merges no two distinct values).
 *   dead        dead-stripe removal (Vo algorithm 6), n_proj >= 10: u[a][x] = float32(sum_{k = a-5 .. a+4} double(s[k][x]) / 10) with
 *               half-sample-symmetric reflection at the ends, diff[x] = float32(sum_a double(|s[a][x] - u[a][x]|)) in angle order, bck
 *               the reflected median of diff along x (window `size`), f = bck != 0 ? diff / bck : 1.  The detector masks columns; the
 *               first two and the last two columns are then cleared.  A masked column is interpolated along x at the same angle
 *               between the nearest unmasked columns xl < x < xr: s[xl] + (s[xr] - s[xl]) * (float(x - xl) / float(xr - xl)) in float32
 *               without contraction.  If norm, `large` (same snr and size, drop_ratio 0.1, norm) runs on the result.
 *   all         `dead` (la_size, norm) followed by `stripe` (sm_size), chunk by chunk on one scratch.
 *               large, dead and all share stripe's limits, chunk z with 10 bytes per value plus 13 bytes per (x, z) of scratch
 *               (tomo_prep_stripe_all_chunk), do not depend on the chunking, run on the caller's stream without a host round trip, and
 *               accept d_out == d_in.  A mask pointer is NULL or ndx * ndz bytes [x][z] that receive the detector's (dilated) mask.
 *   outlier     zinger removal and the 2-D median filter of a stack in[n][rows][cols] (cols fastest), uint16 or float32: raw frames
 *               [n][z][x] and the float32 sinogram (n, nx, nz) alike.  size is 3, 5 or 7; rows >= size and cols >= size.  Per pixel v:
 *               the window is the size x size values around it inside its own frame, with half-sample-symmetric reflection at the
 *               edges (d c b a | a b c d, as in `stripe`; one reflection suffices).  uint16 is ordered by value, float32 by the
 *               stripe sort's key (orderable bits, -0 read as +0, every NaN above +inf); med is the element of rank
 *               (size * size - 1) / 2 decoded from its key, so a median of -0 is written as +0 and a NaN median as 0x7fc00000.
 *               mode OUTLIER: d = float(v) - float(med), one IEEE float32 subtraction (exact for uint16); two_sided: d = fabsf(d);
 *               the pixel becomes med if d >= dif or if v is not finite (float32 only), else it keeps its bits.  dif >= 0 and not
 *               NaN; +inf only repairs non-finite pixels.  mode MEDIAN2D: every pixel becomes med; dif and two_sided are ignored.
 *               d_count: NULL, or n uint32 that the call clears on the stream and that receive, per frame, the pixels replaced
 *               (OUTLIER: those the test chose, whether or not med differs from v; MEDIAN2D: those whose bits changed), summed by
 *               integer atomics, so they are deterministic.  d_out == d_in is allowed: frames then go in batches
 *               (tomo_prep_outlier_batch) through handle-owned scratch bounded by max_scratch_bytes (0: no limit; never fewer than
 *               one frame), each batch filtered into the scratch and copied back on the same stream; the result does not depend on
 *               the batch.  Any other overlap is TOMO_PREP_ERR_ARG.  Everything runs on the caller's stream without a host round
 *               trip.  TOMO_PREP_ERR_ARG, with nothing launched: a dtype, mode or size other than the above, rows or cols below
 *               size, n < 1, rows * cols >= 2^31, a negative or NaN dif (OUTLIER), a NULL d_in or d_out.
 *
 * A handle owns one device, the scratch (of the stripe passes and of the in-place outlier call) and the last error; one handle is used by
 * one thread at a time.  Every entry point returns a tomo_prep_status and checks its arguments before it launches anything; on failure
 * tomo_prep_last_error(h) says why (h may be NULL for errors raised before a handle exists).
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
#define TOMO_PREP_MIN_STRIPE_NDX 8       /* large / dead / all: the detector's line fit needs a middle half */
#define TOMO_PREP_MAX_STRIPE_NDX 8192    /* large / dead / all: one row of factors is sorted in LDS */
#define TOMO_PREP_MIN_DEAD_NPROJ 10      /* dead / all: the 10-angle window */
#define TOMO_PREP_MAX_OUTLIER_SIZE 7     /* outlier: the window is 3, 5 or 7 on a side */

typedef enum {
    TOMO_PREP_OK = 0,
    TOMO_PREP_ERR_ARG = 1,          /* bad argument (shape, dtype, NULL pointer, window) */
    TOMO_PREP_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_PREP_ERR_NODEV = 3,        /* no HIP device */
    TOMO_PREP_ERR_UNSUPPORTED = 4   /* n_proj > TOMO_PREP_MAX_NPROJ, ndx > TOMO_PREP_MAX_STRIPE_NDX, or a median over more than 64 frames */
} tomo_prep_status;

typedef enum { TOMO_PREP_U16 = 0, TOMO_PREP_F32 = 1 } tomo_prep_dtype;
typedef enum { TOMO_PREP_MEAN = 0, TOMO_PREP_MEDIAN = 1 } tomo_prep_method;
typedef enum { TOMO_PREP_OUTLIER = 0, TOMO_PREP_MEDIAN2D = 1 } tomo_prep_outlier_mode;

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
/* The z rows per chunk of tomo_prep_stripe_large / _dead / _all (their scratch per z row is larger than the sorting pass's). */
TOMO_API int tomo_prep_stripe_all_chunk(int n_proj, int ndx, int ndz, size_t max_scratch_bytes, int *chunk_z);
/* Large-stripe removal.  snr > 0; size as in tomo_prep_stripe_sorting; d_mask: NULL or ndx * ndz bytes. */
TOMO_API int tomo_prep_stripe_large(tomo_prep *h, void *stream, const float *d_in, float *d_out, int n_proj, int ndx, int ndz, float snr,
                                    int size, float drop_ratio, int norm, size_t max_scratch_bytes, uint8_t *d_mask);
/* Dead-stripe removal.  d_mask_large (NULL or ndx * ndz bytes) receives the mask of the closing large-stripe pass when norm is set. */
TOMO_API int tomo_prep_stripe_dead(tomo_prep *h, void *stream, const float *d_in, float *d_out, int n_proj, int ndx, int ndz, float snr,
                                   int size, int norm, size_t max_scratch_bytes, uint8_t *d_mask, uint8_t *d_mask_large);
/* dead (la_size, norm) then sorting (sm_size). */
TOMO_API int tomo_prep_stripe_all(tomo_prep *h, void *stream, const float *d_in, float *d_out, int n_proj, int ndx, int ndz, float snr,
                                  int la_size, int sm_size, size_t max_scratch_bytes, uint8_t *d_mask_dead, uint8_t *d_mask_large);
/* The frames per batch the in-place tomo_prep_outlier uses for this shape and budget (how tests and benchmarks see the batching). */
TOMO_API int tomo_prep_outlier_batch(int rows, int cols, int dtype, int n, size_t max_scratch_bytes, int *frames);
/* Zinger removal (mode TOMO_PREP_OUTLIER) or the 2-D median filter (TOMO_PREP_MEDIAN2D) of d_in[n][rows][cols] into d_out (`outlier`
 * above).  d_count: NULL or n uint32. */
TOMO_API int tomo_prep_outlier(tomo_prep *h, void *stream, const void *d_in, void *d_out, int dtype, int n, int rows, int cols, int size,
                               int mode, float dif, int two_sided, size_t max_scratch_bytes, uint32_t *d_count);

#ifdef __cplusplus
}
#endif
#endif
