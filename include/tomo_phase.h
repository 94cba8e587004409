/*
 * libtomo_phase.so -- single-distance phase retrieval (Paganin et al., J. Microsc. 206 (2002)) of a device-resident stack of flat-field
 * corrected projections, and the -log that follows it (gfx950): the device side of tomography_alignment_amd/preprocess.py's
 * retrieve_phase and minus_log.  A separate library from libtomo_hip.so (include/tomo.h) and from libtomo_prep.so, like libtomo_fsc.so,
 * so that the projector's kernel sources (and the hash that keys the committed PMC counters) stay untouched; it links hipFFT and nothing
 * of the package.  All work is enqueued on the caller-given stream (in practice the tomo context's, tomo_ctx_stream);
 * tomo_phase_retrieve waits for it before it returns, because it frees its spectrum buffer.
 *
 * Input: the transmission T[n][nx][nz], float32, z fastest -- what tomo_prep_normalize writes with minus_log = 0.
 *
 * One dimensionless parameter, the strength a in pixels^2: a = pi lambda z (delta / beta) / pixel_size^2.
 *
 * Per projection, independently:
 *   1. pad    by edge replication to (Px, Pz).  P is the smallest EVEN length 2^i 3^j 5^k with P >= n_axis + 2 m; the data sits at
 *             offset (P - n_axis) / 2 (integer division).  m is the caller's (tomo_phase_retrieve's pad_x, pad_z); preprocess.py
 *             defaults it to min(n_axis, ceil(8 l)), l = sqrt(a) / (2 pi), the filter's real-space decay length.
 *   2. filter F = rfft2(padded); F[kx][kz] *= H, H = 1 / (1 + a ((kx / Px)^2 + (kz / Pz)^2)), kx the SIGNED frequency index
 *             (kx - Px for kx > Px / 2), 0 <= kz <= Pz / 2; r = irfft2(F), normalised so that a = 0 is the identity.  The DC gain
 *             is exactly 1.  The two per-axis terms Px Pz a (kx / Px)^2 and Px Pz (1 + a (kz / Pz)^2), which carry the transforms'
 *             normalisation, are tabulated on the host in float64; the kernel adds them in float64, rounds the sum to float32 once and
 *             multiplies by 1.0f / that sum, an IEEE float32 division.
 *   3. crop   back to (nx, nz); out = -log(fmax(r, min_ratio)) with minus_log, else out = r.
 * a = 0 is applied as what it is, the identity: no transform runs, and the result is bit for bit tomo_phase_minus_log's (minus_log) or
 * a copy.  d_out may be d_in (in place); otherwise the two must not overlap (not checked here; preprocess.py does).
 *
 * The transforms are hipFFT's batched in-place 2-D R2C / C2R (rows of 2 (Pz / 2 + 1) floats).  Frames are processed in batches: a batch
 * of b frames needs b Px (Pz / 2 + 1) 8 bytes of spectrum plus hipFFT's work area, and b is the largest count for which both fit
 * max_scratch_bytes (0: no limit; never fewer than one frame).  Every frame is transformed on its own, so the result does not depend
 * on b.  Plans are cached per (Px, Pz, b) and share one work area, both owned by the handle; the spectrum buffer is allocated by the call
 * and freed before it returns.
 *
 * TOMO_PHASE_ERR_UNSUPPORTED, before anything is allocated or launched: a padded axis longer than TOMO_PHASE_MAX_P (not at a = 0,
 * where nothing is padded).
 *
 * A handle owns one device, its plans, work area and tables, and the last error; one handle is used by one thread at a time.  Every
 * entry point returns a tomo_phase_status and checks its arguments before it launches anything; on failure tomo_phase_last_error(h)
 * says why (h may be NULL for errors raised before a handle exists).
 */
#ifndef TOMO_PHASE_H
#define TOMO_PHASE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_PHASE_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_PHASE_MAX_P 8192        /* the longest padded axis */
#define TOMO_PHASE_MAX_STRENGTH 1e12 /* a: far beyond any optics; keeps every table entry finite in float32 */

typedef enum {
    TOMO_PHASE_OK = 0,
    TOMO_PHASE_ERR_ARG = 1,          /* bad argument */
    TOMO_PHASE_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_PHASE_ERR_NODEV = 3,        /* no HIP device */
    TOMO_PHASE_ERR_UNSUPPORTED = 4,  /* a size the library does not handle */
    TOMO_PHASE_ERR_FFT = 5           /* a hipFFT call failed */
} tomo_phase_status;

/* indices of tomo_phase_retrieve's pass_ms */
enum { TOMO_PHASE_MS_PAD = 0, TOMO_PHASE_MS_R2C = 1, TOMO_PHASE_MS_FILTER = 2, TOMO_PHASE_MS_C2R = 3, TOMO_PHASE_MS_CROP = 4, TOMO_PHASE_MS_N = 5 };

typedef struct tomo_phase tomo_phase;

TOMO_API int tomo_phase_abi_version(void);
TOMO_API int tomo_phase_create(int device, tomo_phase **h);
TOMO_API int tomo_phase_destroy(tomo_phase *h);
TOMO_API const char *tomo_phase_last_error(tomo_phase *h);
/* The padded length of an axis of n values with m values of padding on each side; needs no handle or device. */
TOMO_API int tomo_phase_padded_length(int n, int m, int *padded);
/* The frames per batch of a padded shape under a scratch budget, before the work area is known (it is assumed to be as large as the
 * spectrum, which is what hipFFT asks for at most for these transforms; tomo_phase_retrieve lowers the count if a plan asks for more). */
TOMO_API int tomo_phase_batch(int n, int px, int pz, size_t max_scratch_bytes, int *batch);
/* device bytes the handle holds between calls: the hipFFT work area and the tables */
TOMO_API int tomo_phase_device_bytes(tomo_phase *h, int64_t *bytes);
/* the device's free and total memory (hipMemGetInfo): what a caller compares before and after a call to see that nothing stayed behind */
TOMO_API int tomo_phase_mem_info(tomo_phase *h, size_t *free_bytes, size_t *total_bytes);
/* host seconds spent making hipFFT plans since the handle was created */
TOMO_API int tomo_phase_plan_seconds(tomo_phase *h, double *seconds);
/* pass_ms: NULL, or TOMO_PHASE_MS_N floats that receive the device milliseconds of the five passes, summed over the batches. */
TOMO_API int tomo_phase_retrieve(tomo_phase *h, void *stream, const float *d_in, float *d_out, int n, int nx, int nz, double strength,
                                 int pad_x, int pad_z, int minus_log, float min_ratio, size_t max_scratch_bytes, float *pass_ms);
/* out = -log(fmax(in, min_ratio)); d_out may be d_in.  Enqueues and returns. */
TOMO_API int tomo_phase_minus_log(tomo_phase *h, void *stream, const float *d_in, float *d_out, size_t count, float min_ratio);

#ifdef __cplusplus
}
#endif
#endif
