/*
 * libtomo_fbp.so -- the ramp filter of filtered back-projection on the GPU (gfx950): the device side of
 * tomography_alignment_amd/recon/fbp.py.  A separate library from libtomo_hip.so (include/tomo.h), so that the projector's kernel
 * sources stay untouched; it does not link libtomo_hip.so.  The back-projection is tomo_adjoint of include/tomo.h, on the same
 * stream (tomo_ctx_stream), so no host synchronisation separates the two.
 *
 * Sinogram: float32 p[n_proj][ndx][ndz], ndz fastest (include/tomo.h).  Each (projection, z) column of ndx values is zero-padded to
 * Npad = max(64, smallest power of two >= 2 ndx) and filtered on its own:
 *     q[ip][x][z] = scale[ip] * IDFT_Npad(H . DFT_Npad(pad(p[ip][.][z])))[x],   x < ndx
 * H is the real, even response table recon/fbp.py::filter_response computes in float64 (Npad/2 + 1 values, H[Npad - j] = H[j]).
 * ndx <= 4096 (Npad <= 8192: the FFT is held in LDS); larger widths are TOMO_FBP_ERR_UNSUPPORTED, with nothing launched.
 *
 * A handle owns one device, the twiddle and response tables, the device copy of the scales, and the last error; one handle is used
 * by one thread at a time.  Every entry point returns a tomo_fbp_status; on failure tomo_fbp_last_error(h) says why (h may be NULL
 * for errors raised before a handle exists).
 */
#ifndef TOMO_FBP_H
#define TOMO_FBP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_FBP_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_FBP_MAX_NDX 4096

typedef enum {
    TOMO_FBP_OK = 0,
    TOMO_FBP_ERR_ARG = 1,          /* bad argument (shape, NULL pointer, no response set for this ndx) */
    TOMO_FBP_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_FBP_ERR_NODEV = 3,        /* no HIP device */
    TOMO_FBP_ERR_UNSUPPORTED = 4   /* ndx > TOMO_FBP_MAX_NDX */
} tomo_fbp_status;

typedef struct tomo_fbp tomo_fbp;

TOMO_API int tomo_fbp_abi_version(void);
TOMO_API int tomo_fbp_create(int device, tomo_fbp **h);
TOMO_API int tomo_fbp_destroy(tomo_fbp *h);
TOMO_API const char *tomo_fbp_last_error(tomo_fbp *h);
/* The response for detector width ndx: table = H[0 .. Npad/2] (float64, host).  Replaces the previous one (after the work queued
 * with it has finished).  The table carries no length: exactly Npad/2 + 1 doubles are read, Npad = max(64, smallest power of two
 * >= 2 ndx), so the caller's table must hold that many (the Python binding checks it before the call). */
TOMO_API int tomo_fbp_set_response(tomo_fbp *h, int ndx, const double *table);
/* q = scale * filter(p) for n_proj projections of ndx x ndz, enqueued on `stream` (a hipStream_t; NULL: the null stream).
 * d_out may alias d_in (in place).  h_scale: n_proj float64 scales (host; copied before the call returns). */
TOMO_API int tomo_fbp_filter(tomo_fbp *h, void *stream, const float *d_in, float *d_out, int n_proj, int ndx, int ndz,
                             const double *h_scale);

#ifdef __cplusplus
}
#endif
#endif
