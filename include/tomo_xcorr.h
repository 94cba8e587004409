/*
 * libtomo_xcorr.so -- cross-correlation pre-alignment on the GPU (gfx950): the device side of
 * tomography_alignment_amd/align/align_cc.py.  A separate library from libtomo_hip.so (include/tomo.h): it links hipFFT, and the
 * projector's kernel sources stay untouched.
 *
 * Images are C-ordered (nx, nz) planes, one after another.  dtype codes: 0 = float32, 1 = float64.  All arithmetic is float64.
 * A handle owns one device, one stream, the hipFFT plans (set to that stream) and the work buffers; one handle is used by one thread
 * at a time.  Every entry point returns a tomo_xcorr_status; on failure tomo_xcorr_last_error(h) says why (h may be NULL for errors
 * raised before a handle exists).
 */
#ifndef TOMO_XCORR_H
#define TOMO_XCORR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_XCORR_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

typedef enum {
    TOMO_XCORR_OK = 0,
    TOMO_XCORR_ERR_ARG = 1,       /* bad argument (shape, dtype, upsample factor, NULL pointer) */
    TOMO_XCORR_ERR_HIP = 2,       /* a HIP runtime call failed */
    TOMO_XCORR_ERR_FFT = 3,       /* a hipFFT call failed */
    TOMO_XCORR_ERR_NODEV = 4      /* no HIP device */
} tomo_xcorr_status;

typedef struct tomo_xcorr tomo_xcorr;

TOMO_API int tomo_xcorr_abi_version(void);
TOMO_API int tomo_xcorr_device_count(int *n);
TOMO_API int tomo_xcorr_create(int device, tomo_xcorr **h);
TOMO_API int tomo_xcorr_destroy(tomo_xcorr *h);
TOMO_API const char *tomo_xcorr_last_error(tomo_xcorr *h);
/* Device bytes this library holds right now, over all live handles (its own allocations; hipFFT's plan work areas excluded). */
TOMO_API int64_t tomo_xcorr_device_bytes(void);
/* Timings of the handle's last chain or batch call: [0] plan creation (host seconds, 0 when every plan was cached), [1] upload,
 * [2] the enqueued steps, [3] download (device-event milliseconds). */
TOMO_API int tomo_xcorr_last_timing(tomo_xcorr *h, double *t4);

/* The reference's cross_correlation_numpy chain: for i = 1..n-1, crossCorrelationAlign(aligned[i], aligned[i-1], rfilt, kfilt).
 * offsets (n x 2) receives the raw integer peak of each step (row 0 zero; no wrap); aligned (n planes of dtype) the rolled images.
 * rfilt, kfilt: (nx, nz) float64. */
TOMO_API int tomo_xcorr_chain_numpy(tomo_xcorr *h, const void *proj, int dtype, int n, int nx, int nz, const double *rfilt,
                                    const double *kfilt, double *offsets, void *aligned);
/* The reference's cross_correlation_skimage chain: for i = 1..n-1, s = pcc(aligned[i-1], aligned[i], upsample), aligned[i] =
 * ndimage.shift(aligned[i], s) (order 3, mode 'constant', cval 0), rounded to dtype.  offsets (n x 2) receives s per step. */
TOMO_API int tomo_xcorr_chain_skimage(tomo_xcorr *h, const void *proj, int dtype, int n, int nx, int nz, int upsample,
                                      double *offsets, void *aligned);
/* B independent phase cross-correlations of (refs[b], movs[b]), both (B, nx, nz) float64.  normalization: 1 = "phase", 0 = None.
 * shifts (B x 2), error (B), phasediff (B). */
TOMO_API int tomo_xcorr_pcc_batch(tomo_xcorr *h, const double *refs, const double *movs, int B, int nx, int nz, int upsample,
                                  int normalization, double *shifts, double *error, double *phasediff);
/* B images of dtype shifted by shifts (B x 2) as ndimage.shift(order=3, mode='constant', cval=0) does; out has the input dtype. */
TOMO_API int tomo_xcorr_spline_shift(tomo_xcorr *h, const void *img, int dtype, int B, int nx, int nz, const double *shifts,
                                     void *out);

#ifdef __cplusplus
}
#endif
#endif
