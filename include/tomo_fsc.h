/*
 * libtomo_fsc.so -- Fourier shell correlation (FSC) of two device-resident volumes, and its batched 2-D form, the Fourier ring
 * correlation (FRC) of two stacks of planes (gfx950): the device side of tomography_alignment_amd/resolution.py.  A separate library
 * from libtomo_hip.so (include/tomo.h), like libtomo_pyr.so, so that the projector's kernel sources (and the hash that keys the
 * committed PMC counters) stay untouched; it links hipFFT and nothing of the package.  Every operation is enqueued on the caller-given
 * stream (in practice the tomo context's, tomo_ctx_stream); only tomo_fsc_fetch, the download of the shell sums, synchronises.
 *
 * Layouts (include/tomo.h): a volume is float32 v[nx][ny][nz], a stack of planes float32 p[nb][nx][nz]; z is fastest.
 *
 *   set_shape   ndim 3: one volume (nb = 1); ndim 2: nb planes of (nx, nz) (ny = 1).  Makes (and keeps, per shape) the hipFFT R2C
 *               single-precision plan with its work area, and the two spectrum buffers.  The transform is IN PLACE in a padded buffer:
 *               rows of 2 (nz/2 + 1) floats become rows of nz/2 + 1 complex values, so a spectrum costs no real-valued copy beside it.
 *               TOMO_FSC_ERR_UNSUPPORTED, before anything is allocated or launched: an axis shorter than 2 or longer than
 *               TOMO_FSC_MAX_N, nb outside 1 ... TOMO_FSC_MAX_PLANES, ndim other than 2 or 3, more than 2^31 - 1 values.
 *   prepare     slot (0 or 1) <- (v - mean) * m, written into the padded FFT buffer.  m: none (1), a float32 device array (of the
 *               volume's shape; for ndim 2 of ONE plane's shape, applied to every plane), or the built-in soft sphere / disc: with d the
 *               distance of a voxel from the centre ((n - 1) / 2 on every axis), m = 1 for d <= R, 0 for d >= R + E and
 *               (1 + cos(pi (d - R) / E)) / 2 between, in float64.  mean (subtract_mean != 0): sum(m v) / sum(m), per plane for ndim 2,
 *               a two-stage float64 sum in a fixed order (256 block partials, then one fixed tree), 0 where sum(m) is 0.
 *   fft         the R2C transform of a slot, in place.
 *   reduce      the shell sums of the two spectra A (slot 0) and B (slot 1).  For a stored coefficient with integer frequencies
 *               (kx, ky, kz) -- x and y signed, 0 <= kz <= nz/2 -- r = sqrt(sum_i (k_i nmax / n_i)^2), nmax the longest axis, the shell is
 *               s = floor(r + 0.5), the Hermitian weight w = 1 on the planes kz = 0 and (nz even) kz = nz/2 and 2 elsewhere, and for
 *               s <= S - 1, S = min_i(n_i) / 2 + 1 shells:
 *                   C[s] += w Re(A conj B)    PA[s] += w |A|^2    PB[s] += w |B|^2    n[s] += w          (all float64)
 *               The shell index is exact: integer arithmetic where every nmax / n_i is an integer (r^2 is one then), float64 without
 *               contraction otherwise ((k_i nmax) / n_i, squares added in the order x, y, z, a correctly rounded sqrt).  The sums are
 *               deterministic: no float atomics; the same input gives the same bits (see tomo_fsc.hip).
 *   fetch       downloads the table, double out[nb][4][S] in the order C, PA, PB, n, and waits for it.
 *   take_rows   dst[i] = src[first + i * step], i < count, rows of row_elems floats: the even / odd projections of a device sinogram.
 *
 * A handle owns one device, its plans and buffers, and the last error; one handle is used by one thread at a time.  Every entry point
 * returns a tomo_fsc_status and checks its arguments before it launches anything; on failure tomo_fsc_last_error(h) says why (h may be
 * NULL for errors raised before a handle exists).
 */
#ifndef TOMO_FSC_H
#define TOMO_FSC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_FSC_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_FSC_MAX_N 2048          /* the longest axis: 4 (MAX_N / 2 + 1) float64 shell accumulators are 32 KiB of LDS */
#define TOMO_FSC_MAX_PLANES 65535    /* planes of one ndim-2 call: the y extent of a grid */

typedef enum {
    TOMO_FSC_OK = 0,
    TOMO_FSC_ERR_ARG = 1,          /* bad argument (NULL or misaligned pointer, slot, call before set_shape) */
    TOMO_FSC_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_FSC_ERR_NODEV = 3,        /* no HIP device */
    TOMO_FSC_ERR_UNSUPPORTED = 4,  /* a shape the library does not handle (see set_shape) */
    TOMO_FSC_ERR_FFT = 5           /* a hipFFT call failed */
} tomo_fsc_status;

typedef enum { TOMO_FSC_MASK_NONE = 0, TOMO_FSC_MASK_ARRAY = 1, TOMO_FSC_MASK_SPHERE = 2 } tomo_fsc_mask;

typedef struct tomo_fsc tomo_fsc;

TOMO_API int tomo_fsc_abi_version(void);
TOMO_API int tomo_fsc_create(int device, tomo_fsc **h);
TOMO_API int tomo_fsc_destroy(tomo_fsc *h);
TOMO_API const char *tomo_fsc_last_error(tomo_fsc *h);
/* S = min(n) / 2 + 1 of a shape (ny ignored for ndim 2); checks the shape as set_shape does, needs no handle or device. */
TOMO_API int tomo_fsc_n_shells(int ndim, int nb, int nx, int ny, int nz, int *n_shells);
TOMO_API int tomo_fsc_set_shape(tomo_fsc *h, int ndim, int nb, int nx, int ny, int nz);
/* device bytes the handle holds: spectra, hipFFT work areas, partial tables */
TOMO_API int tomo_fsc_device_bytes(tomo_fsc *h, int64_t *bytes);
/* host seconds spent making hipFFT plans since the handle was created */
TOMO_API int tomo_fsc_plan_seconds(tomo_fsc *h, double *seconds);
TOMO_API int tomo_fsc_prepare(tomo_fsc *h, void *stream, int slot, const float *d_vol, int mask, const float *d_mask, double radius,
                              double edge, int subtract_mean);
TOMO_API int tomo_fsc_fft(tomo_fsc *h, void *stream, int slot);
TOMO_API int tomo_fsc_reduce(tomo_fsc *h, void *stream);
TOMO_API int tomo_fsc_fetch(tomo_fsc *h, void *stream, double *out);
TOMO_API int tomo_fsc_take_rows(tomo_fsc *h, void *stream, const float *d_src, size_t row_elems, size_t first, size_t step, size_t count,
                                float *d_dst);

#ifdef __cplusplus
}
#endif
#endif
