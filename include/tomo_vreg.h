/*
 * libtomo_vreg.so -- registration of two device-resident volumes by a translation (gfx950): the 3-D phase / cross correlation with an
 * upsampled-DFT refinement of its peak, and the Fourier shift that applies the result; the device side of
 * tomography_alignment_amd/registration.py.  A separate library from libtomo_hip.so (include/tomo.h), like libtomo_fsc.so, so that the
 * projector's kernel sources (and the hash that keys the committed PMC counters) stay untouched; it links hipFFT and nothing of the
 * package.  Every operation is enqueued on the caller-given stream (in practice the tomo context's, tomo_ctx_stream); only
 * tomo_vreg_fetch and tomo_vreg_argmax synchronise.  tests/vreg_model.py is this text in numpy float64.
 *
 * Layout (include/tomo.h): a volume is float32 v[nx][ny][nz], z fastest.  N = nx ny nz.  Buffer offsets are 64-bit throughout: the
 * padded in-place buffer of a legal shape (rows of 2 (nz/2 + 1) floats) can exceed 2^31 floats.
 *
 *   set_shape   plans the single-precision R2C and C2R (hipFFT, in place) and allocates the two padded buffers (slot 0: the reference,
 *               slot 1: the moving volume) and the copy of P.  TOMO_VREG_ERR_UNSUPPORTED, before anything is allocated or launched: an
 *               axis shorter than 2 or longer than TOMO_VREG_MAX_N, more than 2^31 - 1 values.
 *   prepare     slot <- a = float32((v - mean) m), written into the padded buffer, the pad of every row as zeros.  The mask m and the mean
 *               are those of include/tomo_fsc.h: m is none (1), a float32 device array of the volume's shape, or the soft sphere: with d
 *               the distance of a voxel from the centre ((n - 1) / 2 on every axis), m = 1 for d <= R, 0 for d >= R + E and
 *               (1 + cos(pi (d - R) / E)) / 2 between, in float64.  mean (subtract_mean != 0): sum(m v) / sum(m), a two-stage float64 sum
 *               in a fixed order (256 block partials, then one fixed tree), 0 where sum(m) is 0.  Also E[slot] = sum a^2, a float64 sum
 *               of the float32 values written: one partial per work-group, the partials added in a fixed order, no atomics.
 *   correlate   the R2C of both slots; P = A conj(B) (A: slot 0) written over slot 0 and to the copy; with TOMO_VREG_NORM_PHASE
 *               P / |P| in float32, 0 where |P| = 0.  Then the C2R of slot 0, and the coarse peak: the largest element of it over the
 *               real (unpadded) elements by the rule of argmax below.  c = C2R(P) / N: the peak's value is the float32 element as a
 *               double, divided by N.  Index i on an axis of length n is the shift i if i <= n / 2 (integer division), else i - n.
 *   refine      upsample u = 1 ... TOMO_VREG_MAX_UPSAMPLE.  u = 1: the coarse peak stands.  Otherwise U = ceil(1.5 u), h = U / 2 (integer
 *               division), per axis the candidates d_j = s0 + (j - h) / u, j < U, about the coarse shift s0, and
 *                   c_u(jx, jy, jz) = (1 / N) sum_k w_k Re( P_k exp(2 pi i (kx dx / nx + ky dy / ny + kz dz / nz)) )
 *               over the stored coefficients of the copy of P: kx, ky signed in fftfreq's convention (Nyquist is -n/2), 0 <= kz <= nz/2,
 *               w = 1 on the planes kz = 0 and (nz even) kz = nz/2 and 2 elsewhere.  The phase of a factor is exact:
 *               r = (k (s0 u + j - h)) mod (n u) in int64, 0 <= r < n u, the angle 2 pi r / (n u) in float64.  Products and sums are
 *               float64 in a fixed order (z, then y, then x, each in increasing index of the stored coefficient); P stays the complex64
 *               the transform left.  The largest of the U^3 values wins, a tie goes to the smallest flat index (jx U + jy) U + jz; the
 *               shift is s0 + (j - h) / u per axis, in float64.  The scratch of the z contraction is cut into slabs of kx planes that fit
 *               set_scratch_bytes (default 1 GiB, never less than one plane); the slabs change no bit of the result.
 *               refine reads the copy of P, which shift overwrites: it follows correlate.
 *   fetch       double out[8]: shift[3], peak (the winning c or c_u), E[0], E[1], the coarse flat index (ix ny + iy) nz + iz, u.  Waits.
 *   shift       dst = C2R( R2C(src) prod_i phi_i(k_i) / N ), phi_i(k) = exp(-2 pi i k s_i / n_i) for signed k, evaluated in float64 (the
 *               angle -2 pi (k s_i / n_i)); on an even axis at |k| = n_i / 2 the factor is the real cos(pi s_i).  The product of the three
 *               factors, the coefficient and 1 / N is formed in float64 and rounded to float32 once.  If all three s_i are integers the
 *               result is the circular roll dst[(i + s) mod n] = src[i] on every axis, by a copy kernel, bit for bit, no transform.
 *               dst may be src; any other overlap is TOMO_VREG_ERR_ARG.  Uses the copy of P as its work buffer.
 *   argmax      the reduction of correlate on a caller's float32 volume of the shape set: the flat index and value of the largest
 *               element.  NaN never wins; a tie goes to the smallest flat index; a volume of NaN only gives index 0 and NaN.  Two
 *               stages -- (value, index) pairs through a shuffle tree in a wave, the waves in order, one partial per work-group, one
 *               work-group folds the partials -- whose result does not depend on the grid.  Waits.
 *
 * A handle owns one device, its plans and buffers, and the last error; one handle is used by one thread at a time.  Every entry point
 * returns a tomo_vreg_status and checks its arguments before it launches anything; on failure tomo_vreg_last_error(h) says why (h may
 * be NULL for errors raised before a handle exists).
 */
#ifndef TOMO_VREG_H
#define TOMO_VREG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_VREG_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_VREG_MAX_N 2048         /* the longest axis */
#define TOMO_VREG_MAX_UPSAMPLE 100   /* u; U = ceil(1.5 u) <= 150 candidates an axis */

typedef enum {
    TOMO_VREG_OK = 0,
    TOMO_VREG_ERR_ARG = 1,          /* bad argument (NULL pointer, slot, overlap, call before set_shape) */
    TOMO_VREG_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_VREG_ERR_NODEV = 3,        /* no HIP device */
    TOMO_VREG_ERR_UNSUPPORTED = 4,  /* a shape or an upsampling the library does not handle */
    TOMO_VREG_ERR_FFT = 5           /* a hipFFT call failed */
} tomo_vreg_status;

typedef enum { TOMO_VREG_MASK_NONE = 0, TOMO_VREG_MASK_ARRAY = 1, TOMO_VREG_MASK_SPHERE = 2 } tomo_vreg_mask;
typedef enum { TOMO_VREG_NORM_NONE = 0, TOMO_VREG_NORM_PHASE = 1 } tomo_vreg_norm;

typedef struct tomo_vreg tomo_vreg;

TOMO_API int tomo_vreg_abi_version(void);
TOMO_API int tomo_vreg_create(int device, tomo_vreg **h);
TOMO_API int tomo_vreg_destroy(tomo_vreg *h);
TOMO_API const char *tomo_vreg_last_error(tomo_vreg *h);
/* checks a shape (and u, unless 0 is given for "no refinement asked") as set_shape and refine do; needs no handle or device */
TOMO_API int tomo_vreg_check(int nx, int ny, int nz, int upsample);
TOMO_API int tomo_vreg_set_shape(tomo_vreg *h, int nx, int ny, int nz);
/* device bytes the handle holds: the padded buffers, the copy of P, hipFFT work areas, tables and scratch */
TOMO_API int tomo_vreg_device_bytes(tomo_vreg *h, int64_t *bytes);
/* host seconds spent making hipFFT plans since the handle was created */
TOMO_API int tomo_vreg_plan_seconds(tomo_vreg *h, double *seconds);
/* the budget of refine's z-contraction scratch; 0: the default, 1 GiB */
TOMO_API int tomo_vreg_set_scratch_bytes(tomo_vreg *h, size_t bytes);
TOMO_API int tomo_vreg_prepare(tomo_vreg *h, void *stream, int slot, const float *d_vol, int mask, const float *d_mask, double radius,
                               double edge, int subtract_mean);
TOMO_API int tomo_vreg_correlate(tomo_vreg *h, void *stream, int normalization);
TOMO_API int tomo_vreg_refine(tomo_vreg *h, void *stream, int upsample);
TOMO_API int tomo_vreg_fetch(tomo_vreg *h, void *stream, double *out8);
TOMO_API int tomo_vreg_shift(tomo_vreg *h, void *stream, const float *d_src, const double *s3, float *d_dst);
TOMO_API int tomo_vreg_argmax(tomo_vreg *h, void *stream, const float *d_vol, int64_t *index, float *value);

#ifdef __cplusplus
}
#endif
#endif
