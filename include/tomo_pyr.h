/*
 * libtomo_pyr.so -- the device operations of a resolution pyramid (gfx950): the device side of tomography_alignment_amd/multires.py.
 * A separate library from libtomo_hip.so (include/tomo.h), like libtomo_prep.so, so that the projector's kernel sources (and the hash
 * that keys the committed PMC counters) stay untouched; it does not link libtomo_hip.so.  Every operation is enqueued on a caller-given
 * stream (in practice the tomo context's, tomo_ctx_stream) and none synchronises, so a level's data are ordered with the projector work
 * that reads them.
 *
 * Layouts (include/tomo.h): the sinogram is float32 p[n][nx][nz], a volume float32 v[nx][ny][nz]; z, the rotation axis, is fastest.
 *
 *   bin_sino     dst[i][X][Z] = float32(S * c):  S the float64 sum of src[i][f X + a][f Z + b], 0 <= a, b < f;  c = double(scale) / (f f).
 *   bin_vol      the same over the f x f x f cells of a volume, c = double(scale) / (f f f).
 *                f is 2, 4 or 8 and must divide every binned extent (TOMO_PYR_ERR_UNSUPPORTED otherwise, before any launch).  The sum is
 *                float64, so the result does not depend on the order of summation whenever the sum is exact.
 *   prolong_vol  coarse [nx][ny][nz] -> fine [2 nx][2 ny][2 nz], cell-centred trilinear interpolation: fine index i samples the coarse
 *                axis at (i + 0.5) / 2 - 0.5, i.e. 3/4 of coarse cell i / 2 and 1/4 of its neighbour on the side i lies on, the
 *                neighbour's index clamped to the axis (the outermost fine cell copies its coarse cell); separable, x then y then z,
 *                each step near + 0.25f * (far - near) in float32; times scale.
 *
 * src and dst are distinct buffers, both 16-byte aligned (every tomo_malloc'ed buffer is).  A handle owns one device and the last error;
 * one handle is used by one thread at a time.  Every entry point returns a tomo_pyr_status and checks its arguments before it launches
 * anything; on failure tomo_pyr_last_error(h) says why (h may be NULL for errors raised before a handle exists).
 */
#ifndef TOMO_PYR_H
#define TOMO_PYR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_PYR_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_PYR_MAX_FACTOR 8

typedef enum {
    TOMO_PYR_OK = 0,
    TOMO_PYR_ERR_ARG = 1,          /* bad argument (shape, NULL or misaligned pointer, overlapping buffers) */
    TOMO_PYR_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_PYR_ERR_NODEV = 3,        /* no HIP device */
    TOMO_PYR_ERR_UNSUPPORTED = 4   /* f not 2, 4 or 8, or an extent f does not divide */
} tomo_pyr_status;

typedef struct tomo_pyr tomo_pyr;

TOMO_API int tomo_pyr_abi_version(void);
TOMO_API int tomo_pyr_create(int device, tomo_pyr **h);
TOMO_API int tomo_pyr_destroy(tomo_pyr *h);
TOMO_API const char *tomo_pyr_last_error(tomo_pyr *h);
/* d_dst[n][nx / f][nz / f] from d_src[n][nx][nz]; n == 0 launches nothing. */
TOMO_API int tomo_pyr_bin_sino(tomo_pyr *h, void *stream, const float *d_src, int n, int nx, int nz, int f, float scale, float *d_dst);
/* d_dst[nx / f][ny / f][nz / f] from d_src[nx][ny][nz]. */
TOMO_API int tomo_pyr_bin_vol(tomo_pyr *h, void *stream, const float *d_src, int nx, int ny, int nz, int f, float scale, float *d_dst);
/* d_dst[2 nx][2 ny][2 nz] from the coarse d_src[nx][ny][nz]. */
TOMO_API int tomo_pyr_prolong_vol(tomo_pyr *h, void *stream, const float *d_src, int nx, int ny, int nz, float scale, float *d_dst);

#ifdef __cplusplus
}
#endif
#endif
