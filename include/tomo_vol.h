/*
 * libtomo_vol.so -- what happens to a reconstructed volume before it leaves the device (gfx950): statistics, the grey-value histogram,
 * the conversion to 8 or 16 bit (in place of layout or as the stack of z slices that viewers read), the blanking outside the
 * reconstruction cylinder, minimum / maximum projections and single planes.  The device side of tomography_alignment_amd/postprocess.py.
 * A separate library from libtomo_hip.so (include/tomo.h), like libtomo_mom.so, so that the projector's kernel sources (and the hash
 * that keys the committed PMC counters) stay untouched; it links nothing of the package and no FFT.
 *
 * Definitions (tests/vol_model.py is the same in numpy).  v[nx][ny][nz], float32, z fastest: the layout of every operator; any 3-D
 * float32 array qualifies.  All offsets and counts are 64-bit.
 *
 *   region     R4 < 0: everything.  R4 >= 0: the cylinder about the z axis; voxel (x, y, .) is inside iff
 *              (2x - nx + 1)^2 + (2y - ny + 1)^2 <= R4 in int64 (the host passes R4 = floor((ratio min(nx, ny))^2)).
 *   stats      over the region: n_finite, n_nonfinite (NaN, +-inf), min and max of the finite values (NaN when there are none), sum and
 *              sumsq of the finite values in float64.  The sums are taken in an order that depends on (nx, ny, nz) only; no float atomics.
 *   histogram  lo < hi finite, 1 <= nbins <= TOMO_VOL_MAX_BINS; float32 scale = float32(nbins) / (hi - lo); a finite lo <= v <= hi goes to
 *              bin min(floor((v - lo) * scale), nbins - 1), subtraction and product in float32; finite v < lo: under; finite v > hi: over;
 *              NaN, +-inf: nonfinite.  uint64 counts[nbins] and the three counters; integer atomics only.
 *   quantize   qmax = 255 (8 bit) or 65535 (16 bit); float32 s = float32(qmax) / (hi - lo); code = clamp(rint((v - lo) * s), 0, qmax),
 *              half to even, in float32; NaN -> 0, +inf -> qmax, -inf -> 0; outside the region: fill.  order 0 keeps the layout
 *              out[x][y][z]; order 1 writes out[z][y][x], nz images of ny rows by nx columns.
 *   mask       v inside the region, `value` outside; out may be v itself.
 *   project    the maximum (op 0) or minimum (op 1) of the finite values along an axis, NaN where there are none: [ny][nz] for axis 0,
 *              [nx][nz] for axis 1, [nx][ny] for axis 2.  No region.
 *   slice      the plane `index` of an axis, the same three shapes, bit for bit.
 *
 * Lanes run along z, four consecutive z to a lane: one 16-byte load where nz % 4 == 0 and v is 16-byte aligned, four guarded 4-byte
 * loads of the same elements otherwise; the assignment of elements to lanes, and so every bit of the sums, is the same on both paths.
 * The rows (x, y) are cut into groups of four z (the last of a row may be short) and a work-group of 256 lanes owns
 * TOMO_VOL_SPAN_GROUPS consecutive groups of the volume; stats writes one partial per work-group and a second kernel adds them in a
 * fixed order.  The transposing quantize takes a TOMO_VOL_TILE x TOMO_VOL_TILE tile of (x, z) through LDS.
 *
 * Everything is enqueued on the caller-given stream.  stats and histogram with NULL host pointers only enqueue (tomo_vol_fetch_stats /
 * tomo_vol_fetch_histogram hand the small tables over later); with host pointers they copy them there and wait for the stream.
 *
 * TOMO_VOL_ERR_UNSUPPORTED, before anything is allocated or launched: nx or ny outside 1 ... TOMO_VOL_MAX_DIM, nz outside
 * 1 ... TOMO_VOL_MAX_NZ.  (nz, the contiguous axis, may be long: a flat array is a volume of one row.)
 *
 * A handle owns one device, its buffers and the last error; one handle is used by one thread at a time.  Every entry point returns a
 * tomo_vol_status and checks its arguments before it launches anything; on failure tomo_vol_last_error(h) says why (h may be NULL for
 * errors raised before a handle exists).
 */
#ifndef TOMO_VOL_H
#define TOMO_VOL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_VOL_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_VOL_MAX_DIM 16384         /* nx, ny */
#define TOMO_VOL_MAX_NZ 2147418112     /* nz: 2^31 - 2^16 */
#define TOMO_VOL_MAX_BINS 16384        /* 64 KB of LDS as uint32 */
#define TOMO_VOL_SPAN_GROUPS 4096      /* groups of four z one work-group of the elementwise kernels owns */
#define TOMO_VOL_TILE 64               /* the (x, z) tile of the transposing quantize */

typedef enum {
    TOMO_VOL_OK = 0,
    TOMO_VOL_ERR_ARG = 1,          /* bad argument */
    TOMO_VOL_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_VOL_ERR_NODEV = 3,        /* no HIP device */
    TOMO_VOL_ERR_UNSUPPORTED = 4   /* a size the library does not handle */
} tomo_vol_status;

typedef struct tomo_vol tomo_vol;

typedef struct {
    int64_t n_finite, n_nonfinite;
    double sum, sumsq;             /* of the finite values */
    float min, max;                /* of the finite values; NaN when there are none */
} tomo_vol_stats_t;

TOMO_API int tomo_vol_abi_version(void);
TOMO_API int tomo_vol_create(int device, tomo_vol **h);
TOMO_API int tomo_vol_destroy(tomo_vol *h);
TOMO_API const char *tomo_vol_last_error(tomo_vol *h);
/* device bytes the handle holds between calls */
TOMO_API int tomo_vol_device_bytes(tomo_vol *h, int64_t *bytes);
/* TOMO_VOL_ERR_UNSUPPORTED for a shape beyond the limits above; needs no handle or device. */
TOMO_API int tomo_vol_check_shape(int64_t nx, int64_t ny, int64_t nz);

/* out: NULL (enqueue and return) or where the result goes (waits for the stream). */
TOMO_API int tomo_vol_stats(tomo_vol *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, tomo_vol_stats_t *out);
TOMO_API int tomo_vol_fetch_stats(tomo_vol *h, void *stream, tomo_vol_stats_t *out);
/* counts, extra: both NULL (enqueue and return), or host arrays of nbins and 3 (under, over, nonfinite) uint64 (wait for the stream). */
TOMO_API int tomo_vol_histogram(tomo_vol *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, float lo, float hi, int nbins,
                                uint64_t *counts, uint64_t *extra);
TOMO_API int tomo_vol_fetch_histogram(tomo_vol *h, void *stream, uint64_t *counts, uint64_t *extra);
/* bits: 8 or 16; order: 0 out[x][y][z], 1 out[z][y][x]; 0 <= fill <= qmax; d_out: nx ny nz codes on the device, not overlapping d_v. */
TOMO_API int tomo_vol_quantize(tomo_vol *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, float lo, float hi, int bits,
                               int order, int fill, void *d_out);
/* d_out may be d_v. */
TOMO_API int tomo_vol_mask(tomo_vol *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, float value, float *d_out);
/* axis 0, 1, 2; op 0 (max) or 1 (min); R4 is not used. */
TOMO_API int tomo_vol_project(tomo_vol *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, int axis, int op, float *d_out);
/* axis 0, 1, 2; 0 <= index < the axis' length; R4 is not used. */
TOMO_API int tomo_vol_slice(tomo_vol *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, int axis, int index, float *d_out);

#ifdef __cplusplus
}
#endif
#endif
