/*
 * libtomo_seg.so -- segmentation of a reconstructed volume where it lies in HBM (gfx950): threshold to a mask, 3-D connected-component
 * labels, per-component measures, removal of small components, the largest component.  The device side of
 * tomography_alignment_amd/segment.py.  A separate library like libtomo_vol.so; it links nothing of the package and no FFT.
 *
 * Definitions (tests/seg_model.py is the same in numpy).  Volumes are [nx][ny][nz], z fastest; the linear index of (x, y, z) is
 * i = (x ny + y) nz + z.  A volume has at most 2^31 - 1 voxels, so i is an int32.
 *
 *   region     as include/tomo_vol.h: R4 < 0 everything, else (2x - nx + 1)^2 + (2y - ny + 1)^2 <= R4 in int64.
 *   threshold  mask (uint8) = 1 where the voxel is inside the region, is not NaN and passes the bounds that are given, lo <= v and
 *              v <= hi in float32; 0 otherwise.  At least one bound is given and a given bound is finite.  So NaN gives 0, and +inf
 *              (-inf) gives 0 unless hi (lo) is missing, in which case it passes like any value above lo (below hi).
 *   label      mask: uint8, non-zero is foreground.  connectivity 1, 2, 3: voxels are neighbours when they differ by at most one in
 *              every axis and in at most `connectivity` axes (6, 18, 26 neighbours).  labels (int32): 0 on the background; component
 *              k = 1 ... n is the one whose smallest linear index is the k-th smallest among the components' smallest indices -- the
 *              numbering of scipy.ndimage.label.  It depends on the mask only.
 *   measure    for k = 1 ... n: count[k-1] (int64), bbox[k-1] = (xmin, xmax, ymin, ymax, zmin, zmax) inclusive (int32),
 *              coord_sum[k-1] = (sum x, sum y, sum z) (int64): integer atomics only, exact.  With a volume v: vmin, vmax of the
 *              component's finite values (float32, exact; -0 < +0; NaN where it has none) and vsum, their float64 sum, accumulated
 *              with float64 atomics in no fixed order.  A label outside 0 ... n is an error of the caller and is skipped.
 *              The tables live in handle scratch of at most max_scratch bytes (tomo_seg_set_max_scratch, default 256 MiB, never less
 *              than one component): with more components than fit, the labels 1 ... n go in ranges, one pass over the volume per
 *              range (tomo_seg_measure_passes).  The passes do not change a bit of the integer tables, vmin or vmax.
 *   remove_small   components of fewer than min_size voxels become 0; the others are renumbered 1 ... n_kept in their order.
 *                  d_out may be d_labels.
 *   largest    mask (uint8) = 1 on the component with the most voxels, the lowest label among equals; all 0 when n = 0.
 *
 * The labelling is union-find on the label array itself, which doubles as the parent array: a foreground voxel's parent is always a
 * foreground index <= its own, the background holds a sentinel.  find follows strictly decreasing indices; union installs the smaller
 * root under the larger with an integer atomic minimum on the larger and retries from the value that returned when it lost a race.
 * No work-group waits for another; what needs everything before it is the next launch:
 *   tile      a work-group per brick of TOMO_SEG_TILE_X x TOMO_SEG_TILE_Y x TOMO_SEG_TILE_Z voxels: the mask as one 64-bit word per
 *             row in LDS, the runs along z collapsed from those words, union-find of the runs in LDS, parents out as global indices.
 *   border    unions across brick faces, edges and corners by the connectivity.
 *   compress  label = find(i), and the roots of every stretch of TOMO_SEG_SPAN_GROUPS groups of four z counted.
 *   scan      exclusive prefix sum of those counts (one work-group); rank: every root becomes -(rank + 1); final: every foreground
 *             voxel takes |label of its root|.
 *
 * The elementwise passes give a lane four consecutive z: 16-byte loads of float32 / int32 and one 4-byte access of four mask bytes
 * where nz % 4 == 0 and the pointer is aligned to that, guarded single accesses otherwise, with the same results.
 *
 * Everything is enqueued on the caller-given stream; a call that hands a number or a table to the host waits for it.
 * TOMO_SEG_ERR_UNSUPPORTED, before anything is allocated or launched: nx, ny outside 1 ... TOMO_SEG_MAX_DIM, nz < 1, or more than
 * TOMO_SEG_MAX_VOXELS voxels.  A handle owns one device, its scratch and the last error, and is used by one thread at a time; scratch
 * above TOMO_SEG_KEEP_BYTES is freed before a call returns.  Every entry point checks its arguments before it launches anything.
 */
#ifndef TOMO_SEG_H
#define TOMO_SEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_SEG_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_SEG_MAX_DIM 16384            /* nx, ny */
#define TOMO_SEG_MAX_VOXELS 2147483647    /* 2^31 - 1 */
#define TOMO_SEG_TILE_X 8                 /* the brick of the tile pass */
#define TOMO_SEG_TILE_Y 8
#define TOMO_SEG_TILE_Z 64
#define TOMO_SEG_SPAN_GROUPS 1024         /* groups of four z one work-group of the elementwise passes owns */
#define TOMO_SEG_KEEP_BYTES (16 << 20)    /* scratch the handle keeps between calls */
#define TOMO_SEG_DEFAULT_SCRATCH (256 << 20)

typedef enum {
    TOMO_SEG_OK = 0,
    TOMO_SEG_ERR_ARG = 1,          /* bad argument */
    TOMO_SEG_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_SEG_ERR_NODEV = 3,        /* no HIP device */
    TOMO_SEG_ERR_UNSUPPORTED = 4   /* a size the library does not handle */
} tomo_seg_status;

typedef struct tomo_seg tomo_seg;

TOMO_API int tomo_seg_abi_version(void);
TOMO_API int tomo_seg_create(int device, tomo_seg **h);
TOMO_API int tomo_seg_destroy(tomo_seg *h);
TOMO_API const char *tomo_seg_last_error(tomo_seg *h);
/* device bytes the handle holds between calls */
TOMO_API int tomo_seg_device_bytes(tomo_seg *h, int64_t *bytes);
/* TOMO_SEG_ERR_UNSUPPORTED for a shape beyond the limits above; needs no handle or device. */
TOMO_API int tomo_seg_check_shape(int64_t nx, int64_t ny, int64_t nz);
/* The budget of measure's tables for the calls that follow (0: TOMO_SEG_DEFAULT_SCRATCH). */
TOMO_API int tomo_seg_set_max_scratch(tomo_seg *h, size_t max_scratch_bytes);
/* The passes over the volume measure makes for n components under a budget (0: the default); needs no handle or device. */
TOMO_API int tomo_seg_measure_passes(int64_t n, int with_vol, size_t max_scratch_bytes, int *passes);

/* has_lo, has_hi: whether lo, hi are tested (at least one); d_mask: nx ny nz bytes. */
TOMO_API int tomo_seg_threshold(tomo_seg *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, float lo, float hi, int has_lo,
                                int has_hi, uint8_t *d_mask);
/* connectivity 1, 2, 3; d_labels: nx ny nz int32, not overlapping d_mask; *n: the number of components (waits for the stream). */
TOMO_API int tomo_seg_label(tomo_seg *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int connectivity, int32_t *d_labels,
                            int32_t *n);
/* Host tables of n entries: count[n], bbox[n][6], coord_sum[n][3]; d_v NULL, or the volume and vmin[n], vmax[n], vsum[n].  Waits. */
TOMO_API int tomo_seg_measure(tomo_seg *h, void *stream, const int32_t *d_labels, const float *d_v, int nx, int ny, int nz, int32_t n,
                              int64_t *count, int32_t *bbox, int64_t *coord_sum, float *vmin, float *vmax, double *vsum);
/* d_out may be d_labels; *n_kept: the number of components left (waits). */
TOMO_API int tomo_seg_remove_small(tomo_seg *h, void *stream, const int32_t *d_labels, int nx, int ny, int nz, int32_t n, int64_t min_size,
                                   int32_t *d_out, int32_t *n_kept);
/* d_mask: nx ny nz bytes; *label (0 when n = 0) and *count of the component taken (waits). */
TOMO_API int tomo_seg_largest(tomo_seg *h, void *stream, const int32_t *d_labels, int nx, int ny, int nz, int32_t n, uint8_t *d_mask,
                              int32_t *label, int64_t *count);

#ifdef __cplusplus
}
#endif
#endif
