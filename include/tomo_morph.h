/*
 * libtomo_morph.so -- the exact squared Euclidean distance transform of a mask where it lies in HBM (gfx950) and what follows from it by
 * a comparison: the distance, erosion, dilation, opening and closing by a ball, and the two elementwise kernels of hole filling.  The
 * device side of tomography_alignment_amd/morphology.py.  A separate library like libtomo_seg.so; it links nothing of the package.
 *
 * Definitions (tests/morph_model.py is the same in numpy).  Volumes are [nx][ny][nz], z fastest; the linear index of (x, y, z) is
 * i = (x ny + y) nz + z.  A mask is uint8, non-zero is foreground.  1 <= nx, ny, nz <= TOMO_MORPH_MAX_DIM and at most
 * TOMO_MORPH_MAX_VOXELS voxels, so every finite squared distance is at most 3 * 16383^2 < 2^31 - 1 = TOMO_MORPH_INF.
 *
 *   distance_sq  (int32) 0 on the background; on the foreground the minimum of |p - b|^2 over the background voxels b.
 *                border 0 ("ignore"): only background voxels inside the volume count -- scipy's distance_transform_edt, squared; a mask
 *                without background gives TOMO_MORPH_INF everywhere.  border 1 ("background"): every position outside the volume is
 *                background too, so a voxel is at most min(x + 1, nx - x, y + 1, ny - y, z + 1, nz - z)^2 away and nothing is INF.
 *   distance     (float32) the correctly rounded square root of distance_sq, TOMO_MORPH_INF -> +inf: the float32 rounding of the float64
 *                square root.  (A root that is not an integer lies at least sqrt(n) 2^-49 from a float32 rounding boundary, several float64
 *                ulps, so the two roundings are one.)  tomo_morph_root is that step alone, on any int32 >= 0.
 *   erode        (uint8) 1 iff every offset o in Z^3 with |o|^2 <= r2 lands on foreground, the outside counting as border_value:
 *                distance_sq(mask, border_value == 0 ? "background" : "ignore") > r2, with INF above every r2.  r2 >= 0.
 *   dilate       (uint8) 1 iff distance_sq(not mask, "ignore") <= r2; a mask of zeros stays zeros.
 *   open         dilate(erode(mask, r2, border_value), r2);  close: erode(dilate(mask, r2), r2, border_value).  One call each.
 *   invert       (uint8) 1 where the mask is 0, else 0.
 *   select       mask[i] = 1 where 0 <= labels[i] <= n and table[labels[i]] != 0; other voxels stay (table: n + 1 bytes on the device).
 *                A label outside 0 ... n is skipped.
 *
 * The transform is three exact integer line passes, g[i] = min_j f[j] + (i - j)^2, along z, then y, then x (csrc/tomo_side_lines.h:
 * a lane owns an output and walks outward until k^2 >= its best); f starts as 0 / INF off the mask, and with border 1 the positions -1
 * and n of every line of every pass hold 0.  Lines are staged in LDS: along z a work-group of TOMO_MORPH_GROUP lanes owns whole rows,
 * along x and y all of a line's length times TOMO_MORPH_W or more adjacent z, 16-byte accesses where the columns are a multiple of four
 * and the pointers aligned, guarded single ones otherwise, with the same results.  A line longer than the line limit
 * (TOMO_MORPH_LINE_LIMIT, 4 limit int32 = 64 KiB of LDS a work-group) takes a second path that reads f from global memory and writes to
 * another buffer.  The last pass stores what the call asks for -- int32, the float32 root or the byte of the comparison -- so the last
 * int32 volume of erode / dilate / distance is never written.  No work-group waits for another; what needs everything before it is the
 * next launch.  Only vector stores and plain C++.
 *
 * Scratch: distance_sq and distance work in the output and take one int32 volume only when a line is longer than the limit; erode, dilate,
 * open and close take one int32 volume, and a second one only when the y axis is longer than the limit.  Scratch above
 * TOMO_MORPH_KEEP_BYTES is freed before a call returns (which then waits for the stream); otherwise everything is enqueued on the
 * caller-given stream and nothing waits.  TOMO_MORPH_ERR_UNSUPPORTED, before anything is allocated or launched, for a shape beyond the
 * limits.  A handle owns one device, its scratch and the last error, and is used by one thread at a time.
 */
#ifndef TOMO_MORPH_H
#define TOMO_MORPH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_MORPH_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_MORPH_MAX_DIM 16384            /* nx, ny, nz */
#define TOMO_MORPH_MAX_VOXELS 2147483647    /* 2^31 - 1 */
#define TOMO_MORPH_INF 2147483647           /* no background anywhere */
#define TOMO_MORPH_W 4                      /* adjacent z a lane of the x and y passes owns */
#define TOMO_MORPH_MAX_WQ 16                /* groups of W adjacent z a work-group owns at most */
#define TOMO_MORPH_GROUP 512                /* lanes of a work-group of the staged passes */
#define TOMO_MORPH_LINE_LIMIT 4096          /* the longest line the LDS path takes by default */
#define TOMO_MORPH_KEEP_BYTES (16 << 20)    /* scratch the handle keeps between calls */

typedef enum {
    TOMO_MORPH_OK = 0,
    TOMO_MORPH_ERR_ARG = 1,          /* bad argument */
    TOMO_MORPH_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_MORPH_ERR_NODEV = 3,        /* no HIP device */
    TOMO_MORPH_ERR_UNSUPPORTED = 4   /* a size the library does not handle */
} tomo_morph_status;

typedef struct tomo_morph tomo_morph;

TOMO_API int tomo_morph_abi_version(void);
TOMO_API int tomo_morph_create(int device, tomo_morph **h);
TOMO_API int tomo_morph_destroy(tomo_morph *h);
TOMO_API const char *tomo_morph_last_error(tomo_morph *h);
/* device bytes the handle holds between calls */
TOMO_API int tomo_morph_device_bytes(tomo_morph *h, int64_t *bytes);
/* TOMO_MORPH_ERR_UNSUPPORTED for a shape beyond the limits above; needs no handle or device. */
TOMO_API int tomo_morph_check_shape(int64_t nx, int64_t ny, int64_t nz);
/* The longest line the LDS path takes in the calls that follow: 1 ... TOMO_MORPH_LINE_LIMIT, 0 for the default.  No bit of any result
 * depends on it. */
TOMO_API int tomo_morph_set_line_limit(tomo_morph *h, int n);

/* border 0: "ignore", 1: "background".  d_out: nx ny nz int32, not overlapping d_mask. */
TOMO_API int tomo_morph_distance_sq(tomo_morph *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int border, int32_t *d_out);
/* d_out: nx ny nz float32, not overlapping d_mask. */
TOMO_API int tomo_morph_distance(tomo_morph *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int border, float *d_out);
/* One pass of the transform alone, for timing and tests: axis 2 (z) reads the mask d_src (bytes) and starts the transform, axis 1 (y) and
 * 0 (x) read int32 d_src; d_dst: int32, it may be d_src on axes 1 and 0 while the line is no longer than the line limit. */
TOMO_API int tomo_morph_line_pass(tomo_morph *h, void *stream, const void *d_src, int nx, int ny, int nz, int axis, int border, int32_t *d_dst);
/* d_out[i] = the float32 root of d_d2[i] >= 0, TOMO_MORPH_INF -> +inf, for i < n; d_out may be d_d2. */
TOMO_API int tomo_morph_root(tomo_morph *h, void *stream, const int32_t *d_d2, int64_t n, float *d_out);
/* r2 >= 0; border_value 0 or 1; d_out: nx ny nz bytes, it may be d_mask. */
TOMO_API int tomo_morph_erode(tomo_morph *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int64_t r2, int border_value,
                              uint8_t *d_out);
TOMO_API int tomo_morph_dilate(tomo_morph *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int64_t r2, uint8_t *d_out);
TOMO_API int tomo_morph_open(tomo_morph *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int64_t r2, int border_value,
                             uint8_t *d_out);
TOMO_API int tomo_morph_close(tomo_morph *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int64_t r2, int border_value,
                              uint8_t *d_out);
/* d_out[i] = d_mask[i] == 0 for i < n; d_out may be d_mask. */
TOMO_API int tomo_morph_invert(tomo_morph *h, void *stream, const uint8_t *d_mask, int64_t n, uint8_t *d_out);
/* d_mask[i] = 1 where d_table[d_labels[i]] != 0 (d_table: n + 1 bytes on the device), for i < voxels; labels outside 0 ... n are skipped. */
TOMO_API int tomo_morph_select(tomo_morph *h, void *stream, const int32_t *d_labels, int64_t voxels, int32_t n, const uint8_t *d_table,
                               uint8_t *d_mask);

#ifdef __cplusplus
}
#endif
#endif
