/*
 * libtomo_mesh.so -- the isosurface of a volume where it lies in HBM (gfx950) as a list of triangles, with its area and the volume it
 * encloses: marching tetrahedra, six per cell.  The device side of tomography_alignment_amd/mesh.py.  A separate library like
 * libtomo_seg.so; it links nothing of the package.
 *
 * Definition (tests/mesh_model.py is the same in numpy).  Volumes are [nx][ny][nz], z fastest; voxel (i, j, k) is the lattice point
 * (i, j, k), and vertices are float32 in that index frame.  1 <= nx, ny, nz <= TOMO_MESH_MAX_DIM, at most TOMO_MESH_MAX_VOXELS voxels,
 * and tomo_mesh_extract writes at most TOMO_MESH_MAX_TRIANGLES triangles.
 *
 *   input        dtype TOMO_MESH_F32: a float32 volume, taken at `level` (finite).  dtype TOMO_MESH_U8: a mask, non-zero counting as 1,
 *                taken at 0.5 (`level` is not read).  A corner is inside when v >= level; NaN is outside.
 *   cells        A cell is the cube between eight neighbouring voxels.  border TOMO_MESH_OPEN: cell origins 0 ... n - 2 on each axis; an
 *                axis of length 1 has no cells.  border TOMO_MESH_CLOSED: the volume stands in one layer of voxels of value -inf and cell
 *                origins are -1 ... n - 1, so an object that touches a face gets a closed surface.  Coordinates are those of the
 *                unpadded frame, computed directly: the low end of an edge may be at -1.
 *   tetrahedra   For each permutation (a, b, c) of the axes, in lexicographic order, the tetrahedron with the corners o, o + e_a,
 *                o + e_a + e_b, o + (1, 1, 1), in that order.  Their face diagonals match by translation, so neighbouring cells agree.
 *   vertex       on a crossed edge (one end inside, one outside): lo is the end with the smaller lattice coordinates, hi - lo has
 *                components 0 or 1.  t = (level - v_lo) / (v_hi - v_lo) in float32, the division correctly rounded; t = 0.5 when v_lo,
 *                v_hi or v_hi - v_lo is not finite.  A component in which hi differs from lo is float32(lo) + t, the others are exact.
 *                No multiplication, so contraction changes nothing, and every cell that shares the edge computes the same bits.
 *   triangles    per tetrahedron, corners in corner order.  One inside corner a, outside o1 < o2 < o3: (a o1, a o2, a o3).  Three inside
 *                i1 < i2 < i3, outside o: (i1 o, i2 o, i3 o).  Two inside a < b, two outside c < d: (ac, ad, bd) and (ac, bd, bc).
 *   orientation  (p1 - p0) x (p2 - p0) points away from the inside corners -- decided by the case alone, as if every t were 0.5, by
 *                swapping the last two vertices where needed; never by the positions, which coincide when a voxel equals the level.
 *                Triangles of zero area are kept.  The surface is closed bit for bit: every directed edge with distinct ends has its
 *                reverse.
 *   measures     area = sum |e| / 2 and volume = sum p0 . e / 6 with e = (p1 - p0) x (p2 - p0), which is sum p0 . (p1 x p2) / 6: float64
 *                from the float32 vertices, summed in an order that the shape and the border alone fix.  No float atomics.
 *   order        of the triangles: a function of shape, border and input only -- brick by brick, inside a brick lane by lane, a lane's
 *                cells along x, a cell's tetrahedra in order.  A repeat gives the same bytes, and so does another handle.
 *
 * Kernels (csrc/mesh/tomo_mesh.hip, csrc/tomo_side_tets.h).  A work-group of TOMO_MESH_GROUP lanes owns a brick of TOMO_MESH_BRICK_X x
 * _Y x _Z cells and stages its voxels plus one layer on the high side of each axis in LDS (16-byte loads of float32 and 4-byte loads of
 * mask bytes along z where nz % 4 == 0 and the pointer is aligned, guarded single loads otherwise; the -inf layer is never read from
 * memory).  The count kernel leaves each brick's number of triangles and, for measure, its two float64 partial sums; one work-group
 * turns the counts into int64 offsets and adds the partials up in a fixed order; the emit kernel, whose work-groups without a triangle
 * exit at once, stages again and writes each triangle at offset + rank, the rank from a fixed-order scan of the lanes' counts.  Nothing
 * is appended through an atomic counter.  Only vector stores and plain C++.
 *
 * Scratch: 4 bytes a brick, 8 more in extract, 16 more in measure.  A handle that holds more than TOMO_MESH_KEEP_BYTES of it at the end
 * of a call frees all of it before the call returns.  Both calls wait for the stream: they hand numbers back.
 * TOMO_MESH_ERR_UNSUPPORTED, before anything is allocated or launched, for a shape beyond the limits.  A handle owns one device, its
 * scratch and the last error, and is used by one thread at a time.
 */
#ifndef TOMO_MESH_H
#define TOMO_MESH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_MESH_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_MESH_MAX_DIM 16384               /* nx, ny, nz */
#define TOMO_MESH_MAX_VOXELS 2147483647       /* 2^31 - 1 */
#define TOMO_MESH_MAX_TRIANGLES 2147483647    /* 2^31 - 1 */
#define TOMO_MESH_BRICK_X 8                   /* the cells of a work-group's brick */
#define TOMO_MESH_BRICK_Y 8
#define TOMO_MESH_BRICK_Z 32
#define TOMO_MESH_GROUP 256                   /* lanes of a work-group: one per (y, z) of the brick, walking x */
#define TOMO_MESH_KEEP_BYTES (16 << 20)       /* scratch the handle keeps between calls */

#define TOMO_MESH_F32 0                       /* dtype */
#define TOMO_MESH_U8 1
#define TOMO_MESH_OPEN 0                      /* border */
#define TOMO_MESH_CLOSED 1

typedef enum {
    TOMO_MESH_OK = 0,
    TOMO_MESH_ERR_ARG = 1,          /* bad argument */
    TOMO_MESH_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_MESH_ERR_NODEV = 3,        /* no HIP device */
    TOMO_MESH_ERR_UNSUPPORTED = 4,  /* a size the library does not handle */
    TOMO_MESH_ERR_CAPACITY = 5      /* tomo_mesh_extract: more triangles than the buffer holds; nothing was written */
} tomo_mesh_status;

typedef struct tomo_mesh tomo_mesh;

TOMO_API int tomo_mesh_abi_version(void);
TOMO_API int tomo_mesh_create(int device, tomo_mesh **h);
TOMO_API int tomo_mesh_destroy(tomo_mesh *h);
TOMO_API const char *tomo_mesh_last_error(tomo_mesh *h);
/* device bytes the handle holds between calls */
TOMO_API int tomo_mesh_device_bytes(tomo_mesh *h, int64_t *bytes);
/* TOMO_MESH_ERR_UNSUPPORTED for a shape beyond the limits above; needs no handle or device. */
TOMO_API int tomo_mesh_check_shape(int64_t nx, int64_t ny, int64_t nz);

/* One pass over the volume, no triangle written: their number (which may be above TOMO_MESH_MAX_TRIANGLES: nothing here depends on
 * it), the area and the enclosed volume.  Waits for the stream. */
TOMO_API int tomo_mesh_measure(tomo_mesh *h, void *stream, const void *d_vol, int dtype, int nx, int ny, int nz, float level, int border,
                               int64_t *n_triangles, double *area, double *volume);
/* Counts, scans and writes float32 [n][3][3] to d_triangles (4-byte aligned; it may be NULL with capacity 0).  *n_triangles is the
 * number the surface has; with n > capacity the call returns TOMO_MESH_ERR_CAPACITY and has written nothing.  It keeps nothing of an
 * earlier call.  TOMO_MESH_ERR_UNSUPPORTED, and nothing written, for a surface of more than TOMO_MESH_MAX_TRIANGLES.  Waits for the
 * stream. */
TOMO_API int tomo_mesh_extract(tomo_mesh *h, void *stream, const void *d_vol, int dtype, int nx, int ny, int nz, float level, int border,
                               float *d_triangles, int64_t capacity, int64_t *n_triangles);

#ifdef __cplusplus
}
#endif
#endif
