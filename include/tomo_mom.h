/*
 * libtomo_mom.so -- the two marginals of every projection of a parallel-beam series in one pass over the sinogram (gfx950): the device
 * side of tomography_alignment_amd/align/consistency.py, which turns them into the moments of order 0 and 1 (mass, centroids) and
 * those, through the Helgason-Ludwig conditions, into a drift-free start for the per-projection shifts.  A separate library from
 * libtomo_hip.so (include/tomo.h), like libtomo_cor.so, so that the projector's kernel sources (and the hash that keys the committed
 * PMC counters) stay untouched; it links nothing of the package and no FFT.
 *
 * Definition (tests/mom_model.py is the same in numpy, with correctly rounded sums).  p[n][nx][nz], float32, z fastest: the layout of
 * every operator.  A window 0 <= z0 < z1 <= nz of detector rows and a threshold `floor` (a double; -inf switches it off):
 *   v(p)    = p where p is finite and p >= floor, 0 otherwise.
 *   Q[i][x] = sum over z0 <= z < z1 of v(p[i][x][z])                          float64 [n][nx]
 *   Z[i][z] = sum over x of v(p[i][x][z]) for z0 <= z < z1, 0 outside it      float64 [n][nz]
 *   bad[i]  = how many p[i][x][z] with z0 <= z < z1 are NaN or +-inf          int32 [n]
 * A detector row outside the window is not read, so what it holds -- non-finite values included -- counts nowhere.
 *
 * One kernel reads p once.  A work-group of 256 lanes lies along z, four consecutive z to a lane (one 16-byte load where nz % 4 == 0
 * and p is 16-byte aligned, four guarded 4-byte loads of the same elements otherwise: the assignment of elements to lanes, and so
 * every bit of the result, is the same on both paths), and owns a tile of TOMO_MOM_TILE_X detector columns x of one projection and
 * one chunk of TOMO_MOM_CHUNK_Z rows.  Per column x the lane's four values are added in float64, the 64 lanes of a wave by a fixed
 * shuffle tree, the four waves in order: one partial of Q per (x, chunk).  Per lane the four z of every x of the tile are accumulated in
 * float64 in the order of x: one partial of Z per (tile, z).  Where nz <= 512 (256), two (one) of the four waves span z and the waves
 * form G = 2 (4) groups that split the tile's columns, each with a partial of Z of its own; G = 1 otherwise.  A second kernel adds a
 * projection's partials in index order (tiles and groups for Z, chunks for Q, work-groups for bad).  No atomics; the grid depends on (n, nx, nz) only, so the same input gives the same bits in any
 * call, on a fresh handle and for a sub-stack of the projections.
 *
 * The partials (per projection: 8 nz G ceil(nx / TILE_X) + 8 nx ceil(nz / CHUNK_Z) + 4 ceil(nx / TILE_X) ceil(nz / CHUNK_Z) bytes) and the
 * device tables Q, Z, bad belong to the handle.  tomo_mom_set_max_scratch bounds the partials: the projections are processed in batches
 * of the largest count whose partials fit (0: no limit; never fewer than one projection), which changes no bit.
 *
 * Everything is enqueued on the caller-given stream (in practice the tomo context's, tomo_ctx_stream).  tomo_mom_marginals with NULL
 * host pointers only enqueues; with host pointers, and tomo_mom_fetch, hand the tables to the host and wait for the stream.
 *
 * TOMO_MOM_ERR_UNSUPPORTED, before anything is allocated or launched: n < 1, nx < 1, nz < 1, nz > TOMO_MOM_MAX_NZ, or a window that
 * is not 0 <= z0 < z1 <= nz.
 *
 * A handle owns one device, its buffers and the last error; one handle is used by one thread at a time.  Every entry point returns a
 * tomo_mom_status and checks its arguments before it launches anything; on failure tomo_mom_last_error(h) says why (h may be NULL for
 * errors raised before a handle exists).
 */
#ifndef TOMO_MOM_H
#define TOMO_MOM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_MOM_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_MOM_MAX_NZ 16384  /* detector rows */
#define TOMO_MOM_TILE_X 128    /* detector columns of one work-group */
#define TOMO_MOM_CHUNK_Z 1024  /* detector rows of one work-group: 256 lanes of four */

typedef enum {
    TOMO_MOM_OK = 0,
    TOMO_MOM_ERR_ARG = 1,          /* bad argument */
    TOMO_MOM_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_MOM_ERR_NODEV = 3,        /* no HIP device */
    TOMO_MOM_ERR_UNSUPPORTED = 4   /* a size the library does not handle */
} tomo_mom_status;

typedef struct tomo_mom tomo_mom;

TOMO_API int tomo_mom_abi_version(void);
TOMO_API int tomo_mom_create(int device, tomo_mom **h);
TOMO_API int tomo_mom_destroy(tomo_mom *h);
TOMO_API const char *tomo_mom_last_error(tomo_mom *h);
/* TOMO_MOM_ERR_UNSUPPORTED for a shape or window beyond the limits above; needs no handle or device. */
TOMO_API int tomo_mom_check_shape(int n, int nx, int nz, int z0, int z1);
/* Bytes of partials one projection needs, and the projections per batch under a budget (0: no limit).  Need no handle or device. */
TOMO_API int tomo_mom_scratch_bytes(int nx, int nz, size_t *bytes);
TOMO_API int tomo_mom_batch(int n, int nx, int nz, size_t max_scratch_bytes, int *batch);
/* The budget of the partials for the calls that follow (0, the default: no limit). */
TOMO_API int tomo_mom_set_max_scratch(tomo_mom *h, size_t max_scratch_bytes);
/* device bytes the handle holds between calls */
TOMO_API int tomo_mom_device_bytes(tomo_mom *h, int64_t *bytes);
/* The marginals of d_p, p[n][nx][nz] on the device, into the handle's device tables.  Q, Z, bad: all NULL (enqueue and return), or
 * host arrays of n nx doubles, n nz doubles and n ints (copy the tables there and wait for the stream). */
TOMO_API int tomo_mom_marginals(tomo_mom *h, void *stream, const float *d_p, int n, int nx, int nz, double floor, int z0, int z1, double *Q,
                                double *Z, int *bad);
/* The tables of the last tomo_mom_marginals into host arrays of its sizes; waits for the stream. */
TOMO_API int tomo_mom_fetch(tomo_mom *h, void *stream, double *Q, double *Z, int *bad);

#ifdef __cplusplus
}
#endif
#endif
