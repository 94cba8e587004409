/*
 * libtomo_half.so -- half-acquisition (offset-axis) scans over 2 pi: the position of the rotation axis by the fixed-window overlap search
 * of Vo et al., and the stitch of the 2 pi series to the pi series of double width every other stage expects (gfx950): the device side of
 * tomography_alignment_amd/half_acquisition.py.  A separate library from libtomo_hip.so (include/tomo.h), like libtomo_cor.so and
 * libtomo_mom.so, so that the projector's kernel sources (and the hash that keys the committed PMC counters) stay untouched; it links
 * nothing of the package and no FFT.
 *
 * Definition (tests/half_model.py is the same in numpy).  p[n][nx][nz], float32, z fastest, n even, projection i taken at
 * phi0 + i 2 pi / n; S[n][nx] is one detector row of it.  h = n / 2, A[i][x] = S[i][x], M[i][x] = S[h + i][nx - 1 - x] for i < h.  With
 * the axis at the real column c (centre convention (nx - 1) / 2), A[i][x] = M[i][x + t], t = nx - 1 - 2 c.
 *
 * Search.  A window 4 <= w <= nx / 2 and the candidates p = 0 ... nx - w, np = nx - w + 1 of them.  Side right (curve 0):
 * ref = A[:, nx - w : nx], compared with M[:, p : p + w], t = p - (nx - w).  Side left (curve 1): ref = A[:, 0 : w], t = p.
 *   m(p) = 1 - r,  r = (N Sab - Sa Sb) / sqrt((N Saa - Sa^2) (N Sbb - Sb^2)),  N = h w,  m = 1 where either variance is not > 0,
 * the five sums over the two h x w blocks, the float32 values multiplied (exactly) and added in float64.  The integer minimum, the
 * parabola through its neighbours and the median over the detector rows are the Python layer's, on the table m[row][side][np].
 *   tomo_half_load    gathers the detector rows z of p into contiguous S[row][n][nx], one thread per (angle, column).
 *   tomo_half_search  k_colsums: the sums over i of S and of S^2 of every column of both halves, a thread per column, i in order.
 *                     k_band: Sab is a band sum of the w x nx column Gram G[j][x] = sum_i ref[i][j] M[i][x], Sab(p) = sum_j G[j][p + j].
 *                     A work-group owns TOMO_HALF_TILE_J columns j of ref and TOMO_HALF_TILE_P candidates, stages the rows of ref and of
 *                     M it needs in LDS once, and a lane keeps the Gram entries of four consecutive p and the tile's j in registers
 *                     (i in order), adds them over j in order and writes one partial per (tile of j, p).  Nothing re-reads an h x w
 *                     block per candidate.
 *                     k_fold: a thread per (row, side, p) adds the partials in tile order, forms Sb and Sbb as window sums of the
 *                     per-column sums (Sa, Saa likewise) in column order, and m.
 *                     No atomics; the grid depends on (rows, n, nx, w) only, so the same input gives the same bits in any call and on
 *                     a fresh handle.  The partials (8 ceil(w / TILE_J) np bytes per row and side) are the scratch; under a budget
 *                     (tomo_half_set_max_scratch; 0: no limit; never fewer than one detector row) the rows go in batches, which
 *                     changes no bit.
 *
 * Stitch.  sigma = +1, g = nx - 1 - c for c >= (nx - 1) / 2 (side right); sigma = -1, g = c otherwise.  h rows of
 * W = floor(2 max(c, nx - 1 - c)) + 1 columns; j0 = 0 (right) or W - nx (left); the axis lies at c_out = c + j0.  Output column j takes
 * a = S[i][j - j0] where 0 <= j - j0 <= nx - 1, and b by linear interpolation of the row S[h + i] at x_b = 2 c - (j - j0), i0 = floor(x_b),
 * f = x_b - i0, where 0 <= x_b <= nx - 1.  Both valid: out = wA a + (1 - wA) b, wA = clip((g - sigma u) / (2 g), 0, 1), u = j - c_out,
 * wA = 1 where g = 0; one valid: that one, copied bit for bit.  A column where neither is valid cannot occur.
 *   The table (tomo_half_table) is computed by the host in float64 and uploaded: per column the flags, the three source columns and
 *   the four weights 1 - f, f, wA, 1 - wA rounded to float32 once.  k_stitch only combines: out = fma(wA, a, wB * b),
 *   b = fma(f, s1, (1 - f) * s0), each rounded once (no contraction), so both access paths give the same bits.  Lanes lie along z, four
 *   consecutive z to a lane: one 16-byte load / store where nz % 4 == 0 and p and out are 16-byte aligned, guarded 4-byte accesses of
 *   the same elements otherwise.  A work-group owns TOMO_HALF_TILE_C output columns of one projection and reads their table entries
 *   into LDS once.  The neighbour s1 is not read where f = 0.  out may not overlap p.
 *
 * Everything is enqueued on the caller-given stream (in practice the tomo context's, tomo_ctx_stream); only tomo_half_search with a
 * host pointer, tomo_half_fetch and the debug call hand values to the host and wait for it.
 *
 * TOMO_HALF_ERR_UNSUPPORTED, before anything is allocated or launched: n odd, n < 2 or n > TOMO_HALF_MAX_N, nx < TOMO_HALF_MIN_NX or
 * nx > TOMO_HALF_MAX_NX, nz < 1 or nz > TOMO_HALF_MAX_NZ, more than TOMO_HALF_MAX_ROWS detector rows, a window outside
 * 4 <= w <= nx / 2, an axis outside 0 <= c <= nx - 1.
 *
 * A handle owns one device, its buffers and the last error; one handle is used by one thread at a time.  Every entry point returns a
 * tomo_half_status and checks its arguments before it launches anything; on failure tomo_half_last_error(h) says why (h may be NULL
 * for errors raised before a handle exists).
 */
#ifndef TOMO_HALF_H
#define TOMO_HALF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_HALF_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_HALF_MAX_N 65536     /* projections over 2 pi */
#define TOMO_HALF_MIN_NX 8        /* detector columns: two windows of 4 */
#define TOMO_HALF_MAX_NX 16384
#define TOMO_HALF_MAX_NZ 16384    /* detector rows */
#define TOMO_HALF_MAX_ROWS 4096   /* detector rows of one load */
#define TOMO_HALF_MIN_W 4         /* columns of the search window */
#define TOMO_HALF_TILE_J 8        /* columns of ref of one work-group of the band kernel */
#define TOMO_HALF_TILE_P 1024     /* candidates of one work-group of the band kernel: 256 lanes of four */
#define TOMO_HALF_TILE_C 32       /* output columns of one work-group of the stitch */

typedef enum {
    TOMO_HALF_OK = 0,
    TOMO_HALF_ERR_ARG = 1,          /* bad argument */
    TOMO_HALF_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_HALF_ERR_NODEV = 3,        /* no HIP device */
    TOMO_HALF_ERR_UNSUPPORTED = 4   /* a size the library does not handle */
} tomo_half_status;

/* flags of a column of the stitch table */
enum { TOMO_HALF_A_VALID = 1, TOMO_HALF_B_VALID = 2 };

/* One output column of the stitch: the column ja of the first half's row, the columns i0 and i1 of the second half's row (i1 = i0
 * where f = 0), all in 0 ... nx - 1 whatever the flags say, and the weights as the kernel uses them. */
typedef struct {
    int flags, ja, i0, i1;
    float f0, f1, wa, wb;       /* 1 - f, f, wA, 1 - wA */
} tomo_half_column;

typedef struct tomo_half tomo_half;

TOMO_API int tomo_half_abi_version(void);
TOMO_API int tomo_half_create(int device, tomo_half **h);
TOMO_API int tomo_half_destroy(tomo_half *h);
TOMO_API const char *tomo_half_last_error(tomo_half *h);
/* TOMO_HALF_ERR_UNSUPPORTED for a shape beyond the limits above; nrows and w count only where > 0.  Needs no handle or device. */
TOMO_API int tomo_half_check_shape(int n, int nx, int nz, int nrows, int w);
/* Rows h, columns W, offset j0 and axis c_out of the stitched series.  Needs no handle or device. */
TOMO_API int tomo_half_stitched_shape(int n, int nx, double c, int *h, int *W, int *j0, double *c_out);
/* The table of the stitch: `columns` holds W entries, and f and wa, if not NULL, the float64 values of f and wA before rounding. */
TOMO_API int tomo_half_table(int nx, double c, int W, tomo_half_column *columns, double *f, double *wa);
/* Bytes of partials one detector row of the search needs, and the rows per batch under a budget (0: no limit). */
TOMO_API int tomo_half_scratch_bytes(int nx, int w, size_t *bytes);
TOMO_API int tomo_half_batch(int nrows, int nx, int w, size_t max_scratch_bytes, int *batch);
/* The budget of the partials for the calls that follow (0, the default: no limit). */
TOMO_API int tomo_half_set_max_scratch(tomo_half *h, size_t max_scratch_bytes);
/* device bytes the handle holds between calls */
TOMO_API int tomo_half_device_bytes(tomo_half *h, int64_t *bytes);
/* Gather.  d_p: p[n_p][nx][nz] on the device; rows: nrows host ints in 0 ... nz - 1; the projections 0 ... n - 1 of p are taken,
 * n <= n_p.  Enqueues and returns. */
TOMO_API int tomo_half_load(tomo_half *h, void *stream, const float *d_p, int n_p, int nx, int nz, int n, const int *rows, int nrows);
/* Both curves of every loaded row into the handle's table m[row][2][nx - w + 1].  m: NULL (enqueue and return), or a host array of that
 * size (copy the table there and wait for the stream). */
TOMO_API int tomo_half_search(tomo_half *h, void *stream, int w, double *m);
/* The table of the last tomo_half_search into a host array of its size; waits for the stream. */
TOMO_API int tomo_half_fetch(tomo_half *h, void *stream, double *m);
/* The gathered S[row][n][nx] of one loaded row into host out[n][nx]; waits.  For the tests. */
TOMO_API int tomo_half_debug_sinogram(tomo_half *h, void *stream, int row, float *out);
/* d_out[n / 2][W][nz] = the stitch of d_p[n][nx][nz] about the axis c (both on the device, not overlapping); W as
 * tomo_half_stitched_shape gives it.  Enqueues and returns. */
TOMO_API int tomo_half_stitch(tomo_half *h, void *stream, const float *d_p, int n, int nx, int nz, double c, float *d_out);

#ifdef __cplusplus
}
#endif
#endif
