/*
 * libtomo_dff.so -- dynamic flat-field correction (Van Nieuwenhove et al., Opt. Express 23, 27975, 2015) on gfx950: the device side of
 * preprocess.eigen_flats and preprocess.normalize_dynamic.  The flats say how the beam varies: their principal components are the eigen
 * flat fields (EFFs), every projection gets a flat of its own, fbar + sum_j w_j e_j, and the few weights w are those for which the
 * normalised projection has the least total variation.  A separate library from libtomo_hip.so (include/tomo.h) and from libtomo_prep.so,
 * so that the projector's kernel sources (and the hash that keys the committed PMC counters) stay untouched; it links nothing of the
 * package and no FFT.
 *
 * Layouts are preprocess.py's.  Frames, flats and darks are [n][rows = z][cols = x], x fastest, uint16 (TOMO_DFF_U16) or float32
 * (TOMO_DFF_F32); fbar (the float32 mean flat of tomo_prep_reference), dark and every EFF are float32 [rows][cols]; the sinogram that
 * tomo_dff_apply writes is float32 (n, x1 - x0, z1 - z0), z fastest.  P = rows cols.  tests/dff_model.py is the same arithmetic in numpy.
 *
 * (a) Gram matrix, tomo_dff_gram.  c_k[p] = double(F_k[p]) - double(fbar[p]);  G[k][l] = sum_p c_k[p] c_l[p] in float64.  The pixels
 *     are cut into chunks of C = tomo_dff_gram_chunk(K) consecutive pixels (a multiple of 64: the most that keeps K (C + 1) + C floats
 *     within 32 KiB of LDS and C <= 512, at least 64, which from K = 120 on takes up to 33.5 KiB) and the chunks into groups of max(1, 4096 / C) consecutive chunks.  A work-group
 *     owns a group: it stages a chunk of all K flats in LDS (the flats are read from HBM once), and the thread that owns the pair
 *     l <= k adds c_k[p] c_l[p] over the group's pixels in ascending p.  A second kernel adds the groups' partials in index order and
 *     writes G[k][l] and G[l][k].  No atomics; the order depends on (K, rows, cols) only, so every call and every handle give the same
 *     bits, and G is symmetric bit for bit.  K K doubles come back to the host (the call waits for the stream).
 * (b) Eigen flat fields, tomo_dff_eff.  The host diagonalises G (numpy.linalg.eigh, eigenvalues descending, every eigenvector's sign
 *     such that its component of largest magnitude -- the lowest index on a tie -- is positive) and hands over V[k][j], K x m doubles:
 *         e_j[p] = float32( (1 / sqrt(double(K))) * sum_k V[k][j] c_k[p] )          the sum in float64, k ascending
 *     With this scale the flats' own scores on e_j have unit mean square: a weight is in standard deviations of the flats' variation.
 * (c) Binning, tomo_dff_bin and tomo_dff_load.  For a factor b, zb = rows / b, xb = cols / b (integer division):
 *         out[i][z][x] = sum over the b x b block at (b z, b x), rows then columns, of (float(src_i) - dark)       all float32
 *     Rows and columns beyond b zb and b xb are dropped; b = 1 is a copy with the dark subtracted; dark may be NULL (nothing is
 *     subtracted).  Fb = bin(fbar, dark), Eb_j = bin(e_j, NULL) go where the caller says (tomo_dff_bin); Rb_i = bin(raw_i, dark) goes
 *     into the handle's scratch (tomo_dff_load).
 * (d) TV cost and gradient, tomo_dff_cost: one launch for any list `ids` of loaded projections.  Per listed projection a weight row
 *     w[0..m), a factor s and, for all, the table a[0..m] and eps, all float32.  Per binned pixel, in float32:
 *         D = Fb + sum_j w_j Eb_j (j ascending);  clamped = D < 1e-6, and then D = 1e-6;  q = Rb / D;  v = s q
 *         u_j = a_j q - v Eb_j / D, the second term dropped where the pixel was clamped
 *     a_0 = mean(Fb), a_j = mean(Eb_j) (float64 means, the caller's), s = a_0 + sum_j w_j a_j: the paper's mean(flat), which takes away
 *     the degeneracy "a brighter flat gives a smaller TV".  Over the (zb - 1)(xb - 1) pixels that have a right and a lower neighbour:
 *         gx = v[z][x+1] - v[z][x];  gz = v[z+1][x] - v[z][x];  t = sqrt(gx^2 + gz^2 + eps^2)                      float32
 *         f   = sum t                                                                                           float64
 *         g_j = sum (gx (u_j[z][x+1] - u_j[z][x]) + gz (u_j[z+1][x] - u_j[z][x])) / t     the term float32, the sum float64
 *     The float32 quotients are formed as products with one reciprocal per pixel (1 / D, 1 / t), each within an ulp or two of the
 *     quotient: the float64 model bounds the whole at 1e-5 of f and of sum |terms of g_j|, it does not pin bits.
 *     A work-group owns a tile of TOMO_DFF_TILE_Z x TOMO_DFF_TILE_X such pixels of one projection, staged with a one-pixel halo in LDS;
 *     its lanes add their pixels in float64, the 64 lanes of a wave by a fixed shuffle tree, the four waves in order: one partial per
 *     tile.  A second kernel adds a projection's tiles in index order.  No atomics: the same call gives the same bits, whatever else
 *     `ids` lists.  Fb and Eb are shared by all projections and stay in L2; Rb is the only stream.
 * (e) Apply, tomo_dff_apply: tomo_prep_normalize's definition with a flat per projection.  In float32, w_ij the float32 weight:
 *         flat_i = fbar;  for j ascending: flat_i = flat_i + float32(w_ij * e_j)           product and sum each rounded on its own
 *         den = flat_i - dark;  den = den < 1e-6 ? 1e-6 : den;  r = (float(raw) - dark) / den            IEEE division
 *         r = fmin(r, cutoff) if use_cutoff;  out = minus_log ? -log(fmax(r, min_ratio)) : r
 *     written transposed through LDS tiles into out[i][x - x0][z - z0].  With m = 0 or zero weights every bit is tomo_prep_normalize's.
 * (f) Scratch.  tomo_dff_set_max_scratch bounds Rb: tomo_dff_batch is the largest number of projections whose Rb fits (0: no limit;
 *     never fewer than one), and tomo_dff_load takes at most that many at a time.  Every projection is independent, so the batch
 *     changes no bit.  A tomo_dff_load under a budget gives back a block that an earlier, larger budget left.  The partials of (a) and (d), the weights of a call and G live in the handle too (tomo_dff_device_bytes).
 *
 * Everything is enqueued on the caller-given stream (in practice the tomo context's, tomo_ctx_stream); tomo_dff_gram and tomo_dff_cost
 * hand results to the host and wait for it.
 *
 * TOMO_DFF_ERR_UNSUPPORTED, before anything is allocated or launched, with the reason in the message: K outside 2 ... TOMO_DFF_MAX_FLATS;
 * m outside 0 ... TOMO_DFF_MAX_EFF or m > K - 1; bin outside 1 ... TOMO_DFF_MAX_BIN or rows / bin < 2 or cols / bin < 2; a frame of 2^31
 * pixels or more.
 *
 * A handle owns one device, its buffers and the last error; one handle is used by one thread at a time.  Every entry point returns a
 * tomo_dff_status and checks its arguments before it launches anything; on failure tomo_dff_last_error(h) says why (h may be NULL for
 * errors raised before a handle exists).
 */
#ifndef TOMO_DFF_H
#define TOMO_DFF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(TOMO_DFF_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif

#define TOMO_DFF_MAX_FLATS 128  /* K */
#define TOMO_DFF_MAX_EFF 8      /* m */
#define TOMO_DFF_MAX_BIN 8
#define TOMO_DFF_TILE_Z 16      /* binned rows of one work-group of tomo_dff_cost */
#define TOMO_DFF_TILE_X 64      /* binned columns of it */
#define TOMO_DFF_MAX_IDS 65535  /* projections one tomo_dff_cost lists: the y extent of a grid */

typedef enum {
    TOMO_DFF_OK = 0,
    TOMO_DFF_ERR_ARG = 1,          /* bad argument */
    TOMO_DFF_ERR_HIP = 2,          /* a HIP runtime call failed */
    TOMO_DFF_ERR_NODEV = 3,        /* no HIP device */
    TOMO_DFF_ERR_UNSUPPORTED = 4   /* a size the library does not handle */
} tomo_dff_status;

typedef enum { TOMO_DFF_U16 = 0, TOMO_DFF_F32 = 1 } tomo_dff_dtype;

typedef struct tomo_dff tomo_dff;

TOMO_API int tomo_dff_abi_version(void);
TOMO_API int tomo_dff_create(int device, tomo_dff **h);
TOMO_API int tomo_dff_destroy(tomo_dff *h);
TOMO_API const char *tomo_dff_last_error(tomo_dff *h);
/* TOMO_DFF_ERR_UNSUPPORTED for K flats, m EFFs, frames of rows x cols and a bin factor beyond the limits above; needs no handle or
 * device. */
TOMO_API int tomo_dff_check(int K, int m, int rows, int cols, int bin);
/* The pixels of a chunk of (a) for K flats.  Needs no handle or device. */
TOMO_API int tomo_dff_gram_chunk(int K, int *chunk);
/* Bytes of Rb one projection needs, and the projections per batch under a budget (0: no limit).  Need no handle or device. */
TOMO_API int tomo_dff_scratch_bytes(int rows, int cols, int bin, size_t *bytes);
TOMO_API int tomo_dff_batch(int n, int rows, int cols, int bin, size_t max_scratch_bytes, int *batch);
/* The budget of Rb for the calls that follow (0, the default: no limit). */
TOMO_API int tomo_dff_set_max_scratch(tomo_dff *h, size_t max_scratch_bytes);
/* device bytes the handle holds between calls */
TOMO_API int tomo_dff_device_bytes(tomo_dff *h, int64_t *bytes);
/* (a): G, K K doubles on the host, of the K device flats and the device frame fbar; waits for the stream. */
TOMO_API int tomo_dff_gram(tomo_dff *h, void *stream, const void *d_flats, int dtype, int K, int rows, int cols, const float *d_fbar, double *G);
/* (b): d_eff[m][rows][cols] from the host table V[K][m]; m = 0 does nothing. */
TOMO_API int tomo_dff_eff(tomo_dff *h, void *stream, const void *d_flats, int dtype, int K, int rows, int cols, const float *d_fbar,
                          const double *V, int m, float *d_eff);
/* (c): d_out[n][rows / bin][cols / bin] of the n device frames d_src; d_dark may be NULL. */
TOMO_API int tomo_dff_bin(tomo_dff *h, void *stream, const void *d_src, int dtype, int n, int rows, int cols, int bin, const float *d_dark,
                          float *d_out);
/* (c) into the scratch: Rb of the projections i0 ... i0 + nb - 1 of the stack d_raw (its first frame is projection 0); nb is at most
 * tomo_dff_batch under the handle's budget.  What was loaded before is gone. */
TOMO_API int tomo_dff_load(tomo_dff *h, void *stream, const void *d_raw, int dtype, int i0, int nb, int rows, int cols, int bin,
                           const float *d_dark);
/* (d): for the nids loaded projections ids[] (host; any order, i0 <= id < i0 + nb), w[nids][m], s[nids] and a[m + 1] (host, float32):
 * fg[nids][1 + m] doubles on the host, f then g_0 ... g_(m-1); waits for the stream.  d_Fb, d_Eb[m]: binned as tomo_dff_load was. */
TOMO_API int tomo_dff_cost(tomo_dff *h, void *stream, int nids, const int *ids, const float *w, const float *s, const float *a, int m, float eps,
                           const float *d_Fb, const float *d_Eb, double *fg);
/* (e): the sinogram d_out (n, x1 - x0, z1 - z0) of the n device frames d_raw; w[n][m] float32 on the host (may be NULL where m = 0). */
TOMO_API int tomo_dff_apply(tomo_dff *h, void *stream, const void *d_raw, int dtype, int n, int rows, int cols, const float *d_fbar,
                            const float *d_dark, const float *d_eff, int m, const float *w, int z0, int z1, int x0, int x1, int use_cutoff,
                            float cutoff, int minus_log, float min_ratio, float *d_out);

#ifdef __cplusplus
}
#endif
#endif
