// libtomo_half.so: the axis of a half-acquisition scan over 2 pi by the fixed-window overlap search, and the stitch of the 2 pi series to
// the pi series of double width (include/tomo_half.h, tomography_alignment_amd/half_acquisition.py) on gfx950.
//
// k_gather   one thread per (angle, column): its values p[angle][column][rows[s]] lie within one or a few cache lines (z is the fastest
//            axis of p); the stores to S[s][angle][column] are lane-contiguous along the column.
// k_colsums  one thread per (row, half, column): the float64 sums of S and S^2 over the h angles of the half, in order.
// k_band     Sab(p) = sum_j G[j][p + j], G the w x nx column Gram of ref and M.  A work-group owns (TP candidates, TJ columns j of ref,
//            row and side); a lane owns four consecutive candidates and keeps their 4 x TJ Gram entries in float64 registers.  TI angles
//            at a time are staged in LDS as float32: the TP + TJ - 1 columns of M the tile needs (read mirrored from S, zeros past the
//            detector) and the TJ columns of ref (zeros past the window).  Per angle a lane reads its 4 + TJ - 1 = 11 values of M as three
//            16-byte LDS loads (lane stride 16 bytes: conflict-free) and ref as two broadcast loads.  A product of two float32 is exact
//            in float64, so each accumulator is the correctly ordered sum over i; the lane then adds its TJ entries of a candidate in
//            order and writes one partial per (tile of j, p).
// k_fold     one thread per (row, side, p): the partials in tile order, the window sums of the column sums in column order, m.
// k_stitch   a work-group owns TC output columns of one projection and one chunk of z; its table entries go through LDS once.  zl lanes
//            (a power of two that depends on nz only) lie along z, four consecutive z to a lane, and 256 / zl columns are in flight.
//            VEC: nz % 4 == 0 and 16-byte aligned pointers, one float4 per access; otherwise guarded 4-byte accesses of the same elements.
// No atomics anywhere.  Every grid depends on the shape only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../../include/tomo_half.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_HALF_ERR_ARG, SIDE_ERR_HIP = TOMO_HALF_ERR_HIP, SIDE_ERR_NODEV = TOMO_HALF_ERR_NODEV;
}
#include "../tomo_side_host.h"

namespace {

constexpr int TPB = 256;
constexpr int TJ = TOMO_HALF_TILE_J, TP = TOMO_HALF_TILE_P, TC = TOMO_HALF_TILE_C;
constexpr int TI = 8;                      // angles staged in LDS at a time
constexpr int MS = TP + 8;                 // floats of a staged row of M: TP + TJ - 1 rounded up to a multiple of 4
constexpr int MAX_GRID_Z = 65535;
static_assert(TP == 4 * TPB && TJ == 8 && MS >= TP + TJ - 1 && MS % 4 == 0 && TI * TJ <= TPB, "a lane owns four candidates and eleven columns of M");
static_assert(sizeof(tomo_half_column) == 32 && TC <= TPB, "a table entry is two 16-byte words");

// ---------------------------------------------------------------------------------------------------------------------- kernels

__global__ __launch_bounds__(TPB) void k_gather(const float *__restrict__ p, int nx, int nz, int n, const int *__restrict__ rows, int ns,
                                                float *__restrict__ S) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long per = (long long)n * nx;
    if (idx >= per) return;
    const float *src = p + idx * nz;
    for (int s = 0; s < ns; ++s) S[s * per + idx] = src[rows[s]];
}

// cs[(r 2 + half) nx + x], cs2 likewise
__global__ __launch_bounds__(TPB) void k_colsums(const float *__restrict__ S, int nr, int n, int nx, double *__restrict__ cs, double *__restrict__ cs2) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= (long long)nr * 2 * nx) return;
    const int x = (int)(idx % nx);
    const long long rh = idx / nx;                       // r 2 + half: the half's first angle is row rh h of S
    const int h = n / 2;
    const float *src = S + rh * h * nx + x;
    double s = 0.0, s2 = 0.0;
    for (int i = 0; i < h; ++i) {
        const double v = (double)src[(long long)i * nx];
        s += v;
        s2 += v * v;
    }
    cs[idx] = s;
    cs2[idx] = s2;
}

// part[((rl 2 + side) njt + jt) np + p]; S points at the batch's first row
__global__ __launch_bounds__(TPB) void k_band(const float *__restrict__ S, int n, int nx, int w, int np, double *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float Ms[TI][MS];
    __shared__ __attribute__((aligned(16))) float Rs[TI][TJ];
    const int t = threadIdx.x;
    const int pb = blockIdx.x * TP, jt = blockIdx.y, jb = jt * TJ;
    const int rl = blockIdx.z >> 1, side = blockIdx.z & 1;
    const int h = n / 2;
    const int off = side == 0 ? nx - w : 0;              // the first column of ref
    const float *A = S + (long long)rl * n * nx, *B = A + (long long)h * nx;
    const int xb = pb + jb;                              // the column of M that Ms[.][0] holds
    double acc[4][TJ];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[q][j] = 0.0;
    for (int ic = 0; ic < h; ic += TI) {
        __syncthreads();                                 // the previous chunk has been read
        for (int e = t; e < TI * MS; e += TPB) {
            const int ti = e / MS, k = e - ti * MS;
            const int i = ic + ti, x = xb + k;           // M[i][x] = S[h + i][nx - 1 - x]
            Ms[ti][k] = (i < h && x < nx) ? B[(long long)i * nx + (nx - 1 - x)] : 0.f;
        }
        if (t < TI * TJ) {
            const int ti = t / TJ, j = t - ti * TJ;
            const int i = ic + ti;
            Rs[ti][j] = (i < h && jb + j < w) ? A[(long long)i * nx + off + jb + j] : 0.f;
        }
        __syncthreads();
#pragma unroll 2
        for (int ti = 0; ti < TI; ++ti) {
            const float4 m0 = *reinterpret_cast<const float4 *>(&Ms[ti][4 * t]);
            const float4 m1 = *reinterpret_cast<const float4 *>(&Ms[ti][4 * t + 4]);
            const float4 m2 = *reinterpret_cast<const float4 *>(&Ms[ti][4 * t + 8]);
            const float4 r0 = *reinterpret_cast<const float4 *>(&Rs[ti][0]);
            const float4 r1 = *reinterpret_cast<const float4 *>(&Rs[ti][4]);
            const double mv[12] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w};
            const double rv[TJ] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < TJ; ++j) acc[q][j] = fma(rv[j], mv[q + j], acc[q][j]);
        }
    }
    double *dst = part + ((long long)blockIdx.z * gridDim.y + jt) * np;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int p = pb + 4 * t + q;
        if (p < np) {
            double s = acc[q][0];
#pragma unroll
            for (int j = 1; j < TJ; ++j) s += acc[q][j];
            dst[p] = s;
        }
    }
}

// m[((r0 + rl) 2 + side) np + p]; cs, cs2 are the whole tables, part the batch's
__global__ __launch_bounds__(TPB) void k_fold(const double *__restrict__ part, const double *__restrict__ cs, const double *__restrict__ cs2, int r0, int nrb,
                                              int n, int nx, int w, int np, int njt, double *__restrict__ m) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= (long long)nrb * 2 * np) return;
    const int p = (int)(idx % np);
    const long long pair = idx / np;                     // rl 2 + side
    const int side = (int)(pair & 1);
    const long long r = r0 + (pair >> 1);
    const int off = side == 0 ? nx - w : 0;
    const double *ca = cs + (r * 2) * nx + off, *ca2 = cs2 + (r * 2) * nx + off;
    const double *cb = cs + (r * 2 + 1) * nx + (nx - 1 - p), *cb2 = cs2 + (r * 2 + 1) * nx + (nx - 1 - p);   // column x of M is nx - 1 - x of S
    double sa = 0.0, saa = 0.0, sb = 0.0, sbb = 0.0, sab = 0.0;
    for (int j = 0; j < w; ++j) {
        sa += ca[j];
        saa += ca2[j];
        sb += cb[-j];
        sbb += cb2[-j];
    }
    for (int t = 0; t < njt; ++t) sab += part[(pair * njt + t) * np + p];
    const double N = (double)(n / 2) * (double)w;
    const double va = N * saa - sa * sa, vb = N * sbb - sb * sb;
    m[(r * 2 + side) * np + p] = (va > 0.0 && vb > 0.0) ? 1.0 - (N * sab - sa * sb) / sqrt(va * vb) : 1.0;
}

// A product feeding an explicit fma, twice: nothing is left for -ffp-contract to fuse, so both access paths of k_stitch give the same bits.
__device__ __forceinline__ float combine(const tomo_half_column &c, float a, float s0, float s1) {
    const float b = __builtin_fmaf(c.f1, s1, c.f0 * s0);
    if (c.flags == TOMO_HALF_A_VALID) return a;
    if (c.flags == TOMO_HALF_B_VALID) return b;
    return __builtin_fmaf(c.wa, a, c.wb * b);
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void k_stitch(const float *__restrict__ p, int h, int nx, int nz, int W, int zl, const tomo_half_column *__restrict__ table,
                                                float *__restrict__ out) {
    __shared__ tomo_half_column tab[TC];
    const int t = threadIdx.x;
    const int jb = blockIdx.y * TC;
    const int i = blockIdx.z;
    if (t < TC && jb + t < W) tab[t] = table[jb + t];
    __syncthreads();
    const int zq = t & (zl - 1), cj = t / zl, cpl = TPB / zl;
    const int z = (blockIdx.x * zl + zq) * 4;
    if (z >= nz) return;
    const float *pa = p + (long long)i * nx * nz + z, *pb = p + ((long long)h + i) * nx * nz + z;
    float *po = out + (long long)i * W * nz + z;
    for (int col = cj; col < TC && jb + col < W; col += cpl) {
        const tomo_half_column c = tab[col];
        const bool av = c.flags & TOMO_HALF_A_VALID, bv = c.flags & TOMO_HALF_B_VALID, two = bv && c.i1 != c.i0;
        const float *ra = pa + (long long)c.ja * nz, *r0 = pb + (long long)c.i0 * nz, *r1 = pb + (long long)c.i1 * nz;
        float *ro = po + (long long)(jb + col) * nz;
        if (VEC) {                                       // nz % 4 == 0: z < nz means z + 3 < nz
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 a = av ? *reinterpret_cast<const float4 *>(ra) : zero;
            const float4 s0 = bv ? *reinterpret_cast<const float4 *>(r0) : zero;
            const float4 s1 = two ? *reinterpret_cast<const float4 *>(r1) : s0;
            *reinterpret_cast<float4 *>(ro) = make_float4(combine(c, a.x, s0.x, s1.x), combine(c, a.y, s0.y, s1.y), combine(c, a.z, s0.z, s1.z),
                                                          combine(c, a.w, s0.w, s1.w));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (z + k < nz) {
                    const float a = av ? ra[k] : 0.f;
                    const float s0 = bv ? r0[k] : 0.f;
                    const float s1 = two ? r1[k] : s0;
                    ro[k] = combine(c, a, s0, s1);
                }
            }
        }
    }
}

}  // namespace

struct tomo_half {
    int device = 0;
    std::string err;
    size_t max_scratch = 0;              // 0: no limit
    int nr = 0, n = 0, nx = 0;           // of the last tomo_half_load; nr = 0 before it
    int w = 0;                           // of the last tomo_half_search; 0 before it
    Buf S, rows, cs, cs2, part, m;       // float [nr][n][nx], int [nr], double [nr][2][nx] twice, double [batch][2][njt][np], double [nr][2][np]
    Buf table;                           // tomo_half_column [W]
    auto bufs() { return std::array{&S, &rows, &cs, &cs2, &part, &m, &table}; }
    std::vector<int> host_rows;          // what the asynchronous copies read
    std::vector<tomo_half_column> host_table;
    bool staging_in_flight = false;
    int table_nx = 0;                    // the table on the device is that of (table_nx, table_c); 0: none
    double table_c = 0.0;
};

namespace {

std::string dims(int n, int nx, int nz) { return std::to_string(n) + " projections of " + std::to_string(nx) + " x " + std::to_string(nz); }

int check_window(tomo_half *h, int nx, int w) {
    if (w < TOMO_HALF_MIN_W || w > nx / 2)
        return fail(h, TOMO_HALF_ERR_UNSUPPORTED, "tomo_half: a window of " + std::to_string(w) + " columns is outside " + std::to_string(TOMO_HALF_MIN_W) +
                                                      " <= w <= nx / 2 = " + std::to_string(nx / 2) + "; nothing was launched");
    return TOMO_HALF_OK;
}

// nrows and w count only where > 0
int check_shape(tomo_half *h, int n, int nx, int nz, int nrows, int w) {
    if (n < 2 || n > TOMO_HALF_MAX_N || n % 2)
        return fail(h, TOMO_HALF_ERR_UNSUPPORTED, "tomo_half: " + dims(n, nx, nz) + ": needs an even 2 <= n <= " + std::to_string(TOMO_HALF_MAX_N) +
                                                      " projections over 2 pi; nothing was launched");
    if (nx < TOMO_HALF_MIN_NX || nx > TOMO_HALF_MAX_NX)
        return fail(h, TOMO_HALF_ERR_UNSUPPORTED, "tomo_half: " + dims(n, nx, nz) + ": needs " + std::to_string(TOMO_HALF_MIN_NX) + " <= nx <= " +
                                                      std::to_string(TOMO_HALF_MAX_NX) + " columns; nothing was launched");
    if (nz < 1 || nz > TOMO_HALF_MAX_NZ)
        return fail(h, TOMO_HALF_ERR_UNSUPPORTED, "tomo_half: " + dims(n, nx, nz) + ": needs 1 <= nz <= " + std::to_string(TOMO_HALF_MAX_NZ) +
                                                      " detector rows; nothing was launched");
    if (nrows > TOMO_HALF_MAX_ROWS)
        return fail(h, TOMO_HALF_ERR_UNSUPPORTED, "tomo_half: " + std::to_string(nrows) + " detector rows in one load, more than " +
                                                      std::to_string(TOMO_HALF_MAX_ROWS) + "; nothing was launched");
    return w > 0 ? check_window(h, nx, w) : TOMO_HALF_OK;
}

int check_center(tomo_half *h, int nx, double c) {
    if (!(c >= 0.0 && c <= (double)(nx - 1)))
        return fail(h, TOMO_HALF_ERR_UNSUPPORTED, "tomo_half: the axis at column " + std::to_string(c) + " is outside 0 <= c <= nx - 1 = " +
                                                      std::to_string(nx - 1) + "; nothing was launched");
    return TOMO_HALF_OK;
}

inline int tiles_j(int w) { return (w + TJ - 1) / TJ; }
inline int tiles_p(int np) { return (np + TP - 1) / TP; }
inline size_t scratch_bytes(int nx, int w) { return sizeof(double) * 2 * (size_t)tiles_j(w) * (size_t)(nx - w + 1); }

int batch_for(int nrows, int nx, int w, size_t budget) {
    long long b = nrows;
    if (budget) b = std::min<long long>(b, (long long)(budget / scratch_bytes(nx, w)));
    b = std::min<long long>(b, MAX_GRID_Z / 2);
    return (int)std::max<long long>(b, 1);
}

struct Stitched {
    int W, j0;
    bool right;
    double g, c_out;
};

Stitched stitched(int nx, double c) {
    Stitched s;
    const double mirror = (double)(nx - 1) - c;
    s.right = c >= mirror;
    s.W = (int)std::floor(2.0 * std::max(c, mirror)) + 1;
    s.j0 = s.right ? 0 : s.W - nx;
    s.g = s.right ? mirror : c;
    s.c_out = c + (double)s.j0;
    return s;
}

void fill_table(int nx, double c, const Stitched &s, tomo_half_column *col, double *f_out, double *wa_out) {
    for (int j = 0; j < s.W; ++j) {
        const int ja = j - s.j0;
        const bool av = ja >= 0 && ja <= nx - 1;
        const double xb = 2.0 * c - (double)ja;
        const bool bv = xb >= 0.0 && xb <= (double)(nx - 1);
        const double fl = std::floor(xb);
        const double f = xb - fl;
        const int i0 = (int)std::min<double>(std::max(fl, 0.0), (double)(nx - 1));
        const int i1 = f > 0.0 ? std::min(i0 + 1, nx - 1) : i0;
        const double u = (double)j - s.c_out;
        double wa = 1.0;
        if (s.g > 0.0) wa = std::min(std::max((s.right ? s.g - u : s.g + u) / (2.0 * s.g), 0.0), 1.0);
        col[j].flags = (av ? TOMO_HALF_A_VALID : 0) | (bv ? TOMO_HALF_B_VALID : 0);
        col[j].ja = std::min(std::max(ja, 0), nx - 1);
        col[j].i0 = i0;
        col[j].i1 = i1;
        col[j].f0 = (float)(1.0 - f);
        col[j].f1 = (float)f;
        col[j].wa = (float)wa;
        col[j].wb = (float)(1.0 - wa);
        if (f_out) f_out[j] = f;
        if (wa_out) wa_out[j] = wa;
    }
}

}  // namespace

extern "C" {

TOMO_API int tomo_half_abi_version(void) { return 1; }

TOMO_API int tomo_half_create(int device, tomo_half **out) {
    return create_plain(device, true, out);
}

TOMO_API int tomo_half_destroy(tomo_half *h) {
    if (!h) return TOMO_HALF_OK;
    (void)hipSetDevice(h->device);
    free_bufs(h->bufs());
    delete h;
    return TOMO_HALF_OK;
}

TOMO_API const char *tomo_half_last_error(tomo_half *h) { return last_error(h); }

TOMO_API int tomo_half_check_shape(int n, int nx, int nz, int nrows, int w) { return check_shape(nullptr, n, nx, nz, nrows, w); }

TOMO_API int tomo_half_stitched_shape(int n, int nx, double c, int *hh, int *W, int *j0, double *c_out) {
    if (!hh || !W || !j0 || !c_out) return fail(nullptr, TOMO_HALF_ERR_ARG, "tomo_half_stitched_shape: NULL");
    CHK(check_shape(nullptr, n, nx, 1, 0, 0));
    CHK(check_center(nullptr, nx, c));
    const Stitched s = stitched(nx, c);
    *hh = n / 2, *W = s.W, *j0 = s.j0, *c_out = s.c_out;
    return TOMO_HALF_OK;
}

TOMO_API int tomo_half_table(int nx, double c, int W, tomo_half_column *columns, double *f, double *wa) {
    if (!columns) return fail(nullptr, TOMO_HALF_ERR_ARG, "tomo_half_table: NULL");
    CHK(check_shape(nullptr, 2, nx, 1, 0, 0));
    CHK(check_center(nullptr, nx, c));
    const Stitched s = stitched(nx, c);
    if (W != s.W) return fail(nullptr, TOMO_HALF_ERR_ARG, "tomo_half_table: the table has " + std::to_string(s.W) + " columns, not " + std::to_string(W));
    fill_table(nx, c, s, columns, f, wa);
    return TOMO_HALF_OK;
}

TOMO_API int tomo_half_scratch_bytes(int nx, int w, size_t *bytes) {
    if (!bytes) return fail(nullptr, TOMO_HALF_ERR_ARG, "tomo_half_scratch_bytes: NULL");
    CHK(check_shape(nullptr, 2, nx, 1, 1, 0));
    CHK(check_window(nullptr, nx, w));
    *bytes = scratch_bytes(nx, w);
    return TOMO_HALF_OK;
}

TOMO_API int tomo_half_batch(int nrows, int nx, int w, size_t max_scratch_bytes, int *batch) {
    if (!batch) return fail(nullptr, TOMO_HALF_ERR_ARG, "tomo_half_batch: NULL");
    if (nrows < 1) return fail(nullptr, TOMO_HALF_ERR_ARG, "tomo_half_batch: needs at least one detector row");
    CHK(check_shape(nullptr, 2, nx, 1, nrows, 0));
    CHK(check_window(nullptr, nx, w));
    *batch = batch_for(nrows, nx, w, max_scratch_bytes);
    return TOMO_HALF_OK;
}

TOMO_API int tomo_half_set_max_scratch(tomo_half *h, size_t max_scratch_bytes) {
    if (!h) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_set_max_scratch: NULL handle");
    h->max_scratch = max_scratch_bytes;
    return TOMO_HALF_OK;
}

TOMO_API int tomo_half_device_bytes(tomo_half *h, int64_t *bytes) {
    if (!h || !bytes) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_device_bytes: NULL");
    *bytes = (int64_t)buf_bytes(h->bufs());
    return TOMO_HALF_OK;
}

TOMO_API int tomo_half_load(tomo_half *h, void *stream, const float *d_p, int n_p, int nx, int nz, int n, const int *rows, int nrows) {
    if (!h) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_load: NULL handle");
    if (!d_p || !rows) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_load: NULL pointer");
    if (reinterpret_cast<uintptr_t>(d_p) & 3u) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_load: misaligned pointer");
    if (nrows < 1) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_load: needs at least one detector row");
    if (n > n_p) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_load: the projections 0 ... n - 1 are not in p");
    CHK(check_shape(h, n, nx, nz, nrows, 0));
    for (int s = 0; s < nrows; ++s)
        if (rows[s] < 0 || rows[s] >= nz) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_load: row " + std::to_string(rows[s]) + " is not in 0 ... nz - 1");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    h->nr = 0, h->w = 0;                           // nothing is loaded until everything below is enqueued
    // a grow frees the old block: hipFree waits for the device, so nothing in flight still uses it
    CHK(grow(h, h->S, sizeof(float) * (size_t)nrows * n * nx));
    CHK(grow(h, h->rows, sizeof(int) * (size_t)nrows));
    if (h->staging_in_flight) HIPCHK(h, hipStreamSynchronize(st));     // a staging vector may still feed an earlier copy
    h->host_rows.assign(rows, rows + nrows);
    h->staging_in_flight = true;
    HIPCHK(h, hipMemcpyAsync(h->rows.p, h->host_rows.data(), sizeof(int) * (size_t)nrows, hipMemcpyHostToDevice, st));
    const long long per = (long long)n * nx;
    hipLaunchKernelGGL(k_gather, dim3((unsigned)((per + TPB - 1) / TPB)), dim3(TPB), 0, st, d_p, nx, nz, n, (const int *)h->rows.p, nrows, (float *)h->S.p);
    HIPCHK(h, hipGetLastError());
    h->nr = nrows, h->n = n, h->nx = nx;
    return TOMO_HALF_OK;
}

TOMO_API int tomo_half_fetch(tomo_half *h, void *stream, double *m) {
    if (!h) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_fetch: NULL handle");
    if (h->nr == 0 || h->w == 0) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_fetch: no curves were computed (tomo_half_search)");
    if (!m) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_fetch: NULL pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(m, h->m.p, sizeof(double) * (size_t)h->nr * 2 * (size_t)(h->nx - h->w + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->staging_in_flight = false;
    return TOMO_HALF_OK;
}

TOMO_API int tomo_half_search(tomo_half *h, void *stream, int w, double *m) {
    if (!h) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_search: NULL handle");
    if (h->nr == 0) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_search: no sinogram is loaded (tomo_half_load)");
    const int nr = h->nr, n = h->n, nx = h->nx;
    CHK(check_window(h, nx, w));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    h->w = 0;
    const int np = nx - w + 1, njt = tiles_j(w);
    const int b = batch_for(nr, nx, w, h->max_scratch);
    CHK(grow(h, h->cs, sizeof(double) * (size_t)nr * 2 * nx));
    CHK(grow(h, h->cs2, sizeof(double) * (size_t)nr * 2 * nx));
    CHK(grow(h, h->part, scratch_bytes(nx, w) * (size_t)b));
    CHK(grow(h, h->m, sizeof(double) * (size_t)nr * 2 * np));
    const long long ncs = (long long)nr * 2 * nx;
    hipLaunchKernelGGL(k_colsums, dim3((unsigned)((ncs + TPB - 1) / TPB)), dim3(TPB), 0, st, (const float *)h->S.p, nr, n, nx, (double *)h->cs.p, (double *)h->cs2.p);
    HIPCHK(h, hipGetLastError());
    for (int r0 = 0; r0 < nr; r0 += b) {
        const int bb = std::min(b, nr - r0);
        hipLaunchKernelGGL(k_band, dim3((unsigned)tiles_p(np), (unsigned)njt, (unsigned)(2 * bb)), dim3(TPB), 0, st,
                           (const float *)h->S.p + (size_t)r0 * n * nx, n, nx, w, np, (double *)h->part.p);
        HIPCHK(h, hipGetLastError());
        const long long values = (long long)bb * 2 * np;
        hipLaunchKernelGGL(k_fold, dim3((unsigned)((values + TPB - 1) / TPB)), dim3(TPB), 0, st, (const double *)h->part.p, (const double *)h->cs.p,
                           (const double *)h->cs2.p, r0, bb, n, nx, w, np, njt, (double *)h->m.p);
        HIPCHK(h, hipGetLastError());
    }
    h->w = w;
    if (m) return tomo_half_fetch(h, stream, m);
    return TOMO_HALF_OK;
}

TOMO_API int tomo_half_debug_sinogram(tomo_half *h, void *stream, int row, float *out) {
    if (!h) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_debug_sinogram: NULL handle");
    if (h->nr == 0) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_debug_sinogram: no sinogram is loaded (tomo_half_load)");
    if (!out || row < 0 || row >= h->nr) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_debug_sinogram: bad argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t per = (size_t)h->n * h->nx;
    HIPCHK(h, hipMemcpyAsync(out, static_cast<const float *>(h->S.p) + per * row, sizeof(float) * per, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->staging_in_flight = false;
    return TOMO_HALF_OK;
}

TOMO_API int tomo_half_stitch(tomo_half *h, void *stream, const float *d_p, int n, int nx, int nz, double c, float *d_out) {
    if (!h) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_stitch: NULL handle");
    if (!d_p || !d_out) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_stitch: NULL pointer");
    const uintptr_t pi = reinterpret_cast<uintptr_t>(d_p), po = reinterpret_cast<uintptr_t>(d_out);
    if ((pi | po) & 3u) return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_stitch: misaligned pointer");
    CHK(check_shape(h, n, nx, nz, 0, 0));
    CHK(check_center(h, nx, c));
    const Stitched s = stitched(nx, c);
    const int hh = n / 2;
    const size_t in_bytes = sizeof(float) * (size_t)n * nx * nz, out_bytes = sizeof(float) * (size_t)hh * s.W * nz;
    if (pi < po + out_bytes && po < pi + in_bytes)
        return fail(h, TOMO_HALF_ERR_ARG, "tomo_half_stitch: out overlaps p: the stitch does not work in place; nothing was launched");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    if (!(h->table_nx == nx && h->table_c == c)) {
        h->table_nx = 0;
        // a grow frees the old block: hipFree waits for the device, so nothing in flight still uses it
        CHK(grow(h, h->table, sizeof(tomo_half_column) * (size_t)s.W));
        if (h->staging_in_flight) HIPCHK(h, hipStreamSynchronize(st)); // a staging vector may still feed an earlier copy
        h->host_table.resize((size_t)s.W);
        fill_table(nx, c, s, h->host_table.data(), nullptr, nullptr);
        h->staging_in_flight = true;
        HIPCHK(h, hipMemcpyAsync(h->table.p, h->host_table.data(), sizeof(tomo_half_column) * (size_t)s.W, hipMemcpyHostToDevice, st));
        h->table_nx = nx, h->table_c = c;
    }
    int zl = 1;
    while (zl < TPB && 4 * zl < nz) zl *= 2;             // lanes along z: a power of two that depends on nz only
    const int zc = (nz + 4 * zl - 1) / (4 * zl);
    const bool vec = nz % 4 == 0 && ((pi | po) & 15u) == 0;
    const dim3 grid((unsigned)zc, (unsigned)((s.W + TC - 1) / TC), (unsigned)hh);
    if (vec)
        hipLaunchKernelGGL(k_stitch<true>, grid, dim3(TPB), 0, st, d_p, hh, nx, nz, s.W, zl, (const tomo_half_column *)h->table.p, d_out);
    else
        hipLaunchKernelGGL(k_stitch<false>, grid, dim3(TPB), 0, st, d_p, hh, nx, nz, s.W, zl, (const tomo_half_column *)h->table.p, d_out);
    HIPCHK(h, hipGetLastError());
    return TOMO_HALF_OK;
}

}  // extern "C"
