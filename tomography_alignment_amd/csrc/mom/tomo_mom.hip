// libtomo_mom.so: both marginals of every projection of p[n][nx][nz] (z fastest) in one read of p (include/tomo_mom.h,
// tomography_alignment_amd/align/consistency.py) on gfx950.
//
// k_marginals  a work-group is 256 lanes along z, four consecutive z to a lane, and owns (tile of TX columns x, chunk of CZ rows z,
//              projection).  A row of the tile is one instruction per lane: a 16-byte load (VEC: nz % 4 == 0 and p 16-byte aligned,
//              so every lane's address is) or four guarded 4-byte loads of the same elements; U rows are in flight.  A lane keeps
//              four float64 column sums over the tile's x in order (the partial of Z, written once at the end) and adds its four
//              values of a row in float64, the wave by a fixed shuffle tree, lane 0 to LDS; after the loop lane r adds the four waves
//              of row r in order and writes the partial of Q.  Non-finite values are counted per lane, reduced the same way.
//              Lanes with no z inside the window load nothing, and a wave with none skips the rows.  Where nz <= 512 (256) two (one)
//              waves span z; the others would idle, so the waves form 2 (4) groups, each with a contiguous half (quarter) of the
//              tile's rows and a partial of Z of its own.  The split depends on nz only.
// k_fold       one thread per value of Z, of Q and of bad of a batch: a projection's partials added in index order.
// No atomics.  The grid is (tiles, chunks, projections of the batch): what a projection's sums go through depends on (nx, nz) only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>

#include "../../../include/tomo_mom.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_MOM_ERR_ARG, SIDE_ERR_HIP = TOMO_MOM_ERR_HIP, SIDE_ERR_NODEV = TOMO_MOM_ERR_NODEV;
}
#include "../tomo_side_host.h"

namespace {

constexpr int TPB = 256;
constexpr int TX = TOMO_MOM_TILE_X, CZ = TOMO_MOM_CHUNK_Z;
constexpr int U = 4;                               // rows of a tile whose loads are in flight together
constexpr int MAX_BATCH = 65535;                   // projections of one batch: the z extent of a grid
constexpr long long MAX_FOLD = 1LL << 31;          // values one k_fold launch writes
static_assert(CZ == 4 * TPB && TX <= TPB && (TX / 4) % U == 0, "a lane owns four z of its chunk; lane r finishes row r of the tile");

struct Shape {
    int nx, nz, ntile, nchunk, z0, z1;
    int ng;      // row groups of a work-group: 1, or for nz <= 512 / 256, where two / one wave spans z, 2 / 4 (groups_of)
};

// ---------------------------------------------------------------------------------------------------------------------- kernels

template <bool VEC>
__global__ __launch_bounds__(TPB) void k_marginals(const float *__restrict__ p, Shape g, double floor, double *__restrict__ zpart,
                                                   double *__restrict__ qpart, int *__restrict__ badpart) {
    __shared__ double sq[TX][TPB / 64];
    __shared__ int sbad[TPB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x, chunk = blockIdx.y;
    const long long proj = blockIdx.z;
    const int wz = (TPB / 64) / g.ng;                                    // waves along z: 4, 2 or 1
    const int zpos = wave & (wz - 1), grp = wave / wz;
    const int zw = chunk * CZ + 256 * zpos;                              // the wave's first z
    const int z = zw + 4 * lane;
    const int rg = TX / g.ng;                                            // rows of a group
    const int x0 = tile * TX + grp * rg;
    const int rows = max(0, min(rg, g.nx - x0));
    const bool any = z < g.z1 && z + 4 > g.z0;                           // some of z ... z + 3 is inside the window (z1 <= nz)
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) in[k] = z + k >= g.z0 && z + k < g.z1;
    const float *base = p + (proj * g.nx + x0) * g.nz + z;               // dereferenced only where `any`, i.e. z < nz, and r < rows
    double za[4] = {0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    if (!(zw < g.z1 && zw + 256 > g.z0)) {                               // nothing of the wave is inside the window: its sums are zeros
        for (int r = lane; r < rows; r += 64) sq[grp * rg + r][zpos] = 0.0;
    } else {
        for (int r = 0; r < rows; r += U) {
            float f[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int k = 0; k < 4; ++k) f[u][k] = 0.f;
                if (any && r + u < rows) {
                    const float *row = base + (long long)(r + u) * g.nz;
                    if (VEC) {                                           // nz % 4 == 0: z < nz means z + 3 < nz
                        const float4 t = *reinterpret_cast<const float4 *>(row);
                        f[u][0] = t.x, f[u][1] = t.y, f[u][2] = t.z, f[u][3] = t.w;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (in[k]) f[u][k] = row[k];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (r + u < rows) {                                      // uniform over the wave
                    double d[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float v = f[u][k];
                        const bool fin = fabsf(v) <= FLT_MAX;            // false for NaN and +-inf
                        bad += (in[k] && !fin) ? 1 : 0;
                        d[k] = (in[k] && fin && (double)v >= floor) ? (double)v : 0.0;
                        za[k] += d[k];
                    }
                    double s = ((d[0] + d[1]) + d[2]) + d[3];
#pragma unroll
                    for (int w = 32; w >= 1; w >>= 1) s += __shfl_down(s, w, 64);
                    if (lane == 0) sq[grp * rg + r + u][zpos] = s;
                }
            }
        }
    }
    if (z < g.nz) {
        double *out = zpart + ((proj * g.ntile + tile) * g.ng + grp) * g.nz + z;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (z + k < g.nz) out[k] = za[k];
    }
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) bad += __shfl_down(bad, w, 64);
    if (lane == 0) sbad[wave] = bad;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < TX && tile * TX + t < g.nx) {                                // row t of the tile: its group's waves along z, in order
        double s = sq[t][0];
        for (int j = 1; j < wz; ++j) s += sq[t][j];
        qpart[(proj * g.nchunk + chunk) * g.nx + tile * TX + t] = s;
    }
    if (t == 0) badpart[(proj * g.ntile + tile) * g.nchunk + chunk] = ((sbad[0] + sbad[1]) + sbad[2]) + sbad[3];
}

__global__ __launch_bounds__(TPB) void k_fold(const double *__restrict__ zpart, const double *__restrict__ qpart, const int *__restrict__ badpart,
                                              Shape g, int b, double *__restrict__ Z, double *__restrict__ Q, int *__restrict__ bad) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long nZ = (long long)b * g.nz, nQ = (long long)b * g.nx;
    if (idx < nZ) {
        const long long i = idx / g.nz;
        const int z = (int)(idx - i * g.nz);
        double s = 0.0;
        const int nslab = g.ntile * g.ng;
        for (int t = 0; t < nslab; ++t) s += zpart[(i * nslab + t) * g.nz + z];
        Z[idx] = s;
    } else if (idx < nZ + nQ) {
        const long long j = idx - nZ;
        const long long i = j / g.nx;
        const int x = (int)(j - i * g.nx);
        double s = 0.0;
        for (int c = 0; c < g.nchunk; ++c) s += qpart[(i * g.nchunk + c) * g.nx + x];
        Q[j] = s;
    } else if (idx < nZ + nQ + b) {
        const long long i = idx - nZ - nQ;
        const long long m = (long long)g.ntile * g.nchunk;
        int s = 0;
        for (long long k = 0; k < m; ++k) s += badpart[i * m + k];
        bad[i] = s;
    }
}

}  // namespace

struct tomo_mom {
    int device = 0;
    std::string err;
    size_t max_scratch = 0;          // 0: no limit
    int n = 0, nx = 0, nz = 0;       // of the last tomo_mom_marginals; n = 0 before it
    Buf zpart, qpart, badpart;       // double [batch][ntile * ng][nz], double [batch][nchunk][nx], int [batch][ntile][nchunk]
    Buf Q, Z, bad;                   // double [n][nx], double [n][nz], int [n]
    auto bufs() { return std::array{&zpart, &qpart, &badpart, &Q, &Z, &bad}; }
};

namespace {

int check_shape(tomo_mom *h, int n, int nx, int nz, int z0, int z1) {
    if (n < 1 || nx < 1 || nz < 1 || nz > TOMO_MOM_MAX_NZ)
        return fail(h, TOMO_MOM_ERR_UNSUPPORTED, "tomo_mom: " + std::to_string(n) + " projections of " + std::to_string(nx) + " x " + std::to_string(nz) +
                                                     " are outside 1 <= n, 1 <= nx, 1 <= nz <= " + std::to_string(TOMO_MOM_MAX_NZ) + "; nothing was launched");
    if (z0 < 0 || z0 >= z1 || z1 > nz)
        return fail(h, TOMO_MOM_ERR_UNSUPPORTED, "tomo_mom: the window [" + std::to_string(z0) + ", " + std::to_string(z1) + ") is not 0 <= z0 < z1 <= nz = " +
                                                     std::to_string(nz) + "; nothing was launched");
    return TOMO_MOM_OK;
}

inline int tiles_of(int nx) { return (int)(((long long)nx + TX - 1) / TX); }
inline int chunks_of(int nz) { return (nz + CZ - 1) / CZ; }
inline int groups_of(int nz) { return nz <= 256 ? 4 : nz <= 512 ? 2 : 1; }   // waves that z does not need split the tile's rows instead

size_t scratch_bytes(int nx, int nz) {
    const size_t nt = (size_t)tiles_of(nx), nc = (size_t)chunks_of(nz);
    return sizeof(double) * (size_t)nz * nt * (size_t)groups_of(nz) + sizeof(double) * (size_t)nx * nc + sizeof(int) * nt * nc;
}

int batch_for(int n, int nx, int nz, size_t budget) {
    long long b = n;
    if (budget) b = std::min<long long>(b, (long long)(budget / scratch_bytes(nx, nz)));
    b = std::min<long long>(b, MAX_BATCH);
    b = std::min<long long>(b, MAX_FOLD / ((long long)nx + nz + 1));
    return (int)std::max<long long>(b, 1);
}

}  // namespace

extern "C" {

TOMO_API int tomo_mom_abi_version(void) { return 1; }

TOMO_API int tomo_mom_create(int device, tomo_mom **out) {
    return create_plain(device, true, out);
}

TOMO_API int tomo_mom_destroy(tomo_mom *h) {
    if (!h) return TOMO_MOM_OK;
    (void)hipSetDevice(h->device);
    free_bufs(h->bufs());
    delete h;
    return TOMO_MOM_OK;
}

TOMO_API const char *tomo_mom_last_error(tomo_mom *h) { return last_error(h); }

TOMO_API int tomo_mom_check_shape(int n, int nx, int nz, int z0, int z1) { return check_shape(nullptr, n, nx, nz, z0, z1); }

TOMO_API int tomo_mom_scratch_bytes(int nx, int nz, size_t *bytes) {
    if (!bytes) return fail(nullptr, TOMO_MOM_ERR_ARG, "tomo_mom_scratch_bytes: NULL");
    CHK(check_shape(nullptr, 1, nx, nz, 0, nz));
    *bytes = scratch_bytes(nx, nz);
    return TOMO_MOM_OK;
}

TOMO_API int tomo_mom_batch(int n, int nx, int nz, size_t max_scratch_bytes, int *batch) {
    if (!batch) return fail(nullptr, TOMO_MOM_ERR_ARG, "tomo_mom_batch: NULL");
    CHK(check_shape(nullptr, n, nx, nz, 0, nz));
    *batch = batch_for(n, nx, nz, max_scratch_bytes);
    return TOMO_MOM_OK;
}

TOMO_API int tomo_mom_set_max_scratch(tomo_mom *h, size_t max_scratch_bytes) {
    if (!h) return fail(h, TOMO_MOM_ERR_ARG, "tomo_mom_set_max_scratch: NULL handle");
    h->max_scratch = max_scratch_bytes;
    return TOMO_MOM_OK;
}

TOMO_API int tomo_mom_device_bytes(tomo_mom *h, int64_t *bytes) {
    if (!h || !bytes) return fail(h, TOMO_MOM_ERR_ARG, "tomo_mom_device_bytes: NULL");
    *bytes = (int64_t)buf_bytes(h->bufs());
    return TOMO_MOM_OK;
}

TOMO_API int tomo_mom_fetch(tomo_mom *h, void *stream, double *Q, double *Z, int *bad) {
    if (!h) return fail(h, TOMO_MOM_ERR_ARG, "tomo_mom_fetch: NULL handle");
    if (h->n == 0) return fail(h, TOMO_MOM_ERR_ARG, "tomo_mom_fetch: no marginals were computed (tomo_mom_marginals)");
    if (!Q || !Z || !bad) return fail(h, TOMO_MOM_ERR_ARG, "tomo_mom_fetch: NULL pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(Q, h->Q.p, sizeof(double) * (size_t)h->n * h->nx, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(Z, h->Z.p, sizeof(double) * (size_t)h->n * h->nz, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(bad, h->bad.p, sizeof(int) * (size_t)h->n, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return TOMO_MOM_OK;
}

TOMO_API int tomo_mom_marginals(tomo_mom *h, void *stream, const float *d_p, int n, int nx, int nz, double floor, int z0, int z1, double *Q,
                                double *Z, int *bad) {
    if (!h) return fail(h, TOMO_MOM_ERR_ARG, "tomo_mom_marginals: NULL handle");
    if (!d_p) return fail(h, TOMO_MOM_ERR_ARG, "tomo_mom_marginals: NULL pointer");
    if (reinterpret_cast<uintptr_t>(d_p) & 3u) return fail(h, TOMO_MOM_ERR_ARG, "tomo_mom_marginals: misaligned pointer");
    if (std::isnan(floor)) return fail(h, TOMO_MOM_ERR_ARG, "tomo_mom_marginals: floor is NaN (-inf switches the threshold off)");
    const bool to_host = Q || Z || bad;
    if (to_host && !(Q && Z && bad)) return fail(h, TOMO_MOM_ERR_ARG, "tomo_mom_marginals: Q, Z and bad must be all NULL or all given");
    CHK(check_shape(h, n, nx, nz, z0, z1));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    h->n = 0;                                      // nothing is there to fetch until everything below is enqueued
    Shape g{nx, nz, tiles_of(nx), chunks_of(nz), z0, z1, groups_of(nz)};
    const int b = batch_for(n, nx, nz, h->max_scratch);
    // a grow frees the old block: hipFree waits for the device, so nothing in flight still uses it
    CHK(grow(h, h->zpart, sizeof(double) * (size_t)b * g.ntile * g.ng * nz));
    CHK(grow(h, h->qpart, sizeof(double) * (size_t)b * g.nchunk * nx));
    CHK(grow(h, h->badpart, sizeof(int) * (size_t)b * g.ntile * g.nchunk));
    CHK(grow(h, h->Q, sizeof(double) * (size_t)n * nx));
    CHK(grow(h, h->Z, sizeof(double) * (size_t)n * nz));
    CHK(grow(h, h->bad, sizeof(int) * (size_t)n));
    const bool vec = nz % 4 == 0 && (reinterpret_cast<uintptr_t>(d_p) & 15u) == 0;
    for (int i0 = 0; i0 < n; i0 += b) {
        const int bb = std::min(b, n - i0);
        const float *src = d_p + (size_t)i0 * nx * nz;
        const dim3 grid((unsigned)g.ntile, (unsigned)g.nchunk, (unsigned)bb);
        if (vec)
            hipLaunchKernelGGL(k_marginals<true>, grid, dim3(TPB), 0, st, src, g, floor, (double *)h->zpart.p, (double *)h->qpart.p, (int *)h->badpart.p);
        else
            hipLaunchKernelGGL(k_marginals<false>, grid, dim3(TPB), 0, st, src, g, floor, (double *)h->zpart.p, (double *)h->qpart.p, (int *)h->badpart.p);
        HIPCHK(h, hipGetLastError());
        const long long values = (long long)bb * ((long long)nx + nz + 1);
        hipLaunchKernelGGL(k_fold, dim3((unsigned)((values + TPB - 1) / TPB)), dim3(TPB), 0, st, (const double *)h->zpart.p, (const double *)h->qpart.p,
                           (const int *)h->badpart.p, g, bb, static_cast<double *>(h->Z.p) + (size_t)i0 * nz, static_cast<double *>(h->Q.p) + (size_t)i0 * nx,
                           static_cast<int *>(h->bad.p) + i0);
        HIPCHK(h, hipGetLastError());
    }
    h->n = n, h->nx = nx, h->nz = nz;
    if (to_host) return tomo_mom_fetch(h, stream, Q, Z, bad);
    return TOMO_MOM_OK;
}

}  // extern "C"
