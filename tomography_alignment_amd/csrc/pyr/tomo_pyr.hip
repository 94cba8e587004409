// libtomo_pyr.so: binning and prolongation for the resolution pyramid (tomography_alignment_amd/multires.py) on gfx950.  All three
// kernels stream: z is contiguous in every layout, each input value is read from HBM once and each output written once.
//
// k_bin<F, VW, VOL>   one thread per VW (4, or 2 where nz is not a multiple of 4) adjacent z values of one OUTPUT row: it reads the
//                     F (sinogram) or F x F (volume) input rows of that output row at the same z, lane-contiguous (16 B per lane, a
//                     wave reads 1 KiB of a row per instruction), and adds them per column in float64; the F columns of a bin are then
//                     added within the thread (F <= VW) or with the neighbouring lane (F = 8), and float32(S * c) is stored.
// k_prolong<W>        a work-group stages a 4 x 8 x 32 block of coarse cells plus a one-cell halo (indices clamped to the volume, which
//                     is the clamp of the interpolation rule) in LDS and writes the 8 x 16 x 64 fine cells it determines, W (4, or 2
//                     for an odd coarse nz) adjacent z values per thread and store.
#include <hip/hip_runtime.h>

#include <string>

#include "../../../include/tomo_pyr.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_PYR_ERR_ARG, SIDE_ERR_HIP = TOMO_PYR_ERR_HIP, SIDE_ERR_NODEV = TOMO_PYR_ERR_NODEV;
}
#include "../tomo_side_host.h"

namespace {

constexpr int BIN_T = 256;
constexpr int PRO_T = 256;
constexpr int PRO_CX = 4, PRO_CY = 8, PRO_CZ = 32;                         // coarse cells per work-group
constexpr int PRO_LX = PRO_CX + 2, PRO_LY = PRO_CY + 2, PRO_LZ = PRO_CZ + 2;   // with the halo

template <int VW>
struct vec_of;
template <>
struct vec_of<4> { typedef float4 type; };
template <>
struct vec_of<2> { typedef float2 type; };

template <int F, int VW, bool VOL>
__global__ __launch_bounds__(BIN_T) void k_bin(const float *__restrict__ src, float *__restrict__ dst, size_t n_rows_out, int nyo, int nz,
                                               double c) {
    typedef typename vec_of<VW>::type vec_t;
    const int nzv = nz / VW, nzo = nz / F;
    const size_t total = n_rows_out * (size_t)nzv;
    const size_t g = (size_t)blockIdx.x * BIN_T + threadIdx.x;
    const bool live = g < total;                     // no early return: the F = 8 form exchanges sums between neighbouring lanes
    const size_t r = live ? g / nzv : 0;
    const int zv = live ? (int)(g % nzv) : 0;
    // output row r = (X, Y) of the volume (or row r of the sinogram, X = 0): its input rows are (X F + a) ny + Y F + b
    const size_t X = VOL ? r / nyo : 0, Y = VOL ? r % nyo : r;
    const size_t ny = (size_t)nyo * F;
    double s[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) s[k] = 0.0;
    if (live) {
        for (int a = 0; a < (VOL ? F : 1); ++a) {
#pragma unroll
            for (int b = 0; b < F; ++b) {
                const size_t row = (X * F + a) * ny + Y * F + b;
                const vec_t v = *reinterpret_cast<const vec_t *>(src + row * (size_t)nz + (size_t)zv * VW);
                const float *pv = reinterpret_cast<const float *>(&v);
#pragma unroll
                for (int k = 0; k < VW; ++k) s[k] += (double)pv[k];
            }
        }
    }
    float *out = dst + r * (size_t)nzo;
    if (F == 8) {                                    // VW = 4: lanes 2 m and 2 m + 1 hold the two halves of one bin (nzv is even)
        double t = (s[0] + s[1]) + (s[2] + s[3]);
        t += __shfl_xor(t, 1);
        if (live && !(zv & 1)) out[zv >> 1] = (float)(t * c);
    } else if (F == VW) {
        double t = s[0];
#pragma unroll
        for (int k = 1; k < VW; ++k) t += s[k];
        if (live) out[zv] = (float)(t * c);
    } else {                                         // F = 2, VW = 4: two bins per thread
        if (live) *reinterpret_cast<float2 *>(out + 2 * (size_t)zv) = make_float2((float)((s[0] + s[1]) * c), (float)((s[2] + s[3]) * c));
    }
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ float lerp14(float near, float far) { return near + 0.25f * (far - near); }

template <int W>
__global__ __launch_bounds__(PRO_T) void k_prolong(const float *__restrict__ src, float *__restrict__ dst, int nx, int ny, int nz, int tiles_y,
                                                   int tiles_z, float scale) {
    __shared__ float sh[PRO_LX * PRO_LY * PRO_LZ];
    const int tz = blockIdx.x % tiles_z, ty = (blockIdx.x / tiles_z) % tiles_y, tx = blockIdx.x / (tiles_z * tiles_y);
    const int cx0 = tx * PRO_CX, cy0 = ty * PRO_CY, cz0 = tz * PRO_CZ;
    for (int e = threadIdx.x; e < PRO_LX * PRO_LY * PRO_LZ; e += PRO_T) {
        const int lz = e % PRO_LZ, ly = (e / PRO_LZ) % PRO_LY, lx = e / (PRO_LZ * PRO_LY);
        const int gx = clampi(cx0 + lx - 1, nx - 1), gy = clampi(cy0 + ly - 1, ny - 1), gz = clampi(cz0 + lz - 1, nz - 1);
        sh[e] = src[((size_t)gx * ny + gy) * nz + gz];
    }
    __syncthreads();
    constexpr int MZ = 2 * PRO_CZ / W;               // stores along z per fine row of the block
    constexpr int NC = W / 2 + 2;                    // coarse z cells W fine cells depend on
    const int fnx = 2 * nx, fny = 2 * ny, fnz = 2 * nz;
    for (int it = threadIdx.x; it < 2 * PRO_CX * 2 * PRO_CY * MZ; it += PRO_T) {
        const int m = it % MZ, fj = (it / MZ) % (2 * PRO_CY), fi = it / (MZ * 2 * PRO_CY);
        const int i = 2 * cx0 + fi, j = 2 * cy0 + fj, k0 = 2 * cz0 + W * m;
        if (i >= fnx || j >= fny || k0 >= fnz) continue;          // W divides fnz, so k0 < fnz means k0 + W <= fnz
        // local coarse indices (the halo shifts them by one): the near cell, and the neighbour on the side the fine cell lies on
        const int xn = (fi >> 1) + 1, xf = xn + ((fi & 1) ? 1 : -1);
        const int yn = (fj >> 1) + 1, yf = yn + ((fj & 1) ? 1 : -1);
        const int zb = (W / 2) * m;                  // local index of the coarse cell before the first near cell
        float cz[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const float nn = sh[(xn * PRO_LY + yn) * PRO_LZ + zb + q], fn = sh[(xf * PRO_LY + yn) * PRO_LZ + zb + q];
            const float nf = sh[(xn * PRO_LY + yf) * PRO_LZ + zb + q], ff = sh[(xf * PRO_LY + yf) * PRO_LZ + zb + q];
            cz[q] = lerp14(lerp14(nn, fn), lerp14(nf, ff));       // x, then y
        }
        float o[W];
#pragma unroll
        for (int p = 0; p < W; ++p) {                // fine k0 + p: near cell zb + 1 + p / 2, far one before (p even) or after (p odd)
            const int qn = 1 + (p >> 1);
            o[p] = scale * lerp14(cz[qn], cz[(p & 1) ? qn + 1 : qn - 1]);
        }
        float *out = dst + ((size_t)i * fny + j) * fnz + k0;
        if constexpr (W == 4)
            *reinterpret_cast<float4 *>(out) = make_float4(o[0], o[1], o[2], o[3]);
        else
            *reinterpret_cast<float2 *>(out) = make_float2(o[0], o[1]);
    }
}

}  // namespace

struct tomo_pyr {
    int device = 0;
    std::string err;
};

namespace {


bool overlap(const float *a, size_t na, const float *b, size_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb * sizeof(float) && b0 < a0 + na * sizeof(float);
}

// what bin_sino and bin_vol share: n_rows_out output rows of nz / f values, each from f (sinogram) or f x f (volume) input rows
template <bool VOL>
int launch_bin(tomo_pyr *h, hipStream_t st, const float *src, float *dst, size_t n_rows_out, int nyo, int nz, int f, double c) {
    const int vw = (nz % 4 == 0) ? 4 : 2;            // f = 4, 8 divide nz, so vw = 2 only occurs with f = 2
    const size_t total = n_rows_out * (size_t)(nz / vw);
    const size_t blocks = (total + BIN_T - 1) / BIN_T;
    if (blocks >= (1ull << 31)) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_bin: too many work-groups");
    const dim3 grid((unsigned)blocks), block(BIN_T);
    if (f == 2 && vw == 2)
        hipLaunchKernelGGL((k_bin<2, 2, VOL>), grid, block, 0, st, src, dst, n_rows_out, nyo, nz, c);
    else if (f == 2)
        hipLaunchKernelGGL((k_bin<2, 4, VOL>), grid, block, 0, st, src, dst, n_rows_out, nyo, nz, c);
    else if (f == 4)
        hipLaunchKernelGGL((k_bin<4, 4, VOL>), grid, block, 0, st, src, dst, n_rows_out, nyo, nz, c);
    else
        hipLaunchKernelGGL((k_bin<8, 4, VOL>), grid, block, 0, st, src, dst, n_rows_out, nyo, nz, c);
    HIPCHK(h, hipGetLastError());
    return TOMO_PYR_OK;
}

int check_factor(tomo_pyr *h, const char *who, int f, const int *ext, int n_ext) {
    if (f != 2 && f != 4 && f != 8) return fail(h, TOMO_PYR_ERR_UNSUPPORTED, std::string(who) + ": f must be 2, 4 or 8, got " + std::to_string(f));
    for (int i = 0; i < n_ext; ++i)
        if (ext[i] % f) return fail(h, TOMO_PYR_ERR_UNSUPPORTED, std::string(who) + ": f = " + std::to_string(f) + " does not divide the extent " +
                                                                     std::to_string(ext[i]));
    return TOMO_PYR_OK;
}

}  // namespace

extern "C" {

TOMO_API int tomo_pyr_abi_version(void) { return 1; }

TOMO_API int tomo_pyr_create(int device, tomo_pyr **out) {
    return create_plain(device, false, out);
}

TOMO_API int tomo_pyr_destroy(tomo_pyr *h) {
    delete h;
    return TOMO_PYR_OK;
}

TOMO_API const char *tomo_pyr_last_error(tomo_pyr *h) { return last_error(h); }

TOMO_API int tomo_pyr_bin_sino(tomo_pyr *h, void *stream, const float *d_src, int n, int nx, int nz, int f, float scale, float *d_dst) {
    if (!h) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_bin_sino: NULL handle");
    if (n < 0 || nx < 1 || nz < 1) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_bin_sino: bad shape");
    const int ext[2] = {nx, nz};
    if (int rc = check_factor(h, "tomo_pyr_bin_sino", f, ext, 2)) return rc;
    if (n == 0) return TOMO_PYR_OK;
    if (!d_src || !d_dst) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_bin_sino: NULL pointer");
    if (!aligned(d_src, 16) || !aligned(d_dst, 16)) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_bin_sino: buffers must be 16-byte aligned");
    const size_t n_in = (size_t)n * nx * nz, n_out = n_in / ((size_t)f * f);
    if (overlap(d_src, n_in, d_dst, n_out)) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_bin_sino: source and destination overlap");
    HIPCHK(h, hipSetDevice(h->device));
    return launch_bin<false>(h, reinterpret_cast<hipStream_t>(stream), d_src, d_dst, (size_t)n * (nx / f), 1, nz, f,
                             (double)scale / (double)(f * f));
}

TOMO_API int tomo_pyr_bin_vol(tomo_pyr *h, void *stream, const float *d_src, int nx, int ny, int nz, int f, float scale, float *d_dst) {
    if (!h) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_bin_vol: NULL handle");
    if (nx < 1 || ny < 1 || nz < 1) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_bin_vol: bad shape");
    const int ext[3] = {nx, ny, nz};
    if (int rc = check_factor(h, "tomo_pyr_bin_vol", f, ext, 3)) return rc;
    if (!d_src || !d_dst) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_bin_vol: NULL pointer");
    if (!aligned(d_src, 16) || !aligned(d_dst, 16)) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_bin_vol: buffers must be 16-byte aligned");
    const size_t n_in = (size_t)nx * ny * nz, n_out = n_in / ((size_t)f * f * f);
    if (overlap(d_src, n_in, d_dst, n_out)) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_bin_vol: source and destination overlap");
    HIPCHK(h, hipSetDevice(h->device));
    return launch_bin<true>(h, reinterpret_cast<hipStream_t>(stream), d_src, d_dst, (size_t)(nx / f) * (ny / f), ny / f, nz, f,
                            (double)scale / (double)(f * f * f));
}

TOMO_API int tomo_pyr_prolong_vol(tomo_pyr *h, void *stream, const float *d_src, int nx, int ny, int nz, float scale, float *d_dst) {
    if (!h) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_prolong_vol: NULL handle");
    if (nx < 1 || ny < 1 || nz < 1 || nx > (1 << 29) || ny > (1 << 29) || nz > (1 << 29))
        return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_prolong_vol: bad shape");
    if (!d_src || !d_dst) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_prolong_vol: NULL pointer");
    if (!aligned(d_src, 16) || !aligned(d_dst, 16)) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_prolong_vol: buffers must be 16-byte aligned");
    const size_t n_in = (size_t)nx * ny * nz;
    if (overlap(d_src, n_in, d_dst, 8 * n_in)) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_prolong_vol: source and destination overlap");
    const long long tiles_x = (nx + PRO_CX - 1) / PRO_CX, tiles_y = (ny + PRO_CY - 1) / PRO_CY, tiles_z = (nz + PRO_CZ - 1) / PRO_CZ;
    if (tiles_x * tiles_y * tiles_z >= (1LL << 31)) return fail(h, TOMO_PYR_ERR_ARG, "tomo_pyr_prolong_vol: too many work-groups");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(tiles_x * tiles_y * tiles_z)), block(PRO_T);
    if (nz % 2 == 0)                                 // fine rows of 2 nz values: a multiple of 4, every float4 store is aligned
        hipLaunchKernelGGL(k_prolong<4>, grid, block, 0, st, d_src, d_dst, nx, ny, nz, (int)tiles_y, (int)tiles_z, scale);
    else
        hipLaunchKernelGGL(k_prolong<2>, grid, block, 0, st, d_src, d_dst, nx, ny, nz, (int)tiles_y, (int)tiles_z, scale);
    HIPCHK(h, hipGetLastError());
    return TOMO_PYR_OK;
}

}  // extern "C"
