// libtomo_fsc.so: Fourier shell / ring correlation of device-resident volumes and stacks (tomography_alignment_amd/resolution.py) on gfx950.
// The transforms are hipFFT R2C plans, in place in padded buffers; everything else is the kernels below.
//
// k_mask_sums<DIM>   first stage of the mask-weighted mean: a fixed grid of SUM_G blocks per plane writes block partials of sum(m v)
//                    and sum(m) in float64; the second stage is a fixed tree over those SUM_G partials inside k_prepare.
// k_prepare<DIM>     one thread per voxel: float32((v - mean) m) into the padded FFT buffer.
// k_shell<DIM>       the radial histogram.  Along a row of the half-spectrum (kx, ky fixed, kz = 0 .. nz/2) the shell index does not
//                    decrease.  A work-group is ONE wave: it owns a contiguous range of rows (of one plane for DIM 2), walks each in
//                    chunks of 64 kz -- lane l loads A and B at kz = c + l as float2, lane-contiguous -- and reduces every run of equal
//                    shells within the chunk by a segmented shuffle reduction in a fixed tree (strides 1, 2, .. 32; a lane adds the
//                    value `stride` lanes up if that lane has the same shell).  The first lane of a run then adds the run's four totals
//                    to the work-group's accumulators in LDS, 4 (S) doubles; runs of one chunk have distinct shells, so no two lanes
//                    touch one accumulator, and the chunks of a wave follow each other in program order.  The order of every addition is
//                    thus fixed by the shape alone.  The work-group stores its table; the grid is a function of the shape only.
// k_shell_final      adds the work-groups' tables in index order.  No atomics anywhere.
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "../../../include/tomo_fsc.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_FSC_ERR_ARG, SIDE_ERR_HIP = TOMO_FSC_ERR_HIP, SIDE_ERR_NODEV = TOMO_FSC_ERR_NODEV, SIDE_ERR_FFT = TOMO_FSC_ERR_FFT;
}
#include "../tomo_side_host.h"
#include "../tomo_side_fft.h"
#include "../tomo_side_reduce.h"

namespace {

constexpr int TPB = 256;             // threads per block of the streaming kernels
constexpr int SUM_G = 256;           // blocks per plane of the first-stage sums (== TPB: the second stage is one partial per thread)
constexpr int WAVE = 64;             // k_shell: one wave per work-group
constexpr int SHELL_WGS = 2048;      // k_shell: at most this many work-groups (partial tables); a constant, so the sums do not depend on the device

struct Shape {
    int ndim, nb, nx, ny, nz;        // ny == 1 for ndim 2
    int nzh;                         // nz / 2 + 1 complex values per row
    int nmax, S;                     // the longest axis; the number of shells, min(n) / 2 + 1
    int exact;                       // every nmax / n_i is an integer: the shell index in integer arithmetic
    int kz_nyq;                      // nz / 2 for even nz, else -1
    long long rows;                  // rows of one plane: nx * ny
    long long rows_per_wg;
    int wgs;                         // work-groups per plane
};

// ---------------------------------------------------------------------------------------------------------------------- kernels

// The mask at voxel (ix, iy, iz) of a plane (linear index i within the plane), float64.
template <int DIM>
__device__ inline double mask_at(const Mask &m, const Shape &g, long long i) {
    if (m.mode == TOMO_FSC_MASK_NONE) return 1.0;
    if (m.mode == TOMO_FSC_MASK_ARRAY) return (double)m.arr[i];
    const int iz = (int)(i % g.nz);
    const long long row = i / g.nz;
    double dx, dy = 0.0;
    if (DIM == 3) {
        dx = (double)(row / g.ny) - 0.5 * (g.nx - 1);
        dy = (double)(row % g.ny) - 0.5 * (g.ny - 1);
    } else {
        dx = (double)row - 0.5 * (g.nx - 1);
    }
    const double dz = (double)iz - 0.5 * (g.nz - 1);
    return mask_edge(dx * dx + dy * dy + dz * dz, m.R, m.E);
}

// part[(b * SUM_G + blk) * 2 + {0, 1}] = this block's share of sum(m v), sum(m) over plane b.
template <int DIM>
__global__ __launch_bounds__(TPB) void k_mask_sums(const float *__restrict__ v, Shape g, Mask m, double *__restrict__ part) {
    __shared__ double sh[TPB];
    const long long N = g.rows * g.nz;
    const long long b = blockIdx.y;
    const long long chunk = (N + SUM_G - 1) / SUM_G;
    const long long lo = blockIdx.x * chunk, hi = min(N, lo + chunk);
    double smv = 0.0, sm = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += TPB) {
        const double w = mask_at<DIM>(m, g, i);
        smv += w * (double)v[b * N + i];
        sm += w;
    }
    const double t0 = block_sum<TPB>(smv, sh);
    const double t1 = block_sum<TPB>(sm, sh);
    if (threadIdx.x == 0) {
        part[(b * SUM_G + blockIdx.x) * 2] = t0;
        part[(b * SUM_G + blockIdx.x) * 2 + 1] = t1;
    }
}

// out (rows of 2 nzh floats) = float32((v - mean) m); mean from part (NULL: 0).
template <int DIM>
__global__ __launch_bounds__(TPB) void k_prepare(const float *__restrict__ v, Shape g, Mask m, const double *__restrict__ part,
                                                 float *__restrict__ out) {
    __shared__ double sh[TPB];
    const long long N = g.rows * g.nz;
    const long long b = blockIdx.y;
    double mean = 0.0;
    if (part) {
        const double smv = block_sum<TPB>(part[(b * SUM_G + threadIdx.x) * 2], sh);
        const double sm = block_sum<TPB>(part[(b * SUM_G + threadIdx.x) * 2 + 1], sh);
        mean = sm != 0.0 ? smv / sm : 0.0;
    }
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= N) return;
    const double w = mask_at<DIM>(m, g, i);
    const long long row = i / g.nz;
    const int iz = (int)(i % g.nz);
    out[(b * g.rows + row) * (2 * (long long)g.nzh) + iz] = (float)(((double)v[b * N + i] - mean) * w);
}

// The shell of the coefficient at |kx|, |ky| (their integer frequencies' magnitudes) and kz.  Exact form: r2 is an integer,
// s = isqrt(r2), one more if r2 > s^2 + s, i.e. r > s + 1/2.  General form: float64, nothing contracted, so that a host model which
// does the same operations in the same order gets the same index.
__device__ inline int shell_exact(long long r2) {
    long long s = (long long)sqrtf((float)r2);
    while (s * s > r2) --s;
    while ((s + 1) * (s + 1) <= r2) ++s;
    return (int)(s + (r2 > s * s + s ? 1 : 0));
}

__device__ inline double sq_scaled(int k, int nmax, int n) {
#pragma clang fp contract(off)
    const double f = (double)((long long)k * nmax) / (double)n;
    return f * f;
}

__device__ inline int shell_general(double fx2, double fy2, double fz2) {
#pragma clang fp contract(off)
    const double r2 = (fx2 + fy2) + fz2;
    const double r = __dsqrt_rn(r2);
    return (int)floor(r + 0.5);
}

template <int DIM>
__global__ __launch_bounds__(WAVE) void k_shell(const float2 *__restrict__ A, const float2 *__restrict__ B, Shape g, double *__restrict__ part) {
    extern __shared__ double acc[];                  // [4][S]: C, PA, PB, n
    const int lane = threadIdx.x;
    const int S = g.S;
    for (int i = lane; i < 4 * S; i += WAVE) acc[i] = 0.0;
    __syncthreads();
    const long long plane = blockIdx.y;
    const long long row0 = (long long)blockIdx.x * g.rows_per_wg;
    const long long row1 = min(g.rows, row0 + g.rows_per_wg);
    const long long base = plane * g.rows * g.nzh;
    const int sx = g.nmax / g.nx, sy = g.nmax / g.ny, sz = g.nmax / g.nz;      // used by the exact form only (ny = 1 for DIM 2: ky = 0)
    for (long long row = row0; row < row1; ++row) {
        const int ix = DIM == 3 ? (int)(row / g.ny) : (int)row;
        const int iy = DIM == 3 ? (int)(row % g.ny) : 0;
        const int kx = min(ix, g.nx - ix), ky = DIM == 3 ? min(iy, g.ny - iy) : 0;
        long long r2xy = 0;
        double fx2 = 0.0, fy2 = 0.0;
        if (g.exact) {
            const long long a = (long long)kx * sx, b = (long long)ky * sy;
            r2xy = a * a + b * b;
        } else {
            fx2 = sq_scaled(kx, g.nmax, g.nx);
            fy2 = DIM == 3 ? sq_scaled(ky, g.nmax, g.ny) : 0.0;
        }
        const float2 *ra = A + base + row * g.nzh, *rb = B + base + row * g.nzh;
        for (int c0 = 0; c0 < g.nzh; c0 += WAVE) {
            const int kz = c0 + lane;
            const bool live = kz < g.nzh;
            int s = S;                                // the key of everything that is not accumulated: the tail of the row
            double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
            if (live) {
                if (g.exact) {
                    const long long c = (long long)kz * sz;
                    s = shell_exact(r2xy + c * c);
                } else {
                    s = shell_general(fx2, fy2, sq_scaled(kz, g.nmax, g.nz));
                }
                if (s < S) {
                    const float2 a = ra[kz], b = rb[kz];
                    const double w = (kz == 0 || kz == g.kz_nyq) ? 1.0 : 2.0;
                    const double ar = a.x, ai = a.y, br = b.x, bi = b.y;
                    v0 = w * (ar * br + ai * bi);
                    v1 = w * (ar * ar + ai * ai);
                    v2 = w * (br * br + bi * bi);
                    v3 = w;
                } else {
                    s = S;
                }
            }
            // segmented reduction: after the step of stride d a lane holds the sum over itself and the next 2 d - 1 lanes of its run
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) {
                const int so = __shfl_down(s, d, WAVE);
                const double o0 = __shfl_down(v0, d, WAVE), o1 = __shfl_down(v1, d, WAVE);
                const double o2 = __shfl_down(v2, d, WAVE), o3 = __shfl_down(v3, d, WAVE);
                if (lane + d < WAVE && so == s) {
                    v0 += o0;
                    v1 += o1;
                    v2 += o2;
                    v3 += o3;
                }
            }
            const int sp = __shfl_up(s, 1, WAVE);
            if ((lane == 0 || sp != s) && s < S) {
                acc[s] += v0;
                acc[S + s] += v1;
                acc[2 * S + s] += v2;
                acc[3 * S + s] += v3;
            }
            __syncthreads();                          // one wave: orders this chunk's LDS updates before the next chunk's
        }
    }
    double *out = part + (plane * gridDim.x + blockIdx.x) * (long long)(4 * S);
    for (int i = lane; i < 4 * S; i += WAVE) out[i] = acc[i];
}

// table[b][i] = part[b][0][i] + part[b][1][i] + ... in index order; i < 4 S.
__global__ __launch_bounds__(TPB) void k_shell_final(const double *__restrict__ part, int wgs, int n4, double *__restrict__ table) {
    const long long b = blockIdx.y;
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n4) return;
    double t = 0.0;
    for (int w = 0; w < wgs; ++w) t += part[(b * wgs + w) * (long long)n4 + i];
    table[b * n4 + i] = t;
}

template <int VW>
__global__ __launch_bounds__(TPB) void k_take_rows(const float *__restrict__ src, size_t row_v, size_t first, size_t step, size_t total_v,
                                                   float *__restrict__ dst) {
    typedef typename std::conditional<VW == 4, float4, float>::type vec_t;
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total_v) return;
    const size_t r = i / row_v, c = i % row_v;
    reinterpret_cast<vec_t *>(dst)[i] = reinterpret_cast<const vec_t *>(src)[(first + r * step) * row_v + c];
}

}  // namespace

struct tomo_fsc {
    int device = 0;
    std::string err;
    bool shaped = false;
    Shape g{};
    FftPlans<std::tuple<int, int, int, int, int>> plans;   // R2C per (ndim, nb, nx, ny, nz), each with a work area of its own
    FftPlan *plan = nullptr;
    std::vector<void *> areas;       // the plans' work areas, set when a plan is made; a plan's size is its work_bytes
    Buf spec[2], sums, part, table;
    auto bufs() { return std::array{&spec[0], &spec[1], &sums, &part, &table}; }
};

namespace {

int make_shape(tomo_fsc *h, int ndim, int nb, int nx, int ny, int nz, Shape *out) {
    if (ndim != 2 && ndim != 3) return fail(h, TOMO_FSC_ERR_UNSUPPORTED, "tomo_fsc: ndim must be 2 or 3, got " + std::to_string(ndim));
    if (ndim == 2) ny = 1;
    if (ndim == 3 && nb != 1) return fail(h, TOMO_FSC_ERR_UNSUPPORTED, "tomo_fsc: one volume at a time (nb = 1 for ndim 3)");
    if (nb < 1 || nb > TOMO_FSC_MAX_PLANES)
        return fail(h, TOMO_FSC_ERR_UNSUPPORTED, "tomo_fsc: nb must be 1 ... " + std::to_string(TOMO_FSC_MAX_PLANES) + ", got " + std::to_string(nb));
    const int ext[3] = {nx, nz, ny};
    for (int i = 0; i < ndim; ++i)
        if (ext[i] < 2 || ext[i] > TOMO_FSC_MAX_N)
            return fail(h, TOMO_FSC_ERR_UNSUPPORTED, "tomo_fsc: every axis must have 2 ... " + std::to_string(TOMO_FSC_MAX_N) + " values, got " +
                                                         std::to_string(ext[i]));
    const long long total = (long long)nb * nx * ny * nz;
    if (total > 2147483647LL) return fail(h, TOMO_FSC_ERR_UNSUPPORTED, "tomo_fsc: more than 2^31 - 1 values");
    Shape g{};
    g.ndim = ndim, g.nb = nb, g.nx = nx, g.ny = ny, g.nz = nz;
    g.nzh = nz / 2 + 1;
    g.nmax = std::max(nx, nz);
    int nmin = std::min(nx, nz);
    if (ndim == 3) g.nmax = std::max(g.nmax, ny), nmin = std::min(nmin, ny);
    g.S = nmin / 2 + 1;
    g.exact = g.nmax % nx == 0 && g.nmax % nz == 0 && (ndim == 2 || g.nmax % ny == 0);
    g.kz_nyq = nz % 2 == 0 ? nz / 2 : -1;
    g.rows = (long long)nx * ny;
    const long long want = ndim == 3 ? SHELL_WGS : std::max(8, SHELL_WGS / nb);
    g.rows_per_wg = (g.rows + want - 1) / want;
    g.wgs = (int)((g.rows + g.rows_per_wg - 1) / g.rows_per_wg);
    *out = g;
    return TOMO_FSC_OK;
}

size_t spectrum_bytes(const Shape &g) { return sizeof(float2) * (size_t)g.nb * (size_t)g.rows * (size_t)g.nzh; }

// One 3-D transform, or nb 2-D ones, with the work area they ask for.
int make_plan(tomo_fsc *h, const Shape &g, FftPlan &p) {
    const hipfftResult r = new_plan(&p.fwd, &p.work_bytes, [&](hipfftHandle f, size_t *ws) {
        if (g.ndim == 3) return hipfftMakePlan3d(f, g.nx, g.ny, g.nz, HIPFFT_R2C, ws);
        int n[2] = {g.nx, g.nz};
        return hipfftMakePlanMany(f, 2, n, nullptr, 1, 0, nullptr, 1, 0, HIPFFT_R2C, g.nb, ws);
    });
    if (r != HIPFFT_SUCCESS) return fail(h, TOMO_FSC_ERR_FFT, "hipfft R2C plan: hipfft error " + std::to_string((int)r));
    if (!p.work_bytes) return TOMO_FSC_OK;
    void *work = nullptr;
    const hipError_t e = hipMalloc(&work, p.work_bytes);
    const hipfftResult w = e == hipSuccess ? hipfftSetWorkArea(p.fwd, work) : HIPFFT_SUCCESS;
    if (e != hipSuccess || w != HIPFFT_SUCCESS) {
        if (e == hipSuccess) (void)hipFree(work);
        release(p);
        return e != hipSuccess ? fail(h, TOMO_FSC_ERR_HIP, std::string("hipMalloc of the hipFFT work area: ") + hipGetErrorString(e))
                               : fail(h, TOMO_FSC_ERR_FFT, "hipfftSetWorkArea: hipfft error " + std::to_string((int)w));
    }
    h->areas.push_back(work);
    return TOMO_FSC_OK;
}

int ready(tomo_fsc *h, const char *who) {
    if (!h) return fail(h, TOMO_FSC_ERR_ARG, std::string(who) + ": NULL handle");
    if (!h->shaped) return fail(h, TOMO_FSC_ERR_ARG, std::string(who) + ": call tomo_fsc_set_shape first");
    return TOMO_FSC_OK;
}

inline dim3 grid1(long long n, int b) { return dim3((unsigned)((n + TPB - 1) / TPB), (unsigned)b); }

}  // namespace

extern "C" {

TOMO_API int tomo_fsc_abi_version(void) { return 1; }

TOMO_API int tomo_fsc_create(int device, tomo_fsc **out) {
    return create_plain(device, false, out);
}

TOMO_API int tomo_fsc_destroy(tomo_fsc *h) {
    if (!h) return TOMO_FSC_OK;
    (void)hipSetDevice(h->device);
    h->plans.destroy_all();
    for (void *w : h->areas) (void)hipFree(w);
    free_bufs(h->bufs());
    delete h;
    return TOMO_FSC_OK;
}

TOMO_API const char *tomo_fsc_last_error(tomo_fsc *h) { return last_error(h); }

TOMO_API int tomo_fsc_n_shells(int ndim, int nb, int nx, int ny, int nz, int *n_shells) {
    if (!n_shells) return fail(nullptr, TOMO_FSC_ERR_ARG, "tomo_fsc_n_shells: NULL");
    Shape g{};
    CHK(make_shape(nullptr, ndim, nb, nx, ny, nz, &g));
    *n_shells = g.S;
    return TOMO_FSC_OK;
}

TOMO_API int tomo_fsc_set_shape(tomo_fsc *h, int ndim, int nb, int nx, int ny, int nz) {
    if (!h) return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_set_shape: NULL handle");
    Shape g{};
    CHK(make_shape(h, ndim, nb, nx, ny, nz, &g));
    HIPCHK(h, hipSetDevice(h->device));
    h->shaped = false;
    CHK(h->plans.get(std::make_tuple(g.ndim, g.nb, g.nx, g.ny, g.nz), [&](FftPlan &p) { return make_plan(h, g, p); }, &h->plan));
    CHK(grow(h, h->spec[0], spectrum_bytes(g)));
    CHK(grow(h, h->spec[1], spectrum_bytes(g)));
    CHK(grow(h, h->sums, sizeof(double) * 2 * SUM_G * (size_t)g.nb));
    CHK(grow(h, h->part, sizeof(double) * 4 * (size_t)g.S * (size_t)g.wgs * (size_t)g.nb));
    CHK(grow(h, h->table, sizeof(double) * 4 * (size_t)g.S * (size_t)g.nb));
    h->g = g;
    h->shaped = true;
    return TOMO_FSC_OK;
}

TOMO_API int tomo_fsc_device_bytes(tomo_fsc *h, int64_t *bytes) {
    if (!h || !bytes) return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_device_bytes: NULL");
    size_t t = buf_bytes(h->bufs());
    for (auto &kv : h->plans.plans) t += kv.second.work_bytes;
    *bytes = (int64_t)t;
    return TOMO_FSC_OK;
}

TOMO_API int tomo_fsc_plan_seconds(tomo_fsc *h, double *seconds) {
    if (!h || !seconds) return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_plan_seconds: NULL");
    *seconds = h->plans.seconds;
    return TOMO_FSC_OK;
}

TOMO_API int tomo_fsc_prepare(tomo_fsc *h, void *stream, int slot, const float *d_vol, int mask, const float *d_mask, double radius,
                              double edge, int subtract_mean) {
    CHK(ready(h, "tomo_fsc_prepare"));
    if (slot != 0 && slot != 1) return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_prepare: slot must be 0 or 1");
    if (!d_vol) return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_prepare: NULL volume");
    if (mask != TOMO_FSC_MASK_NONE && mask != TOMO_FSC_MASK_ARRAY && mask != TOMO_FSC_MASK_SPHERE)
        return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_prepare: unknown mask mode");
    if (mask == TOMO_FSC_MASK_ARRAY && !d_mask) return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_prepare: NULL mask array");
    if (mask == TOMO_FSC_MASK_SPHERE && !(radius >= 0.0 && edge >= 0.0 && radius < 1e9 && edge < 1e9))
        return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_prepare: the sphere needs a finite radius >= 0 and edge >= 0");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Shape &g = h->g;
    const Mask m{mask, d_mask, radius, edge};
    const long long N = g.rows * g.nz;
    double *part = subtract_mean ? (double *)h->sums.p : nullptr;
    float *out = (float *)h->spec[slot].p;
    if (g.ndim == 3) {
        if (part) hipLaunchKernelGGL(k_mask_sums<3>, dim3(SUM_G, g.nb), dim3(TPB), 0, st, d_vol, g, m, part);
        hipLaunchKernelGGL(k_prepare<3>, grid1(N, g.nb), dim3(TPB), 0, st, d_vol, g, m, (const double *)part, out);
    } else {
        if (part) hipLaunchKernelGGL(k_mask_sums<2>, dim3(SUM_G, g.nb), dim3(TPB), 0, st, d_vol, g, m, part);
        hipLaunchKernelGGL(k_prepare<2>, grid1(N, g.nb), dim3(TPB), 0, st, d_vol, g, m, (const double *)part, out);
    }
    HIPCHK(h, hipGetLastError());
    return TOMO_FSC_OK;
}

TOMO_API int tomo_fsc_fft(tomo_fsc *h, void *stream, int slot) {
    CHK(ready(h, "tomo_fsc_fft"));
    if (slot != 0 && slot != 1) return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_fft: slot must be 0 or 1");
    HIPCHK(h, hipSetDevice(h->device));
    FFTCHK(h, hipfftSetStream(h->plan->fwd, reinterpret_cast<hipStream_t>(stream)));       // the work area was set with the plan
    FFTCHK(h, hipfftExecR2C(h->plan->fwd, (hipfftReal *)h->spec[slot].p, (hipfftComplex *)h->spec[slot].p));
    return TOMO_FSC_OK;
}

TOMO_API int tomo_fsc_reduce(tomo_fsc *h, void *stream) {
    CHK(ready(h, "tomo_fsc_reduce"));
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Shape &g = h->g;
    const size_t lds = sizeof(double) * 4 * (size_t)g.S;
    const float2 *A = (const float2 *)h->spec[0].p, *B = (const float2 *)h->spec[1].p;
    double *part = (double *)h->part.p, *table = (double *)h->table.p;
    if (g.ndim == 3)
        hipLaunchKernelGGL(k_shell<3>, dim3(g.wgs, g.nb), dim3(WAVE), lds, st, A, B, g, part);
    else
        hipLaunchKernelGGL(k_shell<2>, dim3(g.wgs, g.nb), dim3(WAVE), lds, st, A, B, g, part);
    hipLaunchKernelGGL(k_shell_final, grid1(4 * g.S, g.nb), dim3(TPB), 0, st, (const double *)part, g.wgs, 4 * g.S, table);
    HIPCHK(h, hipGetLastError());
    return TOMO_FSC_OK;
}

TOMO_API int tomo_fsc_fetch(tomo_fsc *h, void *stream, double *out) {
    CHK(ready(h, "tomo_fsc_fetch"));
    if (!out) return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_fetch: NULL");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipMemcpyAsync(out, h->table.p, sizeof(double) * 4 * (size_t)h->g.S * (size_t)h->g.nb, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return TOMO_FSC_OK;
}

TOMO_API int tomo_fsc_take_rows(tomo_fsc *h, void *stream, const float *d_src, size_t row_elems, size_t first, size_t step, size_t count,
                                float *d_dst) {
    if (!h) return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_take_rows: NULL handle");
    if (row_elems < 1 || step < 1) return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_take_rows: row_elems and step must be >= 1");
    if (count == 0) return TOMO_FSC_OK;
    if (!d_src || !d_dst) return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_take_rows: NULL pointer");
    const bool v4 = row_elems % 4 == 0 && ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) & 15u) == 0;
    const size_t row_v = v4 ? row_elems / 4 : row_elems, total_v = row_v * count;
    const size_t blocks = (total_v + TPB - 1) / TPB;
    if (blocks >= (1ull << 31)) return fail(h, TOMO_FSC_ERR_ARG, "tomo_fsc_take_rows: too many work-groups");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (v4)
        hipLaunchKernelGGL(k_take_rows<4>, dim3((unsigned)blocks), dim3(TPB), 0, st, d_src, row_v, first, step, total_v, d_dst);
    else
        hipLaunchKernelGGL(k_take_rows<1>, dim3((unsigned)blocks), dim3(TPB), 0, st, d_src, row_v, first, step, total_v, d_dst);
    HIPCHK(h, hipGetLastError());
    return TOMO_FSC_OK;
}

}  // extern "C"
