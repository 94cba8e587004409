// libtomo_vreg.so: registration of two device-resident volumes by a translation (tomography_alignment_amd/registration.py) on gfx950.
// The transforms are hipFFT R2C / C2R plans, in place in padded buffers; everything else is the kernels below (include/tomo_vreg.h is
// the definition of what they compute).  Vector stores and plain C++ only; no float atomics: every sum and every maximum has a fixed order.
//
// One decomposition serves the streaming kernels: a row (x, y) is cut into groups of four consecutive z and a lane owns a group -- one
// 16-byte load where nz % 4 == 0 and the pointer is 16-byte aligned, four guarded 4-byte loads of the same elements otherwise, so both
// paths give the same bits.
//
// k_mask_sums      first stage of the mask-weighted mean: SUM_G blocks write partials of sum(m v) and sum(m) in float64; the second stage,
//                  k_fold_mean, is tomo_fsc.hip's fixed tree over those partials, done once instead of in every work-group.
// k_prepare        float32((v - mean) m) into the padded row, pad included (two 8-byte stores a group: a padded row starts 8-byte
//                  aligned), and the work-group's float64 sum of the squares written; k_fold_sums adds those partials in a fixed order.
// k_cross_power    P = A conj(B), or its phase, over both half-spectra, two coefficients (16 bytes) a lane; written in place and to the copy.
// k_argmax<T>      (value, index) pairs: a lane folds its elements, a wave folds by a shuffle tree, the waves in order, one partial per
//                  work-group; k_argmax_fold: one work-group folds the partials.  The order "larger value, then smaller index, NaN
//                  never" is total, so the result does not depend on the grid.  The pad columns of a C2R output are skipped.
// k_table          the float64 twiddles of one axis of the refinement, tab[k][j] = w_k exp(2 pi i r / (n u)) by the integer-phase rule,
//                  zero beyond the U candidates and the stored coefficients (so the contractions need no guards on their reads).
// k_up_z<JJ>       T1[kx][ky][jz] = sum_kz P tab_z: a work-group of 256 lanes owns 32 rows of P and all U candidates.  It walks kz in
//                  chunks of KC = 16: the chunk of the 32 rows (complex64) and the matching KC table rows (complex128) are staged in LDS,
//                  lane (jl = lane % 16, rl = lane / 16) keeps 2 rows x JJ candidates (jz = jl + 16 q) of complex128 accumulators.
//                  LDS banks: a 16-lane group of a 16-byte read holds 16 consecutive table entries, 256 contiguous bytes, every bank
//                  once; lanes that share jl read one address (broadcast); the two P rows a 32-lane half reads are 128 bytes apart.
// k_up_y, k_up_x   T2[kx][jy][jz] = sum_ky T1 tab_y, and c_u[jx][jy][jz] = (1 / N) sum_kx Re(T2 tab_x): a lane keeps eight candidates of
//                  the contracted axis for one element of the other two, so what it streams is read U / 8 times.
// k_finish         the eight doubles of fetch, on the device, so that nothing before fetch waits for the host.
// k_ramp_table, k_ramp   the float64 factors exp(-2 pi i k s / n) per axis, and their product with the spectrum and 1 / N.
// k_unpad, k_roll  the padded C2R output to the caller's volume; the integer shift as a copy.  16-byte stores where nz % 4 == 0 and the
//                  destination is 16-byte aligned, guarded 4-byte stores otherwise.
//
// There is no MFMA: P is float32 data whose f32-input MFMA runs at the vector rate, and the accumulation here is float64.
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../../include/tomo_vreg.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_VREG_ERR_ARG, SIDE_ERR_HIP = TOMO_VREG_ERR_HIP, SIDE_ERR_NODEV = TOMO_VREG_ERR_NODEV,
              SIDE_ERR_FFT = TOMO_VREG_ERR_FFT;
}
#include "../tomo_side_host.h"
#include "../tomo_side_fft.h"
#include "../tomo_side_reduce.h"

namespace {

constexpr int TPB = 256;             // threads per block
constexpr int WAVE = 64;
constexpr int SUM_G = 256;           // blocks of the first-stage mean sums (== TPB: the second stage is one partial per thread)
constexpr int GPW = 4 * TPB;         // groups of four a work-group of k_prepare owns
constexpr int ARG_WGS = 2048;        // at most this many work-groups (partials) of k_argmax
constexpr int KC = 16;               // k_up_z: kz of one staged chunk
constexpr int UPZ_ROWS = 32;         // k_up_z: rows of P a work-group owns (2 a lane)
constexpr int JB = 8;                // k_up_y, k_up_x: candidates a lane keeps
constexpr size_t DEFAULT_SCRATCH = (size_t)1 << 30;
constexpr double PI = 3.141592653589793238462643383279502884;

struct Shape {
    int nx, ny, nz;
    int nzh;                         // nz / 2 + 1 complex values per row
    int pitch;                       // 2 nzh floats per padded row
    int kz_nyq;                      // nz / 2 for even nz, else -1
    long long rows;                  // nx * ny
    long long N;                     // nx * ny * nz
    long long M;                     // rows * nzh stored coefficients
};

struct Pair {                        // a candidate of the maximum; i < 0: none yet
    double v;
    long long i;
};

// ---------------------------------------------------------------------------------------------------------------------- kernels

// The mask at voxel (row = ix ny + iy, iz), float64; the edge is tomo_side_reduce.h's.
__device__ inline double mask_at(const Mask &m, const Shape &g, long long row, int iz) {
    if (m.mode == TOMO_VREG_MASK_NONE) return 1.0;
    if (m.mode == TOMO_VREG_MASK_ARRAY) return (double)m.arr[row * g.nz + iz];
    const int r = (int)row;                          // rows <= 2048^2
    const double dx = (double)(r / g.ny) - 0.5 * (g.nx - 1);
    const double dy = (double)(r % g.ny) - 0.5 * (g.ny - 1);
    const double dz = (double)iz - 0.5 * (g.nz - 1);
    return mask_edge(dx * dx + dy * dy + dz * dz, m.R, m.E);
}

// The four values of the group at z of a row of nz floats; elements past the row are 0.  vec: nz % 4 == 0 and the volume is 16-byte aligned.
template <class T>
__device__ inline void load4(const T *row, int z, int nz, bool vec, T (&x)[4]) {
    if (vec) {
        const float4 t = *reinterpret_cast<const float4 *>(row + z);
        x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = z + e < nz ? row[z + e] : T(0);
    }
}

// part[blk * 2 + {0, 1}] = this block's share of sum(m v), sum(m).
__global__ __launch_bounds__(TPB) void k_mask_sums(const float *__restrict__ v, Shape g, Mask m, int vec, double *__restrict__ part) {
    __shared__ double sh[TPB];
    const int GR = (g.nz + 3) / 4;
    const long long total = g.rows * GR;
    const long long chunk = (total + SUM_G - 1) / SUM_G;
    const long long lo = blockIdx.x * chunk, hi = min(total, lo + chunk);
    double smv = 0.0, sm = 0.0;
    constexpr int UN = 8;                            // groups a lane loads before it adds them, in index order: the sums keep their order
    for (long long i0 = lo + threadIdx.x; i0 < hi; i0 += (long long)UN * TPB) {
        float x[UN][4];
        long long row[UN];
        int z[UN];
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            const long long i = i0 + (long long)j * TPB;
            row[j] = (unsigned)i / (unsigned)GR;               // i < rows GR <= 2^31: a 32-bit division
            z[j] = 4 * (int)(i - row[j] * GR);
            if (i < hi) load4(v + row[j] * g.nz, z[j], g.nz, vec != 0, x[j]);
        }
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            if (i0 + (long long)j * TPB >= hi) break;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (z[j] + e < g.nz) {
                    const double w = mask_at(m, g, row[j], z[j] + e);
                    smv += w * (double)x[j][e];
                    sm += w;
                }
        }
    }
    const double t0 = block_sum<TPB>(smv, sh);
    const double t1 = block_sum<TPB>(sm, sh);
    if (threadIdx.x == 0) {
        part[blockIdx.x * 2] = t0;
        part[blockIdx.x * 2 + 1] = t1;
    }
}

// *mean = sum(m v) / sum(m) from the SUM_G partials of k_mask_sums by the fixed tree; 0 where sum(m) is 0.  One work-group.
__global__ __launch_bounds__(TPB) void k_fold_mean(const double *__restrict__ part, double *__restrict__ mean) {
    __shared__ double sh[TPB];
    const double smv = block_sum<TPB>(part[threadIdx.x * 2], sh);
    const double sm = block_sum<TPB>(part[threadIdx.x * 2 + 1], sh);
    if (threadIdx.x == 0) *mean = sm != 0.0 ? smv / sm : 0.0;
}

// out (rows of g.pitch floats) = float32((v - *mean_p) m), the pad as zeros (mean_p NULL: 0); esq[block] = the block's sum of squares of
// what it wrote (NULL: not wanted).  One 64-bit division per work-group, 32-bit ones per group.
__global__ __launch_bounds__(TPB) void k_prepare(const float *__restrict__ v, Shape g, Mask m, int vec, const double *__restrict__ mean_p,
                                                 float *__restrict__ out, double *__restrict__ esq) {
    __shared__ double sh[TPB];
    const double mean = mean_p ? *mean_p : 0.0;
    const int GP = (g.pitch + 3) / 4;
    const long long total = g.rows * GP;
    const long long first = (long long)blockIdx.x * GPW;
    const long long row0 = first / GP;
    const int q0 = (int)(first - row0 * GP);
    double e2 = 0.0;
#pragma unroll
    for (int j = 0; j < GPW / TPB; ++j) {
        const int off = j * TPB + threadIdx.x;
        if (first + off >= total) continue;
        const int q = q0 + off;                       // < GP + GPW
        const long long row = row0 + q / GP;
        const int z = 4 * (q % GP);
        float x[4] = {0.f, 0.f, 0.f, 0.f}, a[4] = {0.f, 0.f, 0.f, 0.f};
        if (z < g.nz) load4(v + row * g.nz, z, g.nz, vec != 0, x);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (z + e < g.nz) {
                a[e] = (float)(((double)x[e] - mean) * mask_at(m, g, row, z + e));
                e2 += (double)a[e] * (double)a[e];
            }
        float *o = out + row * g.pitch + z;          // z is a multiple of 4 and the pitch even: 8-byte aligned, and z + 1 < pitch
        *reinterpret_cast<float2 *>(o) = make_float2(a[0], a[1]);
        if (z + 2 < g.pitch) *reinterpret_cast<float2 *>(o + 2) = make_float2(a[2], a[3]);
    }
    if (esq) {
        const double t = block_sum<TPB>(e2, sh);
        if (threadIdx.x == 0) esq[blockIdx.x] = t;
    }
}

// *dst = part[0] + part[1] + ...: thread t adds t, t + TPB, ... in order, then the fixed tree.  One work-group.
__global__ __launch_bounds__(TPB) void k_fold_sums(const double *__restrict__ part, long long n, double *__restrict__ dst) {
    __shared__ double sh[TPB];
    double t = 0.0;
    for (long long i = threadIdx.x; i < n; i += TPB) t += part[i];
    const double s = block_sum<TPB>(t, sh);
    if (threadIdx.x == 0) *dst = s;
}

__device__ inline float2 cross(float2 a, float2 b, int phase) {
    float2 p = make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
    if (phase) {
        const float m = sqrtf(p.x * p.x + p.y * p.y);
        p = m > 0.f ? make_float2(p.x / m, p.y / m) : make_float2(0.f, 0.f);
    }
    return p;
}

// A <- P = A conj(B) (or P / |P|), and C <- P; M coefficients, two a lane.
__global__ __launch_bounds__(TPB) void k_cross_power(float2 *__restrict__ A, const float2 *__restrict__ B, float2 *__restrict__ C, long long M,
                                                     int phase) {
    const long long i = 2 * ((long long)blockIdx.x * TPB + threadIdx.x);
    if (i + 1 < M) {
        const float4 a = *reinterpret_cast<const float4 *>(A + i), b = *reinterpret_cast<const float4 *>(B + i);
        const float2 p0 = cross(make_float2(a.x, a.y), make_float2(b.x, b.y), phase);
        const float2 p1 = cross(make_float2(a.z, a.w), make_float2(b.z, b.w), phase);
        const float4 p = make_float4(p0.x, p0.y, p1.x, p1.y);
        *reinterpret_cast<float4 *>(A + i) = p;
        *reinterpret_cast<float4 *>(C + i) = p;
    } else if (i < M) {
        const float2 p = cross(A[i], B[i], phase);
        A[i] = p;
        C[i] = p;
    }
}

// Whether candidate (v, i) beats b: NaN never, a larger value does, an equal one with a smaller index does.
__device__ inline bool beats(double v, long long i, const Pair &b) {
    if (i < 0 || v != v) return false;
    return b.i < 0 || v > b.v || (v == b.v && i < b.i);
}
__device__ inline void take(Pair &b, double v, long long i) {
    if (beats(v, i, b)) b.v = v, b.i = i;
}

// The best pair of the block in thread 0: a shuffle tree in every wave, then the waves in order.
__device__ inline Pair block_best(Pair b, Pair *sh) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        const double ov = __shfl_down(b.v, d, WAVE);
        const long long oi = __shfl_down(b.i, d, WAVE);
        take(b, ov, oi);
    }
    if (threadIdx.x % WAVE == 0) sh[threadIdx.x / WAVE] = b;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < TPB / WAVE; ++w) take(b, sh[w].v, sh[w].i);
    return b;
}

// part[block] = the best element of the block's stretch of v: `rows` rows of `len` elements, `pitch` apart; index = row * len + z.
template <class T>
__global__ __launch_bounds__(TPB) void k_argmax(const T *__restrict__ v, long long rows, int len, long long pitch, int vec, Pair *__restrict__ part) {
    __shared__ Pair sh[TPB / WAVE];
    const int GR = (len + 3) / 4;
    const long long total = rows * GR;
    const long long chunk = (total + gridDim.x - 1) / gridDim.x;
    const long long lo = blockIdx.x * chunk, hi = min(total, lo + chunk);
    Pair b{0.0, -1};
    for (long long i = lo + threadIdx.x; i < hi; i += TPB) {
        const long long row = i / GR;
        const int z = 4 * (int)(i % GR);
        T x[4];
        if constexpr (sizeof(T) == 4) {
            load4(v + row * pitch, z, len, vec != 0, x);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = z + e < len ? v[row * pitch + z + e] : T(0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (z + e < len) take(b, (double)x[e], row * len + z + e);
    }
    b = block_best(b, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = b;
}

// *dst = the best of part[0 .. n); none (all NaN): index 0 and NaN.  One work-group.
__global__ __launch_bounds__(TPB) void k_argmax_fold(const Pair *__restrict__ part, int n, Pair *__restrict__ dst) {
    __shared__ Pair sh[TPB / WAVE];
    Pair b{0.0, -1};
    for (int i = threadIdx.x; i < n; i += TPB) take(b, part[i].v, part[i].i);
    b = block_best(b, sh);
    if (threadIdx.x == 0) {
        if (b.i < 0) b.i = 0, b.v = __longlong_as_double(0x7ff8000000000000LL);
        *dst = b;
    }
}

// The signed frequency of index k on an axis of n in fftfreq's convention (Nyquist of an even axis is -n/2).
__device__ inline int signed_k(int k, int n) { return k < (n + 1) / 2 ? k : k - n; }
// The shift of index i on an axis of n.
__device__ inline int wrap_shift(int i, int n) { return i <= n / 2 ? i : i - n; }

// tab[k * JP + j] = w exp(2 pi i r / (n u)), r = (ks (s0 u + j - h)) mod (n u), for k < nk and j < U; 0 for the rest of kpad x JP.
// axis 0, 1: ks signed, w = 1; axis 2: ks = k, w the Hermitian weight.  s0 from the coarse peak on the device.
__global__ __launch_bounds__(TPB) void k_table(double2 *__restrict__ tab, int axis, Shape g, int nk, int kpad, int JP, int U, int u, int h,
                                               const Pair *__restrict__ coarse) {
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
    if (t >= (long long)kpad * JP) return;
    const int k = (int)(t / JP), j = (int)(t % JP);
    double2 o = make_double2(0.0, 0.0);
    if (k < nk && j < U) {
        const long long ci = coarse->i;
        const int n = axis == 0 ? g.nx : axis == 1 ? g.ny : g.nz;
        const int i = axis == 0 ? (int)(ci / ((long long)g.ny * g.nz)) : axis == 1 ? (int)((ci / g.nz) % g.ny) : (int)(ci % g.nz);
        const long long s0 = wrap_shift(i, n);
        const long long ks = axis == 2 ? k : signed_k(k, n);
        const long long nu = (long long)n * u;
        long long r = (ks * (s0 * u + j - h)) % nu;
        if (r < 0) r += nu;
        const double ang = (2.0 * PI * (double)r) / (double)nu;
        const double w = axis == 2 ? ((k == 0 || k == g.kz_nyq) ? 1.0 : 2.0) : 1.0;
        o = make_double2(w * cos(ang), w * sin(ang));
    }
    tab[t] = o;
}

// T1[(row - row0) * U + jz] = sum_kz P[row][kz] tz[kz][jz], rows row0 <= row < row1; tz has ceil(nzh / KC) KC rows of JT = 16 JJ entries.
template <int JJ>
__global__ __launch_bounds__(TPB) void k_up_z(const float2 *__restrict__ P, long long row0, long long row1, int nzh, const double2 *__restrict__ tz,
                                              int U, double2 *__restrict__ T1) {
    constexpr int JT = 16 * JJ;
    __shared__ float2 Ps[UPZ_ROWS][KC];
    __shared__ double2 Ts[KC][JT];
    const int tid = threadIdx.x;
    const int jl = tid % 16, rl = tid / 16;                 // rows rl and rl + 16 of the tile
    const long long base = row0 + (long long)blockIdx.x * UPZ_ROWS;
    double2 acc[2][JJ];
#pragma unroll
    for (int q = 0; q < JJ; ++q) acc[0][q] = acc[1][q] = make_double2(0.0, 0.0);
    for (int kz0 = 0; kz0 < nzh; kz0 += KC) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < UPZ_ROWS * KC / TPB; ++i) {     // the P tile: element e is row e / KC, kz e % KC
            const int e = tid + i * TPB, r = e / KC, k = e % KC;
            const long long row = base + r;
            Ps[r][k] = (row < row1 && kz0 + k < nzh) ? P[row * nzh + kz0 + k] : make_float2(0.f, 0.f);
        }
        const double2 *src = tz + (long long)kz0 * JT;
#pragma unroll
        for (int i = 0; i < JJ; ++i) (&Ts[0][0])[tid + i * TPB] = src[tid + i * TPB];     // KC JT / TPB = JJ entries a lane
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < KC; ++k) {
            const float2 p0 = Ps[rl][k], p1 = Ps[rl + 16][k];
            const double a0 = p0.x, b0 = p0.y, a1 = p1.x, b1 = p1.y;
#pragma unroll
            for (int q = 0; q < JJ; ++q) {
                const double2 e = Ts[k][jl + 16 * q];
                acc[0][q].x += a0 * e.x - b0 * e.y;
                acc[0][q].y += a0 * e.y + b0 * e.x;
                acc[1][q].x += a1 * e.x - b1 * e.y;
                acc[1][q].y += a1 * e.y + b1 * e.x;
            }
        }
    }
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const long long row = base + rl + 16 * rr;
        if (row >= row1) continue;
#pragma unroll
        for (int q = 0; q < JJ; ++q) {
            const int jz = jl + 16 * q;
            if (jz < U) T1[(row - row0) * U + jz] = acc[rr][q];
        }
    }
}

// T2[kx][jy][jz] = sum_ky T1[kx][ky][jz] ty[ky][jy] for the planes kx of a slab (blockIdx.y); ty rows of JP entries, zero past U.
__global__ __launch_bounds__(TPB) void k_up_y(const double2 *__restrict__ T1, int ny, int U, const double2 *__restrict__ ty, int JP,
                                              double2 *__restrict__ T2) {
    const int f = blockIdx.x * TPB + threadIdx.x;
    if (f >= (JP / JB) * U) return;
    const int jg = f / U, jz = f % U;
    const long long kx = blockIdx.y;
    const double2 *t1 = T1 + kx * ny * U + jz;
    double2 acc[JB];
#pragma unroll
    for (int b = 0; b < JB; ++b) acc[b] = make_double2(0.0, 0.0);
    for (int ky = 0; ky < ny; ++ky) {
        const double2 t = t1[(long long)ky * U];
        const double2 *e = ty + (long long)ky * JP + jg * JB;
#pragma unroll
        for (int b = 0; b < JB; ++b) {
            acc[b].x += t.x * e[b].x - t.y * e[b].y;
            acc[b].y += t.x * e[b].y + t.y * e[b].x;
        }
    }
#pragma unroll
    for (int b = 0; b < JB; ++b) {
        const int jy = jg * JB + b;
        if (jy < U) T2[(kx * U + jy) * U + jz] = acc[b];
    }
}

// cu[jx][jy][jz] = (sum_kx Re(T2[kx][jy][jz] tx[kx][jx])) / N, kx in index order.
__global__ __launch_bounds__(TPB) void k_up_x(const double2 *__restrict__ T2, int nx, int U, const double2 *__restrict__ tx, int JP, double N,
                                              double *__restrict__ cu) {
    const long long U2 = (long long)U * U;
    const long long f = (long long)blockIdx.x * TPB + threadIdx.x;
    if (f >= (JP / JB) * U2) return;
    const int jg = (int)(f / U2);
    const long long q = f % U2;
    double acc[JB];
#pragma unroll
    for (int b = 0; b < JB; ++b) acc[b] = 0.0;
    for (int kx = 0; kx < nx; ++kx) {
        const double2 t = T2[kx * U2 + q];
        const double2 *e = tx + (long long)kx * JP + jg * JB;
#pragma unroll
        for (int b = 0; b < JB; ++b) acc[b] += t.x * e[b].x - t.y * e[b].y;
    }
#pragma unroll
    for (int b = 0; b < JB; ++b) {
        const int jx = jg * JB + b;
        if (jx < U) cu[jx * U2 + q] = acc[b] / N;
    }
}

// out[8] of fetch.  u == 1: the coarse peak; else the candidate `fine` of the U^3 grid about it.
__global__ void k_finish(const Pair *__restrict__ coarse, const Pair *__restrict__ fine, Shape g, int u, int U, int h, const double *__restrict__ E,
                         double *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long ci = coarse->i;
    const int i3[3] = {(int)(ci / ((long long)g.ny * g.nz)), (int)((ci / g.nz) % g.ny), (int)(ci % g.nz)};
    const int n3[3] = {g.nx, g.ny, g.nz};
    int j3[3] = {h, h, h};
    if (u > 1) {
        const long long fi = fine->i;
        j3[0] = (int)(fi / ((long long)U * U)), j3[1] = (int)((fi / U) % U), j3[2] = (int)(fi % U);
    }
    for (int a = 0; a < 3; ++a) out[a] = (double)wrap_shift(i3[a], n3[a]) + (double)(j3[a] - h) / (double)u;
    out[3] = u > 1 ? fine->v : coarse->v / (double)g.N;
    out[4] = E[0];
    out[5] = E[1];
    out[6] = (double)ci;
    out[7] = (double)u;
}

// tab[k] = exp(-2 pi i ks s / n), k < nk; the real cos(pi s) at |ks| = n / 2 of an even axis.  half: the z axis, ks = k.
__global__ __launch_bounds__(TPB) void k_ramp_table(double2 *__restrict__ tab, int n, int nk, int half, double s) {
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= nk) return;
    const int ks = half ? k : signed_k(k, n);
    if (n % 2 == 0 && (ks == n / 2 || ks == -(n / 2))) {
        tab[k] = make_double2(cos(PI * s), 0.0);
    } else {
        const double ang = -2.0 * PI * ((double)ks * s / (double)n);
        tab[k] = make_double2(cos(ang), sin(ang));
    }
}

// W[kx][ky][kz] <- float32( ((px py) pz) W / N ), float64 inside.
__global__ __launch_bounds__(TPB) void k_ramp(float2 *__restrict__ W, Shape g, const double2 *__restrict__ px, const double2 *__restrict__ py,
                                              const double2 *__restrict__ pz) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= g.M) return;
    const long long row = i / g.nzh;
    const int kz = (int)(i % g.nzh);
    const double2 a = px[row / g.ny], b = py[row % g.ny], c = pz[kz];
    const double2 ab = make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
    const double2 f = make_double2(ab.x * c.x - ab.y * c.y, ab.x * c.y + ab.y * c.x);
    const float2 w = W[i];
    const double wr = w.x, wi = w.y, N = (double)g.N;
    W[i] = make_float2((float)((wr * f.x - wi * f.y) / N), (float)((wr * f.y + wi * f.x) / N));
}

__device__ inline void store4(float *row, int z, int nz, bool vec, const float (&x)[4]) {
    if (vec) {
        *reinterpret_cast<float4 *>(row + z) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (z + e < nz) row[z + e] = x[e];
    }
}

// dst (rows of nz) = the real columns of W (rows of g.pitch).
__global__ __launch_bounds__(TPB) void k_unpad(const float *__restrict__ W, Shape g, int vec, float *__restrict__ dst) {
    const int GR = (g.nz + 3) / 4;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= g.rows * GR) return;
    const long long row = i / GR;
    const int z = 4 * (int)(i % GR);
    float x[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = z + e < g.nz ? W[row * g.pitch + z + e] : 0.f;
    store4(dst + row * g.nz, z, g.nz, vec != 0, x);
}

// dst[(i + s) mod n] = src[i] on every axis; 0 <= sx < nx and so on.  src and dst do not overlap.
__global__ __launch_bounds__(TPB) void k_roll(const float *__restrict__ src, Shape g, int sx, int sy, int sz, int vec, float *__restrict__ dst) {
    const int GR = (g.nz + 3) / 4;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= g.rows * GR) return;
    const long long row = i / GR;
    const int z = 4 * (int)(i % GR);
    const int x = (int)(row / g.ny), y = (int)(row % g.ny);
    const int xs = x >= sx ? x - sx : x - sx + g.nx, ys = y >= sy ? y - sy : y - sy + g.ny;
    const float *srow = src + ((long long)xs * g.ny + ys) * g.nz;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int zd = z + e;
        const int zs = zd >= sz ? zd - sz : zd - sz + g.nz;
        v[e] = zd < g.nz ? srow[zs] : 0.f;
    }
    store4(dst + row * g.nz, z, g.nz, vec != 0, v);
}

}  // namespace

struct tomo_vreg {
    int device = 0;
    std::string err;
    bool shaped = false;
    Shape g{};
    FftPlans<std::tuple<int, int, int>> plans;     // R2C and C2R per (nx, ny, nz)
    FftPlan *plan = nullptr;
    Buf work;                        // hipFFT's work area, the largest any plan asked for
    Buf spec[2], pcopy;              // the padded buffers of the two slots; the copy of P (and the work buffer of shift)
    Buf sums, esq, apart, small;     // mean partials; E partials; argmax partials; the small results (see Small)
    Buf tab[3], t1, t2, cu, ramp;    // refine's tables and scratch; shift's three tables
    auto bufs() { return std::array{&work, &spec[0], &spec[1], &pcopy, &sums, &esq, &apart, &small, &tab[0], &tab[1], &tab[2], &t1, &t2, &cu, &ramp}; }
    size_t scratch = DEFAULT_SCRATCH;
};

namespace {

struct Small {                       // the layout of h->small
    Pair coarse, fine, user;
    double E[2];
    double mean;
    double out[8];
};

int make_shape(tomo_vreg *h, int nx, int ny, int nz, Shape *out) {
    const int ext[3] = {nx, ny, nz};
    for (int i = 0; i < 3; ++i)
        if (ext[i] < 2 || ext[i] > TOMO_VREG_MAX_N)
            return fail(h, TOMO_VREG_ERR_UNSUPPORTED, "tomo_vreg: every axis must have 2 ... " + std::to_string(TOMO_VREG_MAX_N) + " values, got " +
                                                          std::to_string(ext[i]));
    const long long total = (long long)nx * ny * nz;
    if (total > 2147483647LL) return fail(h, TOMO_VREG_ERR_UNSUPPORTED, "tomo_vreg: more than 2^31 - 1 values");
    Shape g{};
    g.nx = nx, g.ny = ny, g.nz = nz;
    g.nzh = nz / 2 + 1;
    g.pitch = 2 * g.nzh;
    g.kz_nyq = nz % 2 == 0 ? nz / 2 : -1;
    g.rows = (long long)nx * ny;
    g.N = total;
    g.M = g.rows * g.nzh;
    *out = g;
    return TOMO_VREG_OK;
}

int check_upsample(tomo_vreg *h, int u) {
    if (u < 1 || u > TOMO_VREG_MAX_UPSAMPLE)
        return fail(h, TOMO_VREG_ERR_UNSUPPORTED, "tomo_vreg: upsample must be 1 ... " + std::to_string(TOMO_VREG_MAX_UPSAMPLE) + ", got " +
                                                      std::to_string(u));
    return TOMO_VREG_OK;
}

// The in-place 3-D R2C and C2R of a shape; the handle's one work area grows to what they ask for.
int make_plan(tomo_vreg *h, const Shape &g, FftPlan &p) {
    hipfftHandle *hs[2] = {&p.fwd, &p.inv};
    const hipfftType types[2] = {HIPFFT_R2C, HIPFFT_C2R};
    for (int i = 0; i < 2; ++i) {
        size_t ws = 0;
        const hipfftResult r = new_plan(hs[i], &ws, [&](hipfftHandle f, size_t *w) { return hipfftMakePlan3d(f, g.nx, g.ny, g.nz, types[i], w); });
        if (r != HIPFFT_SUCCESS) {
            release(p);
            return fail(h, TOMO_VREG_ERR_FFT, "hipfft 3-D plan: hipfft error " + std::to_string((int)r));
        }
        p.work_bytes = std::max(p.work_bytes, ws);
    }
    const int rc = grow(h, h->work, p.work_bytes);
    if (rc) release(p);
    return rc;
}

int ready(tomo_vreg *h, const char *who) {
    if (!h) return fail(h, TOMO_VREG_ERR_ARG, std::string(who) + ": NULL handle");
    if (!h->shaped) return fail(h, TOMO_VREG_ERR_ARG, std::string(who) + ": call tomo_vreg_set_shape first");
    return TOMO_VREG_OK;
}

inline unsigned blocks(long long n, int per = TPB) { return (unsigned)((n + per - 1) / per); }
inline Small *small(tomo_vreg *h) { return (Small *)h->small.p; }

// (v - mean) m, or v itself, into a padded buffer.  E: where the sum of squares goes (NULL: not wanted).
int launch_prepare(tomo_vreg *h, hipStream_t st, const float *d_vol, const Mask &m, bool subtract_mean, float *out, double *E) {
    const Shape &g = h->g;
    const int vec = g.nz % 4 == 0 && aligned(d_vol, 16);
    double *part = (double *)h->sums.p, *mean = subtract_mean ? &small(h)->mean : nullptr;
    const long long groups = g.rows * ((g.pitch + 3) / 4);
    const unsigned wgs = blocks(groups, GPW);
    if (mean) {
        hipLaunchKernelGGL(k_mask_sums, dim3(SUM_G), dim3(TPB), 0, st, d_vol, g, m, vec, part);
        hipLaunchKernelGGL(k_fold_mean, dim3(1), dim3(TPB), 0, st, (const double *)part, mean);
    }
    hipLaunchKernelGGL(k_prepare, dim3(wgs), dim3(TPB), 0, st, d_vol, g, m, vec, (const double *)mean, out, E ? (double *)h->esq.p : nullptr);
    if (E) hipLaunchKernelGGL(k_fold_sums, dim3(1), dim3(TPB), 0, st, (const double *)h->esq.p, (long long)wgs, E);
    HIPCHK(h, hipGetLastError());
    return TOMO_VREG_OK;
}

template <class T>
int launch_argmax(tomo_vreg *h, hipStream_t st, const T *v, long long rows, int len, long long pitch, int vec, Pair *dst) {
    const long long groups = rows * ((len + 3) / 4);
    const int wgs = (int)std::max<long long>(1, std::min<long long>(ARG_WGS, (groups + TPB - 1) / TPB));
    hipLaunchKernelGGL(k_argmax<T>, dim3(wgs), dim3(TPB), 0, st, v, rows, len, pitch, vec, (Pair *)h->apart.p);
    hipLaunchKernelGGL(k_argmax_fold, dim3(1), dim3(TPB), 0, st, (const Pair *)h->apart.p, wgs, dst);
    HIPCHK(h, hipGetLastError());
    return TOMO_VREG_OK;
}

int exec_r2c(tomo_vreg *h, hipStream_t st, void *buf) {
    FFTCHK(h, hipfftSetStream(h->plan->fwd, st));
    if (h->plan->work_bytes) FFTCHK(h, hipfftSetWorkArea(h->plan->fwd, h->work.p));
    FFTCHK(h, hipfftExecR2C(h->plan->fwd, (hipfftReal *)buf, (hipfftComplex *)buf));
    return TOMO_VREG_OK;
}

int exec_c2r(tomo_vreg *h, hipStream_t st, void *buf) {
    FFTCHK(h, hipfftSetStream(h->plan->inv, st));
    if (h->plan->work_bytes) FFTCHK(h, hipfftSetWorkArea(h->plan->inv, h->work.p));
    FFTCHK(h, hipfftExecC2R(h->plan->inv, (hipfftComplex *)buf, (hipfftReal *)buf));
    return TOMO_VREG_OK;
}

template <int JJ>
void launch_up_z(hipStream_t st, const float2 *P, long long row0, long long row1, int nzh, const double2 *tz, int U, double2 *T1) {
    hipLaunchKernelGGL(k_up_z<JJ>, dim3(blocks(row1 - row0, UPZ_ROWS)), dim3(TPB), 0, st, P, row0, row1, nzh, tz, U, T1);
}

constexpr int JJS[] = {1, 2, 4, 7, 10};        // the instances of k_up_z: the smallest with 16 JJ >= U is used
inline int pick_jj(int U) {
    for (int jj : JJS)
        if (16 * jj >= U) return jj;
    return 0;
}

}  // namespace

extern "C" {

TOMO_API int tomo_vreg_abi_version(void) { return 1; }

TOMO_API int tomo_vreg_create(int device, tomo_vreg **out) {
    return create_plain(device, false, out);
}

TOMO_API int tomo_vreg_destroy(tomo_vreg *h) {
    if (!h) return TOMO_VREG_OK;
    (void)hipSetDevice(h->device);
    h->plans.destroy_all();
    free_bufs(h->bufs());
    delete h;
    return TOMO_VREG_OK;
}

TOMO_API const char *tomo_vreg_last_error(tomo_vreg *h) { return last_error(h); }

TOMO_API int tomo_vreg_check(int nx, int ny, int nz, int upsample) {
    Shape g{};
    CHK(make_shape(nullptr, nx, ny, nz, &g));
    if (upsample != 0) CHK(check_upsample(nullptr, upsample));
    return TOMO_VREG_OK;
}

TOMO_API int tomo_vreg_set_shape(tomo_vreg *h, int nx, int ny, int nz) {
    if (!h) return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_set_shape: NULL handle");
    Shape g{};
    CHK(make_shape(h, nx, ny, nz, &g));
    HIPCHK(h, hipSetDevice(h->device));
    h->shaped = false;
    CHK(h->plans.get(std::make_tuple(nx, ny, nz), [&](FftPlan &p) { return make_plan(h, g, p); }, &h->plan));
    const size_t spec = sizeof(float2) * (size_t)g.M;
    CHK(grow(h, h->spec[0], spec));
    CHK(grow(h, h->spec[1], spec));
    CHK(grow(h, h->pcopy, spec));
    CHK(grow(h, h->sums, sizeof(double) * 2 * SUM_G));
    CHK(grow(h, h->esq, sizeof(double) * (size_t)blocks(g.rows * ((g.pitch + 3) / 4), GPW)));
    CHK(grow(h, h->apart, sizeof(Pair) * ARG_WGS));
    CHK(grow(h, h->ramp, sizeof(double2) * (size_t)(g.nx + g.ny + g.nzh)));
    if (!h->small.p) {
        CHK(grow(h, h->small, sizeof(Small)));
        HIPCHK(h, hipMemset(h->small.p, 0, sizeof(Small)));
    }
    h->g = g;
    h->shaped = true;
    return TOMO_VREG_OK;
}

TOMO_API int tomo_vreg_device_bytes(tomo_vreg *h, int64_t *bytes) {
    if (!h || !bytes) return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_device_bytes: NULL");
    *bytes = (int64_t)buf_bytes(h->bufs());
    return TOMO_VREG_OK;
}

TOMO_API int tomo_vreg_plan_seconds(tomo_vreg *h, double *seconds) {
    if (!h || !seconds) return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_plan_seconds: NULL");
    *seconds = h->plans.seconds;
    return TOMO_VREG_OK;
}

TOMO_API int tomo_vreg_set_scratch_bytes(tomo_vreg *h, size_t bytes) {
    if (!h) return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_set_scratch_bytes: NULL handle");
    h->scratch = bytes ? bytes : DEFAULT_SCRATCH;
    return TOMO_VREG_OK;
}

TOMO_API int tomo_vreg_prepare(tomo_vreg *h, void *stream, int slot, const float *d_vol, int mask, const float *d_mask, double radius,
                               double edge, int subtract_mean) {
    CHK(ready(h, "tomo_vreg_prepare"));
    if (slot != 0 && slot != 1) return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_prepare: slot must be 0 or 1");
    if (!d_vol) return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_prepare: NULL volume");
    if (mask != TOMO_VREG_MASK_NONE && mask != TOMO_VREG_MASK_ARRAY && mask != TOMO_VREG_MASK_SPHERE)
        return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_prepare: unknown mask mode");
    if (mask == TOMO_VREG_MASK_ARRAY && !d_mask) return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_prepare: NULL mask array");
    if (mask == TOMO_VREG_MASK_SPHERE && !(radius >= 0.0 && edge >= 0.0 && radius < 1e9 && edge < 1e9))
        return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_prepare: the sphere needs a finite radius >= 0 and edge >= 0");
    HIPCHK(h, hipSetDevice(h->device));
    const Mask m{mask, d_mask, radius, edge};
    return launch_prepare(h, reinterpret_cast<hipStream_t>(stream), d_vol, m, subtract_mean != 0, (float *)h->spec[slot].p, &small(h)->E[slot]);
}

TOMO_API int tomo_vreg_correlate(tomo_vreg *h, void *stream, int normalization) {
    CHK(ready(h, "tomo_vreg_correlate"));
    if (normalization != TOMO_VREG_NORM_NONE && normalization != TOMO_VREG_NORM_PHASE)
        return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_correlate: unknown normalization");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Shape &g = h->g;
    CHK(exec_r2c(h, st, h->spec[0].p));
    CHK(exec_r2c(h, st, h->spec[1].p));
    hipLaunchKernelGGL(k_cross_power, dim3(blocks((g.M + 1) / 2)), dim3(TPB), 0, st, (float2 *)h->spec[0].p, (const float2 *)h->spec[1].p,
                       (float2 *)h->pcopy.p, g.M, normalization);
    HIPCHK(h, hipGetLastError());
    CHK(exec_c2r(h, st, h->spec[0].p));
    return launch_argmax(h, st, (const float *)h->spec[0].p, g.rows, g.nz, (long long)g.pitch, 0, &small(h)->coarse);
}

TOMO_API int tomo_vreg_refine(tomo_vreg *h, void *stream, int upsample) {
    CHK(ready(h, "tomo_vreg_refine"));
    CHK(check_upsample(h, upsample));
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Shape &g = h->g;
    const int u = upsample, U = (3 * u + 1) / 2, hh = U / 2;
    Small *s = small(h);
    if (u > 1) {
        const int JJ = pick_jj(U), JT = 16 * JJ, JP = JB * ((U + JB - 1) / JB);
        const int kzpad = KC * ((g.nzh + KC - 1) / KC);
        const int nk[3] = {g.nx, g.ny, g.nzh}, kpad[3] = {g.nx, g.ny, kzpad}, jp[3] = {JP, JP, JT};
        const size_t plane = sizeof(double2) * (size_t)g.ny * (size_t)U;                       // T1 of one kx
        const int slab = (int)std::max<size_t>(1, std::min<size_t>((size_t)g.nx, h->scratch / plane));
        for (int a = 0; a < 3; ++a) CHK(grow(h, h->tab[a], sizeof(double2) * (size_t)kpad[a] * (size_t)jp[a]));
        CHK(grow(h, h->t1, plane * (size_t)slab));
        CHK(grow(h, h->t2, sizeof(double2) * (size_t)g.nx * (size_t)U * (size_t)U));
        CHK(grow(h, h->cu, sizeof(double) * (size_t)U * (size_t)U * (size_t)U));
        for (int a = 0; a < 3; ++a)
            hipLaunchKernelGGL(k_table, dim3(blocks((long long)kpad[a] * jp[a])), dim3(TPB), 0, st, (double2 *)h->tab[a].p, a, g, nk[a], kpad[a], jp[a],
                               U, u, hh, (const Pair *)&s->coarse);
        const float2 *P = (const float2 *)h->pcopy.p;
        const double2 *tx = (const double2 *)h->tab[0].p, *ty = (const double2 *)h->tab[1].p, *tz = (const double2 *)h->tab[2].p;
        double2 *T1 = (double2 *)h->t1.p, *T2 = (double2 *)h->t2.p;
        for (int kx0 = 0; kx0 < g.nx; kx0 += slab) {
            const int planes = std::min(slab, g.nx - kx0);
            const long long row0 = (long long)kx0 * g.ny, row1 = row0 + (long long)planes * g.ny;
            switch (JJ) {
                case 1: launch_up_z<1>(st, P, row0, row1, g.nzh, tz, U, T1); break;
                case 2: launch_up_z<2>(st, P, row0, row1, g.nzh, tz, U, T1); break;
                case 4: launch_up_z<4>(st, P, row0, row1, g.nzh, tz, U, T1); break;
                case 7: launch_up_z<7>(st, P, row0, row1, g.nzh, tz, U, T1); break;
                default: launch_up_z<10>(st, P, row0, row1, g.nzh, tz, U, T1); break;
            }
            hipLaunchKernelGGL(k_up_y, dim3(blocks((long long)(JP / JB) * U), planes), dim3(TPB), 0, st, (const double2 *)T1, g.ny, U, ty, JP,
                               T2 + (size_t)kx0 * U * U);
        }
        hipLaunchKernelGGL(k_up_x, dim3(blocks((long long)(JP / JB) * U * U)), dim3(TPB), 0, st, (const double2 *)T2, g.nx, U, tx, JP, (double)g.N,
                           (double *)h->cu.p);
        HIPCHK(h, hipGetLastError());
        CHK(launch_argmax(h, st, (const double *)h->cu.p, 1, U * U * U, (long long)U * U * U, 0, &s->fine));
    }
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(1), 0, st, (const Pair *)&s->coarse, (const Pair *)&s->fine, g, u, U, hh, (const double *)s->E, s->out);
    HIPCHK(h, hipGetLastError());
    return TOMO_VREG_OK;
}

TOMO_API int tomo_vreg_fetch(tomo_vreg *h, void *stream, double *out8) {
    CHK(ready(h, "tomo_vreg_fetch"));
    if (!out8) return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_fetch: NULL");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipMemcpyAsync(out8, small(h)->out, sizeof(double) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return TOMO_VREG_OK;
}

TOMO_API int tomo_vreg_shift(tomo_vreg *h, void *stream, const float *d_src, const double *s3, float *d_dst) {
    CHK(ready(h, "tomo_vreg_shift"));
    if (!d_src || !d_dst || !s3) return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_shift: NULL pointer");
    const Shape &g = h->g;
    const int n3[3] = {g.nx, g.ny, g.nz};
    bool integer = true;
    int roll[3] = {0, 0, 0};
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(s3[a]) || std::fabs(s3[a]) > 1e9) return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_shift: the shift must be finite");
        if (s3[a] != std::rint(s3[a])) integer = false;
        else roll[a] = (int)((((long long)s3[a] % n3[a]) + n3[a]) % n3[a]);
    }
    const char *a0 = (const char *)d_src, *b0 = (const char *)d_dst;
    const size_t bytes = sizeof(float) * (size_t)g.N;
    if (a0 != b0 && a0 < b0 + bytes && b0 < a0 + bytes) return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_shift: src and dst overlap without being equal");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int vec = g.nz % 4 == 0 && aligned(d_dst, 16);
    const unsigned wgs = blocks(g.rows * ((g.nz + 3) / 4));
    if (integer) {
        const float *src = d_src;
        if (a0 == b0) {                                      // in place: from a copy in the work buffer
            HIPCHK(h, hipMemcpyAsync(h->pcopy.p, d_src, bytes, hipMemcpyDeviceToDevice, st));
            src = (const float *)h->pcopy.p;
        }
        hipLaunchKernelGGL(k_roll, dim3(wgs), dim3(TPB), 0, st, src, g, roll[0], roll[1], roll[2], vec, d_dst);
        HIPCHK(h, hipGetLastError());
        return TOMO_VREG_OK;
    }
    float *W = (float *)h->pcopy.p;
    CHK(launch_prepare(h, st, d_src, Mask{TOMO_VREG_MASK_NONE, nullptr, 0.0, 0.0}, false, W, nullptr));
    CHK(exec_r2c(h, st, W));
    double2 *px = (double2 *)h->ramp.p, *py = px + g.nx, *pz = py + g.ny;
    hipLaunchKernelGGL(k_ramp_table, dim3(blocks(g.nx)), dim3(TPB), 0, st, px, g.nx, g.nx, 0, s3[0]);
    hipLaunchKernelGGL(k_ramp_table, dim3(blocks(g.ny)), dim3(TPB), 0, st, py, g.ny, g.ny, 0, s3[1]);
    hipLaunchKernelGGL(k_ramp_table, dim3(blocks(g.nzh)), dim3(TPB), 0, st, pz, g.nz, g.nzh, 1, s3[2]);
    hipLaunchKernelGGL(k_ramp, dim3(blocks(g.M)), dim3(TPB), 0, st, (float2 *)W, g, (const double2 *)px, (const double2 *)py, (const double2 *)pz);
    HIPCHK(h, hipGetLastError());
    CHK(exec_c2r(h, st, W));
    hipLaunchKernelGGL(k_unpad, dim3(wgs), dim3(TPB), 0, st, (const float *)W, g, vec, d_dst);
    HIPCHK(h, hipGetLastError());
    return TOMO_VREG_OK;
}

TOMO_API int tomo_vreg_argmax(tomo_vreg *h, void *stream, const float *d_vol, int64_t *index, float *value) {
    CHK(ready(h, "tomo_vreg_argmax"));
    if (!d_vol || !index || !value) return fail(h, TOMO_VREG_ERR_ARG, "tomo_vreg_argmax: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Shape &g = h->g;
    CHK(launch_argmax(h, st, d_vol, g.rows, g.nz, (long long)g.nz, g.nz % 4 == 0 && aligned(d_vol, 16), &small(h)->user));
    Pair p{};
    HIPCHK(h, hipMemcpyAsync(&p, &small(h)->user, sizeof(Pair), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    *index = (int64_t)p.i;
    *value = (float)p.v;
    return TOMO_VREG_OK;
}

}  // extern "C"
