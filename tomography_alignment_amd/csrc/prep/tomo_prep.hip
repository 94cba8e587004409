// libtomo_prep.so: preprocessing of raw projections (tomography_alignment_amd/preprocess.py) on gfx950.
//
// k_reference_mean     one thread per pixel: a float64 sum over the frames in frame order, / n, rounded once to float32.
// k_reference_median   one thread per pixel, the pixel's n <= 64 values as orderable keys in LDS (column per thread: conflict-free); the
//                      value of rank k is the one whose count of smaller keys is <= k and of smaller-or-equal keys is > k (exact, and the
//                      same value whichever of several equal keys is taken).
// k_normalize          a 64 x 64 (z, x) tile per work-group: frame rows read coalesced along x, normalised on the way into LDS, written
//                      coalesced along z from the transposed tile (row stride 65: the column reads hit distinct banks).
// stripe removal, per chunk of z rows (scratch: sorted values S and median M as float32, the permutation P as uint16, all [rank][x][zl]):
//   k_stripe_sort      (K1) one work-group per x and group of ZC adjacent z columns: the n angles of each column go to LDS as 64-bit
//                      keys (orderable value bits << 32 | angle), padded with ~0 to a power of two Np, and are sorted by a bitonic
//                      network over all ZC segments at once; sorted values and angles are written with rank in place of angle.
//   k_stripe_median    (K2) a z-coalesced stencil: a (64 z) x (64 x) tile plus the reflected halo staged in LDS, one thread per z and
//                      16 x, the window of `size` keys in registers, exact selection by counting.
//   k_stripe_scatter   (K3) the inverse of K1: the filtered values are scattered to their angles in LDS and written coalesced.
// Every key is unique (the angle is part of it), so the sort is the stable order numpy's argsort(kind='stable') gives.
// large and dead stripes (Vo algorithms 5 and 6), per chunk, on top of K1-K3 (a further 13 bytes of scratch per (x, z): three factor
// lists and the mask):
//   k_large_factor     (K4) per (x, z) the float64 means of the sorted and of the smoothed values over the kept ranks, and their ratio.
//   k_dead_diff        (K5) per (x, z) the summed distance of a column from its 10-angle running mean, the window in registers.
//   k_stripe_detect    (K6) per z: the factors sorted in LDS, a float64 line fit through the middle half, two thresholds, dilation.
//   k_large_correct    (K7) K3 with a choice per column: the smoothed value at the angle's rank (masked), or in / factor, or a copy.
//   k_dead_interp      (K8) masked columns interpolated along x between the nearest unmasked ones.
// zinger removal and the 2-D median filter (tomo_prep_outlier):
//   k_outlier          float32.  One work-group per 64 (cols) x 32 (rows) tile of a frame, frames strided over blockIdx.y: the tile and its
//                      reflected halo go to LDS once as orderable keys, rows read coalesced; each lane selects the median of its
//                      size x size window in registers by forgetful selection over min / max exchanges (size a template parameter,
//                      every index static: no scratch), decides the replacement and writes its pixel; the replaced pixels are counted
//                      per wave, then per work-group in LDS, with one integer atomic per work-group and frame.
//   k_outlier_u16x2    uint16.  The same on 128 x 32 tiles with two horizontally adjacent pixels per lane: the tile stays 16 bits wide,
//                      is read as 32-bit words, and the exchanges are the packed unsigned v_pk_min_u16 / v_pk_max_u16, one instruction
//                      for both windows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "../../../include/tomo_prep.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_PREP_ERR_ARG, SIDE_ERR_HIP = TOMO_PREP_ERR_HIP, SIDE_ERR_NODEV = TOMO_PREP_ERR_NODEV;
}
#include "../tomo_side_host.h"

namespace {

constexpr int SORT_KEYS = 8192;        // 64-bit keys per K1 work-group (64 KiB of LDS)
constexpr int SCATTER_VALS = 16384;    // float32 values per K3 work-group (64 KiB of LDS)
constexpr int MAX_ZC = 64;             // z columns per K1 / K3 work-group
constexpr int SORT_T = 512;
constexpr int SCATTER_T = 256;
constexpr int MED_TZ = 64, MED_TX = 64, MED_T = 256;      // K2 tile: 64 z x 64 x, 4 threads along x each doing 16
constexpr int NORM_TILE = 64, NORM_T = 256, NORM_FR = 16;     // k_normalize: 64 x 64 tile, 16 frames per work-group
constexpr int REF_T = 256;
constexpr int DET_T = 256;             // the stripe detector: one work-group per z row, ndx <= SORT_KEYS 32-bit keys in LDS
constexpr int COL_T = 256;             // the per-(x, z) kernels of the large- and dead-stripe passes
constexpr int DEAD_TAPS = 10;          // the angle window of the dead-stripe statistic
constexpr int INTERP_AY = 32;          // angle groups of k_dead_interp
constexpr int OUT_TW = 64, OUT_TH = 32, OUT_T = 256;      // k_outlier tile: 64 cols x 32 rows, a lane per column, 8 rows per lane
constexpr int OUT2_TW = 128;           // k_outlier_u16x2 tile: 128 cols x 32 rows, two columns per lane
constexpr int OUT_MAX_FR = 65535;      // frames k_outlier's grid spans in y; a work-group strides over the rest
constexpr int MAX_LDS = (SORT_KEYS + MAX_ZC) * 8;         // the largest dynamic LDS any kernel here asks for

// orderable bits: unsigned order = float order; -0 is canonicalised to +0 first, every NaN maps to one key above +inf
__device__ __forceinline__ uint32_t ord_bits(float v) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float from_ord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o); }

template <typename T>
__device__ __forceinline__ float to_f(T v) { return (float)v; }

// ---- reference frames
template <typename T>
__global__ __launch_bounds__(REF_T) void k_reference_mean(const T *__restrict__ in, float *__restrict__ out, int n, size_t npix) {
    const size_t p = (size_t)blockIdx.x * REF_T + threadIdx.x;
    if (p >= npix) return;
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += (double)in[(size_t)j * npix + p];
    out[p] = (float)(s / (double)n);
}

template <typename T>
__global__ __launch_bounds__(REF_T) void k_reference_median(const T *__restrict__ in, float *__restrict__ out, int n, size_t npix) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t *keys = reinterpret_cast<uint32_t *>(smem);
    const size_t p = (size_t)blockIdx.x * REF_T + threadIdx.x;
    const bool live = p < npix;
    for (int j = 0; j < n; ++j) keys[j * REF_T + threadIdx.x] = live ? ord_bits(to_f(in[(size_t)j * npix + p])) : 0u;
    if (!live) return;                    // no barrier below: each thread reads only its own column
    const int k1 = (n - 1) / 2, k2 = n / 2;
    uint32_t a = 0, b = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t ki = keys[i * REF_T + threadIdx.x];
        int lt = 0, le = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t kj = keys[j * REF_T + threadIdx.x];
            lt += kj < ki;
            le += kj <= ki;
        }
        if (lt <= k1 && k1 < le) a = ki;
        if (lt <= k2 && k2 < le) b = ki;
    }
    out[p] = (k1 == k2) ? from_ord(a) : (float)(0.5 * ((double)from_ord(a) + (double)from_ord(b)));
}

// ---- normalisation with the transpose; grid: tiles_z * tiles_x * frame groups, tile fastest.  A work-group keeps its tile's flat and
// dark (16 values per thread) in registers across NORM_FR frames, so they are read once per group, not once per frame.
template <typename T>
__global__ __launch_bounds__(NORM_T) void k_normalize(const T *__restrict__ raw, const float *__restrict__ flat, const float *__restrict__ dark,
                                                      float *__restrict__ out, int n, int rows, int cols, int z0, int x0, int nz, int nx,
                                                      int tiles_z, int tiles_x, int use_cutoff, float cutoff, int minus_log, float min_ratio) {
    constexpr int PER = NORM_TILE * NORM_TILE / NORM_T;
    __shared__ float tile[NORM_TILE][NORM_TILE + 1];
    const int tiles = tiles_z * tiles_x;
    const int i0 = (int)(blockIdx.x / (unsigned)tiles) * NORM_FR;
    const int t = (int)(blockIdx.x % (unsigned)tiles);
    const int zt = (t / tiles_x) * NORM_TILE, xt = (t % tiles_x) * NORM_TILE;
    const int tx = threadIdx.x % NORM_TILE, ty = threadIdx.x / NORM_TILE;
    float dk[PER], den[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int z = zt + ty + q * (NORM_T / NORM_TILE), x = xt + tx;
        dk[q] = 0.f;
        den[q] = 1.f;
        if (z < nz && x < nx) {
            const size_t o = (size_t)(z0 + z) * cols + (x0 + x);
            dk[q] = dark[o];
            const float d = flat[o] - dk[q];
            den[q] = d < 1e-6f ? 1e-6f : d;
        }
    }
    const int i1 = min(n, i0 + NORM_FR);
    for (int i = i0; i < i1; ++i) {
        const T *fr = raw + (size_t)i * rows * cols;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int zz = ty + q * (NORM_T / NORM_TILE), z = zt + zz, x = xt + tx;
            float v = 0.f;
            if (z < nz && x < nx) {
                float r = (to_f(fr[(size_t)(z0 + z) * cols + (x0 + x)]) - dk[q]) / den[q];
                if (use_cutoff) r = fminf(r, cutoff);
                v = minus_log ? -logf(fmaxf(r, min_ratio)) : r;
            }
            tile[zz][tx] = v;
        }
        __syncthreads();
        float *po = out + (size_t)i * nx * nz;
        for (int xx = ty; xx < NORM_TILE; xx += NORM_T / NORM_TILE) {
            const int x = xt + xx, z = zt + tx;
            if (x < nx && z < nz) po[(size_t)x * nz + z] = tile[tx][xx];
        }
        __syncthreads();
    }
}

// ---- stripe removal
// K1.  grid: (ndx, groups of ZC z columns of the chunk).  lds index of (segment c, rank r): c (Np + 1) + r.
__global__ __launch_bounds__(SORT_T) void k_stripe_sort(const float *__restrict__ p, float *__restrict__ S, uint16_t *__restrict__ P, int n,
                                                         int ndx, int ndz, int zb, int zw, int logNp, int ZC) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t *keys = reinterpret_cast<uint64_t *>(smem);
    const int Np = 1 << logNp;
    const int x = blockIdx.x, zg = blockIdx.y * ZC;
    const int total = ZC * Np;
    for (int e = threadIdx.x; e < total; e += SORT_T) {
        const int c = e % ZC, a = e / ZC, zl = zg + c;
        uint64_t key = ~0ull;
        if (a < n && zl < zw) key = ((uint64_t)ord_bits(p[((size_t)a * ndx + x) * ndz + zb + zl]) << 32) | (uint32_t)a;
        keys[c * (Np + 1) + a] = key;
    }
    __syncthreads();
    for (int k = 2; k <= Np; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < total / 2; t += SORT_T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));     // i has bit j clear; its partner is i + j, in the same segment
                const int pi = i + (i >> logNp), pl = pi + j;
                const bool asc = (i & k & (Np - 1)) == 0;
                const uint64_t u = keys[pi], v = keys[pl];
                if ((u > v) == asc) {
                    keys[pi] = v;
                    keys[pl] = u;
                }
            }
            __syncthreads();
        }
    }
    for (int e = threadIdx.x; e < ZC * n; e += SORT_T) {
        const int c = e % ZC, r = e / ZC, zl = zg + c;
        if (zl < zw) {
            const uint64_t key = keys[c * (Np + 1) + r];
            const size_t o = ((size_t)r * ndx + x) * zw + zl;
            S[o] = from_ord((uint32_t)(key >> 32));
            P[o] = (uint16_t)(key & 0xffffu);
        }
    }
}

// K2.  grid: (tiles of 64 z of the chunk, tiles of 64 x, n).  W: the compile-time window (>= size); the slots past `size` hold the
// largest key, so they are never counted as smaller than a real value.
__device__ __forceinline__ int reflect(int i, int n) {
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - i - 1;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);      // halo rows of a ragged last tile: any valid row (their outputs are not written)
}

template <int W>
__global__ __launch_bounds__(MED_T) void k_stripe_median(const float *__restrict__ S, float *__restrict__ M, int ndx, int zw, int size) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *tile = reinterpret_cast<float *>(smem);         // [MED_TX + size - 1][MED_TZ]
    const int h = size / 2, k = size / 2;
    const int zt = blockIdx.x * MED_TZ, xt = blockIdx.y * MED_TX;
    const size_t plane = (size_t)blockIdx.z * ndx * zw;
    const int rows = MED_TX + 2 * h;
    const int tz = threadIdx.x % MED_TZ, tx = threadIdx.x / MED_TZ;
    const int z = zt + tz;
    for (int rr = tx; rr < rows; rr += MED_T / MED_TZ) {
        const int x = reflect(xt - h + rr, ndx);
        tile[rr * MED_TZ + tz] = z < zw ? S[plane + (size_t)x * zw + z] : 0.f;
    }
    __syncthreads();
    if (z >= zw) return;
    for (int xx = tx * (MED_TX / 4); xx < (tx + 1) * (MED_TX / 4); ++xx) {
        const int x = xt + xx;
        if (x >= ndx) break;
        float v[W];
        uint32_t o[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            v[j] = j < size ? tile[(xx + j) * MED_TZ + tz] : __uint_as_float(0x7fffffffu);
            o[j] = j < size ? ord_bits(v[j]) : 0xffffffffu;
        }
        float res = 0.f;
#pragma unroll
        for (int i = 0; i < W; ++i) {       // a padding candidate has size smaller keys (> k): never taken, unless NaNs reach rank k
            int lt = 0, le = 0;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                lt += o[j] < o[i];
                le += o[j] <= o[i];
            }
            if (lt <= k && k < le) res = v[i];
        }
        M[plane + (size_t)x * zw + z] = res;
    }
}

// K3.  grid: (ndx, groups of ZC z columns of the chunk).  lds index of (column c, angle a): c (n + 1) + a.
__global__ __launch_bounds__(SCATTER_T) void k_stripe_scatter(const float *__restrict__ M, const uint16_t *__restrict__ P, float *out, int n,
                                                               int ndx, int ndz, int zb, int zw, int ZC) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *vals = reinterpret_cast<float *>(smem);
    const int x = blockIdx.x, zg = blockIdx.y * ZC;
    for (int e = threadIdx.x; e < ZC * n; e += SCATTER_T) {
        const int c = e % ZC, r = e / ZC, zl = zg + c;
        if (zl < zw) {
            const size_t o = ((size_t)r * ndx + x) * zw + zl;
            vals[c * (n + 1) + P[o]] = M[o];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < ZC * n; e += SCATTER_T) {
        const int c = e % ZC, a = e / ZC, zl = zg + c;
        if (zl < zw) out[((size_t)a * ndx + x) * ndz + zb + zl] = vals[c * (n + 1) + a];
    }
}

// ---- large and dead stripes (Vo algorithms 5 and 6).  Per chunk the factor lists and the mask are [x][zl] (zl fastest, cols = ndx zw
// values).  Every kernel below fixes the order of its float64 sums, so a numpy model repeats it.  The library is built with
// -ffp-contract=fast, under which the backend fuses a multiply with a following add whatever a pragma says: a product that must be
// rounded on its own goes through f_mul / d_mul, whose empty asm hides it from that fusion.
__device__ __forceinline__ float f_mul(float a, float b) { float p = a * b; asm volatile("" : "+v"(p)); return p; }
__device__ __forceinline__ double d_mul(double a, double b) { double p = a * b; asm volatile("" : "+v"(p)); return p; }

// K4.  One thread per (x, zl): the float64 means over the ranks r0 <= r < r1 of the sorted and of the smoothed values, and their ratio.
__global__ __launch_bounds__(COL_T) void k_large_factor(const float *__restrict__ S, const float *__restrict__ M, float *__restrict__ f,
                                                         int r0, int r1, size_t cols) {
    const size_t t = (size_t)blockIdx.x * COL_T + threadIdx.x;
    if (t >= cols) return;
    double s1 = 0.0, s2 = 0.0;
    for (int r = r0; r < r1; ++r) {
        s1 += (double)S[(size_t)r * cols + t];
        s2 += (double)M[(size_t)r * cols + t];
    }
    const double cnt = (double)(r1 - r0), l1 = s1 / cnt, l2 = s2 / cnt;
    f[t] = l2 != 0.0 ? (float)(l1 / l2) : 1.f;
}

// K5.  One thread per (x, zl) walks the angles with the 10 values of the window a - 5 ... a + 4 (reflected) in registers:
// u = float32(sum of the window in float64, in angle order, / 10), diff = float32(sum_a double(|s - u|)).
__global__ __launch_bounds__(COL_T) void k_dead_diff(const float *__restrict__ p, float *__restrict__ diff, int n, int ndx, int ndz, int zb,
                                                      int zw) {
    const size_t t = (size_t)blockIdx.x * COL_T + threadIdx.x;
    if (t >= (size_t)ndx * zw) return;
    const int x = (int)(t / zw), zl = (int)(t % zw);
    const float *col = p + (size_t)x * ndz + zb + zl;
    const size_t stride = (size_t)ndx * ndz;
    float w[DEAD_TAPS];
#pragma unroll
    for (int j = 0; j < DEAD_TAPS; ++j) w[j] = col[(size_t)reflect(j - DEAD_TAPS / 2, n) * stride];
    double acc = 0.0;
    for (int a = 0; a < n; ++a) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < DEAD_TAPS; ++j) s += (double)w[j];
        const float u = (float)(s / (double)DEAD_TAPS);
        acc += (double)fabsf(w[DEAD_TAPS / 2] - u);
#pragma unroll
        for (int j = 0; j + 1 < DEAD_TAPS; ++j) w[j] = w[j + 1];
        w[DEAD_TAPS - 1] = col[(size_t)reflect(a + DEAD_TAPS / 2, n) * stride];
    }
    diff[t] = (float)acc;
}

__global__ __launch_bounds__(COL_T) void k_dead_factor(const float *__restrict__ diff, const float *__restrict__ bck, float *__restrict__ f,
                                                        size_t cols) {
    const size_t t = (size_t)blockIdx.x * COL_T + threadIdx.x;
    if (t < cols) f[t] = bck[t] != 0.f ? diff[t] / bck[t] : 1.f;
}

// the detector reads a factor as a finite float32: NaN and +inf count as the largest value, -inf as the smallest
__device__ __forceinline__ float finite_factor(float v) {
    if (v != v) return 3.402823466e+38f;
    return fminf(fmaxf(v, -3.402823466e+38f), 3.402823466e+38f);
}

// K6, the stripe detector.  One work-group per zl: the ndx factors as orderable keys in LDS (padded with 0, below every finite key, to
// a power of two Np), sorted ascending by a bitonic network and read from the top; thread 0 fits the line through the middle half
// in float64 in one fixed order; every thread thresholds its columns, the mask is dilated by one column in LDS.
__global__ __launch_bounds__(DET_T) void k_stripe_detect(const float *__restrict__ f, uint8_t *__restrict__ mk, uint8_t *__restrict__ d_mask,
                                                          int ndx, int ndz, int zb, int zw, int logNp, float snr_f, int clear_edges) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t *keys = reinterpret_cast<uint32_t *>(smem);
    __shared__ double thr[2];
    __shared__ int fire[2];
    const int Np = 1 << logNp, zl = blockIdx.x;
    for (int x = threadIdx.x; x < Np; x += DET_T) keys[x] = x < ndx ? ord_bits(finite_factor(f[(size_t)x * zw + zl])) : 0u;
    __syncthreads();
    for (int k = 2; k <= Np; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < Np / 2; t += DET_T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                const bool asc = (i & k) == 0;
                const uint32_t u = keys[i], v = keys[l];
                if ((u > v) == asc) {
                    keys[i] = v;
                    keys[l] = u;
                }
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {              // d[i], descending, is keys[Np - 1 - i]
        const double snr = (double)snr_f;
        const int nd = ndx / 4, i0 = nd, i1 = ndx - nd - 1, cnt = i1 - i0;
        const double xm = 0.5 * (double)(i0 + i1 - 1);
        double sy = 0.0;
        for (int i = i0; i < i1; ++i) sy += (double)from_ord(keys[Np - 1 - i]);
        const double ym = sy / (double)cnt;
        double sxy = 0.0, sxx = 0.0;
        for (int i = i0; i < i1; ++i) {
            const double dx = (double)i - xm;
            sxy += d_mul(dx, (double)from_ord(keys[Np - 1 - i]) - ym);
            sxx += d_mul(dx, dx);
        }
        const double m = sxy / sxx, c = ym - d_mul(m, xm), t1 = c + d_mul(m, (double)(ndx - 1));
        const double noise = fmax(fabs(t1 - c), 1e-6);
        const double v1 = fabs((double)from_ord(keys[Np - 1]) - c) / noise, v2 = fabs((double)from_ord(keys[Np - ndx]) - t1) / noise;
        fire[0] = v1 >= snr;
        fire[1] = v2 >= snr;
        thr[0] = c + d_mul(0.5 * snr, noise);
        thr[1] = t1 - d_mul(0.5 * snr, noise);
    }
    __syncthreads();
    for (int x = threadIdx.x; x < ndx; x += DET_T) {
        const double g = (double)finite_factor(f[(size_t)x * zw + zl]);
        keys[x] = ((fire[0] && g > thr[0]) || (fire[1] && g <= thr[1])) ? 1u : 0u;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < ndx; x += DET_T) {
        uint32_t r = keys[x] | (x > 0 ? keys[x - 1] : 0u) | (x + 1 < ndx ? keys[x + 1] : 0u);
        if (clear_edges && (x < 2 || x >= ndx - 2)) r = 0u;
        mk[(size_t)x * zw + zl] = (uint8_t)r;
        if (d_mask) d_mask[(size_t)x * ndz + zb + zl] = (uint8_t)r;
    }
}

// K7, K3 with a choice per column.  A masked column takes the smoothed value at the rank its angle had in K1's sort (scattered through
// LDS as in K3); every other column is divided by its factor (norm) or copied.  `in` may be `out`: a thread reads what it writes.
__global__ __launch_bounds__(SCATTER_T) void k_large_correct(const float *in, const float *__restrict__ M, const uint16_t *__restrict__ P,
                                                              const float *__restrict__ f, const uint8_t *__restrict__ mk, float *out, int n,
                                                              int ndx, int ndz, int zb, int zw, int ZC, int norm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *vals = reinterpret_cast<float *>(smem);
    const int x = blockIdx.x, zg = blockIdx.y * ZC;
    for (int e = threadIdx.x; e < ZC * n; e += SCATTER_T) {
        const int c = e % ZC, r = e / ZC, zl = zg + c;
        if (zl < zw && mk[(size_t)x * zw + zl]) {
            const size_t o = ((size_t)r * ndx + x) * zw + zl;
            vals[c * (n + 1) + P[o]] = M[o];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < ZC * n; e += SCATTER_T) {
        const int c = e % ZC, a = e / ZC, zl = zg + c;
        if (zl >= zw) continue;
        const size_t i = ((size_t)a * ndx + x) * ndz + zb + zl, q = (size_t)x * zw + zl;
        float v;
        if (mk[q]) v = vals[c * (n + 1) + a];
        else v = norm ? in[i] / f[q] : in[i];
        out[i] = v;
    }
}

// K8.  One thread per (x, zl), angles strided over blockIdx.y.  A masked column is interpolated in float32, the product rounded on its own, between
// the nearest unmasked columns xl < x < xr of the same angle (they exist: the mask's first and last two columns are clear); an
// unmasked column is copied, or left alone when `in` is `out` -- so the columns read here are never written.
__global__ __launch_bounds__(COL_T) void k_dead_interp(const float *in, const uint8_t *__restrict__ mk, float *out, int n, int ndx, int ndz,
                                                        int zb, int zw) {
    const size_t t = (size_t)blockIdx.x * COL_T + threadIdx.x;
    if (t >= (size_t)ndx * zw) return;
    const int x = (int)(t / zw), zl = (int)(t % zw);
    const bool m = mk[t] != 0;
    if (!m && in == out) return;
    int xl = x, xr = x;
    if (m) {
        while (xl > 0 && mk[(size_t)xl * zw + zl]) --xl;
        while (xr < ndx - 1 && mk[(size_t)xr * zw + zl]) ++xr;
    }
    const float w = m ? (float)(x - xl) / (float)(xr - xl) : 0.f;
    for (int a = blockIdx.y; a < n; a += gridDim.y) {
        const size_t base = (size_t)a * ndx * ndz + zb + zl;
        float v;
        if (m) {
            const float l = in[base + (size_t)xl * ndz], r = in[base + (size_t)xr * ndz];
            v = l + f_mul(r - l, w);
        } else {
            v = in[base + (size_t)x * ndz];
        }
        out[base + (size_t)x * ndz] = v;
    }
}

// ---- zinger removal and the 2-D median filter
// The LDS key of a pixel: uint16 by value, float32 by its orderable bits; both compared as unsigned integers.
template <typename T> struct OutKey;
template <> struct OutKey<uint16_t> {
    static __device__ __forceinline__ uint16_t enc(uint16_t v) { return v; }
    static __device__ __forceinline__ uint32_t bits(uint16_t v) { return v; }
    static __device__ __forceinline__ bool finite(uint16_t) { return true; }
};
template <> struct OutKey<float> {
    typedef uint32_t lds_t;
    static __device__ __forceinline__ uint32_t enc(float v) { return ord_bits(v); }
    static __device__ __forceinline__ float dec(uint32_t k) { return k == 0xffffffffu ? __uint_as_float(0x7fc00000u) : from_ord(k); }
    static __device__ __forceinline__ uint32_t bits(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ bool finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
};

// Two horizontally adjacent uint16 keys in one register: min / max are the packed unsigned v_pk_min_u16 / v_pk_max_u16.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t vmin(uint32_t a, uint32_t b) { return min(a, b); }
__device__ __forceinline__ uint32_t vmax(uint32_t a, uint32_t b) { return max(a, b); }
__device__ __forceinline__ u16x2 vmin(u16x2 a, u16x2 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ u16x2 vmax(u16x2 a, u16x2 b) { return __builtin_elementwise_max(a, b); }

template <typename V>
__device__ __forceinline__ void cx(V &a, V &b) {
    const V lo = vmin(a, b);
    b = vmax(a, b);
    a = lo;
}

// The minimum of v[0 .. K) to v[0] and the maximum to v[K - 1]; the values in between stay a permutation of the rest.
template <int K, int M, typename V>
__device__ __forceinline__ void min_max(V (&v)[M]) {
    constexpr int L = (K + 1) / 2;       // after the first pass v[0 .. L) holds the minimum and v[K - L .. K) the maximum
#pragma unroll
    for (int i = 0; i < K / 2; ++i) cx(v[i], v[K - 1 - i]);
#pragma unroll
    for (int s = 1; s < L; s <<= 1) {
#pragma unroll
        for (int i = 0; i + s < L; i += 2 * s) cx(v[i], v[i + s]);
    }
#pragma unroll
    for (int s = 1; s < L; s <<= 1) {
#pragma unroll
        for (int i = 0; i + s < L; i += 2 * s) cx(v[K - 1 - i - s], v[K - 1 - i]);
    }
}

// The S x S window of a lane, read a row of S keys at a time.  One pixel per lane: the keys as they lie in the tile (row stride LW).
template <int S, int LW, typename L>
struct RowsOfOne {
    typedef uint32_t V;
    const L *win;                         // the window's top left key
    __device__ __forceinline__ void row(int r, V (&b)[S]) const {
#pragma unroll
        for (int c = 0; c < S; ++c) b[c] = win[r * LW + c];
    }
};

// Two pixels per lane (uint16): the tile is read as aligned 32-bit words of two keys; the lane's pair lies HP = 2 or 4 (even, >= S / 2)
// keys into its words, and a pair that starts at an odd key is cut out of two neighbouring words.
template <int S, int LW32>
struct RowsOfTwo {
    typedef u16x2 V;
    static constexpr int H = S / 2, HP = (H + 1) & ~1, C0 = HP - H, NW = (HP + H + 1) / 2 + 1;
    const uint32_t *win;                  // the word of the window's top row that holds the lane's pair, less HP / 2 words
    __device__ __forceinline__ void row(int r, V (&b)[S]) const {
        uint32_t w[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) w[j] = win[r * LW32 + j];
#pragma unroll
        for (int c = 0; c < S; ++c) {
            const int k = C0 + c;
            b[c] = __builtin_bit_cast(u16x2, (k & 1) ? (w[k / 2] >> 16) | (w[k / 2 + 1] << 16) : w[k / 2]);
        }
    }
};

// Forgetful selection: of K candidates the smallest and the largest cannot be the median of all S * S values while K > S * S / 2 + 1, so
// both are dropped and the next value of the window is admitted, until three are left.
template <int K, int S, int M, typename Src>
__device__ __forceinline__ void forget(typename Src::V (&v)[M], typename Src::V (&b)[S], const Src &src) {
    if constexpr (K > 3) {
        min_max<K>(v);
        constexpr int e = 2 * M - K;
        if constexpr (e % S == 0) src.row(e / S, b);
        v[0] = b[e % S];
        forget<K - 1, S, M>(v, b, src);
    }
}

// The key of rank (S * S - 1) / 2 of the S x S window (of each of the lane's windows, for a packed V).
template <int S, typename Src>
__device__ __forceinline__ typename Src::V window_median(const Src &src) {
    typedef typename Src::V V;
    constexpr int M = S * S / 2 + 2;
    V v[M], b[S];
#pragma unroll
    for (int e = 0; e < M; ++e) {
        if (e % S == 0) src.row(e / S, b);
        v[e] = b[e % S];
    }
    forget<M, S, M>(v, b, src);
    return vmax(vmin(v[0], v[1]), vmin(vmax(v[0], v[1]), v[2]));
}

// Whether the pixel v is replaced by the median med, and with what.
template <typename T>
__device__ __forceinline__ bool outlier_hit(T v, T med, int mode, float dif, int two_sided) {
    typedef OutKey<T> KT;
    if (mode == TOMO_PREP_MEDIAN2D) return KT::bits(v) != KT::bits(med);
    float d = to_f(v) - to_f(med);
    if (two_sided) d = fabsf(d);
    return d >= dif || !KT::finite(v);
}

// The rows y0 - H ... of the frame and the columns x0 - HP ... go to tile[LH][LW] as keys, reflected at the frame's edges: a wave per row.
template <typename T, typename L, int LH, int LW>
__device__ __forceinline__ void stage_tile(const T *__restrict__ fin, L *tile, int rows, int cols, int ytop, int xleft) {
    for (int r = threadIdx.x / 64; r < LH; r += OUT_T / 64) {
        const T *row = fin + (size_t)reflect(ytop + r, rows) * cols;
        for (int c = threadIdx.x % 64; c < LW; c += 64) tile[r * LW + c] = OutKey<T>::enc(row[reflect(xleft + c, cols)]);
    }
}

// The work-group's count of replaced pixels goes to count[f] with one atomic; `hits` was cleared before the barrier that preceded the
// waves' work.  Ends with a barrier: the tile and the counter are then free for the next frame.
__device__ __forceinline__ void count_hits(uint32_t mine, uint32_t *hits, uint32_t *__restrict__ count, int f) {
    if (count) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(hits, mine);
    }
    __syncthreads();
    if (count && threadIdx.x == 0 && *hits) atomicAdd(count + f, *hits);
    __syncthreads();
}

// grid: (tiles of a frame, x fastest; min(n, OUT_MAX_FR)).  `in` and `out` never overlap: the in-place call goes through the scratch.
template <typename T, int S>
__global__ __launch_bounds__(OUT_T) void k_outlier(const T *__restrict__ in, T *__restrict__ out, uint32_t *__restrict__ count, int n, int rows,
                                                   int cols, int tiles_x, int mode, float dif, int two_sided) {
    typedef OutKey<T> KT;
    typedef typename KT::lds_t L;
    constexpr int H = S / 2, LW = OUT_TW + S - 1, LH = OUT_TH + S - 1;
    __shared__ L tile[LH * LW];
    __shared__ uint32_t hits;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * OUT_TW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * OUT_TH;
    const int tx = threadIdx.x % OUT_TW, ty = threadIdx.x / OUT_TW;
    const int x = x0 + tx;
    const size_t npix = (size_t)rows * cols;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const T *fin = in + (size_t)f * npix;
        T *fout = out + (size_t)f * npix;
        if (threadIdx.x == 0) hits = 0u;
        stage_tile<T, L, LH, LW>(fin, tile, rows, cols, y0 - H, x0 - H);
        __syncthreads();
        uint32_t mine = 0u;
#pragma unroll 1
        for (int yy = ty; yy < OUT_TH; yy += OUT_T / OUT_TW) {       // a wave shares yy
            const int y = y0 + yy;
            if (y >= rows) break;
            const RowsOfOne<S, LW, L> src = {tile + yy * LW + tx};
            const T med = KT::dec(window_median<S>(src));
            if (x < cols) {
                const size_t o = (size_t)y * cols + x;
                const T v = fin[o];            // the pixel's own bits: the keys fold -0 and the NaN payloads
                const bool hit = outlier_hit(v, med, mode, dif, two_sided);
                fout[o] = hit ? med : v;
                mine += hit ? 1u : 0u;
            }
        }
        count_hits(mine, &hits, count, f);
    }
}

// The same for uint16 with two adjacent pixels per lane: tiles of 128 columns, the selection on packed pairs.  grid as k_outlier.
template <int S>
__global__ __launch_bounds__(OUT_T) void k_outlier_u16x2(const uint16_t *__restrict__ in, uint16_t *__restrict__ out, uint32_t *__restrict__ count,
                                                         int n, int rows, int cols, int tiles_x, int mode, float dif, int two_sided) {
    constexpr int H = S / 2, HP = (H + 1) & ~1, LW = OUT2_TW + 2 * HP, LH = OUT_TH + S - 1;
    __shared__ uint32_t tile32[LH * LW / 2];
    __shared__ uint32_t hits;
    uint16_t *tile = reinterpret_cast<uint16_t *>(tile32);
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * OUT2_TW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * OUT_TH;
    const int tx = threadIdx.x % 64, ty = threadIdx.x / 64;
    const int x = x0 + 2 * tx;
    const size_t npix = (size_t)rows * cols;
    const bool words = (cols & 1) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;       // every pair of the output is an aligned word
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint16_t *fin = in + (size_t)f * npix;
        uint16_t *fout = out + (size_t)f * npix;
        if (threadIdx.x == 0) hits = 0u;
        stage_tile<uint16_t, uint16_t, LH, LW>(fin, tile, rows, cols, y0 - H, x0 - HP);
        __syncthreads();
        uint32_t mine = 0u;
#pragma unroll 1
        for (int yy = ty; yy < OUT_TH; yy += OUT_T / 64) {
            const int y = y0 + yy;
            if (y >= rows) break;
            const RowsOfTwo<S, LW / 2> src = {tile32 + yy * (LW / 2) + tx};
            const u16x2 med = window_median<S>(src);
            const u16x2 v = __builtin_bit_cast(u16x2, tile32[(yy + H) * (LW / 2) + HP / 2 + tx]);
            const bool hit0 = outlier_hit<uint16_t>(v.x, med.x, mode, dif, two_sided);
            const bool hit1 = outlier_hit<uint16_t>(v.y, med.y, mode, dif, two_sided);
            u16x2 res;
            res.x = hit0 ? med.x : v.x;
            res.y = hit1 ? med.y : v.y;
            const size_t o = (size_t)y * cols + x;
            if (x + 1 < cols) {
                if (words) {
                    *reinterpret_cast<uint32_t *>(fout + o) = __builtin_bit_cast(uint32_t, res);
                } else {
                    fout[o] = res.x;
                    fout[o + 1] = res.y;
                }
                mine += (hit0 ? 1u : 0u) + (hit1 ? 1u : 0u);
            } else if (x < cols) {             // the last column of an odd width
                fout[o] = res.x;
                mine += hit0 ? 1u : 0u;
            }
        }
        count_hits(mine, &hits, count, f);
    }
}

}  // namespace

struct tomo_prep {
    int device = 0;
    std::string err;
    Buf scratch;                               // stripe scratch (S, M and P of one chunk), or one batch of frames of the in-place outlier call
    hipStream_t last_stream = nullptr;         // the stream the scratch was last used on
    hipEvent_t ev_done = nullptr;              // after the last use of the scratch
    hipEvent_t ev_pass[4] = {nullptr, nullptr, nullptr, nullptr};
    bool pending = false;
};

namespace {

template <typename K>
int allow_lds(tomo_prep *h, K kernel) {
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS));
    return TOMO_PREP_OK;
}

int drain(tomo_prep *h) {
    if (h->pending) {
        HIPCHK(h, hipEventSynchronize(h->ev_done));
        h->pending = false;
    }
    return TOMO_PREP_OK;
}

int ilog2_ceil(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

int chunk_for(int n_proj, int ndx, int ndz, size_t budget) {
    if (budget == 0) return ndz;
    const size_t per_z = (size_t)10 * (size_t)n_proj * (size_t)ndx;
    size_t zc = budget / per_z;
    if (zc >= (size_t)ndz) return ndz;
    if (zc >= 64) zc -= zc % 64;               // whole 64-wide tiles for the median pass
    return zc < 1 ? 1 : (int)zc;
}

template <int W>
int launch_median(tomo_prep *h, hipStream_t st, const float *S, float *M, int n, int ndx, int zw, int size) {
    static bool attr = false;
    if (!attr) {
        int rc = allow_lds(h, k_stripe_median<W>);
        if (rc) return rc;
        attr = true;
    }
    const size_t lds = (size_t)(MED_TX + size - 1) * MED_TZ * sizeof(float);
    dim3 grid((unsigned)((zw + MED_TZ - 1) / MED_TZ), (unsigned)((ndx + MED_TX - 1) / MED_TX), (unsigned)n);
    hipLaunchKernelGGL(k_stripe_median<W>, grid, dim3(MED_T), lds, st, S, M, ndx, zw, size);
    HIPCHK(h, hipGetLastError());
    return TOMO_PREP_OK;
}

int median(tomo_prep *h, hipStream_t st, const float *S, float *M, int n, int ndx, int zw, int size) {
    if (size <= 3) return launch_median<3>(h, st, S, M, n, ndx, zw, size);
    if (size <= 7) return launch_median<7>(h, st, S, M, n, ndx, zw, size);
    if (size <= 11) return launch_median<11>(h, st, S, M, n, ndx, zw, size);
    if (size <= 15) return launch_median<15>(h, st, S, M, n, ndx, zw, size);
    if (size <= 21) return launch_median<21>(h, st, S, M, n, ndx, zw, size);
    if (size <= 31) return launch_median<31>(h, st, S, M, n, ndx, zw, size);
    if (size <= 41) return launch_median<41>(h, st, S, M, n, ndx, zw, size);
    return launch_median<63>(h, st, S, M, n, ndx, zw, size);
}

template <typename T>
int reference_t(tomo_prep *h, hipStream_t st, const T *in, int n, size_t npix, int method, float *out) {
    const unsigned blocks = (unsigned)((npix + REF_T - 1) / REF_T);
    if (method == TOMO_PREP_MEAN) {
        hipLaunchKernelGGL(k_reference_mean<T>, dim3(blocks), dim3(REF_T), 0, st, in, out, n, npix);
    } else {
        static bool attr = false;
        if (!attr) {
            int rc = allow_lds(h, k_reference_median<T>);
            if (rc) return rc;
            attr = true;
        }
        hipLaunchKernelGGL(k_reference_median<T>, dim3(blocks), dim3(REF_T), (size_t)n * REF_T * sizeof(uint32_t), st, in, out, n, npix);
    }
    HIPCHK(h, hipGetLastError());
    return TOMO_PREP_OK;
}

// ---- large and dead stripes: the scratch of one chunk and the passes over it (all enqueued, no host round trip)
struct Chunk {
    float *S, *M, *f, *diff, *bck;     // S, M: [rank][x][zl]; f, diff, bck: [x][zl]
    uint16_t *P;
    uint8_t *mk;
};

constexpr size_t VAL_BYTES = 10, COL_BYTES = 13;      // scratch per sinogram value, and per (x, z) on top of it

int chunk_for_all(int n_proj, int ndx, int ndz, size_t budget) {
    if (budget == 0) return ndz;
    const size_t per_z = (VAL_BYTES * (size_t)n_proj + COL_BYTES) * (size_t)ndx;
    size_t zc = budget / per_z;
    if (zc >= (size_t)ndz) return ndz;
    if (zc >= 64) zc -= zc % 64;
    return zc < 1 ? 1 : (int)zc;
}

// what every pass of the large / dead / all family checks before anything is launched
int check_stripe(tomo_prep *h, const char *who, const void *d_in, const void *d_out, int n_proj, int ndx, int ndz, float snr, int size,
                 int min_nproj) {
    const std::string w(who);
    if (!h) return fail(h, TOMO_PREP_ERR_ARG, w + ": NULL handle");
    if (n_proj > TOMO_PREP_MAX_NPROJ)
        return fail(h, TOMO_PREP_ERR_UNSUPPORTED, w + ": n_proj " + std::to_string(n_proj) + " > " + std::to_string(TOMO_PREP_MAX_NPROJ) +
                                                      " (one 64-bit key per angle in LDS); nothing was written");
    if (ndx > SORT_KEYS)
        return fail(h, TOMO_PREP_ERR_UNSUPPORTED, w + ": ndx " + std::to_string(ndx) + " > " + std::to_string(SORT_KEYS) +
                                                      " (the detector sorts one row of factors in LDS); nothing was written");
    if (n_proj < min_nproj || ndx < TOMO_PREP_MIN_STRIPE_NDX || ndz < 1)
        return fail(h, TOMO_PREP_ERR_ARG, w + ": bad shape (n_proj >= " + std::to_string(min_nproj) + ", ndx >= 8, ndz >= 1)");
    if (size < 3 || size % 2 == 0 || size > TOMO_PREP_MAX_STRIPE_SIZE || size > ndx)
        return fail(h, TOMO_PREP_ERR_ARG, w + ": size must be odd with 3 <= size <= min(ndx, 63)");
    if (!(snr > 0.f) || !(snr <= 3.402823466e+38f)) return fail(h, TOMO_PREP_ERR_ARG, w + ": snr must be finite and > 0");
    if (!d_in || !d_out) return fail(h, TOMO_PREP_ERR_ARG, w + ": NULL pointer");
    if ((long long)n_proj * ndx >= (1LL << 31) / 10 || ndz > 65535)
        return fail(h, TOMO_PREP_ERR_ARG, w + ": shape too large (n_proj * ndx < 2^31 / 10, ndz <= 65535)");
    return TOMO_PREP_OK;
}

// the handle's scratch for chunks of zc rows, safe to write on stream st
int chunk_scratch(tomo_prep *h, hipStream_t st, int n_proj, int ndx, int zc, Chunk &c) {
    const size_t nchunk = (size_t)n_proj * ndx * zc, cols = (size_t)ndx * zc;
    const size_t need = nchunk * VAL_BYTES + cols * COL_BYTES;
    if (h->pending && (need > h->scratch.n || st != h->last_stream)) CHK(drain(h));
    CHK(grow(h, h->scratch, need));
    static bool attr = false;
    if (!attr) {
        CHK(allow_lds(h, k_stripe_sort));
        CHK(allow_lds(h, k_stripe_scatter));
        CHK(allow_lds(h, k_large_correct));
        attr = true;
    }
    c.S = static_cast<float *>(h->scratch.p);
    c.M = c.S + nchunk;
    c.f = c.M + nchunk;
    c.diff = c.f + cols;
    c.bck = c.diff + cols;
    c.P = reinterpret_cast<uint16_t *>(c.bck + cols);
    c.mk = reinterpret_cast<uint8_t *>(c.P + nchunk);
    return TOMO_PREP_OK;
}

int scratch_used(tomo_prep *h, hipStream_t st) {
    HIPCHK(h, hipEventRecord(h->ev_done, st));
    h->pending = true;
    h->last_stream = st;
    return TOMO_PREP_OK;
}

int sort_pass(tomo_prep *h, hipStream_t st, const float *in, const Chunk &c, int n, int ndx, int ndz, int zb, int zw) {
    const int logNp = ilog2_ceil(n), Np = 1 << logNp;
    const int zc1 = std::min(MAX_ZC, std::max(1, SORT_KEYS / Np));
    hipLaunchKernelGGL(k_stripe_sort, dim3((unsigned)ndx, (unsigned)((zw + zc1 - 1) / zc1)), dim3(SORT_T),
                       (size_t)zc1 * (Np + 1) * sizeof(uint64_t), st, in, c.S, c.P, n, ndx, ndz, zb, zw, logNp, zc1);
    HIPCHK(h, hipGetLastError());
    return TOMO_PREP_OK;
}

int detect_pass(tomo_prep *h, hipStream_t st, const Chunk &c, int ndx, int ndz, int zb, int zw, float snr, int clear_edges, uint8_t *d_mask) {
    const int logNp = ilog2_ceil(ndx);
    hipLaunchKernelGGL(k_stripe_detect, dim3((unsigned)zw), dim3(DET_T), (size_t)(1 << logNp) * sizeof(uint32_t), st, c.f, c.mk, d_mask, ndx,
                       ndz, zb, zw, logNp, snr, clear_edges);
    HIPCHK(h, hipGetLastError());
    return TOMO_PREP_OK;
}

unsigned col_blocks(int ndx, int zw) { return (unsigned)(((size_t)ndx * zw + COL_T - 1) / COL_T); }

// algorithm 5 on the rows zb ... zb + zw of `in` into `out` (which may be `in`)
int large_chunk(tomo_prep *h, hipStream_t st, const float *in, float *out, int n, int ndx, int ndz, int zb, int zw, float snr, int size,
                int nd, int norm, uint8_t *d_mask, const Chunk &c) {
    CHK(sort_pass(h, st, in, c, n, ndx, ndz, zb, zw));
    CHK(median(h, st, c.S, c.M, n, ndx, zw, size));
    hipLaunchKernelGGL(k_large_factor, dim3(col_blocks(ndx, zw)), dim3(COL_T), 0, st, c.S, c.M, c.f, nd, n - nd, (size_t)ndx * zw);
    HIPCHK(h, hipGetLastError());
    CHK(detect_pass(h, st, c, ndx, ndz, zb, zw, snr, 0, d_mask));
    const int zc3 = std::min(MAX_ZC, std::max(1, SCATTER_VALS / n));
    hipLaunchKernelGGL(k_large_correct, dim3((unsigned)ndx, (unsigned)((zw + zc3 - 1) / zc3)), dim3(SCATTER_T),
                       (size_t)zc3 * (n + 1) * sizeof(float), st, in, c.M, c.P, c.f, c.mk, out, n, ndx, ndz, zb, zw, zc3, norm);
    HIPCHK(h, hipGetLastError());
    return TOMO_PREP_OK;
}

// algorithm 6 (without its closing large-stripe pass) on the rows zb ... zb + zw
int dead_chunk(tomo_prep *h, hipStream_t st, const float *in, float *out, int n, int ndx, int ndz, int zb, int zw, float snr, int size,
               uint8_t *d_mask, const Chunk &c) {
    const unsigned blocks = col_blocks(ndx, zw);
    hipLaunchKernelGGL(k_dead_diff, dim3(blocks), dim3(COL_T), 0, st, in, c.diff, n, ndx, ndz, zb, zw);
    HIPCHK(h, hipGetLastError());
    CHK(median(h, st, c.diff, c.bck, 1, ndx, zw, size));
    hipLaunchKernelGGL(k_dead_factor, dim3(blocks), dim3(COL_T), 0, st, c.diff, c.bck, c.f, (size_t)ndx * zw);
    HIPCHK(h, hipGetLastError());
    CHK(detect_pass(h, st, c, ndx, ndz, zb, zw, snr, 1, d_mask));
    hipLaunchKernelGGL(k_dead_interp, dim3(blocks, (unsigned)std::min(n, INTERP_AY)), dim3(COL_T), 0, st, in, c.mk, out, n, ndx, ndz, zb, zw);
    HIPCHK(h, hipGetLastError());
    return TOMO_PREP_OK;
}

// algorithm 3 in place on the rows zb ... zb + zw of `out`
int sorting_chunk(tomo_prep *h, hipStream_t st, float *out, int n, int ndx, int ndz, int zb, int zw, int size, const Chunk &c) {
    CHK(sort_pass(h, st, out, c, n, ndx, ndz, zb, zw));
    CHK(median(h, st, c.S, c.M, n, ndx, zw, size));
    const int zc3 = std::min(MAX_ZC, std::max(1, SCATTER_VALS / n));
    hipLaunchKernelGGL(k_stripe_scatter, dim3((unsigned)ndx, (unsigned)((zw + zc3 - 1) / zc3)), dim3(SCATTER_T),
                       (size_t)zc3 * (n + 1) * sizeof(float), st, c.M, c.P, out, n, ndx, ndz, zb, zw, zc3);
    HIPCHK(h, hipGetLastError());
    return TOMO_PREP_OK;
}

int drop_ranks(float drop_ratio, int n_proj) {
    const double dr = std::min(std::max((double)drop_ratio, 0.0), 0.8);
    return (int)(0.5 * dr * (double)n_proj);
}

constexpr float DEAD_DROP_RATIO = 0.1f;      // the large-stripe pass that closes the dead-stripe pass keeps Vo's default

// ---- zinger removal and the 2-D median filter
size_t dtype_bytes(int dtype) { return dtype == TOMO_PREP_U16 ? sizeof(uint16_t) : sizeof(float); }

// frames per batch of the in-place call: what fits the budget, at least one
int outlier_batch_for(int rows, int cols, int dtype, int n, size_t budget) {
    if (budget == 0) return n;
    const size_t b = budget / ((size_t)rows * (size_t)cols * dtype_bytes(dtype));
    return b >= (size_t)n ? n : (b < 1 ? 1 : (int)b);
}

template <typename T, int S>
int launch_outlier_s(tomo_prep *h, hipStream_t st, const T *in, T *out, uint32_t *count, int n, int rows, int cols, int mode, float dif,
                     int two_sided) {
    constexpr bool packed = std::is_same<T, uint16_t>::value;      // uint16: two pixels per lane (1.4 - 2.1 x the rate of one, measured)
    constexpr int tw = packed ? OUT2_TW : OUT_TW;
    const int tiles_x = (cols + tw - 1) / tw, tiles_y = (rows + OUT_TH - 1) / OUT_TH;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)std::min(n, OUT_MAX_FR));
    if constexpr (packed)
        hipLaunchKernelGGL((k_outlier_u16x2<S>), grid, dim3(OUT_T), 0, st, in, out, count, n, rows, cols, tiles_x, mode, dif, two_sided);
    else
        hipLaunchKernelGGL((k_outlier<T, S>), grid, dim3(OUT_T), 0, st, in, out, count, n, rows, cols, tiles_x, mode, dif, two_sided);
    HIPCHK(h, hipGetLastError());
    return TOMO_PREP_OK;
}

template <typename T>
int launch_outlier(tomo_prep *h, hipStream_t st, const void *in, void *out, uint32_t *count, int n, int rows, int cols, int size, int mode,
                   float dif, int two_sided) {
    const T *i = static_cast<const T *>(in);
    T *o = static_cast<T *>(out);
    if (size == 3) return launch_outlier_s<T, 3>(h, st, i, o, count, n, rows, cols, mode, dif, two_sided);
    if (size == 5) return launch_outlier_s<T, 5>(h, st, i, o, count, n, rows, cols, mode, dif, two_sided);
    return launch_outlier_s<T, 7>(h, st, i, o, count, n, rows, cols, mode, dif, two_sided);
}

// what tomo_prep_outlier and tomo_prep_outlier_batch both check
int check_outlier_shape(tomo_prep *h, const char *who, int dtype, int n, int rows, int cols, int size) {
    const std::string w(who);
    if (dtype != TOMO_PREP_U16 && dtype != TOMO_PREP_F32) return fail(h, TOMO_PREP_ERR_ARG, w + ": dtype must be uint16 or float32");
    if (size != 3 && size != 5 && size != 7) return fail(h, TOMO_PREP_ERR_ARG, w + ": size must be 3, 5 or 7");
    if (n < 1 || rows < size || cols < size)
        return fail(h, TOMO_PREP_ERR_ARG, w + ": bad shape (n >= 1, rows >= size, cols >= size)");
    if ((long long)rows * cols >= (1LL << 31)) return fail(h, TOMO_PREP_ERR_ARG, w + ": frame too large (rows * cols < 2^31)");
    return TOMO_PREP_OK;
}

}  // namespace

extern "C" {

TOMO_API int tomo_prep_abi_version(void) { return 1; }

TOMO_API int tomo_prep_create(int device, tomo_prep **out) {
    CHK(check_create(device, out));
    tomo_prep *h = new tomo_prep();
    h->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&h->ev_pass[i]);
    if (e != hipSuccess) {
        tomo_prep_destroy(h);
        return fail(nullptr, TOMO_PREP_ERR_HIP, std::string("event creation: ") + hipGetErrorString(e));
    }
    *out = h;
    return TOMO_PREP_OK;
}

TOMO_API int tomo_prep_destroy(tomo_prep *h) {
    if (!h) return TOMO_PREP_OK;
    (void)hipSetDevice(h->device);
    if (h->pending) (void)hipEventSynchronize(h->ev_done);
    if (h->scratch.p) (void)hipFree(h->scratch.p);
    if (h->ev_done) (void)hipEventDestroy(h->ev_done);
    for (hipEvent_t ev : h->ev_pass)
        if (ev) (void)hipEventDestroy(ev);
    delete h;
    return TOMO_PREP_OK;
}

TOMO_API const char *tomo_prep_last_error(tomo_prep *h) { return last_error(h); }

TOMO_API int tomo_prep_reference(tomo_prep *h, void *stream, const void *d_frames, int dtype, int n, int rows, int cols, int method,
                                 float *d_out) {
    if (!h) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_reference: NULL handle");
    if (n < 1 || rows < 1 || cols < 1) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_reference: bad shape");
    if (dtype != TOMO_PREP_U16 && dtype != TOMO_PREP_F32) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_reference: dtype must be uint16 or float32");
    if (method != TOMO_PREP_MEAN && method != TOMO_PREP_MEDIAN) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_reference: unknown method");
    if (method == TOMO_PREP_MEDIAN && n > TOMO_PREP_MAX_MEDIAN_FRAMES)
        return fail(h, TOMO_PREP_ERR_UNSUPPORTED, "tomo_prep_reference: median over " + std::to_string(n) + " > 64 frames");
    if (!d_frames || !d_out) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_reference: NULL pointer");
    const size_t npix = (size_t)rows * (size_t)cols;
    if ((npix + REF_T - 1) / REF_T >= (1ull << 31)) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_reference: frame too large");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == TOMO_PREP_U16) return reference_t(h, st, static_cast<const uint16_t *>(d_frames), n, npix, method, d_out);
    return reference_t(h, st, static_cast<const float *>(d_frames), n, npix, method, d_out);
}

TOMO_API int tomo_prep_normalize(tomo_prep *h, void *stream, const void *d_raw, int dtype, int n, int rows, int cols, const float *d_flat,
                                 const float *d_dark, int z0, int z1, int x0, int x1, int use_cutoff, float cutoff, int minus_log,
                                 float min_ratio, float *d_out) {
    if (!h) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_normalize: NULL handle");
    if (n < 0 || rows < 1 || cols < 1) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_normalize: bad shape");
    if (dtype != TOMO_PREP_U16 && dtype != TOMO_PREP_F32) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_normalize: dtype must be uint16 or float32");
    if (z0 < 0 || z1 > rows || z0 >= z1 || x0 < 0 || x1 > cols || x0 >= x1)
        return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_normalize: crop window outside the frame or empty");
    if (n == 0) return TOMO_PREP_OK;
    if (!d_raw || !d_flat || !d_dark || !d_out) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_normalize: NULL pointer");
    const int nz = z1 - z0, nx = x1 - x0;
    const int tiles_z = (nz + NORM_TILE - 1) / NORM_TILE, tiles_x = (nx + NORM_TILE - 1) / NORM_TILE;
    const int groups = (n + NORM_FR - 1) / NORM_FR;
    if ((long long)tiles_z * tiles_x * groups >= (1LL << 31)) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_normalize: too many work-groups");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(tiles_z * tiles_x * groups));
    if (dtype == TOMO_PREP_U16)
        hipLaunchKernelGGL(k_normalize<uint16_t>, grid, dim3(NORM_T), 0, st, static_cast<const uint16_t *>(d_raw), d_flat, d_dark, d_out, n,
                           rows, cols, z0, x0, nz, nx, tiles_z, tiles_x, use_cutoff, cutoff, minus_log, min_ratio);
    else
        hipLaunchKernelGGL(k_normalize<float>, grid, dim3(NORM_T), 0, st, static_cast<const float *>(d_raw), d_flat, d_dark, d_out, n,
                           rows, cols, z0, x0, nz, nx, tiles_z, tiles_x, use_cutoff, cutoff, minus_log, min_ratio);
    HIPCHK(h, hipGetLastError());
    return TOMO_PREP_OK;
}

TOMO_API int tomo_prep_stripe_chunk(int n_proj, int ndx, int ndz, size_t max_scratch_bytes, int *chunk_z) {
    if (!chunk_z || n_proj < 1 || ndx < 1 || ndz < 1) return fail(nullptr, TOMO_PREP_ERR_ARG, "tomo_prep_stripe_chunk: bad args");
    *chunk_z = chunk_for(n_proj, ndx, ndz, max_scratch_bytes);
    return TOMO_PREP_OK;
}

TOMO_API int tomo_prep_stripe_sorting(tomo_prep *h, void *stream, const float *d_in, float *d_out, int n_proj, int ndx, int ndz, int size,
                                      size_t max_scratch_bytes, float *pass_ms) {
    if (!h) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_stripe_sorting: NULL handle");
    if (n_proj > TOMO_PREP_MAX_NPROJ)
        return fail(h, TOMO_PREP_ERR_UNSUPPORTED, "tomo_prep_stripe_sorting: n_proj " + std::to_string(n_proj) + " > " +
                                                      std::to_string(TOMO_PREP_MAX_NPROJ) + " (one 64-bit key per angle in LDS); nothing was written");
    if (n_proj < 1 || ndx < 1 || ndz < 1) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_stripe_sorting: bad shape");
    if (size < 3 || size % 2 == 0 || size > TOMO_PREP_MAX_STRIPE_SIZE || size > ndx)
        return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_stripe_sorting: size must be odd with 3 <= size <= min(ndx, 63)");
    if (!d_in || !d_out) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_stripe_sorting: NULL pointer");
    if ((long long)n_proj * ndx >= (1LL << 31) / 10 || ndz > 65535)
        return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_stripe_sorting: shape too large (n_proj * ndx < 2^31 / 10, ndz <= 65535)");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int zc = chunk_for(n_proj, ndx, ndz, max_scratch_bytes);
    const size_t nchunk = (size_t)n_proj * ndx * zc;
    const size_t need = nchunk * 10;
    if (h->pending && (need > h->scratch.n || st != h->last_stream)) {     // the scratch is replaced or used on another stream
        int rc = drain(h);
        if (rc) return rc;
    }
    CHK(grow(h, h->scratch, need));
    static bool attr = false;
    if (!attr) {
        int rc = allow_lds(h, k_stripe_sort);
        if (!rc) rc = allow_lds(h, k_stripe_scatter);
        if (rc) return rc;
        attr = true;
    }
    float *S = static_cast<float *>(h->scratch.p);
    float *M = S + nchunk;
    uint16_t *P = reinterpret_cast<uint16_t *>(M + nchunk);
    const int logNp = ilog2_ceil(n_proj), Np = 1 << logNp;
    const int zc1 = std::min(MAX_ZC, std::max(1, SORT_KEYS / Np));
    const int zc3 = std::min(MAX_ZC, std::max(1, SCATTER_VALS / n_proj));
    const size_t lds1 = (size_t)zc1 * (Np + 1) * sizeof(uint64_t), lds3 = (size_t)zc3 * (n_proj + 1) * sizeof(float);
    if (pass_ms) pass_ms[0] = pass_ms[1] = pass_ms[2] = 0.f;
    for (int zb = 0; zb < ndz; zb += zc) {
        const int zw = std::min(zc, ndz - zb);
        if (pass_ms) HIPCHK(h, hipEventRecord(h->ev_pass[0], st));
        hipLaunchKernelGGL(k_stripe_sort, dim3((unsigned)ndx, (unsigned)((zw + zc1 - 1) / zc1)), dim3(SORT_T), lds1, st, d_in, S, P, n_proj,
                           ndx, ndz, zb, zw, logNp, zc1);
        HIPCHK(h, hipGetLastError());
        if (pass_ms) HIPCHK(h, hipEventRecord(h->ev_pass[1], st));
        int rc = median(h, st, S, M, n_proj, ndx, zw, size);
        if (rc) return rc;
        if (pass_ms) HIPCHK(h, hipEventRecord(h->ev_pass[2], st));
        hipLaunchKernelGGL(k_stripe_scatter, dim3((unsigned)ndx, (unsigned)((zw + zc3 - 1) / zc3)), dim3(SCATTER_T), lds3, st, M, P, d_out,
                           n_proj, ndx, ndz, zb, zw, zc3);
        HIPCHK(h, hipGetLastError());
        if (pass_ms) {
            HIPCHK(h, hipEventRecord(h->ev_pass[3], st));
            HIPCHK(h, hipEventSynchronize(h->ev_pass[3]));
            for (int p = 0; p < 3; ++p) {
                float ms = 0.f;
                HIPCHK(h, hipEventElapsedTime(&ms, h->ev_pass[p], h->ev_pass[p + 1]));
                pass_ms[p] += ms;
            }
        }
    }
    HIPCHK(h, hipEventRecord(h->ev_done, st));
    h->pending = true;
    h->last_stream = st;
    return TOMO_PREP_OK;
}

TOMO_API int tomo_prep_stripe_all_chunk(int n_proj, int ndx, int ndz, size_t max_scratch_bytes, int *chunk_z) {
    if (!chunk_z || n_proj < 1 || ndx < 1 || ndz < 1) return fail(nullptr, TOMO_PREP_ERR_ARG, "tomo_prep_stripe_all_chunk: bad args");
    *chunk_z = chunk_for_all(n_proj, ndx, ndz, max_scratch_bytes);
    return TOMO_PREP_OK;
}

TOMO_API int tomo_prep_stripe_large(tomo_prep *h, void *stream, const float *d_in, float *d_out, int n_proj, int ndx, int ndz, float snr,
                                    int size, float drop_ratio, int norm, size_t max_scratch_bytes, uint8_t *d_mask) {
    CHK(check_stripe(h, "tomo_prep_stripe_large", d_in, d_out, n_proj, ndx, ndz, snr, size, 1));
    if (!(drop_ratio == drop_ratio)) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_stripe_large: drop_ratio is NaN");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int zc = chunk_for_all(n_proj, ndx, ndz, max_scratch_bytes), nd = drop_ranks(drop_ratio, n_proj);
    Chunk c;
    CHK(chunk_scratch(h, st, n_proj, ndx, zc, c));
    for (int zb = 0; zb < ndz; zb += zc)
        CHK(large_chunk(h, st, d_in, d_out, n_proj, ndx, ndz, zb, std::min(zc, ndz - zb), snr, size, nd, norm, d_mask, c));
    return scratch_used(h, st);
}

TOMO_API int tomo_prep_stripe_dead(tomo_prep *h, void *stream, const float *d_in, float *d_out, int n_proj, int ndx, int ndz, float snr,
                                   int size, int norm, size_t max_scratch_bytes, uint8_t *d_mask, uint8_t *d_mask_large) {
    CHK(check_stripe(h, "tomo_prep_stripe_dead", d_in, d_out, n_proj, ndx, ndz, snr, size, TOMO_PREP_MIN_DEAD_NPROJ));
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int zc = chunk_for_all(n_proj, ndx, ndz, max_scratch_bytes), nd = drop_ranks(DEAD_DROP_RATIO, n_proj);
    Chunk c;
    CHK(chunk_scratch(h, st, n_proj, ndx, zc, c));
    for (int zb = 0; zb < ndz; zb += zc) {
        const int zw = std::min(zc, ndz - zb);
        CHK(dead_chunk(h, st, d_in, d_out, n_proj, ndx, ndz, zb, zw, snr, size, d_mask, c));
        if (norm) CHK(large_chunk(h, st, d_out, d_out, n_proj, ndx, ndz, zb, zw, snr, size, nd, 1, d_mask_large, c));
    }
    return scratch_used(h, st);
}

TOMO_API int tomo_prep_stripe_all(tomo_prep *h, void *stream, const float *d_in, float *d_out, int n_proj, int ndx, int ndz, float snr,
                                  int la_size, int sm_size, size_t max_scratch_bytes, uint8_t *d_mask_dead, uint8_t *d_mask_large) {
    CHK(check_stripe(h, "tomo_prep_stripe_all", d_in, d_out, n_proj, ndx, ndz, snr, la_size, TOMO_PREP_MIN_DEAD_NPROJ));
    CHK(check_stripe(h, "tomo_prep_stripe_all", d_in, d_out, n_proj, ndx, ndz, snr, sm_size, TOMO_PREP_MIN_DEAD_NPROJ));
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int zc = chunk_for_all(n_proj, ndx, ndz, max_scratch_bytes), nd = drop_ranks(DEAD_DROP_RATIO, n_proj);
    Chunk c;
    CHK(chunk_scratch(h, st, n_proj, ndx, zc, c));
    for (int zb = 0; zb < ndz; zb += zc) {
        const int zw = std::min(zc, ndz - zb);
        CHK(dead_chunk(h, st, d_in, d_out, n_proj, ndx, ndz, zb, zw, snr, la_size, d_mask_dead, c));
        CHK(large_chunk(h, st, d_out, d_out, n_proj, ndx, ndz, zb, zw, snr, la_size, nd, 1, d_mask_large, c));
        CHK(sorting_chunk(h, st, d_out, n_proj, ndx, ndz, zb, zw, sm_size, c));
    }
    return scratch_used(h, st);
}

TOMO_API int tomo_prep_outlier_batch(int rows, int cols, int dtype, int n, size_t max_scratch_bytes, int *frames) {
    if (!frames) return fail(nullptr, TOMO_PREP_ERR_ARG, "tomo_prep_outlier_batch: NULL pointer");
    CHK(check_outlier_shape(nullptr, "tomo_prep_outlier_batch", dtype, n, rows, cols, 3));
    *frames = outlier_batch_for(rows, cols, dtype, n, max_scratch_bytes);
    return TOMO_PREP_OK;
}

TOMO_API int tomo_prep_outlier(tomo_prep *h, void *stream, const void *d_in, void *d_out, int dtype, int n, int rows, int cols, int size,
                               int mode, float dif, int two_sided, size_t max_scratch_bytes, uint32_t *d_count) {
    if (!h) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_outlier: NULL handle");
    CHK(check_outlier_shape(h, "tomo_prep_outlier", dtype, n, rows, cols, size));
    if (mode != TOMO_PREP_OUTLIER && mode != TOMO_PREP_MEDIAN2D) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_outlier: unknown mode");
    if (mode == TOMO_PREP_OUTLIER && !(dif >= 0.f)) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_outlier: dif must be >= 0 and not NaN");
    if (!d_in || !d_out) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_outlier: NULL pointer");
    const size_t frame_bytes = (size_t)rows * (size_t)cols * dtype_bytes(dtype), total = frame_bytes * (size_t)n;
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_in), b = reinterpret_cast<uintptr_t>(d_out);
    if (a != b && a < b + total && b < a + total) return fail(h, TOMO_PREP_ERR_ARG, "tomo_prep_outlier: d_out must be d_in itself or not overlap it");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool u16 = dtype == TOMO_PREP_U16;
    if (a != b) {
        if (d_count) HIPCHK(h, hipMemsetAsync(d_count, 0, (size_t)n * sizeof(uint32_t), st));
        return u16 ? launch_outlier<uint16_t>(h, st, d_in, d_out, d_count, n, rows, cols, size, mode, dif, two_sided)
                   : launch_outlier<float>(h, st, d_in, d_out, d_count, n, rows, cols, size, mode, dif, two_sided);
    }
    // in place: batches of frames are filtered into the handle's scratch and copied back, all on the stream
    const int nb = outlier_batch_for(rows, cols, dtype, n, max_scratch_bytes);
    const size_t need = frame_bytes * (size_t)nb;
    if (h->pending && (need > h->scratch.n || st != h->last_stream)) CHK(drain(h));
    CHK(grow(h, h->scratch, need));
    if (d_count) HIPCHK(h, hipMemsetAsync(d_count, 0, (size_t)n * sizeof(uint32_t), st));
    for (int f0 = 0; f0 < n; f0 += nb) {
        const int nf = std::min(nb, n - f0);
        char *frames = static_cast<char *>(d_out) + frame_bytes * (size_t)f0;
        uint32_t *cnt = d_count ? d_count + f0 : nullptr;
        CHK(u16 ? launch_outlier<uint16_t>(h, st, frames, h->scratch.p, cnt, nf, rows, cols, size, mode, dif, two_sided)
                : launch_outlier<float>(h, st, frames, h->scratch.p, cnt, nf, rows, cols, size, mode, dif, two_sided));
        HIPCHK(h, hipMemcpyAsync(frames, h->scratch.p, frame_bytes * (size_t)nf, hipMemcpyDeviceToDevice, st));
    }
    return scratch_used(h, st);
}

}  // extern "C"
