// libtomo_dff.so: dynamic flat-field correction (include/tomo_dff.h, tomography_alignment_amd/preprocess.py) on gfx950.
//
// k_gram       a work-group owns a group of consecutive chunks of C pixels.  Per chunk it stages the K flats' values as float32 (exact for
//              both dtypes) in LDS rows of C + 1 floats (the odd stride puts the rows of different flats on different banks) and fbar
//              beside them; thread t owns the pairs t, t + 256, ... of the K (K + 1) / 2 with l <= k, at most GRAM_R of them, and adds
//              c_k[p] c_l[p] over the chunk's pixels in order into a register per pair.  One partial per (group, pair).
// k_gram_fold  one thread per pair: the groups' partials in index order into G[k][l] and G[l][k].
// k_eff        one thread per pixel: the K values of its pixel once, m float64 sums with V from LDS.
// k_bin        one thread per binned pixel.
// k_cost       a work-group owns (tile of TZ x TX pixels with a right and a lower neighbour, listed projection): v and u_j of the tile
//              and its one-pixel halo go to LDS, a lane adds its four pixels in float64, the wave by a fixed shuffle tree, the waves in
//              order.  One partial of f and of every g_j per (listed projection, tile).
// k_cost_fold  one thread per (listed projection, f or g_j): the tiles in index order.
// k_apply      tomo_prep's k_normalize with the flat rebuilt per projection: a 64 x 64 (z, x) tile per work-group, read coalesced along
//              x, normalised on the way into LDS, written coalesced along z.
// No atomics anywhere: every sum has one owner and a fixed order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/tomo_dff.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_DFF_ERR_ARG, SIDE_ERR_HIP = TOMO_DFF_ERR_HIP, SIDE_ERR_NODEV = TOMO_DFF_ERR_NODEV;
}
#include "../tomo_side_host.h"

namespace {

constexpr int TPB = 256;
constexpr int MAXM = TOMO_DFF_MAX_EFF, MAXK = TOMO_DFF_MAX_FLATS;
constexpr int GRAM_LDS_FLOATS = 8192;                                  // 32 KiB (33.5 KiB where the chunk is floored at 64, K >= 120); 157 VGPRs, not LDS, bound k_gram to three work-groups a CU
constexpr int GRAM_MAX_CHUNK = 512, GRAM_GROUP_PIXELS = 4096;
constexpr int GRAM_R = (MAXK * (MAXK + 1) / 2 + TPB - 1) / TPB;        // pairs a thread owns at most: 33
constexpr int TZ = TOMO_DFF_TILE_Z, TX = TOMO_DFF_TILE_X, HZ = TZ + 1, HX = TX + 1, PLANE = HZ * HX;
constexpr int NORM_TILE = 64, NORM_FR = 16;                            // k_apply: 64 x 64 tile, 16 frames per work-group
static_assert(TX == 64 && TZ * TX == 4 * TPB, "a lane of k_cost owns four rows of one column of the tile");

template <typename T>
__device__ __forceinline__ float to_f(T v) { return (float)v; }

// the pair idx of the lower triangle, rows in order: (k, l) with l <= k and idx = k (k + 1) / 2 + l
__device__ __forceinline__ void pair_of(int idx, int &k, int &l) {
    k = (int)((sqrtf(8.f * (float)idx + 1.f) - 1.f) * 0.5f);
    while (k * (k + 1) / 2 > idx) --k;
    while ((k + 1) * (k + 2) / 2 <= idx) ++k;
    l = idx - k * (k + 1) / 2;
}

// ---------------------------------------------------------------------------------------------------------------------- kernels

template <typename T>
__global__ __launch_bounds__(TPB) void k_gram(const T *__restrict__ flats, const float *__restrict__ fbar, int K, long long npix, int C, int cpg,
                                              double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int S = C + 1;
    float *fb = sm + K * S;
    const int t = threadIdx.x, npairs = K * (K + 1) / 2;
    double acc[GRAM_R];
#pragma unroll
    for (int r = 0; r < GRAM_R; ++r) acc[r] = 0.0;
    const long long g0 = (long long)blockIdx.x * cpg * C;
    for (int c = 0; c < cpg; ++c) {
        const long long p0 = g0 + (long long)c * C;
        if (p0 >= npix) break;                                           // uniform over the work-group
        const int np = (int)min((long long)C, npix - p0);
        __syncthreads();                                                 // the chunk before has been read
        for (int e = t; e < K * C; e += TPB) {
            const int k = e / C, p = e - k * C;
            sm[k * S + p] = p < np ? to_f(flats[(long long)k * npix + p0 + p]) : 0.f;
        }
        for (int p = t; p < C; p += TPB) fb[p] = p < np ? fbar[p0 + p] : 0.f;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < GRAM_R; ++r) {
            const int idx = r * TPB + t;
            if (idx < npairs) {
                int k, l;
                pair_of(idx, k, l);
                const float *sk = sm + k * S, *sl = sm + l * S;
                double a = acc[r];
                for (int p = 0; p < np; ++p) {
                    const double m = (double)fb[p];
                    a += ((double)sk[p] - m) * ((double)sl[p] - m);
                }
                acc[r] = a;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < GRAM_R; ++r) {
        const int idx = r * TPB + t;
        if (idx < npairs) part[(long long)blockIdx.x * npairs + idx] = acc[r];
    }
}

__global__ __launch_bounds__(TPB) void k_gram_fold(const double *__restrict__ part, int K, int ngroups, double *__restrict__ G) {
    const int idx = blockIdx.x * TPB + threadIdx.x, npairs = K * (K + 1) / 2;
    if (idx >= npairs) return;
    double s = 0.0;
    for (int g = 0; g < ngroups; ++g) s += part[(long long)g * npairs + idx];
    int k, l;
    pair_of(idx, k, l);
    G[k * K + l] = s;
    G[l * K + k] = s;
}

template <typename T>
__global__ __launch_bounds__(TPB) void k_eff(const T *__restrict__ flats, const float *__restrict__ fbar, const double *__restrict__ V, int K, int m,
                                             long long npix, double scale, float *__restrict__ eff) {
    __shared__ double sv[MAXK * MAXM];
    for (int e = threadIdx.x; e < K * m; e += TPB) sv[e] = V[e];
    __syncthreads();
    const long long p = (long long)blockIdx.x * TPB + threadIdx.x;
    if (p >= npix) return;
    const double mean = (double)fbar[p];
    double acc[MAXM];
#pragma unroll
    for (int j = 0; j < MAXM; ++j) acc[j] = 0.0;
    for (int k = 0; k < K; ++k) {
        const double c = (double)to_f(flats[(long long)k * npix + p]) - mean;
#pragma unroll
        for (int j = 0; j < MAXM; ++j)
            if (j < m) acc[j] += sv[k * m + j] * c;
    }
#pragma unroll
    for (int j = 0; j < MAXM; ++j)
        if (j < m) eff[(long long)j * npix + p] = (float)(scale * acc[j]);
}

template <typename T>
__global__ __launch_bounds__(TPB) void k_bin(const T *__restrict__ src, const float *__restrict__ dark, long long total, int rows, int cols, int b,
                                             int zb, int xb, float *__restrict__ out) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= total) return;
    const int x = (int)(idx % xb);
    const long long iz = idx / xb;
    const int z = (int)(iz % zb);
    const long long i = iz / zb;
    const T *fr = src + i * (long long)rows * cols;
    float s = 0.f;
    for (int dz = 0; dz < b; ++dz)
        for (int dx = 0; dx < b; ++dx) {
            const long long o = (long long)(z * b + dz) * cols + (x * b + dx);
            s += to_f(fr[o]) - (dark ? dark[o] : 0.f);
        }
    out[idx] = s;
}

// f + w e with the product and the sum each rounded on its own.  The library is built with -ffp-contract=fast, under which the back
// end fuses any product with the sum that uses it -- those of __fmul_rn and __fadd_rn, which this compiler defines as the plain
// operators, and those under a contract(off) pragma included.  The empty asm makes the rounded product a value the compiler cannot look
// through; it emits no instruction.
__device__ __forceinline__ float add_product_unfused(float f, float w, float e) {
    float p = __fmul_rn(w, e);
    asm volatile("" : "+v"(p));
    return __fadd_rn(f, p);
}

struct CostTable {
    float a[MAXM];      // a_1 ... a_m
};

// par: per listed projection 2 + m words: its index in the scratch, s, w_0 ... w_(m-1)
__global__ __launch_bounds__(TPB) void k_cost(const float *__restrict__ Rb, const float *__restrict__ Fb, const float *__restrict__ Eb,
                                              const uint32_t *__restrict__ par, int m, int zb, int xb, int tiles_x, CostTable A, float eps2,
                                              double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float sm[];         // v, u_0, ..., u_(m-1): 1 + m planes of HZ x HX
    __shared__ double sred[TPB / 64][1 + MAXM];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tile = blockIdx.x, li = blockIdx.y, ntiles = gridDim.x;
    const uint32_t *rec = par + (size_t)li * (2 + m);
    const size_t nb = (size_t)zb * xb;
    const float *R = Rb + (size_t)rec[0] * nb;
    const float s = __uint_as_float(rec[1]);
    float w[MAXM];
#pragma unroll
    for (int j = 0; j < MAXM; ++j) w[j] = j < m ? __uint_as_float(rec[2 + j]) : 0.f;
    const int zt = (tile / tiles_x) * TZ, xt = (tile % tiles_x) * TX;
    for (int e = t; e < PLANE; e += TPB) {
        const int hz = e / HX, hx = e - hz * HX;
        const int z = zt + hz, x = xt + hx;
        float v = 0.f, u[MAXM];
#pragma unroll
        for (int j = 0; j < MAXM; ++j) u[j] = 0.f;
        if (z < zb && x < xb) {
            const size_t o = (size_t)z * xb + x;
            float eb[MAXM];
            float D = Fb[o];
#pragma unroll
            for (int j = 0; j < MAXM; ++j) {
                eb[j] = 0.f;
                if (j < m) {
                    eb[j] = Eb[j * nb + o];
                    D += w[j] * eb[j];
                }
            }
            const bool clamped = D < 1e-6f;
            if (clamped) D = 1e-6f;
            const float rD = 1.f / D;                                    // one division per pixel: q and v Eb_j / D as products with it
            const float q = R[o] * rD;
            v = s * q;
            const float vd = clamped ? 0.f : v * rD;
#pragma unroll
            for (int j = 0; j < MAXM; ++j)
                if (j < m) u[j] = A.a[j] * q - vd * eb[j];
        }
        sm[e] = v;
#pragma unroll
        for (int j = 0; j < MAXM; ++j)
            if (j < m) sm[(1 + j) * PLANE + e] = u[j];
    }
    __syncthreads();
    double acc[1 + MAXM];
#pragma unroll
    for (int j = 0; j <= MAXM; ++j) acc[j] = 0.0;
#pragma unroll
    for (int r = 0; r < TZ / (TPB / 64); ++r) {
        const int zz = wave + (TPB / 64) * r, z = zt + zz, x = xt + lane;
        if (z < zb - 1 && x < xb - 1) {
            const int c = zz * HX + lane;
            const float v0 = sm[c];
            const float gx = sm[c + 1] - v0, gz = sm[c + HX] - v0;
            const float tt = sqrtf(gx * gx + gz * gz + eps2);
            const float rt = 1.f / tt;
            acc[0] += (double)tt;
#pragma unroll
            for (int j = 0; j < MAXM; ++j)
                if (j < m) {
                    const float *u = sm + (1 + j) * PLANE;
                    acc[1 + j] += (double)((gx * (u[c + 1] - u[c]) + gz * (u[c + HX] - u[c])) * rt);
                }
        }
    }
#pragma unroll
    for (int j = 0; j <= MAXM; ++j) {
        if (j <= m) {                                                    // uniform
            double val = acc[j];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) val += __shfl_down(val, d, 64);
            if (lane == 0) sred[wave][j] = val;
        }
    }
    __syncthreads();
    if (t <= m) part[((size_t)li * ntiles + tile) * (1 + m) + t] = ((sred[0][t] + sred[1][t]) + sred[2][t]) + sred[3][t];
}

__global__ __launch_bounds__(TPB) void k_cost_fold(const double *__restrict__ part, int nids, int ntiles, int m, double *__restrict__ res) {
    const int idx = blockIdx.x * TPB + threadIdx.x;
    if (idx >= nids * (1 + m)) return;
    const int li = idx / (1 + m), c = idx - li * (1 + m);
    double s = 0.0;
    for (int tile = 0; tile < ntiles; ++tile) s += part[((size_t)li * ntiles + tile) * (1 + m) + c];
    res[idx] = s;
}

// grid: tiles_z * tiles_x * frame groups, tile fastest.  A work-group keeps its tile's fbar and dark (16 values per thread) in registers
// across NORM_FR frames; the EFFs are read per frame and stay in L2.
template <typename T>
__global__ __launch_bounds__(TPB) void k_apply(const T *__restrict__ raw, const float *__restrict__ fbar, const float *__restrict__ dark,
                                               const float *__restrict__ eff, const float *__restrict__ w, int m, float *__restrict__ out, int n,
                                               int rows, int cols, int z0, int x0, int nz, int nx, int tiles_z, int tiles_x, int use_cutoff,
                                               float cutoff, int minus_log, float min_ratio) {
    constexpr int PER = NORM_TILE * NORM_TILE / TPB;
    __shared__ float tile[NORM_TILE][NORM_TILE + 1];
    const int tiles = tiles_z * tiles_x;
    const int i0 = (int)(blockIdx.x / (unsigned)tiles) * NORM_FR;
    const int t = (int)(blockIdx.x % (unsigned)tiles);
    const int zt = (t / tiles_x) * NORM_TILE, xt = (t % tiles_x) * NORM_TILE;
    const int tx = threadIdx.x % NORM_TILE, ty = threadIdx.x / NORM_TILE;
    const size_t npix = (size_t)rows * cols;
    float dk[PER], fb[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int z = zt + ty + q * (TPB / NORM_TILE), x = xt + tx;
        dk[q] = 0.f;
        fb[q] = 1.f;
        if (z < nz && x < nx) {
            const size_t o = (size_t)(z0 + z) * cols + (x0 + x);
            dk[q] = dark[o];
            fb[q] = fbar[o];
        }
    }
    const int i1 = min(n, i0 + NORM_FR);
    for (int i = i0; i < i1; ++i) {
        const T *fr = raw + (size_t)i * npix;
        float fl[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) fl[q] = fb[q];
        for (int j = 0; j < m; ++j) {                                    // one EFF at a time: PER loads in flight, not PER m
            const float wj = w[(size_t)i * m + j];
            const float *e = eff + (size_t)j * npix;
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int z = zt + ty + q * (TPB / NORM_TILE), x = xt + tx;
                if (z < nz && x < nx) fl[q] = add_product_unfused(fl[q], wj, e[(size_t)(z0 + z) * cols + (x0 + x)]);
            }
        }
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int zz = ty + q * (TPB / NORM_TILE), z = zt + zz, x = xt + tx;
            float v = 0.f;
            if (z < nz && x < nx) {
                const float d = fl[q] - dk[q];
                const float den = d < 1e-6f ? 1e-6f : d;
                float r = (to_f(fr[(size_t)(z0 + z) * cols + (x0 + x)]) - dk[q]) / den;
                if (use_cutoff) r = fminf(r, cutoff);
                v = minus_log ? -logf(fmaxf(r, min_ratio)) : r;
            }
            tile[zz][tx] = v;
        }
        __syncthreads();
        float *po = out + (size_t)i * nx * nz;
        for (int xx = ty; xx < NORM_TILE; xx += TPB / NORM_TILE) {
            const int x = xt + xx, z = zt + tx;
            if (x < nx && z < nz) po[(size_t)x * nz + z] = tile[tx][xx];
        }
        __syncthreads();
    }
}

}  // namespace

struct tomo_dff {
    int device = 0;
    std::string err;
    size_t max_scratch = 0;          // 0: no limit
    int i0 = 0, nb = 0, zb = 0, xb = 0;   // what tomo_dff_load left in rb; nb = 0 before it
    Buf rb;                          // float [nb][zb][xb]
    Buf gpart, G, V;                 // double [groups][pairs], double [K][K], double [K][m]
    Buf par, cpart, cres;            // uint32 [nids][2 + m], double [nids][tiles][1 + m], double [nids][1 + m]
    Buf wts;                         // float [n][m] of tomo_dff_apply
    auto bufs() { return std::array{&rb, &gpart, &G, &V, &par, &cpart, &cres, &wts}; }
    std::vector<uint32_t> hpar;      // what par is uploaded from: alive until the copy has been made
    std::vector<double> hV;
    std::vector<float> hw;
};

namespace {

std::string str(long long v) { return std::to_string(v); }

int check_frame(tomo_dff *h, int rows, int cols) {
    if (rows < 1 || cols < 1 || (long long)rows * cols >= (1LL << 31))
        return fail(h, TOMO_DFF_ERR_UNSUPPORTED, "tomo_dff: frames of " + str(rows) + " x " + str(cols) + " are outside 1 <= rows, 1 <= cols, rows cols < 2^31; nothing was launched");
    return TOMO_DFF_OK;
}

int check_flats(tomo_dff *h, int K) {
    if (K < 2 || K > MAXK)
        return fail(h, TOMO_DFF_ERR_UNSUPPORTED, "tomo_dff: " + str(K) + " flats are outside 2 <= K <= " + str(MAXK) + "; nothing was launched");
    return TOMO_DFF_OK;
}

// K < 0: the flats are not this call's business
int check_eff(tomo_dff *h, int m, int K) {
    if (m < 0 || m > MAXM)
        return fail(h, TOMO_DFF_ERR_UNSUPPORTED, "tomo_dff: " + str(m) + " eigen flat fields are outside 0 <= m <= " + str(MAXM) + "; nothing was launched");
    if (K >= 0 && m > K - 1)
        return fail(h, TOMO_DFF_ERR_UNSUPPORTED, "tomo_dff: " + str(m) + " eigen flat fields need m <= K - 1 = " + str(K - 1) + " (the flats' deviations from their mean span no more); nothing was launched");
    return TOMO_DFF_OK;
}

int check_bin(tomo_dff *h, int rows, int cols, int bin) {
    if (bin < 1 || bin > TOMO_DFF_MAX_BIN)
        return fail(h, TOMO_DFF_ERR_UNSUPPORTED, "tomo_dff: bin " + str(bin) + " is outside 1 <= bin <= " + str(TOMO_DFF_MAX_BIN) + "; nothing was launched");
    if (rows / bin < 2 || cols / bin < 2)
        return fail(h, TOMO_DFF_ERR_UNSUPPORTED, "tomo_dff: frames of " + str(rows) + " x " + str(cols) + " binned by " + str(bin) + " leave " + str(rows / bin) + " x " + str(cols / bin) +
                                                     ", fewer than 2 x 2 (the total variation needs a neighbour); nothing was launched");
    return TOMO_DFF_OK;
}

int check_dtype(tomo_dff *h, int dtype, const char *who) {
    if (dtype != TOMO_DFF_U16 && dtype != TOMO_DFF_F32) return fail(h, TOMO_DFF_ERR_ARG, std::string(who) + ": dtype must be uint16 or float32");
    return TOMO_DFF_OK;
}

inline int gram_chunk(int K) { return std::max(64, std::min(GRAM_MAX_CHUNK, ((GRAM_LDS_FLOATS - K) / (K + 1)) / 64 * 64)); }
inline int gram_cpg(int C) { return std::max(1, GRAM_GROUP_PIXELS / C); }

inline size_t scratch_bytes(int rows, int cols, int bin) { return sizeof(float) * (size_t)(rows / bin) * (size_t)(cols / bin); }

int batch_for(int n, int rows, int cols, int bin, size_t budget) {
    long long b = n;
    if (budget) b = std::min<long long>(b, (long long)(budget / scratch_bytes(rows, cols, bin)));
    return (int)std::max<long long>(b, 1);
}

template <typename T>
void launch_bin(hipStream_t st, const void *src, const float *dark, long long total, int rows, int cols, int bin, float *out) {
    hipLaunchKernelGGL(k_bin<T>, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, st, static_cast<const T *>(src), dark, total, rows, cols, bin,
                       rows / bin, cols / bin, out);
}

int bin_into(tomo_dff *h, hipStream_t st, const void *d_src, int dtype, long long n, int rows, int cols, int bin, const float *d_dark, float *d_out) {
    const long long total = n * (rows / bin) * (cols / bin);
    if ((total + TPB - 1) / TPB >= (1LL << 31)) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff: too many work-groups");
    if (dtype == TOMO_DFF_U16)
        launch_bin<uint16_t>(st, d_src, d_dark, total, rows, cols, bin, d_out);
    else
        launch_bin<float>(st, d_src, d_dark, total, rows, cols, bin, d_out);
    HIPCHK(h, hipGetLastError());
    return TOMO_DFF_OK;
}

}  // namespace

extern "C" {

TOMO_API int tomo_dff_abi_version(void) { return 1; }

TOMO_API int tomo_dff_create(int device, tomo_dff **out) {
    return create_plain(device, true, out);
}

TOMO_API int tomo_dff_destroy(tomo_dff *h) {
    if (!h) return TOMO_DFF_OK;
    (void)hipSetDevice(h->device);
    free_bufs(h->bufs());
    delete h;
    return TOMO_DFF_OK;
}

TOMO_API const char *tomo_dff_last_error(tomo_dff *h) { return last_error(h); }

TOMO_API int tomo_dff_check(int K, int m, int rows, int cols, int bin) {
    CHK(check_frame(nullptr, rows, cols));
    CHK(check_flats(nullptr, K));
    CHK(check_eff(nullptr, m, K));
    return check_bin(nullptr, rows, cols, bin);
}

TOMO_API int tomo_dff_gram_chunk(int K, int *chunk) {
    if (!chunk) return fail(nullptr, TOMO_DFF_ERR_ARG, "tomo_dff_gram_chunk: NULL");
    CHK(check_flats(nullptr, K));
    *chunk = gram_chunk(K);
    return TOMO_DFF_OK;
}

TOMO_API int tomo_dff_scratch_bytes(int rows, int cols, int bin, size_t *bytes) {
    if (!bytes) return fail(nullptr, TOMO_DFF_ERR_ARG, "tomo_dff_scratch_bytes: NULL");
    CHK(check_frame(nullptr, rows, cols));
    CHK(check_bin(nullptr, rows, cols, bin));
    *bytes = scratch_bytes(rows, cols, bin);
    return TOMO_DFF_OK;
}

TOMO_API int tomo_dff_batch(int n, int rows, int cols, int bin, size_t max_scratch_bytes, int *batch) {
    if (!batch) return fail(nullptr, TOMO_DFF_ERR_ARG, "tomo_dff_batch: NULL");
    if (n < 1) return fail(nullptr, TOMO_DFF_ERR_ARG, "tomo_dff_batch: n must be >= 1");
    CHK(check_frame(nullptr, rows, cols));
    CHK(check_bin(nullptr, rows, cols, bin));
    *batch = batch_for(n, rows, cols, bin, max_scratch_bytes);
    return TOMO_DFF_OK;
}

TOMO_API int tomo_dff_set_max_scratch(tomo_dff *h, size_t max_scratch_bytes) {
    if (!h) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_set_max_scratch: NULL handle");
    h->max_scratch = max_scratch_bytes;
    return TOMO_DFF_OK;
}

TOMO_API int tomo_dff_device_bytes(tomo_dff *h, int64_t *bytes) {
    if (!h || !bytes) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_device_bytes: NULL");
    *bytes = (int64_t)buf_bytes(h->bufs());
    return TOMO_DFF_OK;
}

TOMO_API int tomo_dff_gram(tomo_dff *h, void *stream, const void *d_flats, int dtype, int K, int rows, int cols, const float *d_fbar, double *G) {
    if (!h) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_gram: NULL handle");
    if (!d_flats || !d_fbar || !G) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_gram: NULL pointer");
    CHK(check_dtype(h, dtype, "tomo_dff_gram"));
    CHK(check_frame(h, rows, cols));
    CHK(check_flats(h, K));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const long long npix = (long long)rows * cols;
    const int C = gram_chunk(K), cpg = gram_cpg(C), npairs = K * (K + 1) / 2;
    const int ngroups = (int)((npix + (long long)C * cpg - 1) / ((long long)C * cpg));
    // a grow frees the old block: hipFree waits for the device, so nothing in flight still uses it
    CHK(grow(h, h->gpart, sizeof(double) * (size_t)ngroups * npairs));
    CHK(grow(h, h->G, sizeof(double) * (size_t)K * K));
    const size_t lds = sizeof(float) * ((size_t)K * (C + 1) + C);
    if (dtype == TOMO_DFF_U16)
        hipLaunchKernelGGL(k_gram<uint16_t>, dim3((unsigned)ngroups), dim3(TPB), lds, st, static_cast<const uint16_t *>(d_flats), d_fbar, K, npix, C, cpg,
                           (double *)h->gpart.p);
    else
        hipLaunchKernelGGL(k_gram<float>, dim3((unsigned)ngroups), dim3(TPB), lds, st, static_cast<const float *>(d_flats), d_fbar, K, npix, C, cpg,
                           (double *)h->gpart.p);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_gram_fold, dim3((unsigned)((npairs + TPB - 1) / TPB)), dim3(TPB), 0, st, (const double *)h->gpart.p, K, ngroups, (double *)h->G.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(G, h->G.p, sizeof(double) * (size_t)K * K, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return TOMO_DFF_OK;
}

TOMO_API int tomo_dff_eff(tomo_dff *h, void *stream, const void *d_flats, int dtype, int K, int rows, int cols, const float *d_fbar,
                          const double *V, int m, float *d_eff) {
    if (!h) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_eff: NULL handle");
    CHK(check_dtype(h, dtype, "tomo_dff_eff"));
    CHK(check_frame(h, rows, cols));
    CHK(check_flats(h, K));
    CHK(check_eff(h, m, K));
    if (m == 0) return TOMO_DFF_OK;
    if (!d_flats || !d_fbar || !V || !d_eff) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_eff: NULL pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const long long npix = (long long)rows * cols;
    CHK(grow(h, h->V, sizeof(double) * (size_t)MAXK * MAXM));
    HIPCHK(h, hipStreamSynchronize(st));                                 // an earlier call's copy out of hV has been made
    h->hV.assign(V, V + (size_t)K * m);
    HIPCHK(h, hipMemcpyAsync(h->V.p, h->hV.data(), sizeof(double) * (size_t)K * m, hipMemcpyHostToDevice, st));
    const double scale = 1.0 / std::sqrt((double)K);
    const dim3 grid((unsigned)((npix + TPB - 1) / TPB));
    if (dtype == TOMO_DFF_U16)
        hipLaunchKernelGGL(k_eff<uint16_t>, grid, dim3(TPB), 0, st, static_cast<const uint16_t *>(d_flats), d_fbar, (const double *)h->V.p, K, m, npix, scale, d_eff);
    else
        hipLaunchKernelGGL(k_eff<float>, grid, dim3(TPB), 0, st, static_cast<const float *>(d_flats), d_fbar, (const double *)h->V.p, K, m, npix, scale, d_eff);
    HIPCHK(h, hipGetLastError());
    return TOMO_DFF_OK;
}

TOMO_API int tomo_dff_bin(tomo_dff *h, void *stream, const void *d_src, int dtype, int n, int rows, int cols, int bin, const float *d_dark,
                          float *d_out) {
    if (!h) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_bin: NULL handle");
    if (n < 0) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_bin: n must be >= 0");
    CHK(check_dtype(h, dtype, "tomo_dff_bin"));
    CHK(check_frame(h, rows, cols));
    CHK(check_bin(h, rows, cols, bin));
    if (n == 0) return TOMO_DFF_OK;
    if (!d_src || !d_out) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_bin: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    return bin_into(h, reinterpret_cast<hipStream_t>(stream), d_src, dtype, n, rows, cols, bin, d_dark, d_out);
}

TOMO_API int tomo_dff_load(tomo_dff *h, void *stream, const void *d_raw, int dtype, int i0, int nb, int rows, int cols, int bin,
                           const float *d_dark) {
    if (!h) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_load: NULL handle");
    if (!d_raw) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_load: NULL pointer");
    if (i0 < 0 || nb < 1) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_load: i0 must be >= 0 and nb >= 1");
    CHK(check_dtype(h, dtype, "tomo_dff_load"));
    CHK(check_frame(h, rows, cols));
    CHK(check_bin(h, rows, cols, bin));
    if (nb > batch_for(nb, rows, cols, bin, h->max_scratch))
        return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_load: " + str(nb) + " projections exceed the scratch budget's batch of " +
                                             str(batch_for(nb, rows, cols, bin, h->max_scratch)) + " (tomo_dff_batch)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    h->nb = 0;
    const size_t need = scratch_bytes(rows, cols, bin) * (size_t)nb;
    if (h->max_scratch && h->rb.n > need && h->rb.n > h->max_scratch) {   // a block from before the budget was set: the budget bounds what is kept
        HIPCHK(h, hipFree(h->rb.p));
        h->rb.p = nullptr, h->rb.n = 0;
    }
    CHK(grow(h, h->rb, need));
    const size_t esz = dtype == TOMO_DFF_U16 ? 2 : 4;
    const char *src = static_cast<const char *>(d_raw) + (size_t)i0 * rows * cols * esz;
    CHK(bin_into(h, st, src, dtype, nb, rows, cols, bin, d_dark, (float *)h->rb.p));
    h->i0 = i0, h->nb = nb, h->zb = rows / bin, h->xb = cols / bin;
    return TOMO_DFF_OK;
}

TOMO_API int tomo_dff_cost(tomo_dff *h, void *stream, int nids, const int *ids, const float *w, const float *s, const float *a, int m, float eps,
                           const float *d_Fb, const float *d_Eb, double *fg) {
    if (!h) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_cost: NULL handle");
    CHK(check_eff(h, m, -1));
    if (h->nb == 0) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_cost: no projections are loaded (tomo_dff_load)");
    if (nids < 0 || nids > TOMO_DFF_MAX_IDS) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_cost: nids must be in 0 ... " + str(TOMO_DFF_MAX_IDS));
    if (nids == 0) return TOMO_DFF_OK;
    if (!ids || !s || !a || !d_Fb || !fg || (m > 0 && (!w || !d_Eb))) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_cost: NULL pointer");
    if (!(eps >= 0.f) || !std::isfinite(eps)) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_cost: eps must be finite and >= 0");
    for (int i = 0; i < nids; ++i)
        if (ids[i] < h->i0 || ids[i] >= h->i0 + h->nb)
            return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_cost: projection " + str(ids[i]) + " is not among the loaded " + str(h->i0) + " ... " + str(h->i0 + h->nb - 1));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const int zb = h->zb, xb = h->xb;
    const int tiles_z = (zb - 1 + TZ - 1) / TZ, tiles_x = (xb - 1 + TX - 1) / TX, ntiles = tiles_z * tiles_x;
    const int rec = 2 + m;
    CHK(grow(h, h->par, sizeof(uint32_t) * (size_t)nids * rec));
    CHK(grow(h, h->cpart, sizeof(double) * (size_t)nids * ntiles * (1 + m)));
    CHK(grow(h, h->cres, sizeof(double) * (size_t)nids * (1 + m)));
    h->hpar.resize((size_t)nids * rec);                                 // every earlier call has waited for its copy
    for (int i = 0; i < nids; ++i) {
        uint32_t *r = h->hpar.data() + (size_t)i * rec;
        r[0] = (uint32_t)(ids[i] - h->i0);
        std::memcpy(r + 1, s + i, sizeof(float));
        if (m) std::memcpy(r + 2, w + (size_t)i * m, sizeof(float) * m);
    }
    CostTable A;
    for (int j = 0; j < MAXM; ++j) A.a[j] = j < m ? a[1 + j] : 0.f;
    HIPCHK(h, hipMemcpyAsync(h->par.p, h->hpar.data(), sizeof(uint32_t) * h->hpar.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_cost, dim3((unsigned)ntiles, (unsigned)nids), dim3(TPB), sizeof(float) * (size_t)(1 + m) * PLANE, st, (const float *)h->rb.p, d_Fb,
                       d_Eb, (const uint32_t *)h->par.p, m, zb, xb, tiles_x, A, eps * eps, (double *)h->cpart.p);
    HIPCHK(h, hipGetLastError());
    const int values = nids * (1 + m);
    hipLaunchKernelGGL(k_cost_fold, dim3((unsigned)((values + TPB - 1) / TPB)), dim3(TPB), 0, st, (const double *)h->cpart.p, nids, ntiles, m,
                       (double *)h->cres.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(fg, h->cres.p, sizeof(double) * (size_t)values, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return TOMO_DFF_OK;
}

TOMO_API int tomo_dff_apply(tomo_dff *h, void *stream, const void *d_raw, int dtype, int n, int rows, int cols, const float *d_fbar,
                            const float *d_dark, const float *d_eff, int m, const float *w, int z0, int z1, int x0, int x1, int use_cutoff,
                            float cutoff, int minus_log, float min_ratio, float *d_out) {
    if (!h) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_apply: NULL handle");
    if (n < 0) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_apply: bad shape");
    CHK(check_dtype(h, dtype, "tomo_dff_apply"));
    CHK(check_frame(h, rows, cols));
    CHK(check_eff(h, m, -1));
    if (z0 < 0 || z1 > rows || z0 >= z1 || x0 < 0 || x1 > cols || x0 >= x1)
        return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_apply: crop window outside the frame or empty");
    if (n == 0) return TOMO_DFF_OK;
    if (!d_raw || !d_fbar || !d_dark || !d_out || (m > 0 && (!d_eff || !w))) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_apply: NULL pointer");
    const int nz = z1 - z0, nx = x1 - x0;
    const int tiles_z = (nz + NORM_TILE - 1) / NORM_TILE, tiles_x = (nx + NORM_TILE - 1) / NORM_TILE;
    const int groups = (n + NORM_FR - 1) / NORM_FR;
    if ((long long)tiles_z * tiles_x * groups >= (1LL << 31)) return fail(h, TOMO_DFF_ERR_ARG, "tomo_dff_apply: too many work-groups");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (m > 0) {
        CHK(grow(h, h->wts, sizeof(float) * (size_t)n * m));
        HIPCHK(h, hipStreamSynchronize(st));                             // an earlier call's copy out of hw has been made
        h->hw.assign(w, w + (size_t)n * m);
        HIPCHK(h, hipMemcpyAsync(h->wts.p, h->hw.data(), sizeof(float) * (size_t)n * m, hipMemcpyHostToDevice, st));
    }
    const dim3 grid((unsigned)(tiles_z * tiles_x * groups));
    if (dtype == TOMO_DFF_U16)
        hipLaunchKernelGGL(k_apply<uint16_t>, grid, dim3(TPB), 0, st, static_cast<const uint16_t *>(d_raw), d_fbar, d_dark, d_eff, (const float *)h->wts.p, m,
                           d_out, n, rows, cols, z0, x0, nz, nx, tiles_z, tiles_x, use_cutoff, cutoff, minus_log, min_ratio);
    else
        hipLaunchKernelGGL(k_apply<float>, grid, dim3(TPB), 0, st, static_cast<const float *>(d_raw), d_fbar, d_dark, d_eff, (const float *)h->wts.p, m, d_out,
                           n, rows, cols, z0, x0, nz, nx, tiles_z, tiles_x, use_cutoff, cutoff, minus_log, min_ratio);
    HIPCHK(h, hipGetLastError());
    return TOMO_DFF_OK;
}

}  // extern "C"
