// libtomo_vol.so: statistics, histogram, 8/16-bit conversion, cylinder mask, projections and planes of a device volume v[nx][ny][nz]
// (z fastest) on gfx950 (include/tomo_vol.h, tomography_alignment_amd/postprocess.py).
//
// The elementwise kernels share the decomposition of csrc/tomo_side_zgroups.h: groups of four z, SPAN of them a work-group (the
// histogram: a longer stretch, see below).
//
// k_stats      per lane float64 sum and sum of squares, min, max and the two counts over its groups in order; the wave by a fixed
//              shuffle tree, the four waves in order: one partial per work-group.  The grid depends on (nx, ny, nz) only.
// k_stats_fold one work-group: lane t adds the partials t, t + 256, ... in order, then the same fixed tree.  No atomics anywhere.
// k_hist       bins in LDS as uint32 (nbins * 4 bytes, dynamic), at most HIST_WGS work-groups each with a contiguous stretch of the
//              volume, so the flush to the global uint64 table is at most HIST_WGS * nbins integer atomics.  A lane merges its four
//              bins when they are equal; a wave whose lanes all hold one merged bin -- the piecewise-constant volume -- adds once.
// k_quant_xyz  codes in the layout of v: four codes are one 4-byte (uint8) or 8-byte (uint16) store where nz % 4 == 0 and out is
//              aligned to that, single codes otherwise.
// k_quant_zyx  out[z][y][x]: a TILE x TILE tile of (x, z) of one y through LDS as uint32 codes, rows of TILE + 1 dwords.  The write
//              (ds_write_b32, banks of 32, 32-lane halves): a half holds 16 z-groups of two x, dword (4 zq + k) 65 + x, bank
//              (4 zq + k + x) mod 32 -- 16 banks, 2-way, which a 4-byte LDS store hides.  The read (4-byte reads: the row stride is odd,
//              so nothing wider is aligned): lane (row r, chunk j) reads dwords r 65 + C j + i, C = 16 / sizeof(code); a half holds 8
//              rows of 4 chunks of 16 (uint8) or 4 rows of 8 chunks of 8 (uint16): bank (r + C j + i) mod 32, 2-way.  A lane packs its
//              C codes into one 16-byte store along x (WIDE: nx % C == 0 and out 16-byte aligned); single codes otherwise.
// k_mask, k_project_outer (axes 0, 1: elementwise across planes), k_project_z (a wave per row, reduced by shuffles), k_slice.
// Only vector stores and plain C++.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/tomo_vol.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_VOL_ERR_ARG, SIDE_ERR_HIP = TOMO_VOL_ERR_HIP, SIDE_ERR_NODEV = TOMO_VOL_ERR_NODEV;
}
#include "../tomo_side_host.h"
#include "../tomo_side_zgroups.h"

namespace {

constexpr int TPB = 256;
constexpr int SPAN = TOMO_VOL_SPAN_GROUPS;         // groups of one work-group of the elementwise kernels
constexpr int HIST_WGS = 2048;                     // at most this many work-groups flush a histogram
constexpr int TILE = TOMO_VOL_TILE, LD = TILE + 1;
constexpr int ZYX_MAX_GRID = 1 << 10;              // z tiles of the grid of k_quant_zyx: 2^10 * 64 = 2^31 - TOMO_VOL_MAX_NZ, so z0 stays an int
constexpr long long MAX_BLOCKS = 0xffffff;         // of 256 lanes along x of a grid: HIP takes fewer than 2^32 threads per dimension
static_assert(SPAN % TPB == 0 && TILE == 64 && TPB == 256, "a work-group walks its span 256 groups at a time; the tile maps assume 64 and 256");

struct Part {                // what one work-group of k_stats leaves
    double sum, sumsq;
    float mn, mx;
    unsigned nfin, nnon;
};

struct Stats {               // tomo_vol_stats_t on the device
    long long nfin, nnon;
    double sum, sumsq;
    float mn, mx;
};
static_assert(sizeof(Stats) == sizeof(tomo_vol_stats_t), "the device result is copied into the caller's struct as it is");

// ---------------------------------------------------------------------------------------------------------------------- device helpers

__device__ inline unsigned quant(float v, float lo, float s, unsigned qmax) {
    const float r = rintf((v - lo) * s);                                 // half to even
    return !(r > 0.f) ? 0u : (r >= (float)qmax ? qmax : (unsigned)r);    // NaN -> 0
}

// ---------------------------------------------------------------------------------------------------------------------- statistics

template <bool VEC>
__global__ __launch_bounds__(TPB) void k_stats(const float *__restrict__ v, Vol g, Part *__restrict__ part) {
    __shared__ Part sp[TPB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Walk w = walk_of(g, (long long)blockIdx.x * SPAN);
    double s = 0.0, q = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    unsigned nf = 0, nn = 0;
#pragma unroll 4
    for (unsigned off = threadIdx.x; off < SPAN; off += TPB) {
        if ((long long)off >= w.left) break;
        const auto [row, zq] = step_of(g, w, off);
        if (!inside(g, (unsigned)row)) continue;
        float f[4];
        bool in[4];
        load4<VEC>(v + row * g.nz, g.nz, zq, f, in);
        double d[4], e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool fin = finite32(f[k]);
            const bool use = in[k] && fin;
            nf += use ? 1u : 0u;
            nn += (in[k] && !fin) ? 1u : 0u;
            d[k] = use ? (double)f[k] : 0.0;
            e[k] = d[k] * d[k];
            if (use) mn = fminf(mn, f[k]), mx = fmaxf(mx, f[k]);
        }
        s += ((d[0] + d[1]) + d[2]) + d[3];
        q += ((e[0] + e[1]) + e[2]) + e[3];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s += __shfl_down(s, o, 64);
        q += __shfl_down(q, o, 64);
        mn = fminf(mn, __shfl_down(mn, o, 64));
        mx = fmaxf(mx, __shfl_down(mx, o, 64));
        nf += __shfl_down(nf, o, 64);
        nn += __shfl_down(nn, o, 64);
    }
    if (lane == 0) sp[wave] = Part{s, q, mn, mx, nf, nn};
    __syncthreads();
    if (threadIdx.x == 0) {
        Part p = sp[0];
        for (int j = 1; j < TPB / 64; ++j) {
            p.sum += sp[j].sum, p.sumsq += sp[j].sumsq;
            p.mn = fminf(p.mn, sp[j].mn), p.mx = fmaxf(p.mx, sp[j].mx);
            p.nfin += sp[j].nfin, p.nnon += sp[j].nnon;
        }
        part[blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(TPB) void k_stats_fold(const Part *__restrict__ part, long long n, Stats *__restrict__ out) {
    __shared__ Stats ss[TPB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s = 0.0, q = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    long long nf = 0, nn = 0;
#pragma unroll 8
    for (long long i = threadIdx.x; i < n; i += TPB) {                   // unrolled: eight loads in flight, the adds in order
        const Part p = part[i];
        s += p.sum, q += p.sumsq;
        mn = fminf(mn, p.mn), mx = fmaxf(mx, p.mx);
        nf += p.nfin, nn += p.nnon;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s += __shfl_down(s, o, 64);
        q += __shfl_down(q, o, 64);
        mn = fminf(mn, __shfl_down(mn, o, 64));
        mx = fmaxf(mx, __shfl_down(mx, o, 64));
        nf += __shfl_down(nf, o, 64);
        nn += __shfl_down(nn, o, 64);
    }
    if (lane == 0) ss[wave] = Stats{nf, nn, s, q, mn, mx};
    __syncthreads();
    if (threadIdx.x == 0) {
        Stats r = ss[0];
        for (int j = 1; j < TPB / 64; ++j) {
            r.sum += ss[j].sum, r.sumsq += ss[j].sumsq;
            r.mn = fminf(r.mn, ss[j].mn), r.mx = fmaxf(r.mx, ss[j].mx);
            r.nfin += ss[j].nfin, r.nnon += ss[j].nnon;
        }
        if (r.nfin == 0) r.mn = r.mx = NAN;
        *out = r;
    }
}

// ---------------------------------------------------------------------------------------------------------------------- histogram

// table: uint64 [nbins] counts, then under, over, nonfinite.  span: the groups of one work-group, a multiple of TPB.
template <bool VEC>
__global__ __launch_bounds__(TPB) void k_hist(const float *__restrict__ v, Vol g, unsigned span, float lo, float hi, float scale, int nbins,
                                              unsigned long long *__restrict__ table) {
    extern __shared__ unsigned bins[];
    const int lane = threadIdx.x & 63;
    for (int b = threadIdx.x; b < nbins; b += TPB) bins[b] = 0u;
    __syncthreads();
    const Walk w = walk_of(g, (long long)blockIdx.x * span);
    unsigned under = 0, over = 0, nonf = 0;
    for (unsigned off = threadIdx.x; off - threadIdx.x < span; off += TPB) {     // uniform trip count: the wave votes inside
        bool live = (long long)off < w.left;
        long long row = 0;
        unsigned zq = 0;
        if (live) {
            const Step s = step_of(g, w, off);
            zq = s.zq, row = s.row;
            live = inside(g, (unsigned)row);
        }
        int b[4] = {-1, -1, -1, -1};                                     // -1: nothing to add to a bin
        if (live) {
            float f[4];
            bool in[4];
            load4<VEC>(v + row * g.nz, g.nz, zq, f, in);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!in[k]) continue;
                const float x = f[k];
                if (!finite32(x)) ++nonf;
                else if (x < lo) ++under;
                else if (x > hi) ++over;
                else b[k] = min((int)floorf((x - lo) * scale), nbins - 1);
            }
        }
        const bool one = b[0] >= 0 && b[0] == b[1] && b[0] == b[2] && b[0] == b[3];      // the lane's four values share a bin
        const int first = __builtin_amdgcn_readfirstlane(b[0]);
        if (__all(one && b[0] == first)) {                               // ... and so does the whole wave
            if (lane == 0) atomicAdd(&bins[first], 4u * 64u);
        } else if (one) {
            atomicAdd(&bins[b[0]], 4u);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (b[k] >= 0) atomicAdd(&bins[b[k]], 1u);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        under += __shfl_down(under, o, 64);
        over += __shfl_down(over, o, 64);
        nonf += __shfl_down(nonf, o, 64);
    }
    if (lane == 0) {
        if (under) atomicAdd(&table[nbins], (unsigned long long)under);
        if (over) atomicAdd(&table[nbins + 1], (unsigned long long)over);
        if (nonf) atomicAdd(&table[nbins + 2], (unsigned long long)nonf);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += TPB) {
        const unsigned c = bins[i];
        if (c) atomicAdd(&table[i], (unsigned long long)c);
    }
}

// ---------------------------------------------------------------------------------------------------------------------- quantize, mask

// out[x][y][z].  PACK: nz % 4 == 0 and out aligned to four codes.
template <typename T, bool VEC, bool PACK>
__global__ __launch_bounds__(TPB) void k_quant_xyz(const float *__restrict__ v, Vol g, float lo, float s, unsigned qmax, unsigned fill,
                                                   T *__restrict__ out) {
    const Walk w = walk_of(g, (long long)blockIdx.x * SPAN);
#pragma unroll 4
    for (unsigned off = threadIdx.x; off < SPAN; off += TPB) {
        if ((long long)off >= w.left) break;
        const auto [row, zq] = step_of(g, w, off);
        const int z = 4 * (int)zq;
        unsigned c[4] = {fill, fill, fill, fill};
        bool in[4];
        if (inside(g, (unsigned)row)) {
            float f[4];
            load4<VEC>(v + row * g.nz, g.nz, zq, f, in);
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = quant(f[k], lo, s, qmax);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) in[k] = z + k < g.nz;
        }
        T *dst = out + row * g.nz + z;
        if (PACK) {
            if (sizeof(T) == 1)
                *reinterpret_cast<unsigned *>(dst) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
            else
                *reinterpret_cast<uint2 *>(dst) = make_uint2(c[0] | (c[1] << 16), c[2] | (c[3] << 16));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (in[k]) dst[k] = (T)c[k];
        }
    }
}

// out[z][y][x].  grid (min(z tiles, ZYX_MAX_GRID), ny, x tiles): a work-group takes the z tiles blockIdx.x, blockIdx.x + gridDim.x, ...
// WIDE: nx % (16 / sizeof(T)) == 0 and out 16-byte aligned.
template <typename T, bool VEC, bool WIDE>
__global__ __launch_bounds__(TPB) void k_quant_zyx(const float *__restrict__ v, Vol g, float lo, float s, unsigned qmax, unsigned fill,
                                                   T *__restrict__ out) {
    __shared__ unsigned tile[TILE][LD];                                  // [z][x]
    const int y = blockIdx.y, x0 = blockIdx.z * TILE;
    const int t = threadIdx.x;
    for (int z0 = blockIdx.x * TILE; z0 < g.nz; z0 += (int)gridDim.x * TILE) {      // z0 < nz + ZYX_MAX_GRID * TILE <= 2^31
    {
        const int zq = t & 15, xr = t >> 4;
        const int z = z0 + 4 * zq;
#pragma unroll
        for (int p = 0; p < TILE / 16; ++p) {
            const int xl = xr + 16 * p, x = x0 + xl;
            if (x < g.nx && z < g.nz) {
                const unsigned row = (unsigned)x * (unsigned)g.ny + (unsigned)y;
                unsigned c[4] = {fill, fill, fill, fill};
                if (inside(g, row)) {
                    float f[4];
                    bool in[4];
                    load4<VEC>(v + (long long)row * g.nz, g.nz, (unsigned)(z >> 2), f, in);
#pragma unroll
                    for (int k = 0; k < 4; ++k) c[k] = quant(f[k], lo, s, qmax);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) tile[4 * zq + k][xl] = c[k];        // rows past nz are written and never read
            }
        }
    }
    __syncthreads();
    constexpr int C = 16 / (int)sizeof(T);                               // codes of one 16-byte store
    constexpr int L = TILE / C;                                          // lanes of one output row of the tile
    constexpr int ROWS = TPB / L;                                        // rows of one pass
    const int j = t % L, r0 = t / L;
#pragma unroll
    for (int p = 0; p < TILE / ROWS; ++p) {
        const int r = r0 + p * ROWS, z = z0 + r, x = x0 + j * C;
        if (z >= g.nz || x >= g.nx) continue;
        unsigned c[C];
#pragma unroll
        for (int i = 0; i < C; ++i) c[i] = tile[r][j * C + i];
        T *dst = out + ((long long)z * g.ny + y) * g.nx + x;
        if (WIDE) {                                                      // nx % C == 0: the whole chunk is inside the row
            uint4 u;
            if (sizeof(T) == 1) {
                u.x = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
                u.y = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
                u.z = c[8 % C] | (c[9 % C] << 8) | (c[10 % C] << 16) | (c[11 % C] << 24);
                u.w = c[12 % C] | (c[13 % C] << 8) | (c[14 % C] << 16) | (c[15 % C] << 24);
            } else {
                u.x = c[0] | (c[1] << 16), u.y = c[2] | (c[3] << 16), u.z = c[4] | (c[5] << 16), u.w = c[6] | (c[7] << 16);
            }
            *reinterpret_cast<uint4 *>(dst) = u;
        } else {
#pragma unroll
            for (int i = 0; i < C; ++i)
                if (x + i < g.nx) dst[i] = (T)c[i];
        }
    }
    __syncthreads();                                                     // the tile is free for the next z0
    }
}

// VOUT: nz % 4 == 0 and out 16-byte aligned.  out may be v: a lane reads its group before it writes it.
template <bool VEC, bool VOUT>
__global__ __launch_bounds__(TPB) void k_mask(const float *v, Vol g, float value, float *out) {
    const Walk w = walk_of(g, (long long)blockIdx.x * SPAN);
#pragma unroll 4
    for (unsigned off = threadIdx.x; off < SPAN; off += TPB) {
        if ((long long)off >= w.left) break;
        const auto [row, zq] = step_of(g, w, off);
        const int z = 4 * (int)zq;
        float f[4] = {value, value, value, value};
        bool in[4];
        if (inside(g, (unsigned)row)) {
            load4<VEC>(v + row * g.nz, g.nz, zq, f, in);
            if (out == v) continue;                                      // in place: the inside stays as it is
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) in[k] = z + k < g.nz;
        }
        float *dst = out + row * g.nz + z;
        if (VOUT) {
            *reinterpret_cast<float4 *>(dst) = make_float4(f[0], f[1], f[2], f[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (in[k]) dst[k] = f[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------- projections, planes

template <bool MIN>
__device__ inline float pick(float a, float b) { return MIN ? fminf(a, b) : fmaxf(a, b); }

// out[a][z] = op over b of v[a sa + b sb + z]: axis 0 (a = y, b = x) and axis 1 (a = x, b = y).  A lane owns one group of four z of one a.
template <bool MIN, bool VEC>
__global__ __launch_bounds__(TPB) void k_project_outer(const float *__restrict__ v, int nz, unsigned G, int na, long long sa, int nb, long long sb,
                                                       float *__restrict__ out) {
    const long long gid = (long long)blockIdx.x * TPB + threadIdx.x;
    if (gid >= (long long)na * G) return;
    const unsigned a = (unsigned)(gid / G), zq = (unsigned)(gid - (long long)a * G);
    const float none = MIN ? INFINITY : -INFINITY;
    float acc[4] = {none, none, none, none};
    bool in[4] = {false, false, false, false};
    const float *base = v + a * sa;
#pragma unroll 4
    for (int b = 0; b < nb; ++b) {
        float f[4];
        load4<VEC>(base + b * sb, nz, zq, f, in);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (in[k] && finite32(f[k])) acc[k] = pick<MIN>(acc[k], f[k]);
    }
    float *dst = out + (long long)a * nz + 4 * (int)zq;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (in[k]) dst[k] = acc[k] == none ? NAN : acc[k];
}

// out[row] = op over z of v[row][z]: a wave per row (x, y).
template <bool MIN, bool VEC>
__global__ __launch_bounds__(TPB) void k_project_z(const float *__restrict__ v, int nz, unsigned G, long long rows, float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;                                             // the whole wave
    const float none = MIN ? INFINITY : -INFINITY;
    float acc = none;
    const float *base = v + row * nz;
    for (unsigned zq = lane; zq < G; zq += 64) {
        float f[4];
        bool in[4];
        load4<VEC>(base, nz, zq, f, in);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (in[k] && finite32(f[k])) acc = pick<MIN>(acc, f[k]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc = pick<MIN>(acc, __shfl_down(acc, o, 64));
    if (lane == 0) out[row] = acc == none ? NAN : acc;
}

// out[i][j] = v[base + i s0 + j s1] as bits.
__global__ __launch_bounds__(TPB) void k_slice(const unsigned *__restrict__ v, long long base, int n0, long long s0, int n1, long long s1,
                                               unsigned *__restrict__ out) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= (long long)n0 * n1) return;
    const long long i = idx / n1, j = idx - i * n1;
    out[idx] = v[base + i * s0 + j * s1];
}

}  // namespace

struct tomo_vol {
    int device = 0;
    std::string err;
    Buf part;                // Part [work-groups of k_stats]
    Buf stats;               // Stats
    Buf table;               // uint64 [nbins + 3]
    bool have_stats = false;
    int nbins = 0;           // of the last tomo_vol_histogram; 0 before it
    auto bufs() { return std::array{&part, &stats, &table}; }
};

namespace {

int check_shape(tomo_vol *h, long long nx, long long ny, long long nz) {
    if (nx < 1 || ny < 1 || nz < 1 || nx > TOMO_VOL_MAX_DIM || ny > TOMO_VOL_MAX_DIM || nz > (long long)TOMO_VOL_MAX_NZ)
        return fail(h, TOMO_VOL_ERR_UNSUPPORTED, "tomo_vol: a volume of " + std::to_string(nx) + " x " + std::to_string(ny) + " x " + std::to_string(nz) +
                                                     " is outside 1 <= nx, ny <= " + std::to_string(TOMO_VOL_MAX_DIM) + ", 1 <= nz <= " +
                                                     std::to_string((long long)TOMO_VOL_MAX_NZ) + "; nothing was launched");
    if ((nx * ny * ((nz + 3) / 4) + SPAN - 1) / SPAN > MAX_BLOCKS)
        return fail(h, TOMO_VOL_ERR_UNSUPPORTED, "tomo_vol: a volume of " + std::to_string(nx) + " x " + std::to_string(ny) + " x " + std::to_string(nz) +
                                                     " is more than one grid of work-groups; nothing was launched");
    return TOMO_VOL_OK;
}

// What every entry point checks first.
int check_call(tomo_vol *h, const char *what, const void *d_v, int nx, int ny, int nz) {
    if (!h) return fail(h, TOMO_VOL_ERR_ARG, std::string(what) + ": NULL handle");
    if (!d_v) return fail(h, TOMO_VOL_ERR_ARG, std::string(what) + ": NULL pointer");
    if (!aligned(d_v, 4)) return fail(h, TOMO_VOL_ERR_ARG, std::string(what) + ": misaligned pointer");
    return check_shape(h, nx, ny, nz);
}

}  // namespace

extern "C" {

TOMO_API int tomo_vol_abi_version(void) { return 1; }

TOMO_API int tomo_vol_create(int device, tomo_vol **out) {
    return create_plain(device, true, out);
}

TOMO_API int tomo_vol_destroy(tomo_vol *h) {
    if (!h) return TOMO_VOL_OK;
    (void)hipSetDevice(h->device);
    free_bufs(h->bufs());
    delete h;
    return TOMO_VOL_OK;
}

TOMO_API const char *tomo_vol_last_error(tomo_vol *h) { return last_error(h); }

TOMO_API int tomo_vol_device_bytes(tomo_vol *h, int64_t *bytes) {
    if (!h || !bytes) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_device_bytes: NULL");
    *bytes = (int64_t)buf_bytes(h->bufs());
    return TOMO_VOL_OK;
}

TOMO_API int tomo_vol_check_shape(int64_t nx, int64_t ny, int64_t nz) { return check_shape(nullptr, nx, ny, nz); }

TOMO_API int tomo_vol_fetch_stats(tomo_vol *h, void *stream, tomo_vol_stats_t *out) {
    if (!h) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_fetch_stats: NULL handle");
    if (!h->have_stats) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_fetch_stats: no statistics were computed (tomo_vol_stats)");
    if (!out) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_fetch_stats: NULL pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(out, h->stats.p, sizeof(Stats), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return TOMO_VOL_OK;
}

TOMO_API int tomo_vol_stats(tomo_vol *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, tomo_vol_stats_t *out) {
    CHK(check_call(h, "tomo_vol_stats", d_v, nx, ny, nz));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    h->have_stats = false;
    const Vol g = vol_of(nx, ny, nz, R4);
    const unsigned nb = span_blocks(g, SPAN);
    // a grow frees the old block: hipFree waits for the device, so nothing in flight still uses it
    CHK(grow(h, h->part, sizeof(Part) * (size_t)nb));
    CHK(grow(h, h->stats, sizeof(Stats)));
    if (nz % 4 == 0 && aligned(d_v, 16))
        hipLaunchKernelGGL(k_stats<true>, dim3(nb), dim3(TPB), 0, st, d_v, g, (Part *)h->part.p);
    else
        hipLaunchKernelGGL(k_stats<false>, dim3(nb), dim3(TPB), 0, st, d_v, g, (Part *)h->part.p);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_stats_fold, dim3(1), dim3(TPB), 0, st, (const Part *)h->part.p, (long long)nb, (Stats *)h->stats.p);
    HIPCHK(h, hipGetLastError());
    h->have_stats = true;
    if (out) return tomo_vol_fetch_stats(h, stream, out);
    return TOMO_VOL_OK;
}

TOMO_API int tomo_vol_fetch_histogram(tomo_vol *h, void *stream, uint64_t *counts, uint64_t *extra) {
    if (!h) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_fetch_histogram: NULL handle");
    if (h->nbins == 0) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_fetch_histogram: no histogram was computed (tomo_vol_histogram)");
    if (!counts || !extra) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_fetch_histogram: NULL pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const uint64_t *t = static_cast<const uint64_t *>(h->table.p);
    HIPCHK(h, hipMemcpyAsync(counts, t, sizeof(uint64_t) * (size_t)h->nbins, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(extra, t + h->nbins, sizeof(uint64_t) * 3, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return TOMO_VOL_OK;
}

TOMO_API int tomo_vol_histogram(tomo_vol *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, float lo, float hi, int nbins,
                                uint64_t *counts, uint64_t *extra) {
    CHK(check_call(h, "tomo_vol_histogram", d_v, nx, ny, nz));
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi) || !std::isfinite(hi - lo))
        return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_histogram: the range needs finite lo < hi; nothing was launched");
    if (nbins < 1 || nbins > TOMO_VOL_MAX_BINS)
        return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_histogram: " + std::to_string(nbins) + " bins are outside 1 ... " + std::to_string(TOMO_VOL_MAX_BINS) +
                                             "; nothing was launched");
    if ((counts || extra) && !(counts && extra)) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_histogram: counts and extra must be both NULL or both given");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    h->nbins = 0;
    const Vol g = vol_of(nx, ny, nz, R4);
    CHK(grow(h, h->table, sizeof(uint64_t) * (TOMO_VOL_MAX_BINS + 3)));
    HIPCHK(h, hipMemsetAsync(h->table.p, 0, sizeof(uint64_t) * (size_t)(nbins + 3), st));
    const long long wgs = std::min<long long>((g.groups + SPAN - 1) / SPAN, HIST_WGS);
    long long span = (g.groups + wgs - 1) / wgs;
    span = (span + TPB - 1) / TPB * TPB;                                 // groups <= MAX_BLOCKS * SPAN (check_shape): span < 2^26, so a
                                                                         // work-group's counts, four values a group, fit uint32
    const unsigned nb = (unsigned)((g.groups + span - 1) / span);
    const float scale = (float)nbins / (hi - lo);
    const size_t lds = sizeof(unsigned) * (size_t)nbins;
    auto *table = static_cast<unsigned long long *>(h->table.p);
        if (nz % 4 == 0 && aligned(d_v, 16)) {
        HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_hist<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * TOMO_VOL_MAX_BINS));
        hipLaunchKernelGGL(k_hist<true>, dim3(nb), dim3(TPB), lds, st, d_v, g, (unsigned)span, lo, hi, scale, nbins, table);
    } else {
        HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_hist<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * TOMO_VOL_MAX_BINS));
        hipLaunchKernelGGL(k_hist<false>, dim3(nb), dim3(TPB), lds, st, d_v, g, (unsigned)span, lo, hi, scale, nbins, table);
    }
    HIPCHK(h, hipGetLastError());
    h->nbins = nbins;
    if (counts) return tomo_vol_fetch_histogram(h, stream, counts, extra);
    return TOMO_VOL_OK;
}

TOMO_API int tomo_vol_quantize(tomo_vol *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, float lo, float hi, int bits,
                               int order, int fill, void *d_out) {
    CHK(check_call(h, "tomo_vol_quantize", d_v, nx, ny, nz));
    if (!d_out) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_quantize: NULL pointer");
    if (bits != 8 && bits != 16) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_quantize: bits must be 8 or 16");
    if (order != 0 && order != 1) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_quantize: order must be 0 (xyz) or 1 (zyx)");
    if (bits == 16 && !aligned(d_out, 2)) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_quantize: misaligned output pointer");
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi) || !std::isfinite(hi - lo))
        return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_quantize: the window needs finite lo < hi; nothing was launched");
    const unsigned qmax = bits == 8 ? 255u : 65535u;
    if (fill < 0 || (unsigned)fill > qmax) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_quantize: fill is outside 0 ... qmax");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const Vol g = vol_of(nx, ny, nz, R4);
    const float s = (float)qmax / (hi - lo);
    const bool vec = nz % 4 == 0 && aligned(d_v, 16);
    const unsigned f = (unsigned)fill;
#define VOL_LAUNCH(K, T, A, B, grid) hipLaunchKernelGGL((K<T, A, B>), grid, dim3(TPB), 0, st, d_v, g, lo, s, qmax, f, static_cast<T *>(d_out))
#define VOL_PICK(K, T, a, b, grid)                     \
    do {                                               \
        if (a && b) VOL_LAUNCH(K, T, true, true, grid);        \
        else if (a) VOL_LAUNCH(K, T, true, false, grid);       \
        else if (b) VOL_LAUNCH(K, T, false, true, grid);       \
        else VOL_LAUNCH(K, T, false, false, grid);             \
    } while (0)
    if (order == 0) {
        const dim3 grid(span_blocks(g, SPAN));
        const bool pack = nz % 4 == 0 && aligned(d_out, (uintptr_t)(bits / 2));       // four codes: 4 or 8 bytes
        if (bits == 8) VOL_PICK(k_quant_xyz, uint8_t, vec, pack, grid);
        else VOL_PICK(k_quant_xyz, uint16_t, vec, pack, grid);
    } else {
        const dim3 grid((unsigned)std::min((nz + TILE - 1) / TILE, ZYX_MAX_GRID), (unsigned)ny, (unsigned)((nx + TILE - 1) / TILE));
        const bool wide = nx % (128 / bits) == 0 && aligned(d_out, 16);
        if (bits == 8) VOL_PICK(k_quant_zyx, uint8_t, vec, wide, grid);
        else VOL_PICK(k_quant_zyx, uint16_t, vec, wide, grid);
    }
#undef VOL_PICK
#undef VOL_LAUNCH
    HIPCHK(h, hipGetLastError());
    return TOMO_VOL_OK;
}

TOMO_API int tomo_vol_mask(tomo_vol *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, float value, float *d_out) {
    CHK(check_call(h, "tomo_vol_mask", d_v, nx, ny, nz));
    if (!d_out) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_mask: NULL pointer");
    if (!aligned(d_out, 4)) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_mask: misaligned output pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const Vol g = vol_of(nx, ny, nz, R4);
    const bool vec = nz % 4 == 0 && aligned(d_v, 16), vout = nz % 4 == 0 && aligned(d_out, 16);
    const dim3 grid(span_blocks(g, SPAN));
    if (vec && vout) hipLaunchKernelGGL((k_mask<true, true>), grid, dim3(TPB), 0, st, d_v, g, value, d_out);
    else if (vec) hipLaunchKernelGGL((k_mask<true, false>), grid, dim3(TPB), 0, st, d_v, g, value, d_out);
    else if (vout) hipLaunchKernelGGL((k_mask<false, true>), grid, dim3(TPB), 0, st, d_v, g, value, d_out);
    else hipLaunchKernelGGL((k_mask<false, false>), grid, dim3(TPB), 0, st, d_v, g, value, d_out);
    HIPCHK(h, hipGetLastError());
    return TOMO_VOL_OK;
}

TOMO_API int tomo_vol_project(tomo_vol *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, int axis, int op, float *d_out) {
    (void)R4;
    CHK(check_call(h, "tomo_vol_project", d_v, nx, ny, nz));
    if (!d_out || !aligned(d_out, 4)) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_project: NULL or misaligned output pointer");
    if (axis < 0 || axis > 2) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_project: axis must be 0, 1 or 2");
    if (op != 0 && op != 1) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_project: op must be 0 (max) or 1 (min)");
    const unsigned G = (unsigned)(((long long)nz + 3) / 4);
    const long long plane = (long long)ny * nz;
    const int na = axis == 0 ? ny : nx, nb = axis == 0 ? nx : ny;
    const long long sa = axis == 0 ? nz : plane, sb = axis == 0 ? plane : nz;
    const long long rows = (long long)nx * ny;
    const long long blocks = axis == 2 ? (rows + TPB / 64 - 1) / (TPB / 64) : ((long long)na * G + TPB - 1) / TPB;
    if (blocks > MAX_BLOCKS) return fail(h, TOMO_VOL_ERR_UNSUPPORTED, "tomo_vol_project: the plane is too large for one grid; nothing was launched");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const bool vec = nz % 4 == 0 && aligned(d_v, 16);
    const dim3 grid((unsigned)blocks);
#define VOL_PROJECT(MIN, VEC)                                                                                                 \
    do {                                                                                                                      \
        if (axis == 2) hipLaunchKernelGGL((k_project_z<MIN, VEC>), grid, dim3(TPB), 0, st, d_v, nz, G, rows, d_out);              \
        else hipLaunchKernelGGL((k_project_outer<MIN, VEC>), grid, dim3(TPB), 0, st, d_v, nz, G, na, sa, nb, sb, d_out);          \
    } while (0)
    if (op == 1 && vec) VOL_PROJECT(true, true);
    else if (op == 1) VOL_PROJECT(true, false);
    else if (vec) VOL_PROJECT(false, true);
    else VOL_PROJECT(false, false);
#undef VOL_PROJECT
    HIPCHK(h, hipGetLastError());
    return TOMO_VOL_OK;
}

TOMO_API int tomo_vol_slice(tomo_vol *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, int axis, int index, float *d_out) {
    (void)R4;
    CHK(check_call(h, "tomo_vol_slice", d_v, nx, ny, nz));
    if (!d_out || !aligned(d_out, 4)) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_slice: NULL or misaligned output pointer");
    if (axis < 0 || axis > 2) return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_slice: axis must be 0, 1 or 2");
    const int len = axis == 0 ? nx : axis == 1 ? ny : nz;
    if (index < 0 || index >= len)
        return fail(h, TOMO_VOL_ERR_ARG, "tomo_vol_slice: index " + std::to_string(index) + " is outside 0 ... " + std::to_string(len - 1));
    const long long plane = (long long)ny * nz;
    const int n0 = axis == 0 ? ny : nx, n1 = axis == 2 ? ny : nz;
    const long long s0 = axis == 0 ? nz : plane, s1 = axis == 2 ? nz : 1;
    const long long base = (long long)index * (axis == 0 ? plane : axis == 1 ? nz : 1);
    const long long blocks = ((long long)n0 * n1 + TPB - 1) / TPB;
    if (blocks > MAX_BLOCKS) return fail(h, TOMO_VOL_ERR_UNSUPPORTED, "tomo_vol_slice: the plane is too large for one grid; nothing was launched");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_slice, dim3((unsigned)blocks), dim3(TPB), 0, st, reinterpret_cast<const unsigned *>(d_v), base, n0, s0, n1, s1,
                       reinterpret_cast<unsigned *>(d_out));
    HIPCHK(h, hipGetLastError());
    return TOMO_VOL_OK;
}

}  // extern "C"
