// libtomo_seg.so: threshold, 3-D connected-component labels, per-component measures, small-component removal and the largest component
// of a device volume [nx][ny][nz] (z fastest) on gfx950 (include/tomo_seg.h, tomography_alignment_amd/segment.py).
//
// The elementwise kernels share the decomposition of csrc/tomo_side_zgroups.h: groups of four z (one 16-byte access of float32 /
// int32, one 4-byte access of four mask bytes), SPAN of them a work-group, i.e. a stretch of the volume in linear-index order.
//
// Labelling is union-find on the label array L itself (int32).  Invariant: the parent L[i] of a foreground voxel i is a foreground
// index <= i of the same component; the background holds SENT = 2^31 - 1, which is no index (a volume has at most 2^31 - 1 voxels).
//   find(i)      follows L while L[i] != i: strictly decreasing indices, so it ends, whatever other lanes do meanwhile (parents only
//                ever decrease; a value read late is still an ancestor).
//   unite(a, b)  a = find(a), b = find(b); with a < b: old = atomicMin(&L[b], a).  old == b: b was a root and now hangs under a.  old < b:
//                b had a parent already, L[b] is now min(old, a), and what is left is to unite a with old: max(a, b) has dropped, so
//                the loop ends.  No lane ever waits for another lane's store.
// k_tile      a work-group per brick of 8 x 8 x 64 voxels (a grid-stride loop over the bricks).  The mask goes to LDS as one 64-bit
//             word per row (64 rows); a foreground voxel's first parent is the start of its run along z, read off that word; the lane
//             that owns a run's start unites it with the runs it touches in the (up to four) rows before it, walking the set bits of
//             the neighbour row's word under the run's mask (widened by one z where the connectivity has that diagonal): ds_min
//             atomics on int P[4096].  Then L[i] = the global index of find(i); local and global order agree inside a brick.
// k_border    every foreground voxel on a brick face looks at its neighbours of smaller linear index (1, 3 + 6, 3 + 6 + 4 of them for
//             connectivity 1, 2, 3) that lie in another brick and unites with the foreground ones; then points itself at its root.
// k_compress  L[i] = find(i); the roots (L[i] == i) of the work-group's stretch counted into counts[block].
// k_scan      one work-group of 1024 lanes: exclusive prefix sum of counts in place, the total behind it.
// k_rank      the roots again, in linear order inside the stretch (wave prefix by shuffles, waves through LDS): L[root] = -(rank + 1).
// k_final     L[i] = 0 (SENT), -L[i] (a root), |L[L[i]]| (the root may or may not have turned itself positive already).
// k_measure   per lane the four voxels.  Up to AGG_ROUNDS times per step the wave takes the next label of its first lane that still has
//             one, every lane folds its voxels of that label into one update, and where at least AGG_MIN_LANES lanes hold it the
//             updates are reduced by shuffles (the other lanes hold the neutral element) and lane 0 commits; fewer lanes commit
//             their own.  What is left goes voxel by voxel.  So a component that fills the wave, or most of it, costs one update a
//             wave and does not serialise on its addresses.  Integer atomics for count, bbox and coordinate sums, ordered-integer
//             atomics for the float minimum and maximum, a float64 atomic add for the sum.  Labels outside the pass's range
//             (l0, l1] are skipped.
// k_count, k_scan (mode 1), k_relabel: remove_small.  k_count, k_argmax, k_pick: largest.
// Only vector stores and plain C++.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/tomo_seg.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_SEG_ERR_ARG, SIDE_ERR_HIP = TOMO_SEG_ERR_HIP, SIDE_ERR_NODEV = TOMO_SEG_ERR_NODEV;
}
#include "../tomo_side_host.h"
#include "../tomo_side_zgroups.h"

namespace {

constexpr int TPB = 256;
constexpr int SPAN = TOMO_SEG_SPAN_GROUPS;
constexpr int BX = TOMO_SEG_TILE_X, BY = TOMO_SEG_TILE_Y, BZ = TOMO_SEG_TILE_Z;
constexpr int ROWS = BX * BY, BVOX = ROWS * BZ;
constexpr int SENT = INT_MAX;
constexpr int SCAN_TPB = 1024, SCAN_ITEMS = 8;
constexpr long long TILE_MAX_GRID = 1 << 20;
constexpr int AGG_ROUNDS = 3;                      // labels a wave of k_measure / k_count combines across its lanes per step
constexpr int AGG_MIN_LANES = 4;                   // ... when at least this many lanes hold the label
static_assert(SPAN % TPB == 0 && BX == 8 && BY == 8 && BZ == 64 && TPB == 256, "the brick maps assume 8 x 8 x 64 and 256 lanes");

struct Tab {                 // the tables of one pass of measure, entry = label - 1 - l0
    unsigned long long *count;
    int *bbox;               // [.][6]
    unsigned long long *csum;        // [.][3]
    int *vmn, *vmx;          // ordered-integer codes of the float minimum and maximum
    double *vsum;
};

struct Acc {                 // what some voxels of one label add to the tables
    int lab;
    unsigned cnt;
    int x0, x1, y0, y1, z0, z1;
    long long sx, sy, sz;
    float fmn, fmx;
    double fs;
};

// ---------------------------------------------------------------------------------------------------------------------- device helpers

// Parents are read with relaxed atomic loads: the compiler may not keep one in a register, and every value ever stored is an ancestor.
__device__ inline int ld_global(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline int ld_local(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

template <bool LOCAL>
__device__ inline int find(const int *P, int i) {
    for (;;) {
        const int p = LOCAL ? ld_local(P + i) : ld_global(P + i);
        if (p == i) return i;
        i = p;                                                           // p < i
    }
}

template <bool LOCAL>
__device__ inline void unite(int *P, int a, int b) {
    a = find<LOCAL>(P, a);
    b = find<LOCAL>(P, b);
    while (a != b) {
        if (a > b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = atomicMin(P + b, a);                             // a < b
        if (old == b) return;                                            // b was a root
        a = find<LOCAL>(P, a);                                           // b had the parent old < b: a and old remain to be united
        b = find<LOCAL>(P, old);
    }
}

__device__ inline unsigned long long zmask(int lo, int hi) {             // bits lo ... hi, 0 <= lo <= hi <= 63
    const unsigned long long upto = hi == 63 ? ~0ULL : (1ULL << (hi + 1)) - 1ULL;
    return upto & ~((1ULL << lo) - 1ULL);
}

__device__ inline int enc(float f) {                                     // monotone float -> int, -0 below +0
    const int i = __float_as_int(f);
    return i < 0 ? i ^ 0x7fffffff : i;
}

// ---------------------------------------------------------------------------------------------------------------------- threshold

template <bool VEC, bool PACK>
__global__ __launch_bounds__(TPB) void k_threshold(const float *__restrict__ v, Vol g, float lo, float hi, int has_lo, int has_hi,
                                                   uint8_t *__restrict__ out) {
    const Walk w = walk_of(g, (long long)blockIdx.x * SPAN);
#pragma unroll 4
    for (unsigned off = threadIdx.x; off < SPAN; off += TPB) {
        if ((long long)off >= w.left) break;
        const auto [row, zq] = step_of(g, w, off);
        unsigned c[4] = {0u, 0u, 0u, 0u};
        if (inside(g, (unsigned)row)) {
            float f[4];
            bool in[4];
            load4<VEC>(v + row * g.nz, g.nz, zq, f, in);
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = (in[k] && f[k] == f[k] && (!has_lo || f[k] >= lo) && (!has_hi || f[k] <= hi)) ? 1u : 0u;
        }
        store4b<PACK>(out + row * g.nz, g.nz, zq, c);
    }
}

// ---------------------------------------------------------------------------------------------------------------------- labels

// MVEC: nz % 4 == 0 and the mask 4-byte aligned; LVEC: nz % 4 == 0 and the labels 16-byte aligned.
template <bool MVEC, bool LVEC>
__global__ __launch_bounds__(TPB) void k_tile(const uint8_t *__restrict__ mask, int *__restrict__ L, int nx, int ny, int nz, int nby, int nbz,
                                              long long nbricks, int conn) {
    __shared__ unsigned bits[ROWS * 2];                                  // row r: words 2r (z 0 ... 31) and 2r + 1
    __shared__ int P[BVOX];
    const int t = threadIdx.x, zq = t & 15, r0 = t >> 4;
    for (long long b = blockIdx.x; b < nbricks; b += gridDim.x) {
        const int bz = (int)(b % nbz);
        const long long q = b / nbz;
        const int by = (int)(q % nby), bx = (int)(q / nby);
        const int x0 = bx * BX, y0 = by * BY, z0 = bz * BZ;
        if (t < ROWS * 2) bits[t] = 0u;
        __syncthreads();
        unsigned nib[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = r0 + 16 * p, x = x0 + (r >> 3), y = y0 + (r & 7), z = z0 + 4 * zq;
            nib[p] = 0u;
            if (x < nx && y < ny && z < nz) {
                const uint8_t *src = mask + ((long long)x * ny + y) * nz + z;
                if (MVEC) {
                    const unsigned u = *reinterpret_cast<const unsigned *>(src);
                    nib[p] = ((u & 0xffu) ? 1u : 0u) | ((u & 0xff00u) ? 2u : 0u) | ((u & 0xff0000u) ? 4u : 0u) | ((u & 0xff000000u) ? 8u : 0u);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (z + k < nz && src[k]) nib[p] |= 1u << k;
                }
                if (nib[p]) atomicOr(&bits[2 * r + (zq >> 3)], nib[p] << (4 * (zq & 7)));
            }
        }
        __syncthreads();
        // first parents: the start of the voxel's run along z
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (!nib[p]) continue;
            const int r = r0 + 16 * p;
            const unsigned long long rb = bits[2 * r] | ((unsigned long long)bits[2 * r + 1] << 32);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!((nib[p] >> k) & 1u)) continue;
                const int lz = 4 * zq + k;
                const unsigned long long below = ~rb & ((1ULL << lz) - 1ULL);
                const int s = below ? 64 - __clzll((long long)below) : 0;
                P[r * BZ + lz] = r * BZ + s;
            }
        }
        __syncthreads();
        // the owner of a run's start unites it with the runs it touches in the rows before it
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (!nib[p]) continue;
            const int r = r0 + 16 * p, lx = r >> 3, ly = r & 7;
            const unsigned long long rb = bits[2 * r] | ((unsigned long long)bits[2 * r + 1] << 32);
            for (int k = 0; k < 4; ++k) {
                if (!((nib[p] >> k) & 1u)) continue;
                const int lz = 4 * zq + k;
                if (lz > 0 && ((rb >> (lz - 1)) & 1ULL)) continue;       // not a start
                const unsigned long long rest = ~(rb >> lz);             // bit j: voxel lz + j is background (or past the brick)
                const int e = lz + (rest ? __ffsll((long long)rest) - 1 : 64 - lz) - 1;
                const unsigned long long narrow = zmask(lz, e), wide = zmask(lz > 0 ? lz - 1 : 0, e < 63 ? e + 1 : 63);
                const int me = r * BZ + lz;
                int nr[4];
                unsigned long long nm[4];
                nr[0] = lx > 0 ? r - 8 : -1, nm[0] = conn >= 2 ? wide : narrow;                              // (x - 1, y)
                nr[1] = ly > 0 ? r - 1 : -1, nm[1] = nm[0];                                                  // (x, y - 1)
                nr[2] = (conn >= 2 && lx > 0 && ly > 0) ? r - 9 : -1, nm[2] = conn == 3 ? wide : narrow;      // (x - 1, y - 1)
                nr[3] = (conn >= 2 && lx > 0 && ly < 7) ? r - 7 : -1, nm[3] = nm[2];                         // (x - 1, y + 1)
                for (int j = 0; j < 4; ++j) {
                    if (nr[j] < 0) continue;
                    unsigned long long nb = (bits[2 * nr[j]] | ((unsigned long long)bits[2 * nr[j] + 1] << 32)) & nm[j];
                    while (nb) {
                        const int z1 = __ffsll((long long)nb) - 1;
                        unite<true>(P, me, nr[j] * BZ + z1);
                        nb &= nb + (nb & (0ULL - nb));                   // drop the run that starts at the lowest set bit
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = r0 + 16 * p, x = x0 + (r >> 3), y = y0 + (r & 7), z = z0 + 4 * zq;
            if (!(x < nx && y < ny && z < nz)) continue;
            int v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = SENT;
                if ((nib[p] >> k) & 1u) {
                    const int root = find<true>(P, r * BZ + 4 * zq + k);
                    v[k] = (int)(((long long)(x0 + (root >> 9)) * ny + (y0 + ((root >> 6) & 7))) * nz + z0 + (root & 63));
                }
            }
            store4i<LVEC>(L + ((long long)x * ny + y) * nz, nz, (unsigned)(z >> 2), v);
        }
        __syncthreads();                                                 // bits and P are free for the next brick
    }
}

template <int CONN, bool VEC>
__global__ __launch_bounds__(TPB) void k_border(int *L, Vol g) {
    const Walk w = walk_of(g, (long long)blockIdx.x * SPAN);
    for (unsigned off = threadIdx.x; off < SPAN; off += TPB) {
        if ((long long)off >= w.left) break;
        const auto [row, zq] = step_of(g, w, off);
        const int x = (int)(row / g.ny), y = (int)(row - (long long)x * g.ny);
        const int lx = x & (BX - 1), ly = y & (BY - 1), lq = (int)(zq & 15u);
        const bool rowc = lx == 0 || ly == 0 || (CONN > 1 && ly == BY - 1);
        if (!(rowc || lq == 0 || (CONN > 1 && lq == 15))) continue;
        int v[4];
        bool in[4];
        load4i<VEC>(L + row * g.nz, g.nz, zq, v, in);
        for (int k = 0; k < 4; ++k) {
            if (!in[k] || v[k] == SENT) continue;
            const int z = 4 * (int)zq + k, lz = z & (BZ - 1);
            if (!(rowc || lz == 0 || (CONN > 1 && lz == BZ - 1))) continue;
            const int i = (int)(row * g.nz + z);
            bool any = false;
#pragma unroll
            for (int dx = -1; dx <= 0; ++dx)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dz = -1; dz <= 1; ++dz) {
                        const bool before = dx < 0 || (dx == 0 && (dy < 0 || (dy == 0 && dz < 0)));
                        if (!before || (dx != 0) + (dy != 0) + (dz != 0) > CONN) continue;
                        const int xj = x + dx, yj = y + dy, zj = z + dz;
                        if (xj < 0 || yj < 0 || yj >= g.ny || zj < 0 || zj >= g.nz) continue;
                        if ((xj >> 3) == (x >> 3) && (yj >> 3) == (y >> 3) && (zj >> 6) == (z >> 6)) continue;      // the tile pass did it
                        const int j = (int)(((long long)xj * g.ny + yj) * g.nz + zj);
                        if (ld_global(L + j) == SENT) continue;
                        unite<false>(L, i, j);
                        any = true;
                    }
            if (any) {
                const int r = find<false>(L, i);
                if (r != i) atomicMin(L + i, r);                         // an ancestor: shortens what the next find walks
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void k_compress(int *L, Vol g, int *__restrict__ counts) {
    __shared__ int ws[TPB / 64];
    const Walk w = walk_of(g, (long long)blockIdx.x * SPAN);
    int roots = 0;
    for (unsigned off = threadIdx.x; off < SPAN; off += TPB) {
        if ((long long)off >= w.left) break;
        const auto [row, zq] = step_of(g, w, off);
        int v[4];
        bool in[4];
        load4i<VEC>(L + row * g.nz, g.nz, zq, v, in);
        const int i0 = (int)(row * g.nz + 4 * (long long)zq);
        int pprev = SENT, rprev = SENT;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!in[k] || v[k] == SENT) continue;
            const int p = v[k];
            v[k] = p == pprev ? rprev : find<false>(L, p);               // the voxels of a run share a parent
            pprev = p, rprev = v[k];
            roots += v[k] == i0 + k ? 1 : 0;
        }
        store4i<VEC>(L + row * g.nz, g.nz, zq, v);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) roots += __shfl_down(roots, o, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = roots;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// One work-group.  mode 0: a[0 ... n) becomes its exclusive prefix sum, a[n] the total.  mode 1: a holds counts; a[i] becomes the new
// label of component i + 1: its rank + 1 among those with a[i] >= min_size, or 0.  *total: the sum / the number kept.
__global__ __launch_bounds__(SCAN_TPB) void k_scan(int *a, long long n, int mode, unsigned min_size, int *total) {
    __shared__ int ws[SCAN_TPB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (long long base = 0; base < n; base += SCAN_TPB * SCAN_ITEMS) {
        const long long i0 = base + (long long)threadIdx.x * SCAN_ITEMS;
        int v[SCAN_ITEMS], s = 0;
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            int x = i0 + j < n ? a[i0 + j] : 0;
            if (mode) x = (i0 + j < n && (unsigned)x >= min_size) ? 1 : 0;
            v[j] = x;
            s += x;
        }
        int inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) ws[wave] = inc;
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int j = 0; j < SCAN_TPB / 64; ++j) {
            before += j < wave ? ws[j] : 0;
            tot += ws[j];
        }
        int ex = carry + before + inc - s;
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            if (i0 + j < n) a[i0 + j] = mode ? (v[j] ? ex + 1 : 0) : ex;
            ex += v[j];
        }
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (!mode) a[n] = carry;
        *total = carry;
    }
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void k_rank(int *L, Vol g, const int *__restrict__ prefix) {
    __shared__ int ws[TPB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Walk w = walk_of(g, (long long)blockIdx.x * SPAN);
    int base = prefix[blockIdx.x];
    for (unsigned off = threadIdx.x; off - threadIdx.x < SPAN; off += TPB) {         // uniform trip count: barriers inside
        const bool live = (long long)off < w.left;
        bool root[4] = {false, false, false, false};
        long long i0 = 0;
        int c = 0;
        if (live) {
            const auto [row, zq] = step_of(g, w, off);
            int v[4];
            bool in[4];
            load4i<VEC>(L + row * g.nz, g.nz, zq, v, in);
            i0 = row * g.nz + 4 * (long long)zq;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                root[k] = in[k] && (long long)v[k] == i0 + k;
                c += root[k] ? 1 : 0;
            }
        }
        int inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) ws[wave] = inc;
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int j = 0; j < TPB / 64; ++j) {
            before += j < wave ? ws[j] : 0;
            tot += ws[j];
        }
        int ex = base + before + inc - c;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (root[k]) L[i0 + k] = -(ex++ + 1);
        base += tot;
        __syncthreads();
    }
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void k_final(int *L, Vol g) {
    const Walk w = walk_of(g, (long long)blockIdx.x * SPAN);
    for (unsigned off = threadIdx.x; off < SPAN; off += TPB) {
        if ((long long)off >= w.left) break;
        const auto [row, zq] = step_of(g, w, off);
        int v[4], out[4];
        bool in[4];
        load4i<VEC>(L + row * g.nz, g.nz, zq, v, in);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            out[k] = 0;
            if (!in[k] || v[k] == SENT) continue;
            if (v[k] < 0) out[k] = -v[k];
            else if (k > 0 && in[k - 1] && v[k] == v[k - 1]) out[k] = out[k - 1];
            else {
                const int r = ld_global(L + v[k]);                       // the root's -(rank + 1), or rank + 1 if it got there first
                out[k] = r < 0 ? -r : r;
            }
        }
        store4i<VEC>(L + row * g.nz, g.nz, zq, out);
    }
}

// ---------------------------------------------------------------------------------------------------------------------- measure

__global__ __launch_bounds__(TPB) void k_tab_init(Tab t, long long m, int with_vol) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    t.count[i] = 0ULL;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        t.bbox[6 * i + 2 * a] = INT_MAX;
        t.bbox[6 * i + 2 * a + 1] = INT_MIN;
        t.csum[3 * i + a] = 0ULL;
    }
    if (with_vol) {
        t.vmn[i] = INT_MAX;                                              // both decode to NaN
        t.vmx[i] = INT_MIN;
        t.vsum[i] = 0.0;
    }
}

template <bool WITHVOL>
__device__ inline void commit(const Tab &t, const Acc &a, int l0) {
    const long long i = (long long)a.lab - 1 - l0;
    atomicAdd(t.count + i, (unsigned long long)a.cnt);
    atomicMin(t.bbox + 6 * i + 0, a.x0);
    atomicMax(t.bbox + 6 * i + 1, a.x1);
    atomicMin(t.bbox + 6 * i + 2, a.y0);
    atomicMax(t.bbox + 6 * i + 3, a.y1);
    atomicMin(t.bbox + 6 * i + 4, a.z0);
    atomicMax(t.bbox + 6 * i + 5, a.z1);
    atomicAdd(t.csum + 3 * i + 0, (unsigned long long)a.sx);
    atomicAdd(t.csum + 3 * i + 1, (unsigned long long)a.sy);
    atomicAdd(t.csum + 3 * i + 2, (unsigned long long)a.sz);
    if (WITHVOL && a.fmn <= a.fmx) {                                     // it has a finite value
        atomicMin(t.vmn + i, enc(a.fmn));
        atomicMax(t.vmx + i, enc(a.fmx));
        atomicAdd(t.vsum + i, a.fs);
    }
}

// Labels in (l0, l1] are measured.
template <bool VEC, bool WITHVOL>
__global__ __launch_bounds__(TPB) void k_measure(const int *__restrict__ L, const float *__restrict__ vol, Vol g, int l0, int l1, Tab t) {
    const int lane = threadIdx.x & 63;
    const Walk w = walk_of(g, (long long)blockIdx.x * SPAN);
    for (unsigned off = threadIdx.x; off - threadIdx.x < SPAN; off += TPB) {         // uniform trip count: the wave votes inside
        const bool live = (long long)off < w.left;
        int lab[4] = {0, 0, 0, 0};
        float f[4] = {0.f, 0.f, 0.f, 0.f};
        int x = 0, y = 0, z = 0;
        if (live) {
            const auto [row, zq] = step_of(g, w, off);
            bool in[4];
            load4i<VEC>(L + row * g.nz, g.nz, zq, lab, in);
            if (WITHVOL) load4<VEC>(vol + row * g.nz, g.nz, zq, f, in);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (!in[k] || lab[k] <= l0 || lab[k] > l1) lab[k] = 0;
            x = (int)(row / g.ny), y = (int)(row - (long long)x * g.ny), z = 4 * (int)zq;
        }
        unsigned todo = 0u;                                              // the lane's voxels that still have to be added
#pragma unroll
        for (int k = 0; k < 4; ++k) todo |= lab[k] > 0 ? 1u << k : 0u;
        for (int it = 0; it < AGG_ROUNDS; ++it) {                        // every condition on `have` and `who` is wave-uniform
            const unsigned long long have = __ballot(todo != 0u);
            if (!have) break;
            const int mine = todo ? lab[__ffs((int)todo) - 1] : 0;
            const int target = __shfl(mine, __ffsll((long long)have) - 1, 64);        // the next label of the first lane that has one
            Acc a;
            a.lab = target, a.cnt = 0u;
            a.x0 = a.y0 = a.z0 = INT_MAX, a.x1 = a.y1 = a.z1 = INT_MIN;
            a.sx = a.sy = a.sz = 0;
            a.fmn = INFINITY, a.fmx = -INFINITY, a.fs = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!((todo >> k) & 1u) || lab[k] != target) continue;
                todo &= ~(1u << k);
                a.cnt += 1u;
                a.x0 = a.x1 = x, a.y0 = a.y1 = y, a.z0 = min(a.z0, z + k), a.z1 = max(a.z1, z + k);
                a.sx += x, a.sy += y, a.sz += z + k;
                if (WITHVOL && finite32(f[k])) a.fmn = fminf(a.fmn, f[k]), a.fmx = fmaxf(a.fmx, f[k]), a.fs += (double)f[k];
            }
            const unsigned long long who = __ballot(a.cnt != 0u);
            if (__popcll(who) < AGG_MIN_LANES) {                         // few lanes: their own atomics are cheaper than the tree
                if (a.cnt) commit<WITHVOL>(t, a, l0);
                continue;
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {                          // the other lanes hold the neutral element
                a.cnt += __shfl_down(a.cnt, o, 64);
                a.x0 = min(a.x0, __shfl_down(a.x0, o, 64)), a.x1 = max(a.x1, __shfl_down(a.x1, o, 64));
                a.y0 = min(a.y0, __shfl_down(a.y0, o, 64)), a.y1 = max(a.y1, __shfl_down(a.y1, o, 64));
                a.z0 = min(a.z0, __shfl_down(a.z0, o, 64)), a.z1 = max(a.z1, __shfl_down(a.z1, o, 64));
                a.sx += __shfl_down(a.sx, o, 64), a.sy += __shfl_down(a.sy, o, 64), a.sz += __shfl_down(a.sz, o, 64);
                if (WITHVOL) {
                    a.fmn = fminf(a.fmn, __shfl_down(a.fmn, o, 64)), a.fmx = fmaxf(a.fmx, __shfl_down(a.fmx, o, 64));
                    a.fs += __shfl_down(a.fs, o, 64);
                }
            }
            if (lane == 0) commit<WITHVOL>(t, a, l0);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                    // what the rounds left: labels rare in this wave
            if (!((todo >> k) & 1u)) continue;
            Acc a;
            a.lab = lab[k], a.cnt = 1u;
            a.x0 = a.x1 = x, a.y0 = a.y1 = y, a.z0 = a.z1 = z + k;
            a.sx = x, a.sy = y, a.sz = z + k;
            const bool fin = WITHVOL && finite32(f[k]);
            a.fmn = fin ? f[k] : INFINITY, a.fmx = fin ? f[k] : -INFINITY, a.fs = fin ? (double)f[k] : 0.0;
            commit<WITHVOL>(t, a, l0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------- sizes

// table[label - 1] += the voxels of the label, 1 <= label <= n.
template <bool VEC>
__global__ __launch_bounds__(TPB) void k_count(const int *__restrict__ L, Vol g, int n, unsigned *__restrict__ table) {
    const int lane = threadIdx.x & 63;
    const Walk w = walk_of(g, (long long)blockIdx.x * SPAN);
    for (unsigned off = threadIdx.x; off - threadIdx.x < SPAN; off += TPB) {         // uniform trip count: the wave votes inside
        const bool live = (long long)off < w.left;
        int lab[4] = {0, 0, 0, 0};
        if (live) {
            const auto [row, zq] = step_of(g, w, off);
            bool in[4];
            load4i<VEC>(L + row * g.nz, g.nz, zq, lab, in);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (!in[k] || lab[k] < 1 || lab[k] > n) lab[k] = 0;
        }
        unsigned todo = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) todo |= lab[k] > 0 ? 1u << k : 0u;
        for (int it = 0; it < AGG_ROUNDS; ++it) {                        // as in k_measure
            const unsigned long long have = __ballot(todo != 0u);
            if (!have) break;
            const int mine = todo ? lab[__ffs((int)todo) - 1] : 0;
            const int target = __shfl(mine, __ffsll((long long)have) - 1, 64);
            unsigned c = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (((todo >> k) & 1u) && lab[k] == target) todo &= ~(1u << k), c += 1u;
            const unsigned long long who = __ballot(c != 0u);
            if (__popcll(who) < AGG_MIN_LANES) {
                if (c) atomicAdd(table + (target - 1), c);
                continue;
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) c += __shfl_down(c, o, 64);
            if (lane == 0) atomicAdd(table + (target - 1), c);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((todo >> k) & 1u) atomicAdd(table + (lab[k] - 1), 1u);
    }
}

// One work-group: res[0] = the label with the largest count, the lowest among equals (-1 when n = 0), res[1] = that count.
__global__ __launch_bounds__(TPB) void k_argmax(const unsigned *__restrict__ table, int n, int *__restrict__ res) {
    __shared__ unsigned sc[TPB];
    __shared__ int sl[TPB];
    unsigned best = 0u;
    int label = -1;
    for (int i = threadIdx.x; i < n; i += TPB) {
        const unsigned c = table[i];
        if (label < 0 || c > best) best = c, label = i + 1;              // i rises: a later equal count does not replace
    }
    sc[threadIdx.x] = best, sl[threadIdx.x] = label;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < TPB; ++j)
            if (sl[j] >= 0 && (label < 0 || sc[j] > best || (sc[j] == best && sl[j] < label))) best = sc[j], label = sl[j];
        res[0] = label, res[1] = (int)best;
    }
}

template <bool VEC, bool PACK>
__global__ __launch_bounds__(TPB) void k_pick(const int *__restrict__ L, Vol g, const int *__restrict__ res, uint8_t *__restrict__ out) {
    const Walk w = walk_of(g, (long long)blockIdx.x * SPAN);
    const int want = res[0];
    for (unsigned off = threadIdx.x; off < SPAN; off += TPB) {
        if ((long long)off >= w.left) break;
        const auto [row, zq] = step_of(g, w, off);
        int v[4];
        bool in[4];
        load4i<VEC>(L + row * g.nz, g.nz, zq, v, in);
        unsigned c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = (in[k] && v[k] == want) ? 1u : 0u;
        store4b<PACK>(out + row * g.nz, g.nz, zq, c);
    }
}

// out = table[label - 1] for 1 <= label <= n, 0 otherwise; out may be L (a lane reads its group before it writes it).
template <bool VEC, bool VOUT>
__global__ __launch_bounds__(TPB) void k_relabel(const int *L, Vol g, int n, const int *__restrict__ table, int *out) {
    const Walk w = walk_of(g, (long long)blockIdx.x * SPAN);
    for (unsigned off = threadIdx.x; off < SPAN; off += TPB) {
        if ((long long)off >= w.left) break;
        const auto [row, zq] = step_of(g, w, off);
        int v[4], o[4];
        bool in[4];
        load4i<VEC>(L + row * g.nz, g.nz, zq, v, in);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k] = 0;
            if (!in[k] || v[k] < 1 || v[k] > n) continue;
            o[k] = (k > 0 && v[k] == v[k - 1]) ? o[k - 1] : table[v[k] - 1];
        }
        store4i<VOUT>(out + row * g.nz, g.nz, zq, o);
    }
}

}  // namespace

struct tomo_seg {
    int device = 0;
    std::string err;
    Buf cnt;                 // int [work-groups + 1]: the root counts and their prefix sums
    Buf tab;                 // measure's tables of one pass; the sizes of remove_small and largest
    Buf res;                 // two int: what k_scan and k_argmax hand back
    size_t max_scratch = 0;  // 0: TOMO_SEG_DEFAULT_SCRATCH
    auto bufs() { return std::array{&cnt, &tab, &res}; }
};

namespace {

std::string dims(long long nx, long long ny, long long nz) { return std::to_string(nx) + " x " + std::to_string(ny) + " x " + std::to_string(nz); }

int check_shape(tomo_seg *h, long long nx, long long ny, long long nz) {
    if (nx < 1 || ny < 1 || nz < 1 || nx > TOMO_SEG_MAX_DIM || ny > TOMO_SEG_MAX_DIM || nz > (long long)TOMO_SEG_MAX_VOXELS)
        return fail(h, TOMO_SEG_ERR_UNSUPPORTED, "tomo_seg: a volume of " + dims(nx, ny, nz) + " is outside 1 <= nx, ny <= " +
                                                     std::to_string(TOMO_SEG_MAX_DIM) + ", 1 <= nz; nothing was launched");
    if (nx * ny * nz > (long long)TOMO_SEG_MAX_VOXELS)                   // at most 2^28 * (2^31 - 1): no overflow
        return fail(h, TOMO_SEG_ERR_UNSUPPORTED, "tomo_seg: a volume of " + dims(nx, ny, nz) + " has more than 2^31 - 1 voxels; nothing was launched");
    // groups <= nx ny nz < 2^31, so there are fewer than 2^21 + 1 work-groups of SPAN groups (span_blocks): one grid.
    return TOMO_SEG_OK;
}

int check_call(tomo_seg *h, const char *what, const void *p, uintptr_t align, const void *q, uintptr_t qalign, int nx, int ny, int nz) {
    if (!h) return fail(h, TOMO_SEG_ERR_ARG, std::string(what) + ": NULL handle");
    if (!p || !q) return fail(h, TOMO_SEG_ERR_ARG, std::string(what) + ": NULL pointer");
    if (!aligned(p, align) || !aligned(q, qalign)) return fail(h, TOMO_SEG_ERR_ARG, std::string(what) + ": misaligned pointer");
    return check_shape(h, nx, ny, nz);
}

// Scratch above TOMO_SEG_KEEP_BYTES goes back before a call returns (the call has waited for the stream by then).
void release(tomo_seg *h) {
    for (Buf *b : h->bufs())
        if (b->p && b->n > (size_t)TOMO_SEG_KEEP_BYTES) {
            (void)hipFree(b->p);
            b->p = nullptr, b->n = 0;
        }
}

size_t entry_bytes(bool with_vol) { return 8 + 24 + 24 + (with_vol ? 16 : 0); }

long long labels_per_pass(bool with_vol, size_t budget) {
    if (budget == 0) budget = (size_t)TOMO_SEG_DEFAULT_SCRATCH;
    return std::max<long long>(1, (long long)(budget / entry_bytes(with_vol)));
}

Tab tab_of(void *base, long long m, bool with_vol) {                     // every table 8-byte aligned: m is rounded up to even
    Tab t;
    char *p = static_cast<char *>(base);
    t.count = reinterpret_cast<unsigned long long *>(p), p += 8 * m;
    t.csum = reinterpret_cast<unsigned long long *>(p), p += 24 * m;
    t.vsum = reinterpret_cast<double *>(p), p += with_vol ? 8 * m : 0;
    t.bbox = reinterpret_cast<int *>(p), p += 24 * m;
    t.vmn = reinterpret_cast<int *>(p), p += with_vol ? 4 * m : 0;
    t.vmx = reinterpret_cast<int *>(p);
    return t;
}

inline float dec(int i) {                                                // an untouched entry (INT_MAX / INT_MIN): the quiet NaN
    if (i == INT_MAX || i == INT_MIN) return std::nanf("");
    const int b = i < 0 ? i ^ 0x7fffffff : i;
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

// The sizes of the components 1 ... n into h->tab as unsigned [n].
int count_sizes(tomo_seg *h, hipStream_t st, const int32_t *d_labels, const Vol &g, int n) {
    CHK(grow(h, h->tab, sizeof(unsigned) * (size_t)std::max(n, 1)));
    HIPCHK(h, hipMemsetAsync(h->tab.p, 0, sizeof(unsigned) * (size_t)std::max(n, 1), st));
    if (g.nz % 4 == 0 && aligned(d_labels, 16))
        hipLaunchKernelGGL(k_count<true>, dim3(span_blocks(g, SPAN)), dim3(TPB), 0, st, d_labels, g, n, (unsigned *)h->tab.p);
    else
        hipLaunchKernelGGL(k_count<false>, dim3(span_blocks(g, SPAN)), dim3(TPB), 0, st, d_labels, g, n, (unsigned *)h->tab.p);
    HIPCHK(h, hipGetLastError());
    return TOMO_SEG_OK;
}

}  // namespace

extern "C" {

TOMO_API int tomo_seg_abi_version(void) { return 1; }

TOMO_API int tomo_seg_create(int device, tomo_seg **out) {
    return create_plain(device, true, out);
}

TOMO_API int tomo_seg_destroy(tomo_seg *h) {
    if (!h) return TOMO_SEG_OK;
    (void)hipSetDevice(h->device);
    free_bufs(h->bufs());
    delete h;
    return TOMO_SEG_OK;
}

TOMO_API const char *tomo_seg_last_error(tomo_seg *h) { return last_error(h); }

TOMO_API int tomo_seg_device_bytes(tomo_seg *h, int64_t *bytes) {
    if (!h || !bytes) return fail(h, TOMO_SEG_ERR_ARG, "tomo_seg_device_bytes: NULL");
    *bytes = (int64_t)buf_bytes(h->bufs());
    return TOMO_SEG_OK;
}

TOMO_API int tomo_seg_check_shape(int64_t nx, int64_t ny, int64_t nz) { return check_shape(nullptr, nx, ny, nz); }

TOMO_API int tomo_seg_set_max_scratch(tomo_seg *h, size_t max_scratch_bytes) {
    if (!h) return fail(h, TOMO_SEG_ERR_ARG, "tomo_seg_set_max_scratch: NULL handle");
    h->max_scratch = max_scratch_bytes;
    return TOMO_SEG_OK;
}

TOMO_API int tomo_seg_measure_passes(int64_t n, int with_vol, size_t max_scratch_bytes, int *passes) {
    if (!passes || n < 0 || n > (int64_t)TOMO_SEG_MAX_VOXELS) return fail(nullptr, TOMO_SEG_ERR_ARG, "tomo_seg_measure_passes: bad argument");
    const long long per = labels_per_pass(with_vol != 0, max_scratch_bytes);
    *passes = (int)((n + per - 1) / per);
    return TOMO_SEG_OK;
}

TOMO_API int tomo_seg_threshold(tomo_seg *h, void *stream, const float *d_v, int nx, int ny, int nz, int64_t R4, float lo, float hi, int has_lo,
                                int has_hi, uint8_t *d_mask) {
    CHK(check_call(h, "tomo_seg_threshold", d_v, 4, d_mask, 1, nx, ny, nz));
    if (!has_lo && !has_hi) return fail(h, TOMO_SEG_ERR_ARG, "tomo_seg_threshold: at least one bound must be given; nothing was launched");
    if ((has_lo && !std::isfinite(lo)) || (has_hi && !std::isfinite(hi)))
        return fail(h, TOMO_SEG_ERR_ARG, "tomo_seg_threshold: a given bound must be finite; nothing was launched");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const Vol g = vol_of(nx, ny, nz, R4);
    const bool vec = nz % 4 == 0 && aligned(d_v, 16), pack = nz % 4 == 0 && aligned(d_mask, 4);
    const dim3 grid(span_blocks(g, SPAN));
    const int a = has_lo ? 1 : 0, b = has_hi ? 1 : 0;
    if (vec && pack) hipLaunchKernelGGL((k_threshold<true, true>), grid, dim3(TPB), 0, st, d_v, g, lo, hi, a, b, d_mask);
    else if (vec) hipLaunchKernelGGL((k_threshold<true, false>), grid, dim3(TPB), 0, st, d_v, g, lo, hi, a, b, d_mask);
    else if (pack) hipLaunchKernelGGL((k_threshold<false, true>), grid, dim3(TPB), 0, st, d_v, g, lo, hi, a, b, d_mask);
    else hipLaunchKernelGGL((k_threshold<false, false>), grid, dim3(TPB), 0, st, d_v, g, lo, hi, a, b, d_mask);
    HIPCHK(h, hipGetLastError());
    return TOMO_SEG_OK;
}

TOMO_API int tomo_seg_label(tomo_seg *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int connectivity, int32_t *d_labels,
                            int32_t *n) {
    CHK(check_call(h, "tomo_seg_label", d_mask, 1, d_labels, 4, nx, ny, nz));
    if (!n) return fail(h, TOMO_SEG_ERR_ARG, "tomo_seg_label: NULL pointer");
    if (connectivity < 1 || connectivity > 3) return fail(h, TOMO_SEG_ERR_ARG, "tomo_seg_label: connectivity must be 1, 2 or 3; nothing was launched");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const Vol g = vol_of(nx, ny, nz, -1);
    const unsigned nb = span_blocks(g, SPAN);
    CHK(grow(h, h->cnt, sizeof(int) * ((size_t)nb + 1)));
    CHK(grow(h, h->res, sizeof(int) * 2));
    int *counts = static_cast<int *>(h->cnt.p), *res = static_cast<int *>(h->res.p);
    const int nbx = (nx + BX - 1) / BX, nby = (ny + BY - 1) / BY, nbz = (nz + BZ - 1) / BZ;
    const long long nbricks = (long long)nbx * nby * nbz;
    const bool mvec = nz % 4 == 0 && aligned(d_mask, 4), lvec = nz % 4 == 0 && aligned(d_labels, 16);
    const dim3 tgrid((unsigned)std::min(nbricks, TILE_MAX_GRID)), grid(nb);
#define SEG_TILE(A, B) hipLaunchKernelGGL((k_tile<A, B>), tgrid, dim3(TPB), 0, st, d_mask, d_labels, nx, ny, nz, nby, nbz, nbricks, connectivity)
    if (mvec && lvec) SEG_TILE(true, true);
    else if (mvec) SEG_TILE(true, false);
    else if (lvec) SEG_TILE(false, true);
    else SEG_TILE(false, false);
#undef SEG_TILE
    HIPCHK(h, hipGetLastError());
#define SEG_PASS(K, ...)                                                                         \
    do {                                                                                         \
        if (lvec) hipLaunchKernelGGL((K<true>), grid, dim3(TPB), 0, st, d_labels, g, ##__VA_ARGS__);  \
        else hipLaunchKernelGGL((K<false>), grid, dim3(TPB), 0, st, d_labels, g, ##__VA_ARGS__);      \
        HIPCHK(h, hipGetLastError());                                                            \
    } while (0)
    if (nbricks > 1) {
#define SEG_BORDER(C)                                                                            \
    do {                                                                                         \
        if (lvec) hipLaunchKernelGGL((k_border<C, true>), grid, dim3(TPB), 0, st, d_labels, g);   \
        else hipLaunchKernelGGL((k_border<C, false>), grid, dim3(TPB), 0, st, d_labels, g);       \
    } while (0)
        if (connectivity == 1) SEG_BORDER(1);
        else if (connectivity == 2) SEG_BORDER(2);
        else SEG_BORDER(3);
#undef SEG_BORDER
        HIPCHK(h, hipGetLastError());
    }
    SEG_PASS(k_compress, counts);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(SCAN_TPB), 0, st, counts, (long long)nb, 0, 0u, res);
    HIPCHK(h, hipGetLastError());
    SEG_PASS(k_rank, (const int *)counts);
    SEG_PASS(k_final);
#undef SEG_PASS
    HIPCHK(h, hipMemcpyAsync(n, res, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    release(h);
    return TOMO_SEG_OK;
}

TOMO_API int tomo_seg_measure(tomo_seg *h, void *stream, const int32_t *d_labels, const float *d_v, int nx, int ny, int nz, int32_t n,
                              int64_t *count, int32_t *bbox, int64_t *coord_sum, float *vmin, float *vmax, double *vsum) {
    CHK(check_call(h, "tomo_seg_measure", d_labels, 4, d_v ? (const void *)d_v : (const void *)d_labels, 4, nx, ny, nz));
    if (n < 0) return fail(h, TOMO_SEG_ERR_ARG, "tomo_seg_measure: n < 0");
    const bool with_vol = d_v != nullptr;
    if (n > 0 && (!count || !bbox || !coord_sum || (with_vol && (!vmin || !vmax || !vsum))))
        return fail(h, TOMO_SEG_ERR_ARG, "tomo_seg_measure: NULL table");
    if (n == 0) return TOMO_SEG_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const Vol g = vol_of(nx, ny, nz, -1);
    const long long per = std::min<long long>(labels_per_pass(with_vol, h->max_scratch), n);
    const long long m = (per + 1) / 2 * 2;
    CHK(grow(h, h->tab, entry_bytes(with_vol) * (size_t)m));
    const Tab t = tab_of(h->tab.p, m, with_vol);
    const bool vec = nz % 4 == 0 && aligned(d_labels, 16) && (!with_vol || aligned(d_v, 16));
    const dim3 grid(span_blocks(g, SPAN));
    std::vector<int> codes;
    for (long long l0 = 0; l0 < n; l0 += per) {
        const long long k = std::min<long long>(per, n - l0);
        hipLaunchKernelGGL(k_tab_init, dim3((unsigned)((k + TPB - 1) / TPB)), dim3(TPB), 0, st, t, k, with_vol ? 1 : 0);
        HIPCHK(h, hipGetLastError());
        const int a = (int)l0, b = (int)(l0 + k);
        if (vec && with_vol) hipLaunchKernelGGL((k_measure<true, true>), grid, dim3(TPB), 0, st, d_labels, d_v, g, a, b, t);
        else if (vec) hipLaunchKernelGGL((k_measure<true, false>), grid, dim3(TPB), 0, st, d_labels, d_v, g, a, b, t);
        else if (with_vol) hipLaunchKernelGGL((k_measure<false, true>), grid, dim3(TPB), 0, st, d_labels, d_v, g, a, b, t);
        else hipLaunchKernelGGL((k_measure<false, false>), grid, dim3(TPB), 0, st, d_labels, d_v, g, a, b, t);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(count + l0, t.count, 8 * (size_t)k, hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipMemcpyAsync(bbox + 6 * l0, t.bbox, 24 * (size_t)k, hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipMemcpyAsync(coord_sum + 3 * l0, t.csum, 24 * (size_t)k, hipMemcpyDeviceToHost, st));
        if (with_vol) {
            HIPCHK(h, hipMemcpyAsync(vmin + l0, t.vmn, 4 * (size_t)k, hipMemcpyDeviceToHost, st));
            HIPCHK(h, hipMemcpyAsync(vmax + l0, t.vmx, 4 * (size_t)k, hipMemcpyDeviceToHost, st));
            HIPCHK(h, hipMemcpyAsync(vsum + l0, t.vsum, 8 * (size_t)k, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(h, hipStreamSynchronize(st));                             // the next pass reuses the tables
        if (with_vol)
            for (long long i = l0; i < l0 + k; ++i) {                    // the ordered-integer codes back to float32
                int c;
                std::memcpy(&c, vmin + i, 4);
                vmin[i] = dec(c);
                std::memcpy(&c, vmax + i, 4);
                vmax[i] = dec(c);
            }
    }
    release(h);
    return TOMO_SEG_OK;
}

TOMO_API int tomo_seg_remove_small(tomo_seg *h, void *stream, const int32_t *d_labels, int nx, int ny, int nz, int32_t n, int64_t min_size,
                                   int32_t *d_out, int32_t *n_kept) {
    CHK(check_call(h, "tomo_seg_remove_small", d_labels, 4, d_out, 4, nx, ny, nz));
    if (!n_kept) return fail(h, TOMO_SEG_ERR_ARG, "tomo_seg_remove_small: NULL pointer");
    if (n < 0 || min_size < 0) return fail(h, TOMO_SEG_ERR_ARG, "tomo_seg_remove_small: n and min_size must not be negative");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const Vol g = vol_of(nx, ny, nz, -1);
    CHK(grow(h, h->res, sizeof(int) * 2));
    CHK(count_sizes(h, st, d_labels, g, n));
    const unsigned ms = (unsigned)std::min<int64_t>(min_size, (int64_t)1 << 31);     // no component has 2^31 voxels
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(SCAN_TPB), 0, st, (int *)h->tab.p, (long long)n, 1, ms, (int *)h->res.p);
    HIPCHK(h, hipGetLastError());
    const bool vec = nz % 4 == 0 && aligned(d_labels, 16), vout = nz % 4 == 0 && aligned(d_out, 16);
    const dim3 grid(span_blocks(g, SPAN));
    const int *table = static_cast<const int *>(h->tab.p);
    if (vec && vout) hipLaunchKernelGGL((k_relabel<true, true>), grid, dim3(TPB), 0, st, d_labels, g, n, table, d_out);
    else if (vec) hipLaunchKernelGGL((k_relabel<true, false>), grid, dim3(TPB), 0, st, d_labels, g, n, table, d_out);
    else if (vout) hipLaunchKernelGGL((k_relabel<false, true>), grid, dim3(TPB), 0, st, d_labels, g, n, table, d_out);
    else hipLaunchKernelGGL((k_relabel<false, false>), grid, dim3(TPB), 0, st, d_labels, g, n, table, d_out);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(n_kept, h->res.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    release(h);
    return TOMO_SEG_OK;
}

TOMO_API int tomo_seg_largest(tomo_seg *h, void *stream, const int32_t *d_labels, int nx, int ny, int nz, int32_t n, uint8_t *d_mask,
                              int32_t *label, int64_t *count) {
    CHK(check_call(h, "tomo_seg_largest", d_labels, 4, d_mask, 1, nx, ny, nz));
    if (!label || !count) return fail(h, TOMO_SEG_ERR_ARG, "tomo_seg_largest: NULL pointer");
    if (n < 0) return fail(h, TOMO_SEG_ERR_ARG, "tomo_seg_largest: n < 0");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const Vol g = vol_of(nx, ny, nz, -1);
    CHK(grow(h, h->res, sizeof(int) * 2));
    CHK(count_sizes(h, st, d_labels, g, n));
    int *res = static_cast<int *>(h->res.p);
    hipLaunchKernelGGL(k_argmax, dim3(1), dim3(TPB), 0, st, (const unsigned *)h->tab.p, n, res);
    HIPCHK(h, hipGetLastError());
    const bool vec = nz % 4 == 0 && aligned(d_labels, 16), pack = nz % 4 == 0 && aligned(d_mask, 4);
    const dim3 grid(span_blocks(g, SPAN));
    if (vec && pack) hipLaunchKernelGGL((k_pick<true, true>), grid, dim3(TPB), 0, st, d_labels, g, (const int *)res, d_mask);
    else if (vec) hipLaunchKernelGGL((k_pick<true, false>), grid, dim3(TPB), 0, st, d_labels, g, (const int *)res, d_mask);
    else if (pack) hipLaunchKernelGGL((k_pick<false, true>), grid, dim3(TPB), 0, st, d_labels, g, (const int *)res, d_mask);
    else hipLaunchKernelGGL((k_pick<false, false>), grid, dim3(TPB), 0, st, d_labels, g, (const int *)res, d_mask);
    HIPCHK(h, hipGetLastError());
    int r[2] = {0, 0};
    HIPCHK(h, hipMemcpyAsync(r, res, sizeof(r), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    *label = r[0] < 0 ? 0 : r[0];
    *count = r[0] < 0 ? 0 : (int64_t)(unsigned)r[1];
    release(h);
    return TOMO_SEG_OK;
}

}  // extern "C"
