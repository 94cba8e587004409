// A device volume v[nx][ny][nz] (z fastest) as groups of four z: the decomposition the elementwise kernels of libtomo_vol.so and
// libtomo_seg.so share.  Internal, as tomo_side_host.h is; the host picks VEC / PACK with that header's aligned().
//
// A row (x, y) is cut into G = ceil(nz / 4) groups of four consecutive z; the volume is nx ny G groups in memory order and a lane owns
// one group at a time: one wide access (VEC / PACK: nz % 4 == 0 and the pointer aligned to four elements, so every group's address is)
// or four guarded single accesses of the same elements.  A work-group of 256 lanes owns `span` consecutive groups and walks them 256 at a
// time, so short rows waste no lanes: work-group b starts at group g0 = b span, and its lane's step `off` (threadIdx.x, + 256, ... below
// span) is group g0 + off, which exists while off < Walk::left.  One 64-bit division per work-group places its first group (walk_of); a
// lane's (row, group of the row) follow by a 32-bit one (step_of).  A row outside the region (inside) is not read.
//
// Nothing here uses a device intrinsic, so a plain C++ compile, to which __device__ is nothing, sees every function:
// tests/side_zgroups.cpp walks whole grids on the host under the address sanitizer.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace {

struct Vol {
    int nx, ny, nz;
    unsigned G;              // groups of four z of a row
    long long R4;            // < 0: no region
    long long groups;        // nx ny G
};

inline Vol vol_of(int nx, int ny, int nz, long long R4) {
    Vol g;
    g.nx = nx, g.ny = ny, g.nz = nz;
    g.G = (unsigned)(((long long)nz + 3) / 4);
    g.R4 = R4 < 0 ? -1 : R4;
    g.groups = (long long)nx * ny * g.G;
    return g;
}

// The work-groups of `span` groups each that cover the volume.
inline unsigned span_blocks(const Vol &g, int span) { return (unsigned)((g.groups + span - 1) / span); }

__device__ inline bool finite32(float v) { return fabsf(v) <= FLT_MAX; }          // false for NaN and +-inf

// Row x ny + y is in the region: (2x - nx + 1)^2 + (2y - ny + 1)^2 <= R4.
__device__ inline bool inside(const Vol &g, unsigned row) {
    if (g.R4 < 0) return true;
    const unsigned x = row / (unsigned)g.ny, y = row - x * (unsigned)g.ny;
    const long long a = 2LL * x - g.nx + 1, b = 2LL * y - g.ny + 1;
    return a * a + b * b <= g.R4;
}

// The walk of a work-group over `span` groups from group g0: lane's step s is group g0 + s * TPB + tid.
struct Walk {
    long long row0;          // the row of the work-group's first group
    unsigned zb;             // that group's index in its row
    long long left;          // groups from g0 to the end of the volume
};

__device__ inline Walk walk_of(const Vol &g, long long g0) {
    Walk w;
    w.row0 = g0 / g.G;
    w.zb = (unsigned)(g0 - w.row0 * g.G);
    w.left = g.groups - g0;
    return w;
}

// Where step `off` < w.left of the walk is: its row and its group of that row.
struct Step {
    long long row;
    unsigned zq;
};

__device__ inline Step step_of(const Vol &g, const Walk &w, unsigned off) {
    const unsigned local = w.zb + off, dr = local / g.G, zq = local - dr * g.G;
    return Step{w.row0 + dr, zq};
}

// The four z of group zq of a row that starts at `row`: f[k] and whether z + k < nz.
template <bool VEC>
__device__ inline void load4(const float *__restrict__ row, int nz, unsigned zq, float f[4], bool in[4]) {
    const int z = 4 * (int)zq;
    if (VEC) {                                                           // nz % 4 == 0: the whole group is inside the row
        const float4 t = *reinterpret_cast<const float4 *>(row + z);
        f[0] = t.x, f[1] = t.y, f[2] = t.z, f[3] = t.w;
        in[0] = in[1] = in[2] = in[3] = true;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            in[k] = z + k < nz;
            f[k] = in[k] ? row[z + k] : 0.f;
        }
    }
}

template <bool VEC>
__device__ inline void load4i(const int *row, int nz, unsigned zq, int v[4], bool in[4]) {
    const int z = 4 * (int)zq;
    if (VEC) {
        const int4 t = *reinterpret_cast<const int4 *>(row + z);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
        in[0] = in[1] = in[2] = in[3] = true;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            in[k] = z + k < nz;
            v[k] = in[k] ? row[z + k] : 0;
        }
    }
}

template <bool VEC>
__device__ inline void store4i(int *row, int nz, unsigned zq, const int v[4]) {
    const int z = 4 * (int)zq;
    if (VEC) {
        *reinterpret_cast<int4 *>(row + z) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (z + k < nz) row[z + k] = v[k];
    }
}

// Four bytes, c[k] < 256.  PACK: nz % 4 == 0 and the row 4-byte aligned.
template <bool PACK>
__device__ inline void store4b(uint8_t *row, int nz, unsigned zq, const unsigned c[4]) {
    const int z = 4 * (int)zq;
    if (PACK) {
        *reinterpret_cast<unsigned *>(row + z) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (z + k < nz) row[z + k] = (uint8_t)c[k];
    }
}

}  // namespace
