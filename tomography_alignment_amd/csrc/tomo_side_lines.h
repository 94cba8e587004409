// The exact line pass of the squared Euclidean distance transform, g[i] = min over j of f[j] + (i - j)^2 along every line of one axis of a
// device volume [nx][ny][nz] (z fastest), and the tiles that stage those lines: what the passes of libtomo_morph.so are made of.
// Internal, as tomo_side_host.h is.
//
// The line routine (line_min): the lane that owns output i walks outward, k = 0, 1, 2, ..., takes min(best, f[i - k] + k^2,
// f[i + k] + k^2) and stops once k^2 >= best or both sides have left the line -- exact in integers, no division, no per-lane stack; the
// cost follows the true distance.  f is 0 ... LINES_INF = 2^31 - 1 ("nothing"); f + k^2 is added in uint32 (k < 16384, so it fits) and
// clamped to LINES_INF.  `border`: positions -1 and n of the line hold f = 0.  V adjacent lines go together (one 16-byte LDS read a step);
// the walk ends when the largest of the V bests allows it, which changes no result: a further step only offers values >= best.
//
// Axis x and y (Cross): the volume is outer x n x cols (x: 1, nx, ny nz; y: nx, ny, nz); element (o, i, c) lies at (o n + i) cols + c.
// The columns are cut into Q = ceil(cols / 4) groups of four; a work-group owns all n positions of wq adjacent groups of one outer index
// and stages them in LDS as [i][4 wq], so that lane (i, group) and its neighbours read consecutive words at every step of the walk: no
// bank conflict and no padding.  Global accesses are 16-byte ones along the columns (VEC: cols % 4 == 0 and the pointer aligned), or
// guarded single ones of the same elements.  Because a work-group has all of its lines in LDS before it stores, a pass may run in place.
// Axis z (Rows): a work-group owns R whole rows, a flat stretch of R nz elements staged as it lies; a lane owns one element.  It is the
// first pass and reads the mask: f = LINES_INF on the foreground, 0 elsewhere (invert: the other way round).
// A line longer than the limit takes the second path (cross_global, rows_global): a lane per group (element), f read from global memory,
// the result into another buffer.
//
// Nothing here uses a device intrinsic, so a plain C++ compile, to which __device__ is nothing, sees every function:
// tests/side_lines.cpp runs whole grids, lane by lane, on the host under the address and undefined-behaviour sanitizers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int LINES_INF = 2147483647;
constexpr int LINES_V = 4;               // adjacent columns a lane of the x and y passes owns
constexpr int LINES_MAX_WQ = 16;         // groups of four columns a work-group owns at most: 256 bytes of a row

__device__ inline int lines_add(int f, int k2) {                         // f + k2 clamped to LINES_INF; f >= 0, 0 <= k2 <= 2^28
    const unsigned s = (unsigned)f + (unsigned)k2;
    return s > (unsigned)LINES_INF ? LINES_INF : (int)s;
}

__device__ inline int lines_f(unsigned m, int invert) { return ((m != 0) != (invert != 0)) ? LINES_INF : 0; }

// best[v] = min over j in 0 ... n - 1 (with border also -1 and n, where f = 0) of f[j][v] + (i - j)^2.  get(j, c): c[0 ... V - 1] = f[j].
template <int V, class Get>
__device__ inline void line_min(const Get &get, int n, int i, bool border, int best[V]) {
    int c[V];
    get(i, best);
    if (border) {
        const int e = i + 1 < n - i ? i + 1 : n - i, e2 = e * e;          // e <= 8192
#pragma unroll
        for (int v = 0; v < V; ++v) best[v] = best[v] < e2 ? best[v] : e2;
    }
    for (int k = 1; k < n; ++k) {
        const int k2 = k * k;
        int top = best[0];
#pragma unroll
        for (int v = 1; v < V; ++v) top = top > best[v] ? top : best[v];
        const bool lo = i - k >= 0, hi = i + k < n;
        if (k2 >= top || !(lo || hi)) break;
        if (lo) {
            get(i - k, c);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int s = lines_add(c[v], k2);
                best[v] = best[v] < s ? best[v] : s;
            }
        }
        if (hi) {
            get(i + k, c);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int s = lines_add(c[v], k2);
                best[v] = best[v] < s ? best[v] : s;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ axis x and y
struct Cross {
    int n;                   // the length of a line
    long long cols;          // lines side by side in memory
    long long outer;         // blocks of n cols elements
    long long Q;             // groups of four columns
    int wq;                  // groups a work-group owns
    long long tiles;         // work-groups per outer index
    long long blocks;        // outer tiles
    long long items;         // outer n Q: the lanes of the second path
};

// axis 0: x, 1: y.  tile_ints: the int32 a work-group may stage (>= 4 n on the LDS path).
inline Cross cross_of(int nx, int ny, int nz, int axis, long long tile_ints) {
    Cross g;
    g.n = axis == 0 ? nx : ny;
    g.cols = axis == 0 ? (long long)ny * nz : nz;
    g.outer = axis == 0 ? 1 : nx;
    g.Q = (g.cols + LINES_V - 1) / LINES_V;
    long long wq = tile_ints / ((long long)LINES_V * g.n);
    wq = wq < 1 ? 1 : wq > LINES_MAX_WQ ? LINES_MAX_WQ : wq;
    g.wq = (int)(wq < g.Q ? wq : g.Q);
    g.tiles = (g.Q + g.wq - 1) / g.wq;
    g.blocks = g.outer * g.tiles;
    g.items = g.outer * g.n * g.Q;
    return g;
}

inline long long cross_lds_ints(const Cross &g) { return (long long)g.n * g.wq * LINES_V; }

// The four columns of group q of position i of outer index o; absent columns (past cols) read LINES_INF.
template <bool VEC>
__device__ inline void cross_load(const int *__restrict__ src, const Cross &g, long long o, int i, long long q, int c[LINES_V]) {
    const long long col = LINES_V * q, at = (o * g.n + i) * g.cols + col;
    if (VEC) {
        const int4 t = *reinterpret_cast<const int4 *>(src + at);
        c[0] = t.x, c[1] = t.y, c[2] = t.z, c[3] = t.w;
    } else {
#pragma unroll
        for (int v = 0; v < LINES_V; ++v) c[v] = col + v < g.cols ? src[at + v] : LINES_INF;
    }
}

// Work-group `block`, lane tid of T: its share of the tile into lds[n][4 wq].
template <bool VEC>
__device__ inline void cross_stage(const int *__restrict__ src, const Cross &g, long long block, int tid, int T, int *lds) {
    const long long o = block / g.tiles, q0 = (block - o * g.tiles) * g.wq;
    const int total = g.n * g.wq;
    for (int idx = tid; idx < total; idx += T) {
        const int i = idx / g.wq, ql = idx - i * g.wq;
        int c[LINES_V] = {LINES_INF, LINES_INF, LINES_INF, LINES_INF};
        if (q0 + ql < g.Q) cross_load<VEC>(src, g, o, i, q0 + ql, c);
#pragma unroll
        for (int v = 0; v < LINES_V; ++v) lds[LINES_V * idx + v] = c[v];
    }
}

// After every lane has staged: the lane's outputs.  lds is aligned to 16 bytes.  put(at, col, best): the four results of the columns
// col ... col + 3 (those below g.cols exist) of the element at linear index `at`.
template <class Put>
__device__ inline void cross_compute(const int *lds, const Cross &g, long long block, int tid, int T, bool border, const Put &put) {
    const long long o = block / g.tiles, q0 = (block - o * g.tiles) * g.wq;
    const int total = g.n * g.wq, pitch = LINES_V * g.wq;
    for (int idx = tid; idx < total; idx += T) {
        const int i = idx / g.wq, ql = idx - i * g.wq;
        if (q0 + ql >= g.Q) continue;
        const int *line = lds + LINES_V * ql;
        int best[LINES_V];
        line_min<LINES_V>([&](int j, int c[LINES_V]) {                    // lds, pitch and 4 ql are multiples of 16 bytes: one 16-byte read
            const int4 t = *reinterpret_cast<const int4 *>(line + j * pitch);
            c[0] = t.x, c[1] = t.y, c[2] = t.z, c[3] = t.w;
        }, g.n, i, border, best);
        const long long col = LINES_V * (q0 + ql);
        put((o * g.n + i) * g.cols + col, col, best);
    }
}

// The second path: item < g.items is one group of one position, f read from src (never the buffer put writes).
template <bool VEC, class Put>
__device__ inline void cross_global(const int *__restrict__ src, const Cross &g, long long item, bool border, const Put &put) {
    const long long q = item % g.Q, oi = item / g.Q, o = oi / g.n;
    const int i = (int)(oi - o * g.n);
    int best[LINES_V];
    line_min<LINES_V>([&](int j, int c[LINES_V]) { cross_load<VEC>(src, g, o, j, q, c); }, g.n, i, border, best);
    put(oi * g.cols + LINES_V * q, LINES_V * q, best);
}

// --------------------------------------------------------------------------------------------------------------------------- axis z
struct Rows {
    int nz;
    long long rows;          // nx ny
    int R;                   // rows a work-group owns
    long long blocks;
    long long items;         // rows nz: the lanes of the second path
};

inline Rows rows_of(int nx, int ny, int nz, long long tile_ints) {
    Rows g;
    g.nz = nz;
    g.rows = (long long)nx * ny;
    long long R = tile_ints / nz;
    R = R < 1 ? 1 : R;
    g.R = (int)(R < g.rows ? R : g.rows);
    g.blocks = (g.rows + g.R - 1) / g.R;
    g.items = g.rows * nz;
    return g;
}

inline long long rows_lds_ints(const Rows &g) { return (long long)g.R * g.nz; }

__device__ inline int rows_count(const Rows &g, long long block) {        // the elements of the work-group's stretch
    const long long row0 = block * g.R, left = g.rows - row0;
    return (int)((left < g.R ? left : g.R) * g.nz);
}

// PACK: nz % 4 == 0 and the mask 4-byte aligned, so every stretch starts and ends on a word of four mask bytes.
template <bool PACK>
__device__ inline void rows_stage(const uint8_t *__restrict__ mask, const Rows &g, long long block, int tid, int T, int invert, int *lds) {
    const long long at = block * g.R * g.nz;
    const int count = rows_count(g, block);
    if (PACK) {
        const unsigned *words = reinterpret_cast<const unsigned *>(mask + at);
        for (int w = tid; w < count / 4; w += T) {
            const unsigned m = words[w];
#pragma unroll
            for (int v = 0; v < 4; ++v) lds[4 * w + v] = lines_f((m >> (8 * v)) & 0xffu, invert);
        }
    } else {
        for (int e = tid; e < count; e += T) lds[e] = lines_f(mask[at + e], invert);
    }
}

// put(at, best): the result of the element at linear index `at`.
template <class Put>
__device__ inline void rows_compute(const int *lds, const Rows &g, long long block, int tid, int T, bool border, const Put &put) {
    const long long at = block * g.R * g.nz;
    const int count = rows_count(g, block);
    for (int e = tid; e < count; e += T) {
        const int i = e % g.nz;
        const int *line = lds + (e - i);
        int best[1];
        line_min<1>([&](int j, int c[1]) { c[0] = line[j]; }, g.nz, i, border, best);
        put(at + e, best[0]);
    }
}

template <class Put>
__device__ inline void rows_global(const uint8_t *__restrict__ mask, const Rows &g, long long item, int invert, bool border, const Put &put) {
    const int i = (int)(item % g.nz);
    const uint8_t *line = mask + (item - i);
    int best[1];
    line_min<1>([&](int j, int c[1]) { c[0] = lines_f(line[j], invert); }, g.nz, i, border, best);
    put(item, best[0]);
}

}  // namespace
