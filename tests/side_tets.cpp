// Runs csrc/tomo_side_tets.h on the host the way the kernels of libtomo_mesh.so do: every work-group, every lane, stage, count, scan,
// emit, over whole small volumes in heap buffers of exactly nx ny nz elements, an LDS stand-in of exactly TETS_LDS_FLOATS floats and a
// triangle buffer of exactly the counted size, so that an index past a brick, a volume or the output is the address sanitizer's to find.
// First all 256 corner patterns of a cell, which are all 16 cases of all six tetrahedra, against a brute-force orientation check at
// t = 0.5; then whole volumes, both borders, both element types, both access widths, against a per-cell brute force that shares
// nothing with the header but the definition.  Built (plain C++: __device__ is nothing) and run by tests/test_side_tets.py; exits 0
// if every check holds, else prints the ones that do not and exits 1.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../tomography_alignment_amd/csrc/tomo_side_tets.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            if (++failures <= 20) std::printf("line %d (%s): %s does not hold\n", __LINE__, what, #cond); \
        }                                                                            \
    } while (0)

unsigned rng_state = 2463534242u;
unsigned rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

using Tri = std::array<float, 9>;
const float NEG = -std::numeric_limits<float>::infinity();

bool same_bits(const Tri &a, const Tri &b) { return std::memcmp(a.data(), b.data(), sizeof(float) * 9) == 0; }
bool less_bits(const Tri &a, const Tri &b) { return std::memcmp(a.data(), b.data(), sizeof(float) * 9) < 0; }

// ---- the definition once more, from scratch: the permutations, the rule, the orientation by geometry at t = 0.5
const int PERMS[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

struct Corner { int d[3]; };

void tet_corners(int tet, Corner c[4]) {
    const int a = PERMS[tet][0], b = PERMS[tet][1];
    for (int i = 0; i < 4; ++i) c[i] = Corner{{0, 0, 0}};
    c[1].d[a] = 1;
    c[2].d[a] = 1, c[2].d[b] = 1;
    c[3] = Corner{{1, 1, 1}};
}

// value(dx, dy, dz): the voxel at that corner of the cell with the origin o.
template <class Value>
void brute_cell(const Value &value, float level, const int o[3], std::vector<Tri> &out) {
    for (int tet = 0; tet < 6; ++tet) {
        Corner c[4];
        tet_corners(tet, c);
        float v[4];
        bool in[4];
        int ins[4], outs[4], ni = 0, no = 0;
        for (int i = 0; i < 4; ++i) {
            v[i] = value(c[i].d[0], c[i].d[1], c[i].d[2]);
            in[i] = v[i] >= level;
            if (in[i]) ins[ni++] = i; else outs[no++] = i;
        }
        int edges[2][3][2], nt = 0;                        // triangles, vertices, the two corners of the edge
        auto set = [&](int t, int m, int p, int q) { edges[t][m][0] = p < q ? p : q, edges[t][m][1] = p < q ? q : p; };
        if (ni == 1) {
            nt = 1;
            for (int m = 0; m < 3; ++m) set(0, m, ins[0], outs[m]);
        } else if (ni == 3) {
            nt = 1;
            for (int m = 0; m < 3; ++m) set(0, m, ins[m], outs[0]);
        } else if (ni == 2) {
            nt = 2;
            const int a = ins[0], b = ins[1], cc = outs[0], d = outs[1];
            set(0, 0, a, cc), set(0, 1, a, d), set(0, 2, b, d);
            set(1, 0, a, cc), set(1, 1, b, d), set(1, 2, b, cc);
        }
        double away[3] = {0, 0, 0};
        for (int k = 0; k < 3; ++k) {
            for (int i = 0; i < no; ++i) away[k] += (double)c[outs[i]].d[k] / (no ? no : 1);
            for (int i = 0; i < ni; ++i) away[k] -= (double)c[ins[i]].d[k] / (ni ? ni : 1);
        }
        for (int t = 0; t < nt; ++t) {
            double mid[3][3];
            float pos[3][3];
            for (int m = 0; m < 3; ++m) {
                const Corner &lo = c[edges[t][m][0]], &hi = c[edges[t][m][1]];
                const float vlo = v[edges[t][m][0]], vhi = v[edges[t][m][1]];
                const float den = vhi - vlo;
                float tt = (level - vlo) / den;
                if (!std::isfinite(vlo) || !std::isfinite(vhi) || !std::isfinite(den)) tt = 0.5f;
                for (int k = 0; k < 3; ++k) {
                    mid[m][k] = 0.5 * (lo.d[k] + hi.d[k]);
                    const float base = (float)(o[k] + lo.d[k]);
                    pos[m][k] = hi.d[k] != lo.d[k] ? base + tt : base;
                }
            }
            const double u[3] = {mid[1][0] - mid[0][0], mid[1][1] - mid[0][1], mid[1][2] - mid[0][2]};
            const double w[3] = {mid[2][0] - mid[0][0], mid[2][1] - mid[0][1], mid[2][2] - mid[0][2]};
            const double s = (u[1] * w[2] - u[2] * w[1]) * away[0] + (u[2] * w[0] - u[0] * w[2]) * away[1] + (u[0] * w[1] - u[1] * w[0]) * away[2];
            const int second = s > 0 ? 1 : 2, third = s > 0 ? 2 : 1;
            Tri tri;
            for (int k = 0; k < 3; ++k) tri[k] = pos[0][k], tri[3 + k] = pos[second][k], tri[6 + k] = pos[third][k];
            out.push_back(tri);
        }
    }
}

// ---- all 256 patterns of one cell
void all_patterns() {
    const char *what = "patterns";
    std::unique_ptr<float[]> lds(new float[TETS_LDS_FLOATS]);
    const Bricks g = bricks_of(2, 2, 2, false);
    const int at = tets_lds_at(g, 0, 0, 0);
    int seen[6][16] = {};
    for (unsigned bits = 0; bits < 256; ++bits) {
        for (int i = 0; i < TETS_LDS_FLOATS; ++i) lds[i] = std::numeric_limits<float>::quiet_NaN();
        for (unsigned code = 0; code < 8; ++code) lds[at + tets_corner_at(code)] = ((bits >> code) & 1u) ? 1.0f : -1.0f;
        const float *s = lds.get() + at;
        CHECK(tets_bits(s, 0.0f) == bits);
        CHECK((tets_spread(tets_face(s, 0.0f)) | (tets_spread(tets_face(s + TETS_SX, 0.0f)) << 1)) == bits);
        for (int tet = 0; tet < 6; ++tet) seen[tet][tets_case_of(bits, tet)]++;
        std::vector<Tri> got, want;
        tets_cell(s, 0.0f, bits, 3, -1, 7, [&](const float *p0, const float *p1, const float *p2) {
            Tri t;
            for (int k = 0; k < 3; ++k) t[k] = p0[k], t[3 + k] = p1[k], t[6 + k] = p2[k];
            got.push_back(t);
        });
        const int o[3] = {3, -1, 7};
        brute_cell([&](int dx, int dy, int dz) { return ((bits >> (dx + 2 * dy + 4 * dz)) & 1u) ? 1.0f : -1.0f; }, 0.0f, o, want);
        CHECK((int)got.size() == tets_count(bits));
        CHECK((int)got.size() <= TETS_MAX_CELL);
        CHECK(got.size() == want.size());
        for (size_t i = 0; i < got.size() && i < want.size(); ++i) CHECK(same_bits(got[i], want[i]));
        // at t = 0.5 no triangle is degenerate
        for (const Tri &t : got) {
            const double u[3] = {(double)t[3] - t[0], (double)t[4] - t[1], (double)t[5] - t[2]};
            const double w[3] = {(double)t[6] - t[0], (double)t[7] - t[1], (double)t[8] - t[2]};
            const double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
            CHECK(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] > 0);
        }
    }
    for (int tet = 0; tet < 6; ++tet)
        for (int c = 0; c < 16; ++c) CHECK(seen[tet][c] == 16);
}

// ---- whole volumes
struct Shape { int nx, ny, nz; };

template <class T>
float as_float(T v) { return tets_value(v); }

template <class T, bool VEC>
void volume(const char *what, const Shape &s, const T *vol, float level, bool closed) {
    const Bricks g = bricks_of(s.nx, s.ny, s.nz, closed);
    auto value = [&](int x, int y, int z) {
        return (x < 0 || y < 0 || z < 0 || x >= s.nx || y >= s.ny || z >= s.nz) ? NEG : as_float(vol[((long long)x * s.ny + y) * s.nz + z]);
    };
    // the brute force, cell by cell
    std::vector<Tri> want;
    long long mixed = 0;
    for (int cx = 0; cx < g.cx; ++cx)
        for (int cy = 0; cy < g.cy; ++cy)
            for (int cz = 0; cz < g.cz; ++cz) {
                const int o[3] = {cx + g.shift, cy + g.shift, cz + g.shift};
                const size_t before = want.size();
                brute_cell([&](int dx, int dy, int dz) { return value(o[0] + dx, o[1] + dy, o[2] + dz); }, level, o, want);
                mixed += want.size() > before ? 1 : 0;
            }
    CHECK((closed ? (g.cx == s.nx + 1 && g.shift == -1) : (g.cx == s.nx - 1 && g.shift == 0)));
    if (g.blocks == 0) {
        CHECK(want.empty());
        return;
    }
    // the kernels: count, scan, emit
    std::unique_ptr<float[]> lds(new float[TETS_LDS_FLOATS]);
    std::vector<long long> offs((size_t)g.blocks + 1, 0);
    long long visited = 0;
    for (long long b = 0; b < g.blocks; ++b) {
        for (int i = 0; i < TETS_LDS_FLOATS; ++i) lds[i] = std::numeric_limits<float>::quiet_NaN();
        for (int tid = 0; tid < TETS_LANES; ++tid) tets_stage<T, VEC>(vol, g, b, tid, TETS_LANES, lds.get());
        const Brick br = brick_of(g, b);
        long long n = 0;
        for (int tid = 0; tid < TETS_LANES; ++tid)
            tets_walk(lds.get(), g, br, tid, level, [&](const float *p, unsigned bits, int ox, int oy, int oz) {
                CHECK(bits == tets_bits(p, level));
                CHECK(ox >= g.shift && ox < g.cx + g.shift && oy >= g.shift && oy < g.cy + g.shift && oz >= g.shift && oz < g.cz + g.shift);
                n += tets_count(bits);
                ++visited;
            });
        offs[(size_t)b + 1] = offs[(size_t)b] + n;
    }
    const long long total = offs[(size_t)g.blocks];
    CHECK(visited == mixed);
    CHECK(total == (long long)want.size());
    std::unique_ptr<float[]> tri(new float[(size_t)total * 9]);
    double area = 0.0, vol6 = 0.0;
    for (long long b = 0; b < g.blocks; ++b) {
        if (offs[(size_t)b + 1] == offs[(size_t)b]) continue;
        for (int tid = 0; tid < TETS_LANES; ++tid) tets_stage<T, VEC>(vol, g, b, tid, TETS_LANES, lds.get());
        const Brick br = brick_of(g, b);
        long long at = offs[(size_t)b];
        for (int tid = 0; tid < TETS_LANES; ++tid)
            tets_walk(lds.get(), g, br, tid, level, [&](const float *p, unsigned bits, int ox, int oy, int oz) {
                tets_cell(p, level, bits, ox, oy, oz, [&](const float *p0, const float *p1, const float *p2) {
                    float *q = tri.get() + 9 * at++;
                    for (int k = 0; k < 3; ++k) q[k] = p0[k], q[3 + k] = p1[k], q[6 + k] = p2[k];
                    tets_measure(p0, p1, p2, area, vol6);
                });
            });
        CHECK(at == offs[(size_t)b + 1]);
    }
    std::vector<Tri> got((size_t)total);
    for (long long i = 0; i < total; ++i) std::memcpy(got[(size_t)i].data(), tri.get() + 9 * i, sizeof(float) * 9);
    std::sort(got.begin(), got.end(), less_bits);
    std::sort(want.begin(), want.end(), less_bits);
    bool equal = got.size() == want.size();
    for (size_t i = 0; equal && i < got.size(); ++i) equal = same_bits(got[i], want[i]);
    CHECK(equal);
    // the measures against the plain formulas on the brute force's triangles
    double a2 = 0.0, v2 = 0.0;
    for (const Tri &t : want) {
        const double p0[3] = {t[0], t[1], t[2]}, p1[3] = {t[3], t[4], t[5]}, p2[3] = {t[6], t[7], t[8]};
        const double e[3] = {(p1[1] - p0[1]) * (p2[2] - p0[2]) - (p1[2] - p0[2]) * (p2[1] - p0[1]),
                             (p1[2] - p0[2]) * (p2[0] - p0[0]) - (p1[0] - p0[0]) * (p2[2] - p0[2]),
                             (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p1[1] - p0[1]) * (p2[0] - p0[0])};
        a2 += 0.5 * std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        v2 += p0[0] * (p1[1] * p2[2] - p1[2] * p2[1]) + p0[1] * (p1[2] * p2[0] - p1[0] * p2[2]) + p0[2] * (p1[0] * p2[1] - p1[1] * p2[0]);
    }
    CHECK(std::fabs(area - a2) <= 1e-10 * (1.0 + a2));
    CHECK(std::fabs(vol6 - v2) <= 1e-8 * (1.0 + std::fabs(v2) + a2));
    if (closed && std::is_same<T, uint8_t>::value && total > 0) CHECK(vol6 > 0.0);
}

template <class T>
void volumes(const char *what, const Shape &s, const T *vol, float level) {
    for (int closed = 0; closed < 2; ++closed) {
        volume<T, false>(what, s, vol, level, closed != 0);
        if (s.nz % 4 == 0 && (reinterpret_cast<uintptr_t>(vol) & (sizeof(T) == 1 ? 3 : 15)) == 0) volume<T, true>(what, s, vol, level, closed != 0);
    }
}

void whole_volumes() {
    const Shape shapes[] = {{1, 1, 1}, {1, 3, 4}, {3, 1, 4}, {3, 4, 1}, {2, 2, 2}, {7, 7, 31}, {8, 8, 32}, {9, 9, 33}, {10, 3, 36},
                            {3, 17, 5}, {17, 2, 3}, {2, 3, 67}, {5, 6, 8}};
    for (const Shape &s : shapes) {
        const size_t n = (size_t)s.nx * s.ny * s.nz;
        char what[64];
        std::snprintf(what, sizeof what, "%d x %d x %d", s.nx, s.ny, s.nz);
        {   // float noise, some voxels at the level, some not finite
            std::unique_ptr<float[]> f(new float[n]);
            for (size_t i = 0; i < n; ++i) {
                const unsigned k = rnd() % 16;
                f[i] = (float)(rnd() % 2001) / 1000.0f - 1.0f;
                if (k == 0) f[i] = 0.25f;
                if (k == 1) f[i] = std::numeric_limits<float>::quiet_NaN();
                if (k == 2) f[i] = std::numeric_limits<float>::infinity();
                if (k == 3) f[i] = NEG;
            }
            volumes<float>(what, s, f.get(), 0.25f);
        }
        {   // integer-valued floats at a level that is one of the values
            std::unique_ptr<float[]> f(new float[n]);
            for (size_t i = 0; i < n; ++i) f[i] = (float)(rnd() % 4);
            volumes<float>(what, s, f.get(), 2.0f);
        }
        for (unsigned p : {1u, 5u, 9u, 10u}) {   // masks: Bernoulli p / 10, all one
            std::unique_ptr<uint8_t[]> m(new uint8_t[n]);
            for (size_t i = 0; i < n; ++i) m[i] = rnd() % 10 < p ? (uint8_t)(1 + rnd() % 255) : 0;
            volumes<uint8_t>(what, s, m.get(), 0.5f);
        }
        {   // the checkerboard: the most triangles a cell can have
            std::unique_ptr<uint8_t[]> m(new uint8_t[n]);
            for (int x = 0; x < s.nx; ++x)
                for (int y = 0; y < s.ny; ++y)
                    for (int z = 0; z < s.nz; ++z) m[((size_t)x * s.ny + y) * s.nz + z] = (x + y + z) & 1;
            volumes<uint8_t>(what, s, m.get(), 0.5f);
        }
    }
}

}  // namespace

int main() {
    all_patterns();
    whole_volumes();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("side_tets: all checks hold\n");
    return 0;
}
