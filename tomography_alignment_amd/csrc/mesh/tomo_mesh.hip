// libtomo_mesh.so (include/tomo_mesh.h): the isosurface of a device volume by marching tetrahedra -- its triangles, their number, the
// area and the enclosed volume.  gfx950 only.  The definition is in the header; the bricks, the staging, the cases and the vertex rule
// are csrc/tomo_side_tets.h.
//
// k_count    a work-group per brick: stages it, every lane walks its cells; the brick's number of triangles and, for measure, its two
//            float64 sums (block_sum: a fixed tree).
// k_scan     one work-group: the bricks' counts into exclusive int64 offsets, the total behind them.
// k_total    one work-group: the counts and the partial sums added up, a lane a fixed stride of bricks, then the tree.
// k_emit     a work-group per brick, gone at once without a triangle: stages again, counts per lane, a fixed-order scan of the lanes
//            (wave prefix by shuffles, waves through LDS), then every lane writes its triangles from offset + rank on.
// Only vector stores and plain C++; no atomics; no work-group waits for another.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/tomo_mesh.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_MESH_ERR_ARG, SIDE_ERR_HIP = TOMO_MESH_ERR_HIP, SIDE_ERR_NODEV = TOMO_MESH_ERR_NODEV;
}
#include "../tomo_side_host.h"
#include "../tomo_side_reduce.h"
#include "../tomo_side_tets.h"

namespace {

constexpr int TPB = TOMO_MESH_GROUP;
constexpr int ONE = 1024;                      // the lanes of the two kernels that are one work-group
constexpr int SCAN_ITEMS = 4;
static_assert(TETS_BX == TOMO_MESH_BRICK_X && TETS_BY == TOMO_MESH_BRICK_Y && TETS_BZ == TOMO_MESH_BRICK_Z && TETS_LANES == TPB,
              "the header and the brick routines agree");

struct Res {
    long long n;
    double area, vol6;
};

template <class T, bool VEC, bool MEASURE>
__global__ __launch_bounds__(TPB) void k_count(const T *__restrict__ vol, Bricks g, float level, int *__restrict__ counts,
                                               double *__restrict__ part) {
    __shared__ __align__(16) float lds[TETS_LDS_FLOATS];
    __shared__ double sh[MEASURE ? TPB : 1];
    __shared__ int ws[TPB / 64];
    tets_stage<T, VEC>(vol, g, blockIdx.x, threadIdx.x, TPB, lds);
    __syncthreads();
    const Brick b = brick_of(g, blockIdx.x);
    int n = 0;
    double area = 0.0, vol6 = 0.0;
    tets_walk(lds, g, b, threadIdx.x, level, [&](const float *s, unsigned bits, int ox, int oy, int oz) {
        n += tets_count(bits);
        if (MEASURE)
            tets_cell(s, level, bits, ox, oy, oz, [&](const float *p0, const float *p1, const float *p2) { tets_measure(p0, p1, p2, area, vol6); });
    });
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) n += __shfl_down(n, o, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int j = 0; j < TPB / 64; ++j) t += ws[j];
    if (threadIdx.x == 0) counts[blockIdx.x] = t;
    if (MEASURE) {
        double a = 0.0, v = 0.0;
        if (t != 0) {                                    // the whole work-group: most bricks of a real volume hold no surface
            a = block_sum<TPB>(area, sh);
            v = block_sum<TPB>(vol6, sh);
        }
        if (threadIdx.x == 0) part[2 * (long long)blockIdx.x] = a, part[2 * (long long)blockIdx.x + 1] = v;
    }
}

// offs[0 ... n) = the exclusive prefix sum of counts, offs[n] and res->n the total.
__global__ __launch_bounds__(ONE) void k_scan(const int *__restrict__ counts, long long n, long long *__restrict__ offs, Res *res) {
    __shared__ long long ws[ONE / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (long long base = 0; base < n; base += ONE * SCAN_ITEMS) {
        const long long i0 = base + (long long)threadIdx.x * SCAN_ITEMS;
        int v[SCAN_ITEMS];
        long long s = 0;
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            v[j] = i0 + j < n ? counts[i0 + j] : 0;
            s += v[j];
        }
        long long inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) ws[wave] = inc;
        __syncthreads();
        long long before = 0, tot = 0;
#pragma unroll
        for (int j = 0; j < ONE / 64; ++j) {
            before += j < wave ? ws[j] : 0;
            tot += ws[j];
        }
        long long ex = carry + before + inc - s;
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            if (i0 + j < n) offs[i0 + j] = ex;
            ex += v[j];
        }
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        offs[n] = carry;
        res->n = carry;
    }
}

// The sums over the bricks.  A count is below 2^15 and there are fewer than 2^31 bricks, so the counts add up exactly as doubles.
__global__ __launch_bounds__(ONE) void k_total(const int *__restrict__ counts, const double *__restrict__ part, long long n, Res *res) {
    __shared__ double sh[ONE];
    double c = 0.0, a = 0.0, v = 0.0;
    for (long long i = threadIdx.x; i < n; i += ONE) {
        c += (double)counts[i];
        a += part[2 * i];
        v += part[2 * i + 1];
    }
    c = block_sum<ONE>(c, sh);
    a = block_sum<ONE>(a, sh);
    v = block_sum<ONE>(v, sh);
    if (threadIdx.x == 0) res->n = (long long)c, res->area = a, res->vol6 = v;
}

template <class T, bool VEC>
__global__ __launch_bounds__(TPB) void k_emit(const T *__restrict__ vol, Bricks g, float level, const int *__restrict__ counts,
                                              const long long *__restrict__ offs, float *__restrict__ tri, long long capacity) {
    __shared__ __align__(16) float lds[TETS_LDS_FLOATS];
    __shared__ int ws[TPB / 64];
    if (counts[blockIdx.x] == 0) return;                 // the whole work-group
    tets_stage<T, VEC>(vol, g, blockIdx.x, threadIdx.x, TPB, lds);
    __syncthreads();
    const Brick b = brick_of(g, blockIdx.x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int n = 0;
    tets_walk(lds, g, b, threadIdx.x, level, [&](const float *, unsigned bits, int, int, int) { n += tets_count(bits); });
    int inc = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int j = 0; j < TPB / 64; ++j) before += j < wave ? ws[j] : 0;
    if (n == 0) return;
    long long at = offs[blockIdx.x] + before + inc - n;
    tets_walk(lds, g, b, threadIdx.x, level, [&](const float *s, unsigned bits, int ox, int oy, int oz) {
        tets_cell(s, level, bits, ox, oy, oz, [&](const float *p0, const float *p1, const float *p2) {
            if (at < capacity) {                         // the host has checked the total; no lane ever writes past the buffer
                float *q = tri + 9 * at;
                q[0] = p0[0], q[1] = p0[1], q[2] = p0[2];
                q[3] = p1[0], q[4] = p1[1], q[5] = p1[2];
                q[6] = p2[0], q[7] = p2[1], q[8] = p2[2];
            }
            ++at;
        });
    });
}

}  // namespace

struct tomo_mesh {
    int device = 0;
    std::string err;
    Buf counts;              // int32 a brick
    Buf offs;                // int64 a brick and one: where its triangles begin
    Buf part;                // two doubles a brick: measure
    Buf res;                 // one Res
    auto bufs() { return std::array{&counts, &offs, &part, &res}; }
};

namespace {

std::string dims(long long nx, long long ny, long long nz) { return std::to_string(nx) + " x " + std::to_string(ny) + " x " + std::to_string(nz); }

int check_shape(tomo_mesh *h, long long nx, long long ny, long long nz) {
    const long long top = TOMO_MESH_MAX_DIM;
    if (nx < 1 || ny < 1 || nz < 1 || nx > top || ny > top || nz > top)
        return fail(h, TOMO_MESH_ERR_UNSUPPORTED, "tomo_mesh: a volume of " + dims(nx, ny, nz) + " is outside 1 <= nx, ny, nz <= " +
                                                      std::to_string(top) + "; nothing was launched");
    if (nx * ny * nz > (long long)TOMO_MESH_MAX_VOXELS)                  // at most 2^42: no overflow
        return fail(h, TOMO_MESH_ERR_UNSUPPORTED, "tomo_mesh: a volume of " + dims(nx, ny, nz) + " has more than 2^31 - 1 voxels; nothing was launched");
    return TOMO_MESH_OK;
}

int check_call(tomo_mesh *h, const char *what, const void *d_vol, int dtype, int nx, int ny, int nz, float level, int border) {
    const std::string w(what);
    if (!h) return fail(h, TOMO_MESH_ERR_ARG, w + ": NULL handle");
    if (!d_vol) return fail(h, TOMO_MESH_ERR_ARG, w + ": NULL pointer");
    if (dtype != TOMO_MESH_F32 && dtype != TOMO_MESH_U8) return fail(h, TOMO_MESH_ERR_ARG, w + ": dtype must be 0 (float32) or 1 (uint8); nothing was launched");
    if (border != TOMO_MESH_OPEN && border != TOMO_MESH_CLOSED) return fail(h, TOMO_MESH_ERR_ARG, w + ": border must be 0 (open) or 1 (closed); nothing was launched");
    if (dtype == TOMO_MESH_F32 && !std::isfinite(level)) return fail(h, TOMO_MESH_ERR_ARG, w + ": level must be finite; nothing was launched");
    if (dtype == TOMO_MESH_F32 && !aligned(d_vol, 4)) return fail(h, TOMO_MESH_ERR_ARG, w + ": misaligned pointer");
    return check_shape(h, nx, ny, nz);
}

// The handle keeps at most TOMO_MESH_KEEP_BYTES between calls: with more, all of it goes back; the stream has run dry by then.
int release(tomo_mesh *h) {
    if (buf_bytes(h->bufs()) <= (size_t)TOMO_MESH_KEEP_BYTES) return TOMO_MESH_OK;
    for (Buf *b : h->bufs())
        if (b->p) {
            HIPCHK(h, hipFree(b->p));
            b->p = nullptr, b->n = 0;
        }
    return TOMO_MESH_OK;
}

struct Call {
    const void *vol;
    int dtype;
    Bricks g;
    float level;
    bool vec;
};

Call call_of(const void *d_vol, int dtype, int nx, int ny, int nz, float level, int border) {
    Call c;
    c.vol = d_vol, c.dtype = dtype;
    c.g = bricks_of(nx, ny, nz, border == TOMO_MESH_CLOSED);
    c.level = dtype == TOMO_MESH_U8 ? 0.5f : level;
    c.vec = nz % 4 == 0 && aligned(d_vol, dtype == TOMO_MESH_U8 ? 4 : 16);
    return c;
}

template <class T, bool MEASURE>
void launch_count(hipStream_t st, const Call &c, int *counts, double *part) {
    const T *vol = static_cast<const T *>(c.vol);
    if (c.vec) hipLaunchKernelGGL((k_count<T, true, MEASURE>), dim3((unsigned)c.g.blocks), dim3(TPB), 0, st, vol, c.g, c.level, counts, part);
    else hipLaunchKernelGGL((k_count<T, false, MEASURE>), dim3((unsigned)c.g.blocks), dim3(TPB), 0, st, vol, c.g, c.level, counts, part);
}

template <class T>
void launch_emit(hipStream_t st, const Call &c, const int *counts, const long long *offs, float *tri, long long capacity) {
    const T *vol = static_cast<const T *>(c.vol);
    if (c.vec) hipLaunchKernelGGL((k_emit<T, true>), dim3((unsigned)c.g.blocks), dim3(TPB), 0, st, vol, c.g, c.level, counts, offs, tri, capacity);
    else hipLaunchKernelGGL((k_emit<T, false>), dim3((unsigned)c.g.blocks), dim3(TPB), 0, st, vol, c.g, c.level, counts, offs, tri, capacity);
}

int too_many(tomo_mesh *h, long long n) {
    return fail(h, TOMO_MESH_ERR_UNSUPPORTED, "tomo_mesh: the surface has " + std::to_string(n) + " triangles, more than 2^31 - 1; nothing was written");
}

int measure(tomo_mesh *h, hipStream_t st, const Call &c, Res *out) {
    *out = Res{0, 0.0, 0.0};
    if (c.g.blocks == 0) return TOMO_MESH_OK;
    CHK(grow(h, h->counts, sizeof(int) * (size_t)c.g.blocks));
    CHK(grow(h, h->part, 2 * sizeof(double) * (size_t)c.g.blocks));
    CHK(grow(h, h->res, sizeof(Res)));
    int *counts = static_cast<int *>(h->counts.p);
    double *part = static_cast<double *>(h->part.p);
    if (c.dtype == TOMO_MESH_U8) launch_count<uint8_t, true>(st, c, counts, part);
    else launch_count<float, true>(st, c, counts, part);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_total, dim3(1), dim3(ONE), 0, st, (const int *)counts, (const double *)part, c.g.blocks, static_cast<Res *>(h->res.p));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->res.p, sizeof(Res), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return TOMO_MESH_OK;
}

int extract(tomo_mesh *h, hipStream_t st, const Call &c, float *d_tri, long long capacity, long long *n_out) {
    *n_out = 0;
    if (c.g.blocks == 0) return TOMO_MESH_OK;
    CHK(grow(h, h->counts, sizeof(int) * (size_t)c.g.blocks));
    CHK(grow(h, h->offs, sizeof(long long) * ((size_t)c.g.blocks + 1)));
    CHK(grow(h, h->res, sizeof(Res)));
    int *counts = static_cast<int *>(h->counts.p);
    long long *offs = static_cast<long long *>(h->offs.p);
    if (c.dtype == TOMO_MESH_U8) launch_count<uint8_t, false>(st, c, counts, nullptr);
    else launch_count<float, false>(st, c, counts, nullptr);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(ONE), 0, st, (const int *)counts, c.g.blocks, offs, static_cast<Res *>(h->res.p));
    HIPCHK(h, hipGetLastError());
    Res r{0, 0.0, 0.0};
    HIPCHK(h, hipMemcpyAsync(&r, h->res.p, sizeof(Res), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (r.n > (long long)TOMO_MESH_MAX_TRIANGLES) return too_many(h, r.n);
    *n_out = r.n;
    if (r.n > capacity)
        return fail(h, TOMO_MESH_ERR_CAPACITY, "tomo_mesh_extract: the surface has " + std::to_string(r.n) + " triangles, the buffer holds " +
                                                   std::to_string(capacity) + "; nothing was written");
    if (r.n == 0) return TOMO_MESH_OK;
    if (c.dtype == TOMO_MESH_U8) launch_emit<uint8_t>(st, c, counts, offs, d_tri, capacity);
    else launch_emit<float>(st, c, counts, offs, d_tri, capacity);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    return TOMO_MESH_OK;
}

}  // namespace

extern "C" {

TOMO_API int tomo_mesh_abi_version(void) { return 1; }

TOMO_API int tomo_mesh_create(int device, tomo_mesh **out) { return create_plain(device, true, out); }

TOMO_API int tomo_mesh_destroy(tomo_mesh *h) {
    if (!h) return TOMO_MESH_OK;
    (void)hipSetDevice(h->device);
    free_bufs(h->bufs());
    delete h;
    return TOMO_MESH_OK;
}

TOMO_API const char *tomo_mesh_last_error(tomo_mesh *h) { return last_error(h); }

TOMO_API int tomo_mesh_device_bytes(tomo_mesh *h, int64_t *bytes) {
    if (!h || !bytes) return fail(h, TOMO_MESH_ERR_ARG, "tomo_mesh_device_bytes: NULL");
    *bytes = (int64_t)buf_bytes(h->bufs());
    return TOMO_MESH_OK;
}

TOMO_API int tomo_mesh_check_shape(int64_t nx, int64_t ny, int64_t nz) { return check_shape(nullptr, nx, ny, nz); }

TOMO_API int tomo_mesh_measure(tomo_mesh *h, void *stream, const void *d_vol, int dtype, int nx, int ny, int nz, float level, int border,
                               int64_t *n_triangles, double *area, double *volume) {
    CHK(check_call(h, "tomo_mesh_measure", d_vol, dtype, nx, ny, nz, level, border));
    if (!n_triangles || !area || !volume) return fail(h, TOMO_MESH_ERR_ARG, "tomo_mesh_measure: NULL result pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    Res r;
    const int rc = measure(h, st, call_of(d_vol, dtype, nx, ny, nz, level, border), &r);
    CHK(release(h));
    CHK(rc);
    *n_triangles = r.n, *area = r.area, *volume = r.vol6 / 6.0;
    return TOMO_MESH_OK;
}

TOMO_API int tomo_mesh_extract(tomo_mesh *h, void *stream, const void *d_vol, int dtype, int nx, int ny, int nz, float level, int border,
                               float *d_triangles, int64_t capacity, int64_t *n_triangles) {
    CHK(check_call(h, "tomo_mesh_extract", d_vol, dtype, nx, ny, nz, level, border));
    if (!n_triangles) return fail(h, TOMO_MESH_ERR_ARG, "tomo_mesh_extract: NULL result pointer");
    if (capacity < 0 || (capacity > 0 && !d_triangles)) return fail(h, TOMO_MESH_ERR_ARG, "tomo_mesh_extract: capacity must be >= 0, with a buffer if > 0");
    if (!aligned(d_triangles, 4)) return fail(h, TOMO_MESH_ERR_ARG, "tomo_mesh_extract: misaligned pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    long long n = 0;
    const int rc = extract(h, st, call_of(d_vol, dtype, nx, ny, nz, level, border), d_triangles, (long long)capacity, &n);
    *n_triangles = n;
    CHK(release(h));
    return rc;
}

}  // extern "C"
