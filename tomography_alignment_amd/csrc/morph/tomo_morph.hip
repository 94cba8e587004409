// libtomo_morph.so (include/tomo_morph.h): the exact squared Euclidean distance transform of a mask and the ball morphology that is a
// comparison on it.  gfx950 only.  The definitions are in the header; the line routine and the tiles are csrc/tomo_side_lines.h.
//
// k_rows / k_rows_global      the pass along z, which reads the mask: whole rows staged in LDS / a lane per voxel reading the mask itself.
// k_cross / k_cross_global    the passes along y and x: all of a line's length times 4 wq adjacent columns staged in LDS, a lane per group of
//                             four columns, in place where source and destination are one buffer / a lane per group reading f from
//                             global memory, into another buffer.  EPI: what the pass stores -- int32 (0), the byte d2 > r2 (1), the byte
//                             d2 <= r2 (2), the float32 root (3); the last pass of a call takes 1, 2 or 3, so the last int32 volume of
//                             erode / dilate / distance is never written or read back.
// k_root, k_invert, k_select  elementwise, a lane per element.
// Only vector stores and plain C++; no atomics; no work-group waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>

#include "../../../include/tomo_morph.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_MORPH_ERR_ARG, SIDE_ERR_HIP = TOMO_MORPH_ERR_HIP, SIDE_ERR_NODEV = TOMO_MORPH_ERR_NODEV;
}
#include "../tomo_side_host.h"
#include "../tomo_side_lines.h"

namespace {

constexpr int TPB = TOMO_MORPH_GROUP;          // the staged passes
constexpr int EPB = 256;                       // the elementwise kernels and the second path
constexpr int EPI_D2 = 0, EPI_GT = 1, EPI_LE = 2, EPI_ROOT = 3;
static_assert(LINES_INF == TOMO_MORPH_INF && LINES_V == TOMO_MORPH_W && LINES_MAX_WQ == TOMO_MORPH_MAX_WQ, "the header and the line passes agree");
static_assert(4 * TOMO_MORPH_LINE_LIMIT * sizeof(int) <= 64 * 1024, "two work-groups fit in a CU's 160 KiB of LDS");

__device__ inline float root_of(int d2) {
    return d2 == LINES_INF ? std::numeric_limits<float>::infinity() : (float)sqrt((double)d2);
}

// What a pass stores for the four columns from `col` of the element at `at`.
template <int EPI, bool VEC>
struct Put4 {
    void *dst;
    long long cols;
    int r2;
    __device__ void operator()(long long at, long long col, const int best[LINES_V]) const {
        if (EPI == EPI_D2) {
            int *p = static_cast<int *>(dst) + at;
            if (VEC) {
                *reinterpret_cast<int4 *>(p) = make_int4(best[0], best[1], best[2], best[3]);
            } else {
#pragma unroll
                for (int v = 0; v < LINES_V; ++v)
                    if (col + v < cols) p[v] = best[v];
            }
        } else if (EPI == EPI_ROOT) {
            float *p = static_cast<float *>(dst) + at;
            if (VEC) {
                *reinterpret_cast<float4 *>(p) = make_float4(root_of(best[0]), root_of(best[1]), root_of(best[2]), root_of(best[3]));
            } else {
#pragma unroll
                for (int v = 0; v < LINES_V; ++v)
                    if (col + v < cols) p[v] = root_of(best[v]);
            }
        } else {
            uint8_t *p = static_cast<uint8_t *>(dst) + at;
            unsigned c[LINES_V];
#pragma unroll
            for (int v = 0; v < LINES_V; ++v) c[v] = (EPI == EPI_GT ? best[v] > r2 : best[v] <= r2) ? 1u : 0u;
            if (VEC) {
                *reinterpret_cast<unsigned *>(p) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
            } else {
#pragma unroll
                for (int v = 0; v < LINES_V; ++v)
                    if (col + v < cols) p[v] = (uint8_t)c[v];
            }
        }
    }
};

template <bool PACK>
__global__ __launch_bounds__(TPB) void k_rows(const uint8_t *__restrict__ mask, Rows g, int invert, int border, int *__restrict__ dst) {
    extern __shared__ __align__(16) int lds[];
    rows_stage<PACK>(mask, g, blockIdx.x, threadIdx.x, TPB, invert, lds);
    __syncthreads();
    rows_compute(lds, g, blockIdx.x, threadIdx.x, TPB, border != 0, [&](long long at, int best) { dst[at] = best; });
}

__global__ __launch_bounds__(EPB) void k_rows_global(const uint8_t *__restrict__ mask, Rows g, int invert, int border, int *__restrict__ dst) {
    const long long item = (long long)blockIdx.x * EPB + threadIdx.x;
    if (item < g.items) rows_global(mask, g, item, invert, border != 0, [&](long long at, int best) { dst[at] = best; });
}

// src may be dst (EPI_D2, EPI_ROOT): every lane has staged before any lane stores, and a work-group stores only what it staged.
template <int EPI, bool VEC>
__global__ __launch_bounds__(TPB) void k_cross(const int *src, Cross g, int border, void *dst, int r2) {
    extern __shared__ __align__(16) int lds[];
    cross_stage<VEC>(src, g, blockIdx.x, threadIdx.x, TPB, lds);
    __syncthreads();
    cross_compute(lds, g, blockIdx.x, threadIdx.x, TPB, border != 0, Put4<EPI, VEC>{dst, g.cols, r2});
}

template <int EPI, bool VEC>
__global__ __launch_bounds__(EPB) void k_cross_global(const int *__restrict__ src, Cross g, int border, void *__restrict__ dst, int r2) {
    const long long item = (long long)blockIdx.x * EPB + threadIdx.x;
    if (item < g.items) cross_global<VEC>(src, g, item, border != 0, Put4<EPI, VEC>{dst, g.cols, r2});
}

__global__ __launch_bounds__(EPB) void k_root(const int *d2, long long n, float *out) {
    const long long i = (long long)blockIdx.x * EPB + threadIdx.x;
    if (i < n) out[i] = root_of(d2[i]);
}

__global__ __launch_bounds__(EPB) void k_invert(const uint8_t *mask, long long n, uint8_t *out) {
    const long long i = (long long)blockIdx.x * EPB + threadIdx.x;
    if (i < n) out[i] = mask[i] == 0 ? 1 : 0;
}

__global__ __launch_bounds__(EPB) void k_select(const int *__restrict__ labels, long long voxels, int n, const uint8_t *__restrict__ table,
                                                uint8_t *__restrict__ mask) {
    const long long i = (long long)blockIdx.x * EPB + threadIdx.x;
    if (i >= voxels) return;
    const int l = labels[i];
    if (l >= 0 && l <= n && table[l] != 0) mask[i] = 1;
}

inline unsigned blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

struct tomo_morph {
    int device = 0;
    std::string err;
    Buf a;                   // one int32 volume
    Buf b;                   // a second one: a byte result with the y axis on the second path
    int line_limit = TOMO_MORPH_LINE_LIMIT;
    auto bufs() { return std::array{&a, &b}; }
};

namespace {

std::string dims(long long nx, long long ny, long long nz) { return std::to_string(nx) + " x " + std::to_string(ny) + " x " + std::to_string(nz); }

int check_shape(tomo_morph *h, long long nx, long long ny, long long nz) {
    const long long top = TOMO_MORPH_MAX_DIM;
    if (nx < 1 || ny < 1 || nz < 1 || nx > top || ny > top || nz > top)
        return fail(h, TOMO_MORPH_ERR_UNSUPPORTED, "tomo_morph: a volume of " + dims(nx, ny, nz) + " is outside 1 <= nx, ny, nz <= " +
                                                       std::to_string(top) + "; nothing was launched");
    if (nx * ny * nz > (long long)TOMO_MORPH_MAX_VOXELS)                 // at most 2^42: no overflow
        return fail(h, TOMO_MORPH_ERR_UNSUPPORTED, "tomo_morph: a volume of " + dims(nx, ny, nz) + " has more than 2^31 - 1 voxels; nothing was launched");
    return TOMO_MORPH_OK;
}

int check_call(tomo_morph *h, const char *what, const void *p, const void *q, uintptr_t qalign, int nx, int ny, int nz) {
    if (!h) return fail(h, TOMO_MORPH_ERR_ARG, std::string(what) + ": NULL handle");
    if (!p || !q) return fail(h, TOMO_MORPH_ERR_ARG, std::string(what) + ": NULL pointer");
    if (!aligned(q, qalign)) return fail(h, TOMO_MORPH_ERR_ARG, std::string(what) + ": misaligned pointer");
    return check_shape(h, nx, ny, nz);
}

// Scratch above TOMO_MORPH_KEEP_BYTES goes back before a call returns, once the stream has run dry.
int release(tomo_morph *h, hipStream_t st) {
    bool waited = false;
    for (Buf *b : h->bufs())
        if (b->p && b->n > (size_t)TOMO_MORPH_KEEP_BYTES) {
            if (!waited) HIPCHK(h, hipStreamSynchronize(st));
            waited = true;
            HIPCHK(h, hipFree(b->p));
            b->p = nullptr, b->n = 0;
        }
    return TOMO_MORPH_OK;
}

int pass_rows(tomo_morph *h, hipStream_t st, const uint8_t *mask, int nx, int ny, int nz, int invert, int border, int *dst) {
    const long long tile = 4LL * h->line_limit;
    const Rows g = rows_of(nx, ny, nz, tile);
    if (nz <= h->line_limit) {
        const size_t lds = sizeof(int) * (size_t)rows_lds_ints(g);
        if (nz % 4 == 0 && aligned(mask, 4))
            hipLaunchKernelGGL(k_rows<true>, dim3((unsigned)g.blocks), dim3(TPB), lds, st, mask, g, invert, border, dst);
        else
            hipLaunchKernelGGL(k_rows<false>, dim3((unsigned)g.blocks), dim3(TPB), lds, st, mask, g, invert, border, dst);
    } else {
        hipLaunchKernelGGL(k_rows_global, dim3(blocks_of(g.items, EPB)), dim3(EPB), 0, st, mask, g, invert, border, dst);
    }
    HIPCHK(h, hipGetLastError());
    return TOMO_MORPH_OK;
}

template <int EPI>
int pass_cross_epi(tomo_morph *h, hipStream_t st, const int *src, int nx, int ny, int nz, int axis, int border, void *dst, int r2) {
    const long long tile = 4LL * h->line_limit;
    const Cross g = cross_of(nx, ny, nz, axis, tile);
    const bool vec = g.cols % 4 == 0 && aligned(src, 16) && aligned(dst, (EPI == EPI_GT || EPI == EPI_LE) ? 4 : 16);
    if (g.n <= h->line_limit) {
        const size_t lds = sizeof(int) * (size_t)cross_lds_ints(g);
        if (vec) hipLaunchKernelGGL((k_cross<EPI, true>), dim3((unsigned)g.blocks), dim3(TPB), lds, st, src, g, border, dst, r2);
        else hipLaunchKernelGGL((k_cross<EPI, false>), dim3((unsigned)g.blocks), dim3(TPB), lds, st, src, g, border, dst, r2);
    } else {
        if (static_cast<const void *>(src) == dst) return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph: the second path cannot run in place");
        if (vec) hipLaunchKernelGGL((k_cross_global<EPI, true>), dim3(blocks_of(g.items, EPB)), dim3(EPB), 0, st, src, g, border, dst, r2);
        else hipLaunchKernelGGL((k_cross_global<EPI, false>), dim3(blocks_of(g.items, EPB)), dim3(EPB), 0, st, src, g, border, dst, r2);
    }
    HIPCHK(h, hipGetLastError());
    return TOMO_MORPH_OK;
}

int pass_cross(tomo_morph *h, hipStream_t st, const int *src, int nx, int ny, int nz, int axis, int border, void *dst, int epi, int r2) {
    switch (epi) {
    case EPI_D2: return pass_cross_epi<EPI_D2>(h, st, src, nx, ny, nz, axis, border, dst, r2);
    case EPI_GT: return pass_cross_epi<EPI_GT>(h, st, src, nx, ny, nz, axis, border, dst, r2);
    case EPI_LE: return pass_cross_epi<EPI_LE>(h, st, src, nx, ny, nz, axis, border, dst, r2);
    default: return pass_cross_epi<EPI_ROOT>(h, st, src, nx, ny, nz, axis, border, dst, r2);
    }
}

// The three passes, z, y, x, from the mask to d_out, which the last pass writes as `epi` says.  A pass on the LDS path may work in place, one
// on the second path needs another buffer than its source; so, from the end: the x pass reads the output itself (a 4-byte type) or scratch a;
// the y pass reads that same buffer or the other one.
int transform(tomo_morph *h, hipStream_t st, const uint8_t *d_mask, int nx, int ny, int nz, int invert, int border, void *d_out, int epi, int r2) {
    const size_t bytes = sizeof(int) * (size_t)nx * ny * nz;
    const bool wide = epi == EPI_D2 || epi == EPI_ROOT, x_lds = nx <= h->line_limit, y_lds = ny <= h->line_limit;
    int *out = static_cast<int *>(d_out), *from_y, *from_z;
    if (wide && x_lds && y_lds) {
        from_y = from_z = out;
    } else {
        CHK(grow(h, h->a, bytes));
        int *a = static_cast<int *>(h->a.p);
        from_y = (wide && x_lds) ? out : a;
        if (y_lds) {
            from_z = from_y;
        } else if (wide) {
            from_z = from_y == out ? a : out;
        } else {
            CHK(grow(h, h->b, bytes));
            from_z = static_cast<int *>(h->b.p);
        }
    }
    CHK(pass_rows(h, st, d_mask, nx, ny, nz, invert, border, from_z));
    CHK(pass_cross(h, st, from_z, nx, ny, nz, 1, border, from_y, EPI_D2, 0));
    CHK(pass_cross(h, st, from_y, nx, ny, nz, 0, border, d_out, epi, r2));
    return TOMO_MORPH_OK;
}

// r2 as the passes compare it: INF is above every r2, and no finite distance is above 2^31 - 2.
int clamp_r2(int64_t r2) { return (int)std::min<int64_t>(r2, (int64_t)TOMO_MORPH_INF - 1); }

int check_ball(tomo_morph *h, const char *what, int64_t r2, int border_value) {
    if (r2 < 0) return fail(h, TOMO_MORPH_ERR_ARG, std::string(what) + ": r2 must be >= 0; nothing was launched");
    if (border_value != 0 && border_value != 1) return fail(h, TOMO_MORPH_ERR_ARG, std::string(what) + ": border_value must be 0 or 1; nothing was launched");
    return TOMO_MORPH_OK;
}

int erode(tomo_morph *h, hipStream_t st, const uint8_t *m, int nx, int ny, int nz, int64_t r2, int border_value, uint8_t *out) {
    return transform(h, st, m, nx, ny, nz, 0, border_value == 0 ? 1 : 0, out, EPI_GT, clamp_r2(r2));
}

int dilate(tomo_morph *h, hipStream_t st, const uint8_t *m, int nx, int ny, int nz, int64_t r2, uint8_t *out) {
    return transform(h, st, m, nx, ny, nz, 1, 0, out, EPI_LE, clamp_r2(r2));
}

}  // namespace

extern "C" {

TOMO_API int tomo_morph_abi_version(void) { return 1; }

TOMO_API int tomo_morph_create(int device, tomo_morph **out) { return create_plain(device, true, out); }

TOMO_API int tomo_morph_destroy(tomo_morph *h) {
    if (!h) return TOMO_MORPH_OK;
    (void)hipSetDevice(h->device);
    free_bufs(h->bufs());
    delete h;
    return TOMO_MORPH_OK;
}

TOMO_API const char *tomo_morph_last_error(tomo_morph *h) { return last_error(h); }

TOMO_API int tomo_morph_device_bytes(tomo_morph *h, int64_t *bytes) {
    if (!h || !bytes) return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_device_bytes: NULL");
    *bytes = (int64_t)buf_bytes(h->bufs());
    return TOMO_MORPH_OK;
}

TOMO_API int tomo_morph_check_shape(int64_t nx, int64_t ny, int64_t nz) { return check_shape(nullptr, nx, ny, nz); }

TOMO_API int tomo_morph_set_line_limit(tomo_morph *h, int n) {
    if (!h) return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_set_line_limit: NULL handle");
    if (n < 0 || n > TOMO_MORPH_LINE_LIMIT) return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_set_line_limit: the limit is 0 ... " + std::to_string(TOMO_MORPH_LINE_LIMIT));
    h->line_limit = n == 0 ? TOMO_MORPH_LINE_LIMIT : n;
    return TOMO_MORPH_OK;
}

TOMO_API int tomo_morph_distance_sq(tomo_morph *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int border, int32_t *d_out) {
    CHK(check_call(h, "tomo_morph_distance_sq", d_mask, d_out, 4, nx, ny, nz));
    if (border != 0 && border != 1) return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_distance_sq: border must be 0 or 1; nothing was launched");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    CHK(transform(h, st, d_mask, nx, ny, nz, 0, border, d_out, EPI_D2, 0));
    return release(h, st);
}

TOMO_API int tomo_morph_distance(tomo_morph *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int border, float *d_out) {
    CHK(check_call(h, "tomo_morph_distance", d_mask, d_out, 4, nx, ny, nz));
    if (border != 0 && border != 1) return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_distance: border must be 0 or 1; nothing was launched");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    CHK(transform(h, st, d_mask, nx, ny, nz, 0, border, d_out, EPI_ROOT, 0));
    return release(h, st);
}

TOMO_API int tomo_morph_line_pass(tomo_morph *h, void *stream, const void *d_src, int nx, int ny, int nz, int axis, int border, int32_t *d_dst) {
    CHK(check_call(h, "tomo_morph_line_pass", d_src, d_dst, 4, nx, ny, nz));
    if (axis < 0 || axis > 2 || (border != 0 && border != 1) || (axis < 2 && !aligned(d_src, 4)))
        return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_line_pass: axis must be 0, 1 or 2, border 0 or 1, an int32 source aligned; nothing was launched");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    if (axis == 2) return pass_rows(h, st, static_cast<const uint8_t *>(d_src), nx, ny, nz, 0, border, d_dst);
    return pass_cross(h, st, static_cast<const int *>(d_src), nx, ny, nz, axis, border, d_dst, EPI_D2, 0);
}

TOMO_API int tomo_morph_root(tomo_morph *h, void *stream, const int32_t *d_d2, int64_t n, float *d_out) {
    if (!h) return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_root: NULL handle");
    if (!d_d2 || !d_out || n < 1 || n > (int64_t)TOMO_MORPH_MAX_VOXELS) return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_root: bad argument");
    if (!aligned(d_d2, 4) || !aligned(d_out, 4)) return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_root: misaligned pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_root, dim3(blocks_of(n, EPB)), dim3(EPB), 0, st, d_d2, (long long)n, d_out);
    HIPCHK(h, hipGetLastError());
    return TOMO_MORPH_OK;
}

TOMO_API int tomo_morph_erode(tomo_morph *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int64_t r2, int border_value,
                              uint8_t *d_out) {
    CHK(check_call(h, "tomo_morph_erode", d_mask, d_out, 1, nx, ny, nz));
    CHK(check_ball(h, "tomo_morph_erode", r2, border_value));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    CHK(erode(h, st, d_mask, nx, ny, nz, r2, border_value, d_out));
    return release(h, st);
}

TOMO_API int tomo_morph_dilate(tomo_morph *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int64_t r2, uint8_t *d_out) {
    CHK(check_call(h, "tomo_morph_dilate", d_mask, d_out, 1, nx, ny, nz));
    CHK(check_ball(h, "tomo_morph_dilate", r2, 0));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    CHK(dilate(h, st, d_mask, nx, ny, nz, r2, d_out));
    return release(h, st);
}

TOMO_API int tomo_morph_open(tomo_morph *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int64_t r2, int border_value,
                             uint8_t *d_out) {
    CHK(check_call(h, "tomo_morph_open", d_mask, d_out, 1, nx, ny, nz));
    CHK(check_ball(h, "tomo_morph_open", r2, border_value));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    CHK(erode(h, st, d_mask, nx, ny, nz, r2, border_value, d_out));
    CHK(dilate(h, st, d_out, nx, ny, nz, r2, d_out));
    return release(h, st);
}

TOMO_API int tomo_morph_close(tomo_morph *h, void *stream, const uint8_t *d_mask, int nx, int ny, int nz, int64_t r2, int border_value,
                              uint8_t *d_out) {
    CHK(check_call(h, "tomo_morph_close", d_mask, d_out, 1, nx, ny, nz));
    CHK(check_ball(h, "tomo_morph_close", r2, border_value));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    CHK(dilate(h, st, d_mask, nx, ny, nz, r2, d_out));
    CHK(erode(h, st, d_out, nx, ny, nz, r2, border_value, d_out));
    return release(h, st);
}

TOMO_API int tomo_morph_invert(tomo_morph *h, void *stream, const uint8_t *d_mask, int64_t n, uint8_t *d_out) {
    if (!h) return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_invert: NULL handle");
    if (!d_mask || !d_out || n < 1 || n > (int64_t)TOMO_MORPH_MAX_VOXELS) return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_invert: bad argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_invert, dim3(blocks_of(n, EPB)), dim3(EPB), 0, st, d_mask, (long long)n, d_out);
    HIPCHK(h, hipGetLastError());
    return TOMO_MORPH_OK;
}

TOMO_API int tomo_morph_select(tomo_morph *h, void *stream, const int32_t *d_labels, int64_t voxels, int32_t n, const uint8_t *d_table,
                               uint8_t *d_mask) {
    if (!h) return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_select: NULL handle");
    if (!d_labels || !d_table || !d_mask || voxels < 1 || voxels > (int64_t)TOMO_MORPH_MAX_VOXELS || n < 0)
        return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_select: bad argument");
    if (!aligned(d_labels, 4)) return fail(h, TOMO_MORPH_ERR_ARG, "tomo_morph_select: misaligned pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_select, dim3(blocks_of(voxels, EPB)), dim3(EPB), 0, st, d_labels, (long long)voxels, (int)n, d_table, d_mask);
    HIPCHK(h, hipGetLastError());
    return TOMO_MORPH_OK;
}

}  // extern "C"
