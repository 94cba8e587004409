// tomo_reg.hip -- the vector kernels of the reference's regularised solvers: the soft-threshold of ISTA /
// LASSO (recon/regularized.py:433-440, used at :278,321,375) and the total-variation proximal step of TV-FISTA
// (utilities/tv_denoise.py:98-170 denoise_fista with its helpers gradient :34-59, div :20-31, _projector_on_dual :67-75,
// dual_gap :78-95; called from recon/regularized.py:93), and the fused per-iteration passes of the solvers' drivers
// (recon/regularized.py RegularizedRecon, below): the device-resident pieces between two projector applications, so a regularised
// iteration never has to bring the volume back over PCIe.  HBM-streaming stencil kernels: lanes along z (the contiguous axis), +-1 neighbours in
// x / y come from rows the same work-group's neighbours touch (L2).
#include <algorithm>
#include <initializer_list>
#include <vector>

#include "tomo_ctx.h"

// out = sign(x) * max(|x| - lambda, 0) written as the reference does: x - l where x > l, x + l where x < -l, else 0
__global__ __launch_bounds__(256) void k_soft_threshold(float *__restrict__ out, const float *__restrict__ x, int64_t n, float l)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float v = x[i];
        out[i] = v > l ? v - l : (v < -l ? v + l : 0.f);
    }
}

extern "C" int tomo_vec_soft_threshold(tomo_ctx *ctx, float *d_out, const float *d_x, int64_t n, float lambda)
{
    if (!ctx) return tomo_fail(nullptr, TOMO_ERR_ARG, "null ctx");
    if (n < 0 || (n > 0 && (!d_out || !d_x))) return tomo_fail(ctx, TOMO_ERR_ARG, "tomo_vec_soft_threshold: bad args");
    if (n == 0) return TOMO_OK;
    TOMO_LAUNCH(ctx, "k_soft_threshold", k_soft_threshold, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, d_out, d_x, n, lambda);
    return TOMO_OK;
}

// a float32 product the backend cannot fuse with the add that follows (the build's -ffp-contract=fast reaches the backend, and
// __fmul_rn is a plain product in this compiler's headers): the empty asm pins the rounded product, as csrc/tomo_f2py.hip does
__device__ __forceinline__ float reg_mul(float a, float b) { float p = a * b; asm volatile("" : "+v"(p)); return p; }

// ------------------------------------------------------------------------------------------------
// TV-FISTA.  Volume [nx][ny][nz], z fastest.  Grid: (z chunks of 256, ny, nx).
// The kernels apply the reference's float32 operations in the reference's order, every product rounded on its own (reg_mul; the
// adds and subtractions are __fadd_rn / __fsub_rn, which have no product left to fuse with): the only fused float32 operations are the
// refinement steps inside the IEEE division; the square root is one v_sqrt_f32, good to a unit in the last place.  A float32 numpy
// model of the iteration (tests/tv_model.py) is therefore met bit for bit wherever the projection on the unit ball divides by 1, and
// to the last place of the square root elsewhere.
// ------------------------------------------------------------------------------------------------
struct TvDims { int nx, ny, nz; int64_t sy, sx; };

// divergence of a 3-component field with the reference's boundary rule (utilities/tv_denoise.py:26-30):
//   d_a[i] = (i < n_a - 1 ? g_a[i] : 0) - (i > 0 ? g_a[i - 1] : 0), summed over the axes in the order x, y, z (adds in the
//   order the reference's in-place += / -= apply them)
__device__ __forceinline__ float tv_div_at(const float *gx, const float *gy, const float *gz, int64_t i, int ix, int iy, int iz, const TvDims &d)
{
    float r = 0.f;
    if (ix < d.nx - 1) r += gx[i];
    if (ix > 0) r -= gx[i - d.sx];
    if (iy < d.ny - 1) r += gy[i];
    if (iy > 0) r -= gy[i - d.sy];
    if (iz < d.nz - 1) r += gz[i];
    if (iz > 0) r -= gz[i - 1];
    return r;
}

// err = weight * div(grad_aux) - im                                                       tv_denoise.py:151
__global__ __launch_bounds__(256) void k_tv_error(const float *__restrict__ ax, const float *__restrict__ ay, const float *__restrict__ az,
                                                  const float *__restrict__ im, float *__restrict__ err, TvDims d, float weight)
{
    const int iz = blockIdx.x * 256 + threadIdx.x, iy = blockIdx.y, ix = blockIdx.z;
    if (iz >= d.nz) return;
    const int64_t i = (int64_t)ix * d.sx + (int64_t)iy * d.sy + iz;
    err[i] = __fsub_rn(reg_mul(weight, tv_div_at(ax, ay, az, i, ix, iy, iz, d)), im[i]);
}

// grad_tmp = gradient(err) / (factor * weight); grad_aux += grad_tmp; project on the unit ball; FISTA combination
//                                                                                          tv_denoise.py:152-158, :34-59, :67-75
__global__ __launch_bounds__(256) void k_tv_update(float *__restrict__ ax, float *__restrict__ ay, float *__restrict__ az,
                                                   float *__restrict__ px, float *__restrict__ py, float *__restrict__ pz,
                                                   const float *__restrict__ err, TvDims d, float c, float one_tf, float tf)
{
    const int iz = blockIdx.x * 256 + threadIdx.x, iy = blockIdx.y, ix = blockIdx.z;
    if (iz >= d.nz) return;
    const int64_t i = (int64_t)ix * d.sx + (int64_t)iy * d.sy + iz;
    const float e0 = err[i];
    const float gx = ix < d.nx - 1 ? __fsub_rn(err[i + d.sx], e0) : 0.f;      // forward differences, 0 at the last index of an axis
    const float gy = iy < d.ny - 1 ? __fsub_rn(err[i + d.sy], e0) : 0.f;
    const float gz = iz < d.nz - 1 ? __fsub_rn(err[i + 1], e0) : 0.f;
    const float a0 = __fadd_rn(ax[i], reg_mul(gx, c)), a1 = __fadd_rn(ay[i], reg_mul(gy, c)), a2 = __fadd_rn(az[i], reg_mul(gz, c));
    const float nrm = fmaxf(__fsqrt_rn(__fadd_rn(__fadd_rn(reg_mul(a0, a0), reg_mul(a1, a1)), reg_mul(a2, a2))), 1.f);
    const float p0 = __fdiv_rn(a0, nrm), p1 = __fdiv_rn(a1, nrm), p2 = __fdiv_rn(a2, nrm);
    ax[i] = __fsub_rn(reg_mul(one_tf, p0), reg_mul(tf, px[i]));                // (1 + t_factor) * grad_tmp - t_factor * grad_im   :158
    ay[i] = __fsub_rn(reg_mul(one_tf, p1), reg_mul(tf, py[i]));
    az[i] = __fsub_rn(reg_mul(one_tf, p2), reg_mul(tf, pz[i]));
    px[i] = p0; py[i] = p1; pz[i] = p2;                                            // grad_im = grad_tmp                               :159
}

__device__ __forceinline__ void tv_block_sum(double v, double *dst)
{
    __shared__ double sh[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(dst, sh[0] + sh[1] + sh[2] + sh[3]);
    __syncthreads();
}

// gap = weight * div(grad_im); new = im - gap; sums of gap^2, new^2, im^2                  tv_denoise.py:162-163, :84,94
__global__ __launch_bounds__(256) void k_tv_new(const float *__restrict__ px, const float *__restrict__ py, const float *__restrict__ pz,
                                                const float *__restrict__ im, float *__restrict__ out, TvDims d, float weight, double *__restrict__ red)
{
    const int iz = blockIdx.x * 256 + threadIdx.x, iy = blockIdx.y, ix = blockIdx.z;
    double s_gap = 0.0, s_new = 0.0, s_im = 0.0;
    if (iz < d.nz) {
        const int64_t i = (int64_t)ix * d.sx + (int64_t)iy * d.sy + iz;
        const float gap = reg_mul(weight, tv_div_at(px, py, pz, i, ix, iy, iz, d));
        const float v = im[i], nw = __fsub_rn(v, gap);
        out[i] = nw;
        s_gap = (double)gap * gap; s_new = (double)nw * nw; s_im = (double)v * v;
    }
    tv_block_sum(s_gap, red + 0);
    tv_block_sum(s_new, red + 1);
    tv_block_sum(s_im, red + 2);
}

// sum over voxels of sqrt(gx^2 + gy^2 + gz^2) (ISO = 1: the isotropic TV of dual_gap, tv_denoise.py:85-92) or of gx^2 + gy^2 + gz^2
// (ISO = 0: tv_norm_3d = ||gradient(x)||_2, :62-64), forward differences with 0 at the last index
template <int ISO>
__global__ __launch_bounds__(256) void k_tv_norm(const float *__restrict__ x, TvDims d, double *__restrict__ red)
{
    const int iz = blockIdx.x * 256 + threadIdx.x, iy = blockIdx.y, ix = blockIdx.z;
    double s = 0.0;
    if (iz < d.nz) {
        const int64_t i = (int64_t)ix * d.sx + (int64_t)iy * d.sy + iz;
        const float v = x[i];
        const float gx = ix < d.nx - 1 ? x[i + d.sx] - v : 0.f, gy = iy < d.ny - 1 ? x[i + d.sy] - v : 0.f, gz = iz < d.nz - 1 ? x[i + 1] - v : 0.f;
        const float q = __fadd_rn(__fadd_rn(reg_mul(gx, gx), reg_mul(gy, gy)), reg_mul(gz, gz));
        s = ISO ? (double)__fsqrt_rn(q) : (double)q;
    }
    tv_block_sum(s, red);
}

static int tv_dims(tomo_ctx *ctx, int nx, int ny, int nz, TvDims &d, dim3 &grid)
{
    if (nx < 2 || ny < 2 || nz < 2) return tomo_fail(ctx, TOMO_ERR_ARG, "tv: every axis needs at least 2 voxels (the reference's div indexes [-2])");
    if (ny > 65535 || nx > 65535) return tomo_fail(ctx, TOMO_ERR_UNSUPPORTED, "tv: nx, ny <= 65535");
    d.nx = nx; d.ny = ny; d.nz = nz; d.sy = nz; d.sx = (int64_t)ny * nz;
    grid = dim3((nz + 255) / 256, ny, nx);
    return TOMO_OK;
}

extern "C" int tomo_tv_norm_3d(tomo_ctx *ctx, const float *d_x, int nx, int ny, int nz, double *h_norm)
{
    if (!ctx || !d_x || !h_norm) return tomo_fail(ctx, TOMO_ERR_ARG, "tomo_tv_norm_3d: bad args");
    TvDims d;
    dim3 grid;
    int rc = tv_dims(ctx, nx, ny, nz, d, grid);
    if (rc) return rc;
    rc = tomo_ensure_red(ctx, 8);
    if (rc) return rc;
    TOMO_HIP(ctx, hipMemsetAsync(ctx->d_red, 0, sizeof(double), ctx->stream));
    TOMO_LAUNCH(ctx, "k_tv_norm", k_tv_norm<0>, grid, dim3(256), 0, d_x, d, ctx->d_red);
    TOMO_HIP(ctx, hipMemcpyAsync(ctx->h_red, ctx->d_red, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TOMO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *h_norm = sqrt(ctx->h_red[0]);
    return TOMO_OK;
}

extern "C" int tomo_tv_denoise_fista(tomo_ctx *ctx, const float *d_im, float *d_out, int nx, int ny, int nz, double weight, int niter, double eps,
                                     int check_gap_frequency, int *h_iters, double *h_dual_gap)
{
    if (!ctx || !d_im || !d_out || niter < 0 || check_gap_frequency < 1 || !(weight > 0.0)) return tomo_fail(ctx, TOMO_ERR_ARG, "tomo_tv_denoise_fista: bad args");
    TvDims d;
    dim3 grid;
    int rc = tv_dims(ctx, nx, ny, nz, d, grid);
    if (rc) return rc;
    rc = tomo_ensure_red(ctx, 8);
    if (rc) return rc;
    const size_t n = (size_t)nx * ny * nz;
    TOMO_HIP(ctx, hipSetDevice(ctx->device));
    // grad_aux[3], grad_im[3], err: kept in the context across calls (grow-only, like d_stage / d_red) -- a proximal step per
    // outer iteration of a regularised solver used to pay a 7 n hipMalloc + hipFree (28 GB at 1024^3, each an implicit device sync)
    rc = tomo_ensure_ws(ctx, 7 * n);
    if (rc) return rc;
    float *ws = ctx->d_ws;
    float *ax = ws, *ay = ws + n, *az = ws + 2 * n, *px = ws + 3 * n, *py = ws + 4 * n, *pz = ws + 5 * n, *err = ws + 6 * n;
    double dgap = 0.0;
    int i = 0;
    if (h_iters) *h_iters = 0;
    if (h_dual_gap) *h_dual_gap = 0.0;
    TOMO_HIP(ctx, hipMemsetAsync(ws, 0, 6 * n * sizeof(float), ctx->stream));                                        // :144-145
    TOMO_HIP(ctx, hipMemcpyAsync(d_out, d_im, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));           // new = im.copy()  :148
    const float w = (float)weight, c = (float)(1.0 / (12.0 * weight));                                               // factor 12 for 3-D  :139-142,153
    double t = 1.0;
    while (i < niter) {                                                                                              // :149
        TOMO_LAUNCH(ctx, "k_tv_error", k_tv_error, grid, dim3(256), 0, (const float *)ax, (const float *)ay, (const float *)az, d_im, err, d, w);
        const double t_new = 0.5 * (1.0 + sqrt(1.0 + 4.0 * t * t)), t_factor = (t - 1.0) / t_new;                   // :156-157
        TOMO_LAUNCH(ctx, "k_tv_update", k_tv_update, grid, dim3(256), 0, ax, ay, az, px, py, pz, (const float *)err, d, c, (float)(1.0 + t_factor), (float)t_factor);
        t = t_new;
        if (i % check_gap_frequency == 0) {                                                                          // :161-166
            TOMO_HIP(ctx, hipMemsetAsync(ctx->d_red, 0, 4 * sizeof(double), ctx->stream));
            TOMO_LAUNCH(ctx, "k_tv_new", k_tv_new, grid, dim3(256), 0, (const float *)px, (const float *)py, (const float *)pz, d_im, d_out, d, w, ctx->d_red);
            TOMO_LAUNCH(ctx, "k_tv_norm", k_tv_norm<1>, grid, dim3(256), 0, (const float *)d_out, d, ctx->d_red + 3);
            TOMO_HIP(ctx, hipMemcpyAsync(ctx->h_red, ctx->d_red, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            TOMO_HIP(ctx, hipStreamSynchronize(ctx->stream));
            const double s_gap = ctx->h_red[0], s_new = ctx->h_red[1], im_norm = ctx->h_red[2], tv_new = 2.0 * weight * ctx->h_red[3];
            dgap = im_norm > 0.0 ? 0.5 / im_norm * (s_gap + tv_new - im_norm + s_new) : 0.0;                        // :93-95
            if (dgap < eps) break;                                                                                   // :165-166 (i is not advanced)
        }
        ++i;
    }
    TOMO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_iters) *h_iters = i;
    if (h_dual_gap) *h_dual_gap = dgap;
    return TOMO_OK;
}

// ------------------------------------------------------------------------------------------------
// The regularised solvers' per-iteration vector work (recon/regularized.py RegularizedRecon; include/tomo.h lists the reference lines
// each entry point restates).  Every kernel is ONE streaming pass over float32 volumes that also produces the iteration's scalars:
//   - elementwise float arithmetic in the reference's operation order, every product rounded on its own (reg_mul, above the TV
//     section), so no contraction into an FMA changes a bit against numpy float32 (the build has -ffp-contract=fast);
//   - 16-byte loads / stores on the body when every operand has the same offset from a 16-byte boundary (a scalar head and tail take
//     the rest; operands of mixed offsets take the scalar loop throughout);
//   - the scalars are summed in float64 DETERMINISTICALLY: a fixed grid (it depends on n only, never on the device) in which every
//     thread adds its elements in a fixed order, every block writes its partial to ctx->d_red_part, and a single-block pass adds the
//     partials in index order to the d_acc slots.  The same input gives the same bits on every call and every rank, which is what
//     lets the sharded solvers take their control decisions (stop rule, line-search acceptance) without a broadcast.
// ------------------------------------------------------------------------------------------------
#define REG_BLOCK 256
#define REG_MAX_GRID 2048
#define REG_MAX_NS 3

__device__ __forceinline__ float reg_soft(float y, float l) { return y > l ? __fsub_rn(y, l) : (y < -l ? __fadd_rn(y, l) : 0.f); }
__device__ __forceinline__ double reg_sq(float v) { return (double)v * (double)v; }

template <int NS>
__device__ __forceinline__ void reg_block_partials(double (&s)[NS], double *part)
{
    __shared__ double sh[NS][REG_BLOCK / 64];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        double v = s[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        const int k = threadIdx.x;
        part[(size_t)k * gridDim.x + blockIdx.x] = ((sh[k][0] + sh[k][1]) + sh[k][2]) + sh[k][3];
    }
}

// acc[slot + k] += sum_b part[k * nb + b] (or = with `assign`), the partials added in index order
__global__ __launch_bounds__(REG_BLOCK) void k_reg_final(const double *__restrict__ part, int nb, int ns, double *dst, int assign)
{
    __shared__ double sh[REG_BLOCK / 64];
    for (int k = 0; k < ns; ++k) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nb; b += REG_BLOCK) v += part[(size_t)k * nb + b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            const double t = ((sh[0] + sh[1]) + sh[2]) + sh[3];
            dst[k] = assign ? t : dst[k] + t;
        }
        __syncthreads();
    }
}

// Element ops: at(i, s) does element i; at4(i, s) does the aligned four from i (same arithmetic per element).
struct OpFistaMom {          // rec = u + c (u - u_old); s0 += (gt - rec)^2                              regularized.py:102,113
    float *rec; const float *u, *uo, *gt; float c;
    static constexpr int NS = 1;
    __device__ __forceinline__ float one(float u_, float uo_) const { return __fadd_rn(u_, reg_mul(c, __fsub_rn(u_, uo_))); }
    __device__ __forceinline__ void at(int64_t i, double (&s)[NS]) const
    {
        const float r = one(u[i], uo[i]);
        rec[i] = r;
        if (gt) s[0] += reg_sq(__fsub_rn(gt[i], r));
    }
    __device__ __forceinline__ void at4(int64_t i, double (&s)[NS]) const
    {
        const float4 a = *(const float4 *)(u + i), b = *(const float4 *)(uo + i);
        const float4 r = make_float4(one(a.x, b.x), one(a.y, b.y), one(a.z, b.z), one(a.w, b.w));
        *(float4 *)(rec + i) = r;
        if (gt) {
            const float4 g = *(const float4 *)(gt + i);
            s[0] += reg_sq(__fsub_rn(g.x, r.x)) + reg_sq(__fsub_rn(g.y, r.y)) + reg_sq(__fsub_rn(g.z, r.z)) + reg_sq(__fsub_rn(g.w, r.w));
        }
    }
};

struct OpTikhGrad {          // bp -> grad = -bp + lam rec; s0 += grad^2, s1 += rec^2                    regularized.py:180,188-189
    float *bp; const float *rec; float lam;
    static constexpr int NS = 2;
    __device__ __forceinline__ float one(float b, float r) const { return __fadd_rn(-b, reg_mul(lam, r)); }
    __device__ __forceinline__ void at(int64_t i, double (&s)[NS]) const
    {
        const float r = rec[i], g = one(bp[i], r);
        bp[i] = g;
        s[0] += reg_sq(g);
        s[1] += reg_sq(r);
    }
    __device__ __forceinline__ void at4(int64_t i, double (&s)[NS]) const
    {
        const float4 b = *(const float4 *)(bp + i), r = *(const float4 *)(rec + i);
        const float4 g = make_float4(one(b.x, r.x), one(b.y, r.y), one(b.z, r.z), one(b.w, r.w));
        *(float4 *)(bp + i) = g;
        s[0] += reg_sq(g.x) + reg_sq(g.y) + reg_sq(g.z) + reg_sq(g.w);
        s[1] += reg_sq(r.x) + reg_sq(r.y) + reg_sq(r.z) + reg_sq(r.w);
    }
};

struct OpTrial {             // out = x + a d; s0 += out^2                         (scipy line_search_armijo's xk + alpha1 * pk)
    float *out; const float *x, *d; float a;
    static constexpr int NS = 1;
    __device__ __forceinline__ float one(float x_, float d_) const { return __fadd_rn(x_, reg_mul(a, d_)); }
    __device__ __forceinline__ void at(int64_t i, double (&s)[NS]) const
    {
        const float o = one(x[i], d[i]);
        out[i] = o;
        s[0] += reg_sq(o);
    }
    __device__ __forceinline__ void at4(int64_t i, double (&s)[NS]) const
    {
        const float4 p = *(const float4 *)(x + i), q = *(const float4 *)(d + i);
        const float4 o = make_float4(one(p.x, q.x), one(p.y, q.y), one(p.z, q.z), one(p.w, q.w));
        *(float4 *)(out + i) = o;
        s[0] += reg_sq(o.x) + reg_sq(o.y) + reg_sq(o.z) + reg_sq(o.w);
    }
};

struct OpClampErr {          // rec[rec < 0] = 0 (positivity); s0 += (gt - rec)^2                         regularized.py:200-207
    float *rec; const float *gt; int pos;
    static constexpr int NS = 1;
    __device__ __forceinline__ float one(float r) const { return (pos && r < 0.f) ? 0.f : r; }
    __device__ __forceinline__ void at(int64_t i, double (&s)[NS]) const
    {
        const float r = one(rec[i]);
        if (pos) rec[i] = r;
        if (gt) s[0] += reg_sq(__fsub_rn(gt[i], r));
    }
    __device__ __forceinline__ void at4(int64_t i, double (&s)[NS]) const
    {
        float4 r = *(const float4 *)(rec + i);
        r = make_float4(one(r.x), one(r.y), one(r.z), one(r.w));
        if (pos) *(float4 *)(rec + i) = r;
        if (gt) {
            const float4 g = *(const float4 *)(gt + i);
            s[0] += reg_sq(__fsub_rn(g.x, r.x)) + reg_sq(__fsub_rn(g.y, r.y)) + reg_sq(__fsub_rn(g.z, r.z)) + reg_sq(__fsub_rn(g.w, r.w));
        }
    }
};

struct OpProxL1Trial {       // xp = soft(x - t g, tl); Gt = x - xp; s0 += g Gt, s1 += Gt^2                regularized.py:321-326
    float *xp; const float *x, *g; float t, tl;
    static constexpr int NS = 2;
    __device__ __forceinline__ float one(float x_, float g_, double (&s)[NS]) const
    {
        const float p = reg_soft(__fsub_rn(x_, reg_mul(t, g_)), tl), G = __fsub_rn(x_, p);
        s[0] += (double)g_ * (double)G;
        s[1] += reg_sq(G);
        return p;
    }
    __device__ __forceinline__ void at(int64_t i, double (&s)[NS]) const { xp[i] = one(x[i], g[i], s); }
    __device__ __forceinline__ void at4(int64_t i, double (&s)[NS]) const
    {
        const float4 a = *(const float4 *)(x + i), b = *(const float4 *)(g + i);
        float4 p;
        p.x = one(a.x, b.x, s); p.y = one(a.y, b.y, s); p.z = one(a.z, b.z, s); p.w = one(a.w, b.w, s);
        *(float4 *)(xp + i) = p;
    }
};

struct OpProxL1Mom {         // v = x1 + c (x1 - x0); out = soft(v - a g, al); s0 += (gt - out)^2          regularized.py:374-375,383
    float *out; const float *x0, *x1, *g, *gt; float c, a, al;     // out may alias x0 (read before written)
    static constexpr int NS = 1;
    __device__ __forceinline__ float one(float p0, float p1, float g_) const
    {
        const float v = __fadd_rn(p1, reg_mul(c, __fsub_rn(p1, p0)));
        return reg_soft(__fsub_rn(v, reg_mul(a, g_)), al);
    }
    __device__ __forceinline__ void at(int64_t i, double (&s)[NS]) const
    {
        const float o = one(x0[i], x1[i], g[i]);
        const float e = gt ? __fsub_rn(gt[i], o) : 0.f;
        out[i] = o;
        if (gt) s[0] += reg_sq(e);
    }
    __device__ __forceinline__ void at4(int64_t i, double (&s)[NS]) const
    {
        const float4 p = *(const float4 *)(x0 + i), q = *(const float4 *)(x1 + i), r = *(const float4 *)(g + i);
        const float4 o = make_float4(one(p.x, q.x, r.x), one(p.y, q.y, r.y), one(p.z, q.z, r.z), one(p.w, q.w, r.w));
        if (gt) {
            const float4 t = *(const float4 *)(gt + i);
            s[0] += reg_sq(__fsub_rn(t.x, o.x)) + reg_sq(__fsub_rn(t.y, o.y)) + reg_sq(__fsub_rn(t.z, o.z)) + reg_sq(__fsub_rn(t.w, o.w));
        }
        *(float4 *)(out + i) = o;
    }
};

struct OpResidual {          // out = +-(ax - b) (out optional, may alias ax); s0 += out^2                regularized.py:85-86,267,324
    float *out; const float *ax, *b; int neg;
    static constexpr int NS = 1;
    __device__ __forceinline__ float one(float p, float q) const { const float d = __fsub_rn(p, q); return neg ? -d : d; }
    __device__ __forceinline__ void at(int64_t i, double (&s)[NS]) const
    {
        const float o = one(ax[i], b[i]);
        if (out) out[i] = o;
        s[0] += reg_sq(o);
    }
    __device__ __forceinline__ void at4(int64_t i, double (&s)[NS]) const
    {
        const float4 p = *(const float4 *)(ax + i), q = *(const float4 *)(b + i);
        const float4 o = make_float4(one(p.x, q.x), one(p.y, q.y), one(p.z, q.z), one(p.w, q.w));
        if (out) *(float4 *)(out + i) = o;
        s[0] += reg_sq(o.x) + reg_sq(o.y) + reg_sq(o.z) + reg_sq(o.w);
    }
};

// [0, head) scalar, [head, head + 4 n4) in float4, [head + 4 n4, n) scalar; every range grid-stride, so a thread's elements and the
// order it adds them in depend on (n, head) only
template <class Op>
__global__ __launch_bounds__(REG_BLOCK) void k_reg(Op op, int64_t n, int64_t head, int64_t n4, double *part)
{
    double s[Op::NS];
#pragma unroll
    for (int k = 0; k < Op::NS; ++k) s[k] = 0.0;
    const int64_t tid = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * REG_BLOCK;
    for (int64_t i = tid; i < head; i += stride) op.at(i, s);
    for (int64_t j = tid; j < n4; j += stride) op.at4(head + 4 * j, s);
    for (int64_t i = head + 4 * n4 + tid; i < n; i += stride) op.at(i, s);
    reg_block_partials<Op::NS>(s, part);
}

static inline int64_t reg_misalign(const void *p) { return p ? (int64_t)(((uintptr_t)p >> 2) & 3) : -1; }

// one streaming pass of `op` over n elements + the deterministic sum of its NS scalars into d_acc[slot ..]
template <class Op>
static int reg_launch(tomo_ctx *ctx, const char *name, const Op &op, int64_t n, int slot, std::initializer_list<const void *> ptrs)
{
    if (slot < 0 || slot + Op::NS > TOMO_N_ACC) return tomo_fail(ctx, TOMO_ERR_ARG, std::string(name) + ": bad accumulator slot");
    int rc = tomo_acc_zero(ctx, 0, 0);             // makes sure the accumulators exist (and sets the context's device)
    if (rc) return rc;
    if (n == 0) return TOMO_OK;
    // float4 body only if every operand sits at the same offset from a 16-byte boundary
    int64_t mis = -1;
    bool same = true;
    for (const void *p : ptrs) {
        if (!p) continue;
        const int64_t m = reg_misalign(p);
        if ((uintptr_t)p & 3) same = false;
        if (mis < 0) mis = m;
        else if (m != mis) same = false;
    }
    int64_t head = n, n4 = 0;
    if (same && mis >= 0) {
        head = std::min<int64_t>(n, (4 - mis) & 3);
        n4 = (n - head) / 4;
    }
    const int64_t work = n4 + (n - 4 * n4 + 3) / 4;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((work + REG_BLOCK - 1) / REG_BLOCK, REG_MAX_GRID));
    rc = tomo_ensure_red_part(ctx, (size_t)REG_MAX_NS * REG_MAX_GRID);
    if (rc) return rc;
    TOMO_LAUNCH(ctx, name, k_reg<Op>, dim3(grid), dim3(REG_BLOCK), 0, op, n, head, n4, ctx->d_red_part);
    TOMO_LAUNCH(ctx, "k_reg_final", k_reg_final, dim3(1), dim3(REG_BLOCK), 0, (const double *)ctx->d_red_part, grid, Op::NS, ctx->d_acc + slot, 0);
    return TOMO_OK;
}

#define REG_ARGS(ctx, cond, name)                                                        \
    do {                                                                                 \
        if (!(ctx)) return tomo_fail(nullptr, TOMO_ERR_ARG, "null ctx");                 \
        if (n < 0 || (n > 0 && !(cond))) return tomo_fail((ctx), TOMO_ERR_ARG, name ": bad args"); \
    } while (0)

extern "C" int tomo_vec_fista_momentum(tomo_ctx *ctx, float *d_rec, const float *d_u, const float *d_u_old, const float *d_gt, int64_t n, float c, int slot)
{
    REG_ARGS(ctx, d_rec && d_u && d_u_old, "tomo_vec_fista_momentum");
    OpFistaMom op{d_rec, d_u, d_u_old, d_gt, c};
    return reg_launch(ctx, "k_reg_fista_momentum", op, n, slot, {d_rec, d_u, d_u_old, d_gt});
}

extern "C" int tomo_vec_tikh_grad(tomo_ctx *ctx, float *d_bp, const float *d_rec, int64_t n, float lambda, int slot)
{
    REG_ARGS(ctx, d_bp && d_rec, "tomo_vec_tikh_grad");
    OpTikhGrad op{d_bp, d_rec, lambda};
    return reg_launch(ctx, "k_reg_tikh_grad", op, n, slot, {d_bp, d_rec});
}

extern "C" int tomo_vec_trial(tomo_ctx *ctx, float *d_out, const float *d_x, const float *d_d, int64_t n, float a, int slot)
{
    REG_ARGS(ctx, d_out && d_x && d_d, "tomo_vec_trial");
    OpTrial op{d_out, d_x, d_d, a};
    return reg_launch(ctx, "k_reg_trial", op, n, slot, {d_out, d_x, d_d});
}

extern "C" int tomo_vec_clamp_err(tomo_ctx *ctx, float *d_rec, const float *d_gt, int64_t n, int positivity, int slot)
{
    REG_ARGS(ctx, d_rec, "tomo_vec_clamp_err");
    if (!positivity && !d_gt) {                       // nothing to write, nothing to sum: only the argument checks
        if (slot < 0 || slot >= TOMO_N_ACC) return tomo_fail(ctx, TOMO_ERR_ARG, "tomo_vec_clamp_err: bad accumulator slot");
        return TOMO_OK;
    }
    OpClampErr op{d_rec, d_gt, positivity ? 1 : 0};
    return reg_launch(ctx, "k_reg_clamp_err", op, n, slot, {d_rec, d_gt});
}

extern "C" int tomo_vec_prox_l1_trial(tomo_ctx *ctx, float *d_xp, const float *d_x, const float *d_g, int64_t n, float t, float t_lambda, int slot)
{
    REG_ARGS(ctx, d_xp && d_x && d_g, "tomo_vec_prox_l1_trial");
    OpProxL1Trial op{d_xp, d_x, d_g, t, t_lambda};
    return reg_launch(ctx, "k_reg_prox_l1_trial", op, n, slot, {d_xp, d_x, d_g});
}

extern "C" int tomo_vec_prox_l1_momentum(tomo_ctx *ctx, float *d_out, const float *d_x0, const float *d_x1, const float *d_g, const float *d_gt, int64_t n,
                                         float c, float a, float a_lambda, int slot)
{
    REG_ARGS(ctx, d_out && d_x0 && d_x1 && d_g, "tomo_vec_prox_l1_momentum");
    OpProxL1Mom op{d_out, d_x0, d_x1, d_g, d_gt, c, a, a_lambda};
    return reg_launch(ctx, "k_reg_prox_l1_momentum", op, n, slot, {d_out, d_x0, d_x1, d_g, d_gt});
}

extern "C" int tomo_vec_residual_acc(tomo_ctx *ctx, float *d_out, const float *d_ax, const float *d_b, int64_t n, int negate, int slot)
{
    REG_ARGS(ctx, d_ax && d_b, "tomo_vec_residual_acc");
    OpResidual op{d_out, d_ax, d_b, negate ? 1 : 0};
    return reg_launch(ctx, "k_reg_residual", op, n, slot, {d_out, d_ax, d_b});
}

// ---- tomo_tv_prox_det: tomo_tv_denoise_fista with deterministic dual-gap sums.  The dual-field updates are the same kernels; the
// gap check's three sums and the isotropic TV norm are taken by a fixed grid over the voxels in linear order (block partials in
// d_red_part, then k_reg_final), instead of atomics per (z chunk, y, x) block -- so the gap, and with it the stop, is a function of the
// input bits alone.
__global__ __launch_bounds__(REG_BLOCK) void k_tv_gap_det(const float *__restrict__ px, const float *__restrict__ py, const float *__restrict__ pz,
                                                          const float *__restrict__ im, float *__restrict__ out, TvDims d, float weight, double *part)
{
    double s[3] = {0.0, 0.0, 0.0};
    const int64_t n = (int64_t)d.nx * d.sx, stride = (int64_t)gridDim.x * REG_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x; i < n; i += stride) {
        const int ix = (int)(i / d.sx), iy = (int)((i - (int64_t)ix * d.sx) / d.sy), iz = (int)(i - (int64_t)ix * d.sx - (int64_t)iy * d.sy);
        const float gap = reg_mul(weight, tv_div_at(px, py, pz, i, ix, iy, iz, d));
        const float v = im[i], nw = __fsub_rn(v, gap);
        out[i] = nw;
        s[0] += (double)gap * gap; s[1] += (double)nw * nw; s[2] += (double)v * v;
    }
    reg_block_partials<3>(s, part);
}

__global__ __launch_bounds__(REG_BLOCK) void k_tv_iso_det(const float *__restrict__ x, TvDims d, double *part)
{
    double s[1] = {0.0};
    const int64_t n = (int64_t)d.nx * d.sx, stride = (int64_t)gridDim.x * REG_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x; i < n; i += stride) {
        const int ix = (int)(i / d.sx), iy = (int)((i - (int64_t)ix * d.sx) / d.sy), iz = (int)(i - (int64_t)ix * d.sx - (int64_t)iy * d.sy);
        const float v = x[i];
        const float gx = ix < d.nx - 1 ? x[i + d.sx] - v : 0.f, gy = iy < d.ny - 1 ? x[i + d.sy] - v : 0.f, gz = iz < d.nz - 1 ? x[i + 1] - v : 0.f;
        s[0] += (double)__fsqrt_rn(__fadd_rn(__fadd_rn(reg_mul(gx, gx), reg_mul(gy, gy)), reg_mul(gz, gz)));
    }
    reg_block_partials<1>(s, part);
}

extern "C" int tomo_tv_prox_det(tomo_ctx *ctx, const float *d_im, float *d_out, int nx, int ny, int nz, double weight, int niter, double eps,
                                int check_gap_frequency, int *h_iters, double *h_dual_gap)
{
    if (!ctx || !d_im || !d_out || niter < 0 || check_gap_frequency < 1 || !(weight > 0.0)) return tomo_fail(ctx, TOMO_ERR_ARG, "tomo_tv_prox_det: bad args");
    TvDims d;
    dim3 grid;
    int rc = tv_dims(ctx, nx, ny, nz, d, grid);
    if (rc) return rc;
    rc = tomo_ensure_red(ctx, 8);
    if (rc) return rc;
    rc = tomo_ensure_red_part(ctx, (size_t)REG_MAX_NS * REG_MAX_GRID);
    if (rc) return rc;
    const size_t n = (size_t)nx * ny * nz;
    const int rgrid = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)n + REG_BLOCK - 1) / REG_BLOCK, REG_MAX_GRID));
    TOMO_HIP(ctx, hipSetDevice(ctx->device));
    rc = tomo_ensure_ws(ctx, 7 * n);
    if (rc) return rc;
    float *ws = ctx->d_ws;
    float *ax = ws, *ay = ws + n, *az = ws + 2 * n, *px = ws + 3 * n, *py = ws + 4 * n, *pz = ws + 5 * n, *err = ws + 6 * n;
    double dgap = 0.0;
    int i = 0;
    if (h_iters) *h_iters = 0;
    if (h_dual_gap) *h_dual_gap = 0.0;
    TOMO_HIP(ctx, hipMemsetAsync(ws, 0, 6 * n * sizeof(float), ctx->stream));
    TOMO_HIP(ctx, hipMemcpyAsync(d_out, d_im, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    const float w = (float)weight, c = (float)(1.0 / (12.0 * weight));
    double t = 1.0;
    while (i < niter) {
        TOMO_LAUNCH(ctx, "k_tv_error", k_tv_error, grid, dim3(256), 0, (const float *)ax, (const float *)ay, (const float *)az, d_im, err, d, w);
        const double t_new = 0.5 * (1.0 + sqrt(1.0 + 4.0 * t * t)), t_factor = (t - 1.0) / t_new;
        TOMO_LAUNCH(ctx, "k_tv_update", k_tv_update, grid, dim3(256), 0, ax, ay, az, px, py, pz, (const float *)err, d, c, (float)(1.0 + t_factor), (float)t_factor);
        t = t_new;
        if (i % check_gap_frequency == 0) {
            TOMO_LAUNCH(ctx, "k_tv_gap_det", k_tv_gap_det, dim3(rgrid), dim3(REG_BLOCK), 0, (const float *)px, (const float *)py, (const float *)pz, d_im, d_out, d, w,
                        ctx->d_red_part);
            TOMO_LAUNCH(ctx, "k_reg_final", k_reg_final, dim3(1), dim3(REG_BLOCK), 0, (const double *)ctx->d_red_part, rgrid, 3, ctx->d_red, 1);
            TOMO_LAUNCH(ctx, "k_tv_iso_det", k_tv_iso_det, dim3(rgrid), dim3(REG_BLOCK), 0, (const float *)d_out, d, ctx->d_red_part);
            TOMO_LAUNCH(ctx, "k_reg_final", k_reg_final, dim3(1), dim3(REG_BLOCK), 0, (const double *)ctx->d_red_part, rgrid, 1, ctx->d_red + 3, 1);
            TOMO_HIP(ctx, hipMemcpyAsync(ctx->h_red, ctx->d_red, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            TOMO_HIP(ctx, hipStreamSynchronize(ctx->stream));
            const double s_gap = ctx->h_red[0], s_new = ctx->h_red[1], im_norm = ctx->h_red[2], tv_new = 2.0 * weight * ctx->h_red[3];
            dgap = im_norm > 0.0 ? 0.5 / im_norm * (s_gap + tv_new - im_norm + s_new) : 0.0;
            if (dgap < eps) break;
        }
        ++i;
    }
    TOMO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_iters) *h_iters = i;
    if (h_dual_gap) *h_dual_gap = dgap;
    return TOMO_OK;
}
