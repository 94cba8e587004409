// libtomo_cor.so: the Fourier-space sinogram metric for the position of the rotation axis (include/tomo_cor.h,
// tomography_alignment_amd/rotation_axis.py) on gfx950.  The transform is hipFFT's batched in-place 2-D R2C; everything else is the
// kernels below.  A stacked sinogram M_t of the batch buffer is R = 2 n rows of RS = 2 (nx/2 + 1) floats, which the R2C turns into R
// rows of H = nx/2 + 1 complex values.
//
// k_gather     one thread per (angle, column): its nslices values p[angle][column][rows[s]] lie within one or a few cache lines (z is
//              the fastest axis of p, so the read of ONE detector row is strided by nz whatever the mapping); the stores to
//              S[s][angle][column] are lane-contiguous along the column.
// k_prefilter  the float64 cubic B-spline coefficients of every flipped row, mirror boundary.  The recursion is sequential along a
//              row, so a lane owns a row; a work-group is one wave and owns PR rows, which it moves through LDS in tiles of PR x TW:
//              the tile is loaded with the lanes along the columns (256 contiguous bytes per row and instruction), each of the first
//              PR lanes runs its row's TW steps out of LDS, and the tile is stored with the lanes along the columns again.  The
//              causal pass walks the tiles left to right, the anticausal pass right to left over the coefficients just written.
// k_build      one thread per float2 of the batch buffer.  The S half is a copy; the B half is the exact copy at integer t, the
//              four-tap float64 spline value rounded once otherwise, and comp on the wrapped columns.  Rows start 8-byte aligned
//              (RS is even), so every store is one aligned float2; the floats past nx of a row are zeros.
// k_reduce     sum W |F| of one pair: a wave per row, lanes along ku (contiguous float2 loads), float64 per-lane sums, a fixed
//              shuffle tree, the four waves added in order through LDS, one partial per work-group.  k_final adds a pair's partials
//              in index order.  The grid depends on (R, batch) only; no atomics.  W comes from a table of R ints (the last column
//              that counts in a row), never stored at full size.
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../../include/tomo_cor.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_COR_ERR_ARG, SIDE_ERR_HIP = TOMO_COR_ERR_HIP, SIDE_ERR_NODEV = TOMO_COR_ERR_NODEV, SIDE_ERR_FFT = TOMO_COR_ERR_FFT;
}
#include "../tomo_side_host.h"
#include "../tomo_side_fft.h"

namespace {

constexpr int TPB = 256;
constexpr int PR = 16, TW = 64;                    // k_prefilter: rows of a work-group, columns of a tile
constexpr int HORIZON = 128;                       // terms of the causal start: |pole|^128 = 5e-74
constexpr int RPB = 16;                            // k_reduce: rows of the spectrum per work-group
constexpr double POLE = -0.26794919243112270647;   // sqrt(3) - 2

struct Shape {
    int n, nx, ns;      // angles, columns, slices
    int R, H;           // 2 n rows of the stack; nx/2 + 1 complex values per row (a row is 2 H floats)
};

// ---------------------------------------------------------------------------------------------------------------------- kernels

__global__ __launch_bounds__(TPB) void k_gather(const float *__restrict__ p, int nx, int nz, int first, int n, const int *__restrict__ rows,
                                                int ns, float *__restrict__ S) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long per = (long long)n * nx;
    if (idx >= per) return;
    const float *src = p + ((long long)first * nx + idx) * nz;       // (first + i) nx + j = first nx + idx
    for (int s = 0; s < ns; ++s) S[s * per + idx] = src[rows[s]];
}

__global__ __launch_bounds__(64) void k_prefilter(const float *__restrict__ S, int nx, long long total, double *coef) {
    __shared__ float tin[PR][TW + 1];
    __shared__ double tout[PR][TW + 1];
    const int lane = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * PR;
    const long long row = row0 + lane;
    const bool active = lane < PR && row < total;
    const double z = POLE;
    double prev = 0.0, cn1 = 0.0, cn2 = 0.0;
    if (active) {                                   // the start of the causal recursion: the mirrored row summed with the pole's powers
        const float *src = S + row * nx + (nx - 1);                  // flip: v[i] = 6 src[-i]
        const double zn = pow(z, (double)(nx - 1));
        double c0 = 6.0 * (double)src[0] + zn * (6.0 * (double)src[-(nx - 1)]);
        double zi = z;
        const int last = min(nx - 2, HORIZON);
        for (int i = 1; i <= last; ++i) {
            c0 += zi * (6.0 * (double)src[-i] + zn * (6.0 * (double)src[-(nx - 1 - i)]));
            zi *= z;
        }
        prev = c0 / (1.0 - zn * zn);
    }
    for (int c0 = 0; c0 < nx; c0 += TW) {           // causal, left to right
        const int w = min(TW, nx - c0);
        for (int rr = 0; rr < PR; ++rr)
            if (row0 + rr < total && lane < w) tin[rr][lane] = S[(row0 + rr) * nx + (nx - 1 - (c0 + lane))];
        __syncthreads();
        if (active)
            for (int c = 0; c < w; ++c) {
                const double cur = (c0 + c == 0) ? prev : 6.0 * (double)tin[lane][c] + z * prev;
                tout[lane][c] = cur;
                cn2 = prev, cn1 = cur, prev = cur;
            }
        __syncthreads();
        for (int rr = 0; rr < PR; ++rr)
            if (row0 + rr < total && lane < w) coef[(row0 + rr) * nx + c0 + lane] = tout[rr][lane];
        __syncthreads();
    }
    // cn1 = c[nx - 1], cn2 = c[nx - 2] of the causal pass (nx >= 16)
    const double end = (z * cn2 + cn1) * z / (z * z - 1.0);
    double next = 0.0;
    for (int c0 = ((nx - 1) / TW) * TW; c0 >= 0; c0 -= TW) {      // anticausal, right to left, over what this work-group wrote
        const int w = min(TW, nx - c0);
        for (int rr = 0; rr < PR; ++rr)
            if (row0 + rr < total && lane < w) tout[rr][lane] = coef[(row0 + rr) * nx + c0 + lane];
        __syncthreads();
        if (active)
            for (int c = w - 1; c >= 0; --c) {
                const double cur = (c0 + c == nx - 1) ? end : z * (next - tout[lane][c]);
                tout[lane][c] = cur;
                next = cur;
            }
        __syncthreads();
        for (int rr = 0; rr < PR; ++rr)
            if (row0 + rr < total && lane < w) coef[(row0 + rr) * nx + c0 + lane] = tout[rr][lane];
        __syncthreads();
    }
}

// B_t[i][j] of slice data Ss (S of the slice) and cs (its coefficients); 0 <= i < n, 0 <= j < nx.
__device__ inline float b_value(const float *__restrict__ Ss, const double *__restrict__ cs, int n, int nx, int i, int j, double t, double tfloor,
                                double tceil) {
    const bool wrapped = t >= 0.0 ? (double)j < tceil : (double)j >= (double)nx + tfloor;
    if (wrapped) return Ss[(long long)(n - 1 - i) * nx + j];
    if (t == tfloor) {
        const int c = min(max(j - (int)tfloor, 0), nx - 1);           // in range where not wrapped; the clamp guards the address
        return Ss[(long long)i * nx + (nx - 1 - c)];
    }
    const double x = (double)j - t;
    const double fk = floor(x);
    const int k = (int)fk;
    const double f = x - fk, g = 1.0 - f;
    const double w1 = (f * f * (f - 2.0) * 3.0 + 4.0) / 6.0;
    const double w2 = (g * g * (g - 2.0) * 3.0 + 4.0) / 6.0;
    const double w0 = g * g * g / 6.0;
    const double w3 = 1.0 - w0 - w1 - w2;
    const double w[4] = {w0, w1, w2, w3};
    const double *c = cs + (long long)i * nx;
    double acc = 0.0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        int q = k - 1 + d;
        q = q < 0 ? -q : q;
        q = q > nx - 1 ? 2 * (nx - 1) - q : q;
        q = min(max(q, 0), nx - 1);
        acc += w[d] * c[q];
    }
    return (float)acc;
}

__global__ __launch_bounds__(TPB) void k_build(const float *__restrict__ S, const double *__restrict__ coef, Shape g, const int *__restrict__ slice,
                                               const double *__restrict__ ts, float *__restrict__ buf) {
    const long long per = (long long)g.R * g.H;                       // float2 of one stacked sinogram
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= per) return;
    const int pair = blockIdx.y;
    const int r = (int)(idx / g.H), q = (int)(idx - (long long)r * g.H);
    const long long off = (long long)slice[pair] * g.n * g.nx;
    const float *Ss = S + off;
    float v[2] = {0.f, 0.f};
    if (r < g.n) {
#pragma unroll
        for (int e = 0; e < 2; ++e)
            if (2 * q + e < g.nx) v[e] = Ss[(long long)r * g.nx + 2 * q + e];
    } else {
        const double t = ts[pair], tf = floor(t), tc = ceil(t);
#pragma unroll
        for (int e = 0; e < 2; ++e)
            if (2 * q + e < g.nx) v[e] = b_value(Ss, coef + off, g.n, g.nx, r - g.n, 2 * q + e, t, tf, tc);
    }
    reinterpret_cast<float2 *>(buf)[pair * per + idx] = make_float2(v[0], v[1]);
}

__global__ __launch_bounds__(TPB) void k_reduce(const float2 *__restrict__ spec, Shape g, const int *__restrict__ hi, int nblk,
                                                double *__restrict__ partial) {
    __shared__ double sw[TPB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pair = blockIdx.y;
    const int rend = min(g.R, ((int)blockIdx.x + 1) * RPB);
    const bool even = (g.nx % 2) == 0;
    double acc = 0.0;
    for (int r = blockIdx.x * RPB + wave; r < rend; r += TPB / 64) {
        const int last = min(hi[r], g.H - 1);
        const float2 *row = spec + ((long long)pair * g.R + r) * g.H;
        for (int ku = 2 + lane; ku <= last; ku += 64) {
            const float2 c = row[ku];
            const double a = sqrt((double)c.x * (double)c.x + (double)c.y * (double)c.y);
            acc += (even && ku == g.H - 1) ? a : 2.0 * a;
        }
    }
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_down(acc, s, 64);
    if (lane == 0) sw[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(long long)pair * nblk + blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

__global__ __launch_bounds__(64) void k_final(const double *__restrict__ partial, int nblk, int b, double denom, double *__restrict__ m) {
    const int pair = blockIdx.x * 64 + threadIdx.x;
    if (pair >= b) return;
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += partial[(long long)pair * nblk + k];
    m[pair] = s / denom;
}

}  // namespace

struct tomo_cor {
    int device = 0;
    std::string err;
    Shape g{};                   // of the last load; n = 0 before it
    FftPlans<std::tuple<int, int, int>> plans;   // R2C per (R, nx, batch)
    Buf work;                    // the hipFFT work area all plans share
    Buf S, coef, rows;           // float S[ns][n][nx], double coef[ns][n][nx], int rows[ns]
    Buf spec;                    // the batch buffer
    Buf pairs;                   // double t[npairs], then int slice[npairs]
    Buf tab;                     // int hi[R]
    Buf part, dm;                // double partial[batch][nblk], double m[npairs]
    auto bufs() { return std::array{&work, &S, &coef, &rows, &spec, &pairs, &tab, &part, &dm}; }
    std::vector<int> host_rows, host_tab;
    std::vector<unsigned char> host_pairs;
    PassTimer<TOMO_COR_METRIC_MS_N> timer;       // of a load's passes as well
    static_assert(TOMO_COR_LOAD_MS_N <= TOMO_COR_METRIC_MS_N, "the timer has an event for every mark of a load");
    bool rows_in_flight = false; // a load's copy of host_rows may not have run yet: cleared by every call that waits for the stream
};

namespace {

int check_shape(tomo_cor *h, int n, int nx, int ns) {
    if (n < TOMO_COR_MIN_N || nx < TOMO_COR_MIN_NX || nx > TOMO_COR_MAX_NX || 2LL * n > TOMO_COR_MAX_R || ns < 1 || ns > TOMO_COR_MAX_SLICES)
        return fail(h, TOMO_COR_ERR_UNSUPPORTED,
                    "tomo_cor: " + std::to_string(ns) + " sinograms of " + std::to_string(n) + " x " + std::to_string(nx) + " are outside " +
                        std::to_string(TOMO_COR_MIN_N) + " <= n <= " + std::to_string(TOMO_COR_MAX_R / 2) + ", " + std::to_string(TOMO_COR_MIN_NX) +
                        " <= nx <= " + std::to_string(TOMO_COR_MAX_NX) + ", 1 ... " + std::to_string(TOMO_COR_MAX_SLICES) + " slices; nothing was launched");
    return TOMO_COR_OK;
}

// hi[r], r < R = 2 n.  The operations in the order tests/cor_model.py's wedge() has them.
void wedge(int n, int nx, double ratio, int drop, int *hi) {
    const int R = 2 * n;
    const double dv = ((double)R - 1.0) / (2.0 * M_PI * (double)R);
    const double du = 1.0 / (double)nx;
    const double radius = 0.5 * ratio * (double)nx;
    const double den = radius * du;
    const int cut = std::min(drop, (int)std::ceil(0.05 * (double)R));
    for (int r = 0; r < R; ++r) {
        const int akv = r <= R / 2 ? r : R - r;
        const double num = (double)akv * dv;
        const double w = std::ceil(num / den);
        hi[r] = akv > cut ? (int)std::min(w, (double)(nx / 2)) : 0;
    }
}

inline dim3 grid(long long per, int b) { return dim3((unsigned)((per + TPB - 1) / TPB), (unsigned)b); }

int launch_build(tomo_cor *h, hipStream_t st, int b, const int *d_slice, const double *d_t, float *buf) {
    const Shape &g = h->g;
    hipLaunchKernelGGL(k_build, grid((long long)g.R * g.H, b), dim3(TPB), 0, st, (const float *)h->S.p, (const double *)h->coef.p, g, d_slice, d_t,
                       buf);
    HIPCHK(h, hipGetLastError());
    return TOMO_COR_OK;
}

// Pairs p0 .. p0 + b - 1, enqueued on st.  ms: NULL or the three pass times to add to (synchronises).
int run_batch(tomo_cor *h, hipStream_t st, const FftPlan *plan, int p0, int b, int npairs, float *ms) {
    const Shape &g = h->g;
    const double *d_t = static_cast<const double *>(h->pairs.p) + p0;
    const int *d_slice = reinterpret_cast<const int *>(static_cast<const double *>(h->pairs.p) + npairs) + p0;
    float *buf = static_cast<float *>(h->spec.p);
    const int nblk = (g.R + RPB - 1) / RPB;
    int e = 0;
    if (ms) CHK(h->timer.mark(h, st, e++));
    CHK(launch_build(h, st, b, d_slice, d_t, buf));
    if (ms) CHK(h->timer.mark(h, st, e++));
    CHK(exec_forward(h, *plan, st, h->work.p, buf));
    if (ms) CHK(h->timer.mark(h, st, e++));
    hipLaunchKernelGGL(k_reduce, dim3((unsigned)nblk, (unsigned)b), dim3(TPB), 0, st, (const float2 *)buf, g, (const int *)h->tab.p, nblk,
                       (double *)h->part.p);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_final, dim3((unsigned)((b + 63) / 64)), dim3(64), 0, st, (const double *)h->part.p, nblk, b, (double)g.R * (double)g.nx,
                       static_cast<double *>(h->dm.p) + p0);
    HIPCHK(h, hipGetLastError());
    if (ms) {
        CHK(h->timer.mark(h, st, e));
        CHK(h->timer.add_elapsed(h, ms, TOMO_COR_METRIC_MS_N));
    }
    return TOMO_COR_OK;
}

int loaded(tomo_cor *h, const char *who) {
    if (!h) return fail(h, TOMO_COR_ERR_ARG, std::string(who) + ": NULL handle");
    if (h->g.n == 0) return fail(h, TOMO_COR_ERR_ARG, std::string(who) + ": no sinogram is loaded (tomo_cor_load)");
    return TOMO_COR_OK;
}

}  // namespace

extern "C" {

TOMO_API int tomo_cor_abi_version(void) { return 1; }

TOMO_API int tomo_cor_create(int device, tomo_cor **out) {
    CHK(create_plain(device, true, out));
    if (!(*out)->timer.create()) {
        delete *out;
        *out = nullptr;
        return fail(nullptr, TOMO_COR_ERR_HIP, "hipEventCreate failed");
    }
    return TOMO_COR_OK;
}

TOMO_API int tomo_cor_destroy(tomo_cor *h) {
    if (!h) return TOMO_COR_OK;
    (void)hipSetDevice(h->device);
    h->plans.destroy_all();
    free_bufs(h->bufs());
    h->timer.destroy();
    delete h;
    return TOMO_COR_OK;
}

TOMO_API const char *tomo_cor_last_error(tomo_cor *h) { return last_error(h); }

TOMO_API int tomo_cor_check_shape(int n, int nx, int nslices) { return check_shape(nullptr, n, nx, nslices); }

TOMO_API int tomo_cor_wedge(int n, int nx, double ratio, int drop, int *hi) {
    if (!hi) return fail(nullptr, TOMO_COR_ERR_ARG, "tomo_cor_wedge: NULL");
    CHK(check_shape(nullptr, n, nx, 1));
    if (!(ratio > 0.0) || !std::isfinite(ratio) || drop < 0) return fail(nullptr, TOMO_COR_ERR_ARG, "tomo_cor_wedge: ratio must be > 0 and drop >= 0");
    wedge(n, nx, ratio, drop, hi);
    return TOMO_COR_OK;
}

TOMO_API int tomo_cor_batch(int npairs, int n, int nx, size_t max_scratch_bytes, int *batch) {
    if (!batch) return fail(nullptr, TOMO_COR_ERR_ARG, "tomo_cor_batch: NULL");
    if (npairs < 1) return fail(nullptr, TOMO_COR_ERR_ARG, "tomo_cor_batch: needs at least one pair");
    CHK(check_shape(nullptr, n, nx, 1));
    *batch = batch_for(npairs, frame_bytes(2 * n, nx), max_scratch_bytes, frame_bytes(2 * n, nx));
    return TOMO_COR_OK;
}

TOMO_API int tomo_cor_device_bytes(tomo_cor *h, int64_t *bytes) {
    if (!h || !bytes) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_device_bytes: NULL");
    *bytes = (int64_t)buf_bytes(h->bufs());
    return TOMO_COR_OK;
}

TOMO_API int tomo_cor_plan_seconds(tomo_cor *h, double *seconds) {
    if (!h || !seconds) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_plan_seconds: NULL");
    *seconds = h->plans.seconds;
    return TOMO_COR_OK;
}

TOMO_API int tomo_cor_load(tomo_cor *h, void *stream, const float *d_p, int n_p, int nx, int nz, int first, int n, const int *rows, int nslices,
                           float *pass_ms) {
    if (!h) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_load: NULL handle");
    if (!d_p || !rows) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_load: NULL pointer");
    if (reinterpret_cast<uintptr_t>(d_p) & 3u) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_load: misaligned pointer");
    if (n_p < 1 || nx < 1 || nz < 1 || nslices < 1 || n < 1) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_load: bad shape");
    if (first < 0 || (long long)first + n > n_p) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_load: the angles first ... first + n - 1 are not in p");
    CHK(check_shape(h, n, nx, nslices));
    for (int s = 0; s < nslices; ++s)
        if (rows[s] < 0 || rows[s] >= nz) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_load: row " + std::to_string(rows[s]) + " is not in 0 ... nz - 1");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    h->g.n = 0;                                    // nothing is loaded until everything below is enqueued
    const size_t count = (size_t)nslices * n * nx;
    // a grow frees the old block: hipFree waits for the device, so nothing in flight still uses it
    CHK(grow(h, h->S, sizeof(float) * count));
    CHK(grow(h, h->coef, sizeof(double) * count));
    CHK(grow(h, h->rows, sizeof(int) * (size_t)nslices));
    if (h->rows_in_flight) HIPCHK(h, hipStreamSynchronize(st));     // the staging vector may still feed an earlier load's copy
    h->host_rows.assign(rows, rows + nslices);
    h->rows_in_flight = true;
    HIPCHK(h, hipMemcpyAsync(h->rows.p, h->host_rows.data(), sizeof(int) * (size_t)nslices, hipMemcpyHostToDevice, st));
    if (pass_ms) CHK(h->timer.mark(h, st, 0));
    const long long per = (long long)n * nx;
    hipLaunchKernelGGL(k_gather, dim3((unsigned)((per + TPB - 1) / TPB)), dim3(TPB), 0, st, d_p, nx, nz, first, n, (const int *)h->rows.p, nslices,
                       (float *)h->S.p);
    HIPCHK(h, hipGetLastError());
    if (pass_ms) CHK(h->timer.mark(h, st, 1));
    const long long total = (long long)nslices * n;
    hipLaunchKernelGGL(k_prefilter, dim3((unsigned)((total + PR - 1) / PR)), dim3(64), 0, st, (const float *)h->S.p, nx, total, (double *)h->coef.p);
    HIPCHK(h, hipGetLastError());
    if (pass_ms) {
        CHK(h->timer.mark(h, st, TOMO_COR_LOAD_MS_N));
        for (int p = 0; p < TOMO_COR_LOAD_MS_N; ++p) pass_ms[p] = 0.f;
        CHK(h->timer.add_elapsed(h, pass_ms, TOMO_COR_LOAD_MS_N));
    }
    h->g.n = n, h->g.nx = nx, h->g.ns = nslices, h->g.R = 2 * n, h->g.H = nx / 2 + 1;
    return TOMO_COR_OK;
}

TOMO_API int tomo_cor_metric(tomo_cor *h, void *stream, const int *slice, const double *t, int npairs, double ratio, int drop,
                             size_t max_scratch_bytes, double *m, float *pass_ms) {
    CHK(loaded(h, "tomo_cor_metric"));
    if (!slice || !t || !m) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_metric: NULL pointer");
    if (npairs < 1) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_metric: needs at least one pair");
    if (!(ratio > 0.0) || !std::isfinite(ratio) || drop < 0) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_metric: ratio must be > 0 and drop >= 0");
    const Shape &g = h->g;
    for (int k = 0; k < npairs; ++k) {
        if (slice[k] < 0 || slice[k] >= g.ns) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_metric: slice " + std::to_string(slice[k]) + " is not loaded");
        if (!(std::fabs(t[k]) <= (double)g.nx)) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_metric: a shift must be within +- nx columns");
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    if (pass_ms)
        for (int p = 0; p < TOMO_COR_METRIC_MS_N; ++p) pass_ms[p] = 0.f;

    // the batch and its plans (fit_batch)
    const size_t fb = frame_bytes(g.R, g.nx);
    BatchFit fit;
    CHK(fit_r2c_2d(h, h->plans, g.R, g.nx, npairs, max_scratch_bytes, false, &fit));
    const int b = fit.b;
    // every call that used these buffers waited for the stream before it returned, so nothing in flight uses a block a grow frees
    const int nblk = (g.R + RPB - 1) / RPB;
    CHK(grow(h, h->work, fit.max_work()));
    CHK(grow(h, h->spec, (size_t)b * fb));
    CHK(grow(h, h->part, sizeof(double) * (size_t)b * nblk));
    CHK(grow(h, h->dm, sizeof(double) * (size_t)npairs));
    CHK(grow(h, h->tab, sizeof(int) * (size_t)g.R));
    CHK(grow(h, h->pairs, (sizeof(double) + sizeof(int)) * (size_t)npairs));
    h->host_tab.resize(g.R);
    wedge(g.n, g.nx, ratio, drop, h->host_tab.data());
    h->host_pairs.resize((sizeof(double) + sizeof(int)) * (size_t)npairs);
    std::copy(t, t + npairs, reinterpret_cast<double *>(h->host_pairs.data()));
    std::copy(slice, slice + npairs, reinterpret_cast<int *>(h->host_pairs.data() + sizeof(double) * (size_t)npairs));
    HIPCHK(h, hipMemcpyAsync(h->tab.p, h->host_tab.data(), sizeof(int) * (size_t)g.R, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->pairs.p, h->host_pairs.data(), h->host_pairs.size(), hipMemcpyHostToDevice, st));
    for (int p0 = 0; p0 < npairs; p0 += b) {
        const int bb = std::min(b, npairs - p0);
        CHK(run_batch(h, st, bb == b ? fit.plan : fit.tail, p0, bb, npairs, pass_ms));
    }
    HIPCHK(h, hipMemcpyAsync(m, h->dm.p, sizeof(double) * (size_t)npairs, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->rows_in_flight = false;
    return TOMO_COR_OK;
}

TOMO_API int tomo_cor_debug_build(tomo_cor *h, void *stream, int slice, double t, float *out) {
    CHK(loaded(h, "tomo_cor_debug_build"));
    const Shape &g = h->g;
    if (!out) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_debug_build: NULL pointer");
    if (slice < 0 || slice >= g.ns) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_debug_build: the slice is not loaded");
    if (!(std::fabs(t) <= (double)g.nx)) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_debug_build: a shift must be within +- nx columns");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    CHK(grow(h, h->spec, frame_bytes(g.R, g.nx)));
    CHK(grow(h, h->pairs, sizeof(double) + sizeof(int)));
    h->host_pairs.resize(sizeof(double) + sizeof(int));
    *reinterpret_cast<double *>(h->host_pairs.data()) = t;
    *reinterpret_cast<int *>(h->host_pairs.data() + sizeof(double)) = slice;
    HIPCHK(h, hipMemcpyAsync(h->pairs.p, h->host_pairs.data(), h->host_pairs.size(), hipMemcpyHostToDevice, st));
    CHK(launch_build(h, st, 1, reinterpret_cast<const int *>(static_cast<const double *>(h->pairs.p) + 1), static_cast<const double *>(h->pairs.p),
                     static_cast<float *>(h->spec.p)));
    HIPCHK(h, hipMemcpy2DAsync(out, sizeof(float) * (size_t)g.nx, h->spec.p, sizeof(float) * (size_t)(2 * g.H), sizeof(float) * (size_t)g.nx,
                               (size_t)g.R, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->rows_in_flight = false;
    return TOMO_COR_OK;
}

TOMO_API int tomo_cor_debug_sinogram(tomo_cor *h, void *stream, int slice, float *out) {
    CHK(loaded(h, "tomo_cor_debug_sinogram"));
    const Shape &g = h->g;
    if (!out || slice < 0 || slice >= g.ns) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_debug_sinogram: NULL pointer, or the slice is not loaded");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t per = (size_t)g.n * g.nx;
    HIPCHK(h, hipMemcpyAsync(out, static_cast<const float *>(h->S.p) + slice * per, sizeof(float) * per, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->rows_in_flight = false;
    return TOMO_COR_OK;
}

TOMO_API int tomo_cor_debug_coefficients(tomo_cor *h, void *stream, int slice, double *out) {
    CHK(loaded(h, "tomo_cor_debug_coefficients"));
    const Shape &g = h->g;
    if (!out || slice < 0 || slice >= g.ns) return fail(h, TOMO_COR_ERR_ARG, "tomo_cor_debug_coefficients: NULL pointer, or the slice is not loaded");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t per = (size_t)g.n * g.nx;
    HIPCHK(h, hipMemcpyAsync(out, static_cast<const double *>(h->coef.p) + slice * per, sizeof(double) * per, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->rows_in_flight = false;
    return TOMO_COR_OK;
}

}  // extern "C"
