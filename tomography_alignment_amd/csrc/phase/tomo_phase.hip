// libtomo_phase.so: Paganin single-distance phase retrieval of a device-resident stack of transmission frames (include/tomo_phase.h,
// tomography_alignment_amd/preprocess.py) on gfx950.  The transforms are hipFFT's batched 2-D R2C / C2R, in place in one padded buffer;
// everything else is the three streaming kernels below.  A frame of the buffer is Px rows of RS = 2 (Pz/2 + 1) floats, which the R2C
// turns into Px rows of Pz/2 + 1 complex values.  Every kernel is a flat grid over one batch: a thread finds its frame from blockIdx.y
// and its row from one integer division, so short rows (a 48-wide frame) fill a work-group as well as long ones.
//
// k_pad      one thread per float2 of the padded buffer: the two source values are T's at the clamped coordinates (edge replication),
//            read lane-contiguous along z, and the pair is stored with one 8-byte store; the two floats past Pz that the in-place layout
//            adds to every row are written as zeros.  There is no real-valued padded copy beside the FFT buffer.
// k_filter   the half-spectrum times H / (Px Pz).  H is never stored: tx[kx] = Px Pz a (kx / Px)^2 and tz[kz] = Px Pz (1 + a (kz / Pz)^2)
//            come from the host in float64, and the multiplier is 1.0f / float(tx[kx] + tz[kz]), an IEEE float32 division.  A thread
//            owns two neighbouring coefficients as one float4.  Rows are Pz/2 + 1 complex values long, an odd count for most lengths, so
//            every other row starts 8 bytes off a 16-byte boundary: the row's pairs are shifted by one there, and the first and last
//            coefficient of such a row go as single float2.
// k_crop     crop + clamp + -log: a thread reads four values of a row of the window (two float2 where the window's z offset is even, so
//            that they are aligned) and stores one float4 of the output; a scalar form serves rows whose length is not a multiple of 4.
//            The output may be the buffer the pad kernel read: a batch's frames are all padded before any of them is written.
// k_log      -log(fmax(v, min_ratio)) of a flat array, float4 with a scalar tail: minus_log alone, and strength 0.
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../../include/tomo_phase.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_PHASE_ERR_ARG, SIDE_ERR_HIP = TOMO_PHASE_ERR_HIP, SIDE_ERR_NODEV = TOMO_PHASE_ERR_NODEV, SIDE_ERR_FFT = TOMO_PHASE_ERR_FFT;
}
#include "../tomo_side_host.h"
#include "../tomo_side_fft.h"

namespace {

constexpr int TPB = 256;

struct Shape {
    int nx, nz;          // a frame
    int px, pz;          // the padded frame
    int ox, oz;          // where the data sits in it
    int pzh;             // pz / 2 + 1 complex values per row; a row is 2 pzh floats
};

// ---------------------------------------------------------------------------------------------------------------------- kernels

__global__ __launch_bounds__(TPB) void k_pad(const float *__restrict__ T, Shape g, float *__restrict__ buf) {
    const long long per_frame = (long long)g.px * g.pzh;          // float2 of one padded frame
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= per_frame) return;
    const long long f = blockIdx.y;
    const int row = (int)(idx / g.pzh), j = (int)(idx - (long long)row * g.pzh);
    const int ix = min(max(row - g.ox, 0), g.nx - 1);
    const int p0 = 2 * j;
    float2 v = make_float2(0.f, 0.f);
    if (p0 < g.pz) {                                               // pz is even: p0 + 1 < pz as well
        const float *src = T + (f * g.nx + ix) * (long long)g.nz;
        v.x = src[min(max(p0 - g.oz, 0), g.nz - 1)];
        v.y = src[min(max(p0 + 1 - g.oz, 0), g.nz - 1)];
    }
    reinterpret_cast<float2 *>(buf)[f * per_frame + idx] = v;
}

__device__ inline float gain(double tx, double tz) { return 1.0f / (float)(tx + tz); }

__global__ __launch_bounds__(TPB) void k_filter(float2 *__restrict__ spec, Shape g, const double *__restrict__ tx, const double *__restrict__ tz,
                                                int per_row) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= (long long)g.px * per_row) return;
    const long long f = blockIdx.y;
    const int kx = (int)(idx / per_row), t = (int)(idx - (long long)kx * per_row);
    const long long row0 = (f * g.px + kx) * (long long)g.pzh;    // the row's first coefficient
    const int c0 = 2 * t - (int)(row0 & 1);                       // row0 + c0 is even: 16-byte aligned
    const double ax = tx[kx];
    if (c0 >= 0 && c0 + 1 < g.pzh) {
        float4 *p = reinterpret_cast<float4 *>(spec + row0 + c0);
        float4 v = *p;
        const float h0 = gain(ax, tz[c0]), h1 = gain(ax, tz[c0 + 1]);
        v.x *= h0, v.y *= h0, v.z *= h1, v.w *= h1;
        *p = v;
        return;
    }
    for (int c = max(c0, 0); c < min(c0 + 2, g.pzh); ++c) {
        float2 v = spec[row0 + c];
        const float h = gain(ax, tz[c]);
        v.x *= h, v.y *= h;
        spec[row0 + c] = v;
    }
}

__device__ inline float finish(float r, int minus_log, float min_ratio) { return minus_log ? -logf(fmaxf(r, min_ratio)) : r; }

// VW 4: nz % 4 == 0 and out 16-byte aligned.  EVEN: oz is even (the float2 loads are aligned).
template <int VW, bool EVEN>
__global__ __launch_bounds__(TPB) void k_crop(const float *__restrict__ buf, Shape g, int minus_log, float min_ratio, float *__restrict__ out) {
    const int nzv = g.nz / VW;
    const long long per_frame = (long long)g.nx * nzv;
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= per_frame) return;
    const long long f = blockIdx.y;
    const int ix = (int)(idx / nzv), iz = (int)(idx - (long long)ix * nzv) * VW;
    const float *src = buf + ((f * g.px + g.ox + ix) * (long long)(2 * g.pzh) + g.oz + iz);
    if (VW == 4) {
        float4 v;
        if (EVEN) {
            const float2 a = reinterpret_cast<const float2 *>(src)[0], b = reinterpret_cast<const float2 *>(src)[1];
            v = make_float4(a.x, a.y, b.x, b.y);
        } else {
            v = make_float4(src[0], src[1], src[2], src[3]);
        }
        v.x = finish(v.x, minus_log, min_ratio);
        v.y = finish(v.y, minus_log, min_ratio);
        v.z = finish(v.z, minus_log, min_ratio);
        v.w = finish(v.w, minus_log, min_ratio);
        reinterpret_cast<float4 *>(out)[f * per_frame + idx] = v;
    } else {
        out[f * per_frame + idx] = finish(src[0], minus_log, min_ratio);
    }
}

__global__ __launch_bounds__(TPB) void k_log(const float *in, float *out, size_t n4, size_t count, float min_ratio) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i < n4) {
        float4 v = reinterpret_cast<const float4 *>(in)[i];
        v.x = finish(v.x, 1, min_ratio);
        v.y = finish(v.y, 1, min_ratio);
        v.z = finish(v.z, 1, min_ratio);
        v.w = finish(v.w, 1, min_ratio);
        reinterpret_cast<float4 *>(out)[i] = v;
    } else {
        const size_t j = 4 * n4 + (i - n4);
        if (j < count) out[j] = finish(in[j], 1, min_ratio);
    }
}

}  // namespace

struct tomo_phase {
    int device = 0;
    std::string err;
    FftPlans<std::tuple<int, int, int>> plans;   // R2C + C2R per (px, pz, batch)
    Buf work;                    // the hipFFT work area all plans share
    Buf tables;                  // double tx[px], tz[pzh]
    auto bufs() { return std::array{&work, &tables}; }
    std::vector<double> host_tables;
    PassTimer<TOMO_PHASE_MS_N> timer;
};

namespace {

// The smallest even 2^i 3^j 5^k >= want (want >= 1); 0 if there is none up to TOMO_PHASE_MAX_P.
int fast_even(long long want) {
    int best = 0;
    for (long long p5 = 1; p5 <= TOMO_PHASE_MAX_P; p5 *= 5)
        for (long long p3 = p5; p3 <= TOMO_PHASE_MAX_P; p3 *= 3)
            for (long long p = 2 * p3; p <= TOMO_PHASE_MAX_P; p *= 2)
                if (p >= want && (best == 0 || p < best)) best = (int)p;
    return best;
}

int padded(tomo_phase *h, int n, int m, int *out) {
    if (n < 1 || m < 0) return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase: an axis needs n >= 1 values and a pad >= 0");
    const int p = fast_even((long long)n + 2LL * m);
    if (!p)
        return fail(h, TOMO_PHASE_ERR_UNSUPPORTED, "tomo_phase: the padded axis (" + std::to_string(n) + " + 2 x " + std::to_string(m) +
                                                       ") would be longer than " + std::to_string(TOMO_PHASE_MAX_P) + "; nothing was written");
    *out = p;
    return TOMO_PHASE_OK;
}

inline dim3 grid(long long per_frame, int b) { return dim3((unsigned)((per_frame + TPB - 1) / TPB), (unsigned)b); }

int launch_log(tomo_phase *h, hipStream_t st, const float *d_in, float *d_out, size_t count, float min_ratio) {
    const bool v4 = ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 15u) == 0;
    const size_t n4 = v4 ? count / 4 : 0, threads = n4 + (count - 4 * n4);
    const size_t blocks = (threads + TPB - 1) / TPB;
    if (blocks >= (1ull << 31)) return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_minus_log: too many values");
    hipLaunchKernelGGL(k_log, dim3((unsigned)blocks), dim3(TPB), 0, st, d_in, d_out, n4, count, min_ratio);
    HIPCHK(h, hipGetLastError());
    return TOMO_PHASE_OK;
}

// One batch of b frames, enqueued on st.  ms: NULL or the five pass times to add to (synchronises).
int run_batch(tomo_phase *h, hipStream_t st, const Shape &g, const FftPlan *plan, int b, const float *d_in, float *d_out, float *buf, int minus_log,
              float min_ratio, float *ms) {
    const double *tx = static_cast<const double *>(h->tables.p), *tz = tx + g.px;
    const int per_row = (g.pzh + 1) / 2 + 1;
    int e = 0;
    if (ms) CHK(h->timer.mark(h, st, e++));
    hipLaunchKernelGGL(k_pad, grid((long long)g.px * g.pzh, b), dim3(TPB), 0, st, d_in, g, buf);
    HIPCHK(h, hipGetLastError());
    if (ms) CHK(h->timer.mark(h, st, e++));
    CHK(exec_forward(h, *plan, st, h->work.p, buf));
    if (ms) CHK(h->timer.mark(h, st, e++));
    hipLaunchKernelGGL(k_filter, grid((long long)g.px * per_row, b), dim3(TPB), 0, st, (float2 *)buf, g, tx, tz, per_row);
    HIPCHK(h, hipGetLastError());
    if (ms) CHK(h->timer.mark(h, st, e++));
    CHK(exec_inverse(h, *plan, st, h->work.p, buf));
    if (ms) CHK(h->timer.mark(h, st, e++));
    const bool v4 = g.nz % 4 == 0 && (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0;
    const dim3 gr = grid((long long)g.nx * (v4 ? g.nz / 4 : g.nz), b);
    if (v4 && g.oz % 2 == 0)
        hipLaunchKernelGGL((k_crop<4, true>), gr, dim3(TPB), 0, st, (const float *)buf, g, minus_log, min_ratio, d_out);
    else if (v4)
        hipLaunchKernelGGL((k_crop<4, false>), gr, dim3(TPB), 0, st, (const float *)buf, g, minus_log, min_ratio, d_out);
    else
        hipLaunchKernelGGL((k_crop<1, false>), gr, dim3(TPB), 0, st, (const float *)buf, g, minus_log, min_ratio, d_out);
    HIPCHK(h, hipGetLastError());
    if (ms) {
        CHK(h->timer.mark(h, st, e));
        CHK(h->timer.add_elapsed(h, ms, TOMO_PHASE_MS_N));
    }
    return TOMO_PHASE_OK;
}

int retrieve(tomo_phase *h, hipStream_t st, const Shape &g, int n, double a, const float *d_in, float *d_out, int minus_log, float min_ratio,
             size_t budget, float *ms, float **spec) {
    // tables, scaled by Px Pz so that the kernel's quotient carries the transforms' normalisation
    const double N = (double)g.px * (double)g.pz;
    h->host_tables.resize((size_t)g.px + g.pzh);
    for (int k = 0; k < g.px; ++k) {
        const double f = (double)(k <= g.px / 2 ? k : k - g.px) / (double)g.px;
        h->host_tables[k] = N * (a * (f * f));
    }
    for (int k = 0; k < g.pzh; ++k) {
        const double f = (double)k / (double)g.pz;
        h->host_tables[g.px + k] = N * (1.0 + a * (f * f));
    }
    const size_t tb = sizeof(double) * h->host_tables.size();
    CHK(grow(h, h->tables, tb));
    HIPCHK(h, hipMemcpyAsync(h->tables.p, h->host_tables.data(), tb, hipMemcpyHostToDevice, st));

    // the batch and its plans (fit_batch)
    const size_t fb = frame_bytes(g.px, g.pz);
    BatchFit fit;
    CHK(fit_r2c_2d(h, h->plans, g.px, g.pz, n, budget, true, &fit));
    const int b = fit.b;
    // retrieve() waits for the stream before it returns, so nothing of this handle is in flight when the work area is replaced
    CHK(grow(h, h->work, fit.max_work()));
    HIPCHK(h, hipMalloc((void **)spec, (size_t)b * fb));
    const size_t in_frame = (size_t)g.nx * g.nz;
    for (int f0 = 0; f0 < n; f0 += b) {
        const int bb = std::min(b, n - f0);
        CHK(run_batch(h, st, g, bb == b ? fit.plan : fit.tail, bb, d_in + f0 * in_frame, d_out + f0 * in_frame, *spec, minus_log, min_ratio, ms));
    }
    HIPCHK(h, hipStreamSynchronize(st));
    return TOMO_PHASE_OK;
}

}  // namespace

extern "C" {

TOMO_API int tomo_phase_abi_version(void) { return 1; }

TOMO_API int tomo_phase_create(int device, tomo_phase **out) {
    CHK(create_plain(device, true, out));
    if (!(*out)->timer.create()) {
        delete *out;
        *out = nullptr;
        return fail(nullptr, TOMO_PHASE_ERR_HIP, "hipEventCreate failed");
    }
    return TOMO_PHASE_OK;
}

TOMO_API int tomo_phase_destroy(tomo_phase *h) {
    if (!h) return TOMO_PHASE_OK;
    (void)hipSetDevice(h->device);
    h->plans.destroy_all();
    free_bufs(h->bufs());
    h->timer.destroy();
    delete h;
    return TOMO_PHASE_OK;
}

TOMO_API const char *tomo_phase_last_error(tomo_phase *h) { return last_error(h); }

TOMO_API int tomo_phase_padded_length(int n, int m, int *out) {
    if (!out) return fail(nullptr, TOMO_PHASE_ERR_ARG, "tomo_phase_padded_length: NULL");
    return padded(nullptr, n, m, out);
}

TOMO_API int tomo_phase_batch(int n, int px, int pz, size_t max_scratch_bytes, int *batch) {
    if (!batch) return fail(nullptr, TOMO_PHASE_ERR_ARG, "tomo_phase_batch: NULL");
    if (n < 1 || px < 2 || pz < 2 || px > TOMO_PHASE_MAX_P || pz > TOMO_PHASE_MAX_P || pz % 2)
        return fail(nullptr, TOMO_PHASE_ERR_ARG, "tomo_phase_batch: bad shape");
    *batch = batch_for(n, frame_bytes(px, pz), max_scratch_bytes, frame_bytes(px, pz));
    return TOMO_PHASE_OK;
}

TOMO_API int tomo_phase_device_bytes(tomo_phase *h, int64_t *bytes) {
    if (!h || !bytes) return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_device_bytes: NULL");
    *bytes = (int64_t)buf_bytes(h->bufs());
    return TOMO_PHASE_OK;
}

TOMO_API int tomo_phase_mem_info(tomo_phase *h, size_t *free_bytes, size_t *total_bytes) {
    if (!h || !free_bytes || !total_bytes) return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_mem_info: NULL");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemGetInfo(free_bytes, total_bytes));
    return TOMO_PHASE_OK;
}

TOMO_API int tomo_phase_plan_seconds(tomo_phase *h, double *seconds) {
    if (!h || !seconds) return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_plan_seconds: NULL");
    *seconds = h->plans.seconds;
    return TOMO_PHASE_OK;
}

TOMO_API int tomo_phase_minus_log(tomo_phase *h, void *stream, const float *d_in, float *d_out, size_t count, float min_ratio) {
    if (!h) return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_minus_log: NULL handle");
    if (!(min_ratio > 0.f) || !std::isfinite(min_ratio)) return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_minus_log: min_ratio must be finite and > 0");
    if (count == 0) return TOMO_PHASE_OK;
    if (!d_in || !d_out) return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_minus_log: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    return launch_log(h, reinterpret_cast<hipStream_t>(stream), d_in, d_out, count, min_ratio);
}

TOMO_API int tomo_phase_retrieve(tomo_phase *h, void *stream, const float *d_in, float *d_out, int n, int nx, int nz, double strength,
                                 int pad_x, int pad_z, int minus_log, float min_ratio, size_t max_scratch_bytes, float *pass_ms) {
    if (!h) return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_retrieve: NULL handle");
    if (n < 1 || nx < 1 || nz < 1) return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_retrieve: bad shape");
    if (!(strength >= 0.0 && strength <= TOMO_PHASE_MAX_STRENGTH))
        return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_retrieve: the strength must be in 0 ... 1e12");
    if (!(min_ratio > 0.f) || !std::isfinite(min_ratio)) return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_retrieve: min_ratio must be finite and > 0");
    if (!d_in || !d_out) return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_retrieve: NULL pointer");
    if ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 3u)
        return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_retrieve: misaligned pointer");
    if (pad_x < 0 || pad_z < 0) return fail(h, TOMO_PHASE_ERR_ARG, "tomo_phase_retrieve: pad must be >= 0");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (pass_ms)
        for (int p = 0; p < TOMO_PHASE_MS_N; ++p) pass_ms[p] = 0.f;
    const size_t count = (size_t)n * nx * nz;
    if (strength == 0.0) {                        // the identity: nothing is padded or transformed, so no limit on the axes applies
        HIPCHK(h, hipSetDevice(h->device));
        if (minus_log) return launch_log(h, st, d_in, d_out, count, min_ratio);
        if (d_out != d_in) HIPCHK(h, hipMemcpyAsync(d_out, d_in, sizeof(float) * count, hipMemcpyDeviceToDevice, st));
        return TOMO_PHASE_OK;
    }
    Shape g{};
    g.nx = nx, g.nz = nz;
    CHK(padded(h, nx, pad_x, &g.px));
    CHK(padded(h, nz, pad_z, &g.pz));
    g.ox = (g.px - nx) / 2, g.oz = (g.pz - nz) / 2, g.pzh = g.pz / 2 + 1;
    HIPCHK(h, hipSetDevice(h->device));
    float *spec = nullptr;
    const int rc = retrieve(h, st, g, n, strength, d_in, d_out, minus_log ? 1 : 0, min_ratio, max_scratch_bytes, pass_ms, &spec);
    if (spec) {
        if (rc) (void)hipStreamSynchronize(st);   // nothing may still be using the buffer
        const hipError_t e = hipFree(spec);
        if (!rc && e != hipSuccess) return fail(h, TOMO_PHASE_ERR_HIP, std::string("hipFree of the spectrum: ") + hipGetErrorString(e));
    }
    return rc;
}

}  // extern "C"
