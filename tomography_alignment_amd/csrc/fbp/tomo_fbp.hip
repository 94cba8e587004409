// libtomo_fbp.so: the ramp filter of filtered back-projection (tomography_alignment_amd/recon/fbp.py) on gfx950.
//
// One work-group filters C = 2 S detector columns (S complex signals) of one projection: it loads the ndx rows of its C columns
// (contiguous z segments, so the loads coalesce), packs columns 2s and 2s+1 into the real and imaginary parts of signal s, zero-pads
// to Npad, and runs a Stockham FFT in LDS (one radix-2 or radix-4 pass, then radix-8 passes), multiplies by the real, even response H
// (times scale[ip] / Npad), and runs the inverse FFT.  Because H is real and even, the real and imaginary parts of the result are
// exactly the two filtered columns: no real-to-complex post-processing.  Each work-group owns its columns entirely, so the output may
// alias the input.
//
// LDS layout: signal s at float2 offset s * SP, element i at i + (i >> 3) -- one float2 of padding every 8 keeps the stride-R stores
// of the early passes (and the stride-8 groups of the second) off shared banks -- and SP odd, so that the columns of one row (the
// scalar stores of the load phase) spread over the banks.  Every thread holds E = 16 (8 at Npad 8192) complex values per pass (read all, barrier,
// write all, barrier), so one buffer suffices.  Twiddles: a float2 table of exp(-2 pi i m / Npad) computed on the host in double.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../../include/tomo_fbp.h"

namespace {
constexpr int SIDE_ERR_ARG = TOMO_FBP_ERR_ARG, SIDE_ERR_HIP = TOMO_FBP_ERR_HIP, SIDE_ERR_NODEV = TOMO_FBP_ERR_NODEV;
}
#include "../tomo_side_host.h"

#ifndef TOMO_FBP_LDS_KIB
#define TOMO_FBP_LDS_KIB 64     // LDS of the complex data per work-group (before padding): 64 -> two work-groups per CU
#endif

namespace {

constexpr double PI = 3.141592653589793238462643383279502884;
constexpr int MIN_LOGN = 6;                      // Npad 64 .. 8192 (launch<6..13>)

template <int LOGN>
struct Cfg {
    static constexpr int N = 1 << LOGN;
    static constexpr int S = ((TOMO_FBP_LDS_KIB * 1024 / 8) >> LOGN) > 0 ? ((TOMO_FBP_LDS_KIB * 1024 / 8) >> LOGN) : 1;
    static constexpr int C = 2 * S;                               // detector columns per work-group
    static constexpr int E0 = LOGN >= 13 ? 8 : 16;                // complex values per thread per pass (8 at Npad 8192: 16 spill there),
    static constexpr int E = (S * N / 1024) > E0 ? (S * N / 1024) : E0;   // more where 1024 threads would not cover the work-group
    static constexpr int T = (S * N / E) < 64 ? 64 : (S * N / E);  // threads
    static constexpr int SP = N + N / 8 + 1;                      // float2 stride of a signal
    static constexpr size_t LDS = (size_t)S * SP * sizeof(float2);
};

__device__ __forceinline__ int pad(int i) { return i + (i >> 3); }

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// multiply by -i (forward) or +i (inverse)
template <bool INV>
__device__ __forceinline__ float2 rot(float2 a) { return INV ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x); }

template <bool INV>
__device__ __forceinline__ void dft2(float2 &a0, float2 &a1) {
    float2 t = a0;
    a0 = cadd(t, a1);
    a1 = csub(t, a1);
}

template <bool INV>
__device__ __forceinline__ void dft4(float2 &a0, float2 &a1, float2 &a2, float2 &a3) {
    float2 s02 = cadd(a0, a2), d02 = csub(a0, a2), s13 = cadd(a1, a3), d13 = rot<INV>(csub(a1, a3));
    a0 = cadd(s02, s13);
    a2 = csub(s02, s13);
    a1 = cadd(d02, d13);
    a3 = csub(d02, d13);
}

template <bool INV>
__device__ __forceinline__ void dft8(float2 *a) {
    constexpr float H = 0.70710678118654752440f;
    dft4<INV>(a[0], a[2], a[4], a[6]);       // evens: E0..E3 in a0, a2, a4, a6
    dft4<INV>(a[1], a[3], a[5], a[7]);       // odds:  O0..O3 in a1, a3, a5, a7
    float2 o1 = INV ? make_float2(H * (a[3].x - a[3].y), H * (a[3].x + a[3].y)) : make_float2(H * (a[3].x + a[3].y), H * (a[3].y - a[3].x));
    float2 o2 = rot<INV>(a[5]);
    float2 o3 = INV ? make_float2(-H * (a[7].x + a[7].y), H * (a[7].x - a[7].y)) : make_float2(H * (a[7].y - a[7].x), -H * (a[7].x + a[7].y));
    float2 e0 = a[0], e1 = a[2], e2 = a[4], e3 = a[6], o0 = a[1];
    a[0] = cadd(e0, o0);
    a[4] = csub(e0, o0);
    a[1] = cadd(e1, o1);
    a[5] = csub(e1, o1);
    a[2] = cadd(e2, o2);
    a[6] = csub(e2, o2);
    a[3] = cadd(e3, o3);
    a[7] = csub(e3, o3);
}

template <int R, bool INV>
__device__ __forceinline__ void dft(float2 *a) {
    if constexpr (R == 8) dft8<INV>(a);
    else if constexpr (R == 4) dft4<INV>(a[0], a[1], a[2], a[3]);
    else dft2<INV>(a[0], a[1]);
}

// One Stockham pass of radix R after sub-transforms of length Ns = 2^NSLOG (Bainville's formulation): butterfly j of a signal reads
// elements j + r N/R, multiplies by w^(k r), k = j mod Ns, w = exp(-+2 pi i / (Ns R)), runs a DFT_R and writes (j - k) R + k + r Ns.
// SCALE (the first inverse pass): the inputs are first multiplied by H[min(i, N - i)] * f.
template <int LOGN, int R, int NSLOG, bool INV, bool SCALE>
__device__ __forceinline__ void pass(float2 *lds, const float2 *__restrict__ tw, const float *__restrict__ H, float f) {
    using K = Cfg<LOGN>;
    constexpr int N = K::N, NB = N / R, PER = K::S * NB / K::T;
    constexpr int RLOG = R == 8 ? 3 : (R == 4 ? 2 : 1);
    constexpr int TWSHIFT = LOGN - NSLOG - RLOG;
    static_assert(PER >= 1 && PER * K::T == K::S * NB, "butterflies must divide evenly over the threads");
    float2 v[PER][R];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int b = threadIdx.x + i * K::T;
        const int s = b / NB, j = b % NB;
        const float2 *sig = lds + s * K::SP;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            v[i][r] = sig[pad(j + r * NB)];
            if constexpr (SCALE) {
                const int idx = j + r * NB;
                const float g = H[idx <= N / 2 ? idx : N - idx] * f;
                v[i][r].x *= g;
                v[i][r].y *= g;
            }
        }
        if constexpr (NSLOG > 0) {
            const int k = j & ((1 << NSLOG) - 1);
            // w^r: radix 8 loads w, w^2, w^4 and forms the rest with one or two products (keeps the live addresses and VGPRs down)
            float2 w[R];
            if constexpr (R == 8) {
                w[1] = tw[k << TWSHIFT];
                w[2] = tw[(2 * k) << TWSHIFT];
                w[4] = tw[(4 * k) << TWSHIFT];
                w[3] = cmul(w[1], w[2]);
                w[5] = cmul(w[1], w[4]);
                w[6] = cmul(w[2], w[4]);
                w[7] = cmul(w[3], w[4]);
            } else {
#pragma unroll
                for (int r = 1; r < R; ++r) w[r] = tw[(k * r) << TWSHIFT];
            }
#pragma unroll
            for (int r = 1; r < R; ++r) {
                if (INV) w[r].y = -w[r].y;
                v[i][r] = cmul(v[i][r], w[r]);
            }
        }
        dft<R, INV>(v[i]);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int b = threadIdx.x + i * K::T;
        const int s = b / NB, j = b % NB;
        const int k = j & ((1 << NSLOG) - 1);
        float2 *sig = lds + s * K::SP;
        const int base = (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) sig[pad(base + r * (1 << NSLOG))] = v[i][r];
    }
    __syncthreads();
}

// The whole transform: one radix-2 or radix-4 pass first when log2 N is not a multiple of 3 (at Ns = 1 it needs no twiddles), then
// radix-8 passes.
template <int LOGN, int NSLOG, bool INV, bool FIRST>
__device__ __forceinline__ void fft(float2 *lds, const float2 *tw, const float *H, float f) {
    if constexpr (NSLOG < LOGN) {
        constexpr int R = (NSLOG == 0 && LOGN % 3 == 1) ? 2 : ((NSLOG == 0 && LOGN % 3 == 2) ? 4 : 8);
        constexpr int RLOG = R == 8 ? 3 : (R == 4 ? 2 : 1);
        pass<LOGN, R, NSLOG, INV, INV && FIRST>(lds, tw, H, f);
        fft<LOGN, NSLOG + RLOG, INV, false>(lds, tw, H, f);
    }
}

// grid: n_chunks * n_proj work-groups, chunk fastest.  scale[ip] / N is folded into the response on the way into the inverse FFT.
// 4 waves per SIMD (<= 128 VGPRs): two 512-thread work-groups (or one of 1024) per CU.
template <int LOGN>
__global__ __launch_bounds__(Cfg<LOGN>::T) __attribute__((amdgpu_waves_per_eu(4))) void k_ramp_filter(const float *in, float *out, int ndx, int ndz, int n_chunks,
                                                              const float2 *__restrict__ tw, const float *__restrict__ H,
                                                              const float *__restrict__ scale) {
    using K = Cfg<LOGN>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *lds = reinterpret_cast<float2 *>(smem);
    float *ldsf = reinterpret_cast<float *>(smem);
    const int chunk = (int)(blockIdx.x % (unsigned)n_chunks);
    const int ip = (int)(blockIdx.x / (unsigned)n_chunks);
    const int z0 = chunk * K::C;
    const size_t base = (size_t)ip * (size_t)ndx * (size_t)ndz;      // 64-bit: a 1024^3 sinogram has 2^30 values
    // load: rows ix < ndx of columns z0 .. z0 + C - 1 (missing columns and the padding rows are zero)
    for (int e = threadIdx.x; e < K::C * K::N; e += K::T) {
        const int c = e % K::C, ix = e / K::C, z = z0 + c;
        float val = 0.f;
        if (ix < ndx && z < ndz) val = in[base + (size_t)ix * ndz + z];
        ldsf[2 * ((c >> 1) * K::SP + pad(ix)) + (c & 1)] = val;
    }
    __syncthreads();
    fft<LOGN, 0, false, true>(lds, tw, H, 0.f);
    fft<LOGN, 0, true, true>(lds, tw, H, scale[ip] * (1.0f / K::N));
    // store: the real part of signal s is column 2s, the imaginary part column 2s + 1
    for (int e = threadIdx.x; e < K::C * ndx; e += K::T) {
        const int c = e % K::C, ix = e / K::C, z = z0 + c;
        if (z < ndz) out[base + (size_t)ix * ndz + z] = ldsf[2 * ((c >> 1) * K::SP + pad(ix)) + (c & 1)];
    }
}

}  // namespace

struct tomo_fbp {
    int device = 0;
    std::string err;
    int ndx = 0, logn = 0;                    // the response set, and its FFT length
    float2 *d_tw = nullptr;                   // twiddles of the current length (2^logn)
    float *d_H = nullptr;                     // response, 2^(logn-1) + 1 values
    float *d_scale = nullptr;                 // per-projection scales
    int scale_cap = 0;
    float *h_scale = nullptr;                 // pinned staging of the scales
    hipEvent_t ev_done = nullptr;             // after the last filter launch (its tables and scales may be replaced once it has passed)
    bool pending = false;
};

namespace {

int log2_npad(int ndx) {
    int l = MIN_LOGN;
    while ((1 << l) < 2 * ndx) ++l;
    return l;
}

int drain(tomo_fbp *h) {
    if (h->pending) {
        HIPCHK(h, hipEventSynchronize(h->ev_done));
        h->pending = false;
    }
    return TOMO_FBP_OK;
}

template <int LOGN>
int launch(tomo_fbp *h, hipStream_t st, const float *in, float *out, int n_proj, int ndx, int ndz) {
    using K = Cfg<LOGN>;
    static bool attr_set = false;
    if (!attr_set) {
        HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ramp_filter<LOGN>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)K::LDS));
        attr_set = true;
    }
    const int n_chunks = (ndz + K::C - 1) / K::C;
    if ((long long)n_chunks * n_proj >= (1LL << 31)) return fail(h, TOMO_FBP_ERR_ARG, "tomo_fbp_filter: too many work-groups");
    hipLaunchKernelGGL(k_ramp_filter<LOGN>, dim3((unsigned)(n_chunks * n_proj)), dim3(K::T), K::LDS, st, in, out, ndx, ndz, n_chunks,
                       h->d_tw, h->d_H, h->d_scale);
    HIPCHK(h, hipGetLastError());
    return TOMO_FBP_OK;
}

}  // namespace

extern "C" {

TOMO_API int tomo_fbp_abi_version(void) { return 1; }

TOMO_API int tomo_fbp_create(int device, tomo_fbp **out) {
    CHK(check_create(device, out));
    tomo_fbp *h = new tomo_fbp();
    h->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming);
    if (e != hipSuccess) {
        tomo_fbp_destroy(h);
        return fail(nullptr, TOMO_FBP_ERR_HIP, std::string("event creation: ") + hipGetErrorString(e));
    }
    *out = h;
    return TOMO_FBP_OK;
}

TOMO_API int tomo_fbp_destroy(tomo_fbp *h) {
    if (!h) return TOMO_FBP_OK;
    (void)hipSetDevice(h->device);
    if (h->pending) (void)hipEventSynchronize(h->ev_done);
    if (h->d_tw) (void)hipFree(h->d_tw);
    if (h->d_H) (void)hipFree(h->d_H);
    if (h->d_scale) (void)hipFree(h->d_scale);
    if (h->h_scale) (void)hipHostFree(h->h_scale);
    if (h->ev_done) (void)hipEventDestroy(h->ev_done);
    delete h;
    return TOMO_FBP_OK;
}

TOMO_API const char *tomo_fbp_last_error(tomo_fbp *h) { return last_error(h); }

TOMO_API int tomo_fbp_set_response(tomo_fbp *h, int ndx, const double *table) {
    if (!h || !table) return fail(h, TOMO_FBP_ERR_ARG, "tomo_fbp_set_response: NULL");
    if (ndx < 1) return fail(h, TOMO_FBP_ERR_ARG, "tomo_fbp_set_response: ndx must be >= 1");
    if (ndx > TOMO_FBP_MAX_NDX)
        return fail(h, TOMO_FBP_ERR_UNSUPPORTED, "tomo_fbp_set_response: ndx " + std::to_string(ndx) + " > " +
                                                     std::to_string(TOMO_FBP_MAX_NDX) + " (Npad > 8192 does not fit in LDS)");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = drain(h);
    if (rc) return rc;
    const int logn = log2_npad(ndx), N = 1 << logn;
    if (logn != h->logn) {
        std::vector<float2> tw(N);
        for (int m = 0; m < N; ++m) {
            const double a = -2.0 * PI * (double)m / (double)N;
            tw[m] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
        if (h->d_tw) HIPCHK(h, hipFree(h->d_tw));
        if (h->d_H) HIPCHK(h, hipFree(h->d_H));
        h->d_tw = nullptr;
        h->d_H = nullptr;
        h->logn = h->ndx = 0;
        HIPCHK(h, hipMalloc(&h->d_tw, N * sizeof(float2)));
        HIPCHK(h, hipMalloc(&h->d_H, (N / 2 + 1) * sizeof(float)));
        HIPCHK(h, hipMemcpy(h->d_tw, tw.data(), N * sizeof(float2), hipMemcpyHostToDevice));
        h->logn = logn;
    }
    std::vector<float> Hf(N / 2 + 1);
    for (int j = 0; j <= N / 2; ++j) Hf[j] = (float)table[j];
    HIPCHK(h, hipMemcpy(h->d_H, Hf.data(), Hf.size() * sizeof(float), hipMemcpyHostToDevice));
    h->ndx = ndx;
    return TOMO_FBP_OK;
}

TOMO_API int tomo_fbp_filter(tomo_fbp *h, void *stream, const float *d_in, float *d_out, int n_proj, int ndx, int ndz,
                             const double *h_scale) {
    if (!h) return fail(h, TOMO_FBP_ERR_ARG, "tomo_fbp_filter: NULL handle");
    if (ndx > TOMO_FBP_MAX_NDX)
        return fail(h, TOMO_FBP_ERR_UNSUPPORTED, "tomo_fbp_filter: ndx " + std::to_string(ndx) + " > " + std::to_string(TOMO_FBP_MAX_NDX) +
                                                     " (Npad > 8192 does not fit in LDS); nothing was written");
    if (n_proj < 0 || ndx < 1 || ndz < 1) return fail(h, TOMO_FBP_ERR_ARG, "tomo_fbp_filter: bad shape");
    if (n_proj == 0) return TOMO_FBP_OK;
    if (!d_in || !d_out || !h_scale) return fail(h, TOMO_FBP_ERR_ARG, "tomo_fbp_filter: NULL pointer");
    if (ndx != h->ndx)
        return fail(h, TOMO_FBP_ERR_ARG, "tomo_fbp_filter: no response set for ndx " + std::to_string(ndx) +
                                             " (tomo_fbp_set_response first; the handle holds ndx " + std::to_string(h->ndx) + ")");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int rc = drain(h);          // the previous call's scales are still being read until its kernel has passed
    if (rc) return rc;
    if (n_proj > h->scale_cap) {
        if (h->d_scale) HIPCHK(h, hipFree(h->d_scale));
        if (h->h_scale) HIPCHK(h, hipHostFree(h->h_scale));
        h->d_scale = nullptr;
        h->h_scale = nullptr;
        h->scale_cap = 0;
        HIPCHK(h, hipMalloc(&h->d_scale, (size_t)n_proj * sizeof(float)));
        HIPCHK(h, hipHostMalloc(&h->h_scale, (size_t)n_proj * sizeof(float)));
        h->scale_cap = n_proj;
    }
    for (int i = 0; i < n_proj; ++i) h->h_scale[i] = (float)h_scale[i];
    HIPCHK(h, hipMemcpyAsync(h->d_scale, h->h_scale, (size_t)n_proj * sizeof(float), hipMemcpyHostToDevice, st));
    switch (h->logn) {
        case 6: rc = launch<6>(h, st, d_in, d_out, n_proj, ndx, ndz); break;
        case 7: rc = launch<7>(h, st, d_in, d_out, n_proj, ndx, ndz); break;
        case 8: rc = launch<8>(h, st, d_in, d_out, n_proj, ndx, ndz); break;
        case 9: rc = launch<9>(h, st, d_in, d_out, n_proj, ndx, ndz); break;
        case 10: rc = launch<10>(h, st, d_in, d_out, n_proj, ndx, ndz); break;
        case 11: rc = launch<11>(h, st, d_in, d_out, n_proj, ndx, ndz); break;
        case 12: rc = launch<12>(h, st, d_in, d_out, n_proj, ndx, ndz); break;
        case 13: rc = launch<13>(h, st, d_in, d_out, n_proj, ndx, ndz); break;
        default: return fail(h, TOMO_FBP_ERR_ARG, "tomo_fbp_filter: no response set");
    }
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(h->ev_done, st));
    h->pending = true;
    return TOMO_FBP_OK;
}

}  // extern "C"
