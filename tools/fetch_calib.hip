// Calibration (development aid): what FETCH_SIZE reports for a KNOWN number of bytes, per access shape.  The project's rule
// "HBM bytes = 2 x FETCH_SIZE KB" (tools/summarise_rocprof.py) was found on wide streaming reads; k_fwd_gather_flat and k_adj_gather_flat load
// one dword per lane, a wave one 256-byte row, rows far apart.  Every kernel below reads each byte of a 2 GiB buffer (8 times the Infinity
// Cache) exactly once:
//   k_stream16   lane = 16 bytes, a wave 1 KiB, consecutive waves consecutive KiB              (the shape the rule was found on)
//   k_rows4      lane = 4 bytes, a wave one 256-byte row per load, through a buffer resource with the row as the scalar offset (the
//                forward's load); the rows of a wave's successive loads lie 64 KiB + 256 B apart (a permutation of all rows)
//   k_rows4_seq  the same loads, rows of a wave consecutive
// Build: hipcc -O3 --offload-arch=gfx950 tools/fetch_calib.hip -o build/fetch_calib
// Run:   rocprofv3 --pmc FETCH_SIZE --output-format csv -d out -o run -- build/fetch_calib     (a counter run of its own, no tracing)
// and set FETCH_SIZE (KB) of each kernel beside the 2 097 152 KB it read.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr size_t BYTES = (size_t)2 << 30;
constexpr unsigned N_ROWS = (unsigned)(BYTES / 256);        // 2^23 rows of 256 bytes
constexpr unsigned ROWS_PER_WAVE = 256;
constexpr unsigned N_WAVES = N_ROWS / ROWS_PER_WAVE;        // 2^15

__global__ __launch_bounds__(256) void k_stream16(const float4 *__restrict__ buf, float *__restrict__ out)
{
    const size_t n16 = BYTES / 16, stride = (size_t)gridDim.x * 256;
    float acc = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) {
        const float4 v = buf[i];
        acc += v.x + v.y + v.z + v.w;
    }
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = acc;
}

template <bool SCATTER> __global__ __launch_bounds__(256) void k_rows4(const float *__restrict__ buf, float *__restrict__ out)
{
    const unsigned lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6);       // grid = N_WAVES / 4 work-groups
    float acc = 0.f;
    // a resource over the quarter of the buffer that holds the wave's rows (a resource addresses < 4 GiB; 512 MiB each here)
    const unsigned quarter = wave / (N_WAVES / 4);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(buf + (size_t)quarter * (BYTES / 16)), 0, (int)(BYTES / 4), 0x00020000);
    const unsigned w = wave % (N_WAVES / 4), rows_q = N_ROWS / 4;
#pragma unroll 8
    for (unsigned i = 0; i < ROWS_PER_WAVE; ++i) {
        const unsigned lin = w * ROWS_PER_WAVE + i;                                // < rows_q
        // SCATTER: lin -> lin * 257 mod rows_q, a permutation (257 is odd, rows_q a power of two): successive rows 257 rows apart
        const unsigned row = SCATTER ? (lin * 257u) & (rows_q - 1) : lin;
        acc += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, lane * 4u, __builtin_amdgcn_readfirstlane(row * 256u), 0));
    }
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = acc;
}

int main()
{
    float *buf, *out;
    CK(hipMalloc(&buf, BYTES));
    CK(hipMemset(buf, 0, BYTES));
    CK(hipMalloc(&out, (size_t)(N_WAVES / 4) * 256 * sizeof(float)));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    float ms;
    for (int rep = 0; rep < 2; ++rep) {
        CK(hipEventRecord(e0));
        k_stream16<<<2048, 256>>>((const float4 *)buf, out);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        printf("k_stream16         read %zu KB in %.3f ms (%.0f GB/s)\n", BYTES / 1024, ms, BYTES / ms / 1e6);
        CK(hipEventRecord(e0));
        k_rows4<true><<<N_WAVES / 4, 256>>>(buf, out);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        printf("k_rows4<scatter>   read %zu KB in %.3f ms (%.0f GB/s)\n", BYTES / 1024, ms, BYTES / ms / 1e6);
        CK(hipEventRecord(e0));
        k_rows4<false><<<N_WAVES / 4, 256>>>(buf, out);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        printf("k_rows4<sequential> read %zu KB in %.3f ms (%.0f GB/s)\n", BYTES / 1024, ms, BYTES / ms / 1e6);
    }
    CK(hipGetLastError());
    CK(hipFree(buf));
    CK(hipFree(out));
    return 0;
}
