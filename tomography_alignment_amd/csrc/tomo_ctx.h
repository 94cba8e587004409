// tomo_ctx.h -- internal context shared by the translation units of libtomo_hip.so
#ifndef TOMO_CTX_H_
#define TOMO_CTX_H_
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <deque>
#include <map>
#include <string>
#include <vector>

#include "../../include/tomo.h"
#include "tomo_raycore.h"

struct BpC {   // voxel-driven back-projector constants of one projection: the reference's three float32 rotation matrices and
               // the translation (src/external_back_projection.f90:17-25, src/rotations_module.f90:6-54)
    float rp[3][3], ra[3][3], rb[3][3];   // Rz(phi), Rx(alpha), Ry(beta)
    float t[3];
};

struct ProfRec { int64_t n = 0; double ms = 0.0; };
struct ProfPending { std::string name; hipEvent_t e0, e1; };

// What stage_tile_consts (tomo_project.hip) staged last for the tile kernels, kept while the same poses come again and nobody else has
// used the staging buffers -- the x-slab calls of one pipelined back-projection, forward + back-projection of a solver iteration, every
// iteration of a solver (a re-stage drains the stream: the GPU would idle between slab kernels).  The staging buffer holds, from offset
// 0: the AdjC array [gather-eligible flat ..., other flat ..., general ...]; at gf_off one GfC per gather-eligible projection; at fg_off
// the gather forward's projection lists (indices into the GfC array): [x walk NW 3 | x walk NW 4 | y walk NW 3 | y walk NW 4], each in
// pose order, fg_n[] entries each.
struct TilePlan {
    bool valid = false;                 // the staging buffers still hold what this plan describes (tomo_ensure_stage clears it)
    bool ok = false;                    // the tile kernels take these poses (a pose set they decline is never kept: valid implies ok)
    std::vector<double> poses;          // key: the poses ...
    int opts = 0;                       // ... and the options "tile_flat" (bit 0) and "adj_flat_gather" (bit 1) it was staged under
    double weight_bound = 2.0;          // bound of the tent weights a voxel collects from one projection (fixed-point scale of the LDS adjoints)
    int n_flat = 0, n_gather = 0;       // untilted projections, and how many of them are gather-eligible
    double eb_max = 0.0;                // largest |m10| + |m11| of the gather-eligible projections (picks NJ)
    int zc_lo = 0, zc_hi = 0;           // range of the gather-eligible projections' integer z offsets (GfC::zc)
    double ea_max = 0.0;                // largest |m00| + |m01| of the gather-eligible projections, and whether all of them have tau == 0:
    bool tau_zero = true;               // what the direct-to-LDS adjoint (option "adj_gather_dma") asks of a plan
    size_t gf_off = 0, fg_off = 0;      // byte offsets into the staging buffer
    int fg_n[4] = {0, 0, 0, 0};
    bool fg_ok = false;                 // every gather-eligible projection also meets the gather forward's bounds
};

// Key of the sinogram plane flags cached in d_blk: everything the cached words depend on -- the sinogram and its shape (layout of the
// flags and their prefix counts), and the volume height and the poses' integer z offsets the chunk shift was computed from.
struct ZfKey {
    const void *src = nullptr;
    int nproj = 0, ndz = 0, ndx = 0, nz = 0, zc_lo = 0, zc_hi = 0;
    bool operator==(const ZfKey &o) const
    {
        return src == o.src && nproj == o.nproj && ndz == o.ndz && ndx == o.ndx && nz == o.nz && zc_lo == o.zc_lo && zc_hi == o.zc_hi;
    }
};

struct tomo_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool has_geom = false;
    TomoGeomC g{};
    double vox_pitch[3] = {1, 1, 1};
    // padded scratch volume (zero halo) and its state
    float *d_volpad = nullptr;
    size_t volpad_elems = 0;
    size_t volpad_rows = 0;             // nx * ny the row scratch behind the padded copy was sized for
    bool halo_dirty = true;
    bool wide_rows = false;             // TOMO_GEOM_WIDE_ROWS: padded x-row pitch >= 2^23 bytes, detector-z pitch or sample step > 1 voxel -- the 24-bit-multiply / fixed-bias kernels are not used
    const void *staged_src = nullptr;   // device pointer whose contents the padded copy currently holds
    int reuse_staged = 0;               // caller vouches: contents of staged_src unchanged since it was staged
    // per-projection constants (pinned host staging + device)
    void *h_stage = nullptr;
    void *d_stage = nullptr;
    size_t stage_bytes = 0;
    // the tile kernels' constants staged last (stage_tile_consts)
    TilePlan plan;
    // reduction scratch
    double *d_red = nullptr;
    double *h_red = nullptr;
    size_t red_cap = 0;     // doubles
    // measurement hook: synthetic copy traffic beside the asynchronous collectives (tomo_ctx.hip: comm_async)
    int comm_test_copy_eighths = 0, comm_test_copy_wgs = 0;
    void *d_comm_scratch = nullptr;
    size_t comm_scratch_bytes = 0;
    // work-group partial sums of the fused cost / gradient kernels (tomo_cost_grad_rows: added in a fixed order, no atomics); grow-only,
    // handed back by tomo_release_workspace
    double *d_red_part = nullptr;
    size_t red_part_cap = 0;     // doubles
    // TOMO_N_ACC double accumulators (tomo_acc_zero / tomo_vec_dot_acc / tomo_acc_fetch) + their pinned host mirror
    double *d_acc = nullptr;
    double *h_acc = nullptr;
    // block buffer (grow-only).  A forward call keeps its live lists here (LiveList), a back-projection the plane flags of its sinogram
    // (BlkHead) and the general kernel's live list behind them
    int *d_blk = nullptr;
    size_t blk_ints = 0;
    int reuse_sino_flags = 0;           // option: the caller vouches the sinogram of the previous back-projection call is unchanged
    ZfKey zf_key;                       // what the plane flags in d_blk were computed for; src == nullptr: d_blk holds none
    bool zf_has_cum = false, zf_has_shift = false;      // ... with their prefix counts / chunk shift
    // true: the flags of zf_key.src were recorded by the pass that WROTE that sinogram (tomo_vec_residual_scale_flags) and nothing has been
    // launched, copied or reduced on this context since -- the next back-projection of it takes them without the caller's word
    // (reuse_sino_flags) and without its own scan.  Dropped by every launch (TOMO_LAUNCH) and by the copies, fills, frees and collectives
    // that can write a caller's buffer (tomo_ctx.hip): recorded flags serve exactly the call that follows their recording.
    bool zf_recorded = false;
    // general float workspace (grow-only): the TV-FISTA proximal step keeps its 7 fields here across calls
    float *d_ws = nullptr;
    size_t ws_elems = 0;
    // assembled CSR kept between tomo_csr_assemble and tomo_csr_fetch (tomo_csr.hip)
    void *csr_data = nullptr, *csr_indices = nullptr, *csr_indptr = nullptr;
    int64_t csr_nnz = 0, csr_rows = 0;
    int csr_value_bytes = 4;
    // options
    int fwd_variant = 3;      // 1 ray-driven plain, 2 ray-driven SGPR-base, 3 LDS tile (default)
    int adj_variant = 2;      // 1 global float atomics, 2 LDS tile fixed-point (default)
    int grad_variant = 4;     // 1 plain, 2 eight dword gathers + packed lerps, 3 four gathers + DPP neighbour shift, 4 (default) 2 or 3 per pose by tilt
    int grad_v1_prec = 0;     // diagnostic for grad_variant 1 (per-ray tomo_proj_grad only): bit 0 float64 sample positions, bit 1 float64 lerps and sums
    int tile_flat = 1;      // 1: untilted projections take the flat tile kernels
    int fused_update = 1;     // 1: tomo_adjoint_update folds the SIRT update into the gather adjoint's store when all its poses take that kernel; 0: it always declines (the caller's two calls)
    int adj_flat_gather = 1;  // 1: untilted unit lattices take the gather-form adjoint (k_adj_gather_flat) instead of the LDS-atomic flat kernel
    int adj_gather_dma = 1;   // 1 (default): a gather adjoint with three samples per row, tau == 0 in every pose and |m00| + |m01| < 1.427 loads its sinogram rows straight into LDS (k_adj_gather_flat<3, UPD, 1>); 0: always through registers
    int fwd_gather_patch = 1; // work-group order of k_fwd_gather_flat: 0 plain (group, row tile) order, 1 (default) XCD patches from FWD_PATCH_MIN patches up, 2 patches at any size
    int fwd_flat_gather = 1;  // 1 (default): whole-volume forward calls ALL of whose poses take the gather adjoint (three samples per row) take the gather-form forward (k_fwd_gather_flat: no atomics, same bits every run); other calls, and 0: the flat forward below
    int fwd_flat_ztiles = 2;  // 2 (default): the flat forward of a volume of two or more z tiles runs over blocks of two z-adjacent 64-plane images, live blocks only (k_fwd_flat_tab); 1, and volumes of one z tile: one tile per work-group (k_tile_flat<true>)
    // timing / profiling
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool profile_on = false;
    std::map<std::string, ProfRec> prof;
    std::vector<ProfPending> pending;
    std::vector<hipEvent_t> ev_pool;
    // comm
    ncclComm_t comm = nullptr;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_compute = nullptr, ev_comm = nullptr;
    bool comm_pending = false;
    std::deque<hipEvent_t> comm_done;    // one event per asynchronous all-reduce / reduce-scatter the compute stream has not yet waited for (issue order)
    std::deque<hipEvent_t> comm_done_g;  // ... and per asynchronous all-gather
    int comm_test_poison_us = 0;         // test hook, see comm_async
    std::vector<hipEvent_t> comm_ev_pool;
    int n_ranks = 1, rank = 0;
    std::string err;
};

int tomo_fail(tomo_ctx *ctx, int code, const std::string &msg);

// roctx ranges around the C-ABI's projector / gradient / collective entry points (the reference has print timings only).  Off by
// default and without a link-time dependency: TOMO_ROCTX=1 in the environment, or tomo_set_option(ctx, "roctx", 1), dlopens
// librocprofiler-sdk-roctx.so (rocprofv3 --marker-trace) -- or libroctx64.so -- on first use; the ranges are named after the entry points.
struct TomoRange {
    bool on;
    explicit TomoRange(const char *name);
    ~TomoRange();
    TomoRange(const TomoRange &) = delete;
    TomoRange &operator=(const TomoRange &) = delete;
};
int tomo_roctx_enable(int on);      // 0 ok, -1: no roctx library could be loaded
int tomo_ensure_stage(tomo_ctx *ctx, size_t bytes);
int tomo_ensure_red(tomo_ctx *ctx, size_t n_doubles);
int tomo_ensure_red_part(tomo_ctx *ctx, size_t n_doubles);
int tomo_ensure_ws(tomo_ctx *ctx, size_t n_floats);
int tomo_ensure_blk(tomo_ctx *ctx, size_t n_ints);
// Head of d_blk during a back-projection: one flag byte per detector-z plane of the sinogram (ndz bytes, padded to ints), their ndz + 1
// prefix counts, the z chunk shift (one int).  tomo_blk_head makes d_blk hold the head and `extra_ints` behind it.
struct BlkHead {
    unsigned char *zf;
    int *zcum, *zshift;
    size_t ints;
};
static inline int tomo_blk_head(tomo_ctx *ctx, size_t extra_ints, BlkHead *h)
{
    const size_t zf_ints = ((size_t)ctx->g.ndz + 3) / 4;
    h->ints = zf_ints + (size_t)ctx->g.ndz + 2;
    const int rc = tomo_ensure_blk(ctx, h->ints + extra_ints);
    if (rc) return rc;
    h->zf = (unsigned char *)ctx->d_blk;
    h->zcum = ctx->d_blk + zf_ints;
    h->zshift = h->zcum + ctx->g.ndz + 1;
    return TOMO_OK;
}
// A live list of n blocks (or tiles) at int offset `at` of d_blk: list[0] = number of live blocks, list[1 ..] their ids in launch order,
// then one flag byte per block.
struct LiveList {
    int *list;
    unsigned char *flags;
    static size_t ints(size_t n) { return 1 + n + (n + 3) / 4; }
    LiveList(int *d_blk, size_t at, size_t n) : list(d_blk + at), flags((unsigned char *)(list + 1 + n)) {}
};
// the passes and the cache key that go with freshly written sinogram plane flags (tomo_project.hip)
int tomo_record_zflags(tomo_ctx *ctx, const void *d_proj, int n_proj, bool want_cum, bool want_shift, const BlkHead &head, const char *prof_name,
                       bool recorded);
void tomo_csr_release(tomo_ctx *ctx);
void tomo_prof_begin(tomo_ctx *ctx, const char *name);
void tomo_prof_end(tomo_ctx *ctx);
void tomo_prof_begin_on(tomo_ctx *ctx, const char *name, hipStream_t stream);
void tomo_prof_end_on(tomo_ctx *ctx, hipStream_t stream);

#define TOMO_HIP(ctx, call)                                                                         \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return tomo_fail((ctx), TOMO_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define TOMO_NEED_GEOM(ctx)                                                              \
    do {                                                                                 \
        if (!(ctx)) return tomo_fail(nullptr, TOMO_ERR_ARG, "null ctx");                 \
        if (!(ctx)->has_geom) return tomo_fail((ctx), TOMO_ERR_STATE, "geometry not set"); \
        {   /* the current device is per THREAD: a caller's helper thread starts on device 0 */                     \
            hipError_t e_ = hipSetDevice((ctx)->device);                                                         \
            if (e_ != hipSuccess) return tomo_fail((ctx), TOMO_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e_)); \
        }                                                                                                        \
    } while (0)

// launch with optional event bracketing (tomo_profile_enable) and launch-error check
#define TOMO_LAUNCH(ctx, name, kern, grid, block, shmem, ...)                                   \
    do {                                                                                        \
        (ctx)->zf_recorded = false;                                                             \
        tomo_prof_begin((ctx), (name));                                                         \
        hipLaunchKernelGGL(kern, (grid), (block), (shmem), (ctx)->stream, __VA_ARGS__);         \
        tomo_prof_end((ctx));                                                                   \
        TOMO_HIP((ctx), hipGetLastError());                                                     \
    } while (0)

#endif
