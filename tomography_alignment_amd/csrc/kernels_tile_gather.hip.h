// kernels_tile_gather.hip.h -- the GATHER-form adjoint for untilted, coarse enough lattices (k_adj_gather_flat<NJ>): no atomics, each voxel
// written once.  Needs kernels_tile.hip.h (helpers) before it; part of the translation unit tomo_project.hip.

// ------------------------------------------------------------------------------------------------
// GATHER-form adjoint for untilted poses (alpha = beta = 0 and detector-z pitch exactly one voxel: every sample has z = iz + zc + tau;
// any phi, translation, COR shift) whose x-y lattice p = p0 + ix u + j d, with (ix, j) = M ((x, y) - p0), meets the rule of
// stage_tile_consts (tomo_project.hip):
//     |m00| + |m01| = (|cos phi| + |sin phi|) / det_dx < 1.45     three consecutive rows cover a voxel's footprint; a tile touches <= GROWS rows
//     |m10| + |m11| = (|cos phi| + |sin phi|) / step   < 2.99     NJ = 6 consecutive samples of a row cover it (< 1.49: NJ = 3)
// The plain parallel-beam scan (detector pitch = step = voxel) meets it at any phi; so does any coarser detector (tested at pitch 1.25
// and 2), a finer one only near the axes (pitch 0.8: within 10 degrees).  Nothing below assumes more than that rule: positions and
// tents come from the lattice constants.  For such a lattice the adjoint separates:
//     (A^T y)(X, Y, Z) = sum_ix  W(X, Y, ix) * Yz(ix, Z)
//     Yz(ix, Z)   = (1 - tau) y[ix, Z - zc] + tau y[ix, Z - zc - 1]                 (every sample has z = iz + zc + tau)
//     W(X, Y, ix) = sum_{j in [0, n)} tent(px(ix, j) - X) * tent(py(ix, j) - Y)       (tent(r) = 1 - |r| on [-1, 1))
// and W does not depend on Z.  A wave owns 8 x 8 voxel columns x 64 planes with the 64 accumulators of a lane (= column) in
// registers for ALL projections -- no atomics, no fixed-point image, no flush, each voxel written once (a lane finally
// stores its column's 64 consecutive floats):
//   1. lane = COLUMN: the <= 3 detector rows ix and <= 3 samples j per row that can reach the column are enumerated from the
//      column's lattice coordinates; their positions are exact 32.32 fixed point (the forward kernels' lattice), the tents
//      are evaluated from them, summed over j -> W0..W2 and the first row i0, per lane.  This table is the same for every
//      z chunk of the tile: the four waves of a work-group (four z chunks) each compute it for every fourth projection and
//      share it through a triple-buffered LDS table, one barrier per four projections;
//   2. lane = PLANE: the z-lerped sinogram rows the tile can touch (<= 14) are loaded once (coalesced) into wave-private LDS
//      rows (pitch 68 dwords: 16-byte aligned plane quads, lanes reading different rows hit different bank quads) -- through registers,
//      or, where nothing is to be done to them on the way (tau = 0, all planes on the detector), straight into LDS (DMA = 1, below);
//   3. lane = COLUMN again, 64 plane accumulators per lane (statically indexed registers, as plane pairs): per four planes
//      3 ds_read_b128 at row(lane) + immediate plane offset and 6 v_pk_fma_f32 with the lane's own W0..W2 -- no broadcasts, no
//      address arithmetic.
// Same sums as k_tile_flat<false> (which needs 4 ds_add_u32 per sample and lane), regrouped by voxel instead of by sample.
// ------------------------------------------------------------------------------------------------
#define GTX 8
#define GTY 8
#define GROWS 14          // rows a tile can touch: i0 spreads over <= 7 (|m00| + |m01|) <= 10.2 -> 11 values, + 3
#define GPITCH 68          // LDS row pitch in dwords: a multiple of 4, so that a row's plane quads (p .. p+3) are 16-byte aligned for ds_read_b128; rows r, r+1, ...
                           // of one plane quad fall in different bank quads (4 r + p mod 64)
#ifndef GWAVES
#define GWAVES 4
#endif
#ifndef GPX
#define GPX 8              // (x, y) tile patch that one XCD's resident work-groups cover together
#define GPY 12
#endif

// wave_min_i32 / wave_max_i32 (kernels_ray.hip.h) for a wave whose 64 lanes are all active: the lane exchange is written so that it becomes
// the DPP operand of the v_min / v_max itself (every lane of these patterns reads a lane of its own row, so bound_ctrl and the old value
// never apply) -- 4 VALU instructions where the plain form compiles to 12 (a copy and a v_mov_dpp in front of each v_min).
#define G_DPP(V, CTRL) __builtin_amdgcn_update_dpp(0, (V), (CTRL), 0xf, 0xf, true)
__device__ __forceinline__ int gwave_min_i32(int v)
{
    v = min(v, G_DPP(v, 0xB1));         // quad_perm [1,0,3,2]
    v = min(v, G_DPP(v, 0x4E));         // quad_perm [2,3,0,1]
    v = min(v, G_DPP(v, 0x141));        // row_half_mirror
    v = min(v, G_DPP(v, 0x140));        // row_mirror
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ int gwave_max_i32(int v)
{
    v = max(v, G_DPP(v, 0xB1));
    v = max(v, G_DPP(v, 0x4E));
    v = max(v, G_DPP(v, 0x141));
    v = max(v, G_DPP(v, 0x140));
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
#undef G_DPP

struct GfC {
    int64_t fp0x, fp0y, fux, fuy, fdx, fdy;   // x, y of the 32.32 lattice  p = fp0 + ix fu + j fd
    float m00, m01, m10, m11;                 // (ix, j) = M ((x, y) - p0)
    float p0x, p0y, tau;
    int32_t n, zc, slot;
};

// flags[iz] = 1 when ANY value of the sinogram in detector-z plane iz is not zero (all projections, all rows of the call).  Thread = plane
// (coalesced), work-groups stride over the n_rows = n_proj * ndx rows; flags pre-zeroed, benign races (everybody stores 1).
__global__ __launch_bounds__(256) void k_sino_zflags(const float *__restrict__ proj, long long n_rows, int ndz, unsigned char *__restrict__ flags)
{
    const int iz = (int)(blockIdx.x * 256 + threadIdx.x);
    if (iz >= ndz) return;
    bool nz = false;
    for (long long r = blockIdx.y; r < n_rows; r += gridDim.y) nz |= proj[(size_t)r * ndz + iz] != 0.f;
    if (nz) flags[iz] = 1;
}

// cum[i] = number of flagged planes below i, i = 0 .. n (one work-group; the general adjoint asks "any flagged plane in [a, b]?" with two loads)
__global__ __launch_bounds__(1024) void k_zflags_prefix(const unsigned char *__restrict__ flags, int n, int *__restrict__ cum)
{
    __shared__ int wsum[16];
    __shared__ int base;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + (int)threadIdx.x;
        const bool f = i < n && flags[i] != 0;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(f);
        if (lane == 0) wsum[wv] = (int)__builtin_popcountll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wv; ++w) off += wsum[w];
        if (i < n) cum[i] = off + (int)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int w = 0; w < 16; ++w) t += wsum[w];
            base += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) cum[n] = base;
}

// How the 64-plane z chunks are grouped into work-groups of GWAVES: *shift = (GWAVES - first live chunk mod GWAVES) mod GWAVES, so that the
// first chunk that can receive anything starts a work-group (work-group q holds chunks q * GWAVES - shift ...).  With the chunks grouped from 0
// a live range that starts mid-group leaves a work-group with dead waves at each end; its live waves then compute the dead ones' share of the
// weight tables.  A chunk c is live when a flagged sinogram plane lies in [64 c - zc_hi - 1, 64 c + 63 - zc_lo] (as in the kernel).
__global__ __launch_bounds__(64) void k_zchunk_shift(const unsigned char *__restrict__ flags, int ndz, int nz, int zc_lo, int zc_hi, int *__restrict__ shift)
{
    const int n_chunk = (nz + 63) / 64;
    int first = n_chunk;
    for (int c = threadIdx.x; c < n_chunk; c += 64) {
        bool any = false;
        for (int i = max(0, 64 * c - zc_hi - 1); i <= min(ndz - 1, 64 * c + 63 - zc_lo) && !any; ++i) any = flags[i] != 0;
        if (any) first = min(first, c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
    if (threadIdx.x == 0) *shift = first >= n_chunk ? 0 : (GWAVES - first % GWAVES) % GWAVES;
}

// The SIRT update as the kernel's store (UPD = 1): a lane holds the 64 back-projected values of its column in registers and every voxel is
// written exactly once, so rec = rec + V * acc (a product and a sum, each rounded, as k_update in tomo_ctx.hip: both pin that, the
// build contracts by default), the clamp at 0 and the error sum
// (gt - rec)^2 go where the store is -- no back-projection volume is filled, written, read back and passed over once more by k_update.
// ZERO: a wave whose planes receive nothing (acc = 0) but whose voxels k_update would still clamp and count.
template <bool ZERO>
__device__ __forceinline__ void gather_update_store(float *__restrict__ dst, const float *__restrict__ vv, const float *__restrict__ gt, const f32x2 (&acc2)[32],
                                                    int z0, int nz, int positivity, double *__restrict__ err_out)
{
    double err = 0.0;
#define G_UPD1(R, A, V, G)                                  \
    {                                                       \
        float pr_ = (A) * (V);                              \
        asm volatile("" : "+v"(pr_));       /* the product is rounded on its own: never contracted into an fma with the sum */ \
        R = R + pr_;                                        \
        if (positivity && R < 0.f) R = 0.f;                 \
        if (gt) { const float e_ = (G) - R; err += (double)e_ * (double)e_; } \
    }
    if (z0 + 64 <= nz && (nz & 3) == 0) {
#pragma unroll
        for (int p = 0; p < 64; p += 4) {
            float4 r = *(float4 *)(dst + p);
            const float4 v = *(const float4 *)(vv + p);
            float4 t = {0.f, 0.f, 0.f, 0.f};
            if (gt) t = *(const float4 *)(gt + p);
            G_UPD1(r.x, ZERO ? 0.f : acc2[p / 2].x, v.x, t.x)
            G_UPD1(r.y, ZERO ? 0.f : acc2[p / 2].y, v.y, t.y)
            G_UPD1(r.z, ZERO ? 0.f : acc2[p / 2 + 1].x, v.z, t.z)
            G_UPD1(r.w, ZERO ? 0.f : acc2[p / 2 + 1].y, v.w, t.w)
            *(float4 *)(dst + p) = r;
            __builtin_amdgcn_sched_barrier(0);      // one quad's loads in flight beside the 64 accumulators, not all sixteen (spills)
        }
    } else {
#pragma unroll
        for (int p = 0; p < 64; ++p)
            if (z0 + p < nz) {
                float r = dst[p];
                G_UPD1(r, ZERO ? 0.f : ((p & 1) ? acc2[p / 2].y : acc2[p / 2].x), vv[p], gt[p])
                dst[p] = r;
            }
    }
#undef G_UPD1
    if (gt) {                                                           // wave-uniform
        err = wave_sum_d(err);
        if ((threadIdx.x & 63) == 0) atomicAdd(err_out, err);           // one double atomic per wave (waves of a work-group end at different times)
    }
}

// DMA = 1 (NJ = 3 only; the host launches it when every pose has tau = 0 and the plan's largest |m00| + |m01| is below GDMA_EA: adjoint_tiles,
// tomo_project.hip): the sinogram rows go STRAIGHT into LDS (buffer_load_dword ... lds), into two row buffers in turn -- with tau = 0 and all
// 64 planes of the wave on the detector the staging pass only copied a loaded 256-byte row to base + 4 * lane, which is what a direct-to-LDS
// load writes by itself (a row of 256 bytes inside a pitch of 272: no wave-instruction crosses a row).  No staging stores, no staged
// registers; the rows of projection ip + 1 fly while ip accumulates from the other buffer.  Both loops keep GDMA_ROWS = 13 rows per
// projection: 7 (|m00| + |m01|) < 9.99 leaves i0 at most 11 values over the tile's 8 x 8 columns, + 2.  A wave whose planes can leave the
// detector under some projection takes the register loop (into the first buffer) for all projections.
#define GDMA_ROWS 13
#define GDMA_EA 1.427
template <int NJ, int UPD, int DMA = 0>      // NJ: samples per row that can reach a column: 3 for step >= 0.95 voxel, 6 for step >= 0.475; UPD: the store is the SIRT update
__global__ __launch_bounds__(GWAVES * 64, 16 / GWAVES) void k_adj_gather_flat(const GfC *__restrict__ cs, int n_proj, const float *__restrict__ proj,
                                                                 float *__restrict__ vol, TomoGeomC g, int xs, int xe, int patched,
                                                                 const unsigned char *__restrict__ zflags, int zc_lo, int zc_hi, const int *__restrict__ zshift,
                                                                 const float *__restrict__ upd_v, const float *__restrict__ upd_gt, int positivity,
                                                                 double *__restrict__ upd_err)
{
    static_assert(DMA == 0 || NJ == 3, "the direct-to-LDS loop is built for NJ = 3 only");
    constexpr int NR = DMA ? GDMA_ROWS : GROWS;         // rows loaded per projection
    __shared__ __attribute__((aligned(16))) float rows[GWAVES][NR * GPITCH];
    __shared__ float4 wtab[3][GWAVES][64];          // [group mod 3][projection of the group][column] = (i0, W0, W1, W2)
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the work-group owns 8 x 8 voxel columns; its four waves take four consecutive 64-plane chunks of them.
    // Work-group -> tile mapping: the ~96 work-groups resident on one XCD (32 CUs x 3) should share sinogram rows in that XCD's
    // L2 -- with a plain (z, y, x) grid they formed a 128 x 1.5-tile strip with almost no common rows and every row load went
    // to the fabric (0.88 TB per launch at 1024^3).  Work-groups are dealt to the XCDs round-robin in dispatch order, so XCD k
    // sees the linear ids k, k+8, ...: those are mapped to compact GPX x GPY patches of (x, y) tiles of one z quad (patch
    // p*8 + k for the p-th group of 96 of them): ~10x row reuse within a patch.  ("XCD patches": k_fwd_gather_flat deals its
    // work-groups the same way.)
    // (Small grids keep the plain order, patched = 0: the patch grid is padded to 8 x 96 work-groups, which costs more than
    // the reuse gains below ~256 patches.  Measured at 1024^3: same speed; fabric traffic -64 % on a 64-angle launch, -15 %
    // (0.89 -> 0.76 TB) over 1024 angles, where the work-groups of a patch drift apart in angle index.)
    const int ntx = (xe - xs + GTX - 1) / GTX, nty = (g.ny + GTY - 1) / GTY, nzq = (g.nz + 64 * GWAVES - 1) / (64 * GWAVES) + 1;
    // (+ 1: the chunks are grouped from -shift, k_zchunk_shift above; with shift = 0 the last layer of work-groups lies past the volume and ends at once)
    int tx, ty, zq;
    if (patched) {
        const int npx = (ntx + GPX - 1) / GPX, npy = (nty + GPY - 1) / GPY;
        const int slot = (int)(blockIdx.x >> 3), patch = (slot / (GPX * GPY)) * 8 + (int)(blockIdx.x & 7), within = slot % (GPX * GPY);
        const int pxy = patch % (npx * npy);
        zq = patch / (npx * npy);
        tx = (pxy / npy) * GPX + within / GPY;
        ty = (pxy % npy) * GPY + within % GPY;
    } else {
        zq = (int)(blockIdx.x % (unsigned)nzq);
        ty = (int)((blockIdx.x / (unsigned)nzq) % (unsigned)nty);
        tx = (int)(blockIdx.x / ((unsigned)nzq * (unsigned)nty));
    }
    const int x0 = xs + tx * GTX, y0 = ty * GTY, z0 = (zq * GWAVES + wv - *zshift) * 64;
    if (tx >= ntx || ty >= nty || zq >= nzq) return;                    // uniform over the WORK-GROUP (barriers below)
    // a wave past the volume still computes its share of tables; so does one whose 64 planes Z can only receive zeros: plane Z gathers from the
    // sinogram planes Z - zc and Z - zc - 1 (zc in [zc_lo, zc_hi] over the projections), and k_sino_zflags marked the planes that hold anything
    bool zlive = z0 >= 0 && z0 < g.nz;
    if (zlive) {
        bool any = false;
        for (int i = z0 - zc_hi - 1 + lane; i <= z0 + 63 - zc_lo; i += 64) any |= i >= 0 && i < g.ndz && zflags[i] != 0;
        zlive = __builtin_amdgcn_ballot_w64(any) != 0;
    }
    // Only the LIVE waves stay: nl of them, this one the rk-th.  They share the weight tables among themselves (a wave that has ended is not
    // waited for by s_barrier); a work-group none of whose z chunks can receive anything ends here (its voxels keep what they hold).
    __shared__ int wlive[GWAVES];
    if (lane == 0) wlive[wv] = zlive ? 1 : 0;
    __syncthreads();
    int nl = 0, rk = 0;
#pragma unroll
    for (int w = 0; w < GWAVES; ++w) { nl += wlive[w]; rk += w < wv ? wlive[w] : 0; }
    // HARDWARE BEHAVIOUR RELIED ON (outside the HIP programming model): on gfx9 / CDNA s_barrier counts only the waves of the
    // work-group that have not terminated, so the live waves may keep calling __syncthreads() after the dead ones returned.
#if !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__) && defined(__HIP_DEVICE_COMPILE__)
#error "k_adj_gather_flat: divergent exit before barriers is only known to be safe on gfx9-family targets (s_barrier ignores ended waves)"
#endif
    if (UPD && !zlive && z0 >= 0 && z0 < g.nz && (positivity || upd_gt)) {
        // its voxels receive nothing, rec + V * 0 = rec: nothing to store -- unless the update clamps or sums the error, which k_update does for every voxel
        const int X = x0 + (lane >> 3), Y = y0 + (lane & 7);
        if (X < xe && Y < g.ny) {
            const size_t o = ((size_t)X * g.ny + Y) * g.nz + z0;
            f32x2 none[32];
            gather_update_store<true>(vol + o, upd_v + o, upd_gt ? upd_gt + o : nullptr, none, z0, g.nz, positivity, upd_err);
        }
    }
    if (!zlive) return;
    // a lane is a voxel COLUMN (X, Y) with 64 plane accumulators, except while loading sinogram rows, where it is plane Zl
    const int X = x0 + (lane >> 3), Y = y0 + (lane & 7), Zl = z0 + lane;
    float *wrows = rows[wv];
    const size_t n_det = (size_t)g.ndx * g.ndz;
    const uint32_t pitch4 = (uint32_t)g.ndz * 4u;                     // one projection's sinogram is < 4 GiB (host check)
    const float two_m32 = 2.3283064365386963e-10f;
    f32x2 acc2[32];                                                   // plane pairs (2k, 2k + 1)
#pragma unroll
    for (int p = 0; p < 32; ++p) acc2[p] = f32x2{0.f, 0.f};

    // ---- 1. the weight table of this lane's column for projection IPX -> wtab[GRP % 3][IPX % GWAVES][lane].  The table does not
    //         depend on z: the nl live waves share it, the rk-th computes the projections nl g + rk (one barrier per nl projections).
    //   candidates: rows i0..i0+2, samples j0..j0+NJ-1 (the footprint |dx|,|dy| < 1 maps to |d ix| <= |m00|+|m01| < 1.5: three
    //   consecutive integers cover an interval shorter than 3; likewise |d j| <= |m10|+|m11| < NJ/2); W_k from exact 32.32
    //   positions relative to the voxel
#define G_TABLE(IPX, BUF, SLOT)                                                                                            \
    {                                                                                                                      \
        float4 t4 = {0.f, 0.f, 0.f, 0.f};                                                                                  \
        if ((IPX) < n_proj) {                                                                                              \
            const GfC &ct = cs[IPX];                                                                                       \
            const float qx = (float)X - ct.p0x, qy = (float)Y - ct.p0y;                                                    \
            const float a = ct.m00 * qx + ct.m01 * qy, b = ct.m10 * qx + ct.m11 * qy;                                      \
            const int i0 = (int)ceilf(a - (fabsf(ct.m00) + fabsf(ct.m01) + 5e-3f));                                        \
            const int j0 = (int)ceilf(b - (fabsf(ct.m10) + fabsf(ct.m11) + 5e-3f));                                        \
            int64_t rx = ct.fp0x + (int64_t)i0 * ct.fux + (int64_t)j0 * ct.fdx - ((int64_t)X << 32);                       \
            int64_t ry = ct.fp0y + (int64_t)i0 * ct.fuy + (int64_t)j0 * ct.fdy - ((int64_t)Y << 32);                       \
            float W[3];                                                                                                    \
            _Pragma("unroll") for (int k = 0; k < 3; ++k) {                                                                \
                int64_t sx = rx, sy = ry;                                                                                  \
                float wsum = 0.f;                                                                                          \
                _Pragma("unroll") for (int mth = 0; mth < NJ; ++mth) {                                                     \
                    const int hx = (int)(sx >> 32), hy = (int)(sy >> 32);                                                  \
                    const float fx = (float)(unsigned)sx * two_m32, fy = (float)(unsigned)sy * two_m32;                    \
                    /* tent on [-1, 1); selects in the SGPR-mask form (select_lanes) */                                    \
                    const float wx = select_lanes2(select_lanes(fx, __builtin_amdgcn_ballot_w64(hx == -1)), 1.f - fx, __builtin_amdgcn_ballot_w64(hx == 0)); \
                    const float wy = select_lanes2(select_lanes(fy, __builtin_amdgcn_ballot_w64(hy == -1)), 1.f - fy, __builtin_amdgcn_ballot_w64(hy == 0)); \
                    wsum += select_lanes(wx * wy, __builtin_amdgcn_ballot_w64((unsigned)(j0 + mth) < (unsigned)ct.n));     \
                    sx += ct.fdx; sy += ct.fdy;                                                                            \
                }                                                                                                          \
                W[k] = select_lanes(wsum, __builtin_amdgcn_ballot_w64((unsigned)(i0 + k) < (unsigned)g.ndx));              \
                rx += ct.fux; ry += ct.fuy;                                                                                \
            }                                                                                                              \
            t4.x = __builtin_bit_cast(float, i0); t4.y = W[0]; t4.z = W[1]; t4.w = W[2];                                   \
        }                                                                                                                  \
        wtab[BUF][SLOT][lane] = t4;                                                                                        \
    }
    // ---- 2. projection IPX's sinogram rows.  G_SETUP fetches the table entry and ISSUES the 15 loads of the rows the tile can touch: rows
    //         ix_lo .. ix_lo+13 at this lane's PLANE (coalesced) plus one gather of their values one plane below the wave's
    //         first, from clamped -- always valid -- addresses, masked when used.  Straight-line on purpose (with a branch per
    //         row every row waited for its own round trip to memory).  G_STAGE z-lerps them into the wave's LDS rows.  The projection
    //         before IPX accumulates between the two: the loads fly meanwhile, and the registers y0v[] live only from the one to the other,
    //         inside one pass of the projection loop (nothing of them is carried round the loop: no copies at the hand-over).
    //         Addresses: a buffer resource over the projection's sinogram (its base is wave-uniform); the lane's plane offset is the
    //         vector offset, the row's byte offset the SCALAR offset of the load.  The 14 clamped row offsets are computed by 14 LANES
    //         at once and handed out with v_readlane: per row one readlane, no add, no scalar clamp / multiply / 64-bit add (the kernel
    //         once issued 335 SALU instructions per projection and wave against 290 VALU -- the scalar unit, one per CU, was the limit).
    //         Every offset is clamped to the sinogram here; the resource's own range check is never relied on.
    //         Whether the projection's rays hit the tile at all (G_HIT, hit_n) is evaluated HERE, from the table entry, not after the
    //         accumulate where it is used: its wave-wide test then no longer sits between the accumulate and G_STAGE (measured at 1024^3 x
    //         1024 angles: 116.3 -> 112.6 ms per launch).  The loads stay unconditional: skipping them for the 13.5 % of wave-projections
    //         that miss put a branch round the block and cost what the early test gained (profiles/slab_range_before_after.md).
#ifdef TOMO_ABLATE_GATHER_LOADS     /* measurement builds only: the kernel without its sinogram loads (wrong sums) */
#define G_ROW_LOAD(RS, VOFF, SOFF) __int_as_float(0x3f800000 + (int)((VOFF) + (SOFF)))
#else
#define G_ROW_LOAD(RS, VOFF, SOFF) __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32((RS), (VOFF), (SOFF), 0))
#endif
    const uint32_t det_bytes = (uint32_t)min((unsigned long long)n_det * 4ull, 0xffffffffull);      // (< 4 GiB, as for pitch4 above: all of it)
#define G_SETUP(IPX, BUF, SLOT)                                                                                            \
    {                                                                                                                      \
        tn = wtab[BUF][SLOT][lane];                                                                                        \
        hit_n = G_HIT(tn);                  /* (here, not after the accumulate: see above) */                              \
        const int i0s = __builtin_bit_cast(int, tn.x);                                                                     \
        ix_lo_n = __builtin_amdgcn_readfirstlane(gwave_min_i32(i0s));                                                      \
        const GfC &cn = cs[IPX];                                                                                           \
        const int iz0 = Zl - cn.zc;                                                                                        \
        const __amdgpu_buffer_rsrc_t srs =                                                                                 \
            __builtin_amdgcn_make_buffer_rsrc((void *)(proj + (size_t)cn.slot * n_det), 0, (int)det_bytes, 0x00020000);    \
        const uint32_t o0 = (uint32_t)min(max(iz0, 0), g.ndz - 1) * 4u;                                                    \
        const uint32_t rowoff = (uint32_t)min(max(ix_lo_n + min(lane, NR - 1), 0), g.ndx - 1) * pitch4;                    \
        _Pragma("unroll") for (int r = 0; r < NR; ++r)                                                                     \
            y0v[r] = G_ROW_LOAD(srs, o0, (uint32_t)__builtin_amdgcn_readlane((int)rowoff, r));                             \
        /* the plane below (iz0 - 1) is the neighbouring lane's value (DPP shift when used); lane 0 has no neighbour: one  */ \
        /* more load, lane r fetching row r at the wave's first plane - 1 -- 15 loads per projection instead of 28      */ \
        if (cn.tau != 0.f) {                                                /* (tau = 0: the plane below is never used) */ \
            const uint32_t oe = (uint32_t)min(max(z0 - cn.zc - 1, 0), g.ndz - 1) * 4u;                                     \
            yedge = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srs, rowoff + oe, 0, 0));               \
        }                                                                                                                  \
    }
#define G_ZLERP(MASKED, TAU)                                                                                                      \
    _Pragma("unroll") for (int r = 0; r < NR; ++r) {                                                                              \
        float y1 = dpp_shr1_f(y0v[r]);                                           /* lane l <- lane l - 1: y(ix, iz0 - 1) for l >= 1 */ \
        asm("v_writelane_b32 %0, %1, 0" : "+v"(y1) : "s"(__builtin_amdgcn_readlane(__builtin_bit_cast(int, yedge), r)));   /* lane 0 <- row r's edge value */ \
        const float a0 = (MASKED) ? select_lanes(y0v[r], m0) : y0v[r], a1 = (MASKED) ? select_lanes(y1, m1) : y1;                \
        wrows[r * GPITCH + lane] = fmaf((TAU), a1 - a0, a0);                                                                      \
    }
    // (no per-row validity test: a row outside the detector was loaded from a clamped, valid address and every lane's
    //  weight for it is 0 (G_TABLE); rows past the last one a lane needs are never read)
#ifdef TOMO_ABLATE_GATHER_STAGE     /* measurement builds only: the nominal scan's staging stores gone -- the loads are kept alive by NR - 1 adds and */
#define G_STAGE_COPY                /* ONE row is stored (wrong sums; loads, VALU and reads as before): profiles/adj_dma_before_after.md               */ \
    {                                                                                                                      \
        float ysum = y0v[0];                                                                                               \
        _Pragma("unroll") for (int r = 1; r < NR; ++r) ysum += y0v[r];                                                     \
        wrows[lane] = ysum;                                                                                                \
    }
#else
#define G_STAGE_COPY _Pragma("unroll") for (int r = 0; r < NR; ++r) wrows[r * GPITCH + lane] = y0v[r];
#endif
#define G_STAGE(IPX)                                                                                                      \
    {                                                                                                                      \
        const GfC &cn = cs[IPX];                                                                                           \
        const int iz0 = Zl - cn.zc, iz1 = iz0 - 1;                                                                         \
        const unsigned long long m0 = __builtin_amdgcn_ballot_w64(iz0 >= 0) & __builtin_amdgcn_ballot_w64(iz0 < g.ndz);    \
        const unsigned long long m1 = __builtin_amdgcn_ballot_w64(iz1 >= 0) & __builtin_amdgcn_ballot_w64(iz1 < g.ndz);    \
        if (cn.tau == 0.f) {            /* samples sit exactly on detector rows (integer z shift: the nominal geometry before */ \
            if (m0 == ~0ull) {          /* alignment): Yz = y -- no neighbour plane, no lerp (fma(0, a1 - a0, a0) = a0)      */ \
                G_STAGE_COPY            /* all 64 planes on the detector: no select either */                              \
            } else {                                                                                                       \
                _Pragma("unroll") for (int r = 0; r < NR; ++r) wrows[r * GPITCH + lane] = select_lanes(y0v[r], m0);        \
            }                                                                                                              \
        }                                                                                                                  \
        else if ((m0 & m1) == ~0ull) { G_ZLERP(false, cn.tau) }     /* all 64 planes and their lower neighbours on the detector: the usual case */ \
        else { G_ZLERP(true, cn.tau) }                                                                                     \
    }
#define G_HIT(T) (__any((T).y != 0.f || (T).z != 0.f || (T).w != 0.f))      /* else this projection's rays miss the tile */
    // ---- 3. accumulate, lane = column: its three rows start at slot0; plane p is an immediate offset.  The LDS rows WR were
    //         written by (or, DMA, loaded for) this same wave, no other wave touches them.
    //         plane QUADS with ds_read_b128 (round 2): 256 B/clk where ds_read_b32 moves 128 B/clk -- the kernel was LDS-bound
    //         (SQ_LDS_IDX_ACTIVE = 0.79 of its cycles) on 3 x 64 dword reads per projection.
    //         two quads of reads in flight: quad p + 4 is issued before quad p is used (24 temporaries; with one quad in
    //         flight a wave had 6 packed FMAs to cover each LDS round trip).
    //         plane pairs as packed FMAs (v_pk_fma_f32: two planes per instruction at 0.83 of the scalar rate).
    //         The sched_barrier keeps the reads from all being hoisted to the top (192 temporaries).
#define G_ACCUM(WR)                                                                                                        \
    {                                                                                                                      \
        const int i0 = __builtin_bit_cast(int, t.x);                                                                       \
        const float W0 = t.y, W1 = t.z, W2 = t.w;                                                                          \
        const int slot0 = min(max(i0 - ix_lo, 0), NR - 3);      /* an 8 x 8 column tile touches <= 13 rows (7 (|cos| + |sin|) + 3); clamped for safety */ \
        const float4 *q = (const float4 *)__builtin_assume_aligned((WR) + slot0 * GPITCH, 16);                             \
        float4 n0 = q[0], n1 = q[GPITCH / 4], n2 = q[2 * GPITCH / 4];                                                      \
        _Pragma("unroll") for (int p = 0; p < 64; p += 4) {                                                                \
            const float4 r0 = n0, r1 = n1, r2 = n2;                                                                        \
            if (p + 4 < 64) { n0 = q[(p + 4) / 4]; n1 = q[(GPITCH + p + 4) / 4]; n2 = q[(2 * GPITCH + p + 4) / 4]; }       \
            acc2[p / 2] = W2 * f32x2{r2.x, r2.y} + (W1 * f32x2{r1.x, r1.y} + (W0 * f32x2{r0.x, r0.y} + acc2[p / 2]));      \
            acc2[p / 2 + 1] = W2 * f32x2{r2.z, r2.w} + (W1 * f32x2{r1.z, r1.w} + (W0 * f32x2{r0.z, r0.w} + acc2[p / 2 + 1])); \
            __builtin_amdgcn_sched_barrier(0);                                                                             \
        }                                                                                                                  \
    }
    const int n_grp = (n_proj + nl - 1) / nl;
    int buf = 0;                                                        // table buffer of the current group (three in rotation)
    float4 t = {0.f, 0.f, 0.f, 0.f};                                    // the projection whose rows are in the LDS rows
    int ix_lo = 0;
    bool hit = false;
    bool reg_loop = true;
    if constexpr (DMA != 0) {
        // ---- the direct-to-LDS loop.  Wave-uniform and decided once: all 64 planes on the detector under every projection (the register
        //      loop below otherwise, from the start and for all projections: nothing is ordered between the two mechanisms).  Both kinds of
        //      wave of a work-group meet at the same barriers, one per group of nl projections.
        __shared__ __attribute__((aligned(16))) float rows_b[GWAVES][NR * GPITCH];     // a second OBJECT, never an index: the compiler's counted vmcnt rests on telling the two apart
        if (z0 - zc_hi >= 0 && z0 + 63 - zc_lo < g.ndz && n_grp > 0) {
            reg_loop = false;
            float *const wrows_b = rows_b[wv];
            // G_DMA_ISSUE: G_SETUP with the LDS row as the loads' destination (LDS address = the row's base, wave-uniform in M0, + 4 * lane)
#define G_DMA_ISSUE(IPX, BUF, SLOT, DST)                                                                                   \
            {                                                                                                              \
                tn = wtab[BUF][SLOT][lane];                                                                                \
                hit_n = G_HIT(tn);                                                                                         \
                const int i0s = __builtin_bit_cast(int, tn.x);                                                             \
                ix_lo_n = __builtin_amdgcn_readfirstlane(gwave_min_i32(i0s));                                              \
                const GfC &cn = cs[IPX];                                                                                   \
                const __amdgpu_buffer_rsrc_t srs =                                                                         \
                    __builtin_amdgcn_make_buffer_rsrc((void *)(proj + (size_t)cn.slot * n_det), 0, (int)det_bytes, 0x00020000); \
                const uint32_t o0 = (uint32_t)min(max(Zl - cn.zc, 0), g.ndz - 1) * 4u;                                     \
                const uint32_t rowoff = (uint32_t)min(max(ix_lo_n + min(lane, NR - 1), 0), g.ndx - 1) * pitch4;            \
                _Pragma("unroll") for (int r = 0; r < NR; ++r)                                                             \
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(srs, (__attribute__((address_space(3))) void *)((DST) + r * GPITCH), 4, (int)o0, \
                                                             __builtin_amdgcn_readlane((int)rowoff, r), 0, 0);             \
            }
            // the tables are published behind lgkmcnt(0) and a RAW barrier: __syncthreads() would drain the loads in flight (vmcnt(0))
#define G_DMA_BARRIER                                                                                                      \
            {                                                                                                              \
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                         \
                __builtin_amdgcn_s_barrier();                                                                              \
                asm volatile("" ::: "memory");                                                                             \
            }
            // One pass: (a group starts: next group's tables, barrier;) issue the rows of projection IP + 1 into NXT; accumulate IP from CUR.
            // The loads are unconditional -- the last pass fetches its own rows once more -- so that every accumulate sees the same queue:
            // its own NR loads landed, NR younger ones in flight (a counted vmcnt).  NXT's last readers are done: the table read above
            // the loads returns behind them (LDS answers a wave in order) and the loads' addresses wait for it.
#define G_DMA_PASS(IP, CUR, NXT)                                                                                           \
            {                                                                                                              \
                if ((IP) == g1) {                                                                                          \
                    if ((IP) > 0) buf = nbuf;                                                                              \
                    nbuf = buf == 2 ? 0 : buf + 1;                                                                         \
                    g0 = (IP); g1 = min(n_proj, g0 + nl);                                                                  \
                    if (g0 + nl < n_proj) G_TABLE(g0 + nl + rk, nbuf, rk)                                                  \
                    G_DMA_BARRIER                                                                                          \
                }                                                                                                          \
                {                                                                                                          \
                    const int ipn = min((IP) + 1, n_proj - 1);                                                             \
                    const bool same = ipn < g1;                                                                            \
                    const int sbuf = same ? buf : nbuf, sslot = same ? ipn - g0 : 0;                                       \
                    G_DMA_ISSUE(ipn, sbuf, sslot, NXT)                                                                     \
                }                                                                                                          \
                if (hit) G_ACCUM(CUR)                                                                                      \
                hit = hit_n; t = tn; ix_lo = ix_lo_n;                                                                      \
            }
            G_TABLE(rk, 0, rk)                                          // group 0
            __syncthreads();                                            // (no load in flight yet)
            float4 tn;
            int ix_lo_n = 0;
            bool hit_n;
            G_DMA_ISSUE(0, 0, 0, wrows)
            hit = hit_n; t = tn; ix_lo = ix_lo_n;
            int g0 = 0, g1 = 0, nbuf = 0;
            for (int ip = 0; ip < n_proj; ip += 2) {                    // by two: each pass names its buffers statically
                G_DMA_PASS(ip, wrows, wrows_b)
                if (ip + 1 >= n_proj) break;
                G_DMA_PASS(ip + 1, wrows_b, wrows)
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the last pass's loads: nothing may land in LDS after the wave has ended
#undef G_DMA_ISSUE
#undef G_DMA_BARRIER
#undef G_DMA_PASS
        }
    }
    if (reg_loop && n_grp > 0) {
        G_TABLE(rk, 0, rk)                                              // group 0
        __syncthreads();
        float4 tn;
        int ix_lo_n = 0;
        bool hit_n;
        float y0v[NR], yedge = 0.f;                                     // yedge: lane r holds row r one plane below the wave's first
        G_SETUP(0, 0, 0)
        hit = hit_n;
        if (hit) G_STAGE(0)
        t = tn; ix_lo = ix_lo_n;
    }
    for (int grp = 0; reg_loop && grp < n_grp; ++grp) {
        const int nbuf = buf == 2 ? 0 : buf + 1;
        if (grp + 1 < n_grp) G_TABLE((grp + 1) * nl + rk, nbuf, rk)     // next group's tables: a third buffer, nobody reads it yet
        __syncthreads();                                                // ... and everybody is done with group grp - 1's buffer
        const int g0 = grp * nl, g1 = min(n_proj, g0 + nl);
        for (int ip = g0; ip < g1; ++ip) {
            float4 tn = t;
            int ix_lo_n = ix_lo;
            bool hit_n = false;
            float y0v[NR], yedge = 0.f;
            const bool more = ip + 1 < n_proj;
            if (more) {
                const bool same = ip + 1 < g1;                              // else the next group's table, already published
                const int sbuf = same ? buf : nbuf, sslot = same ? ip + 1 - g0 : 0;
                G_SETUP(ip + 1, sbuf, sslot)
            }
            if (hit) G_ACCUM(wrows)
            // ---- 2b. the rows loaded above, z-lerped into the wave's LDS rows (lane = plane)
            hit = hit_n;
            if (hit) G_STAGE(ip + 1)
            t = tn; ix_lo = ix_lo_n;
        }
        buf = nbuf;
    }
#undef G_ACCUM
#undef G_STAGE_COPY
#undef G_TABLE
#undef G_ROW_LOAD
#undef G_SETUP
#undef G_ZLERP
#undef G_STAGE
#undef G_HIT
    // ---- store: the lane's column is 64 consecutive floats of the volume
    if (UPD) {
        if (X < xe && Y < g.ny) {
            const size_t o = ((size_t)X * g.ny + Y) * g.nz + z0;
            gather_update_store<false>(vol + o, upd_v + o, upd_gt ? upd_gt + o : nullptr, acc2, z0, g.nz, positivity, upd_err);
        }
    } else if (zlive && X < xe && Y < g.ny) {
        float *dst = vol + ((size_t)X * g.ny + Y) * g.nz + z0;
        if (z0 + 64 <= g.nz && (g.nz & 3) == 0) {
#pragma unroll
            for (int p = 0; p < 64; p += 4) {
                float4 v = *(float4 *)(dst + p);
                v.x += acc2[p / 2].x; v.y += acc2[p / 2].y; v.z += acc2[p / 2 + 1].x; v.w += acc2[p / 2 + 1].y;
                *(float4 *)(dst + p) = v;
            }
        } else {
#pragma unroll
            for (int p = 0; p < 64; ++p)
                if (z0 + p < g.nz) dst[p] += (p & 1) ? acc2[p / 2].y : acc2[p / 2].x;
        }
    }
}


// ------------------------------------------------------------------------------------------------
// GATHER-form FORWARD for the same lattices (k_fwd_gather_flat; per list fwd_gather_flat_body<NW, WALKY>): the role swap of k_adj_gather_flat.  Rays own their sums in
// registers, the volume streams through wave-private LDS rows, nothing is added across work-groups:
//     (A x)(ix, iz) = (1 - tau) S(ix, iz + zc) + tau S(ix, iz + zc + 1),     S(ix, Z) = sum_{X, Y} W(X, Y, ix) x(X, Y, Z)
// with the adjoint's W.  A wave owns 8 projections x 8 adjacent detector rows x 64 volume planes (lane = ray, 64 plane sums per lane) and
// WALKS the volume one slab at a time: x slabs for the projections with |d_x| >= |d_y| (WALKY = 0: slab S = X, line L = Y), y slabs for
// the others (WALKY = 1: S = Y, L = X).  The host sorts the projections into one list per (walk, NW), so no group straddles 45 degrees,
// and pads a list with -1 where it jumps to another range of poses: eight rays of distant angles share no lines.
//   1. lane = RAY: the <= 3 samples with |p_S - S| < 1 (exact 32.32 positions, the adjoint's tents) give the first line L0 and the weights
//      W0 .. W(NW-1) of the nodes (S, L0 + k).  The samples lie in an open interval of p_S of length 2, i.e. of p_L of length
//      2 |d_L / d_S|: <= 1 -> 3 nodes (NW = 3), else (|d_L| <= |d_S|, <= 3 samples, 2 |d_L| < 2) -> 4.  The table does not depend on z: the
//      live waves of a work-group (z chunks of the same rays) share it through the adjoint's triple-buffered LDS table;
//   2. lane = PLANE: the FGROWS lines from wave_min(L0) on are loaded (coalesced 256 B) one slab ahead and written to the wave's LDS rows;
//   3. lane = RAY again: per four planes NW ds_read_b128 at row(lane) + immediate and 2 NW v_pk_fma_f32.
// Rays of eight different projections drift apart with the distance from the rotation centre (tools/fwd_gather_model.py): a slab whose
// lanes span more than FGROWS lines is done in WINDOWS of FGROWS lines advancing by FGROWS - NW + 1 (a lane's NW lines lie in exactly
// one window); the first window rides the pipelined loads, the others (rare at FGROWS = 24 and detector pitch 1) load on the spot.
// Which calls come here is forward_tiles' rule (tomo_project.hip): every pose takes the gather adjoint (above: that is where the detector-x
// pitch enters), 2 / |d_S| + slack < 3 and |d_L| < 1 with d the sample step along the walked and the other axis, i.e.
// step max(|cos|, |sin|) >= 0.67 and step min(|cos|, |sin|) < 0.999, and (|cos| + |sin|) / step < 1.49.  The detector-x pitch itself is
// free: a ray is walked on its own; with rows det_dx voxels apart a wave's eight rows spread over det_dx times as many lines and more
// steps take a second or third window (pitch 2: 7 steps in 10 on the second-window case of tests/test_gpu_pitch.py).
// The z lerp comes last, once per ray.  The sinogram is zero-filled by the caller: a wave stores its rays' 63 (tau != 0) or 64 values
// with plain stores; the value that also needs the next chunk's first plane is completed by one atomic from each of the two waves
// (0 + a + b = 0 + b + a: still the same bits on every run).
// A wave walks only the slabs [s_lo, s_hi) that some ray of it can cross (step 0 of the body); a work-group with none ends at once: its
// rays keep the caller's zeros.
// ------------------------------------------------------------------------------------------------
#define FGROWS 24
#define FG_NONE (1 << 29)          // "this lane has no line": above every real line index, far from integer overflow
#ifndef FPG
#define FPG 16             // patch of (projection groups x row tiles) that an XCD's work-groups cover together.  MEASURED at 1024^3 x 1024
#define FPR 4              // (profiles/fwd_patches_before_after.md): every shape of >= 13 groups x 2 .. 4 row tiles gives the same time, 8 % under the
#endif                     // plain order; the model's choice, 8 x 12, gives none (tools/fwd_gather_model.py counts lines, not when they are asked for)
#define FWD_PATCH_MIN 128  // patches (all lists, all z quads) from which forward_tiles deals patches: 64 (256^3 x 256) lose 12 %, 144 (384^3 x 384) gain 3 %

// Work-groups that one list of n_list entries (padding included) takes in the grid of k_fwd_gather_flat: the (group, row tile) pairs of a z
// quad rounded up to a multiple of the 8 XCDs, times the z quads; or the list's patches of FPG x FPR such pairs (all z quads), rounded up
// to a multiple of 8.  The host sizes the grid with it, the kernel finds a work-group's list with it.
__host__ __device__ static inline unsigned long long fg_list_wgs(int n_list, int nrt, int nzq, int patched)
{
    const unsigned long long npg = (unsigned long long)((n_list + 7) / 8);
    if (!patched) return 8ull * ((npg * (unsigned long long)nrt + 7) / 8) * (unsigned long long)nzq;
    const unsigned long long npq = ((npg + FPG - 1) / FPG) * (unsigned long long)((nrt + FPR - 1) / FPR);
    return 8ull * ((npq * (unsigned long long)nzq + 7) / 8) * (unsigned long long)(FPG * FPR);
}

// The body of k_fwd_gather_flat for one list.  (A line's plane is addressed as slab base, wave-uniform 64-bit, + 32-bit byte offset: the host
// checks that the volume is <= 4 GiB.)
template <int NW, int WALKY>
__device__ __forceinline__ void fwd_gather_flat_body(const GfC *__restrict__ cs, const int *__restrict__ perm, int n_list, unsigned block_id,
                                                     int patched, float *__restrict__ proj, const float *__restrict__ vol, const TomoGeomC &g,
                                                     const unsigned char *__restrict__ vflags, const int *__restrict__ zshift,
                                                     float (*rows)[FGROWS * GPITCH], float4 (*wtab)[GWAVES][64], int (*ltab)[GWAVES][64], int *wlive)
{
    static_assert(NW == 3 || NW == 4, "NW");
    constexpr int SW = FGROWS - NW + 1;             // window advance
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nS = WALKY ? g.ny : g.nx, nL = WALKY ? g.nx : g.ny;
    const uint32_t strideL4 = (WALKY ? (uint32_t)g.ny * (uint32_t)g.nz : (uint32_t)g.nz) * 4u;
    const size_t strideS = WALKY ? (size_t)g.nz : (size_t)g.ny * g.nz;
    // Work-group -> (projection group, row tile, z quad).  Work-groups are dealt to the 8 XCDs round-robin, so XCD k sees the ids k, k + 8, ...
    // of the list ("XCD patches", the scheme of k_adj_gather_flat).  patched: the work-groups that follow each other on an XCD
    // form PATCHES of FPG consecutive projection groups x FPR consecutive row tiles of one z quad: the same few detector rows under many
    // neighbouring angles.  Their rays cross each other inside the volume and their slab ranges nearly coincide, so part of the lines a
    // wave asks for is still in that XCD's L2; with the plain order below the resident work-groups are one group x 96 row tiles, and
    // only neighbouring row tiles overlap.  A patch never leaves its list; groups and row tiles are split evenly over the patches of a
    // list, and the surplus work-groups of a patch (its FPG x FPR slots are not all used) end here.  Patch p * 8 + k of the list goes to
    // XCD k, patches numbered z quad by z quad, row-tile patches fastest: the eight XCDs hold neighbouring patches of one z quad, and
    // every XCD gets its share of the light patches (detector edge, dead z quads) -- the k-th eighth of the patches per XCD was 50 % slower.
    // Plain order (small grids: the padding costs more than the reuse gains): XCD k takes the k-th eighth of the (group, tile) pairs of one
    // z quad after the other, row tiles fastest.
    const int npg = (n_list + 7) / 8, nrt = (g.ndx + 7) / 8, nzq = (g.nz + 64 * GWAVES - 1) / (64 * GWAVES) + 1;
    const int slot_id = (int)(block_id >> 3), xcd = (int)(block_id & 7);
    int pg, rt, zq;
    if (patched) {
        const int npp = (npg + FPG - 1) / FPG, nrp = (nrt + FPR - 1) / FPR, npq = npp * nrp;
        const int within = slot_id % (FPG * FPR);
        const int patch = (slot_id / (FPG * FPR)) * 8 + xcd;
        zq = patch / npq;
        const int pgp = (patch % npq) / nrp, rtp = (patch % npq) % nrp;
        // the groups and the row tiles are split EVENLY over the patches (38 groups: 13 13 12, not 16 16 6): patches of like size
        const int pg0 = pgp * npg / npp, pgc = (pgp + 1) * npg / npp - pg0, rt0 = rtp * nrt / nrp, rtc = (rtp + 1) * nrt / nrp - rt0;
        if (zq >= nzq || within / FPR >= pgc || within % FPR >= rtc) return;     // uniform over the work-group, before the first barrier
        pg = pg0 + within / FPR;
        rt = rt0 + within % FPR;
    } else {
        const int m_all = npg * nrt, m8 = (m_all + 7) / 8;
        const int tile = xcd * m8 + slot_id % m8;
        zq = slot_id / m8;
        if (tile >= m_all) return;                                        // uniform over the work-group
        pg = tile / nrt;
        rt = tile % nrt;
    }
    if (zq >= nzq) return;
    const int z0 = (zq * GWAVES + wv - *zshift) * 64;
    bool zlive = z0 >= 0 && z0 < g.nz;
    if (zlive) {
        const int i = z0 + lane;
        zlive = __builtin_amdgcn_ballot_w64(i < g.nz && vflags[i] != 0) != 0;
    }
    if (lane == 0) wlive[wv] = zlive ? 1 : 0;
    __syncthreads();
    int nl = 0, rk = 0;
#pragma unroll
    for (int w = 0; w < GWAVES; ++w) { nl += wlive[w]; rk += w < wv ? wlive[w] : 0; }
    // (the dead waves leave; the live ones keep meeting at barriers: see k_adj_gather_flat for the hardware behaviour relied on)
#if !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__) && defined(__HIP_DEVICE_COMPILE__)
#error "k_fwd_gather_flat: divergent exit before barriers is only known to be safe on gfx9-family targets (s_barrier ignores ended waves)"
#endif
    if (!zlive) return;

    // ---- the lane's ray
    const int ipl = pg * 8 + (lane >> 3), ix = rt * 8 + (lane & 7);
    const int pe = perm[min(ipl, n_list - 1)];                            // < 0: padding (the host starts a new group where the poses jump)
    const bool ray_ok = ipl < n_list && ix < g.ndx && pe >= 0;
    const GfC &c = cs[max(pe, 0)];
    const int64_t fds = WALKY ? c.fdy : c.fdx, fdl = WALKY ? c.fdx : c.fdy;
    const int64_t bs0 = (WALKY ? c.fp0y : c.fp0x) + (int64_t)ix * (WALKY ? c.fuy : c.fux);
    const int64_t bl0 = (WALKY ? c.fp0x : c.fp0y) + (int64_t)ix * (WALKY ? c.fux : c.fuy);
    const float bsf = (float)((double)bs0 * 2.3283064365386963e-10), inv_ds = (float)(4294967296.0 / (double)fds);
    const int n_smp = ray_ok ? c.n : 0;
    const float two_m32 = 2.3283064365386963e-10f;
    const int Zl = z0 + lane;
    const unsigned long long mz = __builtin_amdgcn_ballot_w64(Zl < g.nz);
    const uint32_t o0 = (uint32_t)min(Zl, g.nz - 1) * 4u;
    float *wrows = rows[wv];
    f32x2 acc2[32];
#pragma unroll
    for (int p = 0; p < 32; ++p) acc2[p] = f32x2{0.f, 0.f};

    // ---- 0. the slabs [s_lo, s_hi) outside which none of the wave's 64 rays can have a weight.  A ray has one in slab S when a sample j of
    //         [0, n) lies within one slab of S on a line p_L in (-1, nL): those j are ONE interval, so the empty slabs are a prefix and a suffix
    //         of the walk.  Conservative: float positions (ulp 1e-3 at 8192) against a line range widened by 0.05, two samples and two slabs
    //         of slack.  The waves of a work-group hold the same rays and find the same range: the barrier count below stays uniform.
    int s_lo, s_hi;
    {
        const float dsf = (float)((double)fds * 2.3283064365386963e-10), dlf = (float)((double)fdl * 2.3283064365386963e-10);
        const float blf = (float)((double)bl0 * 2.3283064365386963e-10);
        float ja = 0.f, jb = (float)(n_smp - 1);                          // (no ray: empty)
        if (fabsf(dlf) > 1e-6f) {
            const float ta = (-1.05f - blf) / dlf, tb = ((float)nL + 0.05f - blf) / dlf;
            ja = fmaxf(ja, fminf(ta, tb) - 2.f);
            jb = fminf(jb, fmaxf(ta, tb) + 2.f);
        } else if (!(blf > -1.5f && blf < (float)nL + 0.5f))              // the line moves by < 0.02 along the whole ray
            jb = -1.f;
        int lo = FG_NONE, hi = -FG_NONE;
        if (ja <= jb) {
            const float pa = bsf + ja * dsf, pb = bsf + jb * dsf, top = (float)nS + 4.f;
            lo = (int)floorf(fminf(fmaxf(fminf(pa, pb), -4.f), top)) - 2;
            hi = (int)ceilf(fminf(fmaxf(fmaxf(pa, pb), -4.f), top)) + 3;
        }
        s_lo = max(__builtin_amdgcn_readfirstlane(gwave_min_i32(lo)), 0);
        s_hi = min(__builtin_amdgcn_readfirstlane(gwave_max_i32(hi)), nS);
    }
    if (s_lo >= s_hi) return;                                     // (the caller's zero fill stands)

    // ---- 1. the table of this lane's ray for slab SX -> wtab / ltab[BUF][SLOT][lane]
#define FG_TABLE(SX, BUF, SLOT)                                                                                            \
    {                                                                                                                      \
        float W[4] = {0.f, 0.f, 0.f, 0.f};                                                                                 \
        int L0 = FG_NONE;                                                                                                  \
        if ((SX) < s_hi) {                                                                                                 \
            const float ta = ((float)((SX) - 1) - bsf) * inv_ds, tb = ((float)((SX) + 1) - bsf) * inv_ds;                  \
            const int j0 = (int)ceilf(fminf(ta, tb) - 5e-3f);                                                              \
            int64_t sx = bs0 + (int64_t)j0 * fds - ((int64_t)(SX) << 32), sl = bl0 + (int64_t)j0 * fdl;                    \
            float wx[3], fl[3];                                                                                            \
            int hl[3];                                                                                                     \
            _Pragma("unroll") for (int mth = 0; mth < 3; ++mth) {                                                          \
                const int hx = (int)(sx >> 32);                                                                            \
                const float fx = (float)(unsigned)sx * two_m32;                                                            \
                float w = hx == -1 ? fx : (hx == 0 ? 1.f - fx : 0.f);                                                      \
                w = (unsigned)(j0 + mth) < (unsigned)n_smp ? w : 0.f;                                                      \
                wx[mth] = w;                                                                                               \
                hl[mth] = (int)(sl >> 32);                                                                                 \
                fl[mth] = (float)(unsigned)sl * two_m32;                                                                   \
                if (w > 0.f) L0 = min(L0, hl[mth]);                                                                        \
                sx += fds; sl += fdl;                                                                                      \
            }                                                                                                              \
            _Pragma("unroll") for (int mth = 0; mth < 3; ++mth) {                                                          \
                const int rel = hl[mth] - L0;                                                                              \
                const float wl1 = wx[mth] * fl[mth], wl0 = wx[mth] - wl1;                                                  \
                _Pragma("unroll") for (int k = 0; k < NW; ++k) W[k] += rel == k ? wl0 : (rel == k - 1 ? wl1 : 0.f);        \
            }                                                                                                              \
            bool any = false;                                                                                              \
            _Pragma("unroll") for (int k = 0; k < NW; ++k) {                                                               \
                W[k] = (unsigned)(L0 + k) < (unsigned)nL ? W[k] : 0.f;                                                     \
                any |= W[k] != 0.f;                                                                                        \
            }                                                                                                              \
            if (!any) L0 = FG_NONE;                                                                                        \
        }                                                                                                                  \
        wtab[BUF][SLOT][lane] = make_float4(W[0], W[1], W[2], W[3]);                                                       \
        ltab[BUF][SLOT][lane] = L0;                                                                                        \
    }
    // ---- 2. slab SX's first window.  FG_SETUP fetches the table entry and ISSUES the loads of the lines (lane = plane); FG_STAGE writes them to the
    //         wave's LDS rows.  The slab before SX accumulates between the two: the loads fly meanwhile, and the registers yv[] live only from
    //         the one to the other, inside one pass of the slab loop -- nothing of them is carried round the loop, so a block of four that is
    //         not loaded holds nothing (no "old value" to keep) and a loaded one is stored from the registers it arrived in.
    //         Addresses: a buffer resource over the SLAB (its base is wave-uniform; a slab's lines end slab_bytes behind it: an x slab is
    //         ny lines in a row, a y slab reaches from its first line to the last x's); the lane's plane offset is the vector offset, the
    //         line's byte offset (clamped line x line pitch, computed by FGROWS lanes at once and handed out with v_readlane) is the SCALAR
    //         offset of the load -- no add per line.  Every offset is clamped to the slab here; the resource's own range check is never
    //         relied on.  (Not one resource over the volume: a resource holds at most 2^32 - 1 bytes, and the last voxel of a volume of
    //         exactly 4 GiB, which the host admits, would lie outside it and read as zero.)
    const uint32_t slab_bytes = (uint32_t)min(WALKY ? (unsigned long long)(g.nx - 1) * strideL4 + (unsigned long long)g.nz * 4ull
                                                    : (unsigned long long)g.ny * g.nz * 4ull, 0xffffffffull);
#ifdef TOMO_ABLATE_FWD_SLAB_LO      /* measurement builds only: every slab's lines are fetched from the wave's FIRST slab (wrong sums) -- the same */
#define FG_SLAB_RSRC(SX) __builtin_amdgcn_make_buffer_rsrc((void *)(vol + (size_t)(s_lo) * strideS), 0, (int)slab_bytes, 0x00020000)   /* instructions, LDS traffic and loads, every line from the cache */
#else
#define FG_SLAB_RSRC(SX) __builtin_amdgcn_make_buffer_rsrc((void *)(vol + (size_t)(SX) * strideS), 0, (int)slab_bytes, 0x00020000)
#endif
#define FG_LINE_LOAD(RS, SOFF) __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32((RS), o0, (SOFF), 0))
#define FG_SETUP(SX, BUF, SLOT)                                                                                            \
    {                                                                                                                      \
        tn = wtab[BUF][SLOT][lane];                                                                                        \
        Ln = ltab[BUF][SLOT][lane];                                                                                        \
        Llo_n = __builtin_amdgcn_readfirstlane(gwave_min_i32(Ln));                                                         \
        Lhi_n = __builtin_amdgcn_readfirstlane(gwave_max_i32(Ln == FG_NONE ? -FG_NONE : Ln));                              \
        need_n = 0;                                                                                                        \
        if (Llo_n != FG_NONE) {                                                                                            \
            const __amdgpu_buffer_rsrc_t srs = FG_SLAB_RSRC(SX);                                                           \
            const uint32_t lineoff = (uint32_t)min(max(Llo_n + min(lane, FGROWS - 1), 0), nL - 1) * strideL4;              \
            /* only the lines the wave needs, in blocks of four (wave-uniform branches): 17 of the 24 on average */        \
            need_n = min(Lhi_n - Llo_n + NW, FGROWS);                                                                      \
            _Pragma("unroll") for (int r4 = 0; r4 < FGROWS; r4 += 4)                                                       \
                if (r4 < need_n) {                                                                                         \
                    _Pragma("unroll") for (int r = r4; r < r4 + 4; ++r)                                                    \
                        yv[r] = FG_LINE_LOAD(srs, (uint32_t)__builtin_amdgcn_readlane((int)lineoff, r));                   \
                }                                                                                                          \
        }                                                                                                                  \
    }
    // (rows past need_n keep stale values: a lane reads rows L - Llo .. + NW - 1 < need_n, one outside the window rows 0 .. NW - 1; planes
    //  past the volume are zeros; need_n = 0 when no lane has a line in the slab)
#define FG_STAGE                                                                                                           \
    {                                                                                                                      \
        if (mz == ~0ull) {                                                                                                 \
            _Pragma("unroll") for (int r4 = 0; r4 < FGROWS; r4 += 4)                                                       \
                if (r4 < need_n) {                                                                                         \
                    _Pragma("unroll") for (int r = r4; r < r4 + 4; ++r) wrows[r * GPITCH + lane] = yv[r];                  \
                }                                                                                                          \
        } else {                                                                                                           \
            _Pragma("unroll") for (int r4 = 0; r4 < FGROWS; r4 += 4)                                                       \
                if (r4 < need_n) {                                                                                         \
                    _Pragma("unroll") for (int r = r4; r < r4 + 4; ++r) wrows[r * GPITCH + lane] = select_lanes(yv[r], mz); \
                }                                                                                                          \
        }                                                                                                                  \
    }
    // ---- 3. accumulate the lanes whose lines lie in the window that starts at line LBASE
#define FG_ACCUM(LBASE)                                                                                                    \
    {                                                                                                                      \
        const int rel = L - (LBASE);                                                                                       \
        const bool inw = (unsigned)rel < (unsigned)SW;                                                                     \
        const int slot0 = inw ? rel : 0;                                                                                   \
        const float W0 = inw ? t.x : 0.f, W1 = inw ? t.y : 0.f, W2 = inw ? t.z : 0.f, W3 = inw ? t.w : 0.f;                \
        const float4 *q = (const float4 *)__builtin_assume_aligned(wrows + slot0 * GPITCH, 16);                            \
        float4 n0 = q[0], n1 = q[GPITCH / 4], n2 = q[2 * GPITCH / 4], n3 = {0.f, 0.f, 0.f, 0.f};                           \
        if (NW == 4) n3 = q[3 * GPITCH / 4];                                                                               \
        _Pragma("unroll") for (int p = 0; p < 64; p += 4) {                                                                \
            const float4 r0 = n0, r1 = n1, r2 = n2, r3 = n3;                                                               \
            if (p + 4 < 64) {                                                                                              \
                n0 = q[(p + 4) / 4]; n1 = q[(GPITCH + p + 4) / 4]; n2 = q[(2 * GPITCH + p + 4) / 4];                       \
                if (NW == 4) n3 = q[(3 * GPITCH + p + 4) / 4];                                                             \
            }                                                                                                              \
            f32x2 a = W2 * f32x2{r2.x, r2.y} + (W1 * f32x2{r1.x, r1.y} + (W0 * f32x2{r0.x, r0.y} + acc2[p / 2]));          \
            f32x2 b = W2 * f32x2{r2.z, r2.w} + (W1 * f32x2{r1.z, r1.w} + (W0 * f32x2{r0.z, r0.w} + acc2[p / 2 + 1]));      \
            if (NW == 4) { a = W3 * f32x2{r3.x, r3.y} + a; b = W3 * f32x2{r3.z, r3.w} + b; }                               \
            acc2[p / 2] = a; acc2[p / 2 + 1] = b;                                                                          \
            __builtin_amdgcn_sched_barrier(0);                                                                             \
        }                                                                                                                  \
    }
    // the walk: slabs s_lo .. s_hi - 1, ascending, in groups of nl from s_lo on
    const int n_grp = (s_hi - s_lo + nl - 1) / nl;
    int buf = 0;
    FG_TABLE(s_lo + rk, 0, rk)
    __syncthreads();
    float4 t;                                                             // the slab whose first window is in the LDS rows
    int L, Llo, Lhi;
    {
        float4 tn;
        int Ln, Llo_n, Lhi_n, need_n;
        float yv[FGROWS];
        FG_SETUP(s_lo, 0, 0)
        FG_STAGE
        t = tn; L = Ln; Llo = Llo_n; Lhi = Lhi_n;
    }
    for (int grp = 0; grp < n_grp; ++grp) {
        const int nbuf = buf == 2 ? 0 : buf + 1;
        if (grp + 1 < n_grp) FG_TABLE(s_lo + (grp + 1) * nl + rk, nbuf, rk)
        __syncthreads();
        const int g0 = s_lo + grp * nl, g1 = min(s_hi, g0 + nl);
        for (int sx = g0; sx < g1; ++sx) {
            float4 tn = t;
            int Ln = L, Llo_n = FG_NONE, Lhi_n = 0, need_n = 0;
            float yv[FGROWS];
            if (sx + 1 < s_hi) {
                const bool same = sx + 1 < g1;                            // else the next group's table, already published
                const int sbuf = same ? buf : nbuf, sslot = same ? sx + 1 - g0 : 0;
                FG_SETUP(sx + 1, sbuf, sslot)
            }
            if (Llo != FG_NONE) {
                FG_ACCUM(Llo)
                // further windows: lines loaded on the spot, four at a time (the registers yv hold the next slab's loads in flight)
                for (int lb = Llo + SW; lb <= Lhi; lb += SW) {
                    const __amdgpu_buffer_rsrc_t srs = FG_SLAB_RSRC(sx);
                    for (int r = 0; r < FGROWS; r += 4) {
                        float e[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) e[k] = FG_LINE_LOAD(srs, (uint32_t)min(max(lb + r + k, 0), nL - 1) * strideL4);
#pragma unroll
                        for (int k = 0; k < 4; ++k) wrows[(r + k) * GPITCH + lane] = select_lanes(e[k], mz);
                    }
                    FG_ACCUM(lb)
                }
            }
            FG_STAGE
            t = tn; L = Ln; Llo = Llo_n; Lhi = Lhi_n;
        }
        buf = nbuf;
    }
#undef FG_TABLE
#undef FG_SLAB_RSRC
#undef FG_LINE_LOAD
#undef FG_SETUP
#undef FG_STAGE
#undef FG_ACCUM
    // ---- z lerp and store: ray iz = Z - zc takes (1 - tau) S(Z) + tau S(Z + 1); the lane's 64 values are consecutive floats of its sinogram row
    if (!ray_ok) return;
    const int iz0 = z0 - c.zc;
    float *dst = proj + (size_t)c.slot * ((size_t)g.ndx * g.ndz) + (size_t)ix * g.ndz + iz0;
    const float tau = c.tau;
    if (tau == 0.f) {
        if (iz0 >= 0 && iz0 + 64 <= g.ndz && ((iz0 | g.ndz) & 3) == 0) {
#pragma unroll
            for (int p = 0; p < 64; p += 4) *(float4 *)(dst + p) = make_float4(acc2[p / 2].x, acc2[p / 2].y, acc2[p / 2 + 1].x, acc2[p / 2 + 1].y);
        } else {
#pragma unroll
            for (int p = 0; p < 64; ++p)
                if ((unsigned)(iz0 + p) < (unsigned)g.ndz) dst[p] = (p & 1) ? acc2[p / 2].y : acc2[p / 2].x;
        }
    } else {
        const float wfz = 1.f - tau;
#define FG_S(P) (((P) & 1) ? acc2[(P) / 2].y : acc2[(P) / 2].x)
#pragma unroll
        for (int p = 0; p < 63; ++p)
            if ((unsigned)(iz0 + p) < (unsigned)g.ndz) dst[p] = wfz * FG_S(p) + tau * FG_S(p + 1);
        // the two values shared with the neighbouring chunks' waves: one atomic from each side onto the caller's zero
        if ((unsigned)(iz0 + 63) < (unsigned)g.ndz) atomicAdd(dst + 63, wfz * FG_S(63));
        if ((unsigned)(iz0 - 1) < (unsigned)g.ndz) atomicAdd(dst - 1, tau * FG_S(0));
#undef FG_S
    }
}

// One launch per forward call: the work-groups of the four lists (x walk NW 3 | x walk NW 4 | y walk NW 3 | y walk NW 4, each fg_list_wgs()
// work-groups, see the body) follow each other in the grid; a work-group finds its list from its index and runs that instantiation.
__global__ __launch_bounds__(GWAVES * 64, 3) void k_fwd_gather_flat(const GfC *__restrict__ cs, const int *__restrict__ perm, int n0, int n1, int n2, int n3,
                                                                    int patched, float *__restrict__ proj, const float *__restrict__ vol, TomoGeomC g,
                                                                    const unsigned char *__restrict__ vflags, const int *__restrict__ zshift)
{
    __shared__ __attribute__((aligned(16))) float rows[GWAVES][FGROWS * GPITCH];
    __shared__ float4 wtab[3][GWAVES][64];          // [group mod 3][slab of the group][ray] = W0 .. W3
    __shared__ int ltab[3][GWAVES][64];             //                                      = L0
    __shared__ int wlive[GWAVES];
    const int nrt = (g.ndx + 7) / 8, nzq = (g.nz + 64 * GWAVES - 1) / (64 * GWAVES) + 1;
    const unsigned w0 = (unsigned)fg_list_wgs(n0, nrt, nzq, patched), w1 = (unsigned)fg_list_wgs(n1, nrt, nzq, patched),
                   w2 = (unsigned)fg_list_wgs(n2, nrt, nzq, patched);         // (the host launches only grids below 2^31)
    unsigned b = blockIdx.x;
    if (b < w0) { fwd_gather_flat_body<3, 0>(cs, perm, n0, b, patched, proj, vol, g, vflags, zshift, rows, wtab, ltab, wlive); return; }
    b -= w0;
    if (b < w1) { fwd_gather_flat_body<4, 0>(cs, perm + n0, n1, b, patched, proj, vol, g, vflags, zshift, rows, wtab, ltab, wlive); return; }
    b -= w1;
    if (b < w2) { fwd_gather_flat_body<3, 1>(cs, perm + n0 + n1, n2, b, patched, proj, vol, g, vflags, zshift, rows, wtab, ltab, wlive); return; }
    b -= w2;
    fwd_gather_flat_body<4, 1>(cs, perm + n0 + n1 + n2, n3, b, patched, proj, vol, g, vflags, zshift, rows, wtab, ltab, wlive);
}
