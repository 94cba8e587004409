// Device code more than one side library has: the fixed-order block sum (libtomo_fsc.so, libtomo_vreg.so, libtomo_xcorr.so) and the
// soft spherical mask of the two libraries that window a volume before they transform it (fsc, vreg).  Internal, as tomo_side_host.h is.
#pragma once

#include <hip/hip_runtime.h>

namespace {

// Tree reduction of a sum over a work-group of N lanes in LDS (sh: N doubles), in an order that N alone fixes; every lane gets the
// total.  It begins with a barrier, so calls may follow each other, or anything else that reads sh, without one in between.
template <int N>
__device__ inline double block_sum(double v, double *sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// The mask of tomo_fsc_mask / tomo_vreg_mask (the same values: 0 none, 1 an array, 2 the soft sphere).  Where a voxel lies, and so each
// library's mask_at, depends on its own indexing.
struct Mask {
    int mode;
    const float *arr;
    double R, E;
};

// The soft sphere at squared distance d2 from the centre: 1 inside radius R, a raised-cosine edge of width E, 0 outside.  R and E are
// a Mask's members, by reference: a kernel reads them from its arguments where the formula first needs them, not ahead of the call.
__device__ inline double mask_edge(double d2, const double &R, const double &E) {
    constexpr double pi = 3.141592653589793238462643383279502884;
    if (d2 <= R * R) return 1.0;
    const double Ro = R + E;
    if (d2 >= Ro * Ro || E <= 0.0) return 0.0;
    return 0.5 * (1.0 + cos(pi * (sqrt(d2) - R) / E));
}

}  // namespace
