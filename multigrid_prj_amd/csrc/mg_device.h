// mg_device.h -- the small device helpers every kernel file shares (gfx950, wave64). Included by the .hip files only:
// it needs the HIP device builtins. Everything here is stateless and force-inlined, so a kernel's code is what it was
// with a private copy -- but there is ONE copy, because each of these carries part of the bit-for-bit contract:
//
//  * Norms and dot products: per-thread accumulation in double -> wave_sum (the shuffle tree 32, 16, .. 1: lane l adds
//    lane l + off) -> one double per wave in LDS, added by thread 0 in ascending wave order -> one partial per
//    workgroup in global memory -> a second kernel (k_reduce_final, k_cg_tail) that adds the partials in a fixed order.
//    No atomics: a sum is reproducible run to run, whatever kernel produced its partials.
//  * Whole-wave shifts by one lane (lane_from_prev / lane_from_next): the lane at the open end keeps `edge`
//    (bound_ctrl off, all rows and banks enabled), which is how the x-neighbour across a wave boundary gets in.
//  * A lane owns one aligned 16-byte vector of x (Vec16). On rows with an odd last column (n = 2^k + 1) that column is
//    written as ONE full 128-byte line -- its value, then the zeros the padding columns hold -- by lanes 56 .. 63 of
//    the wave that holds the row's last full vector, non-temporal like the rest of the row. That store and its
//    `tailwave` test stay written out in each kernel: moved into functions here they compile to the same operations
//    in another order and register assignment, and the kernels' instruction streams are kept exactly as they were.
//  * Workgroups are renumbered so that each of the 8 XCDs (own L2) takes a contiguous run of the work (xcd_block).
#ifndef MG_DEVICE_H
#define MG_DEVICE_H

#include <hip/hip_runtime.h>
#include "mg_geom.h"

namespace mg {

// element index of (z, y, x) in a level's padded array
__device__ __forceinline__ long long lidx(const Geom &g, int z, int y, int x)
{
    return (long long)z * g.plane + (long long)y * g.pitch + x;
}

// the lane's 16-byte vector of T: n elements
template <typename T> struct Vec16;
template <> struct Vec16<double> { static constexpr int n = 2; typedef double type __attribute__((ext_vector_type(2))); };
template <> struct Vec16<float> { static constexpr int n = 4; typedef float type __attribute__((ext_vector_type(4))); };

// sum over the wave; valid in lane 0
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Sum over a one-dimensional workgroup; valid in thread 0 (0 elsewhere). sh: one double per wave; it ends with a barrier,
// so sh can be handed to the next sum at once. (k_sweep3d and k_pairw end with the same sum written out, with their
// compile-time wave counts and no closing barrier: through this function their instruction streams came out reordered.)
__device__ __forceinline__ double block_sum(double v, double *sh)
{
    const int nw = blockDim.x >> 6;
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < nw; w++) s += sh[w];
    __syncthreads();
    return s;
}

// sum over a workgroup of any shape; every thread gets the same value. sh: >= 18 doubles.
__device__ __forceinline__ double block_sum_bcast(double v, double *sh)
{
    const int tid = threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z);
    const int nthreads = blockDim.x * blockDim.y * blockDim.z;
    const int nw = (nthreads + 63) >> 6;
    v = wave_sum(v);
    if ((tid & 63) == 0) sh[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        double s = 0;
        for (int w = 0; w < nw; w++) s += sh[w];
        sh[17] = s;
    }
    __syncthreads();
    double r = sh[17];
    __syncthreads();
    return r;
}

// lane i <- lane i-1 (lane 0 keeps `edge`): DPP wave_shr:1
__device__ __forceinline__ float lane_from_prev(float v, float edge)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ double lane_from_prev(double v, double edge)
{
    int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(v), 0x138, 0xf, 0xf, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(v), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// lane i <- lane i+1 (lane 63 keeps `edge`): DPP wave_shl:1
__device__ __forceinline__ float lane_from_next(float v, float edge)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x130, 0xf, 0xf, false));
}
__device__ __forceinline__ double lane_from_next(double v, double edge)
{
    int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(v), 0x130, 0xf, 0xf, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(v), 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// XCD-aware order: consecutive blockIdx go to the 8 XCDs in turn, so XCD k takes work items k * per .. (k + 1) * per - 1
__device__ __forceinline__ int xcd_block(unsigned b, int per) { return (int)(b & 7) * per + (int)(b >> 3); }

}  // namespace mg
#endif
