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

// ---- the generic per-point expressions and the one-workgroup passes built on them ---------------------------------------
// Shared by the generic kernels (mg_kernels.hip) and the LDS sub-cycle (mg_subcycle.hip): the operand order of every sum
// below is the bit-for-bit contract with oracle/, so there is one copy. The passes take any Geom -- a level in HBM or a
// dense copy of it in LDS (pitch = nx, plane = nx * ny).
__device__ __forceinline__ bool on_boundary(const Geom &g, int z, int y, int x)
{
    // reference src/domain.cpp:20-23, extended to the slab-decomposed z axis
    bool b = (x == 0) | (y == 0) | (x == g.nx - 1) | (y == g.ny - 1);
    if (g.dim == 3) {
        int gz = g.gz0 + z;
        b |= (gz == 0) | (gz == g.gnz - 1);
    }
    return b;
}

template <typename T, int DIM>
__device__ __forceinline__ T offdiag_sum(const T *u, long long i, int pitch,
                                         long long plane, const Coef<T> &c)
{
    T sum = 0;
    if (DIM == 3) sum += c.cz * u[i - plane];
    sum += c.cy * u[i - pitch];
    sum += c.cx * u[i - 1];
    sum += c.cx * u[i + 1];
    sum += c.cy * u[i + pitch];
    if (DIM == 3) sum += c.cz * u[i + plane];
    return sum;
}

template <typename T, int DIM>
__device__ __forceinline__ T full_sum(const T *u, long long i, int pitch,
                                      long long plane, const Coef<T> &c)
{
    // Residual: diagonal included, in row order (solvers.hpp:269-271)
    T sum = 0;
    if (DIM == 3) sum += c.cz * u[i - plane];
    sum += c.cy * u[i - pitch];
    sum += c.cx * u[i - 1];
    sum += c.cd * u[i];
    sum += c.cx * u[i + 1];
    sum += c.cy * u[i + pitch];
    if (DIM == 3) sum += c.cz * u[i + plane];
    return sum;
}

template <typename T, int DIM, bool DAMPED>
__device__ __forceinline__ T point_update(const Geom &g, const Coef<T> &c, T omega,
                                          const T *u, const T *rhs, int z, int y, int x)
{
    long long i = lidx(g, z, y, x);
    T b = rhs[i];
    if (on_boundary(g, z, y, x)) return b;  // (b - 0) / 1
    T sum = offdiag_sum<T, DIM>(u, i, g.pitch, g.plane, c);
    T jac = div_cd<T>(b - sum, c);
    if (DAMPED) {
        T uc = u[i];
        return uc + omega * (jac - uc);
    }
    return jac;
}


// Interpolated value at fine node (zf,yf,xf), built in the reference's phase order
// (src/multigrid.cpp:3-27; slow axis first, fast axis last) so that every fine node
// gets bit for bit what the in-place sequential phases produce.
// DIM == 23: 3-D semi-coarsening (planes map one to one, gzf is then the LOCAL plane index)
template <typename T, int DIM>
__device__ __forceinline__ T interp_z(const Geom &gc, const T *__restrict__ c, int gzf, int yc,
                                      int xc)
{
    if (DIM == 2) return c[lidx(gc, 0, yc, xc)];
    if (DIM == 23) return c[lidx(gc, gzf, yc, xc)];
    if ((gzf & 1) == 0) return c[lidx(gc, (gzf >> 1) - gc.gz0, yc, xc)];
    int k0 = ((gzf - 1) >> 1) - gc.gz0;
    return (T)0.5 * (c[lidx(gc, k0, yc, xc)] + c[lidx(gc, k0 + 1, yc, xc)]);
}
template <typename T, int DIM>
__device__ __forceinline__ T interp_y(const Geom &gc, const T *__restrict__ c, int gzf, int yf,
                                      int xc)
{
    if ((yf & 1) == 0) return interp_z<T, DIM>(gc, c, gzf, yf >> 1, xc);
    return (T)0.5 * (interp_z<T, DIM>(gc, c, gzf, (yf - 1) >> 1, xc) +
                     interp_z<T, DIM>(gc, c, gzf, (yf + 1) >> 1, xc));
}

// Full weighting at coarse node (z, y, x): axis by axis x, y, z, the coarse boundary injected.
// WZ: weights along z too (3-D standard coarsening); otherwise 9-point weights per plane
template <typename T, int DIM, bool WZ>
__device__ __forceinline__ T restrict_fw_point(const Geom &gf, const Geom &gc, const T *__restrict__ fine, int z, int y, int x)
{
    int fz = (DIM == 3) ? (WZ ? 2 * (gc.gz0 + z) - gf.gz0 : z) : 0;
    long long fi = lidx(gf, fz, 2 * y, 2 * x);
    T out;
    if (on_boundary(gc, z, y, x)) {
        out = fine[fi];
    } else {
        const T q = (T)0.25, hlf = (T)0.5;
        T zacc[3];
#pragma unroll
        for (int dz = 0; dz < (WZ ? 3 : 1); dz++) {
            long long oz = WZ ? (long long)(dz - 1) * gf.plane : 0;
            T yacc[3];
#pragma unroll
            for (int dy = 0; dy < 3; dy++) {
                const T *p = fine + fi + oz + (long long)(dy - 1) * gf.pitch;
                yacc[dy] = q * p[-1] + hlf * p[0] + q * p[1];
            }
            zacc[dz] = q * yacc[0] + hlf * yacc[1] + q * yacc[2];
        }
        out = WZ ? q * zacc[0] + hlf * zacc[1] + q * zacc[2] : zacc[0];
    }
    return out;
}

// the value k_prolong adds to (or stores at) fine node (z, y, x)
template <typename T, int DIM>
__device__ __forceinline__ T prolong_point(const Geom &gc, const Geom &gf, const T *__restrict__ coarse, int z, int y, int x)
{
    int gzf = (DIM == 23) ? z : gf.gz0 + z;
    T v;
    if ((x & 1) == 0) v = interp_y<T, DIM>(gc, coarse, gzf, y, x >> 1);
    else v = (T)0.5 * (interp_y<T, DIM>(gc, coarse, gzf, y, (x - 1) >> 1) +
                       interp_y<T, DIM>(gc, coarse, gzf, y, (x + 1) >> 1));
    return v;
}

// ---------------------------------------------------------------- single-workgroup sweeps
// Device-side sweeps executed by ONE workgroup of 1024 threads (coarsest grid,
// and the bit-faithful lexicographic GS on any level). Each ends with a barrier.
constexpr int SWG = 1024;

template <typename T, int DIM, bool DAMPED>
__device__ void wg_jacobi(const Geom &g, const Coef<T> &c, T omega, const T *u, const T *rhs,
                          T *out)
{
    const int npl = g.nx * g.ny;
    const long long total = (long long)npl * g.nz;
    for (long long q = threadIdx.x; q < total; q += SWG) {
        int z = (int)(q / npl);
        int rem = (int)(q - (long long)z * npl);
        int y = rem / g.nx, x = rem - y * g.nx;
        out[lidx(g, z, y, x)] = point_update<T, DIM, DAMPED>(g, c, omega, u, rhs, z, y, x);
    }
    __syncthreads();
}

template <typename T, int DIM>
__device__ void wg_rbgs(const Geom &g, const Coef<T> &c, T *u, const T *rhs)
{
    const int npl = g.nx * g.ny;
    const long long total = (long long)npl * g.nz;
    for (int colour = 0; colour < 2; colour++) {
        for (long long q = threadIdx.x; q < total; q += SWG) {
            int z = (int)(q / npl);
            int rem = (int)(q - (long long)z * npl);
            int y = rem / g.nx, x = rem - y * g.nx;
            if (((x + y + g.gz0 + z) & 1) != colour) continue;
            u[lidx(g, z, y, x)] = point_update<T, DIM, false>(g, c, (T)1, u, rhs, z, y, x);
        }
        __syncthreads();
    }
}


template <typename T, int DIM>
__device__ double wg_residual_sumsq(const Geom &g, const Coef<T> &c, const T *u, const T *rhs,
                                    double *sh)
{
    const int npl = g.nx * g.ny;
    const long long total = (long long)npl * g.nz;
    double sq = 0.;
    for (long long q = threadIdx.x; q < total; q += SWG) {
        int z = (int)(q / npl);
        int rem = (int)(q - (long long)z * npl);
        int y = rem / g.nx, x = rem - y * g.nx;
        long long i = lidx(g, z, y, x);
        T sum;
        if (on_boundary(g, z, y, x)) sum = (T)1 * u[i];
        else sum = full_sum<T, DIM>(u, i, g.pitch, g.plane, c);
        T res = rhs[i] - sum;
        sq += (double)res * (double)res;
    }
    return block_sum_bcast(sq, sh);
}

template <typename T>
__device__ double wg_sumsq(const Geom &g, const T *v, double *sh)
{
    const int npl = g.nx * g.ny;
    const long long total = (long long)npl * g.nz;
    double sq = 0.;
    for (long long q = threadIdx.x; q < total; q += SWG) {
        int z = (int)(q / npl);
        int rem = (int)(q - (long long)z * npl);
        int y = rem / g.nx, x = rem - y * g.nx;
        double t = (double)v[lidx(g, z, y, x)];
        sq += t * t;
    }
    return block_sum_bcast(sq, sh);
}


}  // namespace mg
#endif
