// mg_mixed.hip -- fine-grid kernels of the mixed-precision defect correction (mg_mixed_solve, include/mg_hip.h;
// driver: Solver::mixed_solve in mg_solver.cpp): the solution u and the right-hand side b live in fp64, the multigrid
// cycles that solve A e = r run in the handle's fp32 hierarchy.
//
//   k_mixed_residual          r = b - A u in fp64, written as (float)(s_out r); partial sums of r^2      8+8 R, 4 W per node
//   k_mixed_correct_residual  u' = u + (double)e / s_in (interior), the same residual of u'              8+4+8 R, 8+4 W
//   k_mixed_sumsq             partial sums of b^2
// The fused kernel needs u' at the stencil neighbours, so it forms u + e / s_in for each of them from u and e and stores
// the centre one. u' is written OUT OF PLACE (another workgroup may still read u at a neighbour); the driver swaps the
// two pointers. One pass of 32 B per node instead of 40 B for a correction kernel followed by a residual kernel.
//
// Layout: two pitches. The fp64 arrays use the fp64 geometry of level 0 (rows padded to 128 B of doubles), the fp32 arrays
// the handle's own; a lane owns FOUR consecutive nodes of a row -- two 16-byte accesses of an fp64 array, one of an fp32
// array -- and indexes the two kinds of array separately. Workgroups of 256 lanes, at most 2048 of them striding over the
// level; padding columns (x >= nx) are neither written nor summed; one partial sum per workgroup, added in a fixed order
// by k_reduce_final: two runs give the same bits (no atomics).
//
// Arithmetic contract (compiled with -ffp-contract=off, tests/test_mixed_gpu.py restates it in numpy), all in fp64:
//   u' = u + (double)e / s_in   inside;  u' = u on Dirichlet nodes (e is not looked at there)
//   r  = 0 on Dirichlet nodes; inside, in the residual kernel's row order,
//        r = b - (((((((0 + cz u'[k-1]) + cy u'[j-1]) + cx u'[i-1]) + cd u') + cx u'[i+1]) + cy u'[j+1]) + cz u'[k+1])
//   r32 = (float)(s_out * r), round to nearest even;  sum of r^2 (unscaled) in double
// When s_in is a power of two with a normal reciprocal (what the driver always passes) the division is done as a
// multiplication by that reciprocal: the same correctly rounded quotient, bit for bit. Any other s_in takes the division.
#include "mg_kernels.h"
#include "mg_device.h"

namespace mg {

namespace {

constexpr int MX_THREADS = 256;
constexpr int MX_MAX_BLOCKS = 2048;
constexpr int MX_V = 4;   // nodes per lane

__device__ __forceinline__ void ld4(const double *p, double (&v)[MX_V])
{
    const double2 a = *reinterpret_cast<const double2 *>(p), b = *reinterpret_cast<const double2 *>(p + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}

__device__ __forceinline__ void ld4(const float *p, float (&v)[MX_V])
{
    const float4 a = *reinterpret_cast<const float4 *>(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}

// stores the first `valid` nodes (whole 16-byte stores when the lane's four nodes lie inside the row)
__device__ __forceinline__ void st4(double *p, const double (&v)[MX_V], int valid)
{
    if (valid >= MX_V) {
        *reinterpret_cast<double2 *>(p) = make_double2(v[0], v[1]);
        *reinterpret_cast<double2 *>(p + 2) = make_double2(v[2], v[3]);
        return;
    }
#pragma unroll
    for (int e = 0; e < MX_V; e++)
        if (e < valid) p[e] = v[e];
}

__device__ __forceinline__ void st4(float *p, const float (&v)[MX_V], int valid)
{
    if (valid >= MX_V) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); return; }
#pragma unroll
    for (int e = 0; e < MX_V; e++)
        if (e < valid) p[e] = v[e];
}

struct MixedCoef {
    double cx, cy, cz, cd;
};

// u + e / s;  DIV == false: t holds 1 / s exactly (s a power of two), the product is the same correctly rounded quotient
template <bool DIV>
__device__ __forceinline__ double corrected(double u, float e, double t)
{
    return DIV ? u + (double)e / t : u + (double)e * t;
}

// the (corrected) values of the lane's four nodes in the row at (i64, i32); `dirichlet_row`: a Dirichlet row / plane,
// taken uncorrected. Only used for the y / z neighbours of interior nodes, whose x is interior too.
template <bool CORR, bool DIV>
__device__ __forceinline__ void neighbour_row(const double *u, const float *e, long long i64, long long i32, bool dirichlet_row,
                                              double t, double (&out)[MX_V])
{
    ld4(u + i64, out);
    if (CORR && !dirichlet_row) {
        float ev[MX_V];
        ld4(e + i32, ev);
#pragma unroll
        for (int k = 0; k < MX_V; k++) out[k] = corrected<DIV>(out[k], ev[k], t);
    }
}

template <int DIM, bool CORR, bool DIV>
__device__ __forceinline__ void mixed_body(const Geom &g, const Geom &g32, const MixedCoef &c, const double *__restrict__ u,
                                           const float *__restrict__ e, const double *__restrict__ b, double *__restrict__ un,
                                           float *__restrict__ r32, double t_in, double s_out, double *__restrict__ partials, double *sh)
{
    const unsigned vpr = (unsigned)((g.nx + MX_V - 1) / MX_V), nitems = vpr * (unsigned)g.ny * (unsigned)g.nz;
    double acc = 0.;
    for (unsigned it = blockIdx.x * MX_THREADS + threadIdx.x; it < nitems; it += gridDim.x * MX_THREADS) {
        const unsigned row = it / vpr;
        const int x0 = (int)(it - row * vpr) * MX_V, y = (int)(row % (unsigned)g.ny), z = (int)(row / (unsigned)g.ny);
        const int valid = g.nx - x0;   // >= 1
        const long long i64 = (long long)z * g.plane + (long long)y * g.pitch + x0;
        const long long i32 = (long long)z * g32.plane + (long long)y * g32.pitch + x0;
        float rv[MX_V] = {0.f, 0.f, 0.f, 0.f};
        double uc[MX_V];
        bool dirichlet_row = (y == 0) | (y == g.ny - 1);
        if (DIM == 3) dirichlet_row |= (z == 0) | (z == g.nz - 1);
        if (dirichlet_row) {
            if (CORR) { ld4(u + i64, uc); st4(un + i64, uc, valid); }
            st4(r32 + i32, rv, valid);
            continue;
        }
        ld4(u + i64, uc);
        if (CORR) {
            float ev[MX_V];
            ld4(e + i32, ev);
#pragma unroll
            for (int k = 0; k < MX_V; k++) {
                const int xx = x0 + k;
                if (xx >= 1 && xx <= g.nx - 2) uc[k] = corrected<DIV>(uc[k], ev[k], t_in);
            }
        }
        double us[MX_V], unn[MX_V], ud[MX_V], uu[MX_V];
        neighbour_row<CORR, DIV>(u, e, i64 - g.pitch, i32 - g32.pitch, y - 1 == 0, t_in, us);
        neighbour_row<CORR, DIV>(u, e, i64 + g.pitch, i32 + g32.pitch, y + 1 == g.ny - 1, t_in, unn);
        if (DIM == 3) {
            neighbour_row<CORR, DIV>(u, e, i64 - g.plane, i32 - g32.plane, z - 1 == 0, t_in, ud);
            neighbour_row<CORR, DIV>(u, e, i64 + g.plane, i32 + g32.plane, z + 1 == g.nz - 1, t_in, uu);
        }
        // x-neighbours across the lane's ends: one node each, uncorrected on the Dirichlet columns
        double ul = 0., ur = 0.;
        if (x0 > 0) {
            ul = u[i64 - 1];
            if (CORR && x0 - 1 >= 1) ul = corrected<DIV>(ul, e[i32 - 1], t_in);
        }
        if (x0 + MX_V <= g.nx - 1) {
            ur = u[i64 + MX_V];
            if (CORR && x0 + MX_V <= g.nx - 2) ur = corrected<DIV>(ur, e[i32 + MX_V], t_in);
        }
        double bv[MX_V];
        ld4(b + i64, bv);
#pragma unroll
        for (int k = 0; k < MX_V; k++) {
            const int xx = x0 + k;
            if (xx == 0 || xx >= g.nx - 1) continue;   // Dirichlet column (r = 0) or padding
            const double w = k == 0 ? ul : uc[k - 1 < 0 ? 0 : k - 1];
            const double ea = k == MX_V - 1 ? ur : uc[k + 1 > MX_V - 1 ? MX_V - 1 : k + 1];
            double s = 0.;
            if (DIM == 3) s += c.cz * ud[k];
            s += c.cy * us[k];
            s += c.cx * w;
            s += c.cd * uc[k];
            s += c.cx * ea;
            s += c.cy * unn[k];
            if (DIM == 3) s += c.cz * uu[k];
            const double r = bv[k] - s;
            acc += r * r;
            rv[k] = (float)(s_out * r);
        }
        if (CORR) st4(un + i64, uc, valid);
        st4(r32 + i32, rv, valid);
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

template <int DIM>
__global__ __launch_bounds__(MX_THREADS) void k_mixed_residual(Geom g, Geom g32, MixedCoef c, const double *__restrict__ u,
                                                               const double *__restrict__ b, float *__restrict__ r32,
                                                               double s_out, double *__restrict__ partials)
{
    __shared__ double sh[MX_THREADS / 64];
    mixed_body<DIM, false, false>(g, g32, c, u, nullptr, b, nullptr, r32, 1.0, s_out, partials, sh);
}

template <int DIM, bool DIV>
__global__ __launch_bounds__(MX_THREADS) void k_mixed_correct_residual(Geom g, Geom g32, MixedCoef c, const double *__restrict__ u,
                                                                       const float *__restrict__ e, const double *__restrict__ b,
                                                                       double *__restrict__ un, float *__restrict__ r32,
                                                                       double t_in, double s_out, double *__restrict__ partials)
{
    __shared__ double sh[MX_THREADS / 64];
    mixed_body<DIM, true, DIV>(g, g32, c, u, e, b, un, r32, t_in, s_out, partials, sh);
}

__global__ __launch_bounds__(MX_THREADS) void k_mixed_sumsq(Geom g, const double *__restrict__ v, double *__restrict__ partials)
{
    __shared__ double sh[MX_THREADS / 64];
    const unsigned vpr = (unsigned)((g.nx + MX_V - 1) / MX_V), nitems = vpr * (unsigned)g.ny * (unsigned)g.nz;
    double acc = 0.;
    for (unsigned it = blockIdx.x * MX_THREADS + threadIdx.x; it < nitems; it += gridDim.x * MX_THREADS) {
        const unsigned row = it / vpr;
        const int x0 = (int)(it - row * vpr) * MX_V, y = (int)(row % (unsigned)g.ny), z = (int)(row / (unsigned)g.ny);
        double w[MX_V];
        ld4(v + (long long)z * g.plane + (long long)y * g.pitch + x0, w);
#pragma unroll
        for (int k = 0; k < MX_V; k++)
            if (x0 + k < g.nx) acc += w[k] * w[k];
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

int mixed_grid(const Geom &g)
{
    const long long items = (long long)((g.nx + MX_V - 1) / MX_V) * g.ny * g.nz;
    return (int)std::min<long long>(MX_MAX_BLOCKS, std::max<long long>(1, (items + MX_THREADS - 1) / MX_THREADS));
}

}  // namespace

int mixed_partials_capacity() { return MX_MAX_BLOCKS; }

int launch_mixed_residual(hipStream_t s, const Geom &g64, const Geom &g32, const double coef[4], const double *u, const double *b,
                          float *r32, double scale_out, double *partials)
{
    const int nb = mixed_grid(g64);
    const MixedCoef c{coef[0], coef[1], coef[2], coef[3]};
    if (g64.dim == 3)
        hipLaunchKernelGGL((k_mixed_residual<3>), dim3(nb), dim3(MX_THREADS), 0, s, g64, g32, c, u, b, r32, scale_out, partials);
    else
        hipLaunchKernelGGL((k_mixed_residual<2>), dim3(nb), dim3(MX_THREADS), 0, s, g64, g32, c, u, b, r32, scale_out, partials);
    return nb;
}

int launch_mixed_correct_residual(hipStream_t s, const Geom &g64, const Geom &g32, const double coef[4], const double *u,
                                  const float *e32, const double *b, double *u_out, float *r32, double scale_in, double scale_out,
                                  double *partials)
{
    const int nb = mixed_grid(g64);
    const MixedCoef c{coef[0], coef[1], coef[2], coef[3]};
    // a power of two whose reciprocal is a normal number: multiply by the (exact) reciprocal instead of dividing
    int ex = 0;
    const double inv = 1.0 / scale_in;
    const bool pow2 = scale_in > 0.0 && std::isfinite(scale_in) && std::frexp(scale_in, &ex) == 0.5 && std::isnormal(scale_in) &&
                      std::isnormal(inv);
#define MG_MX(DIM, DIV, T)                                                                                                   \
    hipLaunchKernelGGL((k_mixed_correct_residual<DIM, DIV>), dim3(nb), dim3(MX_THREADS), 0, s, g64, g32, c, u, e32, b, u_out, \
                       r32, T, scale_out, partials)
    if (g64.dim == 3) { if (pow2) MG_MX(3, false, inv); else MG_MX(3, true, scale_in); }
    else { if (pow2) MG_MX(2, false, inv); else MG_MX(2, true, scale_in); }
#undef MG_MX
    return nb;
}

int launch_mixed_sumsq(hipStream_t s, const Geom &g64, const double *v, double *partials)
{
    const int nb = mixed_grid(g64);
    hipLaunchKernelGGL(k_mixed_sumsq, dim3(nb), dim3(MX_THREADS), 0, s, g64, v, partials);
    return nb;
}

}  // namespace mg
