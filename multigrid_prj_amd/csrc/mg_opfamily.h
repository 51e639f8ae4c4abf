// mg_opfamily.h -- what the kernel files of the operator families share (mg_vc.hip, mg_bc.hip, mg_fas.hip; drivers: the
// fam_* templates of mg_drivers.cpp): the plain form, the one-workgroup coarsest-grid solve and the launch planners, written
// once over an operator functor, and the pointwise reaction of mg_fas_* (fas_react, fas_newton_point), which mg_fas.hip and --
// with MG_FAS_ON_COEFFICIENT -- mg_vc.hip add to their linear parts. The marching tiles are each family's own and stay in its file.
//
// An Op is a trivially copyable struct passed to the kernel by value. It carries what the family's point operator needs
// besides u and b (vc: VcCoef and the coefficient array a; bc: Coef and the face mask; fas: Coef and gamma, the reaction kind
// a template parameter of the Op type) and has
//     typedef ... type;                                                     the element type T
//     template <int DIM> T res(g, u, b, z, y, x) const;                     b - L u at one node (Dirichlet nodes: b - u)
//     template <int DIM> T solve(g, omega, damped, u, b, z, y, x) const;    the point solve (Dirichlet nodes: b)
//     template <int DIM> bool n0(g, u, z, y, x, stencil, v) const;          true at a Dirichlet node; else v = the operator's
//                                                                           value at the node (stencil == false: v is left alone
//                                                                           and no neighbour is loaded). The time steppers build
//                                                                           the Op with sigma = 0 / cd0: the UNSHIFTED operator
//
//   k_op_plain<Op, DIM, OP, SAVE, SRC>   OP = residual (stored with SAVE, else norm only) / Jacobi sweep (out of place) / one
//                                   red-black colour pass (in place) / the right-hand side of a theta step (OP_STEP, out of
//                                   place; SRC: with a source, read where the others read b): one thread per node,
//                                   grid-stride, every shape
//   k_op_coarse<Op, DIM>            the Solver::Solve loop of k_coarse_solve (mg_kernels.hip) in one workgroup, with the
//                                   family's sweep (wg_op_jacobi / wg_op_rbgs) and residual (wg_op_residual_sumsq)
#pragma once
#include "mg_kernels.h"
#include "mg_device.h"

#include <algorithm>

namespace mg {

constexpr int OP_THREADS = 256, OP_MAX_BLOCKS = 2048;
constexpr int MBW = 4, MRY = 2;   // waves per workgroup / rows per wave of the marching tiles
enum { OP_RES = 0, OP_JAC = 1, OP_RB = 2, OP_STEP = 3 };

// ---------------------------------------------------------------- Neumann faces (mg_bc.hip, and mg_vc.hip with a face mask)
enum { FXLO = 1, FXHI = 2, FYLO = 4, FYHI = 8, FZLO = 16, FZHI = 32 };   // enum mg_face

// the faces node (z, y, x) lies on, as mg_face bits
__device__ __forceinline__ int bc_faces(const Geom &g, int z, int y, int x)
{
    int f = (x == 0 ? FXLO : 0) | (x == g.nx - 1 ? FXHI : 0) | (y == 0 ? FYLO : 0) | (y == g.ny - 1 ? FYHI : 0);
    if (g.dim == 3) {
        const int gz = g.gz0 + z;
        f |= (gz == 0 ? FZLO : 0) | (gz == g.gnz - 1 ? FZHI : 0);
    }
    return f;
}

// element indices of the six neighbours of unknown i on faces f (all of them Neumann): the mirror image where one is missing
struct BcNb { long long zm, ym, xm, xp, yp, zp; };
__device__ __forceinline__ BcNb bc_neighbours(const Geom &g, long long i, int f)
{
    BcNb n;
    n.xm = (f & FXLO) ? i + 1 : i - 1;
    n.xp = (f & FXHI) ? i - 1 : i + 1;
    n.ym = (f & FYLO) ? i + g.pitch : i - g.pitch;
    n.yp = (f & FYHI) ? i - g.pitch : i + g.pitch;
    n.zm = (f & FZLO) ? i + g.plane : i - g.plane;
    n.zp = (f & FZHI) ? i - g.plane : i + g.plane;
    return n;
}

// w = 1/2 per Neumann face the node lies on (nf = 0 .. 3: at most one face per axis)
__device__ __forceinline__ double bc_weight(int nf) { return nf == 0 ? 1.0 : (nf == 1 ? 0.5 : (nf == 2 ? 0.25 : 0.125)); }

// full weighting at coarse node (z, y, x) with mirrored fine neighbours (k_bc_restrict, and the FAS transition with Neumann
// faces): restrict_fw_point's expression (x, then y inside the z planes, weights q, hlf, q) with the fine indices that leave
// the grid mirrored. WZ: weights along z too (3-D standard coarsening); otherwise 9-point weights per plane
template <typename T, int DIM, bool WZ>
__device__ __forceinline__ T bc_restrict_point(const Geom &gf, const Geom &gc, const T *__restrict__ fine, int z, int y, int x)
{
    const int gzf = (DIM == 3 && WZ) ? 2 * (gc.gz0 + z) : 0;   // global fine plane
    const int fz = (DIM == 3) ? (WZ ? gzf - gf.gz0 : z) : 0;
    const long long fi = lidx(gf, fz, 2 * y, 2 * x);
    const T q = (T)0.25, hlf = (T)0.5;
    // offsets of the lower and the upper fine neighbour per axis, mirrored where the index leaves the grid
    const long long oxl = (2 * x - 1 < 0) ? 1 : -1, oxh = (2 * x + 1 > gf.nx - 1) ? -1 : 1;
    const long long oyl = (2 * y - 1 < 0) ? gf.pitch : -(long long)gf.pitch, oyh = (2 * y + 1 > gf.ny - 1) ? -(long long)gf.pitch : gf.pitch;
    const long long ozl = (gzf - 1 < 0) ? gf.plane : -gf.plane, ozh = (gzf + 1 > gf.gnz - 1) ? -gf.plane : gf.plane;
    const long long oy[3] = {oyl, 0, oyh}, oz[3] = {ozl, 0, ozh};
    T zacc[3];
#pragma unroll
    for (int dz = 0; dz < (WZ ? 3 : 1); dz++) {
        T yacc[3];
#pragma unroll
        for (int dy = 0; dy < 3; dy++) {
            const T *p = fine + fi + (WZ ? oz[dz] : 0) + oy[dy];
            yacc[dy] = q * p[oxl] + hlf * p[0] + q * p[oxh];
        }
        zacc[dz] = q * yacc[0] + hlf * yacc[1] + q * yacc[2];
    }
    return WZ ? q * zacc[0] + hlf * zacc[1] + q * zacc[2] : zacc[0];
}

// The scalars of one theta step of u_t = -N0(u) + f (mg_*_heat_rhs), passed to the kernels by value:
// rdt = (T)(1 / dt), omt = (T)(1 - theta), rth = (T)(1 / theta). The other modes do not look at them.
template <typename T>
struct StepCoef {
    T rdt, omt, rth;
};

template <typename T>
StepCoef<T> step_coef(double dt, double theta)
{
    return StepCoef<T>{(T)(1.0 / dt), (T)(1.0 - theta), (T)(1.0 / theta)};
}

// the step's right-hand side at an unknown from u, the source and the unshifted operator value n0 (k_heat_rhs's expression)
template <typename T, bool SRC>
__device__ __forceinline__ T step_value(const StepCoef<T> &st, T ui, T fi, T n0)
{
    T t = st.rdt * ui;
    if (SRC) t = fi + t;
    return (t - st.omt * n0) * st.rth;
}

// ---------------------------------------------------------------- the pointwise reaction (mg_fas.hip, and mg_vc.hip with MG_FAS_ON_COEFFICIENT)
// enum mg_fas_kind (FAS_CUBIC, FAS_EXP: mg_kernels.h); FAS_LINEAR = no reaction: every use below folds away at compile time
__device__ __forceinline__ double fas_exp(double x) { return exp(x); }
__device__ __forceinline__ float fas_exp(float x) { return expf(x); }

// g(u) and g'(u)
template <typename T, int KIND>
__device__ __forceinline__ void fas_react(T u, T &gv, T &gp)
{
    if (KIND == FAS_CUBIC) {
        const T q = u * u;
        gv = q * u;
        gp = (T)3 * q;
    } else {
        gv = gp = fas_exp(u);
    }
}

// the point solve with the reaction: one Newton step around ui on the node's own equation lin_den * v + G g(v) = lin_num, from
// the numerator and the denominator of the LINEAR point solve (fas: b - s and cd; vc: b + s and d); the IEEE quotient, nothing
// guards den
template <typename T, int KIND>
__device__ __forceinline__ T fas_newton_point(T G, T lin_num, T lin_den, T ui)
{
    T gv, gp;
    fas_react<T, KIND>(ui, gv, gp);
    const T num = lin_num - G * (gv - gp * ui);
    const T den = lin_den + G * gp;
    return num / den;
}

// ---------------------------------------------------------------- the plain form
// out: r (OP_RES with SAVE), u' (OP_JAC, must not alias u), u itself (OP_RB: the other colour is only read) or the step's
// right-hand side (OP_STEP, must not alias u; b is the source, not read without SRC; theta == 1: no neighbour is loaded)
template <typename Op, int DIM, int OP, bool SAVE, bool SRC = true>
__global__ __launch_bounds__(OP_THREADS) void k_op_plain(Geom g, Op op, typename Op::type omega, int colour, const typename Op::type *u,
                                                         const typename Op::type *__restrict__ b, typename Op::type *out,
                                                         double *__restrict__ partials, StepCoef<typename Op::type> st)
{
    typedef typename Op::type T;
    __shared__ double sh[OP_THREADS / 64];
    const int hx = OP == OP_RB ? (g.nx + 1) / 2 : g.nx;   // nodes of a row this launch visits
    const long long nitems = (long long)hx * g.ny * g.nz;
    const bool damped = OP == OP_JAC && omega != (T)1;
    double acc = 0.;
    for (long long it = (long long)blockIdx.x * OP_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * OP_THREADS) {
        const long long row = it / hx;
        int x = (int)(it - row * hx);
        const int y = (int)(row % g.ny), z = (int)(row / g.ny);
        if (OP == OP_RB) {
            x = 2 * x + ((y + g.gz0 + z + colour) & 1);   // the x parity that has (x + y + gz) & 1 == colour
            if (x >= g.nx) continue;
        }
        if (OP == OP_RES) {
            const T res = op.template res<DIM>(g, u, b, z, y, x);
            acc += (double)res * (double)res;
            if (SAVE) out[lidx(g, z, y, x)] = res;
        } else if (OP == OP_STEP) {
            const long long i = lidx(g, z, y, x);
            const T ui = u[i];
            T n0 = (T)0, fi = (T)0;
            const bool fixed = op.template n0<DIM>(g, u, z, y, x, st.omt != (T)0, n0);
            if (SRC) fi = __builtin_nontemporal_load(b + i);
            __builtin_nontemporal_store(fixed ? ui : step_value<T, SRC>(st, ui, fi, n0), out + i);
        } else {
            out[lidx(g, z, y, x)] = op.template solve<DIM>(g, omega, damped, u, b, z, y, x);
        }
    }
    if (OP == OP_RES) {
        const double s = block_sum(acc, sh);
        if (threadIdx.x == 0) partials[blockIdx.x] = s;
    }
}

// ---------------------------------------------------------------- the coarsest-grid solve: one workgroup
template <typename Op, int DIM, typename T>
__device__ void wg_op_jacobi(const Geom &g, const Op &op, T omega, bool damped, const T *u, const T *rhs, T *out)
{
    const int npl = g.nx * g.ny;
    const long long total = (long long)npl * g.nz;
    for (long long q = threadIdx.x; q < total; q += SWG) {
        const int z = (int)(q / npl), rem = (int)(q - (long long)z * npl);
        const int y = rem / g.nx, x = rem - y * g.nx;
        out[lidx(g, z, y, x)] = op.template solve<DIM>(g, omega, damped, u, rhs, z, y, x);
    }
    __syncthreads();
}

template <typename Op, int DIM, typename T>
__device__ void wg_op_rbgs(const Geom &g, const Op &op, T *u, const T *rhs)
{
    const int npl = g.nx * g.ny;
    const long long total = (long long)npl * g.nz;
    for (int colour = 0; colour < 2; colour++) {
        for (long long q = threadIdx.x; q < total; q += SWG) {
            const int z = (int)(q / npl), rem = (int)(q - (long long)z * npl);
            const int y = rem / g.nx, x = rem - y * g.nx;
            if (((x + y + g.gz0 + z) & 1) != colour) continue;
            u[lidx(g, z, y, x)] = op.template solve<DIM>(g, (T)1, false, u, rhs, z, y, x);
        }
        __syncthreads();
    }
}

template <typename Op, int DIM, typename T>
__device__ double wg_op_residual_sumsq(const Geom &g, const Op &op, const T *u, const T *rhs, double *sh)
{
    const int npl = g.nx * g.ny;
    const long long total = (long long)npl * g.nz;
    double sq = 0.;
    for (long long q = threadIdx.x; q < total; q += SWG) {
        const int z = (int)(q / npl), rem = (int)(q - (long long)z * npl);
        const int y = rem / g.nx, x = rem - y * g.nx;
        const T res = op.template res<DIM>(g, u, rhs, z, y, x);
        sq += (double)res * (double)res;
    }
    return block_sum_bcast(sq, sh);
}

// k_coarse_solve's loop (Solver::Solve with maxit, tol, fixed) with the family's sweep and the family's residual
template <typename Op, int DIM>
__global__ __launch_bounds__(SWG) void k_op_coarse(Geom g, Op op, typename Op::type omega, int smoother, typename Op::type *x,
                                                   typename Op::type *tmp, const typename Op::type *rhs, int maxit, double tol, int fixed,
                                                   CoarseOut *out)
{
    typedef typename Op::type T;
    __shared__ double sh[18];
    T *cur = x, *oth = tmp;
    const bool damped = (omega != (T)1);
    auto sweep = [&]() {
        if (smoother == 1) {
            wg_op_jacobi<Op, DIM, T>(g, op, omega, damped, cur, rhs, oth);
            T *t = cur; cur = oth; oth = t;
        } else {
            wg_op_rbgs<Op, DIM, T>(g, op, cur, rhs);
        }
    };
    const double nb = wg_sumsq<T>(g, rhs, sh);
    int iters = 0, flag = 0;
    double nr;
    if (fixed) {
        for (int s = 0; s < maxit; s++) sweep();
        iters = maxit;
        nr = wg_op_residual_sumsq<Op, DIM, T>(g, op, cur, rhs, sh);
    } else {
        int counter = maxit;
        nr = wg_op_residual_sumsq<Op, DIM, T>(g, op, cur, rhs, sh);
        while (sqrt(nr / nb) > tol) {   // NaN (zero rhs) compares false, as in k_coarse_solve
            if (counter > 0) {
                sweep();
                counter -= 1;
                iters++;
                nr = wg_op_residual_sumsq<Op, DIM, T>(g, op, cur, rhs, sh);
            } else {
                flag = 1;
                break;
            }
        }
    }
    if (cur != x) {   // odd number of Jacobi sweeps: move the result back into x
        const int npl = g.nx * g.ny;
        const long long total = (long long)npl * g.nz;
        for (long long q = threadIdx.x; q < total; q += SWG) {
            const int z = (int)(q / npl), rem = (int)(q - (long long)z * npl);
            const int y = rem / g.nx, xx = rem - y * g.nx;
            const long long i = lidx(g, z, y, xx);
            x[i] = cur[i];
        }
    }
    if (threadIdx.x == 0) {
        out->iters = iters;
        out->flag = flag;
        out->relres = sqrt(nr / nb);
        out->sumsq_rhs = nb;
        out->sumsq_r = nr;
    }
}

// ---------------------------------------------------------------- launch planners and the launches every family makes alike
inline int plain_grid(long long items, int cap)
{
    const long long nb = std::min<long long>(OP_MAX_BLOCKS, (items + OP_THREADS - 1) / OP_THREADS);
    return (int)std::max<long long>(1, std::min<long long>(nb, cap));
}

struct MarchGrid { int nbx, nby, nbz, zc, grid; };

template <typename T>
MarchGrid march_grid(const Geom &g)
{
    constexpr int V = Vec16<T>::n;
    // vectors a row needs lanes for: the full ones, and a partial last one unless it is the single tail column
    const int nvec = std::max(1, g.nx / V + (g.nx % V > 1 ? 1 : 0));
    MarchGrid m;
    m.nbx = (nvec + 63) / 64;
    m.nby = (g.ny + MRY * MBW - 1) / (MRY * MBW);
    // a chunk of zc planes loads zc + 2: long chunks while they still fill the chip, never shorter than 4
    m.zc = 16;
    while (m.zc > 4 && (long long)m.nbx * m.nby * ((g.nz + m.zc - 1) / m.zc) < 2048) m.zc >>= 1;
    m.nbz = (g.nz + m.zc - 1) / m.zc;
    m.grid = ((m.nbx * m.nby * m.nbz + 7) / 8) * 8;
    return m;
}

// whole levels only: the mg_vc_*, mg_bc_* and mg_fas_* drivers refuse distributed handles before they get here
template <typename T>
bool march_takes(const Geom &g, bool plain)
{
    return !plain && march_ok(g.dim, g.nx, g.ny, g.nz, (int)sizeof(T)) && g.gz0 == 0 && g.gnz == g.nz;
}

// the plain residual of launch_*_residual (r == nullptr: the norm only) -> the number of partial sums
template <typename Op>
int plain_residual(hipStream_t s, const Geom &g, const Op &op, const typename Op::type *u, const typename Op::type *b,
                   typename Op::type *r, double *partials, int cap)
{
    typedef typename Op::type T;
    const int nb = plain_grid((long long)g.nx * g.ny * g.nz, cap);
    const dim3 gr(nb), bl(OP_THREADS);
#define MG_OP(DIM, SAVE) hipLaunchKernelGGL((k_op_plain<Op, DIM, OP_RES, SAVE>), gr, bl, 0, s, g, op, (T)1, 0, u, b, r, partials, StepCoef<T>{})
    if (g.dim == 3) { if (r) MG_OP(3, true); else MG_OP(3, false); }
    else { if (r) MG_OP(2, true); else MG_OP(2, false); }
#undef MG_OP
    return nb;
}

template <typename Op>
void plain_jacobi(hipStream_t s, const Geom &g, const Op &op, typename Op::type omega, const typename Op::type *u,
                  const typename Op::type *b, typename Op::type *out)
{
    typedef typename Op::type T;
    const dim3 gr(plain_grid((long long)g.nx * g.ny * g.nz, OP_MAX_BLOCKS)), bl(OP_THREADS);
    if (g.dim == 3) hipLaunchKernelGGL((k_op_plain<Op, 3, OP_JAC, false>), gr, bl, 0, s, g, op, omega, 0, u, b, out, (double *)nullptr, StepCoef<T>{});
    else hipLaunchKernelGGL((k_op_plain<Op, 2, OP_JAC, false>), gr, bl, 0, s, g, op, omega, 0, u, b, out, (double *)nullptr, StepCoef<T>{});
}

template <typename Op>
void plain_rb_colour(hipStream_t s, const Geom &g, const Op &op, int colour, typename Op::type *u, const typename Op::type *b)
{
    typedef typename Op::type T;
    const dim3 gr(plain_grid((long long)((g.nx + 1) / 2) * g.ny * g.nz, OP_MAX_BLOCKS)), bl(OP_THREADS);
    if (g.dim == 3) hipLaunchKernelGGL((k_op_plain<Op, 3, OP_RB, false>), gr, bl, 0, s, g, op, (T)1, colour, u, b, u, (double *)nullptr, StepCoef<T>{});
    else hipLaunchKernelGGL((k_op_plain<Op, 2, OP_RB, false>), gr, bl, 0, s, g, op, (T)1, colour, u, b, u, (double *)nullptr, StepCoef<T>{});
}

// the step's right-hand side in the plain form; op carries the UNSHIFTED operator, f == nullptr: no source
template <typename Op>
void plain_step(hipStream_t s, const Geom &g, const Op &op, const StepCoef<typename Op::type> &st, const typename Op::type *u,
                const typename Op::type *f, typename Op::type *out)
{
    typedef typename Op::type T;
    const dim3 gr(plain_grid((long long)g.nx * g.ny * g.nz, OP_MAX_BLOCKS)), bl(OP_THREADS);
#define MG_OP(DIM, SRC) hipLaunchKernelGGL((k_op_plain<Op, DIM, OP_STEP, true, SRC>), gr, bl, 0, s, g, op, (T)1, 0, u, f, out, (double *)nullptr, st)
    if (g.dim == 3) { if (f) MG_OP(3, true); else MG_OP(3, false); }
    else { if (f) MG_OP(2, true); else MG_OP(2, false); }
#undef MG_OP
}

template <typename Op>
void coarse_solve(hipStream_t s, const Geom &g, const Op &op, typename Op::type omega, int smoother, typename Op::type *x,
                  typename Op::type *tmp, const typename Op::type *rhs, int maxit, double tol, int fixed, CoarseOut *d_out)
{
    if (g.dim == 3) hipLaunchKernelGGL((k_op_coarse<Op, 3>), dim3(1), dim3(SWG), 0, s, g, op, omega, smoother, x, tmp, rhs, maxit, tol, fixed, d_out);
    else hipLaunchKernelGGL((k_op_coarse<Op, 2>), dim3(1), dim3(SWG), 0, s, g, op, omega, smoother, x, tmp, rhs, maxit, tol, fixed, d_out);
}

}  // namespace mg
