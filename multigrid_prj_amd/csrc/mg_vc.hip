// mg_vc.hip -- kernels of the variable-coefficient operator -div(a grad u) + sigma u (mg_vc_*, include/mg_hip.h; drivers:
// Solver::vc_* in mg_drivers.cpp). The coefficient a is a nodal, level-shaped array of every level (Level::vc_a); the
// transfers do not depend on the operator, so only the smoother, the residual, the coarsest-grid solve and the Krylov
// direction kernel live here.
//
//   k_vc_plain<T, DIM, OP, SAVE>   OP = residual (stored with SAVE, else norm only) / Jacobi sweep (out of place) / one
//                                  red-black colour pass (in place): one thread per node, grid-stride, every shape
//   k_vc_march<T, OP, SAVE>        the residual and the Jacobi sweep on 3-D levels with rows long enough to fill a wave
//                                  (vc_march_ok, mg_geom.h)
//   k_vc_coarse<T, DIM>            the Solver::Solve loop of k_coarse_solve (mg_kernels.hip) in one workgroup
//   k_vc_cg_direction<T, DIM>      k_cg_direction_apply (mg_krylov.hip) with q = L p'
//
// The marching tile is k_heat_rhs's (mg_heat.hip) with TWO marched fields: a lane owns one aligned 16-byte vector of x, a
// wave covers 64 vectors of VRY = 2 rows, VBW = 4 waves are stacked in y and the workgroup marches zc planes with the
// planes z-1, z, z+1 of u AND a of its columns in registers, so each is loaded once per workgroup column. x-neighbours
// are the neighbouring lanes' values (whole-wave DPP shifts; the two edge lanes load theirs), y-neighbours the wave's
// other row or two halo rows that hit L1 / L2. b is loaded and r / u' stored non-temporally, the block order is
// XCD-aware, the odd last column is written as one full 128-byte line as in mg_heat.hip. Ghost planes and padding
// columns are read (they exist and hold zeros) and what is computed from them is dropped: only Dirichlet nodes touch them.
//
// Arithmetic contract (compiled with -ffp-contract=off; tests/vc_ref.py restates it in numpy), all in T, every operation
// rounded separately, w_a = (T)(-c_a / 2) with c_a the level's off-diagonal of mg_level_coefficients:
//   s = 0, d = (T)sigma; for the neighbours q in the residual kernel's row order z-, y-, x-, x+, y+, z+ (no z in 2-D):
//       g = w_a * (a_i + a_q);  s = s + g * u_q;  d = d + g
//   residual     r = b - (d * u_i - s) on interior nodes, r = b - u on Dirichlet nodes (k_residual's convention, which
//                is npref.residual's too); the sum of r^2 over ALL nodes in double, fixed order, no atomics
//   point solve  ps = (b + s) / d, an IEEE division
//   Jacobi       u' = ps (omega == 1) or u_i + omega * (ps - u_i); Dirichlet nodes: u' = b
//   red-black    in place, colour (i + j + k) & 1, colour 0 first; Dirichlet nodes take b with their colour
//   direction    p' = z + beta * p (0 on Dirichlet nodes), q = d * p'_i - s with u = p' (0 on Dirichlet nodes), p'.q in double
#include "mg_kernels.h"
#include "mg_device.h"

#include <algorithm>

namespace mg {
namespace {

constexpr int VC_THREADS = 256, VC_MAX_BLOCKS = 2048;
constexpr int VBW = 4, VRY = 2;   // waves per workgroup / rows per wave of the marching tile
enum { VC_RES = 0, VC_JAC = 1, VC_RB = 2 };

template <typename T>
struct VcCoef {
    T wx, wy, wz, sigma;
};

// one neighbour of the contract
template <typename T>
__device__ __forceinline__ void vc_nb(T w, T ai, T aq, T uq, T &s, T &d)
{
    const T g = w * (ai + aq);
    s = s + g * uq;
    d = d + g;
}

// s and d at element i; uat(q, k) = u at element q, the k-th neighbour in row order (0: z-, 1: y-, 2: x-, 3: x+, 4: y+, 5: z+)
template <typename T, int DIM, typename F>
__device__ __forceinline__ void vc_parts(F &&uat, const T *a, long long i, int pitch, long long plane, const VcCoef<T> &c, T &s, T &d)
{
    const T ai = a[i];
    s = (T)0;
    d = c.sigma;
    if (DIM == 3) vc_nb<T>(c.wz, ai, a[i - plane], uat(i - plane, 0), s, d);
    vc_nb<T>(c.wy, ai, a[i - pitch], uat(i - pitch, 1), s, d);
    vc_nb<T>(c.wx, ai, a[i - 1], uat(i - 1, 2), s, d);
    vc_nb<T>(c.wx, ai, a[i + 1], uat(i + 1, 3), s, d);
    vc_nb<T>(c.wy, ai, a[i + pitch], uat(i + pitch, 4), s, d);
    if (DIM == 3) vc_nb<T>(c.wz, ai, a[i + plane], uat(i + plane, 5), s, d);
}

template <typename T, int DIM>
__device__ __forceinline__ T vc_point_res(const Geom &g, const VcCoef<T> &c, const T *u, const T *a, const T *b, int z, int y, int x)
{
    const long long i = lidx(g, z, y, x);
    if (on_boundary(g, z, y, x)) return b[i] - u[i];
    T s, d;
    vc_parts<T, DIM>([&](long long q, int) { return u[q]; }, a, i, g.pitch, g.plane, c, s, d);
    return b[i] - (d * u[i] - s);
}

template <typename T, int DIM>
__device__ __forceinline__ T vc_point_solve(const Geom &g, const VcCoef<T> &c, T omega, bool damped, const T *u, const T *a,
                                            const T *b, int z, int y, int x)
{
    const long long i = lidx(g, z, y, x);
    const T bi = b[i];
    if (on_boundary(g, z, y, x)) return bi;
    T s, d;
    vc_parts<T, DIM>([&](long long q, int) { return u[q]; }, a, i, g.pitch, g.plane, c, s, d);
    const T ps = (bi + s) / d;
    if (damped) {
        const T ui = u[i];
        return ui + omega * (ps - ui);
    }
    return ps;
}

// ---------------------------------------------------------------- the plain form
// out: r (VC_RES with SAVE), u' (VC_JAC, must not alias u) or u itself (VC_RB: the other colour is only read)
template <typename T, int DIM, int OP, bool SAVE>
__global__ __launch_bounds__(VC_THREADS) void k_vc_plain(Geom g, VcCoef<T> c, T omega, int colour, const T *u, const T *__restrict__ a,
                                                         const T *__restrict__ b, T *out, double *__restrict__ partials)
{
    __shared__ double sh[VC_THREADS / 64];
    const int hx = OP == VC_RB ? (g.nx + 1) / 2 : g.nx;   // nodes of a row this launch visits
    const long long nitems = (long long)hx * g.ny * g.nz;
    const bool damped = OP == VC_JAC && omega != (T)1;
    double acc = 0.;
    for (long long it = (long long)blockIdx.x * VC_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * VC_THREADS) {
        const long long row = it / hx;
        int x = (int)(it - row * hx);
        const int y = (int)(row % g.ny), z = (int)(row / g.ny);
        if (OP == VC_RB) {
            x = 2 * x + ((y + g.gz0 + z + colour) & 1);   // the x parity that has (x + y + gz) & 1 == colour
            if (x >= g.nx) continue;
        }
        if (OP == VC_RES) {
            const T res = vc_point_res<T, DIM>(g, c, u, a, b, z, y, x);
            acc += (double)res * (double)res;
            if (SAVE) out[lidx(g, z, y, x)] = res;
        } else {
            out[lidx(g, z, y, x)] = vc_point_solve<T, DIM>(g, c, omega, damped, u, a, b, z, y, x);
        }
    }
    if (OP == VC_RES) {
        const double s = block_sum(acc, sh);
        if (threadIdx.x == 0) partials[blockIdx.x] = s;
    }
}

// ---------------------------------------------------------------- the marching tile (3-D)
template <typename T, int OP, bool SAVE>
__global__ __launch_bounds__(64 * VBW) void k_vc_march(Geom g, VcCoef<T> c, T omega, const T *__restrict__ u, const T *__restrict__ a,
                                                       const T *__restrict__ b, T *__restrict__ out, double *__restrict__ partials,
                                                       int nbx, int nby, int nbz, int zc)
{
    constexpr int V = Vec16<T>::n;
    constexpr bool STORE = OP == VC_JAC || SAVE;
    typedef typename Vec16<T>::type vec;
    __shared__ double sh[VBW];

    const int nblocks = nbx * nby * nbz;
    const int bid = xcd_block(blockIdx.x, (nblocks + 7) >> 3);
    if (bid >= nblocks) {   // the whole workgroup
        if (OP == VC_RES && threadIdx.x == 0) partials[blockIdx.x] = 0.;
        return;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int bx = bid % nbx, by = (bid / nbx) % nby, bz = bid / (nbx * nby);
    const int x0 = V * (bx * 64 + lane);
    const int x0c = min(x0, g.pitch - V);   // clamped for loads: every lane stays active
    const bool xfull = x0 + V <= g.nx;      // the lane's vector lies inside the row
    const int yb = (by * VBW + wv) * VRY;
    const int z0 = bz * zc, zend = min(z0 + zc, g.nz);
    // one column left over: the wave that holds the row's last full vector writes it as a full line
    const bool tail1 = g.nx % V == 1 && g.nx > V;
    const bool tailwave = tail1 && (bx * 64 * V <= g.nx - 1 - V) && (g.nx - 1 - V < (bx + 1) * 64 * V);
    const int part = (!tail1 && !xfull && x0 < g.nx) ? g.nx - x0 : 0;   // elements of a partial last vector stored one by one
    const int nown = xfull ? V : part;                                  // elements of the vector this lane stores and sums
    const bool damped = OP == VC_JAC && omega != (T)1;

    long long rowoff[VRY];
    bool yin[VRY], ybnd[VRY];
#pragma unroll
    for (int r = 0; r < VRY; r++) {
        const int y = yb + r;
        yin[r] = y < g.ny;
        const int yc = min(y, g.ny - 1);
        ybnd[r] = (yc == 0) || (yc == g.ny - 1);
        rowoff[r] = (long long)yc * g.pitch + x0c;
    }
    const long long off_lo = (long long)min(max(yb - 1, 0), g.ny - 1) * g.pitch + x0c;
    const long long off_hi = (long long)min(yb + VRY, g.ny - 1) * g.pitch + x0c;
    const bool edge_l = lane == 0 && x0c > 0, edge_r = lane == 63 && x0c + V < g.pitch;

    vec uzm[VRY], ucc[VRY], uzp[VRY], azm[VRY], acc_[VRY], azp[VRY];
    const T *pu = u + (long long)z0 * g.plane, *pa = a + (long long)z0 * g.plane;
#pragma unroll
    for (int r = 0; r < VRY; r++) {
        uzm[r] = *(const vec *)(pu - g.plane + rowoff[r]);
        ucc[r] = *(const vec *)(pu + rowoff[r]);
        azm[r] = *(const vec *)(pa - g.plane + rowoff[r]);
        acc_[r] = *(const vec *)(pa + rowoff[r]);
    }
    double acc = 0.;
    for (int z = z0; z < zend; z++, pu += g.plane, pa += g.plane) {
        const long long zo = (long long)z * g.plane;
        vec bv[VRY];
#pragma unroll
        for (int r = 0; r < VRY; r++) {
            uzp[r] = *(const vec *)(pu + g.plane + rowoff[r]);
            azp[r] = *(const vec *)(pa + g.plane + rowoff[r]);
            bv[r] = __builtin_nontemporal_load((const vec *)(b + zo + rowoff[r]));
        }
        const vec ulo = *(const vec *)(pu + off_lo), uhi = *(const vec *)(pu + off_hi);
        const vec alo = *(const vec *)(pa + off_lo), ahi = *(const vec *)(pa + off_hi);
        const int gz = g.gz0 + z;
        const bool zb = (gz == 0) || (gz == g.gnz - 1);
#pragma unroll
        for (int r = 0; r < VRY; r++) {
            T uel = 0, uer = 0, ael = 0, aer = 0;
            if (edge_l) { uel = pu[rowoff[r] - 1]; ael = pa[rowoff[r] - 1]; }
            if (edge_r) { uer = pu[rowoff[r] + V]; aer = pa[rowoff[r] + V]; }
            const T uxm = lane_from_prev(ucc[r][V - 1], uel), uxp = lane_from_next(ucc[r][0], uer);
            const T axm = lane_from_prev(acc_[r][V - 1], ael), axp = lane_from_next(acc_[r][0], aer);
            const vec uym = (r > 0) ? ucc[r > 0 ? r - 1 : 0] : ulo, uyp = (r < VRY - 1) ? ucc[r < VRY - 1 ? r + 1 : 0] : uhi;
            const vec aym = (r > 0) ? acc_[r > 0 ? r - 1 : 0] : alo, ayp = (r < VRY - 1) ? acc_[r < VRY - 1 ? r + 1 : 0] : ahi;
            const bool rb = zb || ybnd[r];
            vec res;
#pragma unroll
            for (int e = 0; e < V; e++) {
                const T ui = ucc[r][e], ai = acc_[r][e], bi = bv[r][e];
                const T ul = (e == 0) ? uxm : ucc[r][e > 0 ? e - 1 : 0], al = (e == 0) ? axm : acc_[r][e > 0 ? e - 1 : 0];
                const T ur = (e == V - 1) ? uxp : ucc[r][e < V - 1 ? e + 1 : 0], ar = (e == V - 1) ? axp : acc_[r][e < V - 1 ? e + 1 : 0];
                T s = (T)0, d = c.sigma;
                vc_nb<T>(c.wz, ai, azm[r][e], uzm[r][e], s, d);
                vc_nb<T>(c.wy, ai, aym[e], uym[e], s, d);
                vc_nb<T>(c.wx, ai, al, ul, s, d);
                vc_nb<T>(c.wx, ai, ar, ur, s, d);
                vc_nb<T>(c.wy, ai, ayp[e], uyp[e], s, d);
                vc_nb<T>(c.wz, ai, azp[r][e], uzp[r][e], s, d);
                const bool bnd = rb || (x0 + e == 0) || (x0 + e == g.nx - 1);
                T v;
                if (OP == VC_RES) {
                    v = bnd ? bi - ui : bi - (d * ui - s);
                } else {
                    const T ps = (bi + s) / d;
                    v = bnd ? bi : (damped ? ui + omega * (ps - ui) : ps);
                }
                res[e] = v;
            }
            if (yin[r]) {
                if (OP == VC_RES) {
#pragma unroll
                    for (int e = 0; e < V; e++)
                        if (e < nown) acc += (double)res[e] * (double)res[e];
                }
                T *const po = out + zo + rowoff[r];
                if (xfull) {
                    if (STORE) __builtin_nontemporal_store(res, (vec *)po);
                } else if (part) {
#pragma unroll
                    for (int e = 0; e < V; e++)
                        if (STORE && e < part) po[e] = res[e];
                }
                if (tailwave && lane >= 56) {
                    // column nx-1 (Dirichlet: r = b - u, u' = b) as one full 128-byte line: value + zero padding
                    const int j = lane - 56;
                    constexpr int LINE = 128 / (int)sizeof(T);
                    const int xs = g.nx - 1 + V * j;
                    const int line_end = ((g.nx - 1) / LINE + 1) * LINE;
                    const long long ro = zo + (rowoff[r] - x0c);
                    if (xs < line_end) {
                        vec tv = (vec)(0);
                        if (j == 0) {
                            const T bt = b[ro + g.nx - 1];
                            if (OP == VC_RES) {
                                const T rt = bt - u[ro + g.nx - 1];
                                acc += (double)rt * (double)rt;
                                tv[0] = rt;
                            } else {
                                tv[0] = bt;
                            }
                        }
                        if (STORE) __builtin_nontemporal_store(tv, (vec *)(out + ro + xs));
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < VRY; r++) { uzm[r] = ucc[r]; ucc[r] = uzp[r]; azm[r] = acc_[r]; acc_[r] = azp[r]; }
    }
    if (OP == VC_RES) {
        const double s = block_sum(acc, sh);
        if (threadIdx.x == 0) partials[blockIdx.x] = s;
    }
}

// ---------------------------------------------------------------- the coarsest-grid solve: one workgroup
template <typename T, int DIM>
__device__ void wg_vc_jacobi(const Geom &g, const VcCoef<T> &c, T omega, bool damped, const T *u, const T *a, const T *rhs, T *out)
{
    const int npl = g.nx * g.ny;
    const long long total = (long long)npl * g.nz;
    for (long long q = threadIdx.x; q < total; q += SWG) {
        const int z = (int)(q / npl), rem = (int)(q - (long long)z * npl);
        const int y = rem / g.nx, x = rem - y * g.nx;
        out[lidx(g, z, y, x)] = vc_point_solve<T, DIM>(g, c, omega, damped, u, a, rhs, z, y, x);
    }
    __syncthreads();
}

template <typename T, int DIM>
__device__ void wg_vc_rbgs(const Geom &g, const VcCoef<T> &c, T *u, const T *a, const T *rhs)
{
    const int npl = g.nx * g.ny;
    const long long total = (long long)npl * g.nz;
    for (int colour = 0; colour < 2; colour++) {
        for (long long q = threadIdx.x; q < total; q += SWG) {
            const int z = (int)(q / npl), rem = (int)(q - (long long)z * npl);
            const int y = rem / g.nx, x = rem - y * g.nx;
            if (((x + y + g.gz0 + z) & 1) != colour) continue;
            u[lidx(g, z, y, x)] = vc_point_solve<T, DIM>(g, c, (T)1, false, u, a, rhs, z, y, x);
        }
        __syncthreads();
    }
}

template <typename T, int DIM>
__device__ double wg_vc_residual_sumsq(const Geom &g, const VcCoef<T> &c, const T *u, const T *a, const T *rhs, double *sh)
{
    const int npl = g.nx * g.ny;
    const long long total = (long long)npl * g.nz;
    double sq = 0.;
    for (long long q = threadIdx.x; q < total; q += SWG) {
        const int z = (int)(q / npl), rem = (int)(q - (long long)z * npl);
        const int y = rem / g.nx, x = rem - y * g.nx;
        const T res = vc_point_res<T, DIM>(g, c, u, a, rhs, z, y, x);
        sq += (double)res * (double)res;
    }
    return block_sum_bcast(sq, sh);
}

// k_coarse_solve's loop (Solver::Solve with maxit, tol, fixed) with the vc sweep and the vc residual
template <typename T, int DIM>
__global__ __launch_bounds__(SWG) void k_vc_coarse(Geom g, VcCoef<T> c, T omega, int smoother, T *x, T *tmp, const T *rhs, const T *a,
                                                   int maxit, double tol, int fixed, CoarseOut *out)
{
    __shared__ double sh[18];
    T *cur = x, *oth = tmp;
    const bool damped = (omega != (T)1);
    auto sweep = [&]() {
        if (smoother == 1) {
            wg_vc_jacobi<T, DIM>(g, c, omega, damped, cur, a, rhs, oth);
            T *t = cur; cur = oth; oth = t;
        } else {
            wg_vc_rbgs<T, DIM>(g, c, cur, a, rhs);
        }
    };
    const double nb = wg_sumsq<T>(g, rhs, sh);
    int iters = 0, flag = 0;
    double nr;
    if (fixed) {
        for (int s = 0; s < maxit; s++) sweep();
        iters = maxit;
        nr = wg_vc_residual_sumsq<T, DIM>(g, c, cur, a, rhs, sh);
    } else {
        int counter = maxit;
        nr = wg_vc_residual_sumsq<T, DIM>(g, c, cur, a, rhs, sh);
        while (sqrt(nr / nb) > tol) {   // NaN (zero rhs) compares false, as in k_coarse_solve
            if (counter > 0) {
                sweep();
                counter -= 1;
                iters++;
                nr = wg_vc_residual_sumsq<T, DIM>(g, c, cur, a, rhs, sh);
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

// ---------------------------------------------------------------- p' = z + beta p, q = L p', sum p'.q
template <typename T, int DIM>
__global__ __launch_bounds__(VC_THREADS) void k_vc_cg_direction(Geom g, VcCoef<T> c, const T *__restrict__ zv, const T *__restrict__ p,
                                                                const T *__restrict__ a, T *__restrict__ pn, T *__restrict__ q,
                                                                const CgScalars *__restrict__ sc, double *__restrict__ partials)
{
    __shared__ double sh[VC_THREADS / 64];
    if (sc->bad != 0) return;   // breakdown flagged by an earlier tail: nothing is written, the tail that follows returns too
    const T beta = (T)sc->beta;
    const long long nitems = (long long)g.nx * g.ny * g.nz;
    double acc = 0.;
    for (long long it = (long long)blockIdx.x * VC_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * VC_THREADS) {
        const long long row = it / g.nx;
        const int x = (int)(it - row * g.nx), y = (int)(row % g.ny), z = (int)(row / g.ny);
        const long long i = lidx(g, z, y, x);
        T pc = (T)0, qv = (T)0;
        if (!on_boundary(g, z, y, x)) {
            pc = zv[i] + beta * p[i];
            T s, d;
            vc_parts<T, DIM>([&](long long e, int k) -> T {
                const int dz = k == 0 ? -1 : (k == 5 ? 1 : 0), dy = k == 1 ? -1 : (k == 4 ? 1 : 0), dx = k == 2 ? -1 : (k == 3 ? 1 : 0);
                if (on_boundary(g, z + dz, y + dy, x + dx)) return (T)0;
                return zv[e] + beta * p[e];
            }, a, i, g.pitch, g.plane, c, s, d);
            qv = d * pc - s;
            acc += (double)pc * (double)qv;
        }
        pn[i] = pc;
        q[i] = qv;
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---------------------------------------------------------------- launchers
template <typename T>
VcCoef<T> vc_coef(const double coef[4], double sigma)
{
    return VcCoef<T>{(T)(-coef[0] / 2.0), (T)(-coef[1] / 2.0), (T)(-coef[2] / 2.0), (T)sigma};
}

int vc_plain_grid(long long items, int cap)
{
    const long long nb = std::min<long long>(VC_MAX_BLOCKS, (items + VC_THREADS - 1) / VC_THREADS);
    return (int)std::max<long long>(1, std::min<long long>(nb, cap));
}

struct VcMarchGrid { int nbx, nby, nbz, zc, grid; };

template <typename T>
VcMarchGrid vc_march_grid(const Geom &g)
{
    constexpr int V = Vec16<T>::n;
    // vectors a row needs lanes for: the full ones, and a partial last one unless it is the single tail column
    const int nvec = std::max(1, g.nx / V + (g.nx % V > 1 ? 1 : 0));
    VcMarchGrid m;
    m.nbx = (nvec + 63) / 64;
    m.nby = (g.ny + VRY * VBW - 1) / (VRY * VBW);
    // a chunk of zc planes loads zc + 2: long chunks while they still fill the chip, never shorter than 4
    m.zc = 16;
    while (m.zc > 4 && (long long)m.nbx * m.nby * ((g.nz + m.zc - 1) / m.zc) < 2048) m.zc >>= 1;
    m.nbz = (g.nz + m.zc - 1) / m.zc;
    m.grid = ((m.nbx * m.nby * m.nbz + 7) / 8) * 8;
    return m;
}

// whole levels only: mg_vc_* refuse distributed handles before they get here
template <typename T>
bool vc_march_takes(const Geom &g, bool plain)
{
    return !plain && vc_march_ok(g.dim, g.nx, g.ny, g.nz, (int)sizeof(T)) && g.gz0 == 0 && g.gnz == g.nz;
}

}  // namespace

template <typename T>
int launch_vc_residual(hipStream_t s, const Geom &g, const double coef[4], double sigma, const T *u, const T *a, const T *b, T *r,
                       double *partials, int cap, bool plain)
{
    const VcCoef<T> c = vc_coef<T>(coef, sigma);
    if (vc_march_takes<T>(g, plain)) {
        const VcMarchGrid m = vc_march_grid<T>(g);
        if (m.grid <= cap) {
            const dim3 gr(m.grid), bl(64 * VBW);
            if (r) hipLaunchKernelGGL((k_vc_march<T, VC_RES, true>), gr, bl, 0, s, g, c, (T)1, u, a, b, r, partials, m.nbx, m.nby, m.nbz, m.zc);
            else hipLaunchKernelGGL((k_vc_march<T, VC_RES, false>), gr, bl, 0, s, g, c, (T)1, u, a, b, r, partials, m.nbx, m.nby, m.nbz, m.zc);
            return m.grid;
        }
    }
    const int nb = vc_plain_grid((long long)g.nx * g.ny * g.nz, cap);
    const dim3 gr(nb), bl(VC_THREADS);
#define MG_VC(DIM, SAVE) hipLaunchKernelGGL((k_vc_plain<T, DIM, VC_RES, SAVE>), gr, bl, 0, s, g, c, (T)1, 0, u, a, b, r, partials)
    if (g.dim == 3) { if (r) MG_VC(3, true); else MG_VC(3, false); }
    else { if (r) MG_VC(2, true); else MG_VC(2, false); }
#undef MG_VC
    return nb;
}

template <typename T>
void launch_vc_jacobi(hipStream_t s, const Geom &g, const double coef[4], double sigma, T omega, const T *u, const T *a, const T *b,
                      T *out, bool plain)
{
    const VcCoef<T> c = vc_coef<T>(coef, sigma);
    if (vc_march_takes<T>(g, plain)) {
        const VcMarchGrid m = vc_march_grid<T>(g);
        hipLaunchKernelGGL((k_vc_march<T, VC_JAC, false>), dim3(m.grid), dim3(64 * VBW), 0, s, g, c, omega, u, a, b, out,
                           (double *)nullptr, m.nbx, m.nby, m.nbz, m.zc);
        return;
    }
    const dim3 gr(vc_plain_grid((long long)g.nx * g.ny * g.nz, VC_MAX_BLOCKS)), bl(VC_THREADS);
    if (g.dim == 3) hipLaunchKernelGGL((k_vc_plain<T, 3, VC_JAC, false>), gr, bl, 0, s, g, c, omega, 0, u, a, b, out, (double *)nullptr);
    else hipLaunchKernelGGL((k_vc_plain<T, 2, VC_JAC, false>), gr, bl, 0, s, g, c, omega, 0, u, a, b, out, (double *)nullptr);
}

template <typename T>
void launch_vc_rb_colour(hipStream_t s, const Geom &g, const double coef[4], double sigma, int colour, T *u, const T *a, const T *b)
{
    const VcCoef<T> c = vc_coef<T>(coef, sigma);
    const dim3 gr(vc_plain_grid((long long)((g.nx + 1) / 2) * g.ny * g.nz, VC_MAX_BLOCKS)), bl(VC_THREADS);
    if (g.dim == 3) hipLaunchKernelGGL((k_vc_plain<T, 3, VC_RB, false>), gr, bl, 0, s, g, c, (T)1, colour, u, a, b, u, (double *)nullptr);
    else hipLaunchKernelGGL((k_vc_plain<T, 2, VC_RB, false>), gr, bl, 0, s, g, c, (T)1, colour, u, a, b, u, (double *)nullptr);
}

template <typename T>
void launch_vc_coarse(hipStream_t s, const Geom &g, const double coef[4], double sigma, T omega, int smoother, T *x, T *tmp,
                      const T *rhs, const T *a, int maxit, double tol, int fixed, CoarseOut *d_out)
{
    const VcCoef<T> c = vc_coef<T>(coef, sigma);
    if (g.dim == 3) hipLaunchKernelGGL((k_vc_coarse<T, 3>), dim3(1), dim3(SWG), 0, s, g, c, omega, smoother, x, tmp, rhs, a, maxit, tol, fixed, d_out);
    else hipLaunchKernelGGL((k_vc_coarse<T, 2>), dim3(1), dim3(SWG), 0, s, g, c, omega, smoother, x, tmp, rhs, a, maxit, tol, fixed, d_out);
}

template <typename T>
int launch_vc_cg_direction(hipStream_t s, const Geom &g, const double coef[4], double sigma, const T *z, const T *p, const T *a, T *pn,
                           T *q, const CgScalars *sc, double *partials)
{
    const VcCoef<T> c = vc_coef<T>(coef, sigma);
    const int nb = vc_plain_grid((long long)g.nx * g.ny * g.nz, VC_MAX_BLOCKS);
    if (g.dim == 3) hipLaunchKernelGGL((k_vc_cg_direction<T, 3>), dim3(nb), dim3(VC_THREADS), 0, s, g, c, z, p, a, pn, q, sc, partials);
    else hipLaunchKernelGGL((k_vc_cg_direction<T, 2>), dim3(nb), dim3(VC_THREADS), 0, s, g, c, z, p, a, pn, q, sc, partials);
    return nb;
}

#define MG_VC_INST(T)                                                                                                                  \
    template int launch_vc_residual<T>(hipStream_t, const Geom &, const double[4], double, const T *, const T *, const T *, T *,      \
                                       double *, int, bool);                                                                         \
    template void launch_vc_jacobi<T>(hipStream_t, const Geom &, const double[4], double, T, const T *, const T *, const T *, T *,   \
                                      bool);                                                                                         \
    template void launch_vc_rb_colour<T>(hipStream_t, const Geom &, const double[4], double, int, T *, const T *, const T *);         \
    template void launch_vc_coarse<T>(hipStream_t, const Geom &, const double[4], double, T, int, T *, T *, const T *, const T *, int, \
                                      double, int, CoarseOut *);                                                                     \
    template int launch_vc_cg_direction<T>(hipStream_t, const Geom &, const double[4], double, const T *, const T *, const T *, T *,  \
                                           T *, const CgScalars *, double *);
MG_VC_INST(double)
MG_VC_INST(float)
#undef MG_VC_INST

}  // namespace mg
