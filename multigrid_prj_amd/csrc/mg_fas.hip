// mg_fas.hip -- kernels of the SEMILINEAR operator N(u) = (sigma I + A) u + gamma g(u) of the full approximation scheme
// (mg_fas_*, include/mg_hip.h; drivers: Solver::fas_* in mg_drivers.cpp). The linear part is the
// handle's constant operator (alpha, aniso, semi_xy, odd sizes, the shift of mg_set_shift), all faces Dirichlet -- or, with
// MG_FAS_ON_FACES and a non-zero mg_bc_set_faces mask, mg_bc.hip's operator with Neumann faces (section 23); the reaction
// g is pointwise, so every kernel is the 7-point stream of the constant operator plus a few flops on the centre value.
// With MG_FAS_ON_COEFFICIENT the linear part is mg_vc_*'s operator instead and the launches are mg_vc.hip's (section 24): of
// this file only k_fas_diff runs then.
//
//   FasOp<T, KIND>                       the point operator (Coef and G): res<DIM> and solve<DIM> of the contract below. The plain
//                                        form (residual / Jacobi sweep / one red-black colour pass, every shape) and the
//                                        coarsest-grid solve are mg_opfamily.h's k_op_plain<FasOp<T, KIND>, DIM, OP, SAVE> and
//                                        k_op_coarse<FasOp<T, KIND>, DIM>
//   FasFaceOp<T, KIND>                   the same with a mask of Neumann faces: bc_faces / bc_neighbours (mg_opfamily.h), then the reaction
//   k_fas_march<T, KIND, OP, SAVE, SRC, FACES>  the residual, the Jacobi sweep and the right-hand side of a theta step (OP_STEP, with or
//                                        without a source: mg_fas_heat_rhs) on 3-D levels with rows long enough to fill a wave
//                                        (fas_march_ok, mg_geom.h): k_bc_march's tile (mg_bc.hip) with one marched field; FACES: its
//                                        mirror too (a non-zero mask only: the mask-free instantiations are the code they were)
//   k_fas_coarse_rhs<T, DIM, WZ, KIND, FACES>  the FAS transition l -> l+1 in one launch: U(l+1) = E(l+1) = U(l) injected,
//                                        RHS(l+1) = R TMP(l) + N_c(U(l) injected), the coarse neighbours read from U(l)
//   k_fas_diff<T>                        e = x - e (the coarse correction U(l+1) - E(l+1), into E(l+1))
//
// Arithmetic contract (compiled with -ffp-contract=off; tests/fas_ref.py restates it in numpy), all in T, every operation
// rounded separately, c = the level's Coef (mg_level_coefficients: shift and aniso included), G = (T)gamma:
//   reaction     MG_FAS_CUBIC: q = u*u; g = q*u; gp = (T)3 * q.   MG_FAS_EXP: g = gp = exp(u) (the device library's exp / expf)
//   residual     sum = full_sum's expression (z-, y-, x-, d, x+, y+, z+); r = b - (sum + G*g); Dirichlet nodes: r = b - u;
//                the sum of r^2 over ALL nodes in double, fixed order, no atomics
//   point solve  s = offdiag_sum's expression; num = (b - s) - G*(g - gp*u); den = cd + G*gp; ps = num / den (the IEEE
//                quotient: one Newton step on the node's own equation); Dirichlet nodes take b. Nothing guards den.
//   Jacobi       u' = ps (omega == 1) or u_i + omega * (ps - u_i)
//   red-black    in place, colour (i + j + gz) & 1, colour 0 first; Dirichlet nodes take b with their colour
//   step         n0 = sum + G*g with the UNSHIFTED diagonal cd0; rhs = ((f + rdt*u_i) - omt*n0) * rth, without a source
//                (rdt*u_i - omt*n0) * rth; Dirichlet nodes: rhs = u_i (step_value, mg_opfamily.h; tests/step_ref.py)
// With gamma == 0 num = b - s and den = cd, and the correctly rounded quotient is div_cd's: mg_residual's and mg_smooth's bits.
// With a mask m != 0 (FasFaceOp, FACES): the unknowns are the nodes whose faces all lie in m, u(q) is the neighbour or its mirror
// image, sum / s are bc_point_res's / bc_point_solve's in their order, the Dirichlet nodes are those on a face outside m, and the
// transition restricts with bc_restrict_point and mirrors its coarse neighbours (tests/fasn_ref.py restates it). With gamma == 0
// these are mg_bc_*'s bits; with m == 0 the launchers take the mask-free operator, kernels and instantiations.
#include "mg_opfamily.h"

namespace mg {
namespace {

// the point solve from the off-diagonal sum s, the centre value and the right-hand side (fas_react and the Newton step:
// mg_opfamily.h, shared with mg_vc.hip)
template <typename T, int KIND>
__device__ __forceinline__ T fas_newton(const Coef<T> &c, T G, T s, T ui, T bi)
{
    return fas_newton_point<T, KIND>(G, bi - s, c.cd, ui);
}

// the point operator of the plain form and of the coarsest-grid solve (mg_opfamily.h)
template <typename T, int KIND>
struct FasOp {
    typedef T type;
    Coef<T> c;
    T G;

    template <int DIM>
    __device__ __forceinline__ T res(const Geom &g, const T *u, const T *b, int z, int y, int x) const
    {
        const long long i = lidx(g, z, y, x);
        T sum;
        if (on_boundary(g, z, y, x)) {
            sum = (T)1 * u[i];
        } else {
            T gv, gp;
            fas_react<T, KIND>(u[i], gv, gp);
            sum = full_sum<T, DIM>(u, i, g.pitch, g.plane, c) + G * gv;
        }
        return b[i] - sum;
    }

    template <int DIM>
    __device__ __forceinline__ T solve(const Geom &g, T omega, bool damped, const T *u, const T *b, int z, int y, int x) const
    {
        const long long i = lidx(g, z, y, x);
        const T bi = b[i];
        if (on_boundary(g, z, y, x)) return bi;
        const T s = offdiag_sum<T, DIM>(u, i, g.pitch, g.plane, c);
        const T ui = u[i];
        const T ps = fas_newton<T, KIND>(c, G, s, ui, bi);
        if (damped) return ui + omega * (ps - ui);
        return ps;
    }

    // the operator's value sum + G*g at an unknown (c.cd = cd0: the unshifted operator of the time steppers)
    template <int DIM>
    __device__ __forceinline__ bool n0(const Geom &g, const T *u, int z, int y, int x, bool stencil, T &v) const
    {
        if (on_boundary(g, z, y, x)) return true;
        if (stencil) {
            const long long i = lidx(g, z, y, x);
            T gv, gp;
            fas_react<T, KIND>(u[i], gv, gp);
            v = full_sum<T, DIM>(u, i, g.pitch, g.plane, c) + G * gv;
        }
        return false;
    }
};

// FasOp with Neumann faces (MG_FAS_ON_FACES and a non-zero mg_bc_set_faces mask): the linear part is mg_bc.hip's operator --
// a node on a face outside the mask is a Dirichlet node, every other node an unknown whose missing neighbours are mirror
// images (bc_faces, bc_neighbours) -- then the reaction. FasOp itself stays the mask-free operator of every other launch.
template <typename T, int KIND>
struct FasFaceOp {
    typedef T type;
    Coef<T> c;
    T G;
    int mask;

    // bc_point_res's sum (diag) / bc_point_solve's off-diagonal sum at unknown i on faces f
    template <int DIM, bool DIAG>
    __device__ __forceinline__ T lin_sum(const Geom &g, const T *u, long long i, int f) const
    {
        const BcNb n = bc_neighbours(g, i, f);
        T sum = 0;
        if (DIM == 3) sum += c.cz * u[n.zm];
        sum += c.cy * u[n.ym];
        sum += c.cx * u[n.xm];
        if (DIAG) sum += c.cd * u[i];
        sum += c.cx * u[n.xp];
        sum += c.cy * u[n.yp];
        if (DIM == 3) sum += c.cz * u[n.zp];
        return sum;
    }

    template <int DIM>
    __device__ __forceinline__ T res(const Geom &g, const T *u, const T *b, int z, int y, int x) const
    {
        const long long i = lidx(g, z, y, x);
        const int f = bc_faces(g, z, y, x);
        T sum;
        if (f & ~mask) {
            sum = (T)1 * u[i];
        } else {
            T gv, gp;
            fas_react<T, KIND>(u[i], gv, gp);
            sum = lin_sum<DIM, true>(g, u, i, f) + G * gv;
        }
        return b[i] - sum;
    }

    template <int DIM>
    __device__ __forceinline__ T solve(const Geom &g, T omega, bool damped, const T *u, const T *b, int z, int y, int x) const
    {
        const long long i = lidx(g, z, y, x);
        const T bi = b[i];
        const int f = bc_faces(g, z, y, x);
        if (f & ~mask) return bi;
        const T s = lin_sum<DIM, false>(g, u, i, f);
        const T ui = u[i];
        const T ps = fas_newton<T, KIND>(c, G, s, ui, bi);
        if (damped) return ui + omega * (ps - ui);
        return ps;
    }

    template <int DIM>
    __device__ __forceinline__ bool n0(const Geom &g, const T *u, int z, int y, int x, bool stencil, T &v) const
    {
        const int f = bc_faces(g, z, y, x);
        if (f & ~mask) return true;
        if (stencil) {
            const long long i = lidx(g, z, y, x);
            T gv, gp;
            fas_react<T, KIND>(u[i], gv, gp);
            v = lin_sum<DIM, true>(g, u, i, f) + G * gv;
        }
        return false;
    }
};

// ---------------------------------------------------------------- the marching tile (3-D)
// k_bc_march's tile: a lane owns one aligned 16-byte vector of x, a wave covers 64 vectors of MRY = 2 rows, MBW = 4 waves are
// stacked in y and the workgroup marches zc planes with the planes z-1, z, z+1 of u in registers. The reaction term is
// computed from the centre value the lane holds: no load and no branch is added in the interior; Dirichlet nodes are a select.
// OP_STEP: b is the source of the step (not loaded without SRC), st its scalars, c.cd = cd0; out = u on Dirichlet nodes.
// FACES (a non-zero mask of Neumann faces): k_bc_march's mirror, a select on values the lane holds anyway -- the element at
// x = 0 takes its right neighbour for the left one, row 0 takes row 1 for the halo row, plane 0 takes uzp for uzm, likewise at
// the high ends -- and the Dirichlet nodes are those on a face outside the mask. Only the odd last column of a 2^k + 1 row,
// an unknown when x-hi is in the mask, is computed from global memory by FasFaceOp's point functions (one lane per row).
// Without FACES every `FACES ?` below folds away: the mask-free tile is the code it was.
template <typename T, int KIND, int OP, bool SAVE, bool SRC = true, bool FACES = false>
__global__ __launch_bounds__(64 * MBW) void k_fas_march(Geom g, Coef<T> c, T G, T omega, const T *__restrict__ u,
                                                        const T *__restrict__ b, T *__restrict__ out, double *__restrict__ partials,
                                                        int nbx, int nby, int nbz, int zc, StepCoef<T> st, int mask)
{
    constexpr int V = Vec16<T>::n;
    constexpr bool STORE = OP != OP_RES || SAVE;
    constexpr bool LOADB = OP != OP_STEP || SRC;
    typedef typename Vec16<T>::type vec;
    __shared__ double sh[MBW];

    const int nblocks = nbx * nby * nbz;
    const int bid = xcd_block(blockIdx.x, (nblocks + 7) >> 3);
    if (bid >= nblocks) {   // the whole workgroup
        if (OP == OP_RES && threadIdx.x == 0) partials[blockIdx.x] = 0.;
        return;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int bx = bid % nbx, by = (bid / nbx) % nby, bz = bid / (nbx * nby);
    const int x0 = V * (bx * 64 + lane);
    const int x0c = min(x0, g.pitch - V);   // clamped for loads: every lane stays active
    const bool xfull = x0 + V <= g.nx;      // the lane's vector lies inside the row
    const int yb = (by * MBW + wv) * MRY;
    const int z0 = bz * zc, zend = min(z0 + zc, g.nz);
    // one column left over: the wave that holds the row's last full vector writes it as a full line
    const bool tail1 = g.nx % V == 1 && g.nx > V;
    const bool tailwave = tail1 && (bx * 64 * V <= g.nx - 1 - V) && (g.nx - 1 - V < (bx + 1) * 64 * V);
    const int part = (!tail1 && !xfull && x0 < g.nx) ? g.nx - x0 : 0;   // elements of a partial last vector stored one by one
    const int nown = xfull ? V : part;                                  // elements of the vector this lane stores and sums
    const bool damped = OP == OP_JAC && omega != (T)1;
    const int dir = FACES ? ~mask : ~0;   // the Dirichlet faces

    long long rowoff[MRY];
    bool yin[MRY], ybnd[MRY];
    int yface[MRY];
#pragma unroll
    for (int r = 0; r < MRY; r++) {
        const int y = yb + r;
        yin[r] = y < g.ny;
        const int yc = min(y, g.ny - 1);
        ybnd[r] = yc == 0 || yc == g.ny - 1;
        yface[r] = (yc == 0 ? FYLO : 0) | (yc == g.ny - 1 ? FYHI : 0);
        rowoff[r] = (long long)yc * g.pitch + x0c;
    }
    const long long off_lo = (long long)min(max(yb - 1, 0), g.ny - 1) * g.pitch + x0c;
    const long long off_hi = (long long)min(yb + MRY, g.ny - 1) * g.pitch + x0c;
    const bool edge_l = lane == 0 && x0c > 0, edge_r = lane == 63 && x0c + V < g.pitch;

    vec uzm[MRY], ucc[MRY], uzp[MRY];
    const T *pu = u + (long long)z0 * g.plane;
#pragma unroll
    for (int r = 0; r < MRY; r++) {
        uzm[r] = *(const vec *)(pu - g.plane + rowoff[r]);   // z0 == 0: the ghost plane, never used (plane 0 is Dirichlet or mirrored)
        ucc[r] = *(const vec *)(pu + rowoff[r]);
    }
    double acc = 0.;
    for (int z = z0; z < zend; z++, pu += g.plane) {
        const long long zo = (long long)z * g.plane;
        vec bv[MRY];
#pragma unroll
        for (int r = 0; r < MRY; r++) {
            uzp[r] = *(const vec *)(pu + g.plane + rowoff[r]);
            bv[r] = LOADB ? __builtin_nontemporal_load((const vec *)(b + zo + rowoff[r])) : (vec)(0);
        }
        const vec ulo = *(const vec *)(pu + off_lo), uhi = *(const vec *)(pu + off_hi);
        const int gz = g.gz0 + z;
        const bool zbnd = gz == 0 || gz == g.gnz - 1;
        const int zface = (gz == 0 ? FZLO : 0) | (gz == g.gnz - 1 ? FZHI : 0);
#pragma unroll
        for (int r = 0; r < MRY; r++) {
            T uel = 0, uer = 0;
            if (edge_l) uel = pu[rowoff[r] - 1];
            if (edge_r) uer = pu[rowoff[r] + V];
            const T uxm = lane_from_prev(ucc[r][V - 1], uel), uxp = lane_from_next(ucc[r][0], uer);
            const vec uym0 = (r > 0) ? ucc[r > 0 ? r - 1 : 0] : ulo, uyp0 = (r < MRY - 1) ? ucc[r < MRY - 1 ? r + 1 : 0] : uhi;
            // the mirror in y and z: values the lane holds anyway
            const vec uym = (FACES && (yface[r] & FYLO)) ? uyp0 : uym0, uyp = (FACES && (yface[r] & FYHI)) ? uym0 : uyp0;
            const vec uzl = (FACES && (zface & FZLO)) ? uzp[r] : uzm[r], uzh = (FACES && (zface & FZHI)) ? uzm[r] : uzp[r];
            const bool rbnd = zbnd || ybnd[r];
            const int rface = zface | yface[r];
            vec res;
#pragma unroll
            for (int e = 0; e < V; e++) {
                const T ui = ucc[r][e], bi = bv[r][e];
                const T ul0 = (e == 0) ? uxm : ucc[r][e > 0 ? e - 1 : 0];
                const T ur0 = (e == V - 1) ? uxp : ucc[r][e < V - 1 ? e + 1 : 0];
                const int xface = (x0 + e == 0 ? FXLO : 0) | (x0 + e == g.nx - 1 ? FXHI : 0);
                const T ul = (FACES && (xface & FXLO)) ? ur0 : ul0, ur = (FACES && (xface & FXHI)) ? ul0 : ur0;
                const bool dn = FACES ? ((rface | xface) & dir) != 0 : (rbnd || x0 + e == 0 || x0 + e == g.nx - 1);
                T sum = 0;
                sum += c.cz * uzl[e];
                sum += c.cy * uym[e];
                sum += c.cx * ul;
                if (OP == OP_RES || OP == OP_STEP) sum += c.cd * ui;
                sum += c.cx * ur;
                sum += c.cy * uyp[e];
                sum += c.cz * uzh[e];
                if (OP == OP_RES) {
                    T gv, gp;
                    fas_react<T, KIND>(ui, gv, gp);
                    res[e] = dn ? bi - ui : bi - (sum + G * gv);
                } else if (OP == OP_STEP) {
                    T gv, gp;
                    fas_react<T, KIND>(ui, gv, gp);
                    res[e] = dn ? ui : step_value<T, SRC>(st, ui, bi, sum + G * gv);
                } else {
                    const T ps = fas_newton<T, KIND>(c, G, sum, ui, bi);
                    res[e] = dn ? bi : (damped ? ui + omega * (ps - ui) : ps);
                }
            }
            if (yin[r]) {
                if (OP == OP_RES) {
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
                    // column nx-1 as one full 128-byte line: value + zero padding. Without FACES it is a Dirichlet node; with an
                    // x-hi Neumann face it is an unknown: the plain form's point function computes it (u is never the output)
                    const int j = lane - 56;
                    constexpr int LINE = 128 / (int)sizeof(T);
                    const int xs = g.nx - 1 + V * j;
                    const int line_end = ((g.nx - 1) / LINE + 1) * LINE;
                    const long long ro = zo + (rowoff[r] - x0c);
                    if (xs < line_end) {
                        vec tv = (vec)(0);
                        if (FACES && j == 0) {
                            const FasFaceOp<T, KIND> op{c, G, mask};
                            if (OP == OP_RES) {
                                const T rt = op.template res<3>(g, u, b, z, yb + r, g.nx - 1);
                                acc += (double)rt * (double)rt;
                                tv[0] = rt;
                            } else if (OP == OP_STEP) {
                                const long long it = ro + g.nx - 1;
                                const T ut = u[it];
                                T n0 = (T)0;
                                const bool fixed = op.template n0<3>(g, u, z, yb + r, g.nx - 1, true, n0);
                                tv[0] = fixed ? ut : step_value<T, SRC>(st, ut, SRC ? b[it] : (T)0, n0);
                            } else {
                                tv[0] = op.template solve<3>(g, omega, damped, u, b, z, yb + r, g.nx - 1);
                            }
                        } else if (j == 0 && OP == OP_STEP) {
                            tv[0] = u[ro + g.nx - 1];
                        } else if (j == 0) {
                            const T bt = b[ro + g.nx - 1];
                            if (OP == OP_RES) {
                                const T rt = bt - (T)1 * u[ro + g.nx - 1];
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
        for (int r = 0; r < MRY; r++) { uzm[r] = ucc[r]; ucc[r] = uzp[r]; }
    }
    if (OP == OP_RES) {
        const double s = block_sum(acc, sh);
        if (threadIdx.x == 0) partials[blockIdx.x] = s;
    }
}

// ---------------------------------------------------------------- the FAS transition l -> l+1
// uf = U(l), rf = TMP(l) (the residual of level l); per coarse node: uc = uf at the even fine node -> uco and eco;
// rc = restrict_fw_point(rf) (inject: rf at the even fine node); rhsc = rc + (full_sum_c(uc) + G*g(uc)) with the coarse
// neighbours read from uf at distance 2 (z: 1 on a semi transition); coarse Dirichlet nodes: rhsc = uc. cc: Coef of level l+1.
// FACES (a non-zero mask of Neumann faces): the Dirichlet nodes are the coarse nodes on a face outside the mask, rc is
// k_bc_restrict's mirrored full weighting (bc_restrict_point: injecting the residual at the coarse nodes of a Neumann face
// makes the cycle diverge) and a coarse neighbour that leaves the grid is its mirror image in uf.
template <typename T, int DIM, bool WZ, int KIND, bool FACES>
__global__ __launch_bounds__(OP_THREADS) void k_fas_coarse_rhs(Geom gf, Geom gc, Coef<T> cc, T G, int inject, const T *__restrict__ uf,
                                                                const T *__restrict__ rf, T *__restrict__ uco, T *__restrict__ eco,
                                                                T *__restrict__ rhsc, int mask)
{
    const long long nitems = (long long)gc.nx * gc.ny * gc.nz;
    for (long long it = (long long)blockIdx.x * OP_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * OP_THREADS) {
        const long long row = it / gc.nx;
        const int x = (int)(it - row * gc.nx), y = (int)(row % gc.ny), z = (int)(row / gc.ny);
        const int fz = (DIM == 3) ? (WZ ? 2 * (gc.gz0 + z) - gf.gz0 : z) : 0;
        const long long fi = lidx(gf, fz, 2 * y, 2 * x), ci = lidx(gc, z, y, x);
        const T uc = uf[fi];
        T rhs;
        const int cf = FACES ? bc_faces(gc, z, y, x) : 0;
        if (FACES ? (cf & ~mask) != 0 : on_boundary(gc, z, y, x)) {
            rhs = uc;
        } else {
            const T rc = inject ? rf[fi]
                                : (FACES ? bc_restrict_point<T, DIM, WZ>(gf, gc, rf, z, y, x) : restrict_fw_point<T, DIM, WZ>(gf, gc, rf, z, y, x));
            const long long sy = 2 * (long long)gf.pitch, sz = WZ ? 2 * gf.plane : gf.plane;
            // the coarse neighbours in uf; on a Neumann face the one that leaves the grid is its mirror image
            const long long oxm = (cf & FXLO) ? 2 : -2, oxp = (cf & FXHI) ? -2 : 2;
            const long long oym = (cf & FYLO) ? sy : -sy, oyp = (cf & FYHI) ? -sy : sy;
            const long long ozm = (cf & FZLO) ? sz : -sz, ozp = (cf & FZHI) ? -sz : sz;
            T gv, gp;
            fas_react<T, KIND>(uc, gv, gp);
            T sum = 0;
            if (DIM == 3) sum += cc.cz * uf[fi + ozm];
            sum += cc.cy * uf[fi + oym];
            sum += cc.cx * uf[fi + oxm];
            sum += cc.cd * uc;
            sum += cc.cx * uf[fi + oxp];
            sum += cc.cy * uf[fi + oyp];
            if (DIM == 3) sum += cc.cz * uf[fi + ozp];
            rhs = rc + (sum + G * gv);
        }
        uco[ci] = uc;
        eco[ci] = uc;
        rhsc[ci] = rhs;
    }
}

// e = x - e on every node
template <typename T>
__global__ __launch_bounds__(OP_THREADS) void k_fas_diff(Geom g, const T *__restrict__ x_, T *__restrict__ e)
{
    const long long nitems = (long long)g.nx * g.ny * g.nz;
    for (long long it = (long long)blockIdx.x * OP_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * OP_THREADS) {
        const long long row = it / g.nx;
        const int x = (int)(it - row * g.nx), y = (int)(row % g.ny), z = (int)(row / g.ny);
        const long long i = lidx(g, z, y, x);
        e[i] = x_[i] - e[i];
    }
}

// ---------------------------------------------------------------- launchers
// launch(op) with op = the point operator of the reaction `kind`: the launches of mg_opfamily.h take their template arguments
// from its type. mask: the Neumann faces; 0 = the mask-free operator, the launches of a handle without MG_FAS_ON_FACES
template <typename T, typename Launch>
auto with_fas_op(int kind, const Coef<T> &c, T G, int mask, Launch &&launch)
{
    if (mask) {
        if (kind == FAS_CUBIC) return launch(FasFaceOp<T, FAS_CUBIC>{c, G, mask});
        return launch(FasFaceOp<T, FAS_EXP>{c, G, mask});
    }
    if (kind == FAS_CUBIC) return launch(FasOp<T, FAS_CUBIC>{c, G});
    return launch(FasOp<T, FAS_EXP>{c, G});
}

}  // namespace

template <typename T>
int launch_fas_residual(hipStream_t s, const Geom &g, const Coef<T> &c, int kind, T G, int mask, const T *u, const T *b, T *r,
                        double *partials, int cap, bool plain)
{
    if (march_takes<T>(g, plain)) {
        const MarchGrid m = march_grid<T>(g);
        if (m.grid <= cap) {
            const dim3 gr(m.grid), bl(64 * MBW);
#define MG_FAS(KIND, SAVE, FACES) hipLaunchKernelGGL((k_fas_march<T, KIND, OP_RES, SAVE, true, FACES>), gr, bl, 0, s, g, c, G, (T)1, u, b, r, partials, m.nbx, m.nby, m.nbz, m.zc, StepCoef<T>{}, mask)
#define MG_FAS_F(KIND, SAVE) if (mask) MG_FAS(KIND, SAVE, true); else MG_FAS(KIND, SAVE, false);
            if (kind == FAS_CUBIC) { if (r) { MG_FAS_F(FAS_CUBIC, true) } else { MG_FAS_F(FAS_CUBIC, false) } }
            else { if (r) { MG_FAS_F(FAS_EXP, true) } else { MG_FAS_F(FAS_EXP, false) } }
#undef MG_FAS_F
#undef MG_FAS
            return m.grid;
        }
    }
    return with_fas_op(kind, c, G, mask, [&](auto op) { return plain_residual(s, g, op, u, b, r, partials, cap); });
}

template <typename T>
void launch_fas_jacobi(hipStream_t s, const Geom &g, const Coef<T> &c, int kind, T G, int mask, T omega, const T *u, const T *b, T *out,
                       bool plain)
{
    if (march_takes<T>(g, plain)) {
        const MarchGrid m = march_grid<T>(g);
        const dim3 gr(m.grid), bl(64 * MBW);
#define MG_FAS(KIND, FACES) hipLaunchKernelGGL((k_fas_march<T, KIND, OP_JAC, false, true, FACES>), gr, bl, 0, s, g, c, G, omega, u, b, out, (double *)nullptr, m.nbx, m.nby, m.nbz, m.zc, StepCoef<T>{}, mask)
        if (kind == FAS_CUBIC) { if (mask) MG_FAS(FAS_CUBIC, true); else MG_FAS(FAS_CUBIC, false); }
        else { if (mask) MG_FAS(FAS_EXP, true); else MG_FAS(FAS_EXP, false); }
#undef MG_FAS
        return;
    }
    with_fas_op(kind, c, G, mask, [&](auto op) { plain_jacobi(s, g, op, omega, u, b, out); });
}

template <typename T>
void launch_fas_heat_rhs(hipStream_t s, const Geom &g, const Coef<T> &c0, int kind, T G, int mask, double dt, double theta, const T *u,
                         const T *f, T *out, bool plain)
{
    const StepCoef<T> st = step_coef<T>(dt, theta);
    if (march_takes<T>(g, plain)) {
        const MarchGrid m = march_grid<T>(g);
        const dim3 gr(m.grid), bl(64 * MBW);
#define MG_FAS(KIND, SRC, FACES) hipLaunchKernelGGL((k_fas_march<T, KIND, OP_STEP, true, SRC, FACES>), gr, bl, 0, s, g, c0, G, (T)1, u, f, out, (double *)nullptr, m.nbx, m.nby, m.nbz, m.zc, st, mask)
#define MG_FAS_F(KIND, SRC) if (mask) MG_FAS(KIND, SRC, true); else MG_FAS(KIND, SRC, false);
        if (kind == FAS_CUBIC) { if (f) { MG_FAS_F(FAS_CUBIC, true) } else { MG_FAS_F(FAS_CUBIC, false) } }
        else { if (f) { MG_FAS_F(FAS_EXP, true) } else { MG_FAS_F(FAS_EXP, false) } }
#undef MG_FAS_F
#undef MG_FAS
        return;
    }
    with_fas_op(kind, c0, G, mask, [&](auto op) { plain_step(s, g, op, st, u, f, out); });
}

template <typename T>
void launch_fas_rb_colour(hipStream_t s, const Geom &g, const Coef<T> &c, int kind, T G, int mask, int colour, T *u, const T *b)
{
    with_fas_op(kind, c, G, mask, [&](auto op) { plain_rb_colour(s, g, op, colour, u, b); });
}

template <typename T>
void launch_fas_coarse_rhs(hipStream_t s, const Geom &gf, const Geom &gc, const Coef<T> &cc, int kind, T G, int mask, bool inject,
                           const T *uf, const T *rf, T *uc, T *ec, T *rhsc)
{
    const dim3 gr(plain_grid((long long)gc.nx * gc.ny * gc.nz, OP_MAX_BLOCKS)), bl(OP_THREADS);
    const int inj = inject ? 1 : 0;
#define MG_FAS(DIM, WZ, KIND, FACES) hipLaunchKernelGGL((k_fas_coarse_rhs<T, DIM, WZ, KIND, FACES>), gr, bl, 0, s, gf, gc, cc, G, inj, uf, rf, uc, ec, rhsc, mask)
#define MG_FAS_M(DIM, WZ, KIND) if (mask) MG_FAS(DIM, WZ, KIND, true); else MG_FAS(DIM, WZ, KIND, false);
#define MG_FAS_K(DIM, WZ) if (kind == FAS_CUBIC) { MG_FAS_M(DIM, WZ, FAS_CUBIC) } else { MG_FAS_M(DIM, WZ, FAS_EXP) }
    if (gc.dim == 3 && is_semi_transition(gf, gc)) { MG_FAS_K(3, false) }
    else if (gc.dim == 3) { MG_FAS_K(3, true) }
    else { MG_FAS_K(2, false) }
#undef MG_FAS_K
#undef MG_FAS_M
#undef MG_FAS
}

template <typename T>
void launch_fas_diff(hipStream_t s, const Geom &g, const T *x, T *e)
{
    const int nb = plain_grid((long long)g.nx * g.ny * g.nz, OP_MAX_BLOCKS);
    hipLaunchKernelGGL((k_fas_diff<T>), dim3(nb), dim3(OP_THREADS), 0, s, g, x, e);
}

template <typename T>
void launch_fas_coarse(hipStream_t s, const Geom &g, const Coef<T> &c, int kind, T G, int mask, T omega, int smoother, T *x, T *tmp,
                       const T *rhs, int maxit, double tol, int fixed, CoarseOut *d_out)
{
    with_fas_op(kind, c, G, mask, [&](auto op) { coarse_solve(s, g, op, omega, smoother, x, tmp, rhs, maxit, tol, fixed, d_out); });
}

#define MG_FAS_INST(T)                                                                                                                    \
    template int launch_fas_residual<T>(hipStream_t, const Geom &, const Coef<T> &, int, T, int, const T *, const T *, T *, double *, int, \
                                        bool);                                                                                            \
    template void launch_fas_jacobi<T>(hipStream_t, const Geom &, const Coef<T> &, int, T, int, T, const T *, const T *, T *, bool);      \
    template void launch_fas_heat_rhs<T>(hipStream_t, const Geom &, const Coef<T> &, int, T, int, double, double, const T *, const T *,   \
                                         T *, bool);                                                                                      \
    template void launch_fas_rb_colour<T>(hipStream_t, const Geom &, const Coef<T> &, int, T, int, int, T *, const T *);                  \
    template void launch_fas_coarse_rhs<T>(hipStream_t, const Geom &, const Geom &, const Coef<T> &, int, T, int, bool, const T *,        \
                                           const T *, T *, T *, T *);                                                                     \
    template void launch_fas_diff<T>(hipStream_t, const Geom &, const T *, T *);                                                          \
    template void launch_fas_coarse<T>(hipStream_t, const Geom &, const Coef<T> &, int, T, int, T, int, T *, T *, const T *, int, double, \
                                       int, CoarseOut *);
MG_FAS_INST(double)
MG_FAS_INST(float)
#undef MG_FAS_INST

}  // namespace mg
