// mg_vc.hip -- kernels of the variable-coefficient operator -div(a grad u) + sigma u (mg_vc_*, include/mg_hip.h; drivers:
// Solver::vc_* in mg_drivers.cpp). The coefficient a is a nodal, level-shaped array of every level (Level::vc_a); the
// transfers do not depend on the operator, so only the smoother, the residual, the coarsest-grid solve and the Krylov
// direction kernel live here.
//
//   VcOp<T>                        the point operator (VcCoef and a): res<DIM> and solve<DIM> of the contract below. The plain
//                                  form (residual / Jacobi sweep / one red-black colour pass, every shape) and the
//                                  coarsest-grid solve are mg_opfamily.h's k_op_plain<VcOp<T>, DIM, OP, SAVE> and
//                                  k_op_coarse<VcOp<T>, DIM>
//   k_vc_march<T, OP, SAVE, SRC>   the residual, the Jacobi sweep and the right-hand side of a theta step (OP_STEP, with or
//                                  without a source: mg_vc_heat_rhs) on 3-D levels with rows long enough to fill a wave
//                                  (vc_march_ok, mg_geom.h)
//   k_vc_cg_direction<T, DIM>      k_cg_direction_apply (mg_krylov.hip) with q = L p'
//   k_vcn_cg_direction<T, DIM>     the same with a face mask: mirrored neighbours, Dirichlet nodes by the mask, p'.q weighted
//   k_vcn_cg_dots<T>               k_cg_dots (mg_krylov.hip) with the weights: sum w z r and sum w z q
//
// NEUMANN FACES (mg_vc_set_faces). A face mask (enum mg_face) names the zero-flux faces; the node
// classes are mg_bc.hip's: a node on at least one face that is not in the mask is a Dirichlet node, every other node is an
// unknown whose missing neighbour q is the mirror image inside the box, for a and for u alike, so a mirrored slot counts
// twice in s and in d. Nothing else of the contract below changes. The template flag MIR selects that form; without it
// (mask 0) every kernel is the code it was before the mask existed, and the launchers pick MIR only for a non-zero mask.
// w = 1/2 per Neumann face a node lies on makes diag(w) L symmetric: the Krylov dots of a masked handle carry it.
//
// The marching tile is k_heat_rhs's (mg_heat.hip) with TWO marched fields: a lane owns one aligned 16-byte vector of x, a
// wave covers 64 vectors of MRY = 2 rows, MBW = 4 waves are stacked in y and the workgroup marches zc planes with the
// planes z-1, z, z+1 of u AND a of its columns in registers, so each is loaded once per workgroup column. x-neighbours
// are the neighbouring lanes' values (whole-wave DPP shifts; the two edge lanes load theirs), y-neighbours the wave's
// other row or two halo rows that hit L1 / L2. b is loaded and r / u' stored non-temporally, the block order is
// XCD-aware, the odd last column is written as one full 128-byte line as in mg_heat.hip. Ghost planes and padding
// columns are read (they exist and hold zeros) and what is computed from them is dropped: only Dirichlet nodes touch them.
// With MIR the mirror is a select between values the lane holds anyway, for both fields, as in k_bc_march: the element at
// x = 0 takes its right neighbour for the left one, row 0 takes row 1 for the halo row, plane 0 takes uzp / azp for uzm / azm
// (and likewise at the high ends); no load and no branch is added in the interior. Only the odd last column of a 2^k + 1
// row is computed from global memory by the plain form's point function, because with an x-hi Neumann face it is an unknown.
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
//   step         n0 = d * u_i - s with d started from (T)0 (the UNSHIFTED operator); rhs = ((f + rdt*u_i) - omt*n0) * rth, without a
//                source (rdt*u_i - omt*n0) * rth; Dirichlet nodes: rhs = u_i (step_value, mg_opfamily.h; tests/step_ref.py)
#include "mg_opfamily.h"

namespace mg {
namespace {

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

// s and d at element i with the neighbours n (or their mirror images); uat(q, k) = u at element q, the k-th neighbour in
// row order (0: z-, 1: y-, 2: x-, 3: x+, 4: y+, 5: z+)
template <typename T, int DIM, typename F>
__device__ __forceinline__ void vc_parts(F &&uat, const T *a, long long i, const BcNb &n, const VcCoef<T> &c, T &s, T &d)
{
    const T ai = a[i];
    s = (T)0;
    d = c.sigma;
    if (DIM == 3) vc_nb<T>(c.wz, ai, a[n.zm], uat(n.zm, 0), s, d);
    vc_nb<T>(c.wy, ai, a[n.ym], uat(n.ym, 1), s, d);
    vc_nb<T>(c.wx, ai, a[n.xm], uat(n.xm, 2), s, d);
    vc_nb<T>(c.wx, ai, a[n.xp], uat(n.xp, 3), s, d);
    vc_nb<T>(c.wy, ai, a[n.yp], uat(n.yp, 4), s, d);
    if (DIM == 3) vc_nb<T>(c.wz, ai, a[n.zp], uat(n.zp, 5), s, d);
}

__device__ __forceinline__ BcNb vc_straight(const Geom &g, long long i)
{
    return BcNb{i - g.plane, i - g.pitch, i - 1, i + 1, i + g.pitch, i + g.plane};
}

// the mask of a VcOp: no member without MIR, so the mask-0 kernels take the arguments they always took
template <bool MIR>
struct VcMask {
    int mask;
};
template <>
struct VcMask<false> {
    static constexpr int mask = 0;
};

// the point operator of the plain form and of the coarsest-grid solve (mg_opfamily.h)
template <typename T, bool MIR = false>
struct VcOp : VcMask<MIR> {
    typedef T type;
    VcCoef<T> c;
    const T *__restrict__ a;

    // true at a Dirichlet node; else n = the neighbours of unknown i, mirrored on the Neumann faces it lies on
    __device__ __forceinline__ bool fixed(const Geom &g, int z, int y, int x, long long i, BcNb &n) const
    {
        if (MIR) {
            const int f = bc_faces(g, z, y, x);
            if (f & ~this->mask) return true;
            n = bc_neighbours(g, i, f);
            return false;
        }
        if (on_boundary(g, z, y, x)) return true;
        n = vc_straight(g, i);
        return false;
    }

    template <int DIM>
    __device__ __forceinline__ T res(const Geom &g, const T *u, const T *b, int z, int y, int x) const
    {
        const long long i = lidx(g, z, y, x);
        BcNb n;
        if (fixed(g, z, y, x, i, n)) return b[i] - u[i];
        T s, d;
        vc_parts<T, DIM>([&](long long q, int) { return u[q]; }, a, i, n, c, s, d);
        return b[i] - (d * u[i] - s);
    }

    template <int DIM>
    __device__ __forceinline__ T solve(const Geom &g, T omega, bool damped, const T *u, const T *b, int z, int y, int x) const
    {
        const long long i = lidx(g, z, y, x);
        const T bi = b[i];
        BcNb n;
        if (fixed(g, z, y, x, i, n)) return bi;
        T s, d;
        vc_parts<T, DIM>([&](long long q, int) { return u[q]; }, a, i, n, c, s, d);
        const T ps = (bi + s) / d;
        if (damped) {
            const T ui = u[i];
            return ui + omega * (ps - ui);
        }
        return ps;
    }

    // the operator's value d * u_i - s at an unknown (c.sigma = 0: the unshifted operator of the time steppers)
    template <int DIM>
    __device__ __forceinline__ bool n0(const Geom &g, const T *u, int z, int y, int x, bool stencil, T &v) const
    {
        const long long i = lidx(g, z, y, x);
        BcNb n;
        if (fixed(g, z, y, x, i, n)) return true;
        if (stencil) {
            T s, d;
            vc_parts<T, DIM>([&](long long q, int) { return u[q]; }, a, i, n, c, s, d);
            v = d * u[i] - s;
        }
        return false;
    }
};

template <typename T, bool MIR>
__host__ __device__ VcOp<T, MIR> vc_op(const VcCoef<T> &c, const T *a, int mask)
{
    VcOp<T, MIR> op;
    op.c = c;
    op.a = a;
    if constexpr (MIR) op.mask = mask;
    return op;
}

// ---------------------------------------------------------------- the marching tile (3-D)
// OP_STEP: b is the source of the step (not loaded without SRC), st its scalars, c.sigma = 0; out = u on Dirichlet nodes.
// MIR: the faces of `mask` are Neumann (not looked at otherwise)
template <typename T, int OP, bool SAVE, bool SRC = true, bool MIR = false>
__global__ __launch_bounds__(64 * MBW) void k_vc_march(Geom g, VcCoef<T> c, T omega, const T *__restrict__ u, const T *__restrict__ a,
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

    long long rowoff[MRY];
    bool yin[MRY], ybnd[MRY];
#pragma unroll
    for (int r = 0; r < MRY; r++) {
        const int y = yb + r;
        yin[r] = y < g.ny;
        const int yc = min(y, g.ny - 1);
        ybnd[r] = (yc == 0) || (yc == g.ny - 1);
        rowoff[r] = (long long)yc * g.pitch + x0c;
    }
    const long long off_lo = (long long)min(max(yb - 1, 0), g.ny - 1) * g.pitch + x0c;
    const long long off_hi = (long long)min(yb + MRY, g.ny - 1) * g.pitch + x0c;
    const bool edge_l = lane == 0 && x0c > 0, edge_r = lane == 63 && x0c + V < g.pitch;

    vec uzm[MRY], ucc[MRY], uzp[MRY], azm[MRY], acc_[MRY], azp[MRY];
    const T *pu = u + (long long)z0 * g.plane, *pa = a + (long long)z0 * g.plane;
#pragma unroll
    for (int r = 0; r < MRY; r++) {
        uzm[r] = *(const vec *)(pu - g.plane + rowoff[r]);
        ucc[r] = *(const vec *)(pu + rowoff[r]);
        azm[r] = *(const vec *)(pa - g.plane + rowoff[r]);
        acc_[r] = *(const vec *)(pa + rowoff[r]);
    }
    double acc = 0.;
    for (int z = z0; z < zend; z++, pu += g.plane, pa += g.plane) {
        const long long zo = (long long)z * g.plane;
        vec bv[MRY];
#pragma unroll
        for (int r = 0; r < MRY; r++) {
            uzp[r] = *(const vec *)(pu + g.plane + rowoff[r]);
            azp[r] = *(const vec *)(pa + g.plane + rowoff[r]);
            bv[r] = LOADB ? __builtin_nontemporal_load((const vec *)(b + zo + rowoff[r])) : (vec)(0);
        }
        const vec ulo = *(const vec *)(pu + off_lo), uhi = *(const vec *)(pu + off_hi);
        const vec alo = *(const vec *)(pa + off_lo), ahi = *(const vec *)(pa + off_hi);
        const int gz = g.gz0 + z;
        const bool zb = (gz == 0) || (gz == g.gnz - 1);
#pragma unroll
        for (int r = 0; r < MRY; r++) {
            T uel = 0, uer = 0, ael = 0, aer = 0;
            if (edge_l) { uel = pu[rowoff[r] - 1]; ael = pa[rowoff[r] - 1]; }
            if (edge_r) { uer = pu[rowoff[r] + V]; aer = pa[rowoff[r] + V]; }
            const T uxm = lane_from_prev(ucc[r][V - 1], uel), uxp = lane_from_next(ucc[r][0], uer);
            const T axm = lane_from_prev(acc_[r][V - 1], ael), axp = lane_from_next(acc_[r][0], aer);
            const vec uym = (r > 0) ? ucc[r > 0 ? r - 1 : 0] : ulo, uyp = (r < MRY - 1) ? ucc[r < MRY - 1 ? r + 1 : 0] : uhi;
            const vec aym = (r > 0) ? acc_[r > 0 ? r - 1 : 0] : alo, ayp = (r < MRY - 1) ? acc_[r < MRY - 1 ? r + 1 : 0] : ahi;
            const bool rb = zb || ybnd[r];
            vec res;
#pragma unroll
            for (int e = 0; e < V; e++) {
                const T ui = ucc[r][e], ai = acc_[r][e], bi = bv[r][e];
                const T ul = (e == 0) ? uxm : ucc[r][e > 0 ? e - 1 : 0], al = (e == 0) ? axm : acc_[r][e > 0 ? e - 1 : 0];
                const T ur = (e == V - 1) ? uxp : ucc[r][e < V - 1 ? e + 1 : 0], ar = (e == V - 1) ? axp : acc_[r][e < V - 1 ? e + 1 : 0];
                T s = (T)0, d = c.sigma;
                bool bnd;
                if constexpr (MIR) {
                    // the mirror: a select between values the lane holds anyway, element by element; Dirichlet nodes by the mask
                    const int yf = (yb + r == 0 ? FYLO : 0) | (yb + r == g.ny - 1 ? FYHI : 0);
                    const int zf = (gz == 0 ? FZLO : 0) | (gz == g.gnz - 1 ? FZHI : 0);
                    const int xf = (x0 + e == 0 ? FXLO : 0) | (x0 + e == g.nx - 1 ? FXHI : 0);
                    vc_nb<T>(c.wz, ai, (zf & FZLO) ? azp[r][e] : azm[r][e], (zf & FZLO) ? uzp[r][e] : uzm[r][e], s, d);
                    vc_nb<T>(c.wy, ai, (yf & FYLO) ? ayp[e] : aym[e], (yf & FYLO) ? uyp[e] : uym[e], s, d);
                    vc_nb<T>(c.wx, ai, (xf & FXLO) ? ar : al, (xf & FXLO) ? ur : ul, s, d);
                    vc_nb<T>(c.wx, ai, (xf & FXHI) ? al : ar, (xf & FXHI) ? ul : ur, s, d);
                    vc_nb<T>(c.wy, ai, (yf & FYHI) ? aym[e] : ayp[e], (yf & FYHI) ? uym[e] : uyp[e], s, d);
                    vc_nb<T>(c.wz, ai, (zf & FZHI) ? azm[r][e] : azp[r][e], (zf & FZHI) ? uzm[r][e] : uzp[r][e], s, d);
                    bnd = ((zf | yf | xf) & ~mask) != 0;
                } else {
                    vc_nb<T>(c.wz, ai, azm[r][e], uzm[r][e], s, d);
                    vc_nb<T>(c.wy, ai, aym[e], uym[e], s, d);
                    vc_nb<T>(c.wx, ai, al, ul, s, d);
                    vc_nb<T>(c.wx, ai, ar, ur, s, d);
                    vc_nb<T>(c.wy, ai, ayp[e], uyp[e], s, d);
                    vc_nb<T>(c.wz, ai, azp[r][e], uzp[r][e], s, d);
                    bnd = rb || (x0 + e == 0) || (x0 + e == g.nx - 1);
                }
                T v;
                if (OP == OP_RES) {
                    v = bnd ? bi - ui : bi - (d * ui - s);
                } else if (OP == OP_STEP) {
                    v = bnd ? ui : step_value<T, SRC>(st, ui, bi, d * ui - s);
                } else {
                    const T ps = (bi + s) / d;
                    v = bnd ? bi : (damped ? ui + omega * (ps - ui) : ps);
                }
                res[e] = v;
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
                    // column nx-1 (Dirichlet: r = b - u, u' = b, the step's rhs = u) as one full 128-byte line: value + zero padding.
                    // MIR: with an x-hi Neumann face the node is an unknown and the plain form's point function computes it
                    // (one lane per row; u is never the output array)
                    const int j = lane - 56;
                    constexpr int LINE = 128 / (int)sizeof(T);
                    const int xs = g.nx - 1 + V * j;
                    const int line_end = ((g.nx - 1) / LINE + 1) * LINE;
                    const long long ro = zo + (rowoff[r] - x0c);
                    if (xs < line_end) {
                        vec tv = (vec)(0);
                        if (MIR && j == 0) {
                            const VcOp<T, true> op = vc_op<T, true>(c, a, mask);
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
        for (int r = 0; r < MRY; r++) { uzm[r] = ucc[r]; ucc[r] = uzp[r]; azm[r] = acc_[r]; acc_[r] = azp[r]; }
    }
    if (OP == OP_RES) {
        const double s = block_sum(acc, sh);
        if (threadIdx.x == 0) partials[blockIdx.x] = s;
    }
}

// ---------------------------------------------------------------- p' = z + beta p, q = L p', sum p'.q
template <typename T, int DIM>
__global__ __launch_bounds__(OP_THREADS) void k_vc_cg_direction(Geom g, VcCoef<T> c, const T *__restrict__ zv, const T *__restrict__ p,
                                                                const T *__restrict__ a, T *__restrict__ pn, T *__restrict__ q,
                                                                const CgScalars *__restrict__ sc, double *__restrict__ partials)
{
    __shared__ double sh[OP_THREADS / 64];
    if (sc->bad != 0) return;   // breakdown flagged by an earlier tail: nothing is written, the tail that follows returns too
    const T beta = (T)sc->beta;
    const long long nitems = (long long)g.nx * g.ny * g.nz;
    double acc = 0.;
    for (long long it = (long long)blockIdx.x * OP_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * OP_THREADS) {
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
            }, a, i, vc_straight(g, i), c, s, d);
            qv = d * pc - s;
            acc += (double)pc * (double)qv;
        }
        pn[i] = pc;
        q[i] = qv;
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---------------------------------------------------------------- the same with a face mask; sum w p'.q
// p' and q are 0 on the Dirichlet nodes of the mask; a mirrored neighbour is the value of the node it mirrors
template <typename T, int DIM>
__global__ __launch_bounds__(OP_THREADS) void k_vcn_cg_direction(Geom g, VcCoef<T> c, int mask, const T *__restrict__ zv,
                                                                 const T *__restrict__ p, const T *__restrict__ a, T *__restrict__ pn,
                                                                 T *__restrict__ q, const CgScalars *__restrict__ sc,
                                                                 double *__restrict__ partials)
{
    __shared__ double sh[OP_THREADS / 64];
    if (sc->bad != 0) return;
    const T beta = (T)sc->beta;
    const long long nitems = (long long)g.nx * g.ny * g.nz;
    double acc = 0.;
    for (long long it = (long long)blockIdx.x * OP_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * OP_THREADS) {
        const long long row = it / g.nx;
        const int x = (int)(it - row * g.nx), y = (int)(row % g.ny), z = (int)(row / g.ny);
        const long long i = lidx(g, z, y, x);
        const int f = bc_faces(g, z, y, x);
        T pc = (T)0, qv = (T)0;
        if (!(f & ~mask)) {
            pc = zv[i] + beta * p[i];
            // the coordinates of the six neighbours, mirrored like their indices
            const int zs[2] = {(f & FZLO) ? z + 1 : z - 1, (f & FZHI) ? z - 1 : z + 1};
            const int ys[2] = {(f & FYLO) ? y + 1 : y - 1, (f & FYHI) ? y - 1 : y + 1};
            const int xs[2] = {(f & FXLO) ? x + 1 : x - 1, (f & FXHI) ? x - 1 : x + 1};
            T s, d;
            vc_parts<T, DIM>([&](long long e, int k) -> T {
                const int nz = k == 0 ? zs[0] : (k == 5 ? zs[1] : z), ny = k == 1 ? ys[0] : (k == 4 ? ys[1] : y);
                const int nx = k == 2 ? xs[0] : (k == 3 ? xs[1] : x);
                if (bc_faces(g, nz, ny, nx) & ~mask) return (T)0;
                return zv[e] + beta * p[e];
            }, a, i, bc_neighbours(g, i, f), c, s, d);
            qv = d * pc - s;
            acc += bc_weight(__popc((unsigned)f)) * ((double)pc * (double)qv);   // f lies in the mask here
        }
        pn[i] = pc;
        q[i] = qv;
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---------------------------------------------------------------- sum w z.r, sum w z.q (k_cg_dots with the weights of the mask)
template <typename T>
__global__ __launch_bounds__(OP_THREADS) void k_vcn_cg_dots(Geom g, int mask, const T *__restrict__ z, const T *__restrict__ r,
                                                            const T *__restrict__ q, const CgScalars *__restrict__ sc,
                                                            double *__restrict__ partials)
{
    constexpr int V = Vec16<T>::n;
    typedef typename Vec16<T>::type vec;
    __shared__ double sh[OP_THREADS / 64];
    if (sc->bad != 0) return;
    const long long vpr = g.pitch / V, nitems = vpr * g.ny * g.nz;
    double zr = 0., zq = 0.;
    for (long long it = (long long)blockIdx.x * OP_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * OP_THREADS) {
        const long long row = it / vpr;
        const int x0 = (int)(it - row * vpr) * V, y = (int)(row % g.ny), zz = (int)(row / g.ny);
        if (x0 >= g.nx) continue;
        const long long i = lidx(g, zz, y, x0);
        const vec zv = *(const vec *)(z + i), rv = *(const vec *)(r + i), qv = *(const vec *)(q + i);
#pragma unroll
        for (int e = 0; e < V; e++)
            if (x0 + e < g.nx) {
                const double w = bc_weight(__popc((unsigned)(bc_faces(g, zz, y, x0 + e) & mask)));   // a power of two: exact
                zr += w * ((double)zv[e] * (double)rv[e]);
                zq += w * ((double)zv[e] * (double)qv[e]);
            }
    }
    const double s0 = block_sum(zr, sh);
    const double s1 = block_sum(zq, sh);
    if (threadIdx.x == 0) { partials[blockIdx.x] = s0; partials[gridDim.x + blockIdx.x] = s1; }
}

// ---------------------------------------------------------------- launchers
template <typename T>
VcCoef<T> vc_coef(const double coef[4], double sigma)
{
    return VcCoef<T>{(T)(-coef[0] / 2.0), (T)(-coef[1] / 2.0), (T)(-coef[2] / 2.0), (T)sigma};
}

}  // namespace

// mask == 0 launches the instantiations without MIR: the kernels of a handle that never set a mask
template <typename T>
int launch_vc_residual(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, const T *u, const T *a, const T *b, T *r,
                       double *partials, int cap, bool plain)
{
    const VcCoef<T> c = vc_coef<T>(coef, sigma);
    if (march_takes<T>(g, plain)) {
        const MarchGrid m = march_grid<T>(g);
        if (m.grid <= cap) {
            const dim3 gr(m.grid), bl(64 * MBW);
#define MG_VC(SAVE, MIR) hipLaunchKernelGGL((k_vc_march<T, OP_RES, SAVE, true, MIR>), gr, bl, 0, s, g, c, (T)1, u, a, b, r, partials, m.nbx, m.nby, m.nbz, m.zc, StepCoef<T>{}, mask)
            if (mask) { if (r) MG_VC(true, true); else MG_VC(false, true); }
            else { if (r) MG_VC(true, false); else MG_VC(false, false); }
#undef MG_VC
            return m.grid;
        }
    }
    if (mask) return plain_residual(s, g, vc_op<T, true>(c, a, mask), u, b, r, partials, cap);
    return plain_residual(s, g, vc_op<T, false>(c, a, 0), u, b, r, partials, cap);
}

template <typename T>
void launch_vc_jacobi(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, T omega, const T *u, const T *a, const T *b,
                      T *out, bool plain)
{
    const VcCoef<T> c = vc_coef<T>(coef, sigma);
    if (march_takes<T>(g, plain)) {
        const MarchGrid m = march_grid<T>(g);
        const dim3 gr(m.grid), bl(64 * MBW);
#define MG_VC(MIR) hipLaunchKernelGGL((k_vc_march<T, OP_JAC, false, true, MIR>), gr, bl, 0, s, g, c, omega, u, a, b, out, (double *)nullptr, m.nbx, m.nby, m.nbz, m.zc, StepCoef<T>{}, mask)
        if (mask) MG_VC(true); else MG_VC(false);
#undef MG_VC
        return;
    }
    if (mask) plain_jacobi(s, g, vc_op<T, true>(c, a, mask), omega, u, b, out);
    else plain_jacobi(s, g, vc_op<T, false>(c, a, 0), omega, u, b, out);
}

template <typename T>
void launch_vc_heat_rhs(hipStream_t s, const Geom &g, const double coef[4], int mask, double dt, double theta, const T *u, const T *a,
                        const T *f, T *out, bool plain)
{
    const VcCoef<T> c = vc_coef<T>(coef, 0.0);   // the unshifted operator: d starts from (T)0
    const StepCoef<T> st = step_coef<T>(dt, theta);
    if (march_takes<T>(g, plain)) {
        const MarchGrid m = march_grid<T>(g);
        const dim3 gr(m.grid), bl(64 * MBW);
#define MG_VC(SRC, MIR) hipLaunchKernelGGL((k_vc_march<T, OP_STEP, true, SRC, MIR>), gr, bl, 0, s, g, c, (T)1, u, a, f, out, (double *)nullptr, m.nbx, m.nby, m.nbz, m.zc, st, mask)
        if (mask) { if (f) MG_VC(true, true); else MG_VC(false, true); }
        else { if (f) MG_VC(true, false); else MG_VC(false, false); }
#undef MG_VC
        return;
    }
    if (mask) plain_step(s, g, vc_op<T, true>(c, a, mask), st, u, f, out);
    else plain_step(s, g, vc_op<T, false>(c, a, 0), st, u, f, out);
}

template <typename T>
void launch_vc_rb_colour(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, int colour, T *u, const T *a, const T *b)
{
    if (mask) plain_rb_colour(s, g, vc_op<T, true>(vc_coef<T>(coef, sigma), a, mask), colour, u, b);
    else plain_rb_colour(s, g, vc_op<T, false>(vc_coef<T>(coef, sigma), a, 0), colour, u, b);
}

template <typename T>
void launch_vc_coarse(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, T omega, int smoother, T *x, T *tmp,
                      const T *rhs, const T *a, int maxit, double tol, int fixed, CoarseOut *d_out)
{
    if (mask) coarse_solve(s, g, vc_op<T, true>(vc_coef<T>(coef, sigma), a, mask), omega, smoother, x, tmp, rhs, maxit, tol, fixed, d_out);
    else coarse_solve(s, g, vc_op<T, false>(vc_coef<T>(coef, sigma), a, 0), omega, smoother, x, tmp, rhs, maxit, tol, fixed, d_out);
}

template <typename T>
int launch_vc_cg_direction(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, const T *z, const T *p, const T *a,
                           T *pn, T *q, const CgScalars *sc, double *partials)
{
    const VcCoef<T> c = vc_coef<T>(coef, sigma);
    const int nb = plain_grid((long long)g.nx * g.ny * g.nz, OP_MAX_BLOCKS);
    const dim3 gr(nb), bl(OP_THREADS);
    if (mask) {
        if (g.dim == 3) hipLaunchKernelGGL((k_vcn_cg_direction<T, 3>), gr, bl, 0, s, g, c, mask, z, p, a, pn, q, sc, partials);
        else hipLaunchKernelGGL((k_vcn_cg_direction<T, 2>), gr, bl, 0, s, g, c, mask, z, p, a, pn, q, sc, partials);
    } else {
        if (g.dim == 3) hipLaunchKernelGGL((k_vc_cg_direction<T, 3>), gr, bl, 0, s, g, c, z, p, a, pn, q, sc, partials);
        else hipLaunchKernelGGL((k_vc_cg_direction<T, 2>), gr, bl, 0, s, g, c, z, p, a, pn, q, sc, partials);
    }
    return nb;
}

template <typename T>
int launch_vc_cg_wdots(hipStream_t s, const Geom &g, int mask, const T *z, const T *r, const T *q, const CgScalars *sc, double *partials)
{
    const int nb = plain_grid((long long)(g.pitch / Vec16<T>::n) * g.ny * g.nz, OP_MAX_BLOCKS);
    hipLaunchKernelGGL((k_vcn_cg_dots<T>), dim3(nb), dim3(OP_THREADS), 0, s, g, mask, z, r, q, sc, partials);
    return nb;
}

#define MG_VC_INST(T)                                                                                                                  \
    template int launch_vc_residual<T>(hipStream_t, const Geom &, const double[4], double, int, const T *, const T *, const T *, T *, \
                                       double *, int, bool);                                                                         \
    template void launch_vc_jacobi<T>(hipStream_t, const Geom &, const double[4], double, int, T, const T *, const T *, const T *,   \
                                      T *, bool);                                                                                    \
    template void launch_vc_heat_rhs<T>(hipStream_t, const Geom &, const double[4], int, double, double, const T *, const T *,        \
                                        const T *, T *, bool);                                                                       \
    template void launch_vc_rb_colour<T>(hipStream_t, const Geom &, const double[4], double, int, int, T *, const T *, const T *);    \
    template void launch_vc_coarse<T>(hipStream_t, const Geom &, const double[4], double, int, T, int, T *, T *, const T *, const T *, \
                                      int, double, int, CoarseOut *);                                                                \
    template int launch_vc_cg_direction<T>(hipStream_t, const Geom &, const double[4], double, int, const T *, const T *, const T *,  \
                                           T *, T *, const CgScalars *, double *);                                                   \
    template int launch_vc_cg_wdots<T>(hipStream_t, const Geom &, int, const T *, const T *, const T *, const CgScalars *, double *);
MG_VC_INST(double)
MG_VC_INST(float)
#undef MG_VC_INST

}  // namespace mg
