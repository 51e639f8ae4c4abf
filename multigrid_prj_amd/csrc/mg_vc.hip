// mg_vc.hip -- kernels of the variable-coefficient operator -div(a grad u) + sigma u (mg_vc_*, include/mg_hip.h; drivers:
// Solver::vc_* in mg_drivers.cpp). The coefficient a is a nodal, level-shaped array of every level (Level::vc_a); the
// transfers do not depend on the operator, so only the smoother, the residual, the coarsest-grid solve and the Krylov
// direction kernel live here.
//
//   VcOp<T, MIR, KIND>             the point operator (VcCoef and a): res<DIM> and solve<DIM> of the contract below. The plain
//                                  form (residual / Jacobi sweep / one red-black colour pass, every shape) and the
//                                  coarsest-grid solve are mg_opfamily.h's k_op_plain<VcOp<T>, DIM, OP, SAVE> and
//                                  k_op_coarse<VcOp<T>, DIM>
//   k_vc_march<T, OP, SAVE, SRC, MIR, KIND>  the residual, the Jacobi sweep and the right-hand side of a theta step (OP_STEP, with or
//                                  without a source: mg_vc_heat_rhs) on 3-D levels with rows long enough to fill a wave
//                                  (vc_march_ok, mg_geom.h)
//   k_vc_fas_coarse_rhs<T, DIM, WZ, KIND, MIR>  the FAS transition on this operator (see REACTION)
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
// REACTION (MG_FAS_ON_COEFFICIENT): mg_fas_* on this operator, N(u) = L u + G g(u). VcOp and k_vc_march carry
// the reaction as the template parameter KIND (FAS_CUBIC, FAS_EXP; fas_react and fas_newton_point of mg_opfamily.h): residual
// r = b - ((d * u_i - s) + G * g), point solve num = (b + s) - G * (g - gp * u_i), den = d + G * gp, ps = num / den, step n0 =
// (d0 * u_i - s) + G * g. With KIND = FAS_LINEAR (the default: mg_vc_*) VcReact is empty and every such expression folds to the
// one of the contract below: the same kernels, arguments and registers as without the parameter. tests/fasvc_ref.py restates it.
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

// the reaction of a VcOp / of the tile: G = (T)gamma of MG_FAS_ON_COEFFICIENT; no member with FAS_LINEAR, so the kernels of
// mg_vc_* take the arguments they always took
template <typename T, int KIND>
struct VcReact {
    static constexpr int kind = KIND;
    T G;
};
template <typename T>
struct VcReact<T, FAS_LINEAR> {
    static constexpr int kind = FAS_LINEAR;
};

// the operator's value (d * u_i - s) + G * g(u_i) from the linear part lin = d * u_i - s; FAS_LINEAR: lin itself
template <typename T, int KIND>
__device__ __forceinline__ T vc_value(const VcReact<T, KIND> &rx, T lin, T ui)
{
    if constexpr (KIND == FAS_LINEAR) {
        return lin;
    } else {
        T gv, gp;
        fas_react<T, KIND>(ui, gv, gp);
        return lin + rx.G * gv;
    }
}

// the point solve from num = b + s and d; FAS_LINEAR: their IEEE quotient, else one Newton step (fas_newton_point)
template <typename T, int KIND>
__device__ __forceinline__ T vc_point(const VcReact<T, KIND> &rx, T num, T d, T ui)
{
    if constexpr (KIND == FAS_LINEAR) return num / d;
    else return fas_newton_point<T, KIND>(rx.G, num, d, ui);
}

// the point operator of the plain form and of the coarsest-grid solve (mg_opfamily.h); KIND: the reaction of
// MG_FAS_ON_COEFFICIENT, FAS_LINEAR (mg_vc_*) folds it away
template <typename T, bool MIR = false, int KIND = FAS_LINEAR>
struct VcOp : VcMask<MIR>, VcReact<T, KIND> {
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
        return b[i] - vc_value<T, KIND>(*this, d * u[i] - s, u[i]);
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
        if constexpr (KIND == FAS_LINEAR) {
            const T ps = (bi + s) / d;
            if (damped) {
                const T ui = u[i];
                return ui + omega * (ps - ui);
            }
            return ps;
        } else {
            const T ui = u[i];
            const T ps = vc_point<T, KIND>(*this, bi + s, d, ui);
            return damped ? ui + omega * (ps - ui) : ps;
        }
    }

    // the operator's value (d * u_i - s) + G * g at an unknown (c.sigma = 0: the unshifted operator of the time steppers)
    template <int DIM>
    __device__ __forceinline__ bool n0(const Geom &g, const T *u, int z, int y, int x, bool stencil, T &v) const
    {
        const long long i = lidx(g, z, y, x);
        BcNb n;
        if (fixed(g, z, y, x, i, n)) return true;
        if (stencil) {
            T s, d;
            vc_parts<T, DIM>([&](long long q, int) { return u[q]; }, a, i, n, c, s, d);
            v = vc_value<T, KIND>(*this, d * u[i] - s, u[i]);
        }
        return false;
    }
};

template <typename T, bool MIR, int KIND = FAS_LINEAR>
__host__ __device__ VcOp<T, MIR, KIND> vc_op(const VcCoef<T> &c, const T *a, int mask, const VcReact<T, KIND> &rx = VcReact<T, KIND>{})
{
    VcOp<T, MIR, KIND> op;
    op.c = c;
    op.a = a;
    if constexpr (MIR) op.mask = mask;
    if constexpr (KIND != FAS_LINEAR) op.G = rx.G;
    return op;
}

// ---------------------------------------------------------------- the marching tile (3-D)
// OP_STEP: b is the source of the step (not loaded without SRC), st its scalars, c.sigma = 0; out = u on Dirichlet nodes.
// MIR: the faces of `mask` are Neumann (not looked at otherwise). KIND: the reaction rx.G * g(u) of MG_FAS_ON_COEFFICIENT, from the
// centre value the lane holds (no load and no branch is added); FAS_LINEAR: rx is empty and the tile is the code it was
template <typename T, int OP, bool SAVE, bool SRC = true, bool MIR = false, int KIND = FAS_LINEAR>
__global__ __launch_bounds__(64 * MBW) void k_vc_march(Geom g, VcCoef<T> c, T omega, const T *__restrict__ u, const T *__restrict__ a,
                                                       const T *__restrict__ b, T *__restrict__ out, double *__restrict__ partials,
                                                       int nbx, int nby, int nbz, int zc, StepCoef<T> st, int mask, VcReact<T, KIND> rx)
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
                    v = bnd ? bi - ui : bi - vc_value<T, KIND>(rx, d * ui - s, ui);
                } else if (OP == OP_STEP) {
                    v = bnd ? ui : step_value<T, SRC>(st, ui, bi, vc_value<T, KIND>(rx, d * ui - s, ui));
                } else {
                    const T ps = vc_point<T, KIND>(rx, bi + s, d, ui);
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
                            const VcOp<T, true, KIND> op = vc_op<T, true, KIND>(c, a, mask, rx);
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

// ---------------------------------------------------------------- the FAS transition l -> l+1 on this operator
// k_fas_coarse_rhs (mg_fas.hip) with the coarse level's coefficient array: uf = U(l), rf = TMP(l) (the residual of level l), ac =
// vc_a(l+1), cc = the VcCoef of level l+1; per coarse node uc = uf at the even fine node -> uco and eco; rhsc = rc + ((d_c*uc -
// s_c) + G*g(uc)) with vc_parts over ac at the coarse node and its coarse neighbours and the u neighbours read from uf at
// distance 2 (z: 1 on a semi transition); coarse Dirichlet nodes: rhsc = uc. MIR: the Dirichlet nodes are those on a face
// outside the mask, rc is bc_restrict_point and a neighbour that leaves the grid, for a or for u, is its mirror image.
template <typename T, int DIM, bool WZ, int KIND, bool MIR>
__global__ __launch_bounds__(OP_THREADS) void k_vc_fas_coarse_rhs(Geom gf, Geom gc, VcCoef<T> cc, T G, int inject, const T *__restrict__ uf,
                                                                   const T *__restrict__ rf, const T *__restrict__ ac, T *__restrict__ uco,
                                                                   T *__restrict__ eco, T *__restrict__ rhsc, int mask)
{
    const long long nitems = (long long)gc.nx * gc.ny * gc.nz;
    for (long long it = (long long)blockIdx.x * OP_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * OP_THREADS) {
        const long long row = it / gc.nx;
        const int x = (int)(it - row * gc.nx), y = (int)(row % gc.ny), z = (int)(row / gc.ny);
        const int fz = (DIM == 3) ? (WZ ? 2 * (gc.gz0 + z) - gf.gz0 : z) : 0;
        const long long fi = lidx(gf, fz, 2 * y, 2 * x), ci = lidx(gc, z, y, x);
        const T uc = uf[fi];
        T rhs;
        const int cf = MIR ? bc_faces(gc, z, y, x) : 0;
        if (MIR ? (cf & ~mask) != 0 : on_boundary(gc, z, y, x)) {
            rhs = uc;
        } else {
            const T rc = inject ? rf[fi]
                                : (MIR ? bc_restrict_point<T, DIM, WZ>(gf, gc, rf, z, y, x) : restrict_fw_point<T, DIM, WZ>(gf, gc, rf, z, y, x));
            const long long sy = 2 * (long long)gf.pitch, sz = WZ ? 2 * gf.plane : gf.plane;
            // the coarse neighbours in uf, in vc_parts' order; on a Neumann face the one that leaves the grid is its mirror image
            const long long off[6] = {(cf & FZLO) ? sz : -sz, (cf & FYLO) ? sy : -sy, (cf & FXLO) ? 2 : -2,
                                      (cf & FXHI) ? -2 : 2,   (cf & FYHI) ? -sy : sy, (cf & FZHI) ? -sz : sz};
            T sc, dc;
            vc_parts<T, DIM>([&](long long, int k) { return uf[fi + off[k]]; }, ac, ci, bc_neighbours(gc, ci, cf), cc, sc, dc);
            rhs = rc + vc_value<T, KIND>(VcReact<T, KIND>{G}, dc * uc - sc, uc);
        }
        uco[ci] = uc;
        eco[ci] = uc;
        rhsc[ci] = rhs;
    }
}

// ---------------------------------------------------------------- launchers
template <typename T>
VcCoef<T> vc_coef(const double coef[4], double sigma)
{
    return VcCoef<T>{(T)(-coef[0] / 2.0), (T)(-coef[1] / 2.0), (T)(-coef[2] / 2.0), (T)sigma};
}

// launch(rx) with rx = the VcReact of `react`: the kernels and the point operator take KIND from its type
template <typename T, typename Launch>
auto with_vc_react(int react, T G, Launch &&launch)
{
    if (react == FAS_CUBIC) return launch(VcReact<T, FAS_CUBIC>{G});
    if (react == FAS_EXP) return launch(VcReact<T, FAS_EXP>{G});
    return launch(VcReact<T, FAS_LINEAR>{});
}

// launch(op) with the point operator of the mask and of rx
template <typename T, int KIND, typename Launch>
auto with_vc_op(const VcCoef<T> &c, const T *a, int mask, const VcReact<T, KIND> &rx, Launch &&launch)
{
    if (mask) return launch(vc_op<T, true, KIND>(c, a, mask, rx));
    return launch(vc_op<T, false, KIND>(c, a, 0, rx));
}

}  // namespace

// mask == 0 launches the instantiations without MIR, react == FAS_LINEAR those without a reaction: the kernels of mg_vc_*.
// Every (reaction, element type, mirrored) combination runs the tile where march_takes: each has no scratch and beat the plain
// form in profiles/fasvc_times.log
template <typename T>
int launch_vc_residual(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, int react, T G, const T *u, const T *a,
                       const T *b, T *r, double *partials, int cap, bool plain)
{
    const VcCoef<T> c = vc_coef<T>(coef, sigma);
    return with_vc_react<T>(react, G, [&](auto rx) {
        constexpr int KIND = decltype(rx)::kind;
        if (march_takes<T>(g, plain)) {
            const MarchGrid m = march_grid<T>(g);
            if (m.grid <= cap) {
                const dim3 gr(m.grid), bl(64 * MBW);
#define MG_VC(SAVE, MIR) hipLaunchKernelGGL((k_vc_march<T, OP_RES, SAVE, true, MIR, KIND>), gr, bl, 0, s, g, c, (T)1, u, a, b, r, partials, m.nbx, m.nby, m.nbz, m.zc, StepCoef<T>{}, mask, rx)
                if (mask) { if (r) MG_VC(true, true); else MG_VC(false, true); }
                else { if (r) MG_VC(true, false); else MG_VC(false, false); }
#undef MG_VC
                return m.grid;
            }
        }
        return with_vc_op<T, KIND>(c, a, mask, rx, [&](auto op) { return plain_residual(s, g, op, u, b, r, partials, cap); });
    });
}

template <typename T>
void launch_vc_jacobi(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, int react, T G, T omega, const T *u,
                      const T *a, const T *b, T *out, bool plain)
{
    const VcCoef<T> c = vc_coef<T>(coef, sigma);
    with_vc_react<T>(react, G, [&](auto rx) {
        constexpr int KIND = decltype(rx)::kind;
        if (march_takes<T>(g, plain)) {
            const MarchGrid m = march_grid<T>(g);
            const dim3 gr(m.grid), bl(64 * MBW);
#define MG_VC(MIR) hipLaunchKernelGGL((k_vc_march<T, OP_JAC, false, true, MIR, KIND>), gr, bl, 0, s, g, c, omega, u, a, b, out, (double *)nullptr, m.nbx, m.nby, m.nbz, m.zc, StepCoef<T>{}, mask, rx)
            if (mask) MG_VC(true); else MG_VC(false);
#undef MG_VC
            return;
        }
        with_vc_op<T, KIND>(c, a, mask, rx, [&](auto op) { plain_jacobi(s, g, op, omega, u, b, out); });
    });
}

template <typename T>
void launch_vc_heat_rhs(hipStream_t s, const Geom &g, const double coef[4], int mask, int react, T G, double dt, double theta, const T *u,
                        const T *a, const T *f, T *out, bool plain)
{
    const VcCoef<T> c = vc_coef<T>(coef, 0.0);   // the unshifted operator: d starts from (T)0
    const StepCoef<T> st = step_coef<T>(dt, theta);
    with_vc_react<T>(react, G, [&](auto rx) {
        constexpr int KIND = decltype(rx)::kind;
        if (march_takes<T>(g, plain)) {
            const MarchGrid m = march_grid<T>(g);
            const dim3 gr(m.grid), bl(64 * MBW);
#define MG_VC(SRC, MIR) hipLaunchKernelGGL((k_vc_march<T, OP_STEP, true, SRC, MIR, KIND>), gr, bl, 0, s, g, c, (T)1, u, a, f, out, (double *)nullptr, m.nbx, m.nby, m.nbz, m.zc, st, mask, rx)
            if (mask) { if (f) MG_VC(true, true); else MG_VC(false, true); }
            else { if (f) MG_VC(true, false); else MG_VC(false, false); }
#undef MG_VC
            return;
        }
        with_vc_op<T, KIND>(c, a, mask, rx, [&](auto op) { plain_step(s, g, op, st, u, f, out); });
    });
}

template <typename T>
void launch_vc_rb_colour(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, int react, T G, int colour, T *u,
                         const T *a, const T *b)
{
    with_vc_react<T>(react, G, [&](auto rx) {
        with_vc_op<T, decltype(rx)::kind>(vc_coef<T>(coef, sigma), a, mask, rx, [&](auto op) { plain_rb_colour(s, g, op, colour, u, b); });
    });
}

template <typename T>
void launch_vc_coarse(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, int react, T G, T omega, int smoother,
                      T *x, T *tmp, const T *rhs, const T *a, int maxit, double tol, int fixed, CoarseOut *d_out)
{
    with_vc_react<T>(react, G, [&](auto rx) {
        with_vc_op<T, decltype(rx)::kind>(vc_coef<T>(coef, sigma), a, mask, rx,
                                          [&](auto op) { coarse_solve(s, g, op, omega, smoother, x, tmp, rhs, maxit, tol, fixed, d_out); });
    });
}

template <typename T>
void launch_vc_fas_coarse_rhs(hipStream_t s, const Geom &gf, const Geom &gc, const double coefc[4], double sigma, int mask, int react, T G,
                              bool inject, const T *uf, const T *rf, const T *ac, T *uc, T *ec, T *rhsc)
{
    const VcCoef<T> cc = vc_coef<T>(coefc, sigma);
    const dim3 gr(plain_grid((long long)gc.nx * gc.ny * gc.nz, OP_MAX_BLOCKS)), bl(OP_THREADS);
    const int inj = inject ? 1 : 0;
#define MG_VC(DIM, WZ, KIND, MIR) hipLaunchKernelGGL((k_vc_fas_coarse_rhs<T, DIM, WZ, KIND, MIR>), gr, bl, 0, s, gf, gc, cc, G, inj, uf, rf, ac, uc, ec, rhsc, mask)
#define MG_VC_M(DIM, WZ, KIND) if (mask) MG_VC(DIM, WZ, KIND, true); else MG_VC(DIM, WZ, KIND, false);
#define MG_VC_K(DIM, WZ) if (react == FAS_CUBIC) { MG_VC_M(DIM, WZ, FAS_CUBIC) } else { MG_VC_M(DIM, WZ, FAS_EXP) }
    if (gc.dim == 3 && is_semi_transition(gf, gc)) { MG_VC_K(3, false) }
    else if (gc.dim == 3) { MG_VC_K(3, true) }
    else { MG_VC_K(2, false) }
#undef MG_VC_K
#undef MG_VC_M
#undef MG_VC
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
    template int launch_vc_residual<T>(hipStream_t, const Geom &, const double[4], double, int, int, T, const T *, const T *, const T *, \
                                       T *, double *, int, bool);                                                                    \
    template void launch_vc_jacobi<T>(hipStream_t, const Geom &, const double[4], double, int, int, T, T, const T *, const T *,       \
                                      const T *, T *, bool);                                                                         \
    template void launch_vc_heat_rhs<T>(hipStream_t, const Geom &, const double[4], int, int, T, double, double, const T *, const T *, \
                                        const T *, T *, bool);                                                                       \
    template void launch_vc_rb_colour<T>(hipStream_t, const Geom &, const double[4], double, int, int, T, int, T *, const T *,        \
                                         const T *);                                                                                 \
    template void launch_vc_coarse<T>(hipStream_t, const Geom &, const double[4], double, int, int, T, T, int, T *, T *, const T *,   \
                                      const T *, int, double, int, CoarseOut *);                                                     \
    template void launch_vc_fas_coarse_rhs<T>(hipStream_t, const Geom &, const Geom &, const double[4], double, int, int, T, bool,    \
                                              const T *, const T *, const T *, T *, T *, T *);                                       \
    template int launch_vc_cg_direction<T>(hipStream_t, const Geom &, const double[4], double, int, const T *, const T *, const T *,  \
                                           T *, T *, const CgScalars *, double *);                                                   \
    template int launch_vc_cg_wdots<T>(hipStream_t, const Geom &, int, const T *, const T *, const T *, const CgScalars *, double *);
MG_VC_INST(double)
MG_VC_INST(float)
#undef MG_VC_INST

}  // namespace mg
