// mg_bc.hip -- kernels of the constant operator with NEUMANN faces (mg_bc_*, include/mg_hip.h; drivers: Solver::bc_* in
// mg_drivers.cpp). A face mask (enum mg_face) names the faces of the box that are zero-flux walls; a node on at least one
// face that is NOT in the mask is a Dirichlet node (identity row), every other node is an unknown, the nodes that lie
// only on Neumann faces included. At such a node the neighbour outside the box is the MIRROR IMAGE inside it, axis by
// axis; no ghost value is stored or read. The prolongation does not depend on the faces; the restriction does (injecting
// at coarse nodes of a Neumann face makes the cycle diverge), so it lives here too.
//
//   BcOp<T>                        the point operator (Coef and the mask): res<DIM> and solve<DIM> of the contract below. The
//                                  plain form (residual / Jacobi sweep / one red-black colour pass, every shape) and the
//                                  coarsest-grid solve are mg_opfamily.h's k_op_plain<BcOp<T>, DIM, OP, SAVE> and
//                                  k_op_coarse<BcOp<T>, DIM>
//   k_bc_march<T, OP, SAVE, SRC, NB>   the residual, the Jacobi sweep and the right-hand side of a theta step (OP_STEP, with or
//                                  without a source, with the stencil or -- theta == 1 -- without a neighbour loaded:
//                                  mg_bc_heat_rhs) on 3-D levels with rows long enough to fill a wave (bc_march_ok, mg_geom.h)
//   k_bc_restrict<T, DIM, WZ>      full weighting with mirrored fine neighbours, coarse Dirichlet nodes injected
//   k_bc_wsum<T> / k_bc_shift<T>   sum of w v (w = 1/2 per Neumann face the node lies on) / v -= c on every node
//   k_bc_dirichlet_copy<T>         x = rhs on the Dirichlet nodes
//
// The marching tile is k_vc_march's (mg_vc.hip) with ONE marched field: a lane owns one aligned 16-byte vector of x, a wave
// covers 64 vectors of MRY = 2 rows, MBW = 4 waves are stacked in y and the workgroup marches zc planes with the planes
// z-1, z, z+1 of u in registers. x-neighbours are the neighbouring lanes' values (whole-wave DPP shifts; the two edge
// lanes load theirs), y-neighbours the wave's other row or two halo rows that hit L1 / L2. The mirror is a select on values
// the lane holds anyway: the element at x = 0 takes its right neighbour for the left one, row 0 takes row 1 for the halo
// row, plane 0 takes uzp for uzm (and likewise at the high ends) -- no load and no branch is added in the interior. Only
// the odd last column of a 2^k + 1 row, which one lane of the row's last wave writes as part of a full 128-byte line, is
// computed from global memory by the plain form's point function, because with an x-hi Neumann face it is an unknown.
//
// Arithmetic contract (compiled with -ffp-contract=off; tests/bc_ref.py restates it in numpy), all in T, every operation
// rounded separately, c = the level's Coef (mg_level_coefficients: shift and aniso included), u(q) the value of neighbour
// q or of its mirror image:
//   residual     sum = 0; sum += cz u(z-); sum += cy u(y-); sum += cx u(x-); sum += cd u_i; sum += cx u(x+); sum += cy u(y+);
//                sum += cz u(z+) (full_sum's order, no z in 2-D); r = b - sum; Dirichlet nodes: r = b - u;
//                the sum of r^2 over ALL nodes in double, fixed order, no atomics
//   point solve  the same sum without the diagonal term (offdiag_sum's order), ps = (b - sum) / cd (div_cd: the IEEE quotient)
//   Jacobi       u' = ps (omega == 1) or u_i + omega * (ps - u_i); Dirichlet nodes: u' = b
//   red-black    in place, colour (i + j + gz) & 1, colour 0 first; Dirichlet nodes take b with their colour
//   step         n0 = the residual's sum with the UNSHIFTED diagonal cd0; rhs = ((f + rdt*u_i) - omt*n0) * rth, without a source
//                (rdt*u_i - omt*n0) * rth; Dirichlet nodes: rhs = u_i (step_value, mg_opfamily.h; tests/step_ref.py)
//   restriction  restrict_fw_point's expression (x, then y inside the z planes, weights q, hlf, q) with fine indices outside
//                the grid mirrored; coarse Dirichlet nodes injected
// With mask 0 every one of these is the existing kernel's expression: the results are the same bits.
#include "mg_opfamily.h"

namespace mg {
namespace {

// the face bits, bc_faces and bc_neighbours are mg_opfamily.h's: mg_vc.hip mirrors with them too

template <typename T, int DIM>
__device__ __forceinline__ T bc_point_res(const Geom &g, const Coef<T> &c, int mask, const T *u, const T *b, int z, int y, int x)
{
    const long long i = lidx(g, z, y, x);
    const int f = bc_faces(g, z, y, x);
    T sum;
    if (f & ~mask) {
        sum = (T)1 * u[i];
    } else {
        const BcNb n = bc_neighbours(g, i, f);
        sum = 0;
        if (DIM == 3) sum += c.cz * u[n.zm];
        sum += c.cy * u[n.ym];
        sum += c.cx * u[n.xm];
        sum += c.cd * u[i];
        sum += c.cx * u[n.xp];
        sum += c.cy * u[n.yp];
        if (DIM == 3) sum += c.cz * u[n.zp];
    }
    return b[i] - sum;
}

template <typename T, int DIM>
__device__ __forceinline__ T bc_point_solve(const Geom &g, const Coef<T> &c, int mask, T omega, bool damped, const T *u, const T *b,
                                            int z, int y, int x)
{
    const long long i = lidx(g, z, y, x);
    const T bi = b[i];
    const int f = bc_faces(g, z, y, x);
    if (f & ~mask) return bi;
    const BcNb n = bc_neighbours(g, i, f);
    T sum = 0;
    if (DIM == 3) sum += c.cz * u[n.zm];
    sum += c.cy * u[n.ym];
    sum += c.cx * u[n.xm];
    sum += c.cx * u[n.xp];
    sum += c.cy * u[n.yp];
    if (DIM == 3) sum += c.cz * u[n.zp];
    const T ps = div_cd<T>(bi - sum, c);
    if (damped) {
        const T ui = u[i];
        return ui + omega * (ps - ui);
    }
    return ps;
}

// the operator's value at node (z, y, x) into v -- bc_point_res's sum, c.cd = cd0: the unshifted operator of the time
// steppers; stencil == false: v is left alone and no neighbour is loaded -> true at a Dirichlet node
template <typename T, int DIM>
__device__ __forceinline__ bool bc_point_n0(const Geom &g, const Coef<T> &c, int mask, const T *u, int z, int y, int x, bool stencil, T &v)
{
    const int f = bc_faces(g, z, y, x);
    if (f & ~mask) return true;
    if (stencil) {
        const long long i = lidx(g, z, y, x);
        const BcNb n = bc_neighbours(g, i, f);
        T sum = 0;
        if (DIM == 3) sum += c.cz * u[n.zm];
        sum += c.cy * u[n.ym];
        sum += c.cx * u[n.xm];
        sum += c.cd * u[i];
        sum += c.cx * u[n.xp];
        sum += c.cy * u[n.yp];
        if (DIM == 3) sum += c.cz * u[n.zp];
        v = sum;
    }
    return false;
}

// the point operator of the plain form and of the coarsest-grid solve (mg_opfamily.h). The point functions stay free
// functions because the marching tile calls them too, for the odd last column.
template <typename T>
struct BcOp {
    typedef T type;
    Coef<T> c;
    int mask;

    template <int DIM>
    __device__ __forceinline__ T res(const Geom &g, const T *u, const T *b, int z, int y, int x) const
    {
        return bc_point_res<T, DIM>(g, c, mask, u, b, z, y, x);
    }

    template <int DIM>
    __device__ __forceinline__ T solve(const Geom &g, T omega, bool damped, const T *u, const T *b, int z, int y, int x) const
    {
        return bc_point_solve<T, DIM>(g, c, mask, omega, damped, u, b, z, y, x);
    }

    template <int DIM>
    __device__ __forceinline__ bool n0(const Geom &g, const T *u, int z, int y, int x, bool stencil, T &v) const
    {
        return bc_point_n0<T, DIM>(g, c, mask, u, z, y, x, stencil, v);
    }
};

// ---------------------------------------------------------------- the marching tile (3-D)
// OP_STEP: b is the source of the step (not loaded without SRC), st its scalars, c.cd = cd0; out = u on Dirichlet nodes.
// NB == false (theta == 1, where the operator's value is multiplied by zero): u is streamed through, no neighbour is loaded
template <typename T, int OP, bool SAVE, bool SRC = true, bool NB = true>
__global__ __launch_bounds__(64 * MBW) void k_bc_march(Geom g, Coef<T> c, int mask, T omega, const T *__restrict__ u,
                                                       const T *__restrict__ b, T *__restrict__ out, double *__restrict__ partials,
                                                       int nbx, int nby, int nbz, int zc, StepCoef<T> st)
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
    const int dir = ~mask;   // the Dirichlet faces

    long long rowoff[MRY];
    bool yin[MRY];
    int yface[MRY];
#pragma unroll
    for (int r = 0; r < MRY; r++) {
        const int y = yb + r;
        yin[r] = y < g.ny;
        const int yc = min(y, g.ny - 1);
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
        uzm[r] = NB ? *(const vec *)(pu - g.plane + rowoff[r]) : (vec)(0);
        ucc[r] = NB ? *(const vec *)(pu + rowoff[r]) : (vec)(0);
    }
    double acc = 0.;
    for (int z = z0; z < zend; z++, pu += g.plane) {
        const long long zo = (long long)z * g.plane;
        vec bv[MRY];
#pragma unroll
        for (int r = 0; r < MRY; r++) {
            if (NB) uzp[r] = *(const vec *)(pu + g.plane + rowoff[r]);
            else ucc[r] = uzp[r] = __builtin_nontemporal_load((const vec *)(pu + rowoff[r]));
            bv[r] = LOADB ? __builtin_nontemporal_load((const vec *)(b + zo + rowoff[r])) : (vec)(0);
        }
        const vec ulo = NB ? *(const vec *)(pu + off_lo) : (vec)(0), uhi = NB ? *(const vec *)(pu + off_hi) : (vec)(0);
        const int gz = g.gz0 + z;
        const int zface = (gz == 0 ? FZLO : 0) | (gz == g.gnz - 1 ? FZHI : 0);
#pragma unroll
        for (int r = 0; r < MRY; r++) {
            T uel = 0, uer = 0;
            if (NB && edge_l) uel = pu[rowoff[r] - 1];
            if (NB && edge_r) uer = pu[rowoff[r] + V];
            const T uxm = lane_from_prev(ucc[r][V - 1], uel), uxp = lane_from_next(ucc[r][0], uer);
            const vec uym0 = (r > 0) ? ucc[r > 0 ? r - 1 : 0] : ulo, uyp0 = (r < MRY - 1) ? ucc[r < MRY - 1 ? r + 1 : 0] : uhi;
            // the mirror in y and z: values the lane holds anyway
            const vec uym = (yface[r] & FYLO) ? uyp0 : uym0, uyp = (yface[r] & FYHI) ? uym0 : uyp0;
            const vec uzl = (zface & FZLO) ? uzp[r] : uzm[r], uzh = (zface & FZHI) ? uzm[r] : uzp[r];
            const int rface = zface | yface[r];
            T num[V], ps[V];
            bool dn[V];
            vec res;
#pragma unroll
            for (int e = 0; e < V; e++) {
                const T ui = ucc[r][e], bi = bv[r][e];
                const T ul0 = (e == 0) ? uxm : ucc[r][e > 0 ? e - 1 : 0];
                const T ur0 = (e == V - 1) ? uxp : ucc[r][e < V - 1 ? e + 1 : 0];
                const int xface = (x0 + e == 0 ? FXLO : 0) | (x0 + e == g.nx - 1 ? FXHI : 0);
                const T ul = (xface & FXLO) ? ur0 : ul0, ur = (xface & FXHI) ? ul0 : ur0;
                dn[e] = ((rface | xface) & dir) != 0;
                T sum = 0;
                sum += c.cz * uzl[e];
                sum += c.cy * uym[e];
                sum += c.cx * ul;
                if (OP == OP_RES || OP == OP_STEP) sum += c.cd * ui;
                sum += c.cx * ur;
                sum += c.cy * uyp[e];
                sum += c.cz * uzh[e];
                if (OP == OP_RES) res[e] = dn[e] ? bi - ui : bi - sum;
                else if (OP == OP_STEP) res[e] = dn[e] ? ui : step_value<T, SRC>(st, ui, bi, NB ? sum : (T)0);
                else num[e] = bi - sum;
            }
            if (OP == OP_JAC) {
                div_cd_n_wave<T, V>(num, ps, c);
#pragma unroll
                for (int e = 0; e < V; e++) {
                    const T ui = ucc[r][e];
                    res[e] = dn[e] ? bv[r][e] : (damped ? ui + omega * (ps[e] - ui) : ps[e]);
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
                    // column nx-1 as one full 128-byte line: value + zero padding. With an x-hi Neumann face the node is an
                    // unknown: the plain form's point function computes it (one lane per row; u is never the output array)
                    const int j = lane - 56;
                    constexpr int LINE = 128 / (int)sizeof(T);
                    const int xs = g.nx - 1 + V * j;
                    const int line_end = ((g.nx - 1) / LINE + 1) * LINE;
                    const long long ro = zo + (rowoff[r] - x0c);
                    if (xs < line_end) {
                        vec tv = (vec)(0);
                        if (j == 0) {
                            if (OP == OP_RES) {
                                const T rt = bc_point_res<T, 3>(g, c, mask, u, b, z, yb + r, g.nx - 1);
                                acc += (double)rt * (double)rt;
                                tv[0] = rt;
                            } else if (OP == OP_STEP) {
                                const long long it = ro + g.nx - 1;
                                const T ut = u[it];
                                T n0 = (T)0;
                                const bool fixed = bc_point_n0<T, 3>(g, c, mask, u, z, yb + r, g.nx - 1, NB, n0);
                                tv[0] = fixed ? ut : step_value<T, SRC>(st, ut, SRC ? b[it] : (T)0, n0);
                            } else {
                                tv[0] = bc_point_solve<T, 3>(g, c, mask, omega, damped, u, b, z, yb + r, g.nx - 1);
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

// ---------------------------------------------------------------- restriction with mirrored fine neighbours
// WZ: weights along z too (3-D standard coarsening); otherwise 9-point weights per plane (2-D, semi transitions)
template <typename T, int DIM, bool WZ>
__global__ __launch_bounds__(OP_THREADS) void k_bc_restrict(Geom gf, Geom gc, int mask, const T *__restrict__ fine, T *__restrict__ coarse)
{
    const long long nitems = (long long)gc.nx * gc.ny * gc.nz;
    for (long long it = (long long)blockIdx.x * OP_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * OP_THREADS) {
        const long long row = it / gc.nx;
        const int x = (int)(it - row * gc.nx), y = (int)(row % gc.ny), z = (int)(row / gc.ny);
        T out;
        if (bc_faces(gc, z, y, x) & ~mask) {
            const int fz = (DIM == 3) ? (WZ ? 2 * (gc.gz0 + z) - gf.gz0 : z) : 0;
            out = fine[lidx(gf, fz, 2 * y, 2 * x)];
        } else {
            out = bc_restrict_point<T, DIM, WZ>(gf, gc, fine, z, y, x);   // mg_opfamily.h: the FAS transition calls it too
        }
        coarse[lidx(gc, z, y, x)] = out;
    }
}

// ---------------------------------------------------------------- the weighted sum, the shift, the Dirichlet copy
template <typename T>
__global__ __launch_bounds__(OP_THREADS) void k_bc_wsum(Geom g, int mask, const T *__restrict__ v, double *__restrict__ partials)
{
    __shared__ double sh[OP_THREADS / 64];
    const long long nitems = (long long)g.nx * g.ny * g.nz;
    double acc = 0.;
    for (long long it = (long long)blockIdx.x * OP_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * OP_THREADS) {
        const long long row = it / g.nx;
        const int x = (int)(it - row * g.nx), y = (int)(row % g.ny), z = (int)(row / g.ny);
        const int nf = __popc((unsigned)(bc_faces(g, z, y, x) & mask));   // 0 .. 3: at most one face per axis
        const double w = nf == 0 ? 1.0 : (nf == 1 ? 0.5 : (nf == 2 ? 0.25 : 0.125));
        acc += w * (double)v[lidx(g, z, y, x)];
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

template <typename T>
__global__ __launch_bounds__(OP_THREADS) void k_bc_shift(Geom g, T cval, T *__restrict__ v)
{
    const long long nitems = (long long)g.nx * g.ny * g.nz;
    for (long long it = (long long)blockIdx.x * OP_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * OP_THREADS) {
        const long long row = it / g.nx;
        const int x = (int)(it - row * g.nx), y = (int)(row % g.ny), z = (int)(row / g.ny);
        const long long i = lidx(g, z, y, x);
        v[i] = v[i] - cval;
    }
}

template <typename T>
__global__ __launch_bounds__(OP_THREADS) void k_bc_dirichlet_copy(Geom g, int mask, T *__restrict__ x_, const T *__restrict__ rhs)
{
    const long long nitems = (long long)g.nx * g.ny * g.nz;
    for (long long it = (long long)blockIdx.x * OP_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * OP_THREADS) {
        const long long row = it / g.nx;
        const int x = (int)(it - row * g.nx), y = (int)(row % g.ny), z = (int)(row / g.ny);
        if (bc_faces(g, z, y, x) & ~mask) {
            const long long i = lidx(g, z, y, x);
            x_[i] = rhs[i];
        }
    }
}

// ---------------------------------------------------------------- launchers
}  // namespace

template <typename T>
int launch_bc_residual(hipStream_t s, const Geom &g, const Coef<T> &c, int mask, const T *u, const T *b, T *r, double *partials, int cap,
                       bool plain)
{
    if (march_takes<T>(g, plain)) {
        const MarchGrid m = march_grid<T>(g);
        if (m.grid <= cap) {
            const dim3 gr(m.grid), bl(64 * MBW);
            if (r) hipLaunchKernelGGL((k_bc_march<T, OP_RES, true>), gr, bl, 0, s, g, c, mask, (T)1, u, b, r, partials, m.nbx, m.nby, m.nbz, m.zc, StepCoef<T>{});
            else hipLaunchKernelGGL((k_bc_march<T, OP_RES, false>), gr, bl, 0, s, g, c, mask, (T)1, u, b, r, partials, m.nbx, m.nby, m.nbz, m.zc, StepCoef<T>{});
            return m.grid;
        }
    }
    return plain_residual(s, g, BcOp<T>{c, mask}, u, b, r, partials, cap);
}

template <typename T>
void launch_bc_jacobi(hipStream_t s, const Geom &g, const Coef<T> &c, int mask, T omega, const T *u, const T *b, T *out, bool plain)
{
    if (march_takes<T>(g, plain)) {
        const MarchGrid m = march_grid<T>(g);
        hipLaunchKernelGGL((k_bc_march<T, OP_JAC, false>), dim3(m.grid), dim3(64 * MBW), 0, s, g, c, mask, omega, u, b, out,
                           (double *)nullptr, m.nbx, m.nby, m.nbz, m.zc, StepCoef<T>{});
        return;
    }
    plain_jacobi(s, g, BcOp<T>{c, mask}, omega, u, b, out);
}

template <typename T>
void launch_bc_heat_rhs(hipStream_t s, const Geom &g, const Coef<T> &c0, int mask, double dt, double theta, const T *u, const T *f, T *out,
                        bool plain)
{
    const StepCoef<T> st = step_coef<T>(dt, theta);
    if (march_takes<T>(g, plain)) {
        const MarchGrid m = march_grid<T>(g);
        const dim3 gr(m.grid), bl(64 * MBW);
#define MG_BC(SRC, NB) hipLaunchKernelGGL((k_bc_march<T, OP_STEP, true, SRC, NB>), gr, bl, 0, s, g, c0, mask, (T)1, u, f, out, (double *)nullptr, m.nbx, m.nby, m.nbz, m.zc, st)
        if (theta != 1.0) { if (f) MG_BC(true, true); else MG_BC(false, true); }
        else { if (f) MG_BC(true, false); else MG_BC(false, false); }
#undef MG_BC
        return;
    }
    plain_step(s, g, BcOp<T>{c0, mask}, st, u, f, out);
}

template <typename T>
void launch_bc_rb_colour(hipStream_t s, const Geom &g, const Coef<T> &c, int mask, int colour, T *u, const T *b)
{
    plain_rb_colour(s, g, BcOp<T>{c, mask}, colour, u, b);
}

template <typename T>
void launch_bc_restrict_fw(hipStream_t s, const Geom &gf, const Geom &gc, int mask, const T *fine, T *coarse)
{
    const dim3 gr(plain_grid((long long)gc.nx * gc.ny * gc.nz, OP_MAX_BLOCKS)), bl(OP_THREADS);
    if (gc.dim == 3 && is_semi_transition(gf, gc)) hipLaunchKernelGGL((k_bc_restrict<T, 3, false>), gr, bl, 0, s, gf, gc, mask, fine, coarse);
    else if (gc.dim == 3) hipLaunchKernelGGL((k_bc_restrict<T, 3, true>), gr, bl, 0, s, gf, gc, mask, fine, coarse);
    else hipLaunchKernelGGL((k_bc_restrict<T, 2, false>), gr, bl, 0, s, gf, gc, mask, fine, coarse);
}

template <typename T>
void launch_bc_coarse(hipStream_t s, const Geom &g, const Coef<T> &c, int mask, T omega, int smoother, T *x, T *tmp, const T *rhs,
                      int maxit, double tol, int fixed, CoarseOut *d_out)
{
    coarse_solve(s, g, BcOp<T>{c, mask}, omega, smoother, x, tmp, rhs, maxit, tol, fixed, d_out);
}

template <typename T>
int launch_bc_wsum(hipStream_t s, const Geom &g, int mask, const T *v, double *partials, int cap)
{
    const int nb = plain_grid((long long)g.nx * g.ny * g.nz, cap);
    hipLaunchKernelGGL((k_bc_wsum<T>), dim3(nb), dim3(OP_THREADS), 0, s, g, mask, v, partials);
    return nb;
}

template <typename T>
void launch_bc_shift(hipStream_t s, const Geom &g, T cval, T *v)
{
    const int nb = plain_grid((long long)g.nx * g.ny * g.nz, OP_MAX_BLOCKS);
    hipLaunchKernelGGL((k_bc_shift<T>), dim3(nb), dim3(OP_THREADS), 0, s, g, cval, v);
}

template <typename T>
void launch_bc_dirichlet_copy(hipStream_t s, const Geom &g, int mask, T *x, const T *rhs)
{
    const int nb = plain_grid((long long)g.nx * g.ny * g.nz, OP_MAX_BLOCKS);
    hipLaunchKernelGGL((k_bc_dirichlet_copy<T>), dim3(nb), dim3(OP_THREADS), 0, s, g, mask, x, rhs);
}

#define MG_BC_INST(T)                                                                                                                   \
    template int launch_bc_residual<T>(hipStream_t, const Geom &, const Coef<T> &, int, const T *, const T *, T *, double *, int, bool); \
    template void launch_bc_jacobi<T>(hipStream_t, const Geom &, const Coef<T> &, int, T, const T *, const T *, T *, bool);             \
    template void launch_bc_heat_rhs<T>(hipStream_t, const Geom &, const Coef<T> &, int, double, double, const T *, const T *, T *, bool); \
    template void launch_bc_rb_colour<T>(hipStream_t, const Geom &, const Coef<T> &, int, int, T *, const T *);                         \
    template void launch_bc_restrict_fw<T>(hipStream_t, const Geom &, const Geom &, int, const T *, T *);                               \
    template void launch_bc_coarse<T>(hipStream_t, const Geom &, const Coef<T> &, int, T, int, T *, T *, const T *, int, double, int,  \
                                      CoarseOut *);                                                                                     \
    template int launch_bc_wsum<T>(hipStream_t, const Geom &, int, const T *, double *, int);                                           \
    template void launch_bc_shift<T>(hipStream_t, const Geom &, T, T *);                                                                \
    template void launch_bc_dirichlet_copy<T>(hipStream_t, const Geom &, int, T *, const T *);
MG_BC_INST(double)
MG_BC_INST(float)
#undef MG_BC_INST

}  // namespace mg
