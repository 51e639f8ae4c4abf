// mg_heat.hip -- right-hand side of one theta-scheme step of u_t = -A0 u + f on level 0 (mg_heat_step / mg_heat_rhs,
// include/mg_hip.h; driver: Solver::heat_step in mg_solver.cpp). The step's system is
//     (1/(theta dt) I + A0) u' = (f + u/dt - (1 - theta) A0 u) / theta          (interior rows; Dirichlet rows: u' = u)
// and this file builds its right-hand side in ONE streaming pass over u (+ f): 8 R (+ 8 R) + 8 W bytes per fp64 node,
// half of that in fp32 -- the bytes of the saved residual (k_sweep3d<OP_RESIDUAL, SAVE>, mg_jacobi_fast.hip), whose
// tiling this kernel takes over:
//
//  * one lane owns one aligned 16-byte vector of x (Vec16); a wave64 covers 64 vectors of RY = 2 rows, BW = 4 waves are
//    stacked in y; in 3-D the workgroup marches ZC planes with the (z-1, z, z+1) values of its columns in registers, so
//    u is loaded once per workgroup column; x-neighbours come from the neighbouring lanes (DPP whole-wave shifts, one
//    scalar load at either end of the wave), y-neighbours from the wave's other row or two halo rows that hit L1 / L2;
//  * XCD-aware block order (xcd_block): each XCD sweeps a contiguous run of rows / planes;
//  * f and the output have no reuse inside the pass: non-temporal loads and stores (u too in the stencil-free form);
//  * only the first nx elements of a row are looked at; on rows with one column left over (nx % V == 1: every
//    n = 2^k m + 1 grid) that column is written as ONE full 128-byte line -- its value, then the zeros the padding
//    columns hold -- by lanes 56 .. 63 of the wave that holds the row's last full vector (mg_device.h); any other
//    remainder is stored element by element by the lane that owns it.
//
// Arithmetic contract (compiled with -ffp-contract=off; tests/test_heat_gpu.py restates it in numpy), all in T, every
// operation rounded separately, in the row order of mg_residual:
//   s   = (((((((0 + cz u[k-1]) + cy u[j-1]) + cx u[i-1]) + cd0 u) + cx u[i+1]) + cy u[j+1]) + cz u[k+1])   (no cz terms in 2-D)
//   rhs = ((f + rdt u) - omt s) rth      interior nodes;  no source: (rdt u - omt s) rth
//   rhs = u                              Dirichlet nodes, bit for bit
//   rdt = (T)(1 / dt), omt = (T)(1 - theta), rth = (T)(1 / theta), cd0 = the UNSHIFTED diagonal of level 0
// theta == 1 (STENCIL == false): rhs = f + rdt u (rdt u without a source) -- omt = 0 and rth = 1 make the general
// expression give the same value for finite data, so no neighbour is loaded.
// Instantiations: with / without source x with / without stencil, per dtype and dimension.
#include "mg_kernels.h"
#include "mg_device.h"

#include <algorithm>

namespace mg {
namespace {

constexpr int HRY = 2, HBW = 4, HZC = 3;   // rows per wave, waves per workgroup, planes marched (k_sweep3d's tile)

template <typename T>
struct HeatCoef {
    T cx, cy, cz, cd0;
    T rdt, omt, rth;
};

template <typename T, int DIM, bool SRC, bool STENCIL>
__global__ __launch_bounds__(64 * HBW) void k_heat_rhs(Geom g, HeatCoef<T> c, const T *__restrict__ u, const T *__restrict__ f,
                                                       T *__restrict__ out, int nbx, int nby, int nbz)
{
    constexpr int V = Vec16<T>::n;
    constexpr bool MARCH = STENCIL && DIM == 3;   // z-neighbours kept in registers
    typedef typename Vec16<T>::type vec;

    const int nblocks = nbx * nby * nbz;
    const int bid = xcd_block(blockIdx.x, (nblocks + 7) >> 3);
    if (bid >= nblocks) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int bx = bid % nbx, by = (bid / nbx) % nby, bz = bid / (nbx * nby);
    const int x0 = V * (bx * 64 + lane);
    const int x0c = min(x0, g.pitch - V);   // clamped for loads: every lane stays active
    const bool xfull = x0 + V <= g.nx;      // the lane's vector lies inside the row
    const int yb = (by * HBW + wv) * HRY;
    const int zc = (g.nz + nbz - 1) / nbz;
    const int z0 = bz * zc;
    const int zend = min(z0 + zc, g.nz);
    // one column left over: the wave that holds the row's last full vector writes it as a full line
    const bool tail1 = g.nx % V == 1 && g.nx > V;
    const bool tailwave = tail1 && (bx * 64 * V <= g.nx - 1 - V) && (g.nx - 1 - V < (bx + 1) * 64 * V);
    const int part = (!tail1 && !xfull && x0 < g.nx) ? g.nx - x0 : 0;   // elements of a partial last vector stored one by one

    long long rowoff[HRY];
    bool yin[HRY], ybnd[HRY];
#pragma unroll
    for (int r = 0; r < HRY; r++) {
        const int y = yb + r;
        yin[r] = y < g.ny;
        const int yc = min(y, g.ny - 1);
        ybnd[r] = (yc == 0) || (yc == g.ny - 1);
        rowoff[r] = (long long)yc * g.pitch + x0c;
    }
    const long long off_lo = (long long)min(max(yb - 1, 0), g.ny - 1) * g.pitch + x0c;
    const long long off_hi = (long long)min(yb + HRY, g.ny - 1) * g.pitch + x0c;
    const bool edge_l = lane == 0 && x0c > 0, edge_r = lane == 63 && x0c + V < g.pitch;

    vec zm[HRY], cc[HRY], zp[HRY];
    const T *pz = u + (long long)z0 * g.plane;
    if (MARCH) {
#pragma unroll
        for (int r = 0; r < HRY; r++) {
            zm[r] = *(const vec *)(pz - g.plane + rowoff[r]);
            cc[r] = *(const vec *)(pz + rowoff[r]);
        }
    }
    for (int z = z0; z < zend; z++, pz += g.plane) {
        const long long zo = (long long)z * g.plane;
        vec b[HRY];
#pragma unroll
        for (int r = 0; r < HRY; r++) {
            if (MARCH) zp[r] = *(const vec *)(pz + g.plane + rowoff[r]);
            else if (STENCIL) cc[r] = *(const vec *)(pz + rowoff[r]);
            else cc[r] = __builtin_nontemporal_load((const vec *)(pz + rowoff[r]));
            if (SRC) b[r] = __builtin_nontemporal_load((const vec *)(f + zo + rowoff[r]));
        }
        vec hlo = (vec)(0), hhi = (vec)(0);
        if (STENCIL) {
            hlo = *(const vec *)(pz + off_lo);
            hhi = *(const vec *)(pz + off_hi);
        }
        const int gz = g.gz0 + z;
        const bool zb = DIM == 3 && ((gz == 0) || (gz == g.gnz - 1));
#pragma unroll
        for (int r = 0; r < HRY; r++) {
            T xm = 0, xp = 0;
            if (STENCIL) {
                T el = 0, er = 0;
                if (edge_l) el = pz[rowoff[r] - 1];
                if (edge_r) er = pz[rowoff[r] + V];
                xm = lane_from_prev(cc[r][V - 1], el);
                xp = lane_from_next(cc[r][0], er);
            }
            const vec ym = (r > 0) ? cc[r > 0 ? r - 1 : 0] : hlo;
            const vec yp = (r < HRY - 1) ? cc[r < HRY - 1 ? r + 1 : 0] : hhi;
            const bool rb = zb || ybnd[r];
            vec res;
#pragma unroll
            for (int e = 0; e < V; e++) {
                const T uc = cc[r][e];
                T t = c.rdt * uc;
                if (SRC) t = b[r][e] + t;
                if (STENCIL) {
                    const T left = (e == 0) ? xm : cc[r][e > 0 ? e - 1 : 0];
                    const T right = (e == V - 1) ? xp : cc[r][e < V - 1 ? e + 1 : 0];
                    T sum = 0;
                    if (DIM == 3) sum += c.cz * zm[r][e];
                    sum += c.cy * ym[e];
                    sum += c.cx * left;
                    sum += c.cd0 * uc;
                    sum += c.cx * right;
                    sum += c.cy * yp[e];
                    if (DIM == 3) sum += c.cz * zp[r][e];
                    t = (t - c.omt * sum) * c.rth;
                }
                const bool bnd = rb || (x0 + e == 0) || (x0 + e == g.nx - 1);
                res[e] = bnd ? uc : t;
            }
            if (yin[r]) {
                T *const po = out + zo + rowoff[r];
                if (xfull) {
                    __builtin_nontemporal_store(res, (vec *)po);
                } else if (part) {
#pragma unroll
                    for (int e = 0; e < V; e++)
                        if (e < part) po[e] = res[e];
                }
                if (tailwave && lane >= 56) {
                    // column nx-1 (Dirichlet: rhs = u) as one full 128-byte line: value + zero padding
                    const int j = lane - 56;
                    constexpr int LINE = 128 / (int)sizeof(T);
                    const int xs = g.nx - 1 + V * j;
                    const int line_end = ((g.nx - 1) / LINE + 1) * LINE;
                    const long long ro = zo + (rowoff[r] - x0c);
                    if (xs < line_end) {
                        vec tv = (vec)(0);
                        if (j == 0) tv[0] = pz[(rowoff[r] - x0c) + g.nx - 1];
                        __builtin_nontemporal_store(tv, (vec *)(out + ro + xs));
                    }
                }
            }
        }
        if (MARCH) {
#pragma unroll
            for (int r = 0; r < HRY; r++) { zm[r] = cc[r]; cc[r] = zp[r]; }
        }
    }
}

}  // namespace

template <typename T>
void launch_heat_rhs(hipStream_t s, const Geom &g, const double coef0[4], double dt, double theta, const T *u, const T *f, T *out)
{
    constexpr int V = Vec16<T>::n;
    const HeatCoef<T> c{(T)coef0[0], (T)coef0[1], (T)coef0[2], (T)coef0[3], (T)(1.0 / dt), (T)(1.0 - theta), (T)(1.0 / theta)};
    // vectors a row needs lanes for: the full ones, and a partial last one unless it is the single tail column
    const int nvec = std::max(1, g.nx / V + (g.nx % V > 1 ? 1 : 0));
    const int nbx = (nvec + 63) / 64, nby = (g.ny + HRY * HBW - 1) / (HRY * HBW);
    int nbz = (g.nz + HZC - 1) / HZC;
    if (nbx * nby * nbz < 1024) nbz = g.nz;   // latency-bound levels: one plane per workgroup (fast_grid, mg_jacobi_fast.hip)
    const int grid = ((nbx * nby * nbz + 7) / 8) * 8;
    const dim3 gr(grid), bl(64 * HBW);
    const bool stencil = theta != 1.0;
#define MG_HEAT(DIM, SRC, ST) hipLaunchKernelGGL((k_heat_rhs<T, DIM, SRC, ST>), gr, bl, 0, s, g, c, u, f, out, nbx, nby, nbz)
#define MG_HEAT_DIM(DIM)                                                     \
    do {                                                                     \
        if (f) { if (stencil) MG_HEAT(DIM, true, true); else MG_HEAT(DIM, true, false); } \
        else { if (stencil) MG_HEAT(DIM, false, true); else MG_HEAT(DIM, false, false); } \
    } while (0)
    if (g.dim == 3) MG_HEAT_DIM(3); else MG_HEAT_DIM(2);
#undef MG_HEAT_DIM
#undef MG_HEAT
}

template void launch_heat_rhs<double>(hipStream_t, const Geom &, const double[4], double, double, const double *, const double *, double *);
template void launch_heat_rhs<float>(hipStream_t, const Geom &, const double[4], double, double, const float *, const float *, float *);

}  // namespace mg
