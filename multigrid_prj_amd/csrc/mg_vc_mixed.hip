// mg_vc_mixed.hip -- fine-grid kernels of the mixed-precision defect correction on the variable-coefficient operator
// (mg_mixed_solve / mg_mixed_kernel with MG_MIXED_OPERATOR(MG_MIXED_ON_COEFFICIENT), include/mg_hip.h; driver:
// Solver::mixed_solve in mg_drivers.cpp): u and b live in fp64, the coefficient a, the correction e and the scaled residual
// r32 in the handle's fp32 arrays. The operator is mg_vc_*'s -- L = sigma I - div(a grad .) with the face mask of
// mg_vc_set_faces -- evaluated in fp64 with a = (double) of the fp32 level-0 coefficient (every fp32 value is exact in fp64).
//
//   k_vc_mixed_march<CORR, DIV>           the marching tile: mask 0 on 3-D levels with rows of at least 16 fp64 vectors
//                                         (vc_mixed_march_ok, mg_geom.h)                    8+4+4+8 R, 8+4 W per node
//   k_vc_mixed_plain<DIM, CORR, DIV>      one thread per node, every shape and every mask (2-D, short rows, form 1, and every
//                                         non-zero mask: a mirrored form of the tile measured SLOWER than this kernel, 3.03 ms
//                                         against 2.61 ms at 513^3 with all faces Neumann, and is not kept)
// CORR = false is the first residual (no e, no u'); with CORR u' = u + (double)e / s_in is formed and stored OUT OF PLACE
// (another workgroup may still read u at a neighbour; the driver swaps the two pointers).
//
// The tile is k_vc_march<double>'s (mg_vc.hip): a lane owns one aligned 16-byte vector of fp64 x (two nodes; the fp32
// arrays are read and written 8 bytes at a time), a wave covers 64 vectors of MRY = 2 rows, MBW = 4 waves are stacked in y
// and the workgroup marches zc planes with the planes z-1, z, z+1 of u' AND a of its columns in registers. u' is formed
// ONCE, when a plane of u and e arrives (the Dirichlet test there is a select on position), so e is never held; the
// x-neighbours are the neighbouring lanes' u' (whole-wave DPP shifts; the two edge lanes form theirs from one u and one e),
// the y-halo rows come through L1 / L2, u and e both. b is loaded and u' / r32 stored non-temporally, the block order is
// XCD-aware, and the odd last column of a 2^k + 1 row (a Dirichlet column: u' = u, r = 0) is
// written as full 128-byte lines, value + the zeros the padding columns hold, by lanes 48 .. 63 of the wave that holds the
// row's last full vector. Two pitches, as in mg_mixed.hip: g64 for u, b and u', the handle's own g32 for e, a and r32.
// Ghost planes and padding columns are read (they exist and hold zeros) and what is computed from them is dropped by selects.
//
// Arithmetic contract (compiled with -ffp-contract=off; tests/test_mixedvc_gpu.py restates it in numpy), all in fp64, every
// operation rounded separately, w_a = -c_a / 2 with c_a the level's off-diagonal of mg_level_coefficients, a_q = (double)a32_q:
//   u' = u + (double)e / s_in   at the mask's unknowns;  u' = u on its Dirichlet nodes (e is not looked at there)
//   s = 0, d = sigma; for the neighbours q (or their mirror images) in the order z-, y-, x-, x+, y+, z+ (no z in 2-D):
//       g = w_a * (a_i + a_q);  s = s + g * u'_q;  d = d + g
//   r = b - (d * u'_i - s) at unknowns, r = 0 on Dirichlet nodes;  r32 = (float)(s_out * r), round to nearest even
//   the sum of r^2 (unscaled) in double: one partial per workgroup, added in a fixed order by k_reduce_final (no atomics)
// When s_in is a power of two with a normal reciprocal (what the driver always passes) the division is a multiplication by
// that reciprocal: the same correctly rounded quotient. Any other s_in takes the division.
#include "mg_opfamily.h"

namespace mg {
namespace {

struct VmCoef {
    double wx, wy, wz, sigma;
};

template <bool DIV>
__device__ __forceinline__ double vm_corrected(double u, float e, double t)
{
    return DIV ? u + (double)e / t : u + (double)e * t;
}

__device__ __forceinline__ void vm_nb(double w, double ai, double aq, double uq, double &s, double &d)
{
    const double g = w * (ai + aq);
    s = s + g * uq;
    d = d + g;
}

// u' at node (z, y, x), formed from global memory; i64 / i32: the node's element index in the two layouts
template <bool CORR, bool DIV>
__device__ __forceinline__ double vm_uprime(const Geom &g, int mask, const double *__restrict__ u, const float *__restrict__ e,
                                            int z, int y, int x, long long i64, long long i32, double t)
{
    const double uv = u[i64];
    if (!CORR || (bc_faces(g, z, y, x) & ~mask)) return uv;
    return vm_corrected<DIV>(uv, e[i32], t);
}

// the contract at one node from global memory: u' -> up, the residual -> the return value (0 on a Dirichlet node)
template <int DIM, bool CORR, bool DIV>
__device__ __forceinline__ double vm_point(const Geom &g, const Geom &g32, const VmCoef &c, int mask, const double *__restrict__ u,
                                           const float *__restrict__ e, const float *__restrict__ a, const double *__restrict__ b,
                                           double t, int z, int y, int x, double &up)
{
    const long long i64 = lidx(g, z, y, x), i32 = lidx(g32, z, y, x);
    const int f = bc_faces(g, z, y, x);
    if (f & ~mask) { up = u[i64]; return 0.; }
    up = CORR ? vm_corrected<DIV>(u[i64], e[i32], t) : u[i64];
    // the six neighbours, mirrored on the Neumann faces the node lies on
    const int zs[2] = {(f & FZLO) ? z + 1 : z - 1, (f & FZHI) ? z - 1 : z + 1};
    const int ys[2] = {(f & FYLO) ? y + 1 : y - 1, (f & FYHI) ? y - 1 : y + 1};
    const int xs[2] = {(f & FXLO) ? x + 1 : x - 1, (f & FXHI) ? x - 1 : x + 1};
    const double ai = (double)a[i32];
    double s = 0., d = c.sigma;
    auto nb = [&](double w, int nz, int ny, int nx) {
        const long long q64 = lidx(g, nz, ny, nx), q32 = lidx(g32, nz, ny, nx);
        vm_nb(w, ai, (double)a[q32], vm_uprime<CORR, DIV>(g, mask, u, e, nz, ny, nx, q64, q32, t), s, d);
    };
    if (DIM == 3) nb(c.wz, zs[0], y, x);
    nb(c.wy, z, ys[0], x);
    nb(c.wx, z, y, xs[0]);
    nb(c.wx, z, y, xs[1]);
    nb(c.wy, z, ys[1], x);
    if (DIM == 3) nb(c.wz, zs[1], y, x);
    return b[i64] - (d * up - s);
}

// ---------------------------------------------------------------- the plain form
template <int DIM, bool CORR, bool DIV>
__global__ __launch_bounds__(OP_THREADS) void k_vc_mixed_plain(Geom g, Geom g32, VmCoef c, int mask, const double *__restrict__ u,
                                                               const float *__restrict__ e, const float *__restrict__ a,
                                                               const double *__restrict__ b, double *__restrict__ un,
                                                               float *__restrict__ r32, double t_in, double s_out,
                                                               double *__restrict__ partials)
{
    __shared__ double sh[OP_THREADS / 64];
    const long long nitems = (long long)g.nx * g.ny * g.nz;
    double acc = 0.;
    for (long long it = (long long)blockIdx.x * OP_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * OP_THREADS) {
        const long long row = it / g.nx;
        const int x = (int)(it - row * g.nx), y = (int)(row % g.ny), z = (int)(row / g.ny);
        double up;
        const double r = vm_point<DIM, CORR, DIV>(g, g32, c, mask, u, e, a, b, t_in, z, y, x, up);
        acc += r * r;
        if (CORR) un[lidx(g, z, y, x)] = up;
        r32[lidx(g32, z, y, x)] = (float)(s_out * r);
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---------------------------------------------------------------- the marching tile (3-D)
typedef double vd2 __attribute__((ext_vector_type(2)));
typedef float vf2 __attribute__((ext_vector_type(2)));

// the lane's two u' of a row (yzdir: the row or its plane lies on a face, every node of it is a Dirichlet node) from the vectors
// of u and e at (o64, o32); x0: the column of element 0
template <bool CORR, bool DIV>
__device__ __forceinline__ vd2 vm_row(const Geom &g, const double *__restrict__ pu, const float *__restrict__ pe,
                                      long long o64, long long o32, int x0, bool yzdir, double t)
{
    vd2 v = *(const vd2 *)(pu + o64);
    if (CORR) {
        const vf2 ev = *(const vf2 *)(pe + o32);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const double cv = vm_corrected<DIV>(v[k], ev[k], t);
            v[k] = (yzdir || x0 + k == 0 || x0 + k == g.nx - 1) ? v[k] : cv;
        }
    }
    return v;
}

// one u' across the wave's edge, at column x of the same row
template <bool CORR, bool DIV>
__device__ __forceinline__ double vm_one(const Geom &g, const double *__restrict__ pu, const float *__restrict__ pe,
                                         long long o64, long long o32, int x, bool yzdir, double t)
{
    const double v = pu[o64];
    if (!CORR) return v;
    const double cv = vm_corrected<DIV>(v, pe[o32], t);
    return (yzdir || x == 0 || x == g.nx - 1) ? v : cv;
}

template <bool CORR, bool DIV>
__global__ __launch_bounds__(64 * MBW) void k_vc_mixed_march(Geom g, Geom g32, VmCoef c, const double *__restrict__ u,
                                                             const float *__restrict__ e, const float *__restrict__ a,
                                                             const double *__restrict__ b, double *__restrict__ un,
                                                             float *__restrict__ r32, double t_in, double s_out,
                                                             double *__restrict__ partials, int nbx, int nby, int nbz, int zc)
{
    constexpr int V = 2;
    __shared__ double sh[MBW];

    const int nblocks = nbx * nby * nbz;
    const int bid = xcd_block(blockIdx.x, (nblocks + 7) >> 3);
    if (bid >= nblocks) {   // the whole workgroup
        if (threadIdx.x == 0) partials[blockIdx.x] = 0.;
        return;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int bx = bid % nbx, by = (bid / nbx) % nby, bz = bid / (nbx * nby);
    const int x0 = V * (bx * 64 + lane);
    const int x0c = min(x0, g.pitch - V);   // clamped for loads: every lane stays active (g32.pitch >= g.pitch)
    const bool xfull = x0 + V <= g.nx;      // the lane's vector lies inside the row: it stores and sums both nodes
    const int yb = (by * MBW + wv) * MRY;
    const int z0 = bz * zc, zend = min(z0 + zc, g.nz);
    // one column left over (odd nx): the wave that holds the row's last full vector writes it as full lines
    const bool tail1 = g.nx % V == 1;
    const bool tailwave = tail1 && (bx * 64 * V <= g.nx - 1 - V) && (g.nx - 1 - V < (bx + 1) * 64 * V);

    long long ro64[MRY], ro32[MRY];
    bool yin[MRY], ydir[MRY];
#pragma unroll
    for (int r = 0; r < MRY; r++) {
        const int y = yb + r;
        yin[r] = y < g.ny;
        const int yc = min(y, g.ny - 1);
        ydir[r] = yc == 0 || yc == g.ny - 1;
        ro64[r] = (long long)yc * g.pitch + x0c;
        ro32[r] = (long long)yc * g32.pitch + x0c;
    }
    const int ylo = min(max(yb - 1, 0), g.ny - 1), yhi = min(yb + MRY, g.ny - 1);
    const long long lo64 = (long long)ylo * g.pitch + x0c, lo32 = (long long)ylo * g32.pitch + x0c;
    const long long hi64 = (long long)yhi * g.pitch + x0c, hi32 = (long long)yhi * g32.pitch + x0c;
    const bool ylodir = ylo == 0 || ylo == g.ny - 1, yhidir = yhi == 0 || yhi == g.ny - 1;
    const bool edge_l = lane == 0 && x0c > 0, edge_r = lane == 63 && x0c + V < g.pitch;
    auto zdir_of = [&](int z) { return z == 0 || z == g.nz - 1; };   // whole levels: gz == z

    vd2 uzm[MRY], ucc[MRY], uzp[MRY];
    vf2 azm[MRY], acc_[MRY], azp[MRY];
    const double *pu = u + (long long)z0 * g.plane;
    const float *pa = a + (long long)z0 * g32.plane, *pe = (CORR ? e : a) + (long long)z0 * g32.plane;   // !CORR: never read
    {
        const bool zdm = zdir_of(z0 - 1), zd0 = zdir_of(z0);
#pragma unroll
        for (int r = 0; r < MRY; r++) {
            uzm[r] = vm_row<CORR, DIV>(g, pu - g.plane, pe - g32.plane, ro64[r], ro32[r], x0c, zdm || ydir[r], t_in);
            ucc[r] = vm_row<CORR, DIV>(g, pu, pe, ro64[r], ro32[r], x0c, zd0 || ydir[r], t_in);
            azm[r] = *(const vf2 *)(pa - g32.plane + ro32[r]);
            acc_[r] = *(const vf2 *)(pa + ro32[r]);
        }
    }
    double acc = 0.;
    for (int z = z0; z < zend; z++, pu += g.plane, pa += g32.plane, pe += g32.plane) {
        const long long zo64 = (long long)z * g.plane, zo32 = (long long)z * g32.plane;
        const bool zd = zdir_of(z), zdp = zdir_of(z + 1);
        vd2 bv[MRY];
#pragma unroll
        for (int r = 0; r < MRY; r++) {
            uzp[r] = vm_row<CORR, DIV>(g, pu + g.plane, pe + g32.plane, ro64[r], ro32[r], x0c, zdp || ydir[r], t_in);
            azp[r] = *(const vf2 *)(pa + g32.plane + ro32[r]);
            bv[r] = __builtin_nontemporal_load((const vd2 *)(b + zo64 + ro64[r]));
        }
        const vd2 ulo = vm_row<CORR, DIV>(g, pu, pe, lo64, lo32, x0c, zd || ylodir, t_in);
        const vd2 uhi = vm_row<CORR, DIV>(g, pu, pe, hi64, hi32, x0c, zd || yhidir, t_in);
        const vf2 alo = *(const vf2 *)(pa + lo32), ahi = *(const vf2 *)(pa + hi32);
#pragma unroll
        for (int r = 0; r < MRY; r++) {
            double uel = 0., uer = 0.;
            float ael = 0.f, aer = 0.f;
            if (edge_l) { uel = vm_one<CORR, DIV>(g, pu, pe, ro64[r] - 1, ro32[r] - 1, x0c - 1, zd || ydir[r], t_in); ael = pa[ro32[r] - 1]; }
            if (edge_r) { uer = vm_one<CORR, DIV>(g, pu, pe, ro64[r] + V, ro32[r] + V, x0c + V, zd || ydir[r], t_in); aer = pa[ro32[r] + V]; }
            const double uxm = lane_from_prev(ucc[r][V - 1], uel), uxp = lane_from_next(ucc[r][0], uer);
            const float axm = lane_from_prev(acc_[r][V - 1], ael), axp = lane_from_next(acc_[r][0], aer);
            const vd2 uym = (r > 0) ? ucc[r > 0 ? r - 1 : 0] : ulo, uyp = (r < MRY - 1) ? ucc[r < MRY - 1 ? r + 1 : 0] : uhi;
            const vf2 aym = (r > 0) ? acc_[r > 0 ? r - 1 : 0] : alo, ayp = (r < MRY - 1) ? acc_[r < MRY - 1 ? r + 1 : 0] : ahi;
            const bool own = xfull && yin[r];   // the lane stores and sums the row's two nodes
            vf2 rv;
#pragma unroll
            for (int k = 0; k < V; k++) {
                const double ui = ucc[r][k], ai = (double)acc_[r][k];
                const double ul = (k == 0) ? uxm : ucc[r][0], ur = (k == V - 1) ? uxp : ucc[r][V - 1];
                const double al = (double)((k == 0) ? axm : acc_[r][0]), ar = (double)((k == V - 1) ? axp : acc_[r][V - 1]);
                double s = 0., d = c.sigma;
                vm_nb(c.wz, ai, (double)azm[r][k], uzm[r][k], s, d);
                vm_nb(c.wy, ai, (double)aym[k], uym[k], s, d);
                vm_nb(c.wx, ai, al, ul, s, d);
                vm_nb(c.wx, ai, ar, ur, s, d);
                vm_nb(c.wy, ai, (double)ayp[k], uyp[k], s, d);
                vm_nb(c.wz, ai, (double)azp[r][k], uzp[r][k], s, d);
                const bool bnd = zd || ydir[r] || x0 + k == 0 || x0 + k == g.nx - 1;
                const double res = bnd ? 0. : bv[r][k] - (d * ui - s);
                if (own) acc += res * res;
                rv[k] = (float)(s_out * res);
            }
            if (yin[r]) {
                if (xfull) {
                    if (CORR) __builtin_nontemporal_store(ucc[r], (vd2 *)(un + zo64 + ro64[r]));
                    __builtin_nontemporal_store(rv, (vf2 *)(r32 + zo32 + ro32[r]));
                }
                if (tailwave && lane >= 48) {
                    // column nx-1 (Dirichlet: u' = u, r = 0) as full 128-byte lines, value + zero padding: 16 doubles of u' (lanes
                    // 48 .. 55) and 32 floats of r32 (lanes 48 .. 63)
                    const int j = lane - 48;
                    const int xs = g.nx - 1 + V * j;
                    const int end64 = ((g.nx - 1) / 16 + 1) * 16, end32 = ((g.nx - 1) / 32 + 1) * 32;
                    vd2 tu = (vd2)(0.);
                    const vf2 tr = (vf2)(0.f);
                    if (CORR && j == 0) tu[0] = pu[(ro64[r] - x0c) + g.nx - 1];
                    if (CORR && xs < end64) __builtin_nontemporal_store(tu, (vd2 *)(un + zo64 + (ro64[r] - x0c) + xs));
                    if (xs < end32) __builtin_nontemporal_store(tr, (vf2 *)(r32 + zo32 + (ro32[r] - x0c) + xs));
                }
            }
        }
#pragma unroll
        for (int r = 0; r < MRY; r++) { uzm[r] = ucc[r]; ucc[r] = uzp[r]; azm[r] = acc_[r]; acc_[r] = azp[r]; }
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

VmCoef vm_coef(const double coef[4], double sigma) { return VmCoef{-coef[0] / 2.0, -coef[1] / 2.0, -coef[2] / 2.0, sigma}; }

// a power of two whose reciprocal is a normal number: multiply by the (exact) reciprocal instead of dividing
bool vm_pow2(double scale_in, double *t)
{
    int ex = 0;
    const double inv = 1.0 / scale_in;
    const bool pow2 = scale_in > 0.0 && std::isfinite(scale_in) && std::frexp(scale_in, &ex) == 0.5 && std::isnormal(scale_in) &&
                      std::isnormal(inv);
    *t = pow2 ? inv : scale_in;
    return pow2;
}

}  // namespace

bool vc_mixed_march_takes(const Geom &g64, bool plain)
{
    return !plain && vc_mixed_march_ok(g64.dim, g64.nx, g64.ny, g64.nz) && g64.gz0 == 0 && g64.gnz == g64.nz;
}

// e32 == nullptr: the first residual (u_out, scale_in not looked at). -> the number of partial sums left in `partials`
int launch_vc_mixed(hipStream_t s, const Geom &g64, const Geom &g32, const double coef[4], double sigma, int mask, const double *u,
                    const float *e32, const float *a32, const double *b, double *u_out, float *r32, double scale_in, double scale_out,
                    double *partials, int cap, bool plain)
{
    const VmCoef c = vm_coef(coef, sigma);
    double t = 1.0;
    const bool corr = e32 != nullptr;
    const bool div = corr && !vm_pow2(scale_in, &t);
    if (mask == 0 && vc_mixed_march_takes(g64, plain)) {   // a non-zero mask takes the plain form: see the head of the file
        const MarchGrid m = march_grid<double>(g64);
        if (m.grid <= cap) {
            const dim3 gr(m.grid), bl(64 * MBW);
#define MG_VM(CORR, DIV) hipLaunchKernelGGL((k_vc_mixed_march<CORR, DIV>), gr, bl, 0, s, g64, g32, c, u, e32, a32, b, u_out, r32, t, scale_out, partials, m.nbx, m.nby, m.nbz, m.zc)
            if (!corr) MG_VM(false, false);
            else if (div) MG_VM(true, true);
            else MG_VM(true, false);
#undef MG_VM
            return m.grid;
        }
    }
    const int nb = plain_grid((long long)g64.nx * g64.ny * g64.nz, cap);
    const dim3 gr(nb), bl(OP_THREADS);
#define MG_VM(DIM, CORR, DIV) hipLaunchKernelGGL((k_vc_mixed_plain<DIM, CORR, DIV>), gr, bl, 0, s, g64, g32, c, mask, u, e32, a32, b, u_out, r32, t, scale_out, partials)
#define MG_VM_D(DIM) if (!corr) MG_VM(DIM, false, false); else if (div) MG_VM(DIM, true, true); else MG_VM(DIM, true, false)
    if (g64.dim == 3) { MG_VM_D(3); } else { MG_VM_D(2); }
#undef MG_VM_D
#undef MG_VM
    return nb;
}

}  // namespace mg
