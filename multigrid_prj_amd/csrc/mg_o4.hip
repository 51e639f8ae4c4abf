// mg_o4.hip -- level-0 kernels of the fourth-order defect correction (mg_o4_solve / mg_o4_residual /
// mg_o4_correct_residual, include/mg_hip.h; driver: Solver::o4_solve in mg_drivers.cpp): the residual is taken with the
// fourth-order operator sigma I + A4, the handle's second-order cycles solve the correction equation.
//
//   k_o4_residual<T, DIM, SAVE>     r = b - (sigma I + A4) u, stored (SAVE) or norm only; one partial sum of r^2 per workgroup
//   k_o4_correct_residual<T, DIM>   u' = u + e (interior; u on Dirichlet nodes, e not looked at), the same residual of u'
//   k_o4_march<T, CORR, SAVE>       the same two on 3-D levels with rows long enough to fill a wave (o4_march_ok, mg_geom.h)
// u' is written OUT OF PLACE (another workgroup may still read u at a neighbour); the driver swaps the two pointers. One
// pass of u, e, b in and u', r out instead of a correction pass followed by a residual pass.
//
// The plain form: one thread per node, lanes along x, every neighbour through L1 / L2; a grid-stride loop of at most
// O4_MAX_BLOCKS workgroups. It serves 2-D and every 3-D shape the marching tile does not take.
// The marching tile (k_heat_rhs's, mg_heat.hip, with radius 2): a lane owns one aligned 16-byte vector of x, a wave
// covers 64 vectors of RY rows (4 for the residual, 2 for the fused form, whose state is u and e: with 4 rows its fp64
// instantiation needs 256 VGPRs + 64 AGPRs, one wave per SIMD), MBW = 4 waves are stacked in y and the workgroup marches zc planes with the FIVE
// planes z-2 .. z+2 of its columns in registers, so u (and e) is loaded once per workgroup column and corrected once per
// loaded value. x-neighbours at +-1 and +-2 are the neighbouring lanes' vectors (whole-wave DPP shifts; the two edge
// lanes load theirs), y-neighbours the wave's other rows and two halo rows either side that hit L1 / L2. The closure
// rows and planes (j, k = 1 and n-2) are evaluated under wave-uniform tests, their far taps loaded directly; the two
// x-closure columns are the only per-lane branch. XCD-aware block order, non-temporal loads of b and stores of r and
// u'; the odd last column is written as one full 128-byte line as in mg_heat.hip.
//
// Arithmetic contract (compiled with -ffp-contract=off; tests/o4_ref.py restates it in numpy), all in T, every operation
// rounded separately. Per axis a with u(-2) .. u(+2) along it and i the node's index on it (n nodes):
//   2 <= i <= n-3:  p_a = ((16 (u(-1) + u(+1))) - (u(-2) + u(+2))) - 30 u
//   i == 1:         p_a = ((((10 u_0 - 15 u_1) - 4 u_2) + 14 u_3) - 6 u_4) + u_5         (u_0 the Dirichlet node)
//   i == n-2:       the mirror image, counted from the far boundary
//   A4u = ((sigma u + wz p_z) + wy p_y) + wx p_x   (no z term in 2-D),  w_a = (T)(c_a / 12)
//   r = b - A4u on interior nodes, 0 on Dirichlet nodes; the sum of r^2 in double, fixed order, no atomics.
#include "mg_kernels.h"
#include "mg_device.h"

#include <algorithm>
#include <cassert>

namespace mg {
namespace {

constexpr int O4_THREADS = 256, O4_MAX_BLOCKS = 2048;
constexpr int MBW = 4;                   // waves per workgroup of the marching tile
constexpr int RY_RES = 4, RY_CORR = 2;   // rows per wave: the residual / the fused correction + residual

template <typename T>
struct O4Coef {
    T wx, wy, wz, sigma;
};

template <typename T>
__device__ __forceinline__ T p_mid(T m2, T m1, T c, T p1, T p2)
{
    return (((T)16 * (m1 + p1)) - (m2 + p2)) - (T)30 * c;
}

// six-point one-sided closure; u0 is the Dirichlet node, u1 the node itself
template <typename T>
__device__ __forceinline__ T p_end(T u0, T u1, T u2, T u3, T u4, T u5)
{
    return ((((((T)10 * u0 - (T)15 * u1) - (T)4 * u2) + (T)14 * u3) - (T)6 * u4) + u5);
}

template <typename T>
__device__ __forceinline__ T a4_of(const O4Coef<T> &c, T uc, T pz, T py, T px, bool has_z)
{
    T s = c.sigma * uc;
    if (has_z) s = s + c.wz * pz;
    s = s + c.wy * py;
    s = s + c.wx * px;
    return s;
}

// p_a at index i of an axis of n nodes, at(k) = the value at index k of that axis
template <typename T, typename F>
__device__ __forceinline__ T axis_p(int i, int n, F &&at)
{
    if (i == 1) return p_end<T>(at(0), at(1), at(2), at(3), at(4), at(5));
    if (i == n - 2) return p_end<T>(at(n - 1), at(n - 2), at(n - 3), at(n - 4), at(n - 5), at(n - 6));
    return p_mid<T>(at(i - 2), at(i - 1), at(i), at(i + 1), at(i + 2));
}

// ---------------------------------------------------------------- the plain form
template <typename T, int DIM, bool CORR, bool SAVE>
__device__ __forceinline__ void o4_plain_body(const Geom &g, const O4Coef<T> &c, const T *__restrict__ u, const T *__restrict__ e,
                                              const T *__restrict__ b, T *__restrict__ un, T *__restrict__ r,
                                              double *__restrict__ partials, double *sh)
{
    const long long nitems = (long long)g.nx * g.ny * g.nz;
    // u' at (z, y, x): corrected on interior nodes only
    auto val = [&](int z, int y, int x) -> T {
        const long long i = lidx(g, z, y, x);
        T v = u[i];
        if (CORR) {
            bool in = x >= 1 && x <= g.nx - 2 && y >= 1 && y <= g.ny - 2;
            if (DIM == 3) in = in && g.gz0 + z >= 1 && g.gz0 + z <= g.gnz - 2;
            if (in) v = v + e[i];
        }
        return v;
    };
    double acc = 0.;
    for (long long it = (long long)blockIdx.x * O4_THREADS + threadIdx.x; it < nitems; it += (long long)gridDim.x * O4_THREADS) {
        const long long row = it / g.nx;
        const int x = (int)(it - row * g.nx), y = (int)(row % g.ny), z = (int)(row / g.ny);
        const int gz = g.gz0 + z;
        const long long i = lidx(g, z, y, x);
        bool in = x >= 1 && x <= g.nx - 2 && y >= 1 && y <= g.ny - 2;
        if (DIM == 3) in = in && gz >= 1 && gz <= g.gnz - 2;
        if (!in) {
            if (CORR) un[i] = u[i];
            if (SAVE) r[i] = (T)0;
            continue;
        }
        const T uc = val(z, y, x);
        T pz = (T)0;
        if (DIM == 3) pz = axis_p<T>(gz, g.gnz, [&](int k) { return val(k - g.gz0, y, x); });
        const T py = axis_p<T>(y, g.ny, [&](int k) { return val(z, k, x); });
        const T px = axis_p<T>(x, g.nx, [&](int k) { return val(z, y, k); });
        const T res = b[i] - a4_of<T>(c, uc, pz, py, px, DIM == 3);
        acc += (double)res * (double)res;
        if (CORR) un[i] = uc;
        if (SAVE) r[i] = res;
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

template <typename T, int DIM, bool SAVE>
__global__ __launch_bounds__(O4_THREADS) void k_o4_residual(Geom g, O4Coef<T> c, const T *__restrict__ u, const T *__restrict__ b,
                                                            T *__restrict__ r, double *__restrict__ partials)
{
    __shared__ double sh[O4_THREADS / 64];
    o4_plain_body<T, DIM, false, SAVE>(g, c, u, nullptr, b, nullptr, r, partials, sh);
}

template <typename T, int DIM>
__global__ __launch_bounds__(O4_THREADS) void k_o4_correct_residual(Geom g, O4Coef<T> c, const T *__restrict__ u,
                                                                    const T *__restrict__ e, const T *__restrict__ b,
                                                                    T *__restrict__ un, T *__restrict__ r,
                                                                    double *__restrict__ partials)
{
    __shared__ double sh[O4_THREADS / 64];
    o4_plain_body<T, DIM, true, true>(g, c, u, e, b, un, r, partials, sh);
}

// ---------------------------------------------------------------- the marching tile (3-D)
// the lane's vector of u' in the row at element offset `off` (x of its first element: xs); rowin: the row is interior
// in y and z (wave-uniform), so its interior columns are corrected
template <typename T, bool CORR>
__device__ __forceinline__ typename Vec16<T>::type ld_row(const Geom &g, const T *__restrict__ u, const T *__restrict__ e,
                                                          long long off, bool rowin, int xs)
{
    constexpr int V = Vec16<T>::n;
    typedef typename Vec16<T>::type vec;
    vec v = *(const vec *)(u + off);
    if (CORR && rowin) {
        const vec ev = *(const vec *)(e + off);
#pragma unroll
        for (int k = 0; k < V; k++)
            if (xs + k >= 1 && xs + k <= g.nx - 2) v[k] = v[k] + ev[k];
    }
    return v;
}

// one node of u' (the x-closure taps)
template <typename T, bool CORR>
__device__ __forceinline__ T ld_node(const Geom &g, const T *__restrict__ u, const T *__restrict__ e, long long row, bool rowin, int x)
{
    T v = u[row + x];
    if (CORR && rowin && x >= 1 && x <= g.nx - 2) v = v + e[row + x];
    return v;
}

template <typename T, bool CORR, bool SAVE, int RY>
__global__ __launch_bounds__(64 * MBW) void k_o4_march(Geom g, O4Coef<T> c, const T *__restrict__ u, const T *__restrict__ e,
                                                       const T *__restrict__ b, T *__restrict__ un, T *__restrict__ r,
                                                       double *__restrict__ partials, int nbx, int nby, int nbz, int zc)
{
    constexpr int V = Vec16<T>::n;
    typedef typename Vec16<T>::type vec;
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
    const int x0c = min(x0, g.pitch - V);   // clamped for loads: every lane stays active
    const bool xfull = x0 + V <= g.nx;      // the lane's vector lies inside the row
    const int yb = (by * MBW + wv) * RY;
    const int z0 = bz * zc, zend = min(z0 + zc, g.nz);
    // one column left over: the wave that holds the row's last full vector writes it as a full line
    const bool tail1 = g.nx % V == 1 && g.nx > V;
    const bool tailwave = tail1 && (bx * 64 * V <= g.nx - 1 - V) && (g.nx - 1 - V < (bx + 1) * 64 * V);
    const int part = (!tail1 && !xfull && x0 < g.nx) ? g.nx - x0 : 0;   // elements of a partial last vector stored one by one
    const bool edge_l = lane == 0 && x0c > 0, edge_r = lane == 63 && x0c + V < g.pitch;

    // rows yb-2 .. yb+RY+1 (clamped into the plane): the wave's own rows are Y[2 .. RY+1]
    int yoff[RY + 4];   // element offsets of the rows inside a plane
    bool yint[RY + 4];
#pragma unroll
    for (int k = 0; k < RY + 4; k++) {
        const int yc = min(max(yb - 2 + k, 0), g.ny - 1);
        yoff[k] = yc * g.pitch;
        yint[k] = yc >= 1 && yc <= g.ny - 2;
    }
    bool xin[V];   // interior columns this lane owns (none for a clamped lane)
#pragma unroll
    for (int k = 0; k < V; k++) xin[k] = x0 + k >= 1 && x0 + k <= g.nx - 2;
    bool has1 = false, hasn = false;   // the lane owns column 1 / column nx-2
#pragma unroll
    for (int k = 0; k < V; k++) { has1 |= x0 + k == 1; hasn |= x0 + k == g.nx - 2; }

    auto zcl = [&](int z) { return min(max(z, 0), g.nz - 1); };
    auto zin = [&](int z) { return g.gz0 + z >= 1 && g.gz0 + z <= g.gnz - 2; };
    // the wave's row k (index into yoff) of local plane z (clamped)
    auto row_of = [&](int z, int k) -> vec {
        const int zz = zcl(z);
        return ld_row<T, CORR>(g, u, e, (long long)zz * g.plane + yoff[k] + x0c, zin(zz) && yint[k], x0c);
    };

    vec m2[RY], m1[RY], cc[RY], p1[RY], p2[RY];
#pragma unroll
    for (int q = 0; q < RY; q++) {
        m1[q] = row_of(z0 - 2, q + 2);   // rotated into m2 below
        cc[q] = row_of(z0 - 1, q + 2);
        p1[q] = row_of(z0, q + 2);
        p2[q] = row_of(z0 + 1, q + 2);
    }
    double acc = 0.;
    for (int z = z0; z < zend; z++) {
        const long long zo = (long long)z * g.plane;
        const int gz = g.gz0 + z;
        const bool zi = zin(z);
#pragma unroll
        for (int q = 0; q < RY; q++) {
            m2[q] = m1[q]; m1[q] = cc[q]; cc[q] = p1[q]; p1[q] = p2[q];
            p2[q] = row_of(z + 2, q + 2);
        }
        // the plane's rows yb-2 .. yb+RY+1
        vec Y[RY + 4];
        Y[0] = row_of(z, 0);
        Y[1] = row_of(z, 1);
#pragma unroll
        for (int q = 0; q < RY; q++) Y[q + 2] = cc[q];
        Y[RY + 2] = row_of(z, RY + 2);
        Y[RY + 3] = row_of(z, RY + 3);
#pragma unroll
        for (int q = 0; q < RY; q++) {
            const int y = yb + q;
            if (y >= g.ny) continue;   // wave-uniform
            const long long ro = zo + yoff[q + 2];   // the row's first element
            const bool ri = zi && yint[q + 2];
            vec res = (vec)(0);
            if (ri) {   // wave-uniform: an interior row of an interior plane
                const vec bv = __builtin_nontemporal_load((const vec *)(b + ro + x0c));
                // z
                vec pz;
                if (gz == 1 || gz == g.gnz - 2) {
                    const bool lo = gz == 1;
                    const int za = lo ? 4 - g.gz0 : g.gnz - 5 - g.gz0, zb = lo ? 5 - g.gz0 : g.gnz - 6 - g.gz0;
                    const vec u0 = lo ? m1[q] : p1[q], u2 = lo ? p1[q] : m1[q], u3 = lo ? p2[q] : m2[q];
                    const vec u4 = row_of(za, q + 2), u5 = row_of(zb, q + 2);
#pragma unroll
                    for (int k = 0; k < V; k++) pz[k] = p_end<T>(u0[k], cc[q][k], u2[k], u3[k], u4[k], u5[k]);
                } else {
#pragma unroll
                    for (int k = 0; k < V; k++) pz[k] = p_mid<T>(m2[q][k], m1[q][k], cc[q][k], p1[q][k], p2[q][k]);
                }
                // y
                vec py;
                if (y == 1 || y == g.ny - 2) {
                    const int s = y == 1 ? 1 : -1, ya = y == 1 ? 0 : g.ny - 1;
                    vec t[6];
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        const int yy = ya + s * j;
                        t[j] = ld_row<T, CORR>(g, u, e, zo + (long long)yy * g.pitch + x0c, yy >= 1 && yy <= g.ny - 2, x0c);
                    }
#pragma unroll
                    for (int k = 0; k < V; k++) py[k] = p_end<T>(t[0][k], t[1][k], t[2][k], t[3][k], t[4][k], t[5][k]);
                } else {
#pragma unroll
                    for (int k = 0; k < V; k++) py[k] = p_mid<T>(Y[q][k], Y[q + 1][k], Y[q + 2][k], Y[q + 3][k], Y[q + 4][k]);
                }
                // x: the window x0-2 .. x0+V+1 from the neighbouring lanes' vectors
                T w[V + 4];
                {
                    vec el = (vec)(0), er = (vec)(0);
                    if (edge_l) el = ld_row<T, CORR>(g, u, e, ro + x0c - V, true, x0c - V);
                    if (edge_r) er = ld_row<T, CORR>(g, u, e, ro + x0c + V, true, x0c + V);
                    w[0] = lane_from_prev(cc[q][V - 2], el[V - 2]);
                    w[1] = lane_from_prev(cc[q][V - 1], el[V - 1]);
#pragma unroll
                    for (int k = 0; k < V; k++) w[k + 2] = cc[q][k];
                    w[V + 2] = lane_from_next(cc[q][0], er[0]);
                    w[V + 3] = lane_from_next(cc[q][1], er[1]);
                }
                vec px;
#pragma unroll
                for (int k = 0; k < V; k++) px[k] = p_mid<T>(w[k], w[k + 1], w[k + 2], w[k + 3], w[k + 4]);
                if (has1 || hasn) {   // the two x-closure columns: the only per-lane branch
                    T pe1 = (T)0, pen = (T)0;
                    if (has1)
                        pe1 = p_end<T>(ld_node<T, CORR>(g, u, e, ro, true, 0), ld_node<T, CORR>(g, u, e, ro, true, 1),
                                       ld_node<T, CORR>(g, u, e, ro, true, 2), ld_node<T, CORR>(g, u, e, ro, true, 3),
                                       ld_node<T, CORR>(g, u, e, ro, true, 4), ld_node<T, CORR>(g, u, e, ro, true, 5));
                    if (hasn)
                        pen = p_end<T>(ld_node<T, CORR>(g, u, e, ro, true, g.nx - 1), ld_node<T, CORR>(g, u, e, ro, true, g.nx - 2),
                                       ld_node<T, CORR>(g, u, e, ro, true, g.nx - 3), ld_node<T, CORR>(g, u, e, ro, true, g.nx - 4),
                                       ld_node<T, CORR>(g, u, e, ro, true, g.nx - 5), ld_node<T, CORR>(g, u, e, ro, true, g.nx - 6));
#pragma unroll
                    for (int k = 0; k < V; k++) {
                        if (x0 + k == 1) px[k] = pe1;
                        if (x0 + k == g.nx - 2) px[k] = pen;
                    }
                }
#pragma unroll
                for (int k = 0; k < V; k++) {
                    const T t = bv[k] - a4_of<T>(c, cc[q][k], pz[k], py[k], px[k], true);
                    res[k] = xin[k] ? t : (T)0;
                    acc += xin[k] ? (double)t * (double)t : 0.;
                }
            }
            // stores: r (SAVE) and u' (CORR); the same shape for both
            if (xfull) {
                if (SAVE) __builtin_nontemporal_store(res, (vec *)(r + ro + x0c));
                if (CORR) __builtin_nontemporal_store(cc[q], (vec *)(un + ro + x0c));
            } else if (part) {
#pragma unroll
                for (int k = 0; k < V; k++)
                    if (k < part) {
                        if (SAVE) r[ro + x0c + k] = res[k];
                        if (CORR) un[ro + x0c + k] = cc[q][k];
                    }
            }
            if (tailwave && lane >= 56) {
                // column nx-1 (Dirichlet: r = 0, u' = u) as one full 128-byte line: value + zero padding
                const int j = lane - 56;
                constexpr int LINE = 128 / (int)sizeof(T);
                const int xs = g.nx - 1 + V * j;
                const int line_end = ((g.nx - 1) / LINE + 1) * LINE;
                if (xs < line_end) {
                    vec tv = (vec)(0);
                    if (SAVE) __builtin_nontemporal_store(tv, (vec *)(r + ro + xs));
                    if (CORR) {
                        if (j == 0) tv[0] = u[ro + g.nx - 1];
                        __builtin_nontemporal_store(tv, (vec *)(un + ro + xs));
                    }
                }
            }
        }
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

struct MarchGrid { int nbx, nby, nbz, zc, grid; };

template <typename T>
MarchGrid march_grid(const Geom &g, int ry)
{
    constexpr int V = Vec16<T>::n;
    // vectors a row needs lanes for: the full ones, and a partial last one unless it is the single tail column
    const int nvec = std::max(1, g.nx / V + (g.nx % V > 1 ? 1 : 0));
    MarchGrid m;
    m.nbx = (nvec + 63) / 64;
    m.nby = (g.ny + ry * MBW - 1) / (ry * MBW);
    // a chunk of zc planes loads zc + 4: long chunks while they still fill the chip, never shorter than 4
    m.zc = 16;
    while (m.zc > 4 && (long long)m.nbx * m.nby * ((g.nz + m.zc - 1) / m.zc) < 2048) m.zc >>= 1;
    m.nbz = (g.nz + m.zc - 1) / m.zc;
    m.grid = ((m.nbx * m.nby * m.nbz + 7) / 8) * 8;
    return m;
}

template <typename T>
O4Coef<T> o4_coef(const double w[3], double sigma) { return O4Coef<T>{(T)w[0], (T)w[1], (T)w[2], (T)sigma}; }

int plain_grid(const Geom &g, int cap)
{
    const long long items = (long long)g.nx * g.ny * g.nz;
    const long long nb = std::min<long long>(O4_MAX_BLOCKS, (items + O4_THREADS - 1) / O4_THREADS);
    return (int)std::max<long long>(1, std::min<long long>(nb, cap));
}

// the marching tile takes the level (whole levels only: mg_o4_* refuse distributed handles before they get here)
template <typename T>
bool march_takes(const Geom &g)
{
    return o4_march_ok(g.dim, g.nx, g.ny, g.nz, (int)sizeof(T)) && g.gz0 == 0 && g.gnz == g.nz;
}

}  // namespace

template <typename T>
int launch_o4_residual(hipStream_t s, const Geom &g, const double w[3], double sigma, const T *u, const T *b, T *r,
                       double *partials, int cap)
{
    const O4Coef<T> c = o4_coef<T>(w, sigma);
    if (march_takes<T>(g)) {
        const MarchGrid m = march_grid<T>(g, RY_RES);
        assert(m.grid <= cap);   // d_partials_ holds one sum per 64 x 4 nodes of a plane: far more than the tile's workgroups
        const dim3 gr(m.grid), bl(64 * MBW);
        if (r) hipLaunchKernelGGL((k_o4_march<T, false, true, RY_RES>), gr, bl, 0, s, g, c, u, (const T *)nullptr, b, (T *)nullptr, r, partials, m.nbx, m.nby, m.nbz, m.zc);
        else hipLaunchKernelGGL((k_o4_march<T, false, false, RY_RES>), gr, bl, 0, s, g, c, u, (const T *)nullptr, b, (T *)nullptr, r, partials, m.nbx, m.nby, m.nbz, m.zc);
        return m.grid;
    }
    const int nb = plain_grid(g, cap);
    const dim3 gr(nb), bl(O4_THREADS);
#define MG_O4(DIM, SAVE) hipLaunchKernelGGL((k_o4_residual<T, DIM, SAVE>), gr, bl, 0, s, g, c, u, b, r, partials)
    if (g.dim == 3) { if (r) MG_O4(3, true); else MG_O4(3, false); }
    else { if (r) MG_O4(2, true); else MG_O4(2, false); }
#undef MG_O4
    return nb;
}

template <typename T>
int launch_o4_correct_residual(hipStream_t s, const Geom &g, const double w[3], double sigma, const T *u, const T *e, const T *b,
                               T *u_out, T *r, double *partials, int cap)
{
    const O4Coef<T> c = o4_coef<T>(w, sigma);
    if (march_takes<T>(g)) {
        const MarchGrid m = march_grid<T>(g, RY_CORR);
        assert(m.grid <= cap);
        hipLaunchKernelGGL((k_o4_march<T, true, true, RY_CORR>), dim3(m.grid), dim3(64 * MBW), 0, s, g, c, u, e, b, u_out, r, partials, m.nbx,
                           m.nby, m.nbz, m.zc);
        return m.grid;
    }
    const int nb = plain_grid(g, cap);
    if (g.dim == 3) hipLaunchKernelGGL((k_o4_correct_residual<T, 3>), dim3(nb), dim3(O4_THREADS), 0, s, g, c, u, e, b, u_out, r, partials);
    else hipLaunchKernelGGL((k_o4_correct_residual<T, 2>), dim3(nb), dim3(O4_THREADS), 0, s, g, c, u, e, b, u_out, r, partials);
    return nb;
}

template int launch_o4_residual<double>(hipStream_t, const Geom &, const double[3], double, const double *, const double *, double *, double *, int);
template int launch_o4_residual<float>(hipStream_t, const Geom &, const double[3], double, const float *, const float *, float *, double *, int);
template int launch_o4_correct_residual<double>(hipStream_t, const Geom &, const double[3], double, const double *, const double *,
                                                const double *, double *, double *, double *, int);
template int launch_o4_correct_residual<float>(hipStream_t, const Geom &, const double[3], double, const float *, const float *,
                                               const float *, float *, float *, double *, int);

}  // namespace mg
