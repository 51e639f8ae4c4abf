// mg_fmg.hip -- the full-multigrid (nested iteration) interpolation fine = Pi coarse, gfx950 (extension, no reference
// counterpart; driven by Solver::fmg_t and mg_fmg_prolong).
//
// Pi is the tensor product, over the coarsened axes, of the 1-D rule on a coarse row c[0..nc-1], fine row f[0..2nc-2]:
//     f[2m]   = c[m]
//     f[2m+1] = (-c[m-1] + 9 c[m] + 9 c[m+1] - c[m+2]) / 16          1 <= m <= nc-3   (cubic)
//     f[1]    = (3 c[0] + 6 c[1] - c[2]) / 8, and its mirror at the other end            (one-sided quadratic)
// Axes a transition keeps (z of a semi-coarsened transition, z in 2-D) are copied. Fine Dirichlet nodes take bnd[node]
// in the same launch when bnd != nullptr. Every weight is a small integer over a power of two, so fp32 and fp64 are the
// same formula; rule() below is the ONE evaluation of it: ((wb b + wc c) - (a + d)) * 2^-k, operands that a one-sided
// rule does not use replaced by 0. The library is built with -ffp-contract=off, so this is five roundings at most,
// three deep (product, sum, difference; the scaling is exact), and both kernels below, which apply it along x first,
// then y, then z, give the same bits.
//
// With a face mask (enum mg_face; mg_fmg / mg_fmg_prolong with MG_FMG_OPERATOR) the faces in it are
// Neumann faces: per coarsened axis the coarse row is extended by its mirror image at such an end, c[-1] = c[1] and
// c[nc] = c[nc-2], and the odd node next to that end takes the CUBIC rule on the extended row; the one-sided rule stays at
// an end whose face is Dirichlet. The nodes of a Neumann face are interpolated like every other unknown, and bnd goes to
// the fine nodes on at least one face that is NOT in the mask. In both kernels the mirror is an index select where the
// mask-free form clamps the index, and a template flag (MIR): the mask-free instantiations are the code they were.
//
// k_fmg_prolong      one thread per fine point gathering its <= 4 x 4 x 4 coarse points: every shape the library admits
//                    (2-D, semi-coarsened, n = 3 coarse grids). Issue-bound; it runs the small levels.
// k_fmg_prolong3d    the streaming form for whole 3-D levels (257^3 -> 513^3 fp64 reads 0.136 GB and writes 1.08 GB).
//                    Lane <-> CV coarse columns = one aligned 16-byte vector of fine x, wave <-> coarse row, the
//                    workgroup marches coarse planes. Per coarse plane every wave loads ONE coarse row (its own CV
//                    columns and the three neighbours the rule needs, clamped at the row ends), applies the x rule in
//                    registers (the next plane's row is requested before that, one step ahead) and leaves the 16-byte
//                    fine-x vector in LDS; after one barrier the waves that own a coarse row read four of those
//                    vectors (rows m-1 .. m+2) and apply the y rule; the z rule runs on a
//                    register window of the last four planes. FMG_W staged rows feed FMG_W - 3 owned ones and a
//                    workgroup marching FMG_ZC planes reads FMG_ZC + 3, so the coarse array (an eighth of the traffic)
//                    is read (8/5)(19/16) = 1.9 times, mostly out of L2; the fine array is written once with whole
//                    16-byte non-temporal vectors and the odd last column as one full 128-byte line (mg_jacobi_fast.hip).

#include "mg_kernels.h"
#include "mg_device.h"

namespace mg {
namespace {

// which rule the odd fine node between coarse nodes m and m+1 of a row of nc takes
enum { RULE_CUBIC = 0, RULE_LEFT = 1, RULE_RIGHT = 2 };
__device__ __forceinline__ int rule_kind(int m, int nc) { return m == 0 ? RULE_LEFT : (m >= nc - 2 ? RULE_RIGHT : RULE_CUBIC); }
// ... with lo / hi = the row's end is mirrored (its face is in the mask): cubic there
__device__ __forceinline__ int rule_kind(int m, int nc, bool lo, bool hi)
{
    return m == 0 ? (lo ? RULE_CUBIC : RULE_LEFT) : (m >= nc - 2 ? (hi ? RULE_CUBIC : RULE_RIGHT) : RULE_CUBIC);
}
// node j in -1 .. of a row of nc as an index into the row: the mirror image at a mirrored end, else clamped (a node the
// one-sided rule ignores); always inside [0, nc-1]
__device__ __forceinline__ int row_index(int j, int nc, bool lo, bool hi)
{
    return j < 0 ? (lo ? 1 : 0) : (j > nc - 1 ? (hi && j == nc ? nc - 2 : nc - 1) : j);
}
// the bits of the two faces of an axis
enum { FACE_XLO = 1, FACE_XHI = 2, FACE_YLO = 4, FACE_YHI = 8, FACE_ZLO = 16, FACE_ZHI = 32 };

// a, b, c, d = c[m-1], c[m], c[m+1], c[m+2] (a / d: any finite-or-not value where the one-sided rule has no such node)
template <typename T>
__device__ __forceinline__ T rule(T a, T b, T c, T d, int kind)
{
    const T wb = kind == RULE_LEFT ? (T)3 : (kind == RULE_RIGHT ? (T)6 : (T)9);
    const T wc = kind == RULE_LEFT ? (T)6 : (kind == RULE_RIGHT ? (T)3 : (T)9);
    const T aa = kind == RULE_LEFT ? (T)0 : a;
    const T dd = kind == RULE_RIGHT ? (T)0 : d;
    const T sc = kind == RULE_CUBIC ? (T)0.0625 : (T)0.125;
    return ((wb * b + wc * c) - (aa + dd)) * sc;
}

// ------------------------------------------------------------------------------------------ generic gather
// value of the x pass at fine column x of one coarse row
template <typename T, bool MIR>
__device__ __forceinline__ T gather_x(const T *__restrict__ row, int x, int ncx, int mask)
{
    const int m = x >> 1;
    if (!(x & 1)) return row[m];
    if (!MIR) return rule<T>(row[max(m - 1, 0)], row[m], row[m + 1], row[min(m + 2, ncx - 1)], rule_kind(m, ncx));
    const bool lo = mask & FACE_XLO, hi = mask & FACE_XHI;
    return rule<T>(row[row_index(m - 1, ncx, lo, hi)], row[m], row[m + 1], row[row_index(m + 2, ncx, lo, hi)], rule_kind(m, ncx, lo, hi));
}
// ... of the x and y passes at fine (y, x) of one coarse plane
template <typename T, bool MIR>
__device__ __forceinline__ T gather_yx(const T *__restrict__ pl, const Geom &gc, int y, int x, int mask)
{
    const int m = y >> 1;
    if (!(y & 1)) return gather_x<T, MIR>(pl + (long long)m * gc.pitch, x, gc.nx, mask);
    const bool lo = MIR && (mask & FACE_YLO), hi = MIR && (mask & FACE_YHI);
    const int ia = MIR ? row_index(m - 1, gc.ny, lo, hi) : max(m - 1, 0), id = MIR ? row_index(m + 2, gc.ny, lo, hi) : min(m + 2, gc.ny - 1);
    const T a = gather_x<T, MIR>(pl + (long long)ia * gc.pitch, x, gc.nx, mask);
    const T b = gather_x<T, MIR>(pl + (long long)m * gc.pitch, x, gc.nx, mask);
    const T c = gather_x<T, MIR>(pl + (long long)(m + 1) * gc.pitch, x, gc.nx, mask);
    const T d = gather_x<T, MIR>(pl + (long long)id * gc.pitch, x, gc.nx, mask);
    return rule<T>(a, b, c, d, MIR ? rule_kind(m, gc.ny, lo, hi) : rule_kind(m, gc.ny));
}

constexpr int GBX = 64, GBY = 4;

// ZPASS: the transition coarsens z (3-D, not semi-coarsened); otherwise fine plane z <-> coarse plane z
// MIR: mask names the Neumann faces (otherwise it is not read)
template <typename T, bool ZPASS, bool MIR>
__global__ __launch_bounds__(GBX *GBY) void k_fmg_prolong(Geom gc, Geom gf, const T *__restrict__ coarse, T *__restrict__ fine,
                                                          const T *__restrict__ bnd, int mask)
{
    const int x = blockIdx.x * GBX + threadIdx.x, y = blockIdx.y * GBY + threadIdx.y, z = blockIdx.z;
    if (x >= gf.nx || y >= gf.ny) return;
    const long long i = (long long)z * gf.plane + (long long)y * gf.pitch + x;
    if (!MIR) {
        const bool zb = gf.dim == 3 && (z == 0 || z == gf.nz - 1);
        if (bnd && (zb || y == 0 || y == gf.ny - 1 || x == 0 || x == gf.nx - 1)) { fine[i] = bnd[i]; return; }
    } else if (bnd) {   // a node on at least one face that is not in the mask
        const int on = (x == 0 ? FACE_XLO : 0) | (x == gf.nx - 1 ? FACE_XHI : 0) | (y == 0 ? FACE_YLO : 0) | (y == gf.ny - 1 ? FACE_YHI : 0) |
                       (gf.dim == 3 && z == 0 ? FACE_ZLO : 0) | (gf.dim == 3 && z == gf.nz - 1 ? FACE_ZHI : 0);
        if (on & ~mask) { fine[i] = bnd[i]; return; }
    }
    T v;
    if (!ZPASS) v = gather_yx<T, MIR>(coarse + (long long)z * gc.plane, gc, y, x, mask);
    else {
        const int m = z >> 1;
        if (!(z & 1)) v = gather_yx<T, MIR>(coarse + (long long)m * gc.plane, gc, y, x, mask);
        else {
            const bool lo = MIR && (mask & FACE_ZLO), hi = MIR && (mask & FACE_ZHI);
            const int ia = MIR ? row_index(m - 1, gc.nz, lo, hi) : max(m - 1, 0), id = MIR ? row_index(m + 2, gc.nz, lo, hi) : min(m + 2, gc.nz - 1);
            const T a = gather_yx<T, MIR>(coarse + (long long)ia * gc.plane, gc, y, x, mask);
            const T b = gather_yx<T, MIR>(coarse + (long long)m * gc.plane, gc, y, x, mask);
            const T c = gather_yx<T, MIR>(coarse + (long long)(m + 1) * gc.plane, gc, y, x, mask);
            const T d = gather_yx<T, MIR>(coarse + (long long)id * gc.plane, gc, y, x, mask);
            v = rule<T>(a, b, c, d, MIR ? rule_kind(m, gc.nz, lo, hi) : rule_kind(m, gc.nz));
        }
    }
    fine[i] = v;
}

// ------------------------------------------------------------------------------------------ streaming 3-D form
constexpr int FMG_W = 8;           // waves per workgroup = coarse rows staged per plane
constexpr int FMG_R = FMG_W - 3;   // coarse rows a workgroup owns (rows m-1 .. m+2 feed row m)
constexpr int FMG_ZC = 16;         // coarse planes a workgroup marches

template <typename T, typename vec, int V>
__device__ __forceinline__ vec rule_vec(vec a, vec b, vec c, vec d, int kind)
{
    vec r;
#pragma unroll
    for (int e = 0; e < V; e++) r[e] = rule<T>(a[e], b[e], c[e], d[e], kind);
    return r;
}

// one fine row: v = the lane's vector, tailv = the odd last column (the same value in every lane)
// MIR: bnd goes to the nodes on a face that is not in the mask -- the whole row when that face is a y or z face
template <typename T, bool BND, bool MIR>
__device__ __forceinline__ void store_row(const Geom &gf, T *__restrict__ fine, const T *__restrict__ bnd, int zf, int yf, int x0,
                                          bool xin, bool tailwave, int lane, typename Vec16<T>::type v, T tailv, int mask)
{
    constexpr int V = Vec16<T>::n;
    typedef typename Vec16<T>::type vec;
    const long long fo = (long long)zf * gf.plane + (long long)yf * gf.pitch;
    if (BND && !MIR) {
        const bool rowb = zf == 0 || zf == gf.nz - 1 || yf == 0 || yf == gf.ny - 1;   // wave-uniform
        if (rowb) { if (xin) v = *(const vec *)(bnd + fo + x0); }
        else if (x0 == 0) v[0] = bnd[fo];
        tailv = bnd[fo + gf.nx - 1];   // the last column is a Dirichlet column
    }
    if (BND && MIR) {
        const int on = (zf == 0 ? FACE_ZLO : 0) | (zf == gf.nz - 1 ? FACE_ZHI : 0) | (yf == 0 ? FACE_YLO : 0) | (yf == gf.ny - 1 ? FACE_YHI : 0);
        const bool rowb = (on & ~mask) != 0;   // wave-uniform
        if (rowb) { if (xin) v = *(const vec *)(bnd + fo + x0); }
        else if (x0 == 0 && !(mask & FACE_XLO)) v[0] = bnd[fo];
        if (rowb || !(mask & FACE_XHI)) tailv = bnd[fo + gf.nx - 1];
    }
    if (xin) __builtin_nontemporal_store(v, (vec *)(fine + fo + x0));
    if (tailwave && lane >= 56) {
        const int j = lane - 56;
        constexpr int LINE = 128 / (int)sizeof(T);
        const int xs = gf.nx - 1 + V * j;
        const int line_end = ((gf.nx - 1) / LINE + 1) * LINE;   // <= pitch: the padding columns get the zeros they hold
        if (xs < line_end) {
            vec tv = (vec)(0);
            if (j == 0) tv[0] = tailv;
            __builtin_nontemporal_store(tv, (vec *)(fine + fo + xs));
        }
    }
}

// SEMI: the transition keeps z: fine plane z <-> coarse plane z, no z pass
// MIR: mask names the Neumann faces (otherwise it is not read): the mirror is an index select before the load -- col[] for
// x, the staged row yl for y, the plane index for z -- and the rule at a mirrored end is the cubic one
template <typename T, bool SEMI, bool BND, bool MIR>
__global__ __launch_bounds__(64 * FMG_W) void k_fmg_prolong3d(Geom gc, Geom gf, const T *__restrict__ coarse, T *__restrict__ fine,
                                                              const T *__restrict__ bnd, int nbx, int mask)
{
    constexpr int V = Vec16<T>::n, CV = V / 2;
    typedef typename Vec16<T>::type vec;
    __shared__ vec sx[2][FMG_W][64];   // x-passed rows of the plane being staged, double-buffered: one barrier per plane
    __shared__ T st[2][FMG_W];         // their last coarse column (the odd last fine column)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
    const int ncx = gc.nx;
    const bool xlo = MIR && (mask & FACE_XLO), xhi = MIR && (mask & FACE_XHI), ylo = MIR && (mask & FACE_YLO), yhi = MIR && (mask & FACE_YHI);
    const bool zlo = MIR && (mask & FACE_ZLO), zhi = MIR && (mask & FACE_ZHI);
    const int ic0 = CV * (bx * 64 + lane);   // first coarse column of the lane
    const int x0 = 2 * ic0;                  // first fine x
    const bool xin = x0 < V * (gf.nx / V);
    const bool tailwave = (bx * 64 * V <= gf.nx - 1 - V) && (gf.nx - 1 - V < (bx + 1) * 64 * V);
    // staged row of this wave, and the coarse row it owns (waves FMG_R .. FMG_W-1 only stage)
    const int yl = MIR ? row_index(by * FMG_R - 1 + wv, gc.ny, ylo, yhi) : min(max(by * FMG_R - 1 + wv, 0), gc.ny - 1);
    const int my = by * FMG_R + wv;
    const bool owner = wv < FMG_R && my < gc.ny;
    const bool odd_y = my <= gc.ny - 2;
    const int ky = MIR ? rule_kind(my, gc.ny, ylo, yhi) : rule_kind(my, gc.ny);
    const int zc0 = blockIdx.y * FMG_ZC, zc1 = min(zc0 + FMG_ZC, gc.nz);   // owned coarse planes [zc0, zc1)
    const int p0 = SEMI ? zc0 : zc0 - 1, p1 = SEMI ? zc1 - 1 : zc1 + 1;
    // columns ic0-1 .. ic0+CV+1 clamped into the row (lanes past the row end compute values nobody stores)
    int col[CV + 3], kx[CV];
#pragma unroll
    for (int m = 0; m < CV + 3; m++) col[m] = MIR ? row_index(ic0 - 1 + m, ncx, xlo, xhi) : min(max(ic0 - 1 + m, 0), ncx - 1);
#pragma unroll
    for (int m = 0; m < CV; m++) kx[m] = MIR ? rule_kind(min(ic0 + m, ncx - 2), ncx, xlo, xhi) : rule_kind(min(ic0 + m, ncx - 2), ncx);
    // coarse plane p (-1 .. nz) as a plane of the array
    auto plane_of = [&](int p) { return MIR ? row_index(p, gc.nz, zlo, zhi) : min(max(p, 0), gc.nz - 1); };
    const long long rowoff = (long long)yl * gc.pitch;

    vec wE[4], wO[4];
    T tE[4], tO[4];
#pragma unroll
    for (int q = 0; q < 4; q++) { wE[q] = (vec)(0); wO[q] = (vec)(0); tE[q] = 0; tO[q] = 0; }

    // the row of plane p is requested one step ahead (before the previous step's barrier), so that a step does not
    // begin with a memory round trip
    T nv[CV + 3], ntl;
    {
        const T *__restrict__ row = coarse + (long long)plane_of(p0) * gc.plane + rowoff;
#pragma unroll
        for (int m = 0; m < CV + 3; m++) nv[m] = row[col[m]];
        ntl = row[ncx - 1];
    }
    int buf = 0;
    for (int p = p0; p <= p1; p++, buf ^= 1) {
        T cv[CV + 3];
#pragma unroll
        for (int m = 0; m < CV + 3; m++) cv[m] = nv[m];
        const T tl = ntl;
        if (p < p1) {
            const T *__restrict__ row = coarse + (long long)plane_of(p + 1) * gc.plane + rowoff;
#pragma unroll
            for (int m = 0; m < CV + 3; m++) nv[m] = row[col[m]];
            ntl = row[ncx - 1];
        }
        vec X;
#pragma unroll
        for (int m = 0; m < CV; m++) {
            X[2 * m] = cv[m + 1];
            X[2 * m + 1] = rule<T>(cv[m], cv[m + 1], cv[m + 2], cv[m + 3], kx[m]);
        }
        sx[buf][wv][lane] = X;
        if (lane == 0) st[buf][wv] = tl;
        __syncthreads();
        if (!owner) continue;   // wave-uniform; the barrier count is the same for every wave (p0, p1 are block-uniform)
        const vec a = sx[buf][wv][lane], b = sx[buf][wv + 1][lane], c = sx[buf][wv + 2][lane], d = sx[buf][wv + 3][lane];
        const vec Ye = b, Yo = rule_vec<T, vec, V>(a, b, c, d, ky);
        const T Te = st[buf][wv + 1], To = rule<T>(st[buf][wv], st[buf][wv + 1], st[buf][wv + 2], st[buf][wv + 3], ky);
        if (SEMI) {
            store_row<T, BND, MIR>(gf, fine, bnd, p, 2 * my, x0, xin, tailwave, lane, Ye, Te, mask);
            if (odd_y) store_row<T, BND, MIR>(gf, fine, bnd, p, 2 * my + 1, x0, xin, tailwave, lane, Yo, To, mask);
            continue;
        }
#pragma unroll
        for (int q = 0; q < 3; q++) { wE[q] = wE[q + 1]; wO[q] = wO[q + 1]; tE[q] = tE[q + 1]; tO[q] = tO[q + 1]; }
        wE[3] = Ye; wO[3] = Yo; tE[3] = Te; tO[3] = To;
        const int mz = p - 2;   // the window holds coarse planes mz-1 .. mz+2 (at the ends: clamped copies, which the rule ignores, or mirror images)
        if (mz < zc0) continue;
        store_row<T, BND, MIR>(gf, fine, bnd, 2 * mz, 2 * my, x0, xin, tailwave, lane, wE[1], tE[1], mask);
        if (odd_y) store_row<T, BND, MIR>(gf, fine, bnd, 2 * mz, 2 * my + 1, x0, xin, tailwave, lane, wO[1], tO[1], mask);
        if (mz <= gc.nz - 2) {
            const int kz = MIR ? rule_kind(mz, gc.nz, zlo, zhi) : rule_kind(mz, gc.nz);
            store_row<T, BND, MIR>(gf, fine, bnd, 2 * mz + 1, 2 * my, x0, xin, tailwave, lane,
                              rule_vec<T, vec, V>(wE[0], wE[1], wE[2], wE[3], kz), rule<T>(tE[0], tE[1], tE[2], tE[3], kz), mask);
            if (odd_y)
                store_row<T, BND, MIR>(gf, fine, bnd, 2 * mz + 1, 2 * my + 1, x0, xin, tailwave, lane,
                                  rule_vec<T, vec, V>(wO[0], wO[1], wO[2], wO[3], kz), rule<T>(tO[0], tO[1], tO[2], tO[3], kz), mask);
        }
    }
}

}  // namespace

// whole (undistributed) 3-D levels whose rows are at least a quarter wave wide; MG_FMG_FAST=0 sends everything to the
// gather kernel (the two give the same bits; tools and tests use it to compare them)
template <typename T>
bool fmg_prolong_fast_ok(const Geom &gc, const Geom &gf)
{
    constexpr int V = Vec16<T>::n;
    if (!switches().fmg_fast) return false;
    if (!(gf.dim == 3 && gc.dim == 3 && gf.nx == 2 * gc.nx - 1 && gf.ny == 2 * gc.ny - 1 && gc.nx >= 17 && gc.ny >= 3 && (gf.nx % V) == 1)) return false;
    if (gf.gz0 != 0 || gc.gz0 != 0 || gf.gnz != gf.nz || gc.gnz != gc.nz) return false;
    return is_semi_transition(gf, gc) ? gf.nz == gc.nz : (gf.nz == 2 * gc.nz - 1 && gc.nz >= 3);
}

template <typename T>
void launch_fmg_prolong(hipStream_t s, const Geom &gc, const Geom &gf, const T *coarse, T *fine, const T *bnd, int mask)
{
    const bool semi = is_semi_transition(gf, gc);
    if (fmg_prolong_fast_ok<T>(gc, gf)) {
        constexpr int CV = Vec16<T>::n / 2;
        const int nbx = (gc.nx - 1 + 64 * CV - 1) / (64 * CV);   // lanes cover coarse columns 0 .. nc-2 (the last one only feeds the tail)
        const int nby = (gc.ny + FMG_R - 1) / FMG_R;
        const dim3 gr(nbx * nby, (gc.nz + FMG_ZC - 1) / FMG_ZC), bl(64 * FMG_W);
#define MG_FMG(SEMI, BND, MIR) hipLaunchKernelGGL((k_fmg_prolong3d<T, SEMI, BND, MIR>), gr, bl, 0, s, gc, gf, coarse, fine, bnd, nbx, mask)
#define MG_FMG_B(SEMI, MIR) do { if (bnd) MG_FMG(SEMI, true, MIR); else MG_FMG(SEMI, false, MIR); } while (0)
        if (mask) { if (semi) MG_FMG_B(true, true); else MG_FMG_B(false, true); }
        else { if (semi) MG_FMG_B(true, false); else MG_FMG_B(false, false); }
#undef MG_FMG_B
#undef MG_FMG
        return;
    }
    const dim3 gr((gf.nx + GBX - 1) / GBX, (gf.ny + GBY - 1) / GBY, gf.nz), bl(GBX, GBY, 1);
    const bool zpass = gf.dim == 3 && !semi;
#define MG_FMG(ZPASS, MIR) hipLaunchKernelGGL((k_fmg_prolong<T, ZPASS, MIR>), gr, bl, 0, s, gc, gf, coarse, fine, bnd, mask)
    if (mask) { if (zpass) MG_FMG(true, true); else MG_FMG(false, true); }
    else { if (zpass) MG_FMG(true, false); else MG_FMG(false, false); }
#undef MG_FMG
}

template bool fmg_prolong_fast_ok<double>(const Geom &, const Geom &);
template bool fmg_prolong_fast_ok<float>(const Geom &, const Geom &);
template void launch_fmg_prolong<double>(hipStream_t, const Geom &, const Geom &, const double *, double *, const double *, int);
template void launch_fmg_prolong<float>(hipStream_t, const Geom &, const Geom &, const float *, float *, const float *, int);

}  // namespace mg
