// mg_eig.hip -- level-0 block kernels of the multigrid-preconditioned LOBPCG eigensolver (mg_eig_solve, include/mg_hip.h;
// driver: Solver::eig_t in mg_drivers.cpp).
//
// Besides its preconditioning cycles, a LOBPCG iteration on a block of m columns is two kinds of pass over level 0:
//   k_eig_gram     one TILE of the two Gram matrices G = S^T S, H = S^T (A S) of the basis S = [X, W, P]: up to GRAM_ROWS
//                  row vectors against up to GRAM_COLS column vectors b with their images A b. With APPLY the images are
//                  not read but made at the node -- AW = A W in the row order of k_cg_direction_apply, W := 0 on Dirichlet
//                  nodes -- and written out, so the apply costs the pass no extra read of W beyond the stencil's neighbours.
//   k_eig_combine  X' = S Cx, AX' = AS Cx, P' = [W, P] Cp, AP' = [AW, AP] Cp in place, the residual R = AX' - theta X' into
//                  the W family and the sums of R^2, all in one pass: every family is read once and written once.
// and k_eig_reduce adds the per-workgroup partial sums of either in a fixed order (no atomics: two runs give the same bits).
//
// Tiling of the Gram pass. The full pair of 24 x 24 matrices would need 2 * 300 double accumulators per lane; a tile of
// EIG_GRAM_ROWS x EIG_GRAM_COLS = 12 x 4 entries is 48 doubles = 96 VGPRs for ONE of the two matrices, and the two halves
// of a workgroup take one matrix each on the same items (k_eig_gram below), which leaves the registers for having every
// load of an item in flight at once. The driver walks the column blocks of S (four columns of one family at a time) and,
// for each, the rows above and on the diagonal in chunks of 12: for the usual block sizes m <= 4 that is ONE launch for
// the W columns (rows X, W; apply fused) and ONE for the P columns (rows X, W, P). The X x X block is known (X is
// orthonormal, X^T A X = diag(theta)) and is not computed by the solver; the kernel-level entry point computes it too.
//
// Layout as in mg_krylov.hip: a lane owns one 16-byte vector of a row, workgroups of 256 lanes, at most EIG_MAX_BLOCKS
// workgroups striding over the level; padding columns (x >= nx) are neither written nor summed.
//
// Arithmetic contract (compiled with -ffp-contract=off, tests/eig_ref.py restates it in numpy):
//   A w    = ((((((0 + cz w[k-1]) + cy w[j-1]) + cx w[i-1]) + cd w) + cx w[i+1]) + cy w[j+1]) + cz w[k+1] in T, w taken as 0
//            on Dirichlet nodes, result 0 on Dirichlet nodes
//   Gram   products and sums in double
//   S C    each element starts at 0.0 in double and adds (double) S_i * C_ij for i in the column order of S, every product
//            and sum rounded separately, rounded once to T
//   R      r = ax' - (T) theta_j * x' in T from the rounded x', ax'; sums of r^2 in double
//
// The operator families (enum mg_eig_operator; OPK below). With EIG_OP_FACES the stencil is the constant
// one and the faces of a mask are Neumann, with EIG_OP_COEFFICIENT it is mg_vc.hip's with the same kind of mask. Node classes
// are mg_bc.hip's: a node on a face outside the mask is a Dirichlet node, every other node is an unknown whose missing
// neighbours are mirror images. y and z are uniform over an item, so their mirrors are a select between two ADDRESSES before
// the load; the x mirrors are selects between values the lane holds. L is self-adjoint in the inner product of the weights w
// (1/2 per face of the mask a node lies on, bc_weight), so every product of both Gram halves and every r^2 of the combine
// carries w -- a power of two, the scaling is exact. tests/eigop_ref.py restates:
//   FACES        the sum of A w above with the mirrored value in the slot of the missing neighbour
//   COEFFICIENT  s = 0, d = (T)sigma; per slot z-, y-, x-, x+, y+, z+: g = w_a * (a_i + a_q), s = s + g * b_q, d = d + g with
//                w_a = (T)(-c_a / 2); L b = d * b_i - s (k_vcn_cg_direction's q); a is mirrored like b and never zeroed
#include "mg_opfamily.h"

namespace mg {

namespace {

constexpr int EIG_THREADS = 256;
constexpr int EIG_WAVES = EIG_THREADS / 64;

template <typename T>
__device__ __forceinline__ void vload(const T *p, T (&v)[Vec16<T>::n])
{
    const typename Vec16<T>::type w = *reinterpret_cast<const typename Vec16<T>::type *>(p);
    __builtin_memcpy(v, &w, sizeof(w));
}

template <typename T>
__device__ __forceinline__ void vstore(T *p, const T (&v)[Vec16<T>::n])
{
    typename Vec16<T>::type w;
    __builtin_memcpy(&w, v, sizeof(w));
    *reinterpret_cast<typename Vec16<T>::type *>(p) = w;
}

template <typename T>
__device__ __forceinline__ void vstore_masked(T *p, const T (&v)[Vec16<T>::n], int valid)
{
    constexpr int V = Vec16<T>::n;
    if (valid >= V) { vstore(p, v); return; }
#pragma unroll
    for (int e = 0; e < V; e++)
        if (e < valid) p[e] = v[e];
}

struct Item {
    int z, y, x0;
};
__device__ __forceinline__ Item item_of(unsigned it, unsigned vpr, unsigned ny, int V)
{
    const unsigned row = it / vpr;
    Item r;
    r.x0 = (int)(it - row * vpr) * V;
    r.y = (int)(row % ny);
    r.z = (int)(row / ny);
    return r;
}

// the row (z, y) lies on a Dirichlet plane / row
__device__ __forceinline__ bool row_is_boundary(const Geom &g, int z, int y)
{
    bool b = (y == 0) | (y == g.ny - 1);
    if (g.dim == 3) {
        const int gz = g.gz0 + z;
        b |= (gz == 0) | (gz == g.gnz - 1);
    }
    return b;
}

// one 16-byte vector with its Dirichlet nodes taken as zero (row_bnd: the whole row is one)
template <typename T>
__device__ __forceinline__ void vload_interior(const Geom &g, const T *p, int x0, bool row_bnd, T (&out)[Vec16<T>::n])
{
    constexpr int V = Vec16<T>::n;
    if (row_bnd) {
#pragma unroll
        for (int e = 0; e < V; e++) out[e] = (T)0;
        return;
    }
    vload(p, out);
#pragma unroll
    for (int e = 0; e < V; e++) {
        const int xx = x0 + e;
        if (xx == 0 || xx >= g.nx - 1) out[e] = (T)0;
    }
}

// Per-workgroup partial sums of many accumulators: stash() adds one accumulator over the wave and leaves the sum in LDS,
// flush() has lane k add accumulator k's waves in ascending order into partials[k * gridDim.x + blockIdx.x]
__device__ __forceinline__ void stash(double (*sh)[EIG_WAVES], int k, double v)
{
    const double s = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = s;
}
__device__ __forceinline__ void flush(int n, double *__restrict__ partials, double (*sh)[EIG_WAVES])
{
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += EIG_THREADS) {
        double s = 0;
        for (int w = 0; w < EIG_WAVES; w++) s += sh[k][w];
        partials[(size_t)k * gridDim.x + blockIdx.x] = s;
    }
}

// ---------------------------------------------------------------- Gram tile (+ the apply)
// The workgroup's two halves share the items and split the work: lanes 0 .. 127 (role 0) accumulate G = rows . b, lanes
// 128 .. 255 (role 1) make (or read) A b and accumulate H = rows . A b. A lane then holds ONE 12 x 4 tile of accumulators
// (96 VGPRs) instead of two, and the registers that frees hold the item's loads, all issued before the first is waited
// for; the rows are read by both halves at about the same time and the second read is served by the caches.
constexpr int GRAM_ITEMS = EIG_THREADS / 2;

// the mg_face bits of a row, a (global) plane and a column: bc_faces (mg_opfamily.h) axis by axis
__device__ __forceinline__ int y_faces(const Geom &g, int y) { return (y == 0 ? FYLO : 0) | (y == g.ny - 1 ? FYHI : 0); }
__device__ __forceinline__ int z_faces(const Geom &g, int gz) { return g.dim == 3 ? (gz == 0 ? FZLO : 0) | (gz == g.gnz - 1 ? FZHI : 0) : 0; }
__device__ __forceinline__ int x_faces(const Geom &g, int x) { return (x == 0 ? FXLO : 0) | (x == g.nx - 1 ? FXHI : 0); }

// OPK: the operator. EIG_OP_CONSTANT does not look at op and is the code it was before the families came. The others take
// the Dirichlet flags and the weights from op.mask; their apply loads the y / z neighbours from mirrored addresses, and with
// EIG_OP_COEFFICIENT the seven vectors of a once per item: the six g and d of the contract are shared by the tile's columns.
template <typename T, int DIM, bool APPLY, int OPK = EIG_OP_CONSTANT>
__global__ __launch_bounds__(EIG_THREADS) void k_eig_gram(Geom g, Coef<T> c, EigGramArgs<T> a, double *__restrict__ partials, EigOp<T> op)
{
    constexpr bool FAM = OPK != EIG_OP_CONSTANT;
    constexpr int V = Vec16<T>::n;
    constexpr int NA = EIG_GRAM_ROWS, NB = EIG_GRAM_COLS;
    __shared__ double sh[2 * NA * NB][EIG_WAVES];
    const unsigned vpr = (unsigned)(g.pitch / V), nitems = vpr * (unsigned)g.ny * (unsigned)g.nz;
    const int role = threadIdx.x / GRAM_ITEMS;   // uniform over a wave
    double acc[NA][NB];
#pragma unroll
    for (int i = 0; i < NA; i++)
#pragma unroll
        for (int j = 0; j < NB; j++) acc[i][j] = 0.;

    for (unsigned it = blockIdx.x * GRAM_ITEMS + threadIdx.x % GRAM_ITEMS; it < nitems; it += gridDim.x * GRAM_ITEMS) {
        const Item t = item_of(it, vpr, (unsigned)g.ny, V);
        const int valid = g.nx - t.x0;
        if (valid <= 0) continue;
        const long long i = (long long)t.z * g.plane + (long long)t.y * g.pitch + t.x0;
        const int frow = FAM ? y_faces(g, t.y) | z_faces(g, g.gz0 + t.z) : 0;   // the y and z faces the row lies on
        const bool rb = FAM ? (frow & ~op.mask) != 0 : row_is_boundary(g, t.z, t.y);
        bool dir[V];   // the element is a Dirichlet node (or a padding column)
        [[maybe_unused]] T wgt[V];
        [[maybe_unused]] bool any_dir = false;
#pragma unroll
        for (int e = 0; e < V; e++) {
            if constexpr (FAM) {
                const int fx = x_faces(g, t.x0 + e);
                dir[e] = rb || (fx & ~op.mask) != 0 || t.x0 + e >= g.nx;
                wgt[e] = (T)bc_weight(__popc((unsigned)((frow | fx) & op.mask)));
                any_dir |= dir[e] && e < valid;
            } else {
                dir[e] = rb || t.x0 + e == 0 || t.x0 + e >= g.nx - 1;
            }
        }
        // Every load of the item is issued before anything waits for one: no branch stands between them. The launcher points
        // the unused rows and columns at used ones, and a level-shaped array has a ghost plane either side, so the stencil's
        // neighbours of a Dirichlet node are addressable too; what must count as zero is zeroed by selects afterwards.
        T av[NA][V];
#pragma unroll
        for (int r = 0; r < NA; r++) vload(a.row[r] + i, av[r]);
        T cv[NB][V];   // role 0: b, role 1: A b
        if (role == 0) {
#pragma unroll
            for (int j = 0; j < NB; j++) vload(a.col[j] + i, cv[j]);
            if (APPLY || a.col_interior) {
#pragma unroll
                for (int j = 0; j < NB; j++)
#pragma unroll
                    for (int e = 0; e < V; e++) cv[j][e] = dir[e] ? (T)0 : cv[j][e];
            }
            // b := 0 on its Dirichlet nodes: only vectors that hold one are written (every reader takes them masked)
            if (APPLY && (FAM ? any_dir : (rb || t.x0 == 0 || t.x0 + V >= g.nx - 1))) {
#pragma unroll
                for (int j = 0; j < NB; j++)
                    if (j < a.nb) vstore_masked(a.col[j] + i, cv[j], valid);
            }
        } else if (!APPLY) {
#pragma unroll
            for (int j = 0; j < NB; j++) vload(a.acol[j] + i, cv[j]);
        } else if constexpr (FAM) {
            T pc[NB][V], ps[NB][V], pn[NB][V], pd[NB][V], pu[NB][V], pl[NB], pr[NB];
            [[maybe_unused]] T ac[V], as[V], an[V], ad[V], au[V], al, ar;
            const int gz = g.gz0 + t.z;
            // the rows of the y / z neighbours, mirrored on the faces the row lies on (in the mask or not: a row on a Dirichlet
            // face is dropped below, and the mirrored row always lies inside the level)
            const int ys = (frow & FYLO) ? t.y + 1 : t.y - 1, yn = (frow & FYHI) ? t.y - 1 : t.y + 1;
            const int zd = (frow & FZLO) ? gz + 1 : gz - 1, zu = (frow & FZHI) ? gz - 1 : gz + 1;
            const long long is = i + (long long)(ys - t.y) * g.pitch, in = i + (long long)(yn - t.y) * g.pitch;
            const long long id = i + (long long)(zd - gz) * g.plane, iu = i + (long long)(zu - gz) * g.plane;
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const T *const b = a.col[j];
                vload(b + i, pc[j]);
                vload(b + is, ps[j]);
                vload(b + in, pn[j]);
                if (DIM == 3) { vload(b + id, pd[j]); vload(b + iu, pu[j]); }
                pl[j] = b[i - 1];
                pr[j] = b[i + V];
            }
            if constexpr (OPK == EIG_OP_COEFFICIENT) {
                vload(op.a + i, ac);
                vload(op.a + is, as);
                vload(op.a + in, an);
                if (DIM == 3) { vload(op.a + id, ad); vload(op.a + iu, au); }
                al = op.a[i - 1];
                ar = op.a[i + V];
            }
            // a neighbour row counts as zero when it lies on a Dirichlet face
            const bool south0 = (y_faces(g, ys) & ~op.mask) != 0, north0 = (y_faces(g, yn) & ~op.mask) != 0;
            const bool down0 = (z_faces(g, zd) & ~op.mask) != 0, up0 = (z_faces(g, zu) & ~op.mask) != 0;
            // the elements beyond the vector's ends count when their column is an unknown's
            const bool l_in = t.x0 >= 1 && (t.x0 > 1 || (op.mask & FXLO)), r_in = t.x0 + V < g.nx - 1 || (t.x0 + V == g.nx - 1 && (op.mask & FXHI));
            // the six g and d of mg_vc.hip's contract per element, shared by the columns
            [[maybe_unused]] T gq[6][V], dd[V];
            if constexpr (OPK == EIG_OP_COEFFICIENT) {
#pragma unroll
                for (int e = 0; e < V; e++) {
                    const int xx = t.x0 + e;
                    const T aw = e == 0 ? al : ac[e - 1 < 0 ? 0 : e - 1];
                    const T axm = xx == 0 ? ac[1] : aw;
                    const T axp = xx == g.nx - 1 ? aw : (e == V - 1 ? ar : ac[e + 1 > V - 1 ? V - 1 : e + 1]);
                    T d = op.sigma;
                    if (DIM == 3) { gq[0][e] = op.wz * (ac[e] + ad[e]); d = d + gq[0][e]; }
                    gq[1][e] = op.wy * (ac[e] + as[e]); d = d + gq[1][e];
                    gq[2][e] = op.wx * (ac[e] + axm); d = d + gq[2][e];
                    gq[3][e] = op.wx * (ac[e] + axp); d = d + gq[3][e];
                    gq[4][e] = op.wy * (ac[e] + an[e]); d = d + gq[4][e];
                    if (DIM == 3) { gq[5][e] = op.wz * (ac[e] + au[e]); d = d + gq[5][e]; }
                    dd[e] = d;
                }
            }
#pragma unroll
            for (int j = 0; j < NB; j++) {
#pragma unroll
                for (int e = 0; e < V; e++) {
                    const int xx = t.x0 + e;
                    const bool xd = (x_faces(g, xx) & ~op.mask) != 0 || xx >= g.nx;   // a Dirichlet (or padding) column
                    pc[j][e] = xd ? (T)0 : pc[j][e];
                    ps[j][e] = south0 ? (T)0 : ps[j][e];
                    pn[j][e] = north0 ? (T)0 : pn[j][e];
                    if (DIM == 3) {
                        pd[j][e] = down0 ? (T)0 : pd[j][e];
                        pu[j][e] = up0 ? (T)0 : pu[j][e];
                    }
                }
                const T wl = l_in ? pl[j] : (T)0;
                const T er = r_in ? pr[j] : (T)0;
#pragma unroll
                for (int e = 0; e < V; e++) {
                    const int xx = t.x0 + e;
                    // x = 0 takes its right neighbour for the left one; x = nx - 1 its left one, which is pl when the node is
                    // alone in its vector and pc[e - 1] when it lies inside one
                    const T lw = e == 0 ? wl : pc[j][e - 1 < 0 ? 0 : e - 1];
                    const T w = xx == 0 ? pc[j][1] : lw;
                    const T ea = xx == g.nx - 1 ? lw : (e == V - 1 ? er : pc[j][e + 1 > V - 1 ? V - 1 : e + 1]);
                    T s = 0;
                    if constexpr (OPK == EIG_OP_COEFFICIENT) {
                        if (DIM == 3) s = s + gq[0][e] * pd[j][e];
                        s = s + gq[1][e] * ps[j][e];
                        s = s + gq[2][e] * w;
                        s = s + gq[3][e] * ea;
                        s = s + gq[4][e] * pn[j][e];
                        if (DIM == 3) s = s + gq[5][e] * pu[j][e];
                        s = dd[e] * pc[j][e] - s;
                    } else {
                        if (DIM == 3) s += c.cz * pd[j][e];
                        s += c.cy * ps[j][e];
                        s += c.cx * w;
                        s += c.cd * pc[j][e];
                        s += c.cx * ea;
                        s += c.cy * pn[j][e];
                        if (DIM == 3) s += c.cz * pu[j][e];
                    }
                    cv[j][e] = dir[e] ? (T)0 : s;
                }
                if (j < a.nb) vstore_masked(a.acol[j] + i, cv[j], valid);
            }
        } else {
            T pc[NB][V], ps[NB][V], pn[NB][V], pd[NB][V], pu[NB][V], pl[NB], pr[NB];
            const int gz = g.gz0 + t.z;
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const T *const b = a.col[j];
                vload(b + i, pc[j]);
                vload(b + i - g.pitch, ps[j]);
                vload(b + i + g.pitch, pn[j]);
                if (DIM == 3) { vload(b + i - g.plane, pd[j]); vload(b + i + g.plane, pu[j]); }
                pl[j] = b[i - 1];
                pr[j] = b[i + V];
            }
            const bool south0 = t.y - 1 <= 0, north0 = t.y + 1 >= g.ny - 1, down0 = gz - 1 <= 0, up0 = gz + 1 >= g.gnz - 1;
#pragma unroll
            for (int j = 0; j < NB; j++) {
#pragma unroll
                for (int e = 0; e < V; e++) {
                    const int xx = t.x0 + e;
                    const bool xd = xx == 0 || xx >= g.nx - 1;   // a Dirichlet column: zero in every row
                    pc[j][e] = xd ? (T)0 : pc[j][e];
                    ps[j][e] = xd || south0 ? (T)0 : ps[j][e];
                    pn[j][e] = xd || north0 ? (T)0 : pn[j][e];
                    if (DIM == 3) {
                        pd[j][e] = xd || down0 ? (T)0 : pd[j][e];
                        pu[j][e] = xd || up0 ? (T)0 : pu[j][e];
                    }
                }
                // x-neighbours across the vector's ends: one element each, zero on the Dirichlet columns
                const T wl = (t.x0 - 1 >= 1) ? pl[j] : (T)0;
                const T er = (t.x0 + V <= g.nx - 2) ? pr[j] : (T)0;
#pragma unroll
                for (int e = 0; e < V; e++) {
                    const T w = e == 0 ? wl : pc[j][e - 1 < 0 ? 0 : e - 1];
                    const T ea = e == V - 1 ? er : pc[j][e + 1 > V - 1 ? V - 1 : e + 1];
                    T s = 0;
                    if (DIM == 3) s += c.cz * pd[j][e];
                    s += c.cy * ps[j][e];
                    s += c.cx * w;
                    s += c.cd * pc[j][e];
                    s += c.cx * ea;
                    s += c.cy * pn[j][e];
                    if (DIM == 3) s += c.cz * pu[j][e];
                    cv[j][e] = dir[e] ? (T)0 : s;
                }
                if (j < a.nb) vstore_masked(a.acol[j] + i, cv[j], valid);
            }
        }
        if constexpr (FAM) {   // after the store of A b: both halves weigh their products
#pragma unroll
            for (int j = 0; j < NB; j++)
#pragma unroll
                for (int e = 0; e < V; e++) cv[j][e] = cv[j][e] * wgt[e];
        }
#pragma unroll
        for (int r = 0; r < NA; r++) {
            const bool rin = (a.row_interior >> r) & 1u;
#pragma unroll
            for (int e = 0; e < V; e++) av[r][e] = (rin && dir[e]) || e >= valid ? (T)0 : av[r][e];
        }
#pragma unroll
        for (int r = 0; r < NA; r++) {
            if (r >= a.na) continue;
#pragma unroll
            for (int j = 0; j < NB; j++) {
                if (j >= a.nb) continue;
#pragma unroll
                for (int e = 0; e < V; e++) acc[r][j] += (double)av[r][e] * (double)cv[j][e];
            }
        }
    }
    // partial k = (r * NB + j) of G, NA * NB + the same of H; entries outside na x nb are written as the zeros they hold. A
    // role's two waves fill slots 0, 1 of their accumulators, the other two slots stay zero.
    for (int k = threadIdx.x; k < 2 * NA * NB * EIG_WAVES; k += EIG_THREADS) (&sh[0][0])[k] = 0.;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NA; r++)
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const double s = wave_sum(acc[r][j]);
            if ((threadIdx.x & 63) == 0) sh[role * NA * NB + r * NB + j][(threadIdx.x >> 6) & 1] = s;
        }
    flush(2 * NA * NB, partials, sh);
}

// ---------------------------------------------------------------- combine + residual
// MB: columns held as accumulators (the block size rounded up to 4 or 8)
// WGT: the sums of r^2 carry the weights of a.mask; the arrays are written as without it
template <typename T, int MB, bool WGT = false>
__global__ __launch_bounds__(EIG_THREADS) void k_eig_combine(Geom g, EigCombineArgs<T> a, const double *__restrict__ coef,
                                                             const double *__restrict__ theta, double *__restrict__ partials)
{
    constexpr int V = Vec16<T>::n;
    __shared__ double sh[MB][EIG_WAVES];
    const unsigned vpr = (unsigned)(g.pitch / V), nitems = vpr * (unsigned)g.ny * (unsigned)g.nz;
    const int m = a.m, nw = a.nw, s = a.m + a.nw + a.np;
    const double *const cp = coef + (size_t)s * m;   // Cp follows Cx
    double rr[MB];
#pragma unroll
    for (int j = 0; j < MB; j++) rr[j] = 0.;

    for (unsigned it = blockIdx.x * EIG_THREADS + threadIdx.x; it < nitems; it += gridDim.x * EIG_THREADS) {
        const Item t = item_of(it, vpr, (unsigned)g.ny, V);
        const int valid = g.nx - t.x0;
        if (valid <= 0) continue;
        const long long i = (long long)t.z * g.plane + (long long)t.y * g.pitch + t.x0;
        [[maybe_unused]] double wgt[V];
        if constexpr (WGT) {
            const int frow = y_faces(g, t.y) | z_faces(g, g.gz0 + t.z);
#pragma unroll
            for (int e = 0; e < V; e++) wgt[e] = bc_weight(__popc((unsigned)((frow | x_faces(g, t.x0 + e)) & a.mask)));
        }
        double x[MB][V], ax[MB][V], p[MB][V], ap[MB][V];
#pragma unroll
        for (int j = 0; j < MB; j++)
#pragma unroll
            for (int e = 0; e < V; e++) { x[j][e] = 0.; ax[j][e] = 0.; p[j][e] = 0.; ap[j][e] = 0.; }
        for (int k = 0; k < s; k++) {   // the column order of S = [X, W, P]
            T sv[V], asv[V];
            vload(a.s[k] + i, sv);
            vload(a.as[k] + i, asv);
#pragma unroll
            for (int j = 0; j < MB; j++) {
                if (j >= m) continue;
                const double cx = coef[k * m + j];
#pragma unroll
                for (int e = 0; e < V; e++) {
                    x[j][e] += (double)sv[e] * cx;
                    ax[j][e] += (double)asv[e] * cx;
                }
            }
            if (k >= m) {
#pragma unroll
                for (int j = 0; j < MB; j++) {
                    if (j >= nw) continue;
                    const double cpj = cp[(k - m) * nw + j];
#pragma unroll
                    for (int e = 0; e < V; e++) {
                        p[j][e] += (double)sv[e] * cpj;
                        ap[j][e] += (double)asv[e] * cpj;
                    }
                }
            }
        }
        // every family has been read at this node: the in-place stores
#pragma unroll
        for (int j = 0; j < MB; j++) {
            if (j >= m) continue;
            const T th = (T)theta[j];
            T xv[V], axv[V], rv[V];
#pragma unroll
            for (int e = 0; e < V; e++) {
                xv[e] = (T)x[j][e];
                axv[e] = (T)ax[j][e];
                rv[e] = axv[e] - th * xv[e];
                if constexpr (WGT) { if (e < valid) rr[j] += wgt[e] * ((double)rv[e] * (double)rv[e]); }
                else if (e < valid) rr[j] += (double)rv[e] * (double)rv[e];
            }
            vstore_masked(a.x[j] + i, xv, valid);
            vstore_masked(a.ax[j] + i, axv, valid);
            vstore_masked(a.r[j] + i, rv, valid);
        }
#pragma unroll
        for (int j = 0; j < MB; j++) {
            if (j >= nw) continue;
            T pv[V], apv[V];
#pragma unroll
            for (int e = 0; e < V; e++) { pv[e] = (T)p[j][e]; apv[e] = (T)ap[j][e]; }
            vstore_masked(a.p[j] + i, pv, valid);
            vstore_masked(a.ap[j] + i, apv, valid);
        }
    }
#pragma unroll
    for (int j = 0; j < MB; j++) stash(sh, j, rr[j]);
    flush(m, partials, sh);
}

// ---------------------------------------------------------------- fixed-order sums of the partials: one workgroup per sum
__global__ __launch_bounds__(EIG_THREADS) void k_eig_reduce(const double *__restrict__ partials, int nb, double *__restrict__ out)
{
    __shared__ double sh[EIG_WAVES];
    double s = 0.;
    for (int i = threadIdx.x; i < nb; i += EIG_THREADS) s += partials[(size_t)blockIdx.x * nb + i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---------------------------------------------------------------- the default start vectors
// splitmix64 of the node's global index and the column: uniform in [-1, 1), 0 on Dirichlet nodes. The hash has no
// structure a grid symmetry could survive.
template <typename T>
__global__ __launch_bounds__(EIG_THREADS) void k_eig_fill(Geom g, T *__restrict__ x, int column)
{
    const unsigned n = (unsigned)g.pitch * (unsigned)g.ny * (unsigned)g.nz;
    for (unsigned it = blockIdx.x * EIG_THREADS + threadIdx.x; it < n; it += gridDim.x * EIG_THREADS) {
        const unsigned row = it / (unsigned)g.pitch;
        const int xx = (int)(it - row * (unsigned)g.pitch), y = (int)(row % (unsigned)g.ny), zz = (int)(row / (unsigned)g.ny);
        if (xx >= g.nx) continue;
        const long long i = (long long)zz * g.plane + (long long)y * g.pitch + xx;
        T v = (T)0;
        if (!(row_is_boundary(g, zz, y) || xx == 0 || xx == g.nx - 1)) {
            const unsigned long long node = ((unsigned long long)(g.gz0 + zz) * (unsigned)g.ny + (unsigned)y) * (unsigned)g.nx + (unsigned)xx;
            unsigned long long h = node + 0x9E3779B97F4A7C15ull * (unsigned long long)(column + 1);
            h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
            h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
            h ^= h >> 31;
            v = (T)((double)(h >> 11) * (2.0 / 9007199254740992.0) - 1.0);
        }
        x[i] = v;
    }
}

int eig_grid(const Geom &g, int per_item)
{
    const long long items = (long long)(g.pitch / per_item) * g.ny * g.nz;
    return (int)std::min<long long>(EIG_MAX_BLOCKS, std::max<long long>(1, (items + EIG_THREADS - 1) / EIG_THREADS));
}

template <typename T, int OPK>
void eig_gram_launch(hipStream_t s, int nb, const Geom &g, const Coef<T> &c, const EigOp<T> &op, const EigGramArgs<T> &a, bool apply,
                     double *partials)
{
    if (apply) {
        if (g.dim == 3) hipLaunchKernelGGL((k_eig_gram<T, 3, true, OPK>), dim3(nb), dim3(EIG_THREADS), 0, s, g, c, a, partials, op);
        else hipLaunchKernelGGL((k_eig_gram<T, 2, true, OPK>), dim3(nb), dim3(EIG_THREADS), 0, s, g, c, a, partials, op);
    } else {
        // DIM is not looked at, and the operator only decides the Dirichlet flags and the weights: FACES' instantiation serves COEFFICIENT
        constexpr int K = OPK == EIG_OP_COEFFICIENT ? EIG_OP_FACES : OPK;
        hipLaunchKernelGGL((k_eig_gram<T, 2, false, K>), dim3(nb), dim3(EIG_THREADS), 0, s, g, c, a, partials, op);
    }
}

}  // namespace

template <typename T>
int launch_eig_gram(hipStream_t s, const Geom &g, const Coef<T> &c, const EigOp<T> &op, const EigGramArgs<T> &a, bool apply,
                    double *partials)
{
    const long long items = (long long)(g.pitch / Vec16<T>::n) * g.ny * g.nz;
    const int nb = (int)std::min<long long>(EIG_MAX_BLOCKS, std::max<long long>(1, (items + GRAM_ITEMS - 1) / GRAM_ITEMS));
    if (op.kind == EIG_OP_CONSTANT) eig_gram_launch<T, EIG_OP_CONSTANT>(s, nb, g, c, op, a, apply, partials);
    else if (op.kind == EIG_OP_FACES) eig_gram_launch<T, EIG_OP_FACES>(s, nb, g, c, op, a, apply, partials);
    else eig_gram_launch<T, EIG_OP_COEFFICIENT>(s, nb, g, c, op, a, apply, partials);
    return nb;
}

template <typename T>
int launch_eig_combine(hipStream_t s, const Geom &g, const EigCombineArgs<T> &a, const double *coef, const double *theta,
                       double *partials)
{
    const int nb = eig_grid(g, Vec16<T>::n);
#define MG_EIG_COMBINE(MB, WGT) hipLaunchKernelGGL((k_eig_combine<T, MB, WGT>), dim3(nb), dim3(EIG_THREADS), 0, s, g, a, coef, theta, partials)
    if (a.weighted) { if (a.m <= 4) MG_EIG_COMBINE(4, true); else MG_EIG_COMBINE(8, true); }
    else { if (a.m <= 4) MG_EIG_COMBINE(4, false); else MG_EIG_COMBINE(8, false); }
#undef MG_EIG_COMBINE
    return nb;
}

void launch_eig_reduce(hipStream_t s, const double *partials, int nb, int nsums, double *out)
{
    hipLaunchKernelGGL(k_eig_reduce, dim3(nsums), dim3(EIG_THREADS), 0, s, partials, nb, out);
}

template <typename T>
void launch_eig_fill(hipStream_t s, const Geom &g, T *x, int column)
{
    hipLaunchKernelGGL((k_eig_fill<T>), dim3(eig_grid(g, 1)), dim3(EIG_THREADS), 0, s, g, x, column);
}

#define MG_EIG_INST(T)                                                                                                        \
    template int launch_eig_gram<T>(hipStream_t, const Geom &, const Coef<T> &, const EigOp<T> &, const EigGramArgs<T> &, bool, \
                                    double *);                                                                                \
    template int launch_eig_combine<T>(hipStream_t, const Geom &, const EigCombineArgs<T> &, const double *, const double *,  \
                                       double *);                                                                             \
    template void launch_eig_fill<T>(hipStream_t, const Geom &, T *, int);
MG_EIG_INST(double)
MG_EIG_INST(float)
#undef MG_EIG_INST

}  // namespace mg
