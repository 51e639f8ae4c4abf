// mg_geom.h -- device-side description of one grid level as it lives in HBM.
//
// Layout: every level owns dense arrays of
//   (nz + 2) planes x ny rows x pitch elements,
// pitch = nx rounded up to 128 B so every row starts on a 128-byte line and lane
// l of a wave reads x = 2l,2l+1 (fp64) / 4l..4l+3 (fp32) with one aligned 16-byte
// access.  Plane 0 and plane nz+1 are ghost planes (z-halo of the slab
// decomposition; unused and zero on one GPU, where no kernel writes them); `p`
// pointers handed to kernels point at local plane 0, i.e. one plane into the
// allocation.  Padding columns x >= nx stay zero: they are written only with
// zeros -- by the tail-line stores (mg_device.h), the line store of mg_fmg.hip
// and the copies into the layout (mg_io.hip, the host staging of mg_set_array).
// tests/test_storage_gpu.py holds every entry point to both.
#ifndef MG_GEOM_H
#define MG_GEOM_H

#include <algorithm>
#include <cmath>

namespace mg {

struct Geom {
    int dim;          // 2 or 3 (2-D levels have nz == 1 and no z coupling)
    int nx, ny, nz;   // local extents; nx == ny == global n, nz = local planes
    int pitch;        // elements per row
    long long plane;  // elements per plane = ny * pitch
    int gz0;          // global z index of local plane 0
    int gnz;          // global number of planes (n in 3-D, 1 in 2-D)
};

// the transition fine -> coarse keeps z (semi-coarsening): fine plane z <-> coarse plane z
inline bool is_semi_transition(const Geom &gf, const Geom &gc) { return gf.dim == 3 && gf.gnz == gc.gnz && gf.gnz > 1; }

// off-diagonals (negative) per axis and the diagonal of the level's operator,
// include/linear_system.hpp:27-28,37-38 of the reference
// rcd / win drive div_cd() below: rcd = RN(1/cd), win = width of the numerator's exponent window
// in which the three-operation division is exact (0 = always use the hardware division).
template <typename T>
struct Coef {
    T cx, cy, cz, cd;
    T rcd;
    unsigned win;
};

// ---- correctly rounded division by the diagonal in three operations ---------------------------
// The Jacobi / Gauss-Seidel update divides by the constant diagonal cd. An IEEE division costs
// ~20 VALU issue slots in fp64 (v_div_scale, quarter-rate v_rcp, Newton steps, v_div_fmas,
// v_div_fixup); with y = RN(1/cd) computed once on the host,
//     q = RN(a*y);  r = a - q*cd (exact, one FMA);  q' = RN(q + r*y)
// is RN(a/cd) (Markstein's theorem: y correctly rounded, q within one ulp, cd's significand not
// all ones, no intermediate under/overflow). The host checks cd (make_coef); the exponent window
// on `a` keeps q and r far from the subnormal and overflow ranges; numerators outside it (zero,
// tiny, huge, Inf, NaN) take the hardware division. Bit-identical to a / cd either way, which
// the parity tests check on every sweep they compare.
template <typename T> struct DivWindow;
template <> struct DivWindow<double> { static constexpr unsigned lo = 1023 - 900, span = 1800, cd_lo = 1023 - 100, cd_span = 200; };
template <> struct DivWindow<float> { static constexpr unsigned lo = 127 - 60, span = 120, cd_lo = 127 - 30, cd_span = 60; };

inline unsigned biased_exponent(double v) { unsigned long long u; __builtin_memcpy(&u, &v, 8); return (unsigned)(u >> 52) & 0x7ffu; }
inline unsigned biased_exponent(float v) { unsigned u; __builtin_memcpy(&u, &v, 4); return (u >> 23) & 0xffu; }

template <typename T>
inline Coef<T> make_coef(double cx, double cy, double cz, double cd)
{
    Coef<T> c{(T)cx, (T)cy, (T)cz, (T)cd, (T)0, 0u};
    const T one = (T)1;
    c.rcd = one / c.cd;  // correctly rounded by the host FPU
    unsigned long long mant, all;
    if (sizeof(T) == 8) { unsigned long long u; __builtin_memcpy(&u, &c.cd, 8); all = (1ull << 52) - 1; mant = u & all; }
    else { unsigned u; __builtin_memcpy(&u, &c.cd, 4); all = (1u << 23) - 1; mant = u & all; }
    const bool ok = (biased_exponent(c.cd) - DivWindow<T>::cd_lo) < DivWindow<T>::cd_span && mant != all;
    c.win = ok ? DivWindow<T>::span : 0u;
    return c;
}

#ifdef __HIPCC__
__device__ __forceinline__ unsigned dev_biased_exponent(double v) { return ((unsigned)__double2hiint(v) >> 20) & 0x7ffu; }
__device__ __forceinline__ unsigned dev_biased_exponent(float v) { return (__float_as_uint(v) >> 23) & 0xffu; }
__device__ __forceinline__ double dev_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float dev_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

template <typename T>
__device__ __forceinline__ T div_cd(T a, const Coef<T> &c)
{
    if ((dev_biased_exponent(a) - DivWindow<T>::lo) < c.win) {
        const T q = a * c.rcd;
        const T r = dev_fma(-q, c.cd, a);
        return dev_fma(r, c.rcd, q);
    }
    return a / c.cd;
}

// N quotients at once, straight-line: the three-operation quotients are computed for every
// element and ONE rarely taken branch redoes the group with the hardware division when any
// numerator was outside the window (a per-element branch would split the unrolled stencil code
// into basic blocks and serialise the loads and the arithmetic of neighbouring points).
template <typename T, int N>
__device__ __forceinline__ void div_cd_n(const T (&a)[N], T (&q)[N], const Coef<T> &c)
{
    bool ok = true;
#pragma unroll
    for (int e = 0; e < N; e++) {
        const T q0 = a[e] * c.rcd;
        const T r = dev_fma(-q0, c.cd, a[e]);
        q[e] = dev_fma(r, c.rcd, q0);
        ok = ok && ((dev_biased_exponent(a[e]) - DivWindow<T>::lo) < c.win);
    }
    if (__builtin_expect(!ok, 0)) {
#pragma unroll
        for (int e = 0; e < N; e++) q[e] = a[e] / c.cd;
    }
}

// The same with a WAVE-uniform test: the three-operation quotients run for every lane with the full execution mask (the
// per-lane test above makes the compiler wrap them in execution-mask regions, 8-10 scalar instructions per group); when ANY
// lane of the wave fell outside the window the whole wave redoes the group with the hardware division -- same bits for the
// lanes that were inside it.
template <typename T, int N>
__device__ __forceinline__ void div_cd_n_wave(const T (&a)[N], T (&q)[N], const Coef<T> &c)
{
    bool ok = true;
#pragma unroll
    for (int e = 0; e < N; e++) {
        const T q0 = a[e] * c.rcd;
        const T r = dev_fma(-q0, c.cd, a[e]);
        q[e] = dev_fma(r, c.rcd, q0);
        ok = ok && ((dev_biased_exponent(a[e]) - DivWindow<T>::lo) < c.win);
    }
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) != 0ull, 0)) {
#pragma unroll
        for (int e = 0; e < N; e++) q[e] = a[e] / c.cd;
    }
}
#endif

// ---- how a wide-tile launch (k_pairw, k_rrw: one 1024-thread workgroup per CU) is dealt to the CUs ----------------
// Work = ncopy copies x nby y-tiles x nz planes. `grid` workgroups (a multiple of 8 for the XCD-aware order) and either
//  * RANGES (zc = 0; mode 0): the tile-planes are cut into `grid` equal runs, at least min_items_per_wg each, or
//  * z-CHUNKS of zc planes, one workgroup per chunk: nz is cut into kk = 1 .. kk_max equal chunks and the count whose
//    last round on ncu CUs is fullest wins, a chunk of zc planes costing planes_per_step * zc + overhead plane steps;
//    zc_forced > 0 overrides the search.
// Pure: the callers pass the CU count and their switches (mg_pair_wide.hip: wide_plan has the measurements).
struct ChunkPlan { int grid, zc; };
inline ChunkPlan chunk_plan(int nz, int nby, int ncopy, int ncu, int min_items_per_wg, int kk_max, int planes_per_step,
                            double overhead, int mode, int zc_forced)
{
    const long long total = (long long)ncopy * nby * nz;
    const int grid = (int)std::max<long long>(8, (std::min<long long>(ncu, total / min_items_per_wg) / 8) * 8);
    if (mode == 0) return {grid, 0};
    int best_zc = std::max(1, nz);
    double best = 1e30;
    for (int kk = 1; kk <= kk_max; kk++) {
        const int zc = (nz + kk - 1) / kk, nbz = (nz + zc - 1) / zc;
        const double rounds = std::ceil((double)ncopy * nby * nbz / grid);
        const double cost = std::max(rounds, 1.0) * (planes_per_step * zc + overhead);
        if (cost < best - 1e-9) { best = cost; best_zc = zc; }
    }
    if (zc_forced > 0) best_zc = zc_forced;
    const long long items = (long long)ncopy * nby * ((nz + best_zc - 1) / best_zc);
    return {(int)(((items + 7) / 8) * 8), best_zc};
}

// ---- which kernel solves the coarsest grid (launch_coarse_solve, mg_kernels.hip) ------------------------------------
// One workgroup runs the whole Solver::Solve loop; which kernel depends on the shape, the element size, the smoother and
// omega. Pure: the caller passes its switches (MG_COARSE_ROWS, MG_COARSE_RB_ROWS, MG_COARSE_GS_ROWS) and launches what the
// plan says; tests/test_coarse_plan_cpu.py sweeps it over every shape a descriptor can make coarsest and
// tests/coarse_table.py lists what is reachable.
//  * JACOBI_ROWS / RB_ROWS: a thread owns a run of `seg` interior points of one row. The runs must be full and may share
//    at most one point per row (`overlap`), 128 <= threads <= 1024 (512 for runs of 7 and 8: registers). The first run
//    length of the measured order of preference that fits the ROW is taken (2-D: 65^2 -> 8, 504 threads, two waves per
//    SIMD: 52 ms for BASELINE config 1 against 55 ms with 7 and 64 ms with 9; 3-D: 17^3 -> 5, 675 threads; 8 is 2 % slower
//    per V-cycle at 513^3); when that one then lacks LDS room no other length is tried. Only these two take the zero
//    guess as a flag (zero_x); for every other kernel the launcher clears x first (memset).
//  * skip (Jacobi rows): sweeps between two norm tests. 8 needs a third LDS array (the window's first iterate) and
//    0 < omega <= 1 (damped Jacobi on this operator is then a contraction in the 2-norm, so the norm cannot dip below
//    the tolerance and rise again inside a window); otherwise 1, every sweep tested.
//  * GS_ROWS2D: lexicographic Gauss-Seidel, 2-D, at most 256 rows, two LDS copies.
//  * LDS: the generic loop, three arrays in LDS, at most 5 points per thread. GLOBAL: the global-memory loop.
constexpr int COARSE_WG = 1024, COARSE_GS_WG = 256, COARSE_LDS_PT = 5, COARSE_SKIP = 8;
constexpr long long COARSE_LDS_MAX = 150 * 1024;
enum CoarseKernel { COARSE_JACOBI_ROWS = 0, COARSE_RB_ROWS = 1, COARSE_GS_ROWS2D = 2, COARSE_LDS = 3, COARSE_GLOBAL = 4 };
struct CoarsePlan {
    int kernel;           // CoarseKernel
    int seg;              // run length (row kernels), 0 otherwise
    int overlap;          // the last run of a row shares one point with its neighbour
    int skip;             // Jacobi rows: 8 or 1; 0 otherwise
    int threads;          // workgroup size as launched
    long long lds_bytes;  // dynamic LDS
    int zero_x;           // the kernel takes the zero guess as a flag
    int memset;           // the launcher clears x before the kernel
};

inline int coarse_rows_max_threads(int seg) { return seg >= 7 ? COARSE_WG / 2 : COARSE_WG; }

// run length of a row kernel for this shape: the first of `order` whose runs fit; 0 = none
inline int coarse_rows_seg(int dim, int nx, int ny, int nz, const int *order, int norder)
{
    if (ny < 3 || (dim == 3 && nz < 3)) return 0;
    const int W = nx - 2, irows = (ny - 2) * (dim == 3 ? nz - 2 : 1);
    for (int k = 0; k < norder; k++) {
        const int seg = order[k], nseg = (W + seg - 1) / seg, threads = nseg * irows;
        if (W < seg || nseg * seg - W > 1 || threads < 128 || threads > coarse_rows_max_threads(seg)) continue;
        return seg;
    }
    return 0;
}

inline CoarsePlan coarse_plan(int dim, int nx, int ny, int nz, int elem_size, int smoother, double omega, bool x_is_zero,
                              bool whole_level, bool coarse_rows, bool coarse_rb_rows, bool coarse_gs_rows)
{
    const long long total = (long long)nx * ny * nz;
    const int clear = x_is_zero ? 1 : 0;
    auto rows = [&](int kernel, int seg, int skip, int copies) {
        const int W = nx - 2, nseg = (W + seg - 1) / seg;
        const int threads = nseg * (ny - 2) * (dim == 3 ? nz - 2 : 1);
        return CoarsePlan{kernel, seg, nseg * seg - W, skip, ((threads + 63) / 64) * 64, copies * total * elem_size, clear, 0};
    };
    if (smoother == 1 && whole_level && coarse_rows) {  // Jacobi
        static const int order2[4] = {8, 4, 7, 5}, order3[4] = {5, 4, 8, 7};
        const int seg = coarse_rows_seg(dim, nx, ny, nz, dim == 3 ? order3 : order2, 4);
        int skip = COARSE_SKIP;
        if (3 * total * elem_size > COARSE_LDS_MAX) skip = 1;   // no room for the window's first iterate
        if (!(omega > 0 && omega <= 1)) skip = 1;
        const int copies = skip > 1 ? 3 : 2;
        if (seg && copies * total * elem_size <= COARSE_LDS_MAX) return rows(COARSE_JACOBI_ROWS, seg, skip, copies);
    }
    if (smoother == 2 && whole_level && coarse_rb_rows) {  // red-black (runs of 7 / 8 points: the colour selects went through scratch memory)
        static const int order[2] = {5, 4};
        const int seg = coarse_rows_seg(dim, nx, ny, nz, order, 2);
        if (seg && 2 * total * elem_size <= COARSE_LDS_MAX) return rows(COARSE_RB_ROWS, seg, 0, 2);
    }
    if (smoother == 0 && coarse_gs_rows && dim == 2 && ny <= COARSE_GS_WG && nx >= 3 && ny >= 3 &&
        2 * (long long)nx * ny * elem_size <= COARSE_LDS_MAX)
        return CoarsePlan{COARSE_GS_ROWS2D, 0, 0, 0, COARSE_GS_WG, 2 * (long long)nx * ny * elem_size, 0, clear};
    if (total <= (long long)COARSE_LDS_PT * COARSE_WG && 3 * total * elem_size <= COARSE_LDS_MAX)
        return CoarsePlan{COARSE_LDS, 0, 0, 0, COARSE_WG, 3 * total * elem_size, 0, clear};
    return CoarsePlan{COARSE_GLOBAL, 0, 0, 0, COARSE_WG, 0, 0, clear};
}

// ---- which levels the one-launch LDS sub-cycle (k_subcycle, mg_subcycle.hip) can hold ---------------------------------------
// One workgroup runs the whole recursion below a ROOT level out of LDS: for every level l in [root, levels - 1] the arrays
// u_l, t_l (Jacobi's out-of-place target and the residual) and b_l lie dense (pitch = nx) behind the reduction scratch.
// Admissible: 1 <= root <= levels - 2 (level 0 keeps its fused pairs, its folded prolongation, the profiling brackets and
// mg_solve's norm: it always runs by launches), every transition from root downwards coarsens all axes (root >= semi_xy),
// the smoother is Jacobi or red-black, and everything fits COARSE_LDS_MAX. Pure: nx, ny, nz are the extents of ALL levels
// of the hierarchy; the caller adds what only it knows (one GPU, no stage callback). off[k][0..2]: byte offsets of u, t, b
// of level root + k. tests/test_cycle_kinds_cpu.py pins it.
constexpr int SUBCYCLE_MAX_LEVELS = 8;
constexpr long long SUBCYCLE_SCRATCH = 256;   // the block sums' 18 doubles, rounded up
struct SubcyclePlan {
    int root;             // -1: not admissible
    int nres;             // resident levels = levels - root
    long long off[SUBCYCLE_MAX_LEVELS][3];
    long long lds_bytes;  // dynamic LDS, scratch included
};

inline SubcyclePlan subcycle_plan(int levels, const int *nx, const int *ny, const int *nz, int semi_xy, int smoother, int elem_size,
                                  int root)
{
    SubcyclePlan p{};
    p.root = -1;
    if (root < 1 || root > levels - 2 || levels - root > SUBCYCLE_MAX_LEVELS) return p;
    if (root < semi_xy) return p;
    if (smoother != 1 && smoother != 2) return p;   // MG_SMOOTH_JACOBI, MG_SMOOTH_RBGS
    long long at = SUBCYCLE_SCRATCH;
    for (int l = root; l < levels; l++) {
        const long long bytes = (((long long)nx[l] * ny[l] * nz[l] * elem_size + 15) / 16) * 16;
        for (int a = 0; a < 3; a++) { p.off[l - root][a] = at; at += bytes; }
    }
    if (at > COARSE_LDS_MAX) return p;
    p.root = root;
    p.nres = levels - root;
    p.lds_bytes = at;
    return p;
}

// the finest admissible root, -1: none
inline int subcycle_finest_root(int levels, const int *nx, const int *ny, const int *nz, int semi_xy, int smoother, int elem_size)
{
    for (int root = 1; root <= levels - 2; root++)
        if (subcycle_plan(levels, nx, ny, nz, semi_xy, smoother, elem_size, root).root == root) return root;
    return -1;
}

// The root W and F handles take by default (MG_SUBCYCLE_LEVEL = -1): the level below the finest admissible root, or that
// root itself when nothing lies between it and the coarsest level. One workgroup sweeps the finest admissible grid (17^3 in
// 3-D) more slowly than the chip-wide launches do, and only from the next level down (9^3: one point per thread) does a visit
// cost less in the kernel than its five or six launches: tools/cycle_kinds_times.py, profiles/cycle_kinds_times.log (W-cycle
// at 513^3 fp64: 6.13 ms by launches, 5.67 ms rooted at 17^3, 5.39 ms rooted at 9^3; the same order at 1025^3 fp32 and
// 129^3, Jacobi and red-black). -1: none.
inline int subcycle_default_root(int levels, const int *nx, const int *ny, const int *nz, int semi_xy, int smoother, int elem_size)
{
    const int finest = subcycle_finest_root(levels, nx, ny, nz, semi_xy, smoother, elem_size);
    if (finest < 0) return -1;
    return finest + 1 <= levels - 2 ? finest + 1 : finest;
}

// ---- which shapes the marching tiles take; the plain forms take every other one ----
// 3-D, and a row holds at least 16 full 16-byte vectors: with fewer, three quarters of a wave's 64 lanes own no node and
// the one-thread-per-node form has more of the chip at work. One rule for the four files that have such a tile: level 0 of
// mg_o4.hip (launch_o4_*, radius 2), and the residual and the Jacobi sweep of mg_vc.hip (two marched fields), mg_bc.hip and
// mg_fas.hip (one) on every level, where every red-black colour pass and every transfer is plain too. Pure; each name is
// pinned by its family's tests/test_{o4,vc,bc,fas}_cpu.py.
inline bool march_ok(int dim, int nx, int ny, int nz, int elem_size)
{
    const int v = 16 / elem_size;
    return dim == 3 && nx / v >= 16 && ny >= 7 && nz >= 7;
}
inline bool o4_march_ok(int dim, int nx, int ny, int nz, int elem_size) { return march_ok(dim, nx, ny, nz, elem_size); }
inline bool vc_march_ok(int dim, int nx, int ny, int nz, int elem_size) { return march_ok(dim, nx, ny, nz, elem_size); }
inline bool bc_march_ok(int dim, int nx, int ny, int nz, int elem_size) { return march_ok(dim, nx, ny, nz, elem_size); }
inline bool fas_march_ok(int dim, int nx, int ny, int nz, int elem_size) { return march_ok(dim, nx, ny, nz, elem_size); }
// mg_vc_mixed.hip: the fp64 arrays decide (a lane owns one 16-byte vector of doubles), whatever the handle's element size
inline bool vc_mixed_march_ok(int dim, int nx, int ny, int nz) { return march_ok(dim, nx, ny, nz, 8); }

struct CoarseOut {
    int iters;
    int flag;
    double relres;
    double sumsq_rhs;
    double sumsq_r;
};

}  // namespace mg
#endif
