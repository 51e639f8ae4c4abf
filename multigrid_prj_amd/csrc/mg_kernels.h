// mg_kernels.h -- launchers of the hand-written gfx950 kernels (mg_kernels.hip,
// mg_jacobi_fast.hip). All launchers only enqueue on `s`; none synchronises.
#ifndef MG_KERNELS_H
#define MG_KERNELS_H

#include <hip/hip_runtime.h>
#include "mg_geom.h"
#include "mg_switches.h"

namespace mg {

// compute units of the current device, read once, rounded down to a multiple of 8 (one share per XCD), at least 8
inline int cu_count_x8()
{
    static const int ncu = [] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return std::max(8, (n / 8) * 8);
    }();
    return ncu;
}

// number of per-block partial sums a reduction launch over `g` may produce
int reduce_partials_capacity(const Geom &g);

// zero_u: the caller guarantees u == 0 everywhere (fresh coarse-level initial guess); the fast
// path then reads nothing of u. The generic path needs u to really hold zeros.
template <typename T>
void launch_jacobi(hipStream_t s, const Geom &g, const Coef<T> &c, T omega, const T *u,
                   const T *rhs, T *out, bool zero_u = false);

// finest-grid fast paths (mg_jacobi_fast.hip); launch_jacobi / launch_residual pick them
// automatically when fast_path_ok<T>(g)
template <typename T> bool fast_path_ok(const Geom &g);
template <typename T> int fast_partials_capacity(const Geom &g);
template <typename T>
void launch_jacobi_fast(hipStream_t s, const Geom &g, const Coef<T> &c, T omega, const T *u,
                        const T *rhs, T *out, bool zero_u);
// two Jacobi sweeps in one pass (out = J(J(u))), see mg_jacobi_fast.hip
template <typename T> bool jacobi2_ok(const Geom &g);
// d_partials != nullptr: also sum (rhs - A u)^2 of the INPUT u, where the wide-tile kernel runs (returns the number of partial
// sums written there, 0 = no norm was computed)
template <typename T>
int launch_jacobi2(hipStream_t s, const Geom &g, const Coef<T> &c, T omega, const T *u, const T *rhs, T *out,
                   bool zero_u = false, int dup_planes = 0, double *d_partials = nullptr);  // dup_planes > 0: the same geometry once more, that many planes further up, in the same launch
// z-slab of a distributed level: the pair on its inner planes (launch_jacobi2 with g = planes 1 .. nz-2), see pair_on_slab_t
template <typename T> bool jacobi2_slab_ok(const Geom &slab);
// the same with the V-cycle's prolong-add folded in: out = J(J(u + P coarse)); u is not modified
template <typename T> bool jacobi2_corr_ok(const Geom &gf, const Geom &gc);
template <typename T>
void launch_jacobi2_corr(hipStream_t s, const Geom &g, const Geom &gc, const Coef<T> &c, T omega, const T *u,
                         const T *coarse, const T *rhs, T *out, int dup_planes = 0);
// on the pieces of a z-slab: g = the piece, gc = the WHOLE coarse slab, coarse = its local plane 0 (two valid ghost planes either side)
template <typename T> bool jacobi2_corr_slab_ok(const Geom &gf, const Geom &gc);
// wide-tile form of the same pairs (mg_pair_wide.hip): rows of 128 / 256 lanes on levels big enough to fill the chip with
// 1024-thread workgroups; launch_jacobi2 / launch_jacobi2_corr / launch_rb_fused hand over to it when pair_wide_ok
// coarse != nullptr: out = pair(u + P coarse); zero_u: u == 0; rb: one red-black sweep instead of two Jacobi sweeps
template <typename T> bool pair_wide_ok(const Geom &g);
void set_pair_wide(int mode);   // measurement tools only (tools/pairbench.hip): 0 = never, 1 = wherever the shape allows, -1 = default
// d_partials != nullptr (plain Jacobi pair only): the launch also leaves one partial sum of (rhs - A u)^2 per workgroup
// there -- the residual norm of the pair's INPUT; returns how many (0: not computed)
template <typename T>
int launch_pair_wide(hipStream_t s, const Geom &g, const Geom &gc, const Coef<T> &c, T omega, const T *u, const T *coarse,
                     const T *rhs, T *out, bool zero_u, bool rb, int dup_planes, double *d_partials = nullptr);
// sum of n partial sums in a fixed order -> *d_out (mg_kernels.hip: k_reduce_final)
void launch_reduce_final(hipStream_t s, const double *d_partials, long long n, double *d_out);
// zebra line Gauss-Seidel along y: one colour pass; cp_den = the 2*ny factors of zebra_line_factors(cy, cd, ny) (device)
template <typename T>
void launch_zebra_y(hipStream_t s, const Geom &g, const Coef<T> &c, int colour, T *u, const T *rhs, T *dp,
                    const T *cp_den);
// the same with lines along x (k_zebra_x): cp_den = the 2*nx factors of zebra_line_factors(cx, cd, nx)
template <typename T>
void launch_zebra_x(hipStream_t s, const Geom &g, const Coef<T> &c, int colour, T *u, const T *rhs, T *dp,
                    const T *cp_den);
// elimination factors cp(j), den(j) of a line with off-diagonal cl and diagonal cd: out = 2 * n values (host)
template <typename T> void zebra_line_factors(T cl, T cd, int n, T *out);
// one whole red-black sweep in one pass (same gate as the fused double Jacobi sweep)
template <typename T> bool rb_fused_ok(const Geom &g);
template <typename T>
int launch_rb_fused(hipStream_t s, const Geom &g, const Coef<T> &c, const T *u, const T *rhs, T *out,
                    const T *coarse, const Geom &gc, int dup_planes = 0, bool zero_u = false, double *d_partials = nullptr);
// out-of-place colour half-sweep (the other colour is copied): red u->tmp, black tmp->u
template <typename T>
void launch_rb_fast(hipStream_t s, const Geom &g, const Coef<T> &c, int colour, const T *u, const T *rhs, T *out);
template <typename T>
int launch_residual_fast(hipStream_t s, const Geom &g, const Coef<T> &c, const T *u, const T *rhs,
                         T *r, double *d_partials, bool want_norm);

// 3-D prolongation fast path (mg_transfer_fast.hip)
template <typename T> bool prolong_fast_ok(const Geom &gc, const Geom &gf);
template <typename T>
void launch_prolong_fast(hipStream_t s, const Geom &gc, const Geom &gf, const T *coarse, T *fine, bool add);

// fused residual + full-weighting restriction (non-distributed 3-D levels): coarse = R (rhs - A u)
template <typename T> bool resid_restrict_fast_ok(const Geom &gf, const Geom &gc);
// the same launcher on a z-slab (two ghost planes of u and one of rhs below the slab must be valid)
template <typename T> bool resid_restrict_slab_ok(const Geom &gf, const Geom &gc);
template <typename T>
void launch_resid_restrict_fw(hipStream_t s, const Geom &gf, const Geom &gc, const Coef<T> &c, const T *u,
                              const T *rhs, T *coarse, int dup_kc = 0, int dup_nzf = 0);
// dup_kc > 0 (gc.nz must be 1): a second single coarse plane dup_kc coarse planes further up (its fine planes start 2 dup_kc
// further up and there are dup_nzf of them) in the same launch -- the two boundary pieces of a z-slab

// wide-tile form of the same operator (mg_rr_wide.hip): rows of 128 / 256 lanes; launch_resid_restrict_fw hands over to it
template <typename T> bool rr_wide_ok(const Geom &gf, const Geom &gc);
template <typename T>
void launch_rr_wide(hipStream_t s, const Geom &gf, const Geom &gc, const Coef<T> &c, const T *u, const T *rhs, T *coarse,
                    int dup_kc, int dup_nzf);
void set_rr_wide(int mode);   // measurement tools only: 0 = never, 1 = wherever the shape allows, -1 = default

// launch-bound levels (65^3 and below), V(2,2) Jacobi, whole 3-D levels (mg_small_levels.hip): the three launches either side
// of the coarser levels in one each -- u_out = J(J(0)), coarse = R(rhs - A u_out)  /  out = J(J(u + P e))
template <typename T> bool small_fused_ok(const Geom &gf, const Geom &gc);
template <typename T>
void launch_small_pre_rr(hipStream_t s, const Geom &gf, const Geom &gc, const Coef<T> &c, T omega, const T *rhs, T *u_out, T *coarse);
template <typename T>
void launch_small_prolong_post(hipStream_t s, const Geom &gf, const Geom &gc, const Coef<T> &c, T omega, const T *u, const T *e,
                               const T *rhs, T *out);

// one colour half-sweep of red-black Gauss-Seidel, in place
template <typename T>
void launch_rbgs_colour(hipStream_t s, const Geom &g, const Coef<T> &c, int colour, T *u,
                        const T *rhs);

// lexicographic Gauss-Seidel, one persistent workgroup, diagonal wavefronts
template <typename T>
void launch_gs_lex(hipStream_t s, const Geom &g, const Coef<T> &c, int sweeps, T *u,
                   const T *rhs);

// r = rhs - A u (r may be null), sum r^2 -> *d_sumsq (device double), two-pass
// deterministic reduction through d_partials
template <typename T>
void launch_residual(hipStream_t s, const Geom &g, const Coef<T> &c, const T *u, const T *rhs,
                     T *r, double *d_partials, double *d_sumsq);

template <typename T>
void launch_sumsq(hipStream_t s, const Geom &g, const T *v, double *d_partials, double *d_sumsq);

// coarse(K,J,I) = fine(2K,2J,2I)   (gc = coarse geometry, gf = fine geometry)
template <typename T>
void launch_inject(hipStream_t s, const Geom &gf, const Geom &gc, const T *fine, T *coarse);
template <typename T>
void launch_restrict_fw(hipStream_t s, const Geom &gf, const Geom &gc, const T *fine, T *coarse);

// fine = P coarse (add == false, overwrite) or fine += P coarse
template <typename T>
void launch_prolong(hipStream_t s, const Geom &gc, const Geom &gf, const T *coarse, T *fine,
                    bool add);

// u += e; e = 0
template <typename T>
void launch_correct(hipStream_t s, const Geom &g, T *u, T *e);

// Solver::Solve in one persistent workgroup; result vector ends in x
template <typename T>
void launch_coarse_solve(hipStream_t s, const Geom &g, const Coef<T> &c, T omega, int smoother,
                         T *x, T *tmp, const T *rhs, int maxit, double tol, int fixed,
                         CoarseOut *d_out, bool x_is_zero = false);

// ---- the one-launch LDS sub-cycle (mg_subcycle.hip, driven by Solver::subcycle_launch_t) ----
// One workgroup runs cyc(root, kind) of the V / W / F recursion (mg_desc.h) on the resident levels root .. levels - 1 --
// followed, when `second` is set, by the second visit of the root its parent makes (W: another W-cycle, F: a V-cycle) --
// out of LDS as mg::subcycle_plan laid it out. Index k is level root + k.
template <typename T>
struct SubcycleArgs {
    int nres;                                                   // resident levels
    int nx[SUBCYCLE_MAX_LEVELS], ny[SUBCYCLE_MAX_LEVELS], nz[SUBCYCLE_MAX_LEVELS];
    int off[SUBCYCLE_MAX_LEVELS][3];                            // byte offsets of u, t, b in dynamic LDS
    Coef<T> c[SUBCYCLE_MAX_LEVELS];
    Geom groot;                                                 // the root level as it lies in HBM
    T omega;
    int smoother;                                               // 1: Jacobi, 2: red-black
    int nu_pre, nu_post;
    int restriction;                                            // enum mg_restriction
    int kind;                                                   // MG_CYCLE_V / W / F
    int second;                                                 // the parent's second visit of the root too
    int u_zero;                                                 // U(root) starts from zero and is not read
    int maxit, fixed;                                           // the coarsest solve, as launch_coarse_solve takes them
    double tol;
    T *u;                                                       // U(root), local plane 0
    const T *rhs;                                               // RHS(root)
    CoarseOut *out;                                             // iterations summed, flags or-ed, the last solve's norms
};
// false: the runtime refused the kernel its LDS (nothing was launched)
template <typename T>
bool launch_subcycle(hipStream_t s, const SubcycleArgs<T> &a, int dim, size_t lds_bytes);
// acc += cur as mg_cycle_stats reports a W / F cycle (one thread)
void launch_coarse_accum(hipStream_t s, CoarseOut *acc, const CoarseOut *cur);

// ---- flexible conjugate gradients on level 0 (mg_krylov.hip, driven by Solver::pcg_t) ----
// Scalars of the iteration, resident on the device: the tails write them, the vector kernels read them. bad != 0 (a
// breakdown: gamma <= 0, p.q <= 0 or a scalar that is not finite) makes every later launch return without writing.
struct CgScalars {
    double rr;      // r.r after the last update
    double gamma;   // z.r
    double delta;   // z.q
    double beta;
    double alpha;
    double pq;      // p.q
    int bad;
    int pad_;
};
enum CgTail {
    CG_TAIL_RR = 0,     // partials of r.r                -> rr
    CG_TAIL_FIRST = 1,  // partials of z.r, z.q (k = 0)   -> gamma, beta = 0
    CG_TAIL_BETA = 2,   // partials of z.r, z.q           -> beta = -alpha delta / gamma_old, gamma
    CG_TAIL_ALPHA = 3   // partials of p.q                -> alpha = gamma / p.q
};
int cg_partials_capacity();   // doubles the partials buffer of the three kernels needs
// x += a p, r -= a q (a = alpha); partials of r.r; returns the number of partials
template <typename T>
int launch_cg_update(hipStream_t s, const Geom &g, T *x, const T *p, T *r, const T *q, const CgScalars *sc, double *partials);
// partials of z.r in [0, nb), of z.q in [nb, 2 nb); returns nb
template <typename T>
int launch_cg_dots(hipStream_t s, const Geom &g, const T *z, const T *r, const T *q, const CgScalars *sc, double *partials);
// pn = z + b p (b = beta; 0 on Dirichlet nodes), q = A pn, partials of pn.q; pn must not alias p
template <typename T>
int launch_cg_direction_apply(hipStream_t s, const Geom &g, const Coef<T> &c, const T *z, const T *p, T *pn, T *q,
                              const CgScalars *sc, double *partials);
// x = rhs on the Dirichlet nodes, the rest of x untouched
template <typename T>
void launch_cg_boundary_copy(hipStream_t s, const Geom &g, T *x, const T *rhs);
// fixed-order sum of the partials of one launch above + the scalar update `mode` (CgTail), one workgroup
void launch_cg_tail(hipStream_t s, int mode, const double *partials, int nb, CgScalars *sc);

// ---- block kernels of the LOBPCG eigensolver on level 0 (mg_eig.hip, driven by Solver::eig_t) ----
constexpr int EIG_GRAM_ROWS = 12;      // one Gram tile: up to 12 row vectors ...
constexpr int EIG_GRAM_COLS = 4;       // ... against up to 4 column vectors and their images under A
constexpr int EIG_MAX_BLOCKS = 1024;   // workgroups of a launch = partial sums per accumulator
constexpr int EIG_MAX_COLS = 8;        // MG_EIG_MAX_BLOCK
template <typename T>
struct EigGramArgs {
    const T *row[EIG_GRAM_ROWS];
    T *col[EIG_GRAM_COLS];             // b
    T *acol[EIG_GRAM_COLS];            // A b: read, or with the apply written (col is then set to 0 on Dirichlet nodes)
    int na, nb;                        // rows / columns in use; the entries beyond them must repeat a used pointer (the kernel
                                       // loads all of them without a branch and ignores what it got)
    unsigned row_interior;             // bit r: row r is read as 0 on Dirichlet nodes whatever it holds there (the W family)
    int col_interior;                  // the same for the columns of a launch without the apply
};
// The operator of the block kernels (enum mg_eig_operator, MG_EIG_OPERATOR): EIG_OP_CONSTANT is the handle's constant stencil with every face
// Dirichlet and looks at nothing else here. EIG_OP_FACES: the constant stencil with the faces of `mask` Neumann (mg_bc.hip's
// node classes and mirrors). EIG_OP_COEFFICIENT: mg_vc.hip's operator from the level-0 coefficient array a with w_a =
// (T)(-c_a / 2), sigma = (T)shift and the faces of `mask`. With the last two every product of a Gram sum and every r^2 of
// the combine carries the node's weight (1/2 per face of the mask it lies on).
enum { EIG_OP_CONSTANT = 0, EIG_OP_FACES = 1, EIG_OP_COEFFICIENT = 2 };
template <typename T>
struct EigOp {
    int kind, mask;
    T wx, wy, wz, sigma;
    const T *a;
};
// One tile: partials[(r * EIG_GRAM_COLS + j) * nblocks + block] of row[r] . col[j], and EIG_GRAM_ROWS * EIG_GRAM_COLS
// entries further on the same of row[r] . acol[j]. apply: acol[j] = A col[j] is made (and stored) instead of read.
// Every array is level-shaped with a ghost plane either side (the apply reads the neighbours of boundary nodes too and
// zeroes them afterwards). Returns nblocks.
template <typename T>
int launch_eig_gram(hipStream_t s, const Geom &g, const Coef<T> &c, const EigOp<T> &op, const EigGramArgs<T> &a, bool apply,
                    double *partials);
template <typename T>
struct EigCombineArgs {
    const T *s[3 * EIG_MAX_COLS], *as[3 * EIG_MAX_COLS];   // S = [X, W, P] and AS = [AX, AW, AP] in column order
    T *x[EIG_MAX_COLS], *ax[EIG_MAX_COLS], *r[EIG_MAX_COLS], *p[EIG_MAX_COLS], *ap[EIG_MAX_COLS];   // outputs (they alias inputs)
    int m, nw, np;
    int mask;   // weighted: the sums of r^2 carry the weights of this face mask (the arrays are the same bits either way)
    bool weighted;
};
// x_j = S Cx, ax_j = AS Cx (j < m), p_j = [W, P] Cp, ap_j = [AW, AP] Cp (j < nw), r_j = ax_j - theta_j x_j; coef (device) =
// Cx (s x m) followed by Cp ((nw + np) x nw), row-major; partials[j * nblocks + block] of r_j^2. Returns nblocks.
template <typename T>
int launch_eig_combine(hipStream_t s, const Geom &g, const EigCombineArgs<T> &a, const double *coef, const double *theta,
                       double *partials);
// out[k] = the sum of partials[k * nb .. (k + 1) * nb) in a fixed order, k < nsums
void launch_eig_reduce(hipStream_t s, const double *partials, int nb, int nsums, double *out);
// the default start vector of column `column`: a hash of the node's global index, uniform in [-1, 1), 0 on Dirichlet nodes
template <typename T>
void launch_eig_fill(hipStream_t s, const Geom &g, T *x, int column);

// ---- full-multigrid interpolation (mg_fmg.hip, driven by Solver::fmg_t) ----
// fine = Pi coarse: cubic along every coarsened axis (one-sided quadratic next to a boundary), kept axes copied;
// bnd != nullptr: fine Dirichlet nodes = bnd[node] instead, in the same launch. Whole (undistributed) levels only.
template <typename T> bool fmg_prolong_fast_ok(const Geom &gc, const Geom &gf);   // the streaming 3-D form runs (else the gather kernel)
template <typename T>
void launch_fmg_prolong(hipStream_t s, const Geom &gc, const Geom &gf, const T *coarse, T *fine, const T *bnd, int mask = 0);
// mask (enum mg_face) != 0: the faces in it are Neumann faces -- the coarse rows are mirrored there, the odd node next to such
// an end takes the cubic rule, and bnd goes to the fine nodes on at least one face that is not in the mask. mask 0 launches
// the mask-free instantiations: the same code, registers and bits as before the mask existed.

// ---- mixed-precision defect correction on level 0 (mg_mixed.hip, driven by Solver::mixed_solve) ----
// g64 / g32: the fp64 and the fp32 geometry of level 0 (same extents, different pitches); coef = {cx, cy, cz, cd} in fp64.
// Each launch leaves one partial sum per workgroup in `partials` and returns how many (at most mixed_partials_capacity()).
int mixed_partials_capacity();
// r32 = (float)(scale_out * (b - A u)), 0 on Dirichlet nodes; partials of (b - A u)^2
int launch_mixed_residual(hipStream_t s, const Geom &g64, const Geom &g32, const double coef[4], const double *u, const double *b,
                          float *r32, double scale_out, double *partials);
// u_out = u + (double)e32 / scale_in inside, u on Dirichlet nodes; then the same residual of u_out. u_out must not alias u.
int launch_mixed_correct_residual(hipStream_t s, const Geom &g64, const Geom &g32, const double coef[4], const double *u,
                                  const float *e32, const double *b, double *u_out, float *r32, double scale_in, double scale_out,
                                  double *partials);
// partials of v^2 over all nodes
int launch_mixed_sumsq(hipStream_t s, const Geom &g64, const double *v, double *partials);

// ---- the same two kernels on mg_vc_*'s operator (mg_vc_mixed.hip; MG_MIXED_ON_COEFFICIENT) ----
// coef = the level's mg_level_coefficients, sigma the shift, mask the Neumann faces, a32 the handle's fp32 level-0 coefficient
// (its fp64 image is the operator's). e32 == nullptr: the first residual, r32 = (float)(scale_out * (b - L u)), 0 on the mask's
// Dirichlet nodes; otherwise u_out = u + (double)e32 / scale_in at the mask's unknowns (u on its Dirichlet nodes; u_out must not
// alias u) and the same residual of u_out. The marching tile where vc_mixed_march_takes and its grid fits `cap` partial sums,
// the plain form (one thread per node) otherwise. -> the number of partial sums left in `partials`.
bool vc_mixed_march_takes(const Geom &g64, bool plain);
int launch_vc_mixed(hipStream_t s, const Geom &g64, const Geom &g32, const double coef[4], double sigma, int mask, const double *u,
                    const float *e32, const float *a32, const double *b, double *u_out, float *r32, double scale_in, double scale_out,
                    double *partials, int cap, bool plain);

// ---- implicit heat-equation stepper on level 0 (mg_heat.hip, driven by Solver::heat_step) ----
// out = right-hand side of one theta-scheme step built from u (and the source f; nullptr: f = 0): on interior nodes
// ((f + u / dt) - (1 - theta) A0 u) / theta with coef0 = {cx, cy, cz, cd0}, the UNSHIFTED operator of the level in fp64
// (cast to T here); out = u on Dirichlet nodes. out must not alias u or f.
template <typename T>
void launch_heat_rhs(hipStream_t s, const Geom &g, const double coef0[4], double dt, double theta, const T *u, const T *f, T *out);

// ---- fourth-order defect correction on level 0 (mg_o4.hip, driven by Solver::o4_solve) ----
// w = {cx, cy, cz} / 12 of level 0 in fp64 and the handle's shift sigma (both cast to T here). Each launch leaves one partial
// sum of r^2 per workgroup in `partials` (room for `cap`) and returns how many. The marching tile runs where
// o4_march_ok (mg_geom.h), the plain form elsewhere.
// r = b - (sigma I + A4) u on interior nodes, 0 on Dirichlet nodes; r == nullptr: norm only
template <typename T>
int launch_o4_residual(hipStream_t s, const Geom &g, const double w[3], double sigma, const T *u, const T *b, T *r,
                       double *partials, int cap);
// u_out = u + e on interior nodes, u on Dirichlet nodes (e is not looked at there); then the same residual of u_out.
// u_out must not alias u.
template <typename T>
int launch_o4_correct_residual(hipStream_t s, const Geom &g, const double w[3], double sigma, const T *u, const T *e, const T *b,
                               T *u_out, T *r, double *partials, int cap);

// ---- variable-coefficient operator (mg_vc.hip, driven by Solver::vc_*) ----
// coef = {cx, cy, cz, cd} of the level in fp64 (cd is not used: the diagonal is built from a), sigma the handle's shift; a:
// the level's coefficient array (level-shaped, ghost planes and padding zero). plain: never the marching tile. mask: the
// Neumann faces (enum mg_face; mg_vc_set_faces): missing neighbours are mirror images, for a and u alike, and the Dirichlet
// nodes are those on a face outside the mask; 0 launches the kernels a handle without a mask has always run.
// react, G: the pointwise reaction G g(u) added to the operator (MG_FAS_ON_COEFFICIENT: mg_fas_* on this operator) -- react =
// FAS_CUBIC / FAS_EXP (enum mg_fas_kind), or FAS_LINEAR: no reaction (G is not looked at), the launches and instantiations
// of mg_vc_*. With a reaction the point solve is one Newton step on the node's own equation (mg_fas.hip's contract).
enum { FAS_LINEAR = -1, FAS_CUBIC = 0, FAS_EXP = 1 };
// r = b - L u (r == nullptr: norm only); one partial sum of r^2 per workgroup in `partials` (room for `cap`), returns how many
template <typename T>
int launch_vc_residual(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, int react, T G, const T *u, const T *a,
                       const T *b, T *r, double *partials, int cap, bool plain);
// one Jacobi sweep, out of place (out must not alias u)
template <typename T>
void launch_vc_jacobi(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, int react, T G, T omega, const T *u,
                      const T *a, const T *b, T *out, bool plain);
// launch_heat_rhs with the UNSHIFTED operator -div(a grad .) (coef's cd and the handle's shift are not used): out = right-hand
// side of one theta step from u (and the source f; nullptr: f = 0), u on Dirichlet nodes. out must not alias u, a or f.
template <typename T>
void launch_vc_heat_rhs(hipStream_t s, const Geom &g, const double coef[4], int mask, int react, T G, double dt, double theta, const T *u,
                        const T *a, const T *f, T *out, bool plain);
// one colour pass of red-black Gauss-Seidel, in place
template <typename T>
void launch_vc_rb_colour(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, int react, T G, int colour, T *u,
                         const T *a, const T *b);
// launch_coarse_solve's loop with the vc sweep (smoother 1: Jacobi, 2: red-black) and the vc residual, one workgroup
template <typename T>
void launch_vc_coarse(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, int react, T G, T omega, int smoother,
                      T *x, T *tmp, const T *rhs, const T *a, int maxit, double tol, int fixed, CoarseOut *d_out);
// the FAS transition on this operator (launch_fas_coarse_rhs with the coarse level's coefficient array ac and its coef): uc = ec
// = uf injected, rhsc = R rf + ((d_c uc - s_c) + G g(uc)) with s_c, d_c from ac at the coarse node and its coarse neighbours and
// the u neighbours read from uf at distance 2 (z: 1 on a semi transition), mirrored for a and u alike on the faces of the mask;
// R is the mirrored full weighting with a mask, full weighting without, or the injection; coarse Dirichlet nodes: uc.
// react is FAS_CUBIC or FAS_EXP.
template <typename T>
void launch_vc_fas_coarse_rhs(hipStream_t s, const Geom &gf, const Geom &gc, const double coefc[4], double sigma, int mask, int react, T G,
                              bool inject, const T *uf, const T *rf, const T *ac, T *uc, T *ec, T *rhsc);
// launch_cg_direction_apply with q = L pn; partials of pn.q (at most cg_partials_capacity() / 2), returns how many. With a
// mask pn and q are 0 on ITS Dirichlet nodes and the partials are those of sum w pn q, w = 1/2 per Neumann face of the node
template <typename T>
int launch_vc_cg_direction(hipStream_t s, const Geom &g, const double coef[4], double sigma, int mask, const T *z, const T *p, const T *a,
                           T *pn, T *q, const CgScalars *sc, double *partials);
// launch_cg_dots with the weights of the mask: partials of sum w z r, then of sum w z q
template <typename T>
int launch_vc_cg_wdots(hipStream_t s, const Geom &g, int mask, const T *z, const T *r, const T *q, const CgScalars *sc, double *partials);

// ---- the constant operator with Neumann faces (mg_bc.hip, driven by Solver::bc_*) ----
// c: the level's Coef (shift included); mask: the Neumann faces (enum mg_face), 0 = the existing kernels' results bit for
// bit. plain: never the marching tile.
// r = b - L u (r == nullptr: norm only); one partial sum of r^2 per workgroup in `partials` (room for `cap`), returns how many
template <typename T>
int launch_bc_residual(hipStream_t s, const Geom &g, const Coef<T> &c, int mask, const T *u, const T *b, T *r, double *partials, int cap,
                       bool plain);
// one Jacobi sweep, out of place (out must not alias u)
template <typename T>
void launch_bc_jacobi(hipStream_t s, const Geom &g, const Coef<T> &c, int mask, T omega, const T *u, const T *b, T *out, bool plain);
// launch_heat_rhs with Neumann faces; c0: the level's Coef with the UNSHIFTED diagonal cd0. out = u on the Dirichlet nodes of
// the mask; theta == 1 loads no neighbour. out must not alias u or f.
template <typename T>
void launch_bc_heat_rhs(hipStream_t s, const Geom &g, const Coef<T> &c0, int mask, double dt, double theta, const T *u, const T *f, T *out,
                        bool plain);
// one colour pass of red-black Gauss-Seidel, in place
template <typename T>
void launch_bc_rb_colour(hipStream_t s, const Geom &g, const Coef<T> &c, int mask, int colour, T *u, const T *b);
// full weighting with fine neighbours mirrored on the Neumann faces, coarse Dirichlet nodes injected
template <typename T>
void launch_bc_restrict_fw(hipStream_t s, const Geom &gf, const Geom &gc, int mask, const T *fine, T *coarse);
// launch_coarse_solve's loop with the bc sweep (smoother 1: Jacobi, 2: red-black) and the bc residual, one workgroup
template <typename T>
void launch_bc_coarse(hipStream_t s, const Geom &g, const Coef<T> &c, int mask, T omega, int smoother, T *x, T *tmp, const T *rhs,
                      int maxit, double tol, int fixed, CoarseOut *d_out);
// partial sums of w v, w = 1/2 per Neumann face the node lies on (room for `cap`), returns how many
template <typename T>
int launch_bc_wsum(hipStream_t s, const Geom &g, int mask, const T *v, double *partials, int cap);
// v -= cval on every node
template <typename T>
void launch_bc_shift(hipStream_t s, const Geom &g, T cval, T *v);
// x = rhs on the Dirichlet nodes of the mask
template <typename T>
void launch_bc_dirichlet_copy(hipStream_t s, const Geom &g, int mask, T *x, const T *rhs);

// ---- the semilinear operator (sigma I + A) u + gamma g(u) of the full approximation scheme (mg_fas.hip, Solver::fas_*) ----
// c: the level's Coef (shift included); kind: enum mg_fas_kind; G = (T)gamma, 0 = the constant kernels' results bit for bit.
// plain: never the marching tile. mask: the Neumann faces (enum mg_face) of MG_FAS_ON_FACES -- the linear part is mg_bc.hip's
// operator with this mask; 0: all faces Dirichlet, the launches and kernel instantiations of a handle without the flag.
// r = b - N(u) (r == nullptr: norm only); one partial sum of r^2 per workgroup in `partials` (room for `cap`), returns how many
template <typename T>
int launch_fas_residual(hipStream_t s, const Geom &g, const Coef<T> &c, int kind, T G, int mask, const T *u, const T *b, T *r,
                        double *partials, int cap, bool plain);
// one Jacobi sweep of linearised point solves, out of place (out must not alias u)
template <typename T>
void launch_fas_jacobi(hipStream_t s, const Geom &g, const Coef<T> &c, int kind, T G, int mask, T omega, const T *u, const T *b, T *out,
                       bool plain);
// launch_heat_rhs with N0(u) = A0 u + G g(u); c0: the level's Coef with the UNSHIFTED diagonal cd0. out must not alias u or f.
template <typename T>
void launch_fas_heat_rhs(hipStream_t s, const Geom &g, const Coef<T> &c0, int kind, T G, int mask, double dt, double theta, const T *u,
                         const T *f, T *out, bool plain);
// one colour pass of red-black Gauss-Seidel with the linearised point solve, in place
template <typename T>
void launch_fas_rb_colour(hipStream_t s, const Geom &g, const Coef<T> &c, int kind, T G, int mask, int colour, T *u, const T *b);
// the FAS transition: uc = ec = uf injected, rhsc = R rf + N_c(uf injected) (cc: Coef of the coarse level; inject: R is the injection;
// with a mask R is launch_bc_restrict_fw's mirrored full weighting and N_c mirrors its coarse neighbours)
template <typename T>
void launch_fas_coarse_rhs(hipStream_t s, const Geom &gf, const Geom &gc, const Coef<T> &cc, int kind, T G, int mask, bool inject,
                           const T *uf, const T *rf, T *uc, T *ec, T *rhsc);
// e = x - e on every node
template <typename T>
void launch_fas_diff(hipStream_t s, const Geom &g, const T *x, T *e);
// launch_coarse_solve's loop with the nonlinear sweep (smoother 1: Jacobi, 2: red-black) and the nonlinear residual, one workgroup
template <typename T>
void launch_fas_coarse(hipStream_t s, const Geom &g, const Coef<T> &c, int kind, T G, int mask, T omega, int smoother, T *x, T *tmp,
                       const T *rhs, int maxit, double tol, int fixed, CoarseOut *d_out);

// ---- device-resident array I/O (mg_io.hip, driven by Solver::device_copy) ----
// padded: local plane 0 of a level-shaped array of geometry g with elements P; dense: the caller's dense device array of
// g.nx * g.ny * g.nz elements D at any element-aligned address. to_padded: padded = (P)dense, padding columns written as
// zeros (the value they hold: mg_geom.h -- padding is only ever written with zeros, here, by the tail-line stores and by the
// line store of mg_fmg.hip); otherwise dense = (D)padded and no byte outside the dense array is written. Ghost planes are
// not touched.
template <typename P, typename D>
void launch_io_copy(hipStream_t s, const Geom &g, P *padded, D *dense, bool to_padded);

}  // namespace mg
#endif
