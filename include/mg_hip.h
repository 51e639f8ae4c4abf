/*
 * mg_hip.h -- C-ABI of the MI355X-native geometric-multigrid hot path (libmg_hip.so).
 *
 * The reference (Stefo01/multigrid_prj, GeometricMultigrid/) has no FFI: its
 * boundary is a set of C++ operator classes applied to std::vector<double> with
 * `x * Op`.  This header is the plain-C boundary a maintainer binds
 * instead; each entry point names the reference interface it replaces (paths
 * relative to /root/reference/GeometricMultigrid/).  The C++ mirror of the
 * reference classes that sits on top of it is include/multigrid_hip.hpp, the
 * ctypes binding is multigrid_prj_amd/capi.py.
 *
 * Conventions: every function returns 0 on success or a negative mg_status and
 * records a message retrievable with mg_last_error(); no exception crosses the
 * ABI.  The library owns all device memory; the caller owns all host buffers.
 * One handle <-> one host thread. Work is enqueued on a HIP stream owned by the
 * handle; functions that return scalars or copy to host synchronise that stream.
 * There is NO CPU fallback: without a HIP device mg_create fails with
 * MG_ERR_NO_DEVICE.
 *
 * Host arrays are dense and contiguous: 2-D a[j*n+i] (j = reference row, i.e.
 * y = length - j*h; i = column), 3-D a[(k*n+j)*n+i]; element type = desc.dtype.
 */
#ifndef MG_HIP_H
#define MG_HIP_H

#include <stddef.h>
#include "mg_desc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg_solver *mg_handle;

enum mg_status {
    MG_OK = 0,
    MG_ERR_INVALID_DESC = -1,  /* see mg_last_error(); includes n/levels mismatch the
                                  reference silently mis-handles            */
    MG_ERR_NO_DEVICE = -2,
    MG_ERR_HIP = -3,
    MG_ERR_BAD_ARG = -4,
    MG_ERR_COMM = -5
};

/* device arrays of one level, addressable by tests and by the C++ mirror */
enum mg_array {
    MG_ARR_U = 0,   /* level 0: solution `u` (main.cpp:49); V-cycle: u_l on every level  */
    MG_ARR_E = 1,   /* sawtooth error `err` (multigrid.hpp:96), one dense array per level */
    MG_ARR_RHS = 2, /* level 0: `fvec` (main.cpp:45); l>0: restricted residual           */
    MG_ARR_TMP = 3, /* Jacobi `temp` (solvers.hpp:58) / residual scratch                 */
    MG_ARR_RES = 4  /* level 0 only: `res` (multigrid.hpp:95)                            */
};

const char *mg_last_error(void);
int mg_device_count(int *count);

/* SquareDomain + PoissonMatrix hierarchy (main.cpp:32-41) and the operator objects of
 * SawtoothMGIteration's constructor (multigrid.hpp:108-124), resident in HBM.
 * device < 0 selects the current HIP device. */
int mg_create(const mg_desc *desc, int device, mg_handle *out);
int mg_destroy(mg_handle h);

/* SquareDomain::getWidth() of level l (domain.hpp:82, domain.cpp:9-12) */
int mg_level_n(mg_handle h, int level, int *n);
/* number of z-planes this rank holds of level l (1 in 2-D; the local slab when distributed;
 * with semi-coarsening every level keeps the finest grid's z resolution) */
int mg_level_nz(mg_handle h, int level, int *nz);
/* PoissonMatrix coefficients of level l: out = {cx, cy, cz, cd}
 * (linear_system.hpp:17,27-28,37-38) */
int mg_level_coefficients(mg_handle h, int level, double out[4]);

/* DataVector (linear_system.hpp:85-92) is assembled by the caller on the host;
 * these move dense host arrays to/from the padded device layout. */
int mg_set_rhs(mg_handle h, const void *host_b);            /* == set_array(RHS, 0) */
int mg_set_solution(mg_handle h, const void *host_u);       /* == set_array(U, 0)   */
int mg_get_solution(mg_handle h, void *host_u);
int mg_set_array(mg_handle h, int which, int level, const void *host);
int mg_get_array(mg_handle h, int which, int level, void *host);
int mg_zero_array(mg_handle h, int which, int level);

/* Device-resident array I/O (extension): the same arrays from / into a dense array that already lives in HBM -- a torch
 * tensor, the output of the caller's own kernels -- ordered against a stream the caller names, with NO host
 * synchronisation. One streaming kernel (multigrid_prj_amd/csrc/mg_io.hip) converts between the dense layout and the
 * library's 128-byte-pitched one, and between fp64 and fp32.
 * Array: `dev` is device memory of the handle's device holding a dense, contiguous array in the host layout above
 * (a[j*n+i], a[(k*n+j)*n+i]) with the extents mg_set_array uses for that handle and level (a distributed handle: the
 * rank's own planes). dtype = MG_F64 or MG_F32 is the type of ITS elements and need not be desc.dtype: values are converted
 * element by element -- double -> float rounds to nearest even (overflow: +-inf, NaN stays NaN), float -> double is exact;
 * with equal types every bit pattern survives (NaN payloads, -0.0). The address needs only element alignment: a slice
 * that starts in the middle of a larger buffer is admissible. On a get no byte outside the array is written.
 * Stream: the caller's hipStream_t passed as void * (this header stays plain C); NULL = the device's default stream. It
 * must belong to the handle's device and must not be capturing a graph.
 * Ordering (two events owned by the handle, no timing): the copy runs on the HANDLE's stream
 *   - after everything already enqueued on `stream` (set: the kernels that produce the array; get: those that still read it)
 *     and, being on the handle's stream, after everything already enqueued on the handle (a preceding mg_cycle_async);
 *   - before everything enqueued on `stream` after the call. After a set the caller may therefore overwrite or free the
 *     array in stream order as soon as the call returns (a caching allocator needs exactly this); after a get, work
 *     enqueued on `stream` sees the data. Host code synchronises `stream`, or calls mg_sync, before it reads the array.
 * Side effects are mg_set_array's: ghost planes are not touched, padding columns keep the value zero.
 * mg_heat_set_source_device and the mg_mixed_*_device calls (declared beside their host twins below) keep every rule of
 * those twins -- when arrays are allocated, what mg_device_bytes counts, which handles are refused -- with the array
 * passed as here; the mixed arrays may be MG_F32 (converted exactly into the fp64 u / b, rounded on the way out).
 * MG_ERR_BAD_ARG, decided before anything is enqueued or allocated, handle and array untouched: NULL handle; unknown
 * which, level or dtype; NULL dev (except mg_heat_set_source_device: f = 0 again); a pointer that is not aligned to its
 * element type; a pointer that HIP does not report as device memory of the handle's device (host, managed, another
 * device); an allocation that ends before the dense array does, or whose extent hipMemGetAddressRange cannot report
 * (memory of a stream-ordered pool -- hipMallocAsync -- may fall under this: pass memory of hipMalloc, which is what
 * torch's default caching allocator hands out).
 * Any other failure (MG_ERR_HIP from a HIP call) leaves the ordering as documented: once the copy is enqueued, the second
 * hand-over is made before the error is returned. */
int mg_set_array_device(mg_handle h, int which, int level, const void *dev, int dtype, void *stream);
int mg_get_array_device(mg_handle h, int which, int level, void *dev, int dtype, void *stream);

/* `x * smoother` `sweeps` times on level l:  A_l x = rhs
 *   MG_SMOOTH_JACOBI -> Jacobi_iteration::apply_iteration_to_vec  solvers.hpp:64-83
 *   MG_SMOOTH_GS_LEX -> Gauss_Seidel_iteration::…                 solvers.hpp:33-48
 *   MG_SMOOTH_RBGS   -> red-black GS (extension)
 *   MG_SMOOTH_ZEBRA_Y / MG_SMOOTH_ZEBRA_X -> zebra line GS along y / along x (extension; only on a handle created
 *                        with that smoother, which tabulates the line factors per level)
 * arr_x / arr_rhs name which device arrays play x and rhs. */
int mg_smooth(mg_handle h, int level, int smoother, int sweeps, int arr_x, int arr_rhs);

/* `x * RES`: Residual::apply_iteration_to_vec solvers.hpp:257-295. arr_r < 0 is the
 * non-saving branch (:277-294). *sumsq_r = sum r^2 (the member `norm`). */
int mg_residual(mg_handle h, int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r);
/* Residual::refresh_normalization_constant solvers.hpp:244-254 */
int mg_sumsq(mg_handle h, int level, int arr, double *sumsq);

/* level l -> l+1. kind MG_RESTRICT_INJECT is what the reference does implicitly by
 * building every level on `res` through mask() (multigrid.hpp:113,121; domain.hpp:78-80) */
int mg_restrict(mg_handle h, int fine_level, int kind, int arr_src, int arr_dst);
/* level l -> l-1: InterpolationClass::interpolate src/multigrid.cpp:3-27 (add == 0,
 * overwrite); add != 0 is the V-cycle's fine += P coarse (extension) */
int mg_prolong(mg_handle h, int coarse_level, int add, int arr_src, int arr_dst);
/* sol += err; err = 0 on the finest grid, multigrid.hpp:141-144 */
int mg_correct(mg_handle h, int arr_u, int arr_e);
/* Solver::Solve on `level` (solvers.hpp:324-342 as instantiated at multigrid.hpp:123),
 * one persistent workgroup; honours desc.coarse_{mode,maxit,tol}, desc.smoother */
int mg_coarse_solve(mg_handle h, int level, int arr_x, int arr_rhs, mg_cycle_stats *st);
/* the same with the Solver constructor's arguments (smoother, maxit, tol) given per call
 * instead of taken from the descriptor; fixed != 0 runs exactly maxit sweeps */
int mg_coarse_solve_ex(mg_handle h, int level, int arr_x, int arr_rhs, int smoother, int maxit,
                       double tol, int fixed, mg_cycle_stats *st);

/* SawtoothMGIteration::apply_iteration_to_vec multigrid.hpp:126-145 (or the V-cycle
 * extension, per desc.cycle) applied to the solution array U of level 0 */
int mg_cycle(mg_handle h, mg_cycle_stats *st);
/* enqueue `count` cycles without any host synchronisation (benchmark path) */
int mg_cycle_async(mg_handle h, int count);
/* outer loop of main.cpp:72-116; hist[0] = initial relative residual; *n_hist = entries
 * produced (also counted when hist_cap is too small); per_cycle may be NULL */
int mg_solve(mg_handle h, double tol, int maxit, double *hist, int hist_cap, int *n_hist,
             mg_cycle_stats *per_cycle);

/* Lock-step parity mode: mg_solve with the coarse Solver's stopping test taken out of the
 * comparison. Solver::Solve (solvers.hpp:324-342) stops on `Norm() > 0.1`, so a last-bit difference in a
 * sum of squares can move the stop by one sweep and everything after it in the 3rd-4th digit. Here the
 * coarse solve of outer iteration i spends exactly coarse_counts[i] sweeps -- the counts a reference run
 * spent (tests/golden/ref_solve.json) -- so that every kernel of the solve can be held to the
 * reference's numbers tightly. Iterations beyond n_counts run free, like mg_solve. */
int mg_solve_lockstep(mg_handle h, double tol, int maxit, const int *coarse_counts, int n_counts,
                      double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle);

/* Multigrid-preconditioned conjugate gradients (extension; the reference's Krylov option `-smt 2`, BiCGSTAB, is
 * never applied by its program). Solves A x = b on level 0, b = the RHS array, x0 = the U array (mg_solve's
 * contract), with flexible CG -- Notay's FCG(1), the Polak-Ribiere beta:
 *   x0 = b on the Dirichlet nodes;  r0 = b - A x0;  z0 = M r0;  p0 = z0;  gamma0 = z0.r0
 *   for k = 0, 1, ...:  q = A p;  alpha = gamma / p.q;  x += alpha p;  r -= alpha q;  stop if ||r|| / ||b|| <= tol
 *                       z = M r;  gamma' = z.r;  beta = -alpha (z.q) / gamma;  gamma = gamma';  p = z + beta p
 * M r is one outer iteration of mg_solve started from zero on A z = r: desc.outer_pre_gs lexicographic Gauss-Seidel
 * sweeps, then one mg_cycle of the descriptor's kind. The flexible beta makes every cycle the library builds an
 * admissible preconditioner (red-black sweeps in the same colour order, the sawtooth, the residual-tested coarse solve
 * are not symmetric linear operators); with a symmetric M it equals standard PCG in exact arithmetic.
 * hist[k] = sqrt(r_k.r_k / b.b) with the recursively updated r (hist[0]: after the boundary copy, mg_solve's hist[0]
 * when U already holds b's boundary values); the loop stops when k > 0 and hist[k] <= tol, after maxit iterations, or
 * on a breakdown (p.q <= 0, gamma <= 0 or a scalar that is not finite: status 2, x = the last iterate, never NaN).
 * Dot products accumulate in double for both dtypes, in a fixed order: two runs give the same bits. b.b == 0 or
 * r0 == 0: nothing to do (status 0, iters 0).
 * On return U holds x and RHS holds b unchanged; E, TMP, RES and the coarse levels are unspecified (as after mg_solve).
 * Memory: the first call allocates five more level-0 arrays (z, r, two directions, A p) kept until mg_destroy and
 * counted by mg_device_bytes from then on -- 5 x 1.1 GB at 513^3 fp64, 5 x 4.4 GB at 1025^3 fp32.
 * Refused with MG_ERR_BAD_ARG (U untouched): distributed handles (nranks > 1, dry runs included) and a handle with
 * a stage callback installed. mg_profile_* brackets keep timing the cycles inside. */
typedef struct mg_krylov_stats {
    int32_t iters;        /* CG iterations done (= preconditioner applications after the first) */
    int32_t status;       /* 0 converged, 1 hit maxit, 2 breakdown                               */
    double  relres;       /* last recursive ||r|| / ||b||                                         */
    double  relres_true;  /* ||b - A x|| / ||b|| recomputed at exit                               */
} mg_krylov_stats;
int mg_pcg_solve(mg_handle h, double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_krylov_stats *st);

/* Kernel-level check of mg_pcg_solve's three vector kernels on level-0 arrays (arrs[] name mg_array slots; the
 * element-wise formulas are in multigrid_prj_amd/csrc/mg_krylov.hip):
 *   MG_PCG_K_UPDATE     arrs = {x, p, r, q}:   x += scalar p,  r -= scalar q;       dots[0] = r.r (after)
 *   MG_PCG_K_DOTS       arrs = {z, r, q}:      dots[0] = z.r,  dots[1] = z.q
 *   MG_PCG_K_DIRECTION  arrs = {z, p, p', q}:  p' = z + scalar p (0 on Dirichlet nodes), q = A p';  dots[0] = p'.q
 * Single-GPU handles only; the arrays named must be distinct. */
enum mg_pcg_kernel_kind { MG_PCG_K_UPDATE = 0, MG_PCG_K_DOTS = 1, MG_PCG_K_DIRECTION = 2 };
int mg_pcg_kernel(mg_handle h, int kernel, double scalar, const int *arrs, double dots[2]);

/* Full multigrid (nested iteration) -- extension, no reference counterpart. Builds the first finest-grid iterate
 * from the coarsest grid up instead of starting level 0 from whatever U holds:
 *     RHS(l+1) = R RHS(l) down the hierarchy          (desc.restriction; the coarse boundary is injected, so the
 *                                                      Dirichlet data travels with the right-hand side)
 *     U(L-1) = 0 inside, RHS(L-1) on Dirichlet nodes;  coarse solve of A U = RHS   (desc.coarse_* as in a cycle)
 *     for l = L-2 .. 0:   U(l) = Pi U(l+1) inside, RHS(l) on Dirichlet nodes      (one launch)
 *                         cycles_per_level cycles of the descriptor's kind (V, W or F) started on level l
 * Pi is the FMG interpolation: along every coarsened axis f[2m] = c[m], f[2m+1] = (-c[m-1] + 9 c[m] + 9 c[m+1] -
 * c[m+2]) / 16, next to a boundary (3 c[0] + 6 c[1] - c[2]) / 8 and its mirror; kept axes (z of a semi-coarsened
 * transition) are copied. Its O(h^4) error stays below the discretisation error, which mg_prolong's linear
 * interpolation (right for corrections) does not. On return U(0) holds the FMG iterate -- algebraic error at the level
 * of the discretisation error after about 8/7 of the work of the cycles run on level 0 -- and RHS(0) is unchanged; the
 * incoming U(0) is ignored; every other array is unspecified, as after mg_solve. It is the natural first guess of
 * mg_solve / mg_pcg_solve when a tighter tolerance is wanted. No host synchronisation inside the pass except the one
 * residual at its end. MG_CYCLE_V, _W and _F (the levels of a sawtooth cycle hold errors, not solutions), every smoother,
 * both restrictions, aniso, semi_xy, 2-D and 3-D, both dtypes; levels == 1 is just the coarse solve. MG_ERR_BAD_ARG
 * with U untouched: MG_CYCLE_SAWTOOTH, cycles_per_level < 1, distributed handles (dry runs included), a stage callback
 * installed. mg_profile_* brackets keep timing the level-0 cycles inside (cycles on inner levels are not counted). */
typedef struct mg_fmg_stats {
    int32_t levels;            /* levels visited (= desc.levels)                                  */
    int32_t cycles_per_level;
    int32_t coarse_iters;      /* of the first, true coarse solve (mg_cycle_stats semantics)      */
    int32_t coarse_flag;
    double  relres;            /* ||b - A u|| / ||b|| of the result, one residual at the end      */
} mg_fmg_stats;
int mg_fmg(mg_handle h, int cycles_per_level, mg_fmg_stats *st);
/* The interpolation alone, for tests and for callers that drive their own nested iteration:
 * arr_dst(coarse_level - 1) = Pi arr_src(coarse_level); fine Dirichlet nodes take arr_bnd(coarse_level - 1) bit for bit
 * (arr_bnd < 0: they are interpolated like every other node). Single-GPU handles only; arr_dst != arr_bnd. */
int mg_fmg_prolong(mg_handle h, int coarse_level, int arr_src, int arr_dst, int arr_bnd);

/* NESTED ITERATION ON THE OPERATOR FAMILIES (mg_bc_*, mg_vc_*, mg_fas_*, declared further down). No new entry point: a flag
 * OR-ed into arguments the two calls already have.
 *   mg_fmg(h, count | MG_FMG_OPERATOR(op), &st)
 *   mg_fmg_prolong(h, coarse_level | MG_FMG_OPERATOR(op), arr_src, arr_dst, arr_bnd)
 * count and coarse_level are bits 0 .. 15 (count 1 .. 65535). With no bit above 15 set both calls do what they always did, bit
 * for bit (MG_FMG_ON_CONSTANT is 0). The operator is the family's AS THE HANDLE HOLDS IT AT THE CALL; the handle keeps nothing new:
 *   MG_FMG_ON_FACES        mg_bc_*'s operator, the Neumann faces of mg_bc_set_faces
 *   MG_FMG_ON_COEFFICIENT  mg_vc_*'s operator: the coefficient, the shift, the Neumann faces of mg_vc_set_faces
 *   MG_FMG_ON_REACTION     mg_fas_*'s operator exactly as mg_fas_set_reaction left it: its MG_FAS_ON_FACES / MG_FAS_ON_COEFFICIENT
 *                          flags decide the linear part and which mask applies, as in every mg_fas_* call
 * The pass is mg_fmg's with the family's launches:
 *   1. singular case only (linear families, every face Neumann, shift 0): RHS(0) is projected with the family's weights, as
 *      mg_<family>_solve does, and stays projected
 *   2. RHS(l+1) = R RHS(l): the family's restriction (desc.restriction; mirrored full weighting at the Neumann faces, Dirichlet
 *      data injected on the mask's Dirichlet nodes)
 *   3. U(L-1) = 0 at the unknowns, RHS(L-1) on the mask's Dirichlet nodes; the family's coarsest-grid solve, one workgroup or
 *      chip-wide sweeps as in its cycle; stats.coarse_* are this solve's
 *   4. for l = L-2 .. 0: U(l) = Pi_mask U(l+1) at the unknowns, RHS(l) on the Dirichlet nodes (one launch), then count cycles of
 *      the descriptor's kind started on level l
 *   5. singular case: U(0) is projected
 *   6. one residual: stats.relres = ||b - L u|| / ||b||, for mg_fas_*'s operator ||f - N(u)|| / ||f||
 * For mg_fas_* the restricted f is the coarse right-hand side: these are the coarse PROBLEMS, not coarse corrections, so there
 * is no tau term; the cycles started on level l then overwrite RHS / U / E of the levels below it as usual. No host
 * synchronisation before the last residual (the two projections of the singular case synchronise, as in mg_<family>_solve).
 * RHS(0) is unchanged (projected in the singular case); the incoming U(0) is ignored; nothing is allocated.
 * Pi_mask, per coarsened axis: at an end whose face is in the mask the coarse row is extended by its mirror image, c[-1] =
 * c[1] and c[nc] = c[nc-2], and the odd node next to that end takes the cubic rule on the extended row; the one-sided rule
 * stays at an end whose face is Dirichlet. The nodes of a Neumann face are interpolated like every other unknown. Fine nodes on
 * at least one face that is not in the mask take arr_bnd; with arr_bnd < 0 they are interpolated too. Each 1-D pass is
 * ((wb b + wc c) - (a + d)) * 2^-k with every operation rounded separately, along x, then y, then z, for either kernel form
 * (the streaming 3-D kernel or the gather kernel, MG_FMG_FAST): the same bits, and with mask 0 the bits of the unflagged call.
 * MG_ERR_BAD_ARG with U untouched: any other bit above 15, count == 0, MG_FMG_ON_COEFFICIENT (or MG_FMG_ON_REACTION on a
 * reaction with MG_FAS_ON_COEFFICIENT) with no coefficient set, whatever the family's cycle refuses (MG_CYCLE_SAWTOOTH, a
 * smoother other than Jacobi or red-black, a stage callback, distributed handles) -- mg_fmg_prolong with a flag asks for a
 * single-GPU handle and the coefficient only -- and everything the unflagged calls refuse.
 * The FMG property ||u_fmg - u_h|| <= ||u_h - u*|| (max norm; u_h the discrete solution, u* a smooth solution compatible with
 * the mask) with ONE red-black V(2,2) per level is tested on 33^3 / 4 levels for: mg_bc_* with x-lo and with all faces but y-hi
 * Neumann (and a 2-D 65^2 case), mg_vc_* with a smooth factor-100 coefficient and x-lo, mg_fas_* cubic (gamma 1e3) and exp,
 * each plain, MG_FAS_ON_FACES and MG_FAS_ON_COEFFICIENT with both masks. One listed case was dropped: mg_vc_* with all faces
 * but y-hi Neumann, whose float64 reference pass reaches 1.21 x the discretisation error with one cycle per level (two cycles
 * per level are below it); the pass itself is compared with the reference on that case like on the others. */
enum mg_fmg_operator { MG_FMG_ON_CONSTANT = 0 /* default */, MG_FMG_ON_FACES = 1, MG_FMG_ON_COEFFICIENT = 2, MG_FMG_ON_REACTION = 3 };
#define MG_FMG_OPERATOR(op) ((op) << 16)   /* OR-ed into mg_fmg's cycles_per_level or mg_fmg_prolong's coarse_level */

/* W- and F-cycles (extension, mg_desc.h: MG_CYCLE_W, MG_CYCLE_F). With L = desc.levels, one cycle of kind V, W or F started
 * on level l is
 *     cyc(l, kind):
 *       if l == L-1:  coarse solve of A U = RHS (desc.coarse_*);  return
 *       nu_pre sweeps;  RHS(l+1) = R (RHS(l) - A U(l))  (desc.restriction);  U(l+1) = 0
 *       cyc(l+1, kind)
 *       if l+1 < L-1:                      the coarsest grid is solved once per visit of its parent
 *           kind == W: cyc(l+1, W)         the second visit continues from U(l+1), RHS(l+1) unchanged
 *           kind == F: cyc(l+1, V)
 *       U(l) += P U(l+1);  nu_post sweeps
 * and mg_cycle, mg_solve(_lockstep), mg_pcg_solve, mg_fmg, mg_mixed_solve, mg_heat_step, mg_o4_solve run it wherever they
 * run "the handle's cycle". mg_cycle_stats of a W / F cycle: coarse_iters is the sum over the cycle's coarse solves (2^(L-2)
 * of them for W, L-1 for F), coarse_flag the OR, coarse_relres that of the last one; mg_solve_lockstep gives coarse_counts[i]
 * to every coarse solve of iteration i. Level 0 is visited once per cycle whatever the kind and runs as in a V-cycle. The
 * levels below a ROOT level that fit one CU's LDS together (Jacobi or red-black, standard coarsening from the root down, no
 * stage callback) run as ONE launch per visit of the root (MG_SUBCYCLE_LEVEL); mg_subcycle_root says
 * which. Single-GPU handles only: mg_create_distributed* (dry runs included) answer MG_ERR_INVALID_DESC.
 *
 * mg_subcycle: one cyc(level, kind) on U(level), RHS(level), started from the U it holds; kind = MG_CYCLE_V / W / F whatever
 * desc.cycle says (not on a sawtooth handle). path 0: launch by launch (the cycle driver's own code); path 1: the LDS kernel
 * rooted at `level` (no second visit), MG_ERR_BAD_ARG when [level, L-1] is not admissible. The two paths give the same bits
 * with MG_COARSE_FIXED. st as for a W / F cycle. The arrays of the levels below `level` are unspecified afterwards.
 * MG_ERR_BAD_ARG with U untouched: a sawtooth handle, an unknown kind or path, a level outside [0, L-1], distributed
 * handles. */
int mg_subcycle(mg_handle h, int level, int kind, int path, mg_cycle_stats *st);
/* root level the handle's cycles hand to the LDS kernel, -1: none */
int mg_subcycle_root(mg_handle h, int *root);

/* Mixed-precision defect correction (extension, no reference counterpart): an fp64 answer paid for with fp32 cycles.
 * On a handle created with desc.dtype == MG_F32 the solution u and the right-hand side b of level 0 are kept in fp64
 * next to the fp32 hierarchy; the residual r = b - A u is evaluated in fp64, the fp32 hierarchy solves A e = r
 * approximately with inner_cycles of its cycles, and u += e. `maxit` counts corrections:
 *   u = b on the Dirichlet nodes (fp64, bit for bit);  bb = sum b^2 (all nodes, as mg_solve)
 *   r = b - A u in fp64 (written as 0 on Dirichlet nodes whatever u holds there);  rr = sum r^2;  hist[0] = sqrt(rr / bb)
 *   RHS32(0) = (float)(s_0 * r),  s_0 = scale(bb)
 *   for k = 0, 1, ... :   stop if (k > 0 and hist[k] <= tol) or k == maxit
 *       U32(0) = 0;  inner_cycles times: desc.outer_pre_gs lexicographic GS sweeps + one mg_cycle   (mg_solve's outer
 *                                                                                    iteration, as in mg_pcg_solve's M)
 *       ONE launch:  u += (double)U32 / s_k  (interior; Dirichlet nodes untouched)
 *                    r  = b - A u  with the corrected u;  rr_new = sum r^2
 *                    RHS32(0) = (float)(s_{k+1} * r),  s_{k+1} = scale(rr)   (rr of the PREVIOUS residual: known on
 *                                                                              the host before the launch)
 *       hist[k+1] = sqrt(rr_new / bb)
 *   scale(v) = 2^-e with frexp(sqrt(v)) = (m, e); 1.0 when v is 0 or not finite
 * The scale is a power of two, so multiplying and dividing by it is exact: it changes no digit, it only keeps the fp32
 * right-hand side near 1 whatever the size of b and however far the residual has fallen. The history of b * 2^p is
 * bit-identical to that of b, and u is the scaled u bit for bit.
 * Residual arithmetic: fp64 without contraction, in the row order of mg_residual:
 *   r = b - (((((((0 + cz u[k-1]) + cy u[j-1]) + cx u[i-1]) + cd u) + cx u[i+1]) + cy u[j+1]) + cz u[k+1])
 * with mg_level_coefficients(h, 0) (cz terms absent in 2-D); (float) rounds to nearest even; the sums of squares are
 * accumulated in double in a fixed order: two runs give the same bits. A residual that is exactly zero (b == 0 with
 * u == 0 included) gives hist[0] = 0, status 0, no correction.
 * Every cycle the descriptor can describe is admissible (sawtooth or V, every smoother, both restrictions, aniso,
 * semi_xy, 2-D and 3-D, both coarse modes). On return u64 holds the iterate and b64 is unchanged; every fp32 array of
 * the handle is unspecified, as after mg_solve. status == 2: the loop stops at the first residual norm that is not
 * finite (it is the last hist entry) and does NOT take that correction -- the launch writes the corrected u out of place,
 * so u64 stays the last iterate with a finite norm, never NaN.
 * One host synchronisation per correction (the stopping test), none inside the inner cycles. mg_profile_* brackets keep
 * timing the fp32 level-0 launches inside.
 * Memory: the first mg_mixed_set_* allocates three fp64 level-0 arrays (b64 and two copies of u64, written out of place
 * and swapped: 3 x 8 bytes per level-0 node, 3 x 1.1 GB at 513^3), kept until mg_destroy and counted by mg_device_bytes
 * from then on. Host arrays are dense arrays of doubles in the usual layout, whatever desc.dtype says.
 * MG_ERR_BAD_ARG with u64 untouched: a handle that was not created with MG_F32, inner_cycles < 1, maxit < 0,
 * mg_mixed_solve before both arrays were set (mg_mixed_get_solution: before the solution was), distributed handles (dry
 * runs included), a stage callback installed, NULL handle. */
int mg_mixed_set_rhs(mg_handle h, const double *host_b);
int mg_mixed_set_solution(mg_handle h, const double *host_u);
int mg_mixed_get_solution(mg_handle h, double *host_u);
/* the same from / into dense device arrays on the caller's stream (see mg_set_array_device) */
int mg_mixed_set_rhs_device(mg_handle h, const void *dev_b, int dtype, void *stream);
int mg_mixed_set_solution_device(mg_handle h, const void *dev_u, int dtype, void *stream);
int mg_mixed_get_solution_device(mg_handle h, void *dev_u, int dtype, void *stream);

typedef struct mg_mixed_stats {
    int32_t outer;        /* corrections applied                                        */
    int32_t cycles;       /* fp32 cycles run = inner_cycles per correction started      */
    int32_t status;       /* 0 converged, 1 hit maxit, 2 residual norm not finite       */
    int32_t reserved;
    double  relres;       /* last hist entry: the TRUE fp64 ||b - A u|| / ||b||         */
} mg_mixed_stats;
int mg_mixed_solve(mg_handle h, double tol, int maxit, int inner_cycles,
                   double *hist, int hist_cap, int *n_hist, mg_mixed_stats *st);

/* Kernel-level check of the two level-0 kernels of mg_mixed_solve (multigrid_prj_amd/csrc/mg_mixed.hip) on the handle's
 * u64 / b64; arr_e32 / arr_r32 name fp32 level-0 arrays of the handle (mg_array slots):
 *   MG_MIXED_K_RESIDUAL          arr_r32 = (float)(scale_out * (b64 - A u64)), 0 on Dirichlet nodes; arr_e32 is ignored
 *   MG_MIXED_K_CORRECT_RESIDUAL  u64 += (double)arr_e32 / scale_in on interior nodes, then the same residual of the
 *                                corrected u64; arr_e32 != arr_r32
 * *sumsq_r = sum r^2 (unscaled). Any finite non-zero scale_in is honoured (a power of two is divided by exactly). */
enum mg_mixed_kernel_kind { MG_MIXED_K_RESIDUAL = 0, MG_MIXED_K_CORRECT_RESIDUAL = 1 };
int mg_mixed_kernel(mg_handle h, int kernel, double scale_in, double scale_out,
                    int arr_e32, int arr_r32, double *sumsq_r);

/* THE VARIABLE-COEFFICIENT OPERATOR in mg_mixed_solve and mg_mixed_kernel. No new entry point: flags OR-ed into arguments the
 * two calls already have.
 *   mg_mixed_solve(h, tol, maxit, count | MG_MIXED_OPERATOR(MG_MIXED_ON_COEFFICIENT) [| MG_MIXED_INNER_PCG], ...)
 *   mg_mixed_kernel(h, kernel | MG_MIXED_OPERATOR(MG_MIXED_ON_COEFFICIENT), scale_in, scale_out, arr_e32, arr_r32, &sumsq)
 * count (bits 0 .. 15, 1 .. 65535) is the number of cycles -- with MG_MIXED_INNER_PCG of CG iterations -- per correction. With
 * no bit above 15 set every value below 65536 does what it always did, bit for bit.
 * The operator is mg_vc_*'s as the handle holds it AT THE CALL: L = sigma I - div(a grad .) with the coefficient of
 * mg_vc_set_coefficient[_device] on this MG_F32 handle, sigma = mg_get_shift and the Neumann faces of mg_vc_set_faces; the
 * handle keeps nothing new. u64 / b64 are the arrays of mg_mixed_set_*. The fp64 operator uses a = (double) of the handle's
 * fp32 level-0 coefficient: every fp32 value is exact in fp64, so this is a well-defined system -- the user's field rounded
 * to fp32, a relative perturbation of at most 6e-8, none for piecewise-constant fields with representable values. No fp64
 * copy of a is stored and the residual pass reads 4 bytes per node for it, not 8.
 * Arithmetic (fp64, no contraction, every operation rounded separately), c_a from mg_level_coefficients(h, 0), w_a = -c_a / 2:
 *   u' = u + (double)e / s_in at the mask's unknowns; u' = u on its Dirichlet nodes (nodes on at least one face that is not
 *        in the mask; e is not looked at there)
 *   s = 0, d = sigma; for the neighbours q (or their mirror images through a Neumann face) z-, y-, x-, x+, y+, z+ (no z in 2-D):
 *        g = w_a * (a_i + a_q);  s = s + g * u'_q;  d = d + g
 *   r = b - (d * u'_i - s) at unknowns, r = 0 on Dirichlet nodes; r32 = (float)(s_out * r), round to nearest even; the sum of
 *        r^2 (unscaled) in double, per-workgroup partials added in a fixed order: two runs give the same bits
 * (a power-of-two s_in with a normal reciprocal multiplies by the reciprocal, any other divides). mg_vc_set_form chooses the
 * marching tile (mask 0 on 3-D levels with at least 16 fp64 vectors per row) or the one-thread-per-node form, as for every vc
 * kernel; a non-zero mask always takes the latter (a mirrored tile measured slower). Same bits either way.
 * The solve is mg_mixed_solve's loop with: u64 = b64 on the mask's Dirichlet nodes; the inner solve from U32(0) = 0 is count
 * mg_vc_cycle (desc.outer_pre_gs ignored, as in mg_vc_solve) or, with MG_MIXED_INNER_PCG, count iterations of mg_vc_pcg_solve's
 * weighted flexible CG with tolerance 0 (it allocates the Krylov arrays on first use; a breakdown ends the inner solve early
 * and the iterate it holds is the correction; it synchronises once per iteration). stats.cycles counts the cycles run, a CG
 * iteration as one. In the singular case (every face Neumann, shift 0) b64 is projected first with mg_vc_project's weights
 * and STAYS projected, hist is relative to the projected b, u64 is projected after the last correction and stats.relres is
 * evaluated once more on the projected u64 (it is the residual of the u64 returned; the last hist entry is the one before
 * the projection and agrees with it to rounding).
 * MG_ERR_BAD_ARG with u64 untouched and nothing allocated: any other bit above 15, operator value 1 (kept for a faces-only
 * operator) or 3, MG_MIXED_INNER_PCG without MG_MIXED_ON_COEFFICIENT, count == 0, no coefficient set, whatever mg_vc_cycle /
 * mg_vc_pcg_solve refuse (sawtooth, a smoother other than Jacobi or red-black, a stage callback, distributed handles) and
 * everything mg_mixed_solve / mg_mixed_kernel refuse without the flags. */
enum mg_mixed_operator { MG_MIXED_ON_CONSTANT = 0 /* default */, MG_MIXED_ON_COEFFICIENT = 2 };  /* 1: kept for a faces-only operator, refused */
#define MG_MIXED_OPERATOR(op) ((op) << 16)   /* OR-ed into mg_mixed_solve's inner_cycles or mg_mixed_kernel's kernel */
#define MG_MIXED_INNER_PCG    (1 << 20)      /* mg_mixed_solve only, only with MG_MIXED_ON_COEFFICIENT */

/* Fourth-order accurate solves by defect correction (extension, no reference counterpart). The residual is evaluated with
 * the fourth-order operator sigma I + A4 of level 0, the correction equation (sigma I + A2) e = r is solved approximately by
 * the handle's own second-order cycles, u += e (Trottenberg et al., Multigrid, section 5.4.1). The fixed point solves the
 * fourth-order system: its error against the PDE's solution is O(h^4) where mg_solve's is O(h^2).
 * The operator (level 0 only), from mg_level_coefficients(h, 0) = {cx, cy, cz, cd} and sigma = mg_get_shift: w_a = c_a / 12
 * in fp64, cast to the working dtype T like every coefficient. Per axis a, with u(-2) .. u(+2) along it and i the node's
 * index on it (n nodes),
 *   2 <= i <= n-3:  p_a = ((16*(u(-1) + u(+1))) - (u(-2) + u(+2))) - 30*u
 *   i == 1:         p_a = ((((10*u_0 - 15*u_1) - 4*u_2) + 14*u_3) - 6*u_4) + u_5     (u_0 the Dirichlet node, u_1 the node)
 *   i == n-2:       the mirror image, the same order of operations counted from the far boundary
 *   A4u = ((sigma*u + wz*p_z) + wy*p_y) + wx*p_x       (no z term in 2-D)
 *   r = b - A4u on interior nodes, r = 0 on Dirichlet nodes whatever u holds there
 * all in T, every operation rounded separately; the sum of r^2 is accumulated in double in a fixed order (no atomics: two
 * runs give the same bits). Both stencils are exact for polynomials of degree <= 5 along the axis. Level 0 needs n >= 7 on
 * every axis; semi_xy, aniso, grids that are not 2^k + 1, 2-D and 3-D, MG_F64 and MG_F32 are all admissible.
 *
 * mg_o4_residual:  arr_r(0) = arr_b(0) - (sigma I + A4) arr_u(0); arr_r < 0: norm only; arr_r != arr_u, arr_r != arr_b.
 * mg_o4_correct_residual (the fused pass of mg_o4_solve, for kernel-level checks): arr_unew = arr_u + arr_e on interior
 *   nodes, arr_unew = arr_u on Dirichlet nodes (arr_e is not looked at there), arr_r = arr_b - (sigma I + A4) arr_unew in
 *   the same launch; five distinct level-0 arrays; arr_u and arr_e are not modified.
 * Both: *sumsq_r = sum r^2 (may be NULL: nothing is fetched and the call does not synchronise).
 *
 * mg_o4_solve keeps mg_solve's contract for its arrays: b = RHS(0), first iterate = U(0); on return U(0) holds the answer
 * and RHS(0) holds b unchanged, every other array is unspecified.
 *   b4 = RHS(0), u4 = U(0) (device copies); u4 = b4 on Dirichlet nodes; bb = sum b^2 (all nodes, as mg_solve)
 *   r = b4 - A4 u4 -> RHS(0); hist[0] = sqrt(rr / bb)
 *   for k = 0, 1, ...: stop if (k > 0 and hist[k] <= tol) or k == maxit
 *       U(0) = 0; inner_cycles times: desc.outer_pre_gs lexicographic GS sweeps + one mg_cycle (mg_solve's outer iteration)
 *       ONE launch: u4' = u4 + U(0); RHS(0) = b4 - A4 u4'; rr_new; swap u4 / u4'
 *       hist[k+1] = sqrt(rr_new / bb)
 *   U(0) = u4, RHS(0) = b4
 * One host synchronisation per correction (the stopping test), none inside the inner cycles; mg_profile_* brackets keep
 * timing the level-0 launches of the cycles inside. Every cycle the descriptor can describe is admissible and the shift is
 * honoured (the inner cycles work on sigma I + A2 as they do today). The outer iteration contracts by at most
 * max |1 - A4^/A2^| = 1/3 per correction with an exact inner solve. status: 0 converged, 1 maxit reached, 2 at the first
 * residual norm that is not finite (the last hist entry) -- that correction is not taken and U holds the last iterate
 * with a finite norm (the caller's U when the first norm already is not finite). b == 0 with a zero residual gives
 * hist[0] = 0, status 0 and no correction.
 * Memory: the first mg_o4_solve allocates three more level-0 arrays (b4 and two copies of u4), kept until mg_destroy and
 * counted by mg_device_bytes from then on. A call that fails with MG_ERR_HIP after the loop has started (an allocation or a
 * launch failed) leaves U(0) and RHS(0) unspecified: RHS(0) holds a residual, b is still in the handle's b4.
 * MG_ERR_BAD_ARG with U untouched: n < 7, inner_cycles < 1, maxit < 0, distributed handles (dry runs included), a stage
 * callback installed (mg_o4_solve), a bad or repeated array (the two kernel calls), NULL handle. */
int mg_o4_residual(mg_handle h, int arr_u, int arr_b, int arr_r, double *sumsq_r);
int mg_o4_correct_residual(mg_handle h, int arr_u, int arr_e, int arr_b, int arr_unew, int arr_r, double *sumsq_r);
typedef struct mg_o4_stats {
    int32_t outer;        /* corrections applied                                              */
    int32_t cycles;       /* cycles run = inner_cycles per correction started                 */
    int32_t status;       /* 0 converged, 1 hit maxit, 2 residual norm not finite             */
    int32_t reserved;
    double  relres;       /* last hist entry: ||b - (sigma I + A4) u|| / ||b||                */
} mg_o4_stats;
int mg_o4_solve(mg_handle h, double tol, int maxit, int inner_cycles,
                double *hist, int hist_cap, int *n_hist, mg_o4_stats *st);

/* Variable-coefficient diffusion (extension, no reference counterpart): sigma u - div(a(x) grad u) with a nodal coefficient
 * field a >= a_min > 0 -- heterogeneous conduction, porous-media pressure, variable-density projection. On every level l,
 * at interior nodes,
 *   (L u)_i = sigma u_i + sum over axes a of (-c_a / 2) [ (a_i + a_i+)(u_i - u_i+) + (a_i + a_i-)(u_i - u_i-) ]
 * with c_a the off-diagonals of mg_level_coefficients(h, l) and sigma = mg_get_shift: desc.alpha, aniso, semi_xy, grids that
 * are not 2^k + 1 and the shift keep their meaning; Dirichlet rows are identity rows; a == 1 is the handle's constant
 * operator up to rounding. Face coefficients are ARITHMETIC means of the two nodal values (a harmonic mean saves Krylov
 * iterations on jumps and costs six divisions per node per sweep); the coefficient of level l + 1 is the FULL-WEIGHTED
 * coefficient of level l (injected on the coarse boundary, semi transitions as mg_restrict handles them) -- injection
 * diverges on a jump that does not lie on the coarse grids.
 * Arithmetic, in the working dtype T, every operation rounded separately (no contraction), w_a = (T)(-c_a / 2), the
 * neighbours q in the row order of mg_residual, z-, y-, x-, x+, y+, z+ (no z terms in 2-D):
 *   s = 0, d = (T)sigma;  per neighbour on axis a:  g = w_a*(a_i + a_q);  s = s + g*u_q;  d = d + g
 *   residual     r = b - (d*u_i - s) on interior nodes, r = b - u on Dirichlet nodes (mg_residual's convention)
 *   point solve  ps = (b + s) / d, an IEEE division
 *   Jacobi       out of place: u' = ps when desc.omega == 1, else u_i + omega*(ps - u_i); Dirichlet nodes take b
 *   red-black    in place, colour (i + j + k) & 1, colour 0 first; Dirichlet nodes take b with their colour
 *   the sum of r^2 (all nodes) is accumulated in double in a fixed order, no atomics: two runs give the same bits.
 *
 * mg_vc_set_coefficient: a as a dense host array of desc.dtype in the usual layout (level 0); a value that is not finite
 *   and > 0 is refused. The FIRST set call allocates one more level-shaped array per level, kept until mg_destroy and
 *   counted by mg_device_bytes from then on (8/7 of a level-0 array in 3-D); every set call re-restricts all levels.
 * mg_vc_set_coefficient_device: the same from a dense device array on the caller's stream, every rule of
 *   mg_set_array_device (dtype conversion included); positive finite values are a PRECONDITION, nothing looks at them.
 * mg_vc_get_coefficient: the coefficient of any level as a dense host array.
 * mg_vc_residual: arr_r(level) = arr_rhs - L arr_x; arr_r < 0: norm only; *sumsq_r = sum r^2 (may be NULL: no fetch, no
 *   synchronisation); arr_r != arr_x, arr_r != arr_rhs.
 * mg_vc_smooth: `sweeps` sweeps of MG_SMOOTH_JACOBI (desc.omega) or MG_SMOOTH_RBGS; the result is in arr_x (a Jacobi sweep
 *   writes MG_ARR_TMP and the two are swapped, as mg_smooth does: neither array may be MG_ARR_TMP).
 * mg_vc_coarse_solve: mg_coarse_solve's loop (desc.coarse_mode, coarse_maxit, coarse_tol, the handle's smoother) in one
 *   workgroup with the vc sweep and the vc residual; any level.
 * mg_vc_cycle: cyc(0, desc.cycle) exactly as the W / F block above words it -- nu_pre sweeps; RHS(l+1) = R (RHS(l) - L U(l))
 *   with desc.restriction; U(l+1) = 0; the recursion; the second visit for W and F; U(l) += P U(l+1); nu_post sweeps -- every
 *   sweep, residual and the coarse solve by the vc kernels, the transfers by the handle's own; launch by launch (no fused
 *   pairs, no LDS sub-cycle, no folded prolongation). A coarsest level too big for one workgroup in MG_COARSE_FIXED mode
 *   runs coarse_maxit chip-wide sweeps, as mg_cycle does. mg_cycle_stats have the W / F semantics of mg_desc.h.
 * mg_vc_solve: mg_solve's loop and history contract on L: U = RHS on the Dirichlet nodes first, hist[0] the initial
 *   relative residual over all nodes, one mg_vc_cycle per iteration. desc.outer_pre_gs is IGNORED (the lexicographic sweep
 *   has no variable-coefficient form).
 * mg_vc_pcg_solve: mg_pcg_solve's algorithm, statuses and history word for word with A -> L and M r = one mg_vc_cycle from
 *   zero. The cycle alone stalls on coefficient jumps that the coarse grids do not resolve; this is the solver for them.
 * mg_vc_direction (the direction kernel of mg_vc_pcg_solve alone, for kernel-level checks and measurements, as mg_pcg_kernel):
 *   arr_pn = arr_z + (T)beta * arr_p on interior nodes, 0 on Dirichlet nodes; arr_q = L arr_pn by the contract above with
 *   u = arr_pn (q = d*pn_i - s), 0 on Dirichlet nodes; *pq = the sum of pn*q in double (may be NULL: no fetch, no
 *   synchronisation). Four distinct level-0 arrays; arr_z and arr_p are not modified.
 * mg_vc_set_form (tests and measurement tools): form 1 runs the one-thread-per-node kernels on every level, form 0 (the
 *   default) the marching tile where the level's shape admits it (3-D, at least 16 full 16-byte vectors per row).
 * On return of the three drivers U(0) holds the iterate and RHS(0) is unchanged; every other array is unspecified.
 * MG_ERR_BAD_ARG with U untouched: no coefficient set (every call but the two set calls); a sawtooth handle or a stage
 * callback installed (cycle, solve, pcg_solve); a handle smoother other than Jacobi or red-black (cycle, solve, pcg_solve,
 * coarse_solve); an unknown smoother in mg_vc_smooth; distributed handles (dry runs included); bad arrays or levels; NULL
 * handle. No other entry point changes behaviour, and a handle that never calls mg_vc_* allocates nothing new. */
int mg_vc_set_coefficient(mg_handle h, const void *host_a);
int mg_vc_set_coefficient_device(mg_handle h, const void *dev_a, int dtype, void *stream);
int mg_vc_get_coefficient(mg_handle h, int level, void *host_a);
int mg_vc_set_form(mg_handle h, int form);
int mg_vc_residual(mg_handle h, int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r);
int mg_vc_smooth(mg_handle h, int level, int smoother, int sweeps, int arr_x, int arr_rhs);
int mg_vc_coarse_solve(mg_handle h, int level, int arr_x, int arr_rhs, mg_cycle_stats *st);
int mg_vc_cycle(mg_handle h, mg_cycle_stats *st);
int mg_vc_solve(mg_handle h, double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle);
int mg_vc_pcg_solve(mg_handle h, double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_krylov_stats *st);
int mg_vc_direction(mg_handle h, double beta, int arr_z, int arr_p, int arr_pn, int arr_q, double *pq);

/* Neumann faces (extension, no reference counterpart): the handle's constant operator -- alpha, aniso, semi_xy, grids that
 * are not 2^k + 1 and the shift of mg_set_shift keep their meaning -- with zero-flux walls or symmetry planes on any of the
 * 2*dim faces of the box. x is the fast index i, y is j, z is k; LO is index 0 and HI index n-1 of the host layout. */
enum mg_face { MG_FACE_XLO = 1, MG_FACE_XHI = 2, MG_FACE_YLO = 4, MG_FACE_YHI = 8, MG_FACE_ZLO = 16, MG_FACE_ZHI = 32 };
/* The mask is the set of NEUMANN faces; 0 (the default) means all Dirichlet. A node is a DIRICHLET NODE if it lies on at
 * least one face that is not in the mask: its row is the identity row with mg_residual's and mg_smooth's conventions (the
 * residual is b - u, the sweeps take b, red-black with the node's colour). Every other node is an unknown: the interior
 * nodes and the nodes that lie only on Neumann faces, the edges and corners between Neumann faces included. At an unknown on
 * the LO face of an axis the missing neighbour u(i-) is the mirror image u(i+), likewise on HI, each axis on its own; no
 * ghost value is stored or read. Arithmetic in the working dtype T, every operation rounded separately, the coefficients
 * of mg_level_coefficients(h, l):
 *   residual     sum = cz u(z-) + cy u(y-) + cx u(x-) + cd u_i + cx u(x+) + cy u(y+) + cz u(z+), added left to right (no z terms
 *                in 2-D); r = b - sum; the sum of r^2 over all nodes in double in a fixed order, no atomics
 *   point solve  the same sum without the diagonal term; ps = (b - sum) / cd, the IEEE quotient
 *   Jacobi       out of place: u' = ps when desc.omega == 1, else u_i + omega*(ps - u_i)
 *   red-black    in place, colour (i + j + k) & 1, colour 0 first
 * With mask 0 these are mg_residual's and mg_smooth's results bit for bit.
 * INHOMOGENEOUS FLUX is the caller's business: for an outward normal derivative g on a Neumann face of axis a, add
 * -2 h_a c_a g = +(2 alpha aniso_a / h_a) g to b at that face's nodes (c_a the level-0 off-diagonal, h_a the mesh width; at
 * an edge or corner between Neumann faces one term per face). The discretisation stays second-order accurate.
 *
 * mg_bc_set_faces / mg_bc_get_faces: set and read the mask. Nothing is allocated and the mask may be changed at any time;
 *   z bits on a 2-D handle are MG_ERR_BAD_ARG.
 * mg_bc_residual, mg_bc_smooth, mg_bc_coarse_solve: the argument lists and aliasing rules of mg_vc_residual, mg_vc_smooth and
 *   mg_vc_coarse_solve.
 * mg_bc_restrict: MG_RESTRICT_INJECT is mg_restrict's injection. MG_RESTRICT_FULLW at a coarse unknown is mg_restrict's
 *   9-/27-point full weighting in its order of operations with fine indices that fall outside the grid mirrored
 *   (2x-1 < 0 -> 2x+1, 2x+1 > nx_f-1 -> 2x-1, per axis); coarse Dirichlet nodes are injected; semi transitions keep z.
 *   Mask 0 equals mg_restrict bit for bit. (Injecting at coarse nodes of a Neumann face, which mg_restrict would do, makes
 *   the red-black cycle diverge: DESIGN.md section 19.)
 * mg_bc_cycle: cyc(0, desc.cycle) exactly as mg_vc_cycle words it, with the sweeps, the residual, the restriction
 *   (desc.restriction) and the coarse solve of this operator and mg_prolong(add = 1); launch by launch. A coarsest level too big
 *   for one workgroup in MG_COARSE_FIXED mode runs coarse_maxit chip-wide sweeps, as mg_cycle does.
 * mg_bc_solve: mg_solve's loop and history contract on this operator: U = RHS on the Dirichlet nodes first, hist[0] the
 *   initial relative residual over all nodes, one mg_bc_cycle per iteration. desc.outer_pre_gs is IGNORED.
 *   THE SINGULAR CASE -- all 2*dim faces Neumann and the current shift 0: the constants are the null space. mg_bc_solve then
 *   projects RHS(0) (mg_bc_project) before anything else, so hist is relative to the projected right-hand side, and projects
 *   U(0) after the last cycle; RHS(0) holds the PROJECTED right-hand side on return. In every other combination RHS(0) is
 *   unchanged.
 * mg_bc_project: c = (sum w_i v_i) / (sum w_i) in double in a fixed order, then v_i -= (T)c on every node; *mean = c (may be
 *   NULL). w_i is the product over the axes of 1/2 for each Neumann face the node lies on, else 1: diag(w) L is symmetric,
 *   so w spans the left null space of the singular operator, and the mirrored full weighting keeps a compatible right-hand
 *   side compatible from level to level (R^T w_coarse = w_fine / 2^dim). Synchronises.
 * mg_bc_set_form (tests and measurement tools): form 1 runs the one-thread-per-node kernels on every level, form 0 (the
 *   default) the marching tile where the level's shape admits it (3-D, at least 16 full 16-byte vectors per row).
 * MG_ERR_BAD_ARG with U untouched: a sawtooth handle or a stage callback installed (cycle, solve); a handle smoother other
 * than Jacobi or red-black (cycle, solve, coarse_solve); an unknown smoother in mg_bc_smooth; distributed handles (dry runs
 * included); bad arrays, levels or masks; NULL handle. No other entry point changes behaviour, and the family allocates
 * nothing. Not combined with mg_vc_*, mg_o4_*, mg_heat_step, mg_fmg, mg_eig_solve, mg_mixed_solve or mg_pcg_solve, which
 * keep treating every face as Dirichlet (mg_fas_* reads this mask when its kind carries MG_FAS_ON_FACES, mg_eig_solve after
 * MG_EIG_OPERATOR(MG_EIG_ON_FACES) OR-ed into its m, mg_fmg / mg_fmg_prolong after MG_FMG_OPERATOR(MG_FMG_ON_FACES), see there). mg_mixed_solve has no faces-only operator (value 1 of
 * mg_mixed_operator is refused): its Neumann faces are mg_vc_set_faces' with MG_MIXED_ON_COEFFICIENT, and a == 1 there is
 * this family's operator; mg_set_shift + mg_bc_solve is the implicit step with insulated walls. */
int mg_bc_set_faces(mg_handle h, int mask);
int mg_bc_get_faces(mg_handle h, int *mask);
int mg_bc_set_form(mg_handle h, int form);
int mg_bc_residual(mg_handle h, int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r);
int mg_bc_smooth(mg_handle h, int level, int smoother, int sweeps, int arr_x, int arr_rhs);
int mg_bc_restrict(mg_handle h, int fine_level, int kind, int arr_src, int arr_dst);
int mg_bc_coarse_solve(mg_handle h, int level, int arr_x, int arr_rhs, mg_cycle_stats *st);
int mg_bc_project(mg_handle h, int level, int arr, double *mean);
int mg_bc_cycle(mg_handle h, mg_cycle_stats *st);
int mg_bc_solve(mg_handle h, double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle);

/* Neumann faces of the variable-coefficient operator (extension, no reference counterpart): mg_vc_* with zero-flux walls or
 * symmetry planes -- insulated walls of a heterogeneous conductor, no-flow boundaries of a porous medium, the all-Neumann
 * and singular variable-density projection. A SECOND face mask on the handle, independent of mg_bc_set_faces, default 0.
 * The node classes are those of the block above: a node on at least one face that is not in the mask is a Dirichlet node
 * (identity row: r = b - u, the sweeps take b), every other node is an unknown, edges and corners between Neumann faces
 * included. At an unknown the arithmetic is mg_vc_*'s word for word with the MIRRORED index substituted for a missing
 * neighbour, for a and for u alike; no ghost value is stored or read:
 *   w_a = (T)(-c_a / 2);  s = 0;  d = (T)sigma;  for the slots z-, y-, x-, x+, y+, z+ (no z in 2-D), q the neighbour or its
 *   mirror image i+ when i- falls outside through a Neumann face (i- for a missing i+):
 *       g = w_a * (a_i + a_q);  s = s + g * u_q;  d = d + g                (a mirrored slot counts twice, in s and in d)
 *   residual r = b - (d * u_i - s), point solve (b + s) / d, Jacobi / damping / red-black colour as for mg_vc_*; the sum of r^2
 *   over all nodes in double in a fixed order.
 * With w_i = the product of 1/2 per Neumann face the node lies on (mg_bc_project's weights) diag(w) L is symmetric for any a,
 * and with every face Neumann and shift 0 the constants span the null space.
 * COARSE COEFFICIENTS: with a non-zero mask level l + 1 is the MIRRORED full weighting of level l (mg_bc_restrict's
 * MG_RESTRICT_FULLW with this mask, coarse Dirichlet nodes injected), which keeps min a <= a_coarse <= max a;
 * mg_vc_set_coefficient* restricts with the current mask and mg_vc_set_faces restricts again from the stored level 0 when a
 * coefficient is set, so the two may come in either order. With mask 0 everything is mg_vc_*'s kernels and bits as before.
 * INHOMOGENEOUS FLUX is the caller's business: for an outward normal derivative g on a Neumann face of axis a add
 * (2 alpha aniso_a / h_a) a_i g to b at that face's nodes, a_i the coefficient AT the wall node (one term per face at an edge
 * or corner): second-order accurate for any a. (alpha aniso_a / h_a) (a_i + a_i+) g, with the coefficient of the mirrored
 * slot, is second order only where a has no normal derivative at the wall and first order otherwise.
 *
 * mg_vc_set_faces / mg_vc_get_faces: set and read the mask; nothing is allocated; z bits on a 2-D handle and masks outside
 *   0..63 are MG_ERR_BAD_ARG and leave the mask and the coefficients as they were.
 * These entry points honour the mask with unchanged signatures: mg_vc_residual, mg_vc_smooth, mg_vc_coarse_solve, mg_vc_cycle
 *   (V, W, F; the residual goes down by mg_vc_restrict with desc.restriction), mg_vc_solve, mg_vc_heat_rhs, mg_vc_heat_step
 *   (theta == 1 copies u on the mask's Dirichlet nodes), mg_vc_pcg_solve and mg_vc_direction.
 * mg_vc_solve, THE SINGULAR CASE (every face of the handle's dimension Neumann, shift 0): as mg_bc_solve -- RHS(0) is projected
 *   first and stays projected, U(0) is projected after the last cycle.
 * mg_vc_pcg_solve with a mask: every inner product of the iteration is sum w x y (z.r, z.q, p.q), in which L is self-adjoint;
 *   the stopping test and the history stay sqrt(sum r^2) / ||b||. In the singular case RHS(0) is projected first, z after
 *   every preconditioner application and x at the end.
 * mg_vc_direction with a mask: arr_pn and arr_q are 0 on the mask's Dirichlet nodes, neighbours are mirrored, *pq = sum w pn q.
 * mg_vc_restrict, mg_vc_project: mg_bc_restrict and mg_bc_project with this mask (no coefficient is needed).
 * MG_ERR_BAD_ARG as for mg_vc_*. Not combined with mg_fas_*, mg_o4_* or mg_fmg (mg_fas_* with MG_FAS_ON_COEFFICIENT,
 * mg_eig_solve with MG_EIG_ON_COEFFICIENT and, on an MG_F32 handle, mg_mixed_solve / mg_mixed_kernel with
 * MG_MIXED_OPERATOR(MG_MIXED_ON_COEFFICIENT) read the coefficient, the shift and this mask at the call, see there; so does mg_fmg
 * with MG_FMG_OPERATOR(MG_FMG_ON_COEFFICIENT)). */
int mg_vc_set_faces(mg_handle h, int mask);
int mg_vc_get_faces(mg_handle h, int *mask);
int mg_vc_restrict(mg_handle h, int fine_level, int kind, int arr_src, int arr_dst);
int mg_vc_project(mg_handle h, int level, int arr, double *mean);

/* Nonlinear solves by the full approximation scheme, FAS (extension, no reference counterpart): the semilinear problem
 *     N(u) = (sigma I + A) u + gamma g(u) = f
 * with the handle's constant operator -- alpha, aniso, semi_xy, grids that are not 2^k + 1 and the shift of mg_set_shift keep
 * their meaning --, all faces Dirichlet, and a pointwise reaction g; gamma is the same on every level. The cycle is the
 * smoothing / restriction / prolongation recursion on the nonlinear problem itself: no global linearisation, no Jacobian. */
enum mg_fas_kind { MG_FAS_CUBIC = 0 /* g = u^3 */, MG_FAS_EXP = 1 /* g = exp(u) */,
                   MG_FAS_ON_FACES = 256 /* OR-ed into the kind: the linear part is mg_bc_*'s operator */,
                   /* 512 is skipped on purpose: it has always been a refused kind value that callers and the suite rely on */
                   MG_FAS_ON_COEFFICIENT = 1024 /* OR-ed into the kind: the linear part is mg_vc_*'s operator (not with 256) */ };
typedef struct mg_fas_stats {
    int32_t status;   /* 0 converged, 1 hit maxit, 2 a norm that is not finite (it is the last hist entry; U is unspecified) */
    int32_t cycles;   /* cycles done = n_hist - 1                                                                            */
    double  norm0;    /* hist[0]                                                                                             */
    double  norm;     /* the last norm                                                                                       */
} mg_fas_stats;
/* Arithmetic in the working dtype T, every operation rounded separately, the coefficients of mg_level_coefficients(h, l),
 * G = (T)gamma. At interior nodes:
 *   reaction     MG_FAS_CUBIC: q = u*u; g = q*u; gp = (T)3 * q.  MG_FAS_EXP: g = gp = exp(u) (the device library's exp / expf)
 *   residual     sum = cz u(z-) + cy u(y-) + cx u(x-) + cd u_i + cx u(x+) + cy u(y+) + cz u(z+), added left to right (no z terms
 *                in 2-D); r = b - (sum + G*g). Dirichlet nodes: r = b - u. The sum of r^2 over all nodes in double in a fixed
 *                order, no atomics
 *   point solve  s = the same sum without the diagonal term; num = (b - s) - G*(g - gp*u); den = cd + G*gp; ps = num / den,
 *                the IEEE quotient -- one Newton step on the node's own equation, no inner iteration. Dirichlet nodes take b.
 *                NOTHING GUARDS den: the supported regime is gamma g' >= 0 (monotone); other signs are the caller's risk
 *                and end in status 2 of mg_fas_solve when a norm stops being finite.
 *   Jacobi       out of place: u' = ps when desc.omega == 1, else u_i + omega*(ps - u_i)
 *   red-black    in place, colour (i + j + k) & 1, colour 0 first
 * With gamma == 0 these are mg_residual's and mg_smooth's results bit for bit, for both kinds.
 *
 * mg_fas_set_reaction / mg_fas_get_reaction: the kind and gamma (default MG_FAS_CUBIC, 0). Nothing is allocated and the
 *   reaction may change at any time.
 * mg_fas_residual, mg_fas_smooth, mg_fas_coarse_solve: the argument lists and aliasing rules of mg_vc_residual, mg_vc_smooth
 *   and mg_vc_coarse_solve; the coarse solve is mg_coarse_solve's loop on the nonlinear residual and point solve.
 * mg_fas_coarse_rhs(l): the FAS transition l -> l+1 in one launch, after the residual of level l is in TMP(l). Per coarse
 *   node: uc = U(l) at the even fine node (the iterate goes down by INJECTION), written to U(l+1) and to E(l+1), the kept
 *   copy; rc = the full weighting of TMP(l) in mg_restrict's order of operations, or its injection with MG_RESTRICT_INJECT
 *   (desc.restriction); RHS(l+1) = rc + (sum_c + G*g(uc)), sum_c the residual's sum with the coefficients of level l+1 and the
 *   coarse neighbours read from U(l). Coarse Dirichlet nodes: RHS(l+1) = uc. Semi transitions keep z as mg_restrict does.
 * mg_fas_correct(l): E(l+1) = U(l+1) - E(l+1) rounded in T, then U(l) += P E(l+1) by mg_prolong(add = 1); E(l+1) holds the
 *   coarse correction afterwards.
 * mg_fas_cycle: cyc(0, desc.cycle) exactly as mg_vc_cycle words it, with these differences: the transition and the correction
 *   are the two calls above, so U(l+1) starts from the injected iterate instead of 0, and a second visit (W, F) continues
 *   from U(l+1) with RHS(l+1) and E(l+1) unchanged; the coarsest level runs mg_fas_coarse_solve. Launch by launch.
 * mg_fas_solve: U = RHS on the Dirichlet nodes first; hist[k] = sqrt(sum r^2) over all nodes after k cycles -- ABSOLUTE
 *   norms, because b = 0 is an ordinary nonlinear problem; stops when hist[k] <= max(atol, rtol * hist[0]) (k = 0 included) or
 *   k == maxit; at the first norm that is not finite it stops with status 2. One host synchronisation per cycle.
 *   desc.outer_pre_gs is IGNORED. FAS CONVERGES LOCALLY: the starting iterate in U is the caller's (DESIGN.md section 20 has
 *   a case that diverges from u = 0); there is no line search and no nested iteration.
 * mg_fas_set_form (tests and measurement tools): form 1 runs the one-thread-per-node kernels on every level, form 0 (the
 *   default) the marching tile where the level's shape admits it (3-D, at least 16 full 16-byte vectors per row).
 * MG_ERR_BAD_ARG with nothing changed: an unknown kind or a gamma that is not finite; a smoother other than Jacobi or
 * red-black (mg_fas_smooth's argument; the handle's for cycle, solve, coarse_solve); a sawtooth handle or a stage callback
 * installed (cycle, solve); distributed handles (dry runs included); bad arrays or levels and the aliasing mg_vc_residual /
 * mg_vc_smooth reject; negative or non-finite tolerances, maxit < 0; NULL handle. No other entry point changes behaviour, and
 * the family allocates nothing. Not combined with mg_vc_*, mg_o4_*, mg_fmg (unless MG_FMG_OPERATOR(MG_FMG_ON_REACTION) is
 * OR-ed into its count, see there), mg_mixed_solve or mg_heat_step, and with
 * mg_bc_* only as described next; mg_set_shift(1/dt) + mg_fas_solve is one implicit reaction-diffusion step.
 *
 * NEUMANN FACES. mg_fas_set_reaction(h, MG_FAS_CUBIC | MG_FAS_ON_FACES, gamma) (or MG_FAS_EXP | MG_FAS_ON_FACES) makes the
 * linear part mg_bc_*'s operator: while the flag is set every mg_fas_* entry point, mg_fas_heat_* included, uses the handle's
 * current mg_bc_set_faces mask m, read at call time -- the two calls may come in either order and mg_bc_set_faces keeps its
 * own validation. mg_fas_get_reaction returns the kind with the flag; every other kind value stays refused. The unknowns are
 * the nodes whose faces all lie in m, u(q) is the neighbour or its mirror image as for mg_bc_*, and with m != 0:
 *   residual     sum = mg_bc_residual's sum in its order; r = b - (sum + G*g); Dirichlet nodes (a face outside m): r = b - u
 *   point solve  s = mg_bc_smooth's off-diagonal sum; ps from s as above; Dirichlet nodes take b; damping and colouring as above
 *   mg_fas_coarse_rhs  uc as above at every coarse node; rc = mg_bc_restrict's mirrored full weighting of TMP(l) (or the
 *                injection with MG_RESTRICT_INJECT); at a coarse unknown RHS(l+1) = rc + (sum_c + G*g(uc)) with a coarse
 *                neighbour that leaves the grid replaced by its mirror image in U(l); coarse Dirichlet nodes by m: RHS(l+1) = uc.
 *                Still one launch. (Injecting the residual at the coarse nodes of a Neumann face makes the cycle diverge.)
 *   mg_fas_correct  unchanged: the prolongation writes face nodes already
 *   mg_fas_cycle, mg_fas_coarse_solve  the same recursion and loop over this point operator (V, W and F cycles)
 *   mg_fas_solve  U = RHS on m's Dirichlet nodes first, then as above
 *   mg_fas_heat_rhs, mg_fas_heat_step  n0 = the mirrored sum with cd0, plus G*g; m's Dirichlet nodes copy u; theta == 1 is
 *                mg_bc_heat_rhs's stencil-free form with m
 * - With the flag clear, or the flag set and mask 0, every mg_fas_* call makes the launches it makes without this feature,
 *   with the same kernel instantiations: the same bits.
 * - With gamma == 0 and the flag set, mg_fas_residual, mg_fas_smooth and mg_fas_coarse_solve give mg_bc_*'s bits and
 *   mg_fas_heat_rhs gives mg_bc_heat_rhs's (num = b - s and den = cd, whose IEEE quotient is mg_bc_smooth's).
 * - NO PROJECTION is done. With all 2*dim faces in m, shift 0 and gamma == 0 the operator is singular and mg_bc_solve is the
 *   entry point; with gamma g' > 0 somewhere the problem is regular. The singular case is documented, not refused.
 * - Nothing is allocated; mg_bc_* and mg_vc_* are unchanged; the refusals are those listed above.
 *
 * VARIABLE COEFFICIENT. mg_fas_set_reaction(h, MG_FAS_CUBIC | MG_FAS_ON_COEFFICIENT, gamma) (or MG_FAS_EXP | ...) makes the
 * linear part mg_vc_*'s operator: sigma u - div(a(x) grad u) + gamma g(u) = f. While the flag is set every mg_fas_* entry
 * point -- residual, smooth, coarse_rhs, correct, coarse_solve, cycle (V, W, F), solve, heat_rhs, heat_step -- uses the
 * handle's coefficient hierarchy (mg_vc_set_coefficient*), the shift of mg_set_shift and the handle's mg_vc_set_faces mask
 * m, all read at call time: the calls may come in any order. mg_bc_set_faces is not looked at. MG_FAS_ON_COEFFICIENT is
 * 1024, not 512: 512 has always been a refused kind value and stays one. The valid kinds are 0 and 1, alone or OR-ed with
 * exactly one of 256 and 1024; every other value, 256 | 1024 included, is MG_ERR_BAD_ARG and changes nothing.
 * mg_fas_get_reaction returns the kind with the flag. While the flag is set an mg_fas_* compute call on a handle with no
 * coefficient set is MG_ERR_BAD_ARG with mg_vc_*'s "no coefficient set" message.
 * Arithmetic in T, every operation rounded separately; s and d are mg_vc_*'s (d started from (T)sigma, neighbour order z-,
 * y-, x-, x+, y+, z+, w_a of the level; with a mask the mirrored index is used for a and u alike), G = (T)gamma, g and gp as
 * above:
 *   residual     r = b - ((d*u_i - s) + G*g) at unknowns; Dirichlet nodes (a face outside m): r = b - u; the sum of r^2 over
 *                all nodes in double, fixed order
 *   point solve  num = (b + s) - G*(g - gp*u_i); den = d + G*gp; ps = num / den; Dirichlet nodes take b; Jacobi damping and
 *                red-black colouring as mg_vc_*. Nothing guards den.
 *   mg_fas_coarse_rhs  still one launch: uc = U(l) injected into U(l+1) and E(l+1); rc = mg_bc_restrict's mirrored full
 *                weighting with m (plain full weighting for m == 0, the injection with MG_RESTRICT_INJECT); at a coarse
 *                unknown RHS(l+1) = rc + ((d_c*uc - s_c) + G*g(uc)) with s_c, d_c from level l+1's coefficient array at the
 *                coarse node and its coarse neighbours and level l+1's w_a, the u neighbours read from U(l) at distance 2
 *                (z: 1 on a semi transition); on a face in m a neighbour that leaves the grid, for a or for u, is its
 *                mirror image; coarse Dirichlet nodes: RHS(l+1) = uc
 *   mg_fas_correct  unchanged
 *   mg_fas_solve  U = RHS on m's Dirichlet nodes first, then as above
 *   mg_fas_heat_rhs, mg_fas_heat_step  n0 = (d0*u_i - s) + G*g with d0 started from (T)0; Dirichlet nodes copy u; theta == 1
 *                takes the stencil-free launches mg_vc_heat_rhs takes
 * - With gamma == 0 and the flag set, mg_fas_residual, mg_fas_smooth, mg_fas_coarse_solve and mg_fas_heat_rhs give
 *   mg_vc_residual's, mg_vc_smooth's, mg_vc_coarse_solve's and mg_vc_heat_rhs's bits, for mask 0 and non-zero masks
 *   (num = b + s, den = d). With the flag clear every call gives the bits it gave before the flag existed.
 * - NO PROJECTION is done: all faces in m, shift 0 and gamma == 0 is singular, and mg_vc_solve is the entry point for it.
 * - Nothing is allocated; mg_vc_* and mg_bc_* are unchanged; mg_fas_set_form(1) selects the plain kernels here too. */
int mg_fas_set_reaction(mg_handle h, int kind, double gamma);
int mg_fas_get_reaction(mg_handle h, int *kind, double *gamma);
int mg_fas_set_form(mg_handle h, int form);
int mg_fas_residual(mg_handle h, int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r);
int mg_fas_smooth(mg_handle h, int level, int smoother, int sweeps, int arr_x, int arr_rhs);
int mg_fas_coarse_rhs(mg_handle h, int fine_level);
int mg_fas_correct(mg_handle h, int fine_level);
int mg_fas_coarse_solve(mg_handle h, int level, int arr_x, int arr_rhs, mg_cycle_stats *st);
int mg_fas_cycle(mg_handle h, mg_cycle_stats *st);
int mg_fas_solve(mg_handle h, double rtol, double atol, int maxit, double *hist, int hist_cap, int *n_hist, mg_fas_stats *st);

/* Diagonal shift (extension, no reference counterpart): from this call on the handle works on sigma I + A, sigma >= 0 --
 * the operator of an implicit time step or a screened-Poisson / Helmholtz-type solve. On every level the diagonal becomes
 * cd0_l + sigma (one fp64 addition, then cast to the working dtype like every coefficient), cd0_l being the diagonal the
 * handle was created with; off-diagonals and Dirichlet rows (identity) are untouched. mg_level_coefficients reports the
 * shifted diagonal, and everything works on the shifted operator with no further change of interface: mg_smooth,
 * mg_residual, mg_coarse_solve(_ex), mg_cycle(_async), mg_solve, mg_solve_lockstep, mg_pcg_solve, mg_pcg_kernel, mg_fmg,
 * mg_mixed_solve / mg_mixed_kernel (which document themselves in terms of mg_level_coefficients). sigma == 0 restores the
 * creation state bit for bit; a handle on which this is never called behaves exactly as before. On a zebra handle the
 * line factors of every level are re-tabulated for the new diagonal after the handle's stream has been synchronised.
 * MG_ERR_BAD_ARG with the handle unchanged: NULL handle, sigma negative or not finite, distributed handles (dry runs
 * included). */
int mg_set_shift(mg_handle h, double sigma);
int mg_get_shift(mg_handle h, double *sigma);

/* Implicit heat-equation stepper (extension): integrates u_t = -A0 u + f on level 0 with the theta scheme, A0 being the
 * UNSHIFTED operator of level 0 (desc.alpha is its diffusion constant). The Dirichlet values are those the U array holds
 * on the Dirichlet nodes: constant over a call, the caller may rewrite them between calls. One step solves, on the
 * interior rows,
 *     (1/(theta dt) I + A0) u' = (f + u/dt - (1 - theta) A0 u) / theta
 * theta = 1: backward Euler, theta = 1/2: Crank-Nicolson. mg_heat_step(h, dt, theta, nsteps, cycles_per_step, st):
 *   1. mg_set_shift(h, 1.0 / (theta * dt)) -- that expression in fp64 -- unless that is the current shift already. The
 *      shift STAYS set on return (mg_get_shift tells; mg_residual then evaluates the step's operator).
 *   2. nsteps times:  RHS(0) = the step's right-hand side built from U(0) (+ f), ONE launch (mg_heat.hip);
 *                     cycles_per_step times: desc.outer_pre_gs lexicographic GS sweeps + one mg_cycle -- mg_solve's outer
 *                     iteration, warm-started from u (U is not cleared).
 *   3. one residual and one sum of squares: st->relres = ||rhs - (sigma I + A0) u|| / ||rhs|| of the LAST step (all
 *      nodes, as mg_solve; what mg_residual / mg_sumsq on U, RHS return afterwards).
 * No host synchronisation inside or between the steps: nsteps = 100 enqueues 100 steps back to back; the residual at the
 * end is the only one. Sawtooth and V-cycle, every smoother, both restrictions, aniso, semi_xy, 2-D and 3-D, both dtypes.
 * mg_profile_* brackets keep timing the level-0 launches of the cycles inside. On return U holds u after nsteps steps and
 * RHS(0) the last step's right-hand side; every other array is unspecified, as after mg_solve.
 * Right-hand-side arithmetic, in the working dtype T, every operation rounded separately (no contraction), the stencil
 * in the row order of mg_residual with cd0 = the unshifted diagonal of level 0:
 *   s   = (((((((0 + cz u[k-1]) + cy u[j-1]) + cx u[i-1]) + cd0 u) + cx u[i+1]) + cy u[j+1]) + cz u[k+1])  (cz terms absent in 2-D)
 *   rhs = ((f + rdt*u) - omt*s) * rth      interior nodes;  without a source (rdt*u - omt*s) * rth
 *   rhs = u                                Dirichlet nodes, bit for bit
 *   rdt = (T)(1.0/dt),  omt = (T)(1.0 - theta),  rth = (T)(1.0/theta)   (fp64 on the host, then cast)
 * theta == 1 takes the stencil-free form rhs = f + rdt*u: for finite data the value of the general expression
 * (omt = 0, rth = 1).
 * mg_heat_set_source: f as a dense host array of desc.dtype in the usual layout (its values on Dirichlet nodes are
 * ignored); NULL: f = 0 again. The first call with an array allocates one more level-0 array, kept until mg_destroy and
 * counted by mg_device_bytes from then on (1.1 GB at 513^3 fp64); without a source the kernel reads none.
 * mg_heat_rhs is the assembly kernel alone, for tests and for callers that drive their own steps (mg_set_shift +
 * mg_heat_rhs + mg_solve is a step solved to a tolerance): arr_dst(0) = the right-hand side of one step built from
 * arr_u(0); arr_u is not modified and the shift is not touched.
 * MG_ERR_BAD_ARG, with U and the shift untouched: dt not positive or not finite (or so small that 1/(theta dt) is not
 * finite), theta outside (0, 1], nsteps < 1, cycles_per_step < 1, arr_dst == arr_u (mg_heat_rhs), distributed handles
 * (dry runs included), a stage callback installed (mg_heat_step), NULL handle. */
int mg_heat_set_source(mg_handle h, const void *host_f);
/* f from a dense device array on the caller's stream (see mg_set_array_device); dev_f == NULL: f = 0 again */
int mg_heat_set_source_device(mg_handle h, const void *dev_f, int dtype, void *stream);
typedef struct mg_heat_stats {
    int32_t steps;    /* steps taken                                              */
    int32_t cycles;   /* cycles run = steps * cycles_per_step                     */
    double  time;     /* steps * dt                                               */
    double  relres;   /* ||rhs - (sigma I + A0) u|| / ||rhs|| of the LAST step    */
} mg_heat_stats;
int mg_heat_step(mg_handle h, double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st);
int mg_heat_rhs(mg_handle h, double dt, double theta, int arr_u, int arr_dst);

/* ---- implicit time steps on the operator families (extension) ----
 * mg_vc_heat_*, mg_bc_heat_* and mg_fas_heat_* are mg_heat_step / mg_heat_rhs for u_t = -N0(u) + f, with N0 the family's
 * operator on level 0 WITHOUT the handle's shift:
 *   vc    N0(u) = -div(a grad u)          (a of mg_vc_set_coefficient; Dirichlet nodes: the box boundary)
 *   bc    N0(u) = A0 u with mirrored neighbours at the unknowns on the faces of the mask (mg_bc_set_faces; Dirichlet nodes:
 *                 the nodes on a face that is NOT in the mask)
 *   fas   N0(u) = A0 u + gamma g(u)       (mg_fas_set_reaction; Dirichlet nodes: the box boundary; with MG_FAS_ON_FACES A0 and
 *                 the Dirichlet nodes are bc's, by the mg_bc_set_faces mask)
 * f is the source of mg_heat_set_source[_device]: a handle holds ONE source, shared by mg_heat_step and these three
 * steppers. One theta step solves, on the unknowns,
 *     (1/(theta dt)) u' + N0(u') = (f + u/dt - (1 - theta) N0(u)) / theta
 * which holds for the nonlinear N0 as it stands (theta = 1: backward Euler, 1/2: the trapezoidal rule).
 * mg_X_heat_step(h, dt, theta, nsteps, cycles_per_step, st) is mg_heat_step with step 2's launch replaced by the family's
 * right-hand side launch and its outer iteration by ONE mg_X_cycle (warm-started from u; desc.outer_pre_gs is ignored, as
 * in mg_X_solve): mg_set_shift(h, 1.0 / (theta * dt)) first, which STAYS set; no host synchronisation between the steps;
 * at the end one mg_X_residual norm and one sum of squares, st->relres = ||rhs - (sigma I + N0)(u')|| / ||rhs|| of the
 * LAST step (0 when the numerator is 0). bc with every face Neumann is not singular here (sigma > 0): nothing is projected.
 * mg_X_heat_rhs(h, dt, theta, arr_u, arr_dst) is the assembly launch alone: arr_dst(0) = the step's right-hand side from
 * arr_u(0) in ONE launch, with the UNSHIFTED operator whatever the handle's shift is; arr_u and the shift are not touched.
 * mg_set_shift(h, 1/(theta dt)) + mg_X_heat_rhs + mg_X_solve is a step solved to a tolerance.
 * Arithmetic, in the working dtype T, every operation rounded separately, rdt / omt / rth as for mg_heat_rhs:
 *   rhs = ((f + rdt*u) - omt*n0) * rth     unknowns;  without a source (rdt*u - omt*n0) * rth
 *   rhs = u                                Dirichlet nodes, bit for bit
 *   n0  = the family's residual expression with the shift taken out: vc d*u_i - s with d started from (T)0; bc the sum of
 *         mg_bc_residual with the unshifted diagonal cd0; fas that sum + G*g(u) (see the families' contracts above).
 * theta == 1 loads no neighbour: rhs = f + rdt*u on the unknowns, the general expression's value for finite data. For
 * finite data mg_bc_heat_rhs with mask 0, mg_fas_heat_rhs with gamma 0 and, with theta == 1, mg_vc_heat_rhs and
 * mg_fas_heat_rhs give mg_heat_rhs's bits. mg_X_set_form(1) selects the plain kernel here too.
 * MG_ERR_BAD_ARG, with U, RHS and the shift untouched: what mg_heat_step / mg_heat_rhs refuse (same messages, with the
 * function's name), and what mg_X_cycle refuses (step) or mg_X_residual refuses of the handle (rhs): a sawtooth handle, a
 * smoother other than Jacobi or red-black, a stage callback, distributed handles, vc without a coefficient. Nothing is
 * allocated, and no other entry point changes behaviour. */
int mg_vc_heat_rhs(mg_handle h, double dt, double theta, int arr_u, int arr_dst);
int mg_bc_heat_rhs(mg_handle h, double dt, double theta, int arr_u, int arr_dst);
int mg_fas_heat_rhs(mg_handle h, double dt, double theta, int arr_u, int arr_dst);
int mg_vc_heat_step(mg_handle h, double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st);
int mg_bc_heat_step(mg_handle h, double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st);
int mg_fas_heat_step(mg_handle h, double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st);

/* ---- lowest eigenpairs by multigrid-preconditioned LOBPCG ----
 * mg_eig_solve finds the nev smallest eigenpairs of sigma I + A on the interior nodes of level 0, (sigma I + A) x =
 * lambda x with x = 0 on Dirichlet nodes -- the operator of mg_level_coefficients(h, 0): aniso, the current shift
 * (mg_set_shift) and grids that are not 2^k + 1 included -- by LOBPCG (Knyazev 2001) on a block of m >= nev vectors.
 * The preconditioner is M = one outer iteration of mg_solve from zero (outer_pre_gs sweeps + one cycle of the
 * descriptor's kind), exactly mg_pcg_solve's.
 *
 * Each iteration: R_j = AX_j - theta_j X_j and relres_j = ||R_j|| / (|theta_j| ||X_j||); the columns with relres > tol are
 * active (soft locking: the others stay in the Rayleigh-Ritz basis but get no W and no P); W_j = M R_j for the active
 * columns, 0 on Dirichlet nodes; S = [X, W, P]; G = S^T S and H = S^T A S in double on the device; on the host in fp64 the
 * m smallest eigenpairs of H c = theta G c (scaling by diag(G)^-1/2, Cholesky, cyclic Jacobi -- csrc/mg_dense.h); then
 * X' = S Cx, P' = [W, P] Cp (X' without its X part), AX' and AP' likewise, in place. P is absent in the first iteration,
 * after a restart -- a Cholesky pivot of the scaled G below 1e-10: P is dropped for that iteration and `restarts`
 * counts it -- and in an iteration whose active set holds a column the previous one did not (a column that came back
 * from the locked set has no P). The solve stops when columns 0 .. nev-1 all have relres <= tol; hist[k] is the largest
 * of those nev values at iteration k (n_hist may exceed hist_cap: only hist_cap entries are written). With tol below
 * the dtype's rounding floor, about eps_T |cd| / lambda_1, the loop runs to maxit.
 *
 * On return: lambda[0 .. m) ascending and relres[0 .. m), both recomputed from a fresh A X of the returned vectors (one
 * apply, one Gram, one Rayleigh-Ritz rotation of the block), not the running recurrences; the X columns are orthonormal
 * in the Euclidean inner product over the nodes of level 0 and exactly 0 on Dirichlet nodes.
 * status: 0 converged, 1 maxit reached, 2 a Gram entry or norm is not finite or the block is rank-deficient (X is then
 * the last block that was whole).
 *
 * State: the block lives in the handle -- six families of m level-0 arrays (enum mg_eig_family), allocated by the first
 * call (or by mg_eig_set_vector), re-sized by a call with another m, kept until mg_destroy and counted by
 * mg_device_bytes, beside a few MB of partial sums. A second call warm-starts from the X it finds. Columns nobody has
 * set hold the default start: a hash (splitmix64) of the node's global index and the column, uniform in [-1, 1), which
 * has no grid symmetry. mg_eig_set_vector(MG_EIG_X, j, ...) with j beyond the current block grows the block to j + 1.
 * U(0) and RHS(0) are preserved bit for bit (the preconditioner works by swapping pointers into their slots); E, TMP,
 * RES and the coarse levels are unspecified afterwards, as after mg_solve. Two host synchronisations per iteration: the
 * stopping test / active set, and the dense problem. Two runs give the same bits.
 *
 * MG_ERR_BAD_ARG with nothing touched: m outside [1, MG_EIG_MAX_BLOCK], nev outside [1, m], m above the number of
 * interior nodes, tol not positive and finite, maxit < 0, a bad history buffer, NULL lambda / relres, distributed handles
 * (dry runs included), a stage callback installed, an unknown family, j outside the block, NULL handle. The device
 * variants follow every rule of mg_set_array_device.
 *
 * THE OPERATOR FAMILIES. The operator of a call is OR-ed into an argument it already has, as
 * MG_FAS_ON_* is into the kind of mg_fas_set_reaction: mg_eig_solve(h, m | MG_EIG_OPERATOR(op), ...) and
 * mg_eig_kernel(h, kernel | MG_EIG_OPERATOR(op), ...), op an enum mg_eig_operator. There is no entry point of its own and
 * the handle keeps nothing: every call names its operator, and everything the choice stands for is read at that call:
 *   MG_EIG_ON_CONSTANT     the default, everything above;
 *   MG_EIG_ON_FACES        mg_bc_*'s operator: the constant stencil of level 0 with the current shift and the faces of
 *                          mg_bc_set_faces Neumann (mask 0: MG_EIG_ON_CONSTANT, bit for bit);
 *   MG_EIG_ON_COEFFICIENT  mg_vc_*'s operator sigma u - div(a grad u): the coefficient of mg_vc_set_coefficient, the shift and
 *                          the faces of mg_vc_set_faces.
 * Node classes are mg_bc_*'s: a node on a face outside the mask is a Dirichlet node, x = 0 there; every other node is an
 * unknown whose missing neighbours are mirror images. With Neumann faces L is not symmetric but diag(w) L is, w = 1/2 per
 * Neumann face a node lies on, and L x = lambda x is solved in that inner product: G = S^T diag(w) S, H = S^T diag(w) L S,
 * relres_j = ||R_j||_w / (|theta_j| ||X_j||_w), the returned X is w-orthonormal (X^T diag(w) X = I). The preconditioner is
 * one cycle of the family (mg_bc_cycle / mg_vc_cycle from zero, as in mg_vc_pcg_solve; no Gauss-Seidel sweeps before it).
 * Everything else -- the host dense step, soft locking, restarts, the exit by a fresh apply -- is as above. The block may
 * be kept across a change of operator, mask, shift or coefficient: a solve first zeroes X on the Dirichlet nodes of its
 * operator and recomputes A X, and uses no P in its first iteration. mg_eig_kernel honours the operator too: A is the
 * family's operator and G, H and sums carry w.
 * MG_ERR_BAD_ARG with nothing touched, beside the list above (m is checked against the unknowns of the mask): an unknown
 * op (bits 8 and up of m / kernel other than 0, 1, 2), MG_EIG_ON_COEFFICIENT without a coefficient, what the family's cycle refuses (a cycle that is not
 * V / W / F, a smoother other than MG_SMOOTH_JACOBI / MG_SMOOTH_RBGS), distributed handles, and the singular case: every
 * face of the box in the mask and shift == 0 -- the operator then has the eigenvalue 0 and relres divides by |theta|; set a
 * positive shift and subtract it from the eigenvalues. */
#define MG_EIG_MAX_BLOCK 8
enum mg_eig_family { MG_EIG_X = 0, MG_EIG_AX = 1, MG_EIG_W = 2, MG_EIG_AW = 3, MG_EIG_P = 4, MG_EIG_AP = 5 };
typedef struct mg_eig_stats {
    int32_t iters;      /* LOBPCG iterations done                                        */
    int32_t status;     /* 0 converged, 1 hit maxit, 2 a Gram entry / norm not finite    */
    int32_t cycles;     /* preconditioner applications (= active columns summed over iterations) */
    int32_t restarts;   /* iterations that dropped P because the basis Gram matrix was not safely positive definite */
    double  max_relres; /* max over the first nev columns of the returned relres         */
} mg_eig_stats;
int mg_eig_solve(mg_handle h, int m, int nev, double tol, int maxit,
                 double *lambda /*m*/, double *relres /*m*/,
                 double *hist, int hist_cap, int *n_hist, mg_eig_stats *st);
int mg_eig_set_vector(mg_handle h, int family, int j, const void *host);   /* dense, desc.dtype, usual layout */
int mg_eig_get_vector(mg_handle h, int family, int j, void *host);
int mg_eig_set_vector_device(mg_handle h, int family, int j, const void *dev, int dtype, void *stream);
int mg_eig_get_vector_device(mg_handle h, int family, int j, void *dev, int dtype, void *stream);
int mg_eig_block(mg_handle h, int *m);   /* block size currently allocated, 0: none */
enum mg_eig_operator { MG_EIG_ON_CONSTANT = 0 /* the default */, MG_EIG_ON_FACES = 1, MG_EIG_ON_COEFFICIENT = 2 };
#define MG_EIG_OPERATOR(op) ((op) << 8)   /* OR-ed into mg_eig_solve's m (<= MG_EIG_MAX_BLOCK) or mg_eig_kernel's kernel */

/* Kernel-level check of the two block kernels of mg_eig.hip on the handle's block of m = mg_eig_block columns.
 * APPLY_GRAM: the first nw W columns and np P columns (np = 0 or nw) are active. AW_j = A W_j (row order of the
 *             residual kernel, in T; W_j := 0 on Dirichlet nodes). G, H (s x s row-major doubles, s = m + nw + np) over
 *             S = [X, W, P], AS = [AX, AW, AP]: G_ab = S_a . S_b and H_ab = S_a . AS_b for a <= b, both mirrored into
 *             the lower triangle (H is symmetric when AS really is A S). Products and sums in double, fixed order.
 * COMBINE:    coef = Cx (s x m) followed by Cp ((nw+np) x nw), row-major doubles; theta (m doubles). In place:
 *             X' = S Cx, AX' = AS Cx, P' = [W, P] Cp, AP' = [AW, AP] Cp; each element starts at 0.0 in double, adds
 *             (double) S_i * C_ij in the column order of S with every product and sum rounded, and is rounded once to T.
 *             R into the W family's first m columns: r = ax' - (T) theta_j * x', in T. sums[j] = sum r_j^2 (m doubles).
 * With kernel | MG_EIG_OPERATOR(op): A is the family's operator (Dirichlet nodes and mirrors by its mask), every product of G and H
 * and every r^2 of sums carries the node's weight w; the arrays COMBINE writes are the same bits whatever the operator.
 * MG_ERR_BAD_ARG: no block, nw outside [0, m], np not 0 or nw, a NULL output, distributed handles, MG_EIG_ON_COEFFICIENT
 * without a coefficient. */
enum mg_eig_kernel_kind { MG_EIG_K_APPLY_GRAM = 0, MG_EIG_K_COMBINE = 1 };
int mg_eig_kernel(mg_handle h, int kernel, int nw, int np, const double *coef, const double *theta,
                  double *G, double *H, double *sums);

/* Debug stage dumps of the sawtooth cycle -- the reference's CREATE_GIF twin
 * (multigrid.hpp:160-316) writes `sol + err` sampled on the level being worked on after every
 * stage: before and after the coarse solve, after each interpolation, after each level's
 * sweeps, and the corrected solution. With a callback installed mg_cycle does the same
 * (synchronising after every stage): `values` is a dense host array of n*n*nz elements of the
 * descriptor's dtype, `stage` counts the calls since the callback was installed (the
 * reference's frame counter). fn == NULL removes it. Single-GPU handles only. */
typedef void (*mg_stage_fn)(void *user, int stage, int level, int n, int nz, const void *values);
int mg_set_stage_callback(mg_handle h, mg_stage_fn fn, void *user);

int mg_sync(mg_handle h);
/* HIP-event timing on the handle's own stream (torch.cuda.Event would not see it) */
int mg_timer_start(mg_handle h);
int mg_timer_stop(mg_handle h, double *milliseconds);
/* In-region kernel timing for bench.py: between begin and end every finest-grid
 * smoother call made by mg_cycle/mg_cycle_async/mg_smooth is bracketed by HIP events on
 * the handle's stream. end synchronises and returns the summed time and the number of
 * sweeps (kernel launches; a red-black sweep counts once, both colours included). */
int mg_profile_begin(mg_handle h);
int mg_profile_end(mg_handle h, double *smoother_ms, int *smoother_sweeps);
/* A V-cycle folds the prolongation into the first post-smoothing pair when it can (one
 * launch computing J(J(u + P e))); those segments are not smoother-only work, so they are
 * left out of mg_profile_end's totals and reported here (valid after mg_profile_end). */
int mg_profile_fused(mg_handle h, double *fused_ms, int *fused_sweeps);
/* The same events, by kind of finest-level launch (valid after mg_profile_end): summed milliseconds and
 * number of launches of  MG_PROF_SMOOTH          smoother launches (a fused pair is ONE launch of two sweeps)
 *                        MG_PROF_SMOOTH_PROLONG  the post-smoothing launch that also applies P e
 *                        MG_PROF_RESID_RESTRICT  residual + restriction of level 0 (fused or as two kernels)
 *                        MG_PROF_PROLONG         separate prolongation into level 0 */
enum mg_prof_kind { MG_PROF_SMOOTH = 0, MG_PROF_SMOOTH_PROLONG = 1, MG_PROF_RESID_RESTRICT = 2, MG_PROF_PROLONG = 3, MG_PROF_KINDS = 4 };
int mg_profile_get(mg_handle h, int kind, double *ms, int *launches);
/* bytes of HBM held by the handle */
int mg_device_bytes(mg_handle h, size_t *bytes);

/* TEST AND DEBUGGING WINDOW, not a data path: the whole allocation behind one level-shaped array of a single-GPU handle --
 * (nz + 2 ghost) planes x ny rows x pitch elements, ghost planes and padding columns included -- as the kernels see it.
 * tests/test_storage_gpu.py holds every kernel entry point to the layout's invariant with it (padding
 * columns and ghost planes are +0 and stay +0). Neither call launches a kernel, allocates, or changes any state of the
 * handle that a driver caches; use mg_set_array / mg_get_array (or their _device twins) to move data.
 *   space                 index                          level     the array
 *   MG_RAW_LEVEL          enum mg_array                  any       the slot's CURRENT buffer (out-of-place sweeps swap U / TMP)
 *   MG_RAW_VC             0                              any       the coefficient of mg_vc_set_coefficient
 *   MG_RAW_KRYLOV         0 .. 4                         0         the buffers of mg_pcg_solve / mg_vc_pcg_solve
 *   MG_RAW_MIXED          0 = b64, 1 = u64, 2 = its twin 0         fp64 arrays of mg_mixed_*: 8-byte elements, their own pitch
 *   MG_RAW_EIG            family * MG_EIG_MAX_BLOCK + j  0         column j of an enum mg_eig_family
 *   MG_RAW_HEAT           0                              0         the source of mg_heat_set_source
 *   MG_RAW_O4             0 = b4, 1 = u4, 2 = its twin   0         the outer arrays of mg_o4_solve
 * mg_debug_raw_layout fills *out for any admissible (space, index, level); allocated == 0 when the handle has not made that
 * array yet (the geometry is the one it will have). Element (z, y, x) of the dense array is element
 * ((z + ghost) * ny + y) * pitch + x of the allocation.
 * mg_debug_raw_copy copies the whole allocation host -> device (to_device != 0) or device -> host on the handle's stream
 * and waits for it. bytes must equal elems * elem_size. An upload into MG_ARR_RHS drops the level's cached halo state as
 * mg_set_array does; nothing else is touched (mg_mixed_solve's "array was set" flags included).
 * MG_ERR_BAD_ARG, nothing copied: NULL handle, NULL out / host, distributed handles (dry runs included: their ghost planes
 * are live halo), an unknown space, index or level, an array that is not allocated (copy), bytes of another size. */
enum mg_raw_space { MG_RAW_LEVEL = 0, MG_RAW_VC = 1, MG_RAW_KRYLOV = 2, MG_RAW_MIXED = 3, MG_RAW_EIG = 4, MG_RAW_HEAT = 5,
                    MG_RAW_O4 = 6, MG_RAW_SPACES = 7 };
typedef struct mg_debug_raw_info {
    int32_t elem_size;   /* 8 or 4                                        */
    int32_t nx, ny, nz;  /* dense extents                                 */
    int32_t pitch;       /* elements per row, >= nx                       */
    int32_t ghost;       /* ghost planes either side of the nz dense ones */
    int32_t allocated;   /* 0: the handle has not allocated this array    */
    int32_t reserved;
    uint64_t elems;      /* (nz + 2 * ghost) * ny * pitch                 */
} mg_debug_raw_info;
int mg_debug_raw_layout(mg_handle h, int space, int index, int level, mg_debug_raw_info *out);
int mg_debug_raw_copy(mg_handle h, int space, int index, int level, void *host, size_t bytes, int to_device);

/* ---- multi-GPU (z-slab domain decomposition, RCCL halo exchange) ---- */
#define MG_COMM_ID_BYTES 128
/* rank 0 creates the RCCL unique id; the caller ships it to the other ranks by any
 * means (bench.py: torch.distributed broadcast) */
int mg_comm_unique_id(void *id128);
/* single-process smoke test of the RCCL transport on the current device: communicator of
 * one rank, grouped send/recv to self of `bytes` bytes, all-reduce of one double */
int mg_comm_selftest(size_t bytes);
/* rank / size of the handle's decomposition and what the transport itself reports (RCCL: ncclCommCount;
 * 1 for a single-GPU handle); transport = "none" | "rccl" | "host-callbacks" (static string) */
int mg_comm_info(mg_handle h, int *rank, int *nranks, int *transport_ranks, const char **transport);
/* cumulative communication of this rank since creation: message groups posted (halo exchanges, gathers, scatters,
 * all-reduces: one ncclGroup / one host batch each) and bytes sent in them */
int mg_comm_stats(mg_handle h, long long *groups, long long *bytes_sent);
/* like mg_create, for rank `rank` of `nranks` (one process per GPU) */
int mg_create_distributed(const mg_desc *desc, int device, int rank, int nranks,
                          const void *id128, mg_handle *out);
/* The same distributed solver with the exchanges delegated to the HOST (test transport:
 * the library stages halo planes through pinned host buffers and calls back; tests wire the
 * callbacks to torch.distributed/gloo so two processes sharing one GPU can exercise the
 * whole multi-rank path). `batch` must post every op of the list concurrently and return
 * when all have completed; `allreduce_sum` sums n doubles over all ranks in place. Both
 * return 0 on success. */
typedef struct mg_p2p_op {
    int32_t peer;     /* rank to send to / receive from */
    int32_t is_send;  /* 1 = send, 0 = receive          */
    void   *buf;      /* host buffer                    */
    size_t  bytes;
} mg_p2p_op;
typedef struct mg_host_comm {
    void *ctx;
    int (*batch)(void *ctx, const mg_p2p_op *ops, int nops);
    int (*allreduce_sum)(void *ctx, double *vals, int n);
} mg_host_comm;
int mg_create_distributed_hostcomm(const mg_desc *desc, int device, int rank, int nranks,
                                   const mg_host_comm *comm, mg_handle *out);
/* MEASUREMENT ONLY: rank `rank` of `nranks` with no peers -- every exchange and all-reduce is a no-op, so the
 * results are meaningless; the handle runs one rank's launch schedule (slab kernels, boundary launches, replicated
 * coarse levels) so that its compute time can be measured on a single GPU (bench.py --transport dry). */
int mg_create_distributed_dryrun(const mg_desc *desc, int device, int rank, int nranks, mg_handle *out);
/* host-only partition plan (no GPU needed): z-planes [z0, z0+nz) of level l owned by
 * rank r, and the first level that is agglomerated on rank 0 */
int mg_plan_slab(const mg_desc *desc, int nranks, int rank, int level, int *z0, int *nz,
                 int *first_gathered_level);

#ifdef __cplusplus
}
#endif
#endif /* MG_HIP_H */
