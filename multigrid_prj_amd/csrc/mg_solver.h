// mg_solver.h -- host-side owner of the HBM-resident grid hierarchy behind the C-ABI of include/mg_hip.h. One class, two
// translation units: mg_solver.cpp holds the hierarchy, the communication, the per-operator launch paths and the cycle
// (vcycle_rec_t for the V, W and F kinds, visit_child_t, subcycle_launch_t, cycle_from_t, cycle_enqueue*, cycle); mg_drivers.cpp
// holds what calls the cycle from above (solve, pcg_*, fmg*, subcycle, mixed_*, set_shift, heat_*, eig_*) and the helpers those drivers share.
// The member templates that mg_drivers.cpp calls and mg_solver.cpp defines (smooth_t, pair_norm_ok, residual_t, sumsq_t,
// restrict_t, prolong_t, coarse_level_t, vcycle_rec_t, cycle_from_t, subcycle_launch_t) cross the file boundary by ONE mechanism: explicit instantiation definitions
// for double and float, in one block at the end of mg_solver.cpp.
#ifndef MG_SOLVER_H
#define MG_SOLVER_H

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/mg_hip.h"
#include "mg_comm.h"
#include "mg_geom.h"
#include "mg_kernels.h"

// early returns of the mg_status functions of both translation units
#define MG_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            mg::set_last_error(std::string(#call) + ": " + hipGetErrorString(e_));           \
            return MG_ERR_HIP;                                                               \
        }                                                                                    \
    } while (0)
#define MG_TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

namespace mg {

void set_last_error(const std::string &msg);
const std::string &last_error();
int validate_desc(const mg_desc *d, std::string *why);
int level_n(const mg_desc &d, int level);
int level_nz(const mg_desc &d, int level);  // planes of a level (== n unless semi-coarsening)
void level_coefficients(const mg_desc &d, int level, double out[4]);

struct SlabPlan {
    int z0 = 0, nz = 0;           // owned planes of this rank on the level
    int first_gathered_level = 0;  // levels >= this live on rank 0 only
};
// host-only partition arithmetic (no HIP call), shared by the library and the CPU tests
int plan_slab(const mg_desc &d, int nranks, int rank, int level, SlabPlan *out, std::string *why);
// the planes of the FIRST GATHERED level (level == first_gathered_level) that coincide with this
// rank's slab of the last distributed level: what the rank restricts into / prolongs from before
// the level is gathered on / after it is scattered from rank 0
int plan_stage(const mg_desc &d, int nranks, int rank, SlabPlan *out, std::string *why);

constexpr int NUM_ARR = 5;

inline bool is_zebra(int smoother) { return smoother == MG_SMOOTH_ZEBRA_Y || smoother == MG_SMOOTH_ZEBRA_X; }
// the cycles of the V-cycle's recursion (every level holds a solution, not an error): V, W and F
inline bool is_vwf(int cycle) { return cycle == MG_CYCLE_V || cycle == MG_CYCLE_W || cycle == MG_CYCLE_F; }

struct Level {
    Geom g{};
    size_t alloc_elems = 0;      // (nz + 2) * plane
    void *base[NUM_ARR] = {};    // allocations (ghost plane first)
    double coef[4] = {};
    double cd0 = 0;              // coef[3] as created (level_coefficients): coef[3] = cd0 + the handle's shift (mg_set_shift)
    bool present = true;         // false: level not held by this rank (gathered on rank 0)
    bool dist = false;           // true: z-slab of a level distributed over all ranks
    int nz_min = 0;              // thinnest slab of the level over all ranks (== g.nz when the level is not distributed)
    int gh = 1;                  // ghost planes either side of the owned ones: 2 on distributed levels (one exchange then
                                 // feeds a fused sweep pair / residual + restriction), 1 elsewhere (unused, zero)
    bool overlap = false;        // distributed level whose slabs are big enough for the interior launch to hide the halo exchange
                                 // (MG_OVERLAP_MIN_MB, decided on the thinnest slab: the same answer on every rank)
    bool rhs_halo_ok = false;    // distributed level: the RHS array's first ghost planes hold the neighbours' planes
    void *zebra = nullptr;       // MG_SMOOTH_ZEBRA_Y / _X: cp(j), den(j) of the line solve (2 * ny or 2 * nx values, device)
    void *vc_a = nullptr;        // mg_vc_*: the level's diffusion coefficient, level-shaped like base[] (allocated by the first set)
};

class Solver {
public:
    // takes ownership of `comm` (nullptr: single GPU)
    Solver(const mg_desc &d, int device, Comm *comm = nullptr);
    ~Solver();
    int init();  // allocates; returns mg_status

    int set_array(int which, int level, const void *host);
    int stage_rows(int which, int level, void *host, bool to_device);
    int get_array(int which, int level, void *host);
    int zero_array(int which, int level);
    // the same arrays from / into a dense DEVICE array of the caller, ordered against the caller's stream, no host
    // synchronisation (mg_set_array_device / mg_get_array_device)
    int array_device(int which, int level, void *dense, int dense_dtype, bool to_handle, hipStream_t caller);

    int smooth(int level, int smoother, int sweeps, int arr_x, int arr_rhs);
    int residual(int level, int arr_x, int arr_rhs, int arr_r, double *sumsq);
    int sumsq(int level, int arr, double *out);
    int restrict_to(int fine_level, int kind, int arr_src, int arr_dst);
    int prolong(int coarse_level, int add, int arr_src, int arr_dst);
    int correct(int arr_u, int arr_e);
    int coarse_solve(int level, int arr_x, int arr_rhs, mg_cycle_stats *st);
    int coarse_solve_ex(int level, int arr_x, int arr_rhs, int smoother, int maxit, double tol, int fixed,
                        mg_cycle_stats *st);
    int cycle(mg_cycle_stats *st);
    int cycle_async(int count);
    // lock_counts != nullptr: outer iteration i < n_lock runs its coarse solve for exactly
    // lock_counts[i] sweeps (mg_solve_lockstep)
    int solve(double tol, int maxit, double *hist, int hist_cap, int *n_hist,
              mg_cycle_stats *per_cycle, const int *lock_counts = nullptr, int n_lock = 0);
    // multigrid-preconditioned flexible CG on level 0 (mg_pcg_solve); the Krylov buffers are allocated on the first call
    int pcg_solve(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_krylov_stats *st);
    // one of the three vector kernels of pcg_solve on level-0 arrays (mg_pcg_kernel)
    int pcg_kernel(int kernel, double scalar, const int *arrs, double *dots);
    // full multigrid (nested iteration): coarsest-grid solve, then per level cubic interpolation of the solution +
    // cycles_per_level V-cycles started on that level (mg_fmg)
    int fmg(int cycles_per_level, mg_fmg_stats *st);
    // arr_dst(l) = Pi arr_src(l + 1), Dirichlet nodes from arr_bnd(l) (< 0: interpolated too) (mg_fmg_prolong)
    int fmg_prolong(int coarse_level, int arr_src, int arr_dst, int arr_bnd);
    int fmg_prolong_mask(int mask, int coarse_level, int arr_src, int arr_dst, int arr_bnd);   // its checks and launch, by a face mask
    // one cyc(level, kind) on U(level), RHS(level): launch by launch (path 0) or by the LDS kernel rooted there (path 1)
    int subcycle(int level, int kind, int path, mg_cycle_stats *st);
    // root level the handle's cycles hand to the LDS kernel, -1: none
    int subcycle_root() const { return stage_fn_ ? -1 : sub_root_; }
    // mixed-precision defect correction: fp64 u / b of level 0 beside an MG_F32 hierarchy (mg_mixed_*); the fp64 arrays are
    // allocated by the first mixed_set_*
    int mixed_set(bool rhs, const double *host);
    int mixed_get_solution(double *host);
    int mixed_set_device(bool rhs, const void *dense, int dense_dtype, hipStream_t caller);
    int mixed_get_solution_device(void *dense, int dense_dtype, hipStream_t caller);
    int mixed_solve(double tol, int maxit, int inner_cycles, double *hist, int hist_cap, int *n_hist, mg_mixed_stats *st);
    int mixed_kernel(int kernel, double scale_in, double scale_out, int arr_e32, int arr_r32, double *sumsq_r);
    // fourth-order defect correction on level 0 (mg_o4_*): the residual with sigma I + A4, the correction by the handle's
    // own cycles; b4 and two copies of u4 are allocated by the first o4_solve
    int o4_residual(int arr_u, int arr_b, int arr_r, double *sumsq_r);
    int o4_correct_residual(int arr_u, int arr_e, int arr_b, int arr_unew, int arr_r, double *sumsq_r);
    int o4_solve(double tol, int maxit, int inner_cycles, double *hist, int hist_cap, int *n_hist, mg_o4_stats *st);
    // the operator sigma I + A on every level (mg_set_shift): coef[3] = cd0 + sigma, zebra line factors re-tabulated
    int set_shift(double sigma);
    double shift() const { return shift_; }
    // implicit theta-scheme steps of u_t = -A0 u + f on level 0 (mg_heat_*); the source array is allocated by the first
    // heat_set_source
    int heat_set_source(const void *host);
    int heat_set_source_device(const void *dense, int dense_dtype, hipStream_t caller);
    int heat_step(double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st);
    int heat_rhs(double dt, double theta, int arr_u, int arr_dst);
    // the same steps of u_t = -N0(u) + f with N0 the unshifted operator of a family (mg_vc_heat_*, mg_bc_heat_*, mg_fas_heat_*);
    // f is the one source of the handle
    int vc_heat_rhs(double dt, double theta, int arr_u, int arr_dst);
    int bc_heat_rhs(double dt, double theta, int arr_u, int arr_dst);
    int fas_heat_rhs(double dt, double theta, int arr_u, int arr_dst);
    int vc_heat_step(double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st);
    int bc_heat_step(double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st);
    int fas_heat_step(double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st);
    // lowest eigenpairs of sigma I + A on level 0 by multigrid-preconditioned LOBPCG (mg_eig_*); the block of 6 m level-0
    // arrays is allocated on first use and kept until the handle goes
    int eig_solve(int m, int nev, double tol, int maxit, double *lambda, double *relres, double *hist, int hist_cap, int *n_hist,
                  mg_eig_stats *st);
    int eig_vector(int family, int j, void *host, bool to_handle);
    int eig_vector_device(int family, int j, void *dense, int dense_dtype, bool to_handle, hipStream_t caller);
    int eig_block() const { return eig_m_; }
    int eig_kernel(int kernel, int nw, int np, const double *coef, const double *theta, double *G, double *H, double *sums);
    // variable-coefficient diffusion -div(a grad u) + sigma u (mg_vc_*): one coefficient array per level, allocated by the
    // first vc_set_coefficient*; level l + 1 is the full-weighted level l
    int vc_set_coefficient(const void *host);
    int vc_set_coefficient_device(const void *dense, int dense_dtype, hipStream_t caller);
    int vc_get_coefficient(int level, void *host);
    int vc_set_form(int form);   // tests and measurement tools: 1 = the plain kernels on every level, 0 = the default
    int vc_residual(int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r);
    int vc_smooth(int level, int smoother, int sweeps, int arr_x, int arr_rhs);
    int vc_coarse_solve(int level, int arr_x, int arr_rhs, mg_cycle_stats *st);
    int vc_cycle(mg_cycle_stats *st);
    int vc_solve(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle);
    int vc_pcg_solve(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_krylov_stats *st);
    int vc_direction(double beta, int arr_z, int arr_p, int arr_pn, int arr_q, double *pq);   // the direction kernel alone
    // Neumann faces of mg_vc_*: a second face mask, independent of bc_set_faces; with a non-zero mask the coarse coefficients
    // are the MIRRORED full weighting of the stored level 0 (set_faces re-restricts when a coefficient is set)
    int vc_set_faces(int mask);
    int vc_get_faces(int *mask) const;
    int vc_restrict(int fine_level, int kind, int arr_src, int arr_dst);   // mg_bc_restrict with this mask
    int vc_project(int level, int arr, double *mean);                      // mg_bc_project with this mask
    // the constant operator with Neumann faces (mg_bc_*): a face mask (enum mg_face), nothing allocated
    int bc_set_faces(int mask);
    int bc_get_faces(int *mask) const;
    int bc_set_form(int form);   // tests and measurement tools: 1 = the plain kernels on every level, 0 = the default
    int bc_residual(int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r);
    int bc_smooth(int level, int smoother, int sweeps, int arr_x, int arr_rhs);
    int bc_restrict(int fine_level, int kind, int arr_src, int arr_dst);
    int bc_coarse_solve(int level, int arr_x, int arr_rhs, mg_cycle_stats *st);
    int bc_project(int level, int arr, double *mean);
    int bc_cycle(mg_cycle_stats *st);
    int bc_solve(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle);
    // the semilinear operator (sigma I + A) u + gamma g(u) by the full approximation scheme (mg_fas_*): a kind and gamma, nothing allocated
    int fas_set_reaction(int kind, double gamma);
    int fas_get_reaction(int *kind, double *gamma) const;
    int fas_set_form(int form);   // tests and measurement tools: 1 = the plain kernels on every level, 0 = the default
    int fas_residual(int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r);
    int fas_smooth(int level, int smoother, int sweeps, int arr_x, int arr_rhs);
    int fas_coarse_rhs(int fine_level);
    int fas_correct(int fine_level);
    int fas_coarse_solve(int level, int arr_x, int arr_rhs, mg_cycle_stats *st);
    int fas_cycle(mg_cycle_stats *st);
    int fas_solve(double rtol, double atol, int maxit, double *hist, int hist_cap, int *n_hist, mg_fas_stats *st);
    int set_stage_callback(mg_stage_fn fn, void *user);
    int sync();
    int timer_start();
    int timer_stop(double *ms);
    int profile_begin();
    int profile_end(double *ms, int *sweeps);
    int profile_fused(double *ms, int *sweeps) const;
    int profile_get(int kind, double *ms, int *launches) const;
    int comm_info(int *rank, int *nranks, int *transport_ranks, const char **transport) const;
    size_t device_bytes() const { return bytes_; }
    // test and debugging window (mg_debug_raw_*): the whole allocation behind one level-shaped array, ghost planes and
    // padding columns included; no kernel, no allocation, no driver state
    int raw_layout(const char *fn, int space, int index, int level, mg_debug_raw_info *out, void **dev = nullptr) const;
    int raw_copy(int space, int index, int level, void *host, size_t bytes, bool to_device);
    long long comm_groups() const { return comm_groups_; }
    long long comm_bytes_sent() const { return comm_bytes_; }

    const mg_desc &desc() const { return d_; }
    int nlevels() const { return d_.levels; }
    const Level &level(int l) const { return lv_[l]; }

private:
    template <typename T> T *ptr(int which, int level) const   // local plane 0: skips the lower ghost plane(s)
    {
        const Level &L = lv_[level];
        return reinterpret_cast<T *>(L.base[which]) + L.gh * L.g.plane;
    }
    template <typename T> static Coef<T> coef_of(const Level &L)
    {
        Coef<T> c = make_coef<T>(L.coef[0], L.coef[1], L.coef[2], L.coef[3]);
        if (!switches().fast_div) c.win = 0;  // A/B switch: hardware division everywhere
        return c;
    }
    // the level's UNSHIFTED operator (cd0): what the time steppers apply to u; nothing divides by its diagonal
    template <typename T> static Coef<T> coef0_of(const Level &L) { return make_coef<T>(L.coef[0], L.coef[1], L.coef[2], L.cd0); }
    // x_zero: the caller knows x == 0 (fresh coarse-level guess): the first Jacobi sweep of a
    // fast-path level then skips reading x (and the caller skips the memset)
    template <typename T> int smooth_t(int level, int smoother, int sweeps, int ax, int ar, bool x_zero = false,
                                       int corr_level = -1, bool e_scratch = false, bool u_halo_ok = false);
    template <typename T> bool can_fold_prolong(int level) const;
    template <typename T> bool can_fold_prolong_slab(int level) const;   // both levels distributed: the slab pair folds P e in
    template <typename T> bool can_fold_prolong_replicated(int level) const;   // slab level over a level every rank holds whole
    template <typename T> int pair_on_slab_t(int level, bool rb);
    template <typename T> int pair_on_slab2_t(int level, bool rb, int corr_level = -1, bool u_halo_ok = false, double *norm_partials = nullptr, int *norm_np = nullptr);   // depth-2 ghosts: one exchange, the fused kernel on the whole slab
    template <typename T> int resid_restrict_on_slab_t(int level, const Geom &gc, T *coarse_rhs);
    int refresh_rhs_halo(int level);
    template <typename T> bool can_skip_zeroing(int level) const;
    template <typename T> int residual_t(int level, int ax, int ar, int arr_r, bool want_norm);
    template <typename T> int sumsq_t(int level, int arr);
    template <typename T> int restrict_t(int fl, int kind, int as, int ad);
    template <typename T> int prolong_t(int cl, int add, int as, int ad);
    template <typename T> int correct_t(int level, int au, int ae);
    template <typename T> int coarse_full_t();
    // coarse "solve" of level l: persistent one-workgroup kernel, or -- when the level is too big
    // for one workgroup and the mode is MG_COARSE_FIXED -- coarse_maxit regular sweeps
    template <typename T> int coarse_level_t(int l, int ax, int ar, bool x_zero = false);  // coarse solve of a still-distributed coarsest level, gathered
    int exchange(int which, int level, int depth = 1);        // `depth` ghost planes <-> z-neighbours (on the main stream)
    // the same on the comm stream, after the main stream's work so far; record = false: the caller puts more work that needs the halo
    // on the comm stream (the boundary pieces of a slab operation) and records the event itself with halo_work_done()
    int exchange_begin(int which, int level, int depth = 1, bool record = true);
    int halo_work_done();
    // level whose U boundary planes were last written on the COMMUNICATION stream (by the boundary piece of a slab pair) with
    // nothing touching U since: the next exchange of those planes needs no wait for the main stream. -1: none.
    int pair_on_comm_level_ = -1;
    int halo_ops(int which, int level, int depth, P2POp *ops);
    int exchange_end();                          // main stream waits for the halo
    // Runs a stencil launch over a distributed level with the halo exchange of `arr_x` hidden
    // behind the interior planes: launch(sub-slab geometry, element offset of its first plane)
    template <typename F> int overlapped(int level, int arr_x, F &&launch);
    int gather_S(int arr);                       // staging rhs slabs -> lv_[T_+1].base[arr] on rank 0
    int scatter_S(int arr);                      // lv_[T_+1].base[arr] on rank 0 -> staging u slabs (+ upper ghost)
    template <typename T> T *stageptr(int k) const { return reinterpret_cast<T *>(stage_base_[k]) + stage_g_.plane; }
    int gather_T(int which, int fullk);          // slabs of level T_ -> full_[fullk] on rank 0
    int scatter_T(int fullk, int which);         // full_[fullk] on rank 0 -> slabs of level T_
    int allreduce(double *dptr, int n);
    template <typename T> T *fullptr(int k) const { return reinterpret_cast<T *>(full_[k]) + gfull_.plane; }
    template <typename T> int coarse_t(int level, int ax, int ar, bool x_zero = false);
    template <typename T> int coarse_ex_t(int level, int ax, int ar, int smoother, int maxit, double tol, int fixed, bool x_zero = false);
    template <typename T> int cycle_enqueue_t();
    // ---- shared by the drivers (mg_drivers.cpp)
    // One outer iteration of mg_solve on (U, RHS) of level 0: outer_pre_gs lexicographic Gauss-Seidel sweeps if asked, then
    // one cycle. Stream-ordered, no synchronisation.
    int outer_iteration_enqueue();
    // Refuses what `refuse` names, then makes the handle's device current and clears the per-call driver state
    // (pair_on_comm_level_, lock_iters_, fine_pre_done_). Messages start with "<fn>: ".
    enum : unsigned { REFUSE_DIST = 1u, REFUSE_STAGE_CB = 2u };   // a distributed handle / an installed stage callback
    int driver_begin(const char *fn, unsigned refuse);
    // h_scal_[slot .. slot + n) = dev[0 .. n), then waits for the stream
    int fetch_scalars(int slot, const double *dev, int n = 1);
    // h_coarse_ = *d_coarse_ (with_fine: and the cycle's fine sum r^2), one wait for the stream, then *st (may be null)
    int fetch_cycle_stats(mg_cycle_stats *st, bool with_fine = false);
    void fill_cycle_stats(mg_cycle_stats *st, double fine_sumsq_r) const;   // from h_coarse_ as it stands
    // *p = nbytes of zeroed device memory (the memset is queued on stream_), counted in bytes_. Level-shaped arrays made
    // this way keep their ghost planes and padding columns zero: on a one-GPU level no kernel writes a ghost plane, and the
    // padding columns are written only with zeros (the tail-line stores of mg_device.h, the line store of mg_fmg.hip).
    // tests/test_storage_gpu.py holds every entry point to that.
    int alloc_zeroed(void **p, size_t nbytes);
    template <typename T> int pcg_t(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_krylov_stats *st);
    // pcg_t's and vc_pcg_t's iteration; the two callables are the operator's residual with its sum and its direction kernel.
    // vc_mask != 0 (mg_vc_pcg_solve on a handle with Neumann faces): the Dirichlet copy and the two dots are the mask's
    // (launch_bc_dirichlet_copy, launch_vc_cg_wdots); singular (every face in the mask and no shift: the caller decides): RHS(0),
    // every z and the final x are projected, each projection with a fetch of its mean
    template <typename T, class ResidualSum, class DirectionApply>
    int pcg_body_t(bool vc, ResidualSum residual_sum, DirectionApply direction_apply, double tol, int maxit, double *hist, int hist_cap,
                   int *n_hist, mg_krylov_stats *st, int vc_mask = 0, bool singular = false);
    // *z = M r: one mg_solve outer iteration from zero with the buffers *z and r in level 0's U / RHS slots. The cycle may leave
    // its result in the buffer that was TMP: *z is whatever U points at afterwards, and TMP keeps the other buffer.
    // PRE_VC / PRE_BC: the cycle is mg_vc_cycle's (mg_vc_pcg_solve, mg_eig_solve on the coefficient) / mg_bc_cycle's
    // (mg_eig_solve on the faces) and no Gauss-Seidel sweeps come before it
    enum Precond { PRE_CONSTANT = 0, PRE_VC = 1, PRE_BC = 2 };
    int precondition(void **z, void *r, Precond fam = PRE_CONSTANT);
    template <typename T> int pcg_kernel_t(int kernel, double scalar, const int *arrs, double *dots);
    template <typename T> int fmg_t(int cycles_per_level, mg_fmg_stats *st);
    int mixed_check(const char *fn, unsigned refuse = REFUSE_DIST);      // MG_F32, then driver_begin(fn, refuse)
    int mixed_alloc();
    int mixed_solve_vc(double tol, int maxit, int count, bool inner_pcg, double *hist, int hist_cap, int *n_hist, mg_mixed_stats *st);   // MG_MIXED_ON_COEFFICIENT
    // U(0) = 0, then inner_cycles outer iterations of mg_solve on RHS(0): the approximate solve of the correction equation
    // of mixed_solve and o4_solve; no synchronisation
    int correction_cycles(int inner_cycles);
    int stage_copy(char *dev, const Geom &g, size_t es, void *host, bool to_device);   // stage_rows on any level-shaped array
    // stage_copy's twin for a dense array in device memory: device_check, then the copy kernel (mg_io.hip) on stream_ between
    // two event hand-overs with the caller's stream -- it runs after what `caller` holds, and what `caller` gets afterwards
    // runs after it. dev_padded: local plane 0, elements of es bytes. No host synchronisation.
    int device_copy(const char *fn, char *dev_padded, const Geom &g, size_t es, void *dense, int dense_dtype, bool to_padded,
                    hipStream_t caller);
    // MG_ERR_BAD_ARG unless `dense` is device memory of device_ that holds g.nx * g.ny * g.nz elements of dense_dtype from
    // there on; enqueues and allocates nothing
    int device_check(const char *fn, const void *dense, int dense_dtype, const Geom &g);
    int krylov_scalars_alloc();
    int krylov_alloc();
    // cyc(l, kind) of mg_desc.h; kind V is the V-cycle, launch for launch what it was before W and F existed
    template <typename T> int vcycle_rec_t(int l, bool u_zero = false, int kind = MG_CYCLE_V);
    // what a level does with its child l1: U(l1) = 0, cyc(l1, kind) and the second visit W / F make -- by launches, or by
    // one launch of the LDS kernel when l1 is the handle's sub-cycle root
    template <typename T> int visit_child_t(int l1, int kind);
    // one cycle of the descriptor's kind (V / W / F) started on level l, the W / F statistics accumulated into d_coarse_
    template <typename T> int cycle_from_t(int l);
    template <typename T> int subcycle_launch_t(int root, int kind, bool second, bool u_zero);
    SubcyclePlan subcycle_plan_of(int root) const;   // mg::subcycle_plan on this handle's hierarchy (single GPU)
    int sub_root_ = -1;               // level the cycles hand to the LDS kernel (MG_SUBCYCLE_LEVEL, init()); -1: none
    CoarseOut *d_coarse_acc_ = nullptr;   // W / F: the cycle's coarse solves summed up (launch_coarse_accum)
    bool acc_stats_ = false;          // a W / F cycle is being enqueued: every coarse solve is added to d_coarse_acc_
    int stats_begin();                // clears d_coarse_acc_, sets acc_stats_
    int stats_end();                  // d_coarse_ = d_coarse_acc_, clears acc_stats_
    int cycle_enqueue();
    bool check_arr(int which, int level, const char *fn) const;
    int zebra_tabulate(Level &L);   // the level's zebra line factors from its current coefficients -> L.zebra
    size_t esize() const { return d_.dtype == MG_F64 ? 8 : 4; }

    mg_desc d_;
    int device_;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
    hipEvent_t ev_stage_[2] = {nullptr, nullptr};   // one per half of the host staging buffer (stage_rows)
    hipEvent_t ev_io_[2] = {nullptr, nullptr};      // device_copy: [0] caller's stream -> stream_, [1] stream_ -> caller's stream
    std::vector<Level> lv_;
    double *d_partials_ = nullptr;  // per-block partial sums
    // Slots of the pinned h_scal_. d_scal_ has the same slots; only the first three are written on the device (the Krylov and
    // mixed-precision sums have device buffers of their own). A new driver adds a slot here, it does not borrow one.
    enum ScalSlot {
        SC_RR = 0,        // sum r^2: residual_t, the norm carried by a pre-smoothing pair (smooth_t hands d_scal_ itself to it)
        SC_BB = 1,        // sum of squares of an array: sumsq_t (follows SC_RR: heat_step fetches the two in one copy)
        SC_CYCLE_RR = 2,  // the sawtooth cycle's fine sum r^2 (a copy of SC_RR taken inside the cycle)
        SC_CG_DOT = 3,    // the two sums of pcg_kernel's check (fetched in one copy)
        SC_CG_DOT1 = 4,
        SC_MX_SUM = 5,    // d_mx_sum_: mixed_solve, mixed_kernel
        SC_O4_SUM = 6,    // sum r^2 of the fourth-order residual: o4_solve, o4_residual, o4_correct_residual (written on the device)
        SC_FAM_SUM = 7,   // mg_vc_*, mg_bc_*, mg_fas_*: sum r^2 of the family's residual, or bc_project's sum w v (written on the
                          // device; every call fetches its sum before another family runs)
        SC_COUNT = 8      // the eight slots: one 64-byte line
    };
    double *d_scal_ = nullptr;      // [SC_COUNT]
    CoarseOut *d_coarse_ = nullptr;
    double *h_scal_ = nullptr;      // pinned mirrors ([SC_COUNT])
    CoarseOut *h_coarse_ = nullptr;
    CoarseOut *h_fixed_ = nullptr;  // pinned: stats reported when the coarse level is swept, not solved
    size_t bytes_ = 0;
    // slab decomposition (mg_create_distributed*): levels 0..T_ are distributed, deeper
    // levels live on rank 0; full_[] are rank 0's gathered copies of level T_
    Comm *comm_ = nullptr;
    int rank_ = 0, nranks_ = 1, T_ = -1;
    hipStream_t comm_stream_ = nullptr;
    hipEvent_t ev_ready_ = nullptr, ev_halo_ = nullptr;
    void *h_stage_ = nullptr;      // pinned staging buffer of set_array / get_array
    size_t h_stage_bytes_ = 0;
    HandleSwitches sw_;  // the HANDLE rows of mg_switches.def as init() found them (replicate_tail: gathered levels are held and run by every rank)
    long long comm_groups_ = 0, comm_bytes_ = 0;   // message groups posted / bytes sent by this rank (mg_comm_stats)
    int post(const P2POp *ops, int n, hipStream_t s);  // comm_->batch + the counters
    int lock_iters_ = -1;  // >= 0: the next coarse solve runs exactly this many sweeps (lock-step parity mode)
    // Outer loop with the residual norm taken inside the next cycle's first pre-smoothing pair (Solver::solve): want_pair_norm_
    // asks smooth_t for it, pair_norm_done_ says the launch delivered it into d_scal_[0], fine_pre_done_ tells vcycle_rec_t how
    // many of level 0's pre-smoothing sweeps have already run (Jacobi: the pair = 2; red-black: the first sweep = 1).
    bool want_pair_norm_ = false, pair_norm_done_ = false;
    int fine_pre_done_ = 0;
    template <typename T> bool pair_norm_ok() const;
    // Krylov state of pcg_solve (allocated on first use, kept until the handle goes): level-0-shaped buffers z, r, p, p', q
    // -- z and r take the U / RHS slots of level 0 while the preconditioning cycle runs; device scalars + partial sums
    enum { KZ = 0, KR = 1, KP0 = 2, KP1 = 3, KQ = 4, NKRY = 5 };
    void *kry_[NKRY] = {};
    CgScalars *d_cg_ = nullptr, *h_cg_ = nullptr;
    double *d_cg_part_ = nullptr;
    double *d_cg_dot_ = nullptr;    // [2]: sums of the kernel check (mg_pcg_kernel)
    // fp64 outer arrays of mixed_solve (allocated on first use, kept until the handle goes): b64 and two copies of u64 -- the
    // fused correction + residual launch writes u out of place and the two are swapped, like U / TMP under a sweep
    enum { MXB = 0, MXU = 1, MXU2 = 2, NMX = 3 };
    void *mx_[NMX] = {};
    Geom g64_{};                    // level 0 with the fp64 pitch
    size_t mx_alloc_elems_ = 0;
    bool mx_has_b_ = false, mx_has_u_ = false;
    double *d_mx_part_ = nullptr, *d_mx_sum_ = nullptr;   // per-workgroup partial sums and their total
    double *mxptr(int k) const { return reinterpret_cast<double *>(mx_[k]) + g64_.plane; }   // local plane 0
    // outer arrays of o4_solve (allocated on first use, kept until the handle goes): b4 and two copies of u4, level-0 shaped
    enum { O4B = 0, O4U = 1, O4U2 = 2, NO4 = 3 };
    void *o4_[NO4] = {};
    int o4_check(const char *fn, unsigned refuse);   // driver_begin(fn, refuse), then n >= 7 on every axis of level 0
    int o4_partials_cap_ = 0;                        // room in d_partials_ (set by init)
    template <typename T> int o4_kernel_t(bool corr, int arr_u, int arr_e, int arr_b, int arr_unew, int arr_r, double *sumsq_r);
    template <typename T> int o4_solve_t(double tol, int maxit, int inner_cycles, double *hist, int hist_cap, int *n_hist, mg_o4_stats *st);
    // diagonal shift of every level (set_shift) and the stepper's source term f: one more level-0 array (allocated on first
    // use, kept until the handle goes); heat_has_f_ == false: f = 0, the array is not read
    double shift_ = 0;
    int heat_check(const char *fn, double dt, double theta);   // driver_begin(fn, REFUSE_DIST), then dt > 0, theta in (0, 1], finite shift
    template <typename T> int heat_rhs_t(double dt, double theta, int arr_u, int arr_dst);
    template <typename T> int heat_step_t(double dt, double theta, int nsteps, int cycles_per_step);
    void *heat_f_ = nullptr;
    bool heat_has_f_ = false;
    // ---- operator families (mg_vc_*, mg_bc_*, mg_fas_*): one driver skeleton, the fam_* templates, over a policy F<T> per
    // family (defined in mg_drivers.cpp) that supplies what differs: the residual / Jacobi / red-black colour / coarse launches
    // with the family's plain flag, the precondition of the check, and the cycle's hooks on the way down and up
    template <typename T> struct VcFam;
    template <typename T> struct BcFam;
    template <typename T> struct FasFam;
    enum : unsigned { FAM_NEED_CYCLE = 1u, FAM_NEED_SMOOTHER = 2u };   // what fam_check asks of the descriptor beyond F's own precondition
    template <template <typename> class F> int fam_check(const char *fn, unsigned need);   // driver_begin, F::ready, the cycle / smoother the family drivers run
    int set_form(const char *fn, int form, bool *plain);   // mg_*_set_form
    template <class F> int fam_residual_t(int level, int ax, int ar, int arr_r, bool want_sum, int slot = SC_FAM_SUM);   // the sum -> d_scal_[slot]
    template <class F> int fam_residual_sum_t(int level, int ax, int ar, int arr_r, double *sumsq_r);   // ... and fetched: synchronises
    template <class F> int fam_smooth_t(int level, int smoother, int sweeps, int ax, int ar);
    template <class F> int fam_coarse_t(int level, int ax, int ar);
    template <class F> int fam_cycle_rec_t(int l, int kind);
    template <class F> int fam_cycle_enqueue_t();
    template <class F> int fam_solve_t(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle);   // vc, bc
    // nested iteration on the family's operator (mg_fmg with MG_FMG_OPERATOR): the mirrored FMG interpolation by F::mask
    template <class F> int fam_fmg_t(int count, mg_fmg_stats *st);
    template <template <typename> class F> int fam_fmg(int count, mg_fmg_stats *st);   // fam_check, then by the handle's dtype
    template <template <typename> class F> int fam_fmg_prolong(int coarse_level, int arr_src, int arr_dst, int arr_bnd);
    template <template <typename> class F> int fam_cycle_enqueue();   // by the handle's dtype
    // the public mg_<family>_<fn>: fam_check, the argument checks (messages start with fn), then the template by dtype
    template <template <typename> class F> int fam_residual(const char *fn, int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r);
    template <template <typename> class F> int fam_smooth(const char *fn, int level, int smoother, int sweeps, int arr_x, int arr_rhs);
    template <template <typename> class F> int fam_coarse_solve(const char *fn, int level, int arr_x, int arr_rhs, mg_cycle_stats *st);
    template <template <typename> class F> int fam_cycle(const char *fn, mg_cycle_stats *st);
    template <template <typename> class F>
    int fam_solve(const char *fn, double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle);
    // mg_<family>_heat_rhs / mg_<family>_heat_step: heat_check, fam_check, then F::heat_rhs (one launch) and the family's cycle
    template <class F> int fam_heat_rhs_t(double dt, double theta, int arr_u, int arr_dst);
    template <class F> int fam_heat_step_t(double dt, double theta, int nsteps, int cycles_per_step);   // sums -> SC_RR, SC_BB
    template <template <typename> class F> int fam_heat_rhs(const char *fn, double dt, double theta, int arr_u, int arr_dst);
    template <template <typename> class F>
    int fam_heat_step(const char *fn, double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st);
    // variable-coefficient drivers (mg_vc_*): Level::vc_a of every level, valid once vc_set_ is true
    bool vc_set_ = false, vc_plain_ = false;
    int vc_alloc();
    template <typename T> T *vcptr(int level) const { return reinterpret_cast<T *>(lv_[level].vc_a) + lv_[level].gh * lv_[level].g.plane; }
    template <typename T> int vc_restrict_all_t();   // vc_a(l + 1) = full weighting of vc_a(l) (mirrored with a mask), every transition
    int vc_mask_ = 0;   // the Neumann faces of mg_vc_* (mg_vc_set_faces), 0 = all Dirichlet
    bool vc_singular() const { return vc_mask_ == (d_.dim == 3 ? 63 : 15) && shift_ == 0.0; }   // constants are the null space
    template <typename T> int vc_direction_t(double beta, const int *arrs, double *pq);
    template <typename T> int vc_pcg_t(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_krylov_stats *st);
    // Neumann-face drivers (mg_bc_*): the mask of Neumann faces, 0 = all Dirichlet
    int bc_mask_ = 0;
    bool bc_plain_ = false;
    bool bc_singular() const { return bc_mask_ == (d_.dim == 3 ? 63 : 15) && shift_ == 0.0; }   // all faces Neumann, no shift: constants are the null space
    // the two below take the mask as an argument: mg_vc_* runs them with its own
    template <typename T> int bc_restrict_t(int mask, int fl, int kind, int as, int ad);
    template <typename T> int bc_project_t(int mask, int level, int arr, double *mean);   // synchronises: the mean is fetched
    template <typename T> int bc_project_ptr_t(int mask, const Geom &g, T *v, double *mean);   // the same on a level-shaped buffer
    int face_mask_check(const char *fn, int mask);
    int fam_restrict(const char *fn, int mask, int fine_level, int kind, int arr_src, int arr_dst);
    // full-approximation-scheme drivers (mg_fas_*): the reaction gamma g(u), g of enum mg_fas_kind
    int fas_kind_ = MG_FAS_CUBIC;
    double fas_gamma_ = 0.0;
    bool fas_plain_ = false;
    bool fas_faces_ = false;   // MG_FAS_ON_FACES: the linear part is mg_bc_*'s operator with bc_mask_, read at call time
    bool fas_coef_ = false;    // MG_FAS_ON_COEFFICIENT: the linear part is mg_vc_*'s operator (vc_a, shift_) with vc_mask_, read at call time
    int fas_mask() const { return fas_coef_ ? vc_mask_ : (fas_faces_ ? bc_mask_ : 0); }
    template <typename T> int fas_coarse_rhs_t(int fl);
    template <typename T> int fas_correct_t(int fl);
    template <typename T> int fas_solve_t(double rtol, double atol, int maxit, double *hist, int hist_cap, int *n_hist, mg_fas_stats *st);
    // block of eig_solve: eig_[family][column] (enum mg_eig_family), level-0-shaped; the per-workgroup partial sums of up to
    // EIG_MAX_LAUNCHES Gram tiles, their totals, the coefficients of the combine (device) and a pinned mirror of the last two
    enum { EIG_FAMILIES = 6, EIG_MAX_LAUNCHES = 9, EIG_HOST_DOUBLES = 2048 };
    enum EigGramMode { EIG_GRAM_X = 0, EIG_GRAM_ITER = 1, EIG_GRAM_FULL = 2 };
    void *eig_[EIG_FAMILIES][MG_EIG_MAX_BLOCK] = {};
    int eig_m_ = 0;
    double *d_eig_part_ = nullptr, *d_eig_out_ = nullptr, *d_eig_coef_ = nullptr, *h_eig_ = nullptr;
    int eig_op_ = MG_EIG_ON_CONSTANT;   // the operator of the eig_solve / eig_kernel call in progress (enum mg_eig_operator): taken
                                        // from the call's m / kernel argument (MG_EIG_OPERATOR) at its entry, nothing keeps it between calls
    // m_or_kernel = value | MG_EIG_OPERATOR(op) -> value, eig_op_ = op; an unknown op is refused
    int eig_take_operator(const char *fn, int *m_or_kernel);
    // the operator as the block kernels take it, from the handle's state NOW: MG_EIG_ON_FACES with mask 0 is the constant one
    template <typename T> EigOp<T> eig_op_t() const;
    // what eig_solve and eig_kernel refuse because of the operator: the family's own precondition (cycle: and what its cycle
    // asks of the descriptor)
    int eig_op_check(const char *fn, bool cycle);
    int eig_check(const char *fn, int family, int j, bool may_grow);   // driver_begin + the family / column rules
    int eig_resize(int m);
    // G, H (s x s, s = m or m + nw + np) of the block. EIG_GRAM_X: S = [X], AX = A X made on the way (X := 0 on Dirichlet
    // nodes); EIG_GRAM_ITER: S = [X, W, P], AW made, the X x X block left as the caller filled it; EIG_GRAM_FULL: every block
    template <typename T> int eig_gram_t(int mode, int nw, int np, double *G, double *H);
    template <typename T> int eig_combine_t(int nw, int np, const double *coef, const double *theta, double *sums);
    template <typename T> int eig_t(int nev, double tol, int maxit, double *lambda, double *relres, double *hist, int hist_cap,
                                    int *n_hist, mg_eig_stats *st);
    Geom gfull_{};
    void *full_[3] = {nullptr, nullptr, nullptr};
    std::vector<SlabPlan> planT_;
    // staging slab of the first gathered level (every rank): [0] restricted rhs, [1] correction
    Geom stage_g_{};
    void *stage_base_[2] = {nullptr, nullptr};
    std::vector<SlabPlan> planS_;
    // CREATE_GIF-style stage dumps (mg_set_stage_callback)
    int dump_stage(int level, bool add_err);
    mg_stage_fn stage_fn_ = nullptr;
    void *stage_user_ = nullptr;
    int stage_count_ = 0;
    std::vector<char> stage_u_, stage_e_;
    // in-region timing of the finest-grid smoother (mg_profile_begin/end)
    bool profiling_ = false;
    std::vector<hipEvent_t> prof_ev_;
    size_t prof_used_ = 0;
    int prof_sweeps_ = 0;
    std::vector<int> prof_kind_;   // per event pair: mg_prof_kind
    std::vector<int> prof_units_;  // per event pair: sweeps (smoother kinds) or 1
    std::vector<int> prof_launches_;
    double prof_fused_ms_ = 0;
    int prof_fused_sweeps_ = 0;
    double prof_ms_[MG_PROF_KINDS] = {};
    int prof_n_[MG_PROF_KINDS] = {};
    // brackets [begin, end) with HIP events when profiling the finest level
    int prof_begin(int level);
    int prof_end(int level, int kind, int units, int launches);
};

}  // namespace mg
#endif
