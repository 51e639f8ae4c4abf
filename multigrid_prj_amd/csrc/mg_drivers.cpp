// mg_drivers.cpp -- the solve drivers of mg::Solver: everything that calls the cycle from above (mg_solve, mg_pcg_*, mg_fmg*,
// mg_mixed_*, mg_o4_*, mg_set_shift, mg_heat_*, mg_eig_*, mg_vc_*, mg_bc_*, mg_fas_*) and the helpers they share. The hierarchy and the cycle itself are in mg_solver.cpp.
// Reference call structure being replaced by solve(): the outer loop of src/main.cpp:72-116.
#include "mg_solver.h"
#include "mg_dense.h"

#include <algorithm>
#include <cmath>

namespace mg {

// ---------------------------------------------------------------- what the drivers share
int Solver::driver_begin(const char *fn, unsigned refuse)
{
    if ((refuse & REFUSE_DIST) && nranks_ > 1) {
        set_last_error(std::string(fn) + ": distributed handles are not supported (single-GPU handles only)");
        return MG_ERR_BAD_ARG;
    }
    if ((refuse & REFUSE_STAGE_CB) && stage_fn_) {
        set_last_error(std::string(fn) + ": a stage callback is installed (remove it with mg_set_stage_callback(h, NULL, NULL))");
        return MG_ERR_BAD_ARG;
    }
    MG_HIP(hipSetDevice(device_));
    pair_on_comm_level_ = -1;
    lock_iters_ = -1;
    fine_pre_done_ = 0;
    return MG_OK;
}

int Solver::outer_iteration_enqueue()
{
    if (d_.outer_pre_gs > 0)                                 // `u * GS * GS` main.cpp:85
        MG_TRY(d_.dtype == MG_F64 ? smooth_t<double>(0, MG_SMOOTH_GS_LEX, d_.outer_pre_gs, MG_ARR_U, MG_ARR_RHS)
                                  : smooth_t<float>(0, MG_SMOOTH_GS_LEX, d_.outer_pre_gs, MG_ARR_U, MG_ARR_RHS));
    return cycle_enqueue();                                  // `* MGx`
}

// ---------------------------------------------------------------- mg_solve
// Outer loop of src/main.cpp:72-116.
int Solver::solve(double tol, int maxit, double *hist, int hist_cap, int *n_hist,
                  mg_cycle_stats *per_cycle, const int *lock_counts, int n_lock)
{
    MG_HIP(hipSetDevice(device_));
    double nb = 0, nr = 0;
    MG_TRY(sumsq(0, MG_ARR_RHS, &nb));                       // Residual ctor, solvers.hpp:237-242
    const bool fused_norm = !lock_counts && (d_.dtype == MG_F64 ? pair_norm_ok<double>() : pair_norm_ok<float>());
    if (fused_norm) {
        // Same loop, same history: entry k is the norm after k cycles. It is computed by the first pre-smoothing pair of cycle
        // k + 1, which runs before the test; when the test says stop (or maxit is reached) that pair's output is dropped -- it
        // was written out of place, U still holds the iterate the norm belongs to.
        Level &L0 = lv_[0];
        int nh = 0;
        for (int it = 0; it <= maxit; it++) {
            void *const base_u = L0.base[MG_ARR_U], *const base_t = L0.base[MG_ARR_TMP];
            want_pair_norm_ = true; pair_norm_done_ = false;
            // the speculative launch: the Jacobi pair (both pre-smoothing sweeps), or the first red-black sweep -- ONE out-of-place
            // launch either way, so the iterate the norm belongs to is still whole when the test says stop
            const int spec = d_.smoother == MG_SMOOTH_JACOBI ? d_.nu_pre : 1;
            const int rc = d_.dtype == MG_F64 ? smooth_t<double>(0, d_.smoother, spec, MG_ARR_U, MG_ARR_RHS, false, -1, true)
                                              : smooth_t<float>(0, d_.smoother, spec, MG_ARR_U, MG_ARR_RHS, false, -1, true);
            want_pair_norm_ = false;
            MG_TRY(rc);
            if (!pair_norm_done_) { set_last_error("mg_solve: the pre-smoothing pair did not deliver the residual norm"); return MG_ERR_HIP; }
            MG_TRY(fetch_scalars(SC_RR, d_scal_ + SC_RR));
            nr = h_scal_[SC_RR];
            if (per_cycle && it > 0) fill_cycle_stats(&per_cycle[it - 1], 0.0);   // the coarse solver's record of the cycle that has just finished
            const double rel = std::sqrt(nr / nb);
            if (hist && nh < hist_cap) hist[nh] = rel;
            nh++;
            if ((it > 0 && rel <= tol) || it == maxit) {     // main.cpp:88-89 / the loop bound: drop the speculative pair
                L0.base[MG_ARR_U] = base_u; L0.base[MG_ARR_TMP] = base_t;
                break;
            }
            fine_pre_done_ = spec;
            const int crc = cycle_enqueue();
            fine_pre_done_ = 0;
            MG_TRY(crc);
            if (per_cycle) MG_HIP(hipMemcpyAsync(h_coarse_, d_coarse_, sizeof(CoarseOut), hipMemcpyDeviceToHost, stream_));
        }
        MG_HIP(hipStreamSynchronize(stream_));
        if (n_hist) *n_hist = nh;
        return MG_OK;
    }
    MG_TRY(residual(0, MG_ARR_U, MG_ARR_RHS, -1, &nr));      // main.cpp:73-74
    int nh = 0;
    if (hist && nh < hist_cap) hist[nh] = std::sqrt(nr / nb);
    nh++;
    for (int it = 0; it < maxit; it++) {
        lock_iters_ = (lock_counts && it < n_lock) ? lock_counts[it] : -1;
        const int crc = outer_iteration_enqueue();
        lock_iters_ = -1;
        MG_TRY(crc);
        MG_TRY(fetch_cycle_stats(per_cycle ? &per_cycle[it] : nullptr, true));   // as mg_cycle reports them
        MG_TRY(residual(0, MG_ARR_U, MG_ARR_RHS, -1, &nr));  // main.cpp:86
        double rel = std::sqrt(nr / nb);
        if (hist && nh < hist_cap) hist[nh] = rel;
        nh++;
        if (rel <= tol) break;                               // main.cpp:88-89
    }
    if (n_hist) *n_hist = nh;
    return MG_OK;
}

// ---------------------------------------------------------------- multigrid-preconditioned flexible CG (mg_pcg_solve)
int Solver::krylov_scalars_alloc()
{
    if (d_cg_) return MG_OK;
    const size_t npart = (size_t)cg_partials_capacity();
    MG_HIP(hipMalloc((void **)&d_cg_, sizeof(CgScalars)));
    MG_HIP(hipMalloc((void **)&d_cg_part_, sizeof(double) * npart));
    MG_HIP(hipMalloc((void **)&d_cg_dot_, sizeof(double) * 2));
    MG_HIP(hipHostMalloc((void **)&h_cg_, sizeof(CgScalars)));
    bytes_ += sizeof(CgScalars) + sizeof(double) * (npart + 2);
    return MG_OK;
}

int Solver::krylov_alloc()
{
    MG_TRY(krylov_scalars_alloc());
    if (kry_[0]) return MG_OK;
    const size_t nbytes = lv_[0].alloc_elems * esize();
    for (auto &b : kry_) MG_TRY(alloc_zeroed(&b, nbytes));
    return MG_OK;
}

// z = M r: the cycle code works on level 0's U / RHS slots, so z and r take them for the duration (pointer swap, no copy).
// The cycle may itself leave its result in the array that was TMP (out-of-place sweeps swap U / TMP): whatever U points
// at afterwards is z, and TMP keeps the other buffer.
int Solver::precondition(void **z, void *r, Precond fam)
{
    Level &L0 = lv_[0];
    void *const x_base = L0.base[MG_ARR_U], *const b_base = L0.base[MG_ARR_RHS];
    MG_HIP(hipMemsetAsync(*z, 0, L0.alloc_elems * esize(), stream_));
    L0.base[MG_ARR_U] = *z;
    L0.base[MG_ARR_RHS] = r;
    const int rc = fam == PRE_VC ? fam_cycle_enqueue<VcFam>() : (fam == PRE_BC ? fam_cycle_enqueue<BcFam>() : outer_iteration_enqueue());
    *z = L0.base[MG_ARR_U];
    L0.base[MG_ARR_U] = x_base;
    L0.base[MG_ARR_RHS] = b_base;
    return rc;
}

// The flexible CG iteration of mg_pcg_solve and mg_vc_pcg_solve on level 0. What the two operators do differently comes in:
// residual_sum(r, v): r = b - A x (r may be null), *v = r.r, fetched (it synchronises); direction_apply(z, p, pn, q): pn = z +
// beta p, q = A pn, returns the number of partial sums of pn.q; vc: precondition()'s flag.
// vc_mask != 0: L is self-adjoint in the inner product of the weights w (1/2 per Neumann face of a node), so z.r, z.q and
// p.q carry them (the direction kernel's partials come weighted); the stopping test stays the plain norm. In the singular case
// the iteration lives on the complement of the constants: RHS(0) is projected first, z after every cycle, x at the end.
template <typename T, class ResidualSum, class DirectionApply>
int Solver::pcg_body_t(bool vc, ResidualSum residual_sum, DirectionApply direction_apply, double tol, int maxit, double *hist,
                       int hist_cap, int *n_hist, mg_krylov_stats *st, int vc_mask, bool singular)
{
    if (singular) MG_TRY(bc_project_t<T>(vc_mask, 0, MG_ARR_RHS, nullptr));
    Level &L0 = lv_[0];
    const Geom &g = L0.g;
    auto kp = [&](int k) { return reinterpret_cast<T *>(kry_[k]) + L0.gh * g.plane; };
    T *const x = ptr<T>(MG_ARR_U, 0);
    const T *const b = ptr<T>(MG_ARR_RHS, 0);
    mg_krylov_stats out{0, 0, 0.0, 0.0};
    int nh = 0;
    auto record = [&](double rel) { if (hist && nh < hist_cap) hist[nh] = rel; nh++; out.relres = rel; };

    double nb = 0;
    MG_TRY(sumsq(0, MG_ARR_RHS, &nb));
    // Dirichlet rows are identity rows carrying the boundary data: x takes b's values there, after which r, z, p and q
    // vanish on the boundary and the iteration lives on the interior, where A is symmetric positive definite
    if (vc_mask) launch_bc_dirichlet_copy<T>(stream_, g, vc_mask, x, b);
    else launch_cg_boundary_copy<T>(stream_, g, x, b);
    MG_HIP(hipGetLastError());
    double rr0 = 0;
    MG_TRY(residual_sum(kp(KR), &rr0));   // r0 = b - A x0, r0.r0
    record(std::sqrt(rr0 / nb));

    if (nb == 0.0 || rr0 == 0.0) {
        out.status = 0;   // nothing to do: b == 0 (x0 = 0 is the answer once its boundary is b's) or x0 solves the system
    } else if (maxit == 0) {
        out.status = 1;
    } else {
        MG_HIP(hipMemsetAsync(d_cg_, 0, sizeof(CgScalars), stream_));
        int pc = KP0, pn = KP1;   // p ping-pongs: another workgroup may still read p_k at a neighbour while p_{k+1} is written
        MG_HIP(hipMemsetAsync(kry_[pc], 0, L0.alloc_elems * esize(), stream_));   // p_{-1} = 0: p_0 = z_0 + 0 p_{-1} = z_0
        auto direction = [&](int mode) -> int {   // z = M r, gamma, beta, p_{k+1} = z + beta p_k, q = A p_{k+1}, alpha
            MG_TRY(precondition(&kry_[KZ], kry_[KR], vc ? PRE_VC : PRE_CONSTANT));
            if (singular) MG_TRY(bc_project_ptr_t<T>(vc_mask, g, kp(KZ), nullptr));   // fetches the mean: a second synchronisation per iteration, in this case only
            int np = vc_mask ? launch_vc_cg_wdots<T>(stream_, g, vc_mask, kp(KZ), kp(KR), kp(KQ), d_cg_, d_cg_part_)
                             : launch_cg_dots<T>(stream_, g, kp(KZ), kp(KR), kp(KQ), d_cg_, d_cg_part_);
            launch_cg_tail(stream_, mode, d_cg_part_, np, d_cg_);
            np = direction_apply(kp(KZ), kp(pc), kp(pn), kp(KQ));
            launch_cg_tail(stream_, CG_TAIL_ALPHA, d_cg_part_, np, d_cg_);
            MG_HIP(hipGetLastError());
            std::swap(pc, pn);
            return MG_OK;
        };
        MG_TRY(direction(CG_TAIL_FIRST));
        for (int k = 0; k < maxit; k++) {
            const int np = launch_cg_update<T>(stream_, g, x, kp(pc), kp(KR), kp(KQ), d_cg_, d_cg_part_);
            launch_cg_tail(stream_, CG_TAIL_RR, d_cg_part_, np, d_cg_);
            MG_HIP(hipGetLastError());
            MG_HIP(hipMemcpyAsync(h_cg_, d_cg_, sizeof(CgScalars), hipMemcpyDeviceToHost, stream_));
            MG_HIP(hipStreamSynchronize(stream_));   // the stopping test: the one host synchronisation per iteration (the singular masked case has the projection's too)
            if (h_cg_->bad) { out.status = 2; break; }   // the update was skipped: x is the last iterate
            out.iters = k + 1;
            const double rel = std::sqrt(h_cg_->rr / nb);
            record(rel);
            if (rel <= tol) { out.status = 0; break; }
            if (k + 1 == maxit) { out.status = 1; break; }
            MG_TRY(direction(CG_TAIL_BETA));
        }
    }
    if (singular) MG_TRY(bc_project_t<T>(vc_mask, 0, MG_ARR_U, nullptr));
    double nr = 0;
    MG_TRY(residual_sum((T *)nullptr, &nr));   // the true residual of the returned x
    out.relres_true = std::sqrt(nr / nb);
    if (n_hist) *n_hist = nh;
    if (st) *st = out;
    return MG_OK;
}

// A = the handle's constant operator, M r = one mg_solve outer iteration from zero; the sum of the residual comes out of
// launch_residual in SC_RR
template <typename T>
int Solver::pcg_t(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_krylov_stats *st)
{
    const Level &L0 = lv_[0];
    const Coef<T> c = coef_of<T>(L0);
    auto residual_sum = [&](T *r, double *v) -> int {
        launch_residual<T>(stream_, L0.g, c, ptr<T>(MG_ARR_U, 0), ptr<T>(MG_ARR_RHS, 0), r, d_partials_, d_scal_ + SC_RR);
        MG_HIP(hipGetLastError());
        MG_TRY(fetch_scalars(SC_RR, d_scal_ + SC_RR));
        *v = h_scal_[SC_RR];
        return MG_OK;
    };
    auto direction_apply = [&](const T *z, const T *p, T *pn, T *q) {
        return launch_cg_direction_apply<T>(stream_, L0.g, c, z, p, pn, q, d_cg_, d_cg_part_);
    };
    return pcg_body_t<T>(false, residual_sum, direction_apply, tol, maxit, hist, hist_cap, n_hist, st);
}

int Solver::pcg_solve(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_krylov_stats *st)
{
    MG_TRY(driver_begin("mg_pcg_solve", REFUSE_DIST | REFUSE_STAGE_CB));
    MG_TRY(krylov_alloc());
    return d_.dtype == MG_F64 ? pcg_t<double>(tol, maxit, hist, hist_cap, n_hist, st)
                              : pcg_t<float>(tol, maxit, hist, hist_cap, n_hist, st);
}

template <typename T>
int Solver::pcg_kernel_t(int kernel, double scalar, const int *a, double *dots)
{
    const Level &L0 = lv_[0];
    const Geom &g = L0.g;
    *h_cg_ = CgScalars{};
    h_cg_->alpha = h_cg_->beta = scalar;
    MG_HIP(hipMemcpyAsync(d_cg_, h_cg_, sizeof(CgScalars), hipMemcpyHostToDevice, stream_));
    int np = 0;
    if (kernel == MG_PCG_K_UPDATE) {
        np = launch_cg_update<T>(stream_, g, ptr<T>(a[0], 0), ptr<T>(a[1], 0), ptr<T>(a[2], 0), ptr<T>(a[3], 0), d_cg_, d_cg_part_);
        launch_reduce_final(stream_, d_cg_part_, np, d_cg_dot_);
    } else if (kernel == MG_PCG_K_DOTS) {
        np = launch_cg_dots<T>(stream_, g, ptr<T>(a[0], 0), ptr<T>(a[1], 0), ptr<T>(a[2], 0), d_cg_, d_cg_part_);
        launch_reduce_final(stream_, d_cg_part_, np, d_cg_dot_);
        launch_reduce_final(stream_, d_cg_part_ + np, np, d_cg_dot_ + 1);
    } else {
        np = launch_cg_direction_apply<T>(stream_, g, coef_of<T>(L0), ptr<T>(a[0], 0), ptr<T>(a[1], 0), ptr<T>(a[2], 0),
                                          ptr<T>(a[3], 0), d_cg_, d_cg_part_);
        launch_reduce_final(stream_, d_cg_part_, np, d_cg_dot_);
    }
    MG_HIP(hipGetLastError());
    MG_TRY(fetch_scalars(SC_CG_DOT, d_cg_dot_, 2));
    dots[0] = h_scal_[SC_CG_DOT];
    dots[1] = kernel == MG_PCG_K_DOTS ? h_scal_[SC_CG_DOT1] : 0.0;
    return MG_OK;
}

int Solver::pcg_kernel(int kernel, double scalar, const int *arrs, double *dots)
{
    MG_TRY(driver_begin("mg_pcg_kernel", REFUSE_DIST));
    if (kernel < MG_PCG_K_UPDATE || kernel > MG_PCG_K_DIRECTION) { set_last_error("mg_pcg_kernel: unknown kernel"); return MG_ERR_BAD_ARG; }
    const int na = kernel == MG_PCG_K_DOTS ? 3 : 4;
    for (int i = 0; i < na; i++) {
        if (!check_arr(arrs[i], 0, "mg_pcg_kernel")) return MG_ERR_BAD_ARG;
        for (int j = 0; j < i; j++)
            if (arrs[i] == arrs[j]) { set_last_error("mg_pcg_kernel: the arrays must be distinct"); return MG_ERR_BAD_ARG; }
    }
    MG_TRY(krylov_scalars_alloc());
    return d_.dtype == MG_F64 ? pcg_kernel_t<double>(kernel, scalar, arrs, dots)
                              : pcg_kernel_t<float>(kernel, scalar, arrs, dots);
}

// ---------------------------------------------------------------- full multigrid (nested iteration), mg_fmg
// f_{l+1} = R f_l down the hierarchy (the level operators are unscaled and the restrictions inject on the coarse boundary,
// so this carries the right-hand side and the Dirichlet data), the coarsest-grid solve, then coarse to fine: U(l) = Pi U(l+1)
// (mg_fmg.hip; Dirichlet nodes from RHS(l)) and cycles_per_level cycles of the descriptor's kind (V, W or F) started on level l. A cycle started on level l
// only overwrites U and RHS of the levels below it, which the pass has finished with: no storage of its own.
template <typename T>
int Solver::fmg_t(int cycles_per_level, mg_fmg_stats *st)
{
    const int L = d_.levels;
    for (int l = 0; l + 1 < L; l++) MG_TRY(restrict_t<T>(l, d_.restriction, MG_ARR_RHS, MG_ARR_RHS));
    MG_TRY(zero_array(MG_ARR_U, L - 1));
    launch_cg_boundary_copy<T>(stream_, lv_[L - 1].g, ptr<T>(MG_ARR_U, L - 1), ptr<T>(MG_ARR_RHS, L - 1));
    MG_HIP(hipGetLastError());
    MG_TRY(coarse_level_t<T>(L - 1, MG_ARR_U, MG_ARR_RHS, false));
    MG_HIP(hipMemcpyAsync(h_coarse_, d_coarse_, sizeof(CoarseOut), hipMemcpyDeviceToHost, stream_));   // of this first, true coarse solve
    for (int l = L - 2; l >= 0; l--) {
        launch_fmg_prolong<T>(stream_, lv_[l + 1].g, lv_[l].g, ptr<T>(MG_ARR_U, l + 1), ptr<T>(MG_ARR_U, l), ptr<T>(MG_ARR_RHS, l));
        MG_HIP(hipGetLastError());
        for (int k = 0; k < cycles_per_level; k++) MG_TRY(cycle_from_t<T>(l));   // of the descriptor's kind: V, W or F
    }
    double nb = 0, nr = 0;
    MG_TRY(sumsq(0, MG_ARR_RHS, &nb));
    MG_TRY(residual(0, MG_ARR_U, MG_ARR_RHS, -1, &nr));   // synchronises: h_coarse_ is valid from here
    if (st) {
        st->levels = L;
        st->cycles_per_level = cycles_per_level;
        st->coarse_iters = h_coarse_->iters;
        st->coarse_flag = h_coarse_->flag;
        st->relres = std::sqrt(nr / nb);
    }
    return MG_OK;
}

// bits 16 and up of mg_fmg's count / mg_fmg_prolong's level: MG_FMG_OPERATOR(op); anything but the four operators is refused
static int fmg_operator_of(const char *fn, int arg, int *op)
{
    if (arg < 0 || (arg >> 16) > MG_FMG_ON_REACTION) {
        set_last_error(std::string(fn) + ": bits 16 and up must be MG_FMG_OPERATOR(op) with op an enum mg_fmg_operator");
        return MG_ERR_BAD_ARG;
    }
    *op = arg >> 16;
    return MG_OK;
}

int Solver::fmg(int cycles_per_level, mg_fmg_stats *st)
{
    if (cycles_per_level >> 16) {   // flagged (or negative): the pass on a family's operator
        int op = 0;
        MG_TRY(fmg_operator_of("mg_fmg", cycles_per_level, &op));
        const int count = cycles_per_level & 0xffff;
        return op == MG_FMG_ON_FACES ? fam_fmg<BcFam>(count, st) : (op == MG_FMG_ON_COEFFICIENT ? fam_fmg<VcFam>(count, st) : fam_fmg<FasFam>(count, st));
    }
    MG_TRY(driver_begin("mg_fmg", REFUSE_DIST | REFUSE_STAGE_CB));
    if (!is_vwf(d_.cycle)) {
        set_last_error("mg_fmg: the descriptor's cycle must be MG_CYCLE_V (the levels of a sawtooth cycle hold errors, not solutions)");
        return MG_ERR_BAD_ARG;
    }
    if (cycles_per_level < 1) {
        set_last_error("mg_fmg: cycles_per_level must be at least 1");
        return MG_ERR_BAD_ARG;
    }
    return d_.dtype == MG_F64 ? fmg_t<double>(cycles_per_level, st) : fmg_t<float>(cycles_per_level, st);
}

// ---------------------------------------------------------------- one cyc(level, kind), mg_subcycle
// The kernel-level check of mg_subcycle.hip and the building block of a caller's own nested iteration: path 0 runs the cycle
// driver's launches (never the kernel, whatever the handle's root is), path 1 the LDS kernel rooted at `level`.
int Solver::subcycle(int level, int kind, int path, mg_cycle_stats *st)
{
    MG_TRY(driver_begin("mg_subcycle", REFUSE_DIST));
    if (!is_vwf(d_.cycle)) { set_last_error("mg_subcycle: not on a sawtooth handle (its levels hold errors, not solutions)"); return MG_ERR_BAD_ARG; }
    if (!is_vwf(kind)) { set_last_error("mg_subcycle: kind must be MG_CYCLE_V, MG_CYCLE_W or MG_CYCLE_F"); return MG_ERR_BAD_ARG; }
    if (level < 0 || level >= d_.levels) { set_last_error("mg_subcycle: level out of range"); return MG_ERR_BAD_ARG; }
    if (path != 0 && path != 1) { set_last_error("mg_subcycle: path must be 0 (launches) or 1 (the LDS kernel)"); return MG_ERR_BAD_ARG; }
    if (path == 1 && (stage_fn_ || subcycle_plan_of(level).root != level)) {
        set_last_error("mg_subcycle: the LDS kernel does not admit the levels from this one down (mg::subcycle_plan)");
        return MG_ERR_BAD_ARG;
    }
    MG_TRY(stats_begin());
    const int root_saved = sub_root_;
    int rc;
    if (path == 0) {
        sub_root_ = -1;
        rc = d_.dtype == MG_F64 ? vcycle_rec_t<double>(level, false, kind) : vcycle_rec_t<float>(level, false, kind);
        sub_root_ = root_saved;
    } else {
        rc = d_.dtype == MG_F64 ? subcycle_launch_t<double>(level, kind, false, false) : subcycle_launch_t<float>(level, kind, false, false);
    }
    acc_stats_ = false;
    MG_TRY(rc);
    MG_TRY(stats_end());
    return fetch_cycle_stats(st);
}

int Solver::fmg_prolong(int coarse_level, int arr_src, int arr_dst, int arr_bnd)
{
    if (coarse_level >> 16) {   // flagged (or negative): the interpolation by a family's mask
        int op = 0;
        MG_TRY(fmg_operator_of("mg_fmg_prolong", coarse_level, &op));
        const int cl = coarse_level & 0xffff;
        return op == MG_FMG_ON_FACES ? fam_fmg_prolong<BcFam>(cl, arr_src, arr_dst, arr_bnd)
                                     : (op == MG_FMG_ON_COEFFICIENT ? fam_fmg_prolong<VcFam>(cl, arr_src, arr_dst, arr_bnd)
                                                                    : fam_fmg_prolong<FasFam>(cl, arr_src, arr_dst, arr_bnd));
    }
    MG_TRY(driver_begin("mg_fmg_prolong", REFUSE_DIST));
    return fmg_prolong_mask(0, coarse_level, arr_src, arr_dst, arr_bnd);
}

// the argument checks and the launch; mask: the Neumann faces (0: the mask-free launch)
int Solver::fmg_prolong_mask(int mask, int coarse_level, int arr_src, int arr_dst, int arr_bnd)
{
    if (coarse_level < 1 || coarse_level >= d_.levels || !check_arr(arr_src, coarse_level, "mg_fmg_prolong") ||
        !check_arr(arr_dst, coarse_level - 1, "mg_fmg_prolong") || (arr_bnd >= 0 && !check_arr(arr_bnd, coarse_level - 1, "mg_fmg_prolong"))) {
        set_last_error("mg_fmg_prolong: bad level / array");
        return MG_ERR_BAD_ARG;
    }
    if (arr_bnd == arr_dst) { set_last_error("mg_fmg_prolong: arr_bnd must differ from arr_dst"); return MG_ERR_BAD_ARG; }
    const int fl = coarse_level - 1;
    if (arr_dst == MG_ARR_RHS) lv_[fl].rhs_halo_ok = false;
    if (d_.dtype == MG_F64)
        launch_fmg_prolong<double>(stream_, lv_[coarse_level].g, lv_[fl].g, ptr<double>(arr_src, coarse_level), ptr<double>(arr_dst, fl),
                                   arr_bnd >= 0 ? ptr<double>(arr_bnd, fl) : (double *)nullptr, mask);
    else
        launch_fmg_prolong<float>(stream_, lv_[coarse_level].g, lv_[fl].g, ptr<float>(arr_src, coarse_level), ptr<float>(arr_dst, fl),
                                  arr_bnd >= 0 ? ptr<float>(arr_bnd, fl) : (float *)nullptr, mask);
    MG_HIP(hipGetLastError());
    return MG_OK;
}

// ---------------------------------------------------------------- mixed-precision defect correction (mg_mixed_solve)
// u and b of level 0 in fp64 beside the handle's fp32 hierarchy: r = b - A u in fp64, A e = r solved approximately by
// inner_cycles of the fp32 cycles, u += e. The fp32 right-hand side is the residual times a power of two that keeps it
// near 1 (exact both ways); the kernels are in mg_mixed.hip.
int Solver::mixed_check(const char *fn, unsigned refuse)
{
    if (d_.dtype != MG_F32) {
        set_last_error(std::string(fn) + ": the handle has to be created with MG_F32 (the cycles of the mixed-precision solver run in fp32; "
                                         "this handle is MG_F64)");
        return MG_ERR_BAD_ARG;
    }
    return driver_begin(fn, refuse);
}

int Solver::mixed_alloc()
{
    if (mx_[0]) return MG_OK;
    const Level &L0 = lv_[0];
    g64_ = L0.g;
    g64_.pitch = ((L0.g.nx + 15) / 16) * 16;   // rows of doubles padded to 128 B
    g64_.plane = (long long)g64_.ny * g64_.pitch;
    mx_alloc_elems_ = (size_t)(g64_.nz + 2) * (size_t)g64_.plane;   // one (zero, unused) ghost plane either side, as every level
    const size_t nbytes = mx_alloc_elems_ * sizeof(double), npart = (size_t)mixed_partials_capacity();
    for (auto &b : mx_) MG_TRY(alloc_zeroed(&b, nbytes));
    MG_HIP(hipMalloc((void **)&d_mx_part_, sizeof(double) * npart));
    MG_HIP(hipMalloc((void **)&d_mx_sum_, sizeof(double)));
    bytes_ += sizeof(double) * (npart + 1);
    return MG_OK;
}

int Solver::mixed_set(bool rhs, const double *host)
{
    const char *fn = rhs ? "mg_mixed_set_rhs" : "mg_mixed_set_solution";
    MG_TRY(mixed_check(fn));
    MG_TRY(mixed_alloc());
    MG_TRY(stage_copy(reinterpret_cast<char *>(mxptr(rhs ? MXB : MXU)), g64_, sizeof(double), const_cast<double *>(host), true));
    (rhs ? mx_has_b_ : mx_has_u_) = true;
    return MG_OK;
}

int Solver::mixed_get_solution(double *host)
{
    MG_TRY(mixed_check("mg_mixed_get_solution"));
    if (!mx_has_u_) { set_last_error("mg_mixed_get_solution: no solution yet (call mg_mixed_set_solution first)"); return MG_ERR_BAD_ARG; }
    return stage_copy(reinterpret_cast<char *>(mxptr(MXU)), g64_, sizeof(double), host, false);
}

// the device twins: every rule of the host calls above; the copy is Solver::device_copy's (no host synchronisation)
int Solver::mixed_set_device(bool rhs, const void *dense, int dense_dtype, hipStream_t caller)
{
    const char *fn = rhs ? "mg_mixed_set_rhs_device" : "mg_mixed_set_solution_device";
    MG_TRY(mixed_check(fn));
    if (!mx_[0]) MG_TRY(device_check(fn, dense, dense_dtype, lv_[0].g));   // nothing is allocated for an array that is refused
    MG_TRY(mixed_alloc());
    MG_TRY(device_copy(fn, reinterpret_cast<char *>(mxptr(rhs ? MXB : MXU)), g64_, sizeof(double), const_cast<void *>(dense), dense_dtype,
                       true, caller));
    (rhs ? mx_has_b_ : mx_has_u_) = true;
    return MG_OK;
}

int Solver::mixed_get_solution_device(void *dense, int dense_dtype, hipStream_t caller)
{
    const char *fn = "mg_mixed_get_solution_device";
    MG_TRY(mixed_check(fn));
    if (!mx_has_u_) { set_last_error("mg_mixed_get_solution_device: no solution yet (call mg_mixed_set_solution first)"); return MG_ERR_BAD_ARG; }
    return device_copy(fn, reinterpret_cast<char *>(mxptr(MXU)), g64_, sizeof(double), dense, dense_dtype, false, caller);
}

// 2^-e with frexp(sqrt(v)) = (m, e): brings a vector of squared norm v to a norm in [0.5, 1)
static double mixed_scale(double v)
{
    if (!(v > 0.0) || !std::isfinite(v)) return 1.0;
    int e = 0;
    (void)std::frexp(std::sqrt(v), &e);
    return std::ldexp(1.0, -e);
}

int Solver::correction_cycles(int inner_cycles)
{
    MG_HIP(hipMemsetAsync(lv_[0].base[MG_ARR_U], 0, lv_[0].alloc_elems * esize(), stream_));
    for (int c = 0; c < inner_cycles; c++) MG_TRY(outer_iteration_enqueue());
    return MG_OK;
}

int Solver::mixed_solve(double tol, int maxit, int inner_cycles, double *hist, int hist_cap, int *n_hist, mg_mixed_stats *st)
{
    MG_TRY(mixed_check("mg_mixed_solve", REFUSE_DIST | REFUSE_STAGE_CB));
    if (inner_cycles < 1) { set_last_error("mg_mixed_solve: inner_cycles must be at least 1"); return MG_ERR_BAD_ARG; }
    // bits 0 .. 15: the count; MG_MIXED_OPERATOR in bits 16, 17; MG_MIXED_INNER_PCG; no other bit
    const unsigned flags = (unsigned)inner_cycles;
    const int mx_op = (int)((flags >> 16) & 3u);
    const bool inner_pcg = (flags & (unsigned)MG_MIXED_INNER_PCG) != 0;
    inner_cycles = (int)(flags & 0xffffu);
    if ((flags & ~(0xffffu | (3u << 16) | (unsigned)MG_MIXED_INNER_PCG)) || (mx_op != MG_MIXED_ON_CONSTANT && mx_op != MG_MIXED_ON_COEFFICIENT)) {
        set_last_error("mg_mixed_solve: unknown bits above the count (MG_MIXED_OPERATOR(MG_MIXED_ON_COEFFICIENT) and MG_MIXED_INNER_PCG are the only ones)");
        return MG_ERR_BAD_ARG;
    }
    if (inner_pcg && mx_op != MG_MIXED_ON_COEFFICIENT) { set_last_error("mg_mixed_solve: MG_MIXED_INNER_PCG needs MG_MIXED_ON_COEFFICIENT"); return MG_ERR_BAD_ARG; }
    if (inner_cycles < 1) { set_last_error("mg_mixed_solve: the count (bits 0 .. 15) must be at least 1"); return MG_ERR_BAD_ARG; }
    if (maxit < 0) { set_last_error("mg_mixed_solve: negative maxit"); return MG_ERR_BAD_ARG; }
    if (!mx_has_b_ || !mx_has_u_) {
        set_last_error("mg_mixed_solve: call mg_mixed_set_rhs and mg_mixed_set_solution first");
        return MG_ERR_BAD_ARG;
    }
    if (mx_op == MG_MIXED_ON_COEFFICIENT) {
        MG_TRY(fam_check<VcFam>("mg_mixed_solve", FAM_NEED_CYCLE));   // a coefficient, V / W / F, Jacobi or red-black
        return mixed_solve_vc(tol, maxit, inner_cycles, inner_pcg, hist, hist_cap, n_hist, st);
    }
    Level &L0 = lv_[0];
    const Geom &g32 = L0.g;
    const double *const b = mxptr(MXB);
    mg_mixed_stats out{0, 0, 0, 0, 0.0};
    int nh = 0;
    auto record = [&](double rel) { if (hist && nh < hist_cap) hist[nh] = rel; nh++; out.relres = rel; };
    auto fetch_sum = [&](double *v) -> int {   // the sum the last launch left in d_mx_sum_; synchronises
        MG_HIP(hipGetLastError());
        MG_TRY(fetch_scalars(SC_MX_SUM, d_mx_sum_));
        *v = h_scal_[SC_MX_SUM];
        return MG_OK;
    };

    // u = b on the Dirichlet nodes; b.b over all nodes, as mg_solve
    launch_cg_boundary_copy<double>(stream_, g64_, mxptr(MXU), b);
    int np = launch_mixed_sumsq(stream_, g64_, b, d_mx_part_);
    launch_reduce_final(stream_, d_mx_part_, np, d_mx_sum_);
    double bb = 0, rr = 0;
    MG_TRY(fetch_sum(&bb));
    double s = mixed_scale(bb);   // the scale RHS32(0) currently carries
    L0.rhs_halo_ok = false;
    np = launch_mixed_residual(stream_, g64_, g32, L0.coef, mxptr(MXU), b, ptr<float>(MG_ARR_RHS, 0), s, d_mx_part_);
    launch_reduce_final(stream_, d_mx_part_, np, d_mx_sum_);
    MG_TRY(fetch_sum(&rr));
    auto relres = [&](double v) { return v == 0.0 ? 0.0 : std::sqrt(v / bb); };
    record(relres(rr));
    if (!std::isfinite(rr) || !std::isfinite(out.relres)) {
        out.status = 2;
    } else if (rr == 0.0) {
        out.status = 0;   // nothing to do: u solves the system (b == 0 with u == 0 inside included)
    } else {
        for (int k = 0;; k++) {
            if (k > 0 && out.relres <= tol) { out.status = 0; break; }
            if (k == maxit) { out.status = 1; break; }
            MG_TRY(correction_cycles(inner_cycles));
            out.cycles += inner_cycles;
            const double s_next = mixed_scale(rr);   // from the PREVIOUS residual: known before the launch
            np = launch_mixed_correct_residual(stream_, g64_, g32, L0.coef, mxptr(MXU), ptr<float>(MG_ARR_U, 0), b, mxptr(MXU2),
                                               ptr<float>(MG_ARR_RHS, 0), s, s_next, d_mx_part_);
            launch_reduce_final(stream_, d_mx_part_, np, d_mx_sum_);
            double rr_new = 0;
            MG_TRY(fetch_sum(&rr_new));   // the one host synchronisation per correction: the stopping test
            record(relres(rr_new));
            if (!std::isfinite(rr_new) || !std::isfinite(out.relres)) { out.status = 2; break; }   // not taken: u64 stays the last iterate
            std::swap(mx_[MXU], mx_[MXU2]);
            out.outer = k + 1;
            rr = rr_new;
            s = s_next;
        }
    }
    if (n_hist) *n_hist = nh;
    if (st) *st = out;
    return MG_OK;
}

// The same loop on mg_vc_*'s operator (MG_MIXED_ON_COEFFICIENT; kernels: mg_vc_mixed.hip): the operator is the handle's as it
// stands at the call -- the fp32 level-0 coefficient read as fp64, shift_, vc_mask_, the form of mg_vc_set_form -- and nothing
// new is kept. The Dirichlet nodes are the mask's; in the singular case (every face Neumann, no shift) b64 is projected first
// with mg_vc_project's weights and stays projected, u64 is projected after the last correction, and relres is evaluated once
// more on the projected u64, so that it is the residual of what is returned. The inner solve from U32(0) = 0 is `count` vc
// cycles, or -- inner_pcg -- `count` iterations of mg_vc_pcg_solve's weighted flexible CG with tolerance 0 (a breakdown ends
// it early; the iterate it holds is the correction). One fused launch and one host synchronisation per correction, plus the
// CG's own in that mode.
int Solver::mixed_solve_vc(double tol, int maxit, int count, bool inner_pcg, double *hist, int hist_cap, int *n_hist, mg_mixed_stats *st)
{
    if (inner_pcg) MG_TRY(krylov_alloc());
    Level &L0 = lv_[0];
    const Geom &g32 = L0.g;
    const bool singular = vc_singular();
    double *const b = mxptr(MXB);
    mg_mixed_stats out{0, 0, 0, 0, 0.0};
    int nh = 0;
    auto record = [&](double rel) { if (hist && nh < hist_cap) hist[nh] = rel; nh++; out.relres = rel; };
    auto fetch_sum = [&](double *partials, int np, double *v) -> int {   // the fixed-order sum of the partials; synchronises
        launch_reduce_final(stream_, partials, np, d_mx_sum_);
        MG_HIP(hipGetLastError());
        MG_TRY(fetch_scalars(SC_MX_SUM, d_mx_sum_));
        *v = h_scal_[SC_MX_SUM];
        return MG_OK;
    };
    // e32 == nullptr: the residual of u64 alone; -> sum r^2
    auto residual = [&](const float *e32, double s_in, double s_out, double *v) -> int {
        L0.rhs_halo_ok = false;
        const int np = launch_vc_mixed(stream_, g64_, g32, L0.coef, shift_, vc_mask_, mxptr(MXU), e32, vcptr<float>(0), b, mxptr(MXU2),
                                       ptr<float>(MG_ARR_RHS, 0), s_in, s_out, d_partials_, o4_partials_cap_, vc_plain_);
        return fetch_sum(d_partials_, np, v);
    };

    if (singular) MG_TRY(bc_project_ptr_t<double>(vc_mask_, g64_, b, nullptr));
    if (vc_mask_) launch_bc_dirichlet_copy<double>(stream_, g64_, vc_mask_, mxptr(MXU), b);
    else launch_cg_boundary_copy<double>(stream_, g64_, mxptr(MXU), b);
    double bb = 0, rr = 0;
    MG_TRY(fetch_sum(d_mx_part_, launch_mixed_sumsq(stream_, g64_, b, d_mx_part_), &bb));
    double s = mixed_scale(bb);   // the scale RHS32(0) currently carries
    MG_TRY(residual(nullptr, 1.0, s, &rr));
    auto relres = [&](double v) { return v == 0.0 ? 0.0 : std::sqrt(v / bb); };
    record(relres(rr));
    if (!std::isfinite(rr) || !std::isfinite(out.relres)) {
        out.status = 2;
    } else if (rr == 0.0) {
        out.status = 0;   // nothing to do: u solves the system
    } else {
        for (int k = 0;; k++) {
            if (k > 0 && out.relres <= tol) { out.status = 0; break; }
            if (k == maxit) { out.status = 1; break; }
            MG_HIP(hipMemsetAsync(L0.base[MG_ARR_U], 0, L0.alloc_elems * esize(), stream_));
            if (inner_pcg) {
                mg_krylov_stats ks{0, 0, 0.0, 0.0};
                MG_TRY(vc_pcg_t<float>(0.0, count, nullptr, 0, nullptr, &ks));
                out.cycles += ks.iters;
            } else {
                for (int c = 0; c < count; c++) MG_TRY(fam_cycle_enqueue_t<VcFam<float>>());
                out.cycles += count;
            }
            const double s_next = mixed_scale(rr);   // from the PREVIOUS residual: known before the launch
            double rr_new = 0;
            MG_TRY(residual(ptr<float>(MG_ARR_U, 0), s, s_next, &rr_new));   // the one host synchronisation per correction
            record(relres(rr_new));
            if (!std::isfinite(rr_new) || !std::isfinite(out.relres)) { out.status = 2; break; }   // not taken: u64 stays the last iterate
            std::swap(mx_[MXU], mx_[MXU2]);
            out.outer = k + 1;
            rr = rr_new;
            s = s_next;
        }
    }
    if (singular && out.status != 2) {
        MG_TRY(bc_project_ptr_t<double>(vc_mask_, g64_, mxptr(MXU), nullptr));
        MG_TRY(residual(nullptr, 1.0, mixed_scale(rr), &rr));   // of the u64 returned
        out.relres = relres(rr);
    }
    if (n_hist) *n_hist = nh;
    if (st) *st = out;
    return MG_OK;
}

int Solver::mixed_kernel(int kernel, double scale_in, double scale_out, int arr_e32, int arr_r32, double *sumsq_r)
{
    MG_TRY(mixed_check("mg_mixed_kernel"));
    const int mx_op = kernel >= 0 ? (kernel >> 16) : 0;   // MG_MIXED_OPERATOR; any other bit above the kind fails the test below
    if (mx_op == MG_MIXED_ON_COEFFICIENT) kernel &= 0xffff;
    if (kernel != MG_MIXED_K_RESIDUAL && kernel != MG_MIXED_K_CORRECT_RESIDUAL) { set_last_error("mg_mixed_kernel: unknown kernel"); return MG_ERR_BAD_ARG; }
    const bool corr = kernel == MG_MIXED_K_CORRECT_RESIDUAL;
    if (!check_arr(arr_r32, 0, "mg_mixed_kernel") || (corr && !check_arr(arr_e32, 0, "mg_mixed_kernel"))) return MG_ERR_BAD_ARG;
    if (corr && arr_e32 == arr_r32) { set_last_error("mg_mixed_kernel: the arrays must be distinct"); return MG_ERR_BAD_ARG; }
    if (corr && !(scale_in != 0.0 && std::isfinite(scale_in))) { set_last_error("mg_mixed_kernel: scale_in must be finite and not zero"); return MG_ERR_BAD_ARG; }
    if (!mx_has_b_ || !mx_has_u_) {
        set_last_error("mg_mixed_kernel: call mg_mixed_set_rhs and mg_mixed_set_solution first");
        return MG_ERR_BAD_ARG;
    }
    Level &L0 = lv_[0];
    if (mx_op == MG_MIXED_ON_COEFFICIENT) MG_TRY(fam_check<VcFam>("mg_mixed_kernel", 0));   // a coefficient
    if (arr_r32 == MG_ARR_RHS) L0.rhs_halo_ok = false;
    int np = 0;
    double *part = d_mx_part_;
    if (mx_op == MG_MIXED_ON_COEFFICIENT) {   // mg_vc_*'s operator as it stands: coefficient, shift, mask, form (mg_vc_mixed.hip)
        part = d_partials_;
        np = launch_vc_mixed(stream_, g64_, L0.g, L0.coef, shift_, vc_mask_, mxptr(MXU), corr ? ptr<float>(arr_e32, 0) : (const float *)nullptr,
                             vcptr<float>(0), mxptr(MXB), mxptr(MXU2), ptr<float>(arr_r32, 0), scale_in, scale_out, d_partials_,
                             o4_partials_cap_, vc_plain_);
    } else if (corr)
        np = launch_mixed_correct_residual(stream_, g64_, L0.g, L0.coef, mxptr(MXU), ptr<float>(arr_e32, 0), mxptr(MXB), mxptr(MXU2),
                                           ptr<float>(arr_r32, 0), scale_in, scale_out, d_mx_part_);
    else
        np = launch_mixed_residual(stream_, g64_, L0.g, L0.coef, mxptr(MXU), mxptr(MXB), ptr<float>(arr_r32, 0), scale_out, d_mx_part_);
    launch_reduce_final(stream_, part, np, d_mx_sum_);
    MG_HIP(hipGetLastError());
    MG_TRY(fetch_scalars(SC_MX_SUM, d_mx_sum_));
    if (corr) std::swap(mx_[MXU], mx_[MXU2]);
    if (sumsq_r) *sumsq_r = h_scal_[SC_MX_SUM];
    return MG_OK;
}

// ---------------------------------------------------------------- fourth-order defect correction (mg_o4_solve)
// r = b - (sigma I + A4) u with the fourth-order operator of level 0 (mg_o4.hip), (sigma I + A2) e = r solved approximately by
// inner_cycles of the handle's own cycles, u += e: mixed_solve with another operator in place of another precision. The
// outer iterate u4 and the right-hand side b4 live beside the hierarchy, whose U(0) / RHS(0) hold e and r meanwhile.
int Solver::o4_check(const char *fn, unsigned refuse)
{
    MG_TRY(driver_begin(fn, refuse));
    const Geom &g = lv_[0].g;
    if (g.nx < 7 || g.ny < 7 || (g.dim == 3 && g.gnz < 7)) {
        set_last_error(std::string(fn) + ": the fourth-order operator needs n >= 7 on every axis of level 0");
        return MG_ERR_BAD_ARG;
    }
    return MG_OK;
}

template <typename T>
int Solver::o4_kernel_t(bool corr, int arr_u, int arr_e, int arr_b, int arr_unew, int arr_r, double *sumsq_r)
{
    Level &L0 = lv_[0];
    const double w[3] = {L0.coef[0] / 12.0, L0.coef[1] / 12.0, L0.coef[2] / 12.0};
    T *const r = arr_r >= 0 ? ptr<T>(arr_r, 0) : (T *)nullptr;
    if (arr_r == MG_ARR_RHS || (corr && arr_unew == MG_ARR_RHS)) L0.rhs_halo_ok = false;
    const int np = corr ? launch_o4_correct_residual<T>(stream_, L0.g, w, shift_, ptr<T>(arr_u, 0), ptr<T>(arr_e, 0), ptr<T>(arr_b, 0),
                                                        ptr<T>(arr_unew, 0), r, d_partials_, o4_partials_cap_)
                        : launch_o4_residual<T>(stream_, L0.g, w, shift_, ptr<T>(arr_u, 0), ptr<T>(arr_b, 0), r, d_partials_, o4_partials_cap_);
    launch_reduce_final(stream_, d_partials_, np, d_scal_ + SC_O4_SUM);
    MG_HIP(hipGetLastError());
    if (sumsq_r) {
        MG_TRY(fetch_scalars(SC_O4_SUM, d_scal_ + SC_O4_SUM));
        *sumsq_r = h_scal_[SC_O4_SUM];
    }
    return MG_OK;
}

int Solver::o4_residual(int arr_u, int arr_b, int arr_r, double *sumsq_r)
{
    MG_TRY(o4_check("mg_o4_residual", REFUSE_DIST));
    if (!check_arr(arr_u, 0, "mg_o4_residual") || !check_arr(arr_b, 0, "mg_o4_residual")) return MG_ERR_BAD_ARG;
    if (arr_r >= 0 && (!check_arr(arr_r, 0, "mg_o4_residual") || arr_r == arr_u || arr_r == arr_b)) {
        set_last_error("mg_o4_residual: bad output array");
        return MG_ERR_BAD_ARG;
    }
    return d_.dtype == MG_F64 ? o4_kernel_t<double>(false, arr_u, -1, arr_b, -1, arr_r, sumsq_r)
                              : o4_kernel_t<float>(false, arr_u, -1, arr_b, -1, arr_r, sumsq_r);
}

int Solver::o4_correct_residual(int arr_u, int arr_e, int arr_b, int arr_unew, int arr_r, double *sumsq_r)
{
    MG_TRY(o4_check("mg_o4_correct_residual", REFUSE_DIST));
    const int a[5] = {arr_u, arr_e, arr_b, arr_unew, arr_r};
    for (int i = 0; i < 5; i++) {
        if (!check_arr(a[i], 0, "mg_o4_correct_residual")) return MG_ERR_BAD_ARG;
        for (int j = 0; j < i; j++)
            if (a[i] == a[j]) { set_last_error("mg_o4_correct_residual: the five arrays must be distinct"); return MG_ERR_BAD_ARG; }
    }
    return d_.dtype == MG_F64 ? o4_kernel_t<double>(true, arr_u, arr_e, arr_b, arr_unew, arr_r, sumsq_r)
                              : o4_kernel_t<float>(true, arr_u, arr_e, arr_b, arr_unew, arr_r, sumsq_r);
}

template <typename T>
int Solver::o4_solve_t(double tol, int maxit, int inner_cycles, double *hist, int hist_cap, int *n_hist, mg_o4_stats *st)
{
    Level &L0 = lv_[0];
    const Geom &g = L0.g;
    const size_t nbytes = L0.alloc_elems * esize();
    const double w[3] = {L0.coef[0] / 12.0, L0.coef[1] / 12.0, L0.coef[2] / 12.0};
    auto op = [&](int k) { return reinterpret_cast<T *>(o4_[k]) + L0.gh * g.plane; };
    mg_o4_stats out{0, 0, 0, 0, 0.0};
    int nh = 0;
    auto record = [&](double rel) { if (hist && nh < hist_cap) hist[nh] = rel; nh++; out.relres = rel; };
    auto fetch_sum = [&](int np, double *v) -> int {   // the sum of the last launch's partials; synchronises
        launch_reduce_final(stream_, d_partials_, np, d_scal_ + SC_O4_SUM);
        MG_HIP(hipGetLastError());
        MG_TRY(fetch_scalars(SC_O4_SUM, d_scal_ + SC_O4_SUM));
        *v = h_scal_[SC_O4_SUM];
        return MG_OK;
    };

    // b4 = RHS(0), u4 = U(0) with b's values on the Dirichlet nodes; b.b over all nodes, as mg_solve
    double bb = 0, rr = 0;
    MG_TRY(sumsq(0, MG_ARR_RHS, &bb));
    MG_HIP(hipMemcpyAsync(o4_[O4B], L0.base[MG_ARR_RHS], nbytes, hipMemcpyDeviceToDevice, stream_));
    MG_HIP(hipMemcpyAsync(o4_[O4U], L0.base[MG_ARR_U], nbytes, hipMemcpyDeviceToDevice, stream_));
    launch_cg_boundary_copy<T>(stream_, g, op(O4U), op(O4B));
    L0.rhs_halo_ok = false;
    MG_TRY(fetch_sum(launch_o4_residual<T>(stream_, g, w, shift_, op(O4U), op(O4B), ptr<T>(MG_ARR_RHS, 0), d_partials_, o4_partials_cap_), &rr));
    auto relres = [&](double v) { return v == 0.0 ? 0.0 : std::sqrt(v / bb); };
    record(relres(rr));
    bool take_u = true;
    if (!std::isfinite(rr) || !std::isfinite(out.relres)) {
        out.status = 2;
        take_u = false;   // no iterate with a finite norm: U stays what the caller passed
    } else if (rr == 0.0) {
        out.status = 0;   // nothing to do: u solves the system (b == 0 with u == 0 inside included)
    } else {
        for (int k = 0;; k++) {
            if (k > 0 && out.relres <= tol) { out.status = 0; break; }
            if (k == maxit) { out.status = 1; break; }
            MG_TRY(correction_cycles(inner_cycles));
            out.cycles += inner_cycles;
            double rr_new = 0;   // the one host synchronisation per correction: the stopping test
            MG_TRY(fetch_sum(launch_o4_correct_residual<T>(stream_, g, w, shift_, op(O4U), ptr<T>(MG_ARR_U, 0), op(O4B), op(O4U2),
                                                           ptr<T>(MG_ARR_RHS, 0), d_partials_, o4_partials_cap_), &rr_new));
            record(relres(rr_new));
            if (!std::isfinite(rr_new) || !std::isfinite(out.relres)) { out.status = 2; break; }   // not taken: u4 stays the last iterate
            std::swap(o4_[O4U], o4_[O4U2]);
            out.outer = k + 1;
        }
    }
    if (take_u) MG_HIP(hipMemcpyAsync(L0.base[MG_ARR_U], o4_[O4U], nbytes, hipMemcpyDeviceToDevice, stream_));
    MG_HIP(hipMemcpyAsync(L0.base[MG_ARR_RHS], o4_[O4B], nbytes, hipMemcpyDeviceToDevice, stream_));
    MG_HIP(hipStreamSynchronize(stream_));
    if (n_hist) *n_hist = nh;
    if (st) *st = out;
    return MG_OK;
}

int Solver::o4_solve(double tol, int maxit, int inner_cycles, double *hist, int hist_cap, int *n_hist, mg_o4_stats *st)
{
    MG_TRY(o4_check("mg_o4_solve", REFUSE_DIST | REFUSE_STAGE_CB));
    if (inner_cycles < 1) { set_last_error("mg_o4_solve: inner_cycles must be at least 1"); return MG_ERR_BAD_ARG; }
    if (maxit < 0) { set_last_error("mg_o4_solve: negative maxit"); return MG_ERR_BAD_ARG; }
    for (auto &b : o4_)   // slot by slot: a call that failed half way leaves the rest to the next one
        if (!b) MG_TRY(alloc_zeroed(&b, lv_[0].alloc_elems * esize()));
    return d_.dtype == MG_F64 ? o4_solve_t<double>(tol, maxit, inner_cycles, hist, hist_cap, n_hist, st)
                              : o4_solve_t<float>(tol, maxit, inner_cycles, hist, hist_cap, n_hist, st);
}

// ---------------------------------------------------------------- diagonal shift (mg_set_shift)
// Every launch rebuilds its Coef from Level::coef (coef_of; mixed_solve hands L0.coef to its fp64 kernels), so the shifted
// operator needs nothing but the new diagonal -- and new line factors where the smoother is a zebra one, the only data
// derived from cd when the handle is created.
int Solver::set_shift(double sigma)
{
    if (!(sigma >= 0.0) || !std::isfinite(sigma)) { set_last_error("mg_set_shift: sigma must be finite and not negative"); return MG_ERR_BAD_ARG; }
    MG_TRY(driver_begin("mg_set_shift", REFUSE_DIST));
    if (sigma == shift_) return MG_OK;
    const bool zebra = is_zebra(d_.smoother);
    if (zebra) MG_HIP(hipStreamSynchronize(stream_));   // no queued sweep may read a half-written table
    for (auto &L : lv_) {
        L.coef[3] = L.cd0 + sigma;
        if (zebra && L.zebra) MG_TRY(zebra_tabulate(L));
    }
    shift_ = sigma;
    return MG_OK;
}

// ---------------------------------------------------------------- implicit heat-equation stepper (mg_heat_*)
// u_t = -A0 u + f by the theta scheme: per step one launch of mg_heat.hip builds the right-hand side from U (+ f) into
// RHS, then cycles_per_step outer iterations of mg_solve on (1/(theta dt) I + A0) u' = rhs, warm-started from u.
int Solver::heat_check(const char *fn, double dt, double theta)
{
    MG_TRY(driver_begin(fn, REFUSE_DIST));
    if (!(dt > 0.0) || !std::isfinite(dt)) { set_last_error(std::string(fn) + ": dt must be positive and finite"); return MG_ERR_BAD_ARG; }
    if (!(theta > 0.0 && theta <= 1.0)) { set_last_error(std::string(fn) + ": theta must be in (0, 1]"); return MG_ERR_BAD_ARG; }
    if (!std::isfinite(1.0 / (theta * dt)) || !std::isfinite(1.0 / dt)) {
        set_last_error(std::string(fn) + ": dt is too small: 1 / (theta dt) is not finite");
        return MG_ERR_BAD_ARG;
    }
    return MG_OK;
}

int Solver::heat_set_source(const void *host)
{
    MG_TRY(driver_begin("mg_heat_set_source", REFUSE_DIST));
    if (!host) { heat_has_f_ = false; return MG_OK; }
    const Level &L0 = lv_[0];
    if (!heat_f_) MG_TRY(alloc_zeroed(&heat_f_, L0.alloc_elems * esize()));
    MG_TRY(stage_copy(static_cast<char *>(heat_f_) + (size_t)L0.gh * (size_t)L0.g.plane * esize(), L0.g, esize(), const_cast<void *>(host), true));
    heat_has_f_ = true;
    return MG_OK;
}

int Solver::heat_set_source_device(const void *dense, int dense_dtype, hipStream_t caller)
{
    const char *fn = "mg_heat_set_source_device";
    MG_TRY(driver_begin(fn, REFUSE_DIST));
    if (!dense) {
        if (dense_dtype != MG_F64 && dense_dtype != MG_F32) { set_last_error(std::string(fn) + ": dtype must be MG_F64 or MG_F32"); return MG_ERR_BAD_ARG; }
        heat_has_f_ = false;
        return MG_OK;
    }
    const Level &L0 = lv_[0];
    if (!heat_f_) {
        MG_TRY(device_check(fn, dense, dense_dtype, L0.g));   // nothing is allocated for an array that is refused
        MG_TRY(alloc_zeroed(&heat_f_, L0.alloc_elems * esize()));
    }
    MG_TRY(device_copy(fn, static_cast<char *>(heat_f_) + (size_t)L0.gh * (size_t)L0.g.plane * esize(), L0.g, esize(),
                       const_cast<void *>(dense), dense_dtype, true, caller));
    heat_has_f_ = true;
    return MG_OK;
}

template <typename T>
int Solver::heat_rhs_t(double dt, double theta, int arr_u, int arr_dst)
{
    Level &L0 = lv_[0];
    const double coef0[4] = {L0.coef[0], L0.coef[1], L0.coef[2], L0.cd0};
    const T *f = heat_has_f_ ? reinterpret_cast<const T *>(heat_f_) + L0.gh * L0.g.plane : (const T *)nullptr;
    if (arr_dst == MG_ARR_RHS) L0.rhs_halo_ok = false;
    launch_heat_rhs<T>(stream_, L0.g, coef0, dt, theta, ptr<T>(arr_u, 0), f, ptr<T>(arr_dst, 0));
    MG_HIP(hipGetLastError());
    return MG_OK;
}

int Solver::heat_rhs(double dt, double theta, int arr_u, int arr_dst)
{
    MG_TRY(heat_check("mg_heat_rhs", dt, theta));
    if (!check_arr(arr_u, 0, "mg_heat_rhs") || !check_arr(arr_dst, 0, "mg_heat_rhs")) return MG_ERR_BAD_ARG;
    if (arr_u == arr_dst) { set_last_error("mg_heat_rhs: arr_dst must differ from arr_u"); return MG_ERR_BAD_ARG; }
    return d_.dtype == MG_F64 ? heat_rhs_t<double>(dt, theta, arr_u, arr_dst) : heat_rhs_t<float>(dt, theta, arr_u, arr_dst);
}

template <typename T>
int Solver::heat_step_t(double dt, double theta, int nsteps, int cycles_per_step)
{
    for (int n = 0; n < nsteps; n++) {
        MG_TRY(heat_rhs_t<T>(dt, theta, MG_ARR_U, MG_ARR_RHS));
        for (int c = 0; c < cycles_per_step; c++) MG_TRY(outer_iteration_enqueue());
    }
    MG_TRY(residual_t<T>(0, MG_ARR_U, MG_ARR_RHS, -1, true));
    return sumsq_t<T>(0, MG_ARR_RHS);
}

int Solver::heat_step(double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st)
{
    MG_TRY(heat_check("mg_heat_step", dt, theta));
    MG_TRY(driver_begin("mg_heat_step", REFUSE_STAGE_CB));   // a call of its own: a bad dt or theta is reported first
    if (nsteps < 1) { set_last_error("mg_heat_step: nsteps must be at least 1"); return MG_ERR_BAD_ARG; }
    if (cycles_per_step < 1) { set_last_error("mg_heat_step: cycles_per_step must be at least 1"); return MG_ERR_BAD_ARG; }
    MG_TRY(set_shift(1.0 / (theta * dt)));
    MG_TRY(d_.dtype == MG_F64 ? heat_step_t<double>(dt, theta, nsteps, cycles_per_step) : heat_step_t<float>(dt, theta, nsteps, cycles_per_step));
    // the one host synchronisation of the call: ||rhs - (sigma I + A0) u|| / ||rhs|| of the last step
    MG_TRY(fetch_scalars(SC_RR, d_scal_ + SC_RR, 2));   // SC_RR and SC_BB
    if (st) {
        st->steps = nsteps;
        st->cycles = nsteps * cycles_per_step;
        st->time = (double)nsteps * dt;
        st->relres = h_scal_[SC_RR] == 0.0 ? 0.0 : std::sqrt(h_scal_[SC_RR] / h_scal_[SC_BB]);
    }
    return MG_OK;
}

// ---------------------------------------------------------------- lowest eigenpairs by LOBPCG (mg_eig_*), DESIGN.md section 17
// The block: six families of eig_m_ level-0 arrays. The preconditioner takes a residual column (W family) as RHS and a free
// column of the AW family as z, by pointer; the families are tables of pointers, so a column "moves" by swapping entries.
int Solver::eig_resize(int m)
{
    if (!d_eig_part_) {
        const size_t npart = (size_t)EIG_MAX_LAUNCHES * 2 * EIG_GRAM_ROWS * EIG_GRAM_COLS * EIG_MAX_BLOCKS;
        const size_t nout = (size_t)EIG_MAX_LAUNCHES * 2 * EIG_GRAM_ROWS * EIG_GRAM_COLS;
        MG_HIP(hipMalloc((void **)&d_eig_part_, sizeof(double) * npart));
        MG_HIP(hipMalloc((void **)&d_eig_out_, sizeof(double) * nout));
        MG_HIP(hipMalloc((void **)&d_eig_coef_, sizeof(double) * EIG_HOST_DOUBLES));
        MG_HIP(hipHostMalloc((void **)&h_eig_, sizeof(double) * EIG_HOST_DOUBLES));
        bytes_ += sizeof(double) * (npart + nout + EIG_HOST_DOUBLES);
    }
    const size_t nbytes = lv_[0].alloc_elems * esize();
    for (int j = eig_m_; j < m; j++) {          // grow: new columns, X holding the default start vector
        for (int f = 0; f < EIG_FAMILIES; f++) MG_TRY(alloc_zeroed(&eig_[f][j], nbytes));
        char *x = reinterpret_cast<char *>(eig_[MG_EIG_X][j]) + (size_t)lv_[0].gh * (size_t)lv_[0].g.plane * esize();
        if (d_.dtype == MG_F64) launch_eig_fill<double>(stream_, lv_[0].g, reinterpret_cast<double *>(x), j);
        else launch_eig_fill<float>(stream_, lv_[0].g, reinterpret_cast<float *>(x), j);
        MG_HIP(hipGetLastError());
        eig_m_ = j + 1;
    }
    if (m < eig_m_) {                           // shrink: the columns beyond m go
        MG_HIP(hipStreamSynchronize(stream_));
        for (int j = m; j < eig_m_; j++)
            for (int f = 0; f < EIG_FAMILIES; f++) {
                MG_HIP(hipFree(eig_[f][j]));
                eig_[f][j] = nullptr;
                bytes_ -= nbytes;
            }
        eig_m_ = m;
    }
    return MG_OK;
}

template <typename T>
int Solver::eig_gram_t(int mode, int nw, int np, double *G, double *H)
{
    const Level &L0 = lv_[0];
    const Geom &g = L0.g;
    const Coef<T> c = coef_of<T>(L0);
    const EigOp<T> op = eig_op_t<T>();
    const int m = eig_m_;
    auto col = [&](int fam, int j) { return reinterpret_cast<T *>(eig_[fam][j]) + L0.gh * g.plane; };
    // S and AS in column order; `interior`: the column is read as 0 on Dirichlet nodes (what the apply is about to make of it)
    T *sp[3 * MG_EIG_MAX_BLOCK], *asp[3 * MG_EIG_MAX_BLOCK];
    bool interior[3 * MG_EIG_MAX_BLOCK], applied[3 * MG_EIG_MAX_BLOCK];
    int s = 0;
    for (int j = 0; j < m; j++, s++) { sp[s] = col(MG_EIG_X, j); asp[s] = col(MG_EIG_AX, j); interior[s] = applied[s] = mode == EIG_GRAM_X; }
    if (mode != EIG_GRAM_X) {
        for (int j = 0; j < nw; j++, s++) { sp[s] = col(MG_EIG_W, j); asp[s] = col(MG_EIG_AW, j); interior[s] = applied[s] = true; }
        for (int j = 0; j < np; j++, s++) { sp[s] = col(MG_EIG_P, j); asp[s] = col(MG_EIG_AP, j); interior[s] = applied[s] = false; }
    }
    // column blocks of at most EIG_GRAM_COLS columns of ONE family, each against the rows above and on the diagonal in chunks
    // of EIG_GRAM_ROWS; the first chunk of a block carries the apply
    struct Tile { int r0, na, c0, nb; } tiles[EIG_MAX_LAUNCHES];
    constexpr int TILE = 2 * EIG_GRAM_ROWS * EIG_GRAM_COLS;
    int nt = 0, nblocks = 0;
    const int fam_begin[4] = {0, m, m + (mode == EIG_GRAM_X ? 0 : nw), s};
    for (int f = 0; f < 3; f++) {
        if (f == 0 && mode == EIG_GRAM_ITER) continue;   // X^T X = I and X^T A X = diag(theta): the caller has filled them in
        for (int c0 = fam_begin[f]; c0 < fam_begin[f + 1]; c0 += EIG_GRAM_COLS) {
            const int nb = std::min(EIG_GRAM_COLS, fam_begin[f + 1] - c0);
            for (int r0 = 0; r0 < c0 + nb; r0 += EIG_GRAM_ROWS) {
                if (nt == EIG_MAX_LAUNCHES) { set_last_error("mg_eig: more Gram tiles than the partial-sum buffer holds"); return MG_ERR_HIP; }
                EigGramArgs<T> a{};
                a.na = std::min(EIG_GRAM_ROWS, c0 + nb - r0);
                a.nb = nb;
                for (int r = 0; r < a.na; r++) {
                    a.row[r] = sp[r0 + r];
                    if (interior[r0 + r]) a.row_interior |= 1u << r;
                }
                for (int j = 0; j < nb; j++) { a.col[j] = sp[c0 + j]; a.acol[j] = asp[c0 + j]; }
                // the kernel loads all EIG_GRAM_ROWS rows and EIG_GRAM_COLS columns without a branch: the unused ones repeat a used one
                for (int r = a.na; r < EIG_GRAM_ROWS; r++) a.row[r] = a.row[0];
                for (int j = nb; j < EIG_GRAM_COLS; j++) { a.col[j] = a.col[0]; a.acol[j] = a.acol[0]; }
                a.col_interior = interior[c0] ? 1 : 0;
                nblocks = launch_eig_gram<T>(stream_, g, c, op, a, applied[c0] && r0 == 0, d_eig_part_ + (size_t)nt * TILE * EIG_MAX_BLOCKS);
                tiles[nt++] = Tile{r0, a.na, c0, nb};
            }
        }
    }
    MG_HIP(hipGetLastError());
    if (nt == 0) return MG_OK;
    // every tile left TILE * nblocks partials at a stride of TILE * EIG_MAX_BLOCKS: one reduction launch per tile
    for (int t = 0; t < nt; t++)
        launch_eig_reduce(stream_, d_eig_part_ + (size_t)t * TILE * EIG_MAX_BLOCKS, nblocks, TILE, d_eig_out_ + (size_t)t * TILE);
    MG_HIP(hipGetLastError());
    MG_HIP(hipMemcpyAsync(h_eig_, d_eig_out_, sizeof(double) * (size_t)nt * TILE, hipMemcpyDeviceToHost, stream_));
    MG_HIP(hipStreamSynchronize(stream_));
    for (int t = 0; t < nt; t++)
        for (int r = 0; r < tiles[t].na; r++)
            for (int j = 0; j < tiles[t].nb; j++) {
                const int a = tiles[t].r0 + r, b = tiles[t].c0 + j;
                if (a > b) continue;
                G[a * s + b] = G[b * s + a] = h_eig_[t * TILE + r * EIG_GRAM_COLS + j];
                H[a * s + b] = H[b * s + a] = h_eig_[t * TILE + TILE / 2 + r * EIG_GRAM_COLS + j];
            }
    return MG_OK;
}

template <typename T>
int Solver::eig_combine_t(int nw, int np, const double *coef, const double *theta, double *sums)
{
    const Level &L0 = lv_[0];
    const Geom &g = L0.g;
    const int m = eig_m_, s = m + nw + np;
    auto col = [&](int fam, int j) { return reinterpret_cast<T *>(eig_[fam][j]) + L0.gh * g.plane; };
    EigCombineArgs<T> a{};
    a.m = m; a.nw = nw; a.np = np;
    const EigOp<T> op = eig_op_t<T>();
    a.mask = op.mask;
    a.weighted = op.kind != EIG_OP_CONSTANT && op.mask != 0;   // mask 0: every weight is 1
    int k = 0;
    for (int j = 0; j < m; j++, k++) { a.s[k] = col(MG_EIG_X, j); a.as[k] = col(MG_EIG_AX, j); }
    for (int j = 0; j < nw; j++, k++) { a.s[k] = col(MG_EIG_W, j); a.as[k] = col(MG_EIG_AW, j); }
    for (int j = 0; j < np; j++, k++) { a.s[k] = col(MG_EIG_P, j); a.as[k] = col(MG_EIG_AP, j); }
    for (int j = 0; j < m; j++) {
        a.x[j] = col(MG_EIG_X, j); a.ax[j] = col(MG_EIG_AX, j); a.r[j] = col(MG_EIG_W, j);
        a.p[j] = col(MG_EIG_P, j); a.ap[j] = col(MG_EIG_AP, j);
    }
    const int ncoef = s * m + (nw + np) * nw;   // <= 24 * 8 + 16 * 8
    for (int i = 0; i < ncoef; i++) h_eig_[i] = coef[i];
    for (int j = 0; j < m; j++) h_eig_[ncoef + j] = theta[j];
    MG_HIP(hipMemcpyAsync(d_eig_coef_, h_eig_, sizeof(double) * (size_t)(ncoef + m), hipMemcpyHostToDevice, stream_));
    const int nblocks = launch_eig_combine<T>(stream_, g, a, d_eig_coef_, d_eig_coef_ + ncoef, d_eig_part_);
    launch_eig_reduce(stream_, d_eig_part_, nblocks, m, d_eig_out_);
    MG_HIP(hipGetLastError());
    MG_HIP(hipMemcpyAsync(h_eig_ + ncoef + m, d_eig_out_, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, stream_));
    MG_HIP(hipStreamSynchronize(stream_));
    for (int j = 0; j < m; j++) sums[j] = h_eig_[ncoef + m + j];
    return MG_OK;
}

template <typename T>
int Solver::eig_t(int nev, double tol, int maxit, double *lambda, double *relres, double *hist, int hist_cap, int *n_hist,
                  mg_eig_stats *st)
{
    constexpr int SMAX = 3 * MG_EIG_MAX_BLOCK;
    const int m = eig_m_;
    mg_eig_stats out{0, 1, 0, 0, 0.0};
    double G[SMAX * SMAX], H[SMAX * SMAX], C[SMAX * MG_EIG_MAX_BLOCK + 2 * MG_EIG_MAX_BLOCK * MG_EIG_MAX_BLOCK];
    double theta[MG_EIG_MAX_BLOCK], sums[MG_EIG_MAX_BLOCK], rel[MG_EIG_MAX_BLOCK];
    int nh = 0;
    const int opk = eig_op_t<T>().kind;
    const Precond pre = opk == EIG_OP_COEFFICIENT ? PRE_VC : (opk == EIG_OP_FACES ? PRE_BC : PRE_CONSTANT);
    // Rayleigh-Ritz on X alone from a fresh A X (X need not be orthonormal): X, AX rotated, theta, R in the W family, rel
    auto ritz_x = [&]() -> int {
        MG_TRY(eig_gram_t<T>(EIG_GRAM_X, 0, 0, G, H));
        if (dense_rayleigh_ritz(m, m, G, H, DENSE_PIVOT_MIN, theta, C) != DENSE_OK) return 1;
        MG_TRY(eig_combine_t<T>(0, 0, C, theta, sums));
        for (int j = 0; j < m; j++) rel[j] = std::sqrt(sums[j]) / std::fabs(theta[j]);   // ||x_j|| = 1 (in the operator's inner product)
        return MG_OK;
    };
    auto all_finite = [&]() {
        for (int j = 0; j < m; j++)
            if (!std::isfinite(rel[j])) return false;
        return true;
    };
    int rc = ritz_x();
    if (rc < 0) return rc;
    bool whole = rc == 0 && all_finite();
    if (!whole) out.status = 2;
    int act_prev[MG_EIG_MAX_BLOCK], n_prev = 0;   // the columns P belongs to (P column k goes with X column act_prev[k])
    while (whole) {
        double worst = 0;
        for (int j = 0; j < nev; j++) worst = std::max(worst, rel[j]);
        if (hist && nh < hist_cap) hist[nh] = worst;
        nh++;
        if (worst <= tol) { out.status = 0; break; }
        if (out.iters == maxit) { out.status = 1; break; }
        int act[MG_EIG_MAX_BLOCK], nw = 0;
        for (int j = 0; j < m; j++)
            if (rel[j] > tol) act[nw++] = j;
        // P of the active columns, compacted to the front of its family; none when a column has no P
        int np = n_prev > 0 ? nw : 0;
        for (int k = 0; k < nw && np; k++) {
            int from = -1;
            for (int q = 0; q < n_prev; q++)
                if (act_prev[q] == act[k]) from = q;
            if (from < 0) { np = 0; break; }
            if (from != k) {   // from > k: act and act_prev both ascend
                std::swap(eig_[MG_EIG_P][k], eig_[MG_EIG_P][from]);
                std::swap(eig_[MG_EIG_AP][k], eig_[MG_EIG_AP][from]);
                std::swap(act_prev[k], act_prev[from]);
            }
        }
        // W_k = M R_{act[k]}: the residual column is the right-hand side, a free AW column takes the result; afterwards the
        // result is W column k and the buffer R_k lay in (a finished or locked column's: act[k] >= k) is the free AW column
        for (int k = 0; k < nw; k++) {
            void *z = eig_[MG_EIG_AW][k];
            MG_TRY(precondition(&z, eig_[MG_EIG_W][act[k]], pre));
            eig_[MG_EIG_AW][k] = eig_[MG_EIG_W][k];
            eig_[MG_EIG_W][k] = z;
            out.cycles++;
        }
        int status = DENSE_RANK;
        for (int attempt = 0; attempt < 2; attempt++) {
            const int s = m + nw + np;
            if (attempt == 0) {
                for (int i = 0; i < s * s; i++) G[i] = H[i] = 0.0;
                for (int j = 0; j < m; j++) { G[j * s + j] = 1.0; H[j * s + j] = theta[j]; }
                MG_TRY(eig_gram_t<T>(EIG_GRAM_ITER, nw, np, G, H));
            }
            status = dense_rayleigh_ritz(s, m, G, H, DENSE_PIVOT_MIN, theta, C);
            if (status == DENSE_OK || np == 0) break;
            // the basis with P is not safely positive definite: the same iteration without P (the leading block of G, H)
            const int s2 = m + nw;
            for (int i = 0; i < s2; i++)
                for (int j = 0; j < s2; j++) { G[i * s2 + j] = G[i * s + j]; H[i * s2 + j] = H[i * s + j]; }
            np = 0;
            out.restarts++;
        }
        if (status != DENSE_OK) { out.status = 2; whole = false; break; }
        {
            const int s = m + nw + np;
            double *Cp = C + s * m;   // P' = X' without its X part, for the active columns
            for (int r = 0; r < nw + np; r++)
                for (int k = 0; k < nw; k++) Cp[r * nw + k] = C[(m + r) * m + act[k]];
            MG_TRY(eig_combine_t<T>(nw, np, C, theta, sums));
        }
        for (int j = 0; j < m; j++) rel[j] = std::sqrt(sums[j]) / std::fabs(theta[j]);
        for (int k = 0; k < nw; k++) act_prev[k] = act[k];
        n_prev = nw;
        out.iters++;
        if (!all_finite()) { out.status = 2; whole = false; break; }
    }
    // what is returned: Ritz values and residuals of the returned block from a fresh A X
    rc = ritz_x();
    if (rc < 0) return rc;
    if (rc != 0 || !all_finite()) {
        out.status = 2;
        for (int j = 0; j < m; j++) theta[j] = rel[j] = std::nan("");
    }
    for (int j = 0; j < m; j++) { lambda[j] = theta[j]; relres[j] = rel[j]; }
    out.max_relres = 0;
    for (int j = 0; j < nev; j++) out.max_relres = rel[j] > out.max_relres || std::isnan(rel[j]) ? rel[j] : out.max_relres;
    if (n_hist) *n_hist = nh;
    if (st) *st = out;
    return MG_OK;
}

// The operator of mg_eig_*  comes with every call, OR-ed into mg_eig_solve's m and mg_eig_kernel's kernel
// (MG_EIG_OPERATOR); which kernels and which cycle that means is decided from the handle's state at that call, so the mask, the
// shift and the coefficient may change between two calls.
int Solver::eig_take_operator(const char *fn, int *m_or_kernel)
{
    const int v = *m_or_kernel, op = v >= 0 ? v >> 8 : 0;
    if (op != MG_EIG_ON_CONSTANT && op != MG_EIG_ON_FACES && op != MG_EIG_ON_COEFFICIENT) {
        set_last_error(std::string(fn) + ": the operator OR-ed in must be MG_EIG_OPERATOR of MG_EIG_ON_CONSTANT, MG_EIG_ON_FACES or MG_EIG_ON_COEFFICIENT");
        return MG_ERR_BAD_ARG;
    }
    if (v >= 0) *m_or_kernel = v & 0xff;
    eig_op_ = op;
    return MG_OK;
}

template <typename T>
EigOp<T> Solver::eig_op_t() const
{
    EigOp<T> op{};
    op.kind = EIG_OP_CONSTANT;
    if (eig_op_ == MG_EIG_ON_FACES && bc_mask_ != 0) {
        op.kind = EIG_OP_FACES;
        op.mask = bc_mask_;
    } else if (eig_op_ == MG_EIG_ON_COEFFICIENT) {
        const Level &L0 = lv_[0];
        op.kind = EIG_OP_COEFFICIENT;
        op.mask = vc_mask_;
        op.wx = (T)(-L0.coef[0] / 2.0); op.wy = (T)(-L0.coef[1] / 2.0); op.wz = (T)(-L0.coef[2] / 2.0);   // mg_vc.hip's vc_coef
        op.sigma = (T)shift_;
        op.a = vcptr<T>(0);
    }
    return op;
}

int Solver::eig_op_check(const char *fn, bool cycle)
{
    const unsigned need = cycle ? FAM_NEED_CYCLE : 0u;
    if (eig_op_ == MG_EIG_ON_COEFFICIENT) return fam_check<VcFam>(fn, need);
    if (eig_op_ == MG_EIG_ON_FACES && bc_mask_ != 0) return fam_check<BcFam>(fn, need);
    return MG_OK;
}

int Solver::eig_solve(int m, int nev, double tol, int maxit, double *lambda, double *relres, double *hist, int hist_cap,
                      int *n_hist, mg_eig_stats *st)
{
    MG_TRY(eig_take_operator("mg_eig_solve", &m));
    const Geom &g = lv_[0].g;
    const int mask = eig_op_ == MG_EIG_ON_COEFFICIENT ? vc_mask_ : (eig_op_ == MG_EIG_ON_FACES ? bc_mask_ : 0);
    // the unknowns of the mask: an axis loses a node per Dirichlet face
    auto axis = [&](int n, int lo, int hi) { return (long long)n - ((mask & lo) ? 0 : 1) - ((mask & hi) ? 0 : 1); };
    const long long unknowns = axis(g.nx, MG_FACE_XLO, MG_FACE_XHI) * axis(g.ny, MG_FACE_YLO, MG_FACE_YHI) *
                               (g.dim == 3 ? axis(g.gnz, MG_FACE_ZLO, MG_FACE_ZHI) : 1);
    if (m < 1 || m > MG_EIG_MAX_BLOCK || nev < 1 || nev > m || m > unknowns || !(tol > 0.0) || !std::isfinite(tol) || maxit < 0 ||
        !lambda || !relres) {
        set_last_error("mg_eig_solve: need 1 <= nev <= m <= min(MG_EIG_MAX_BLOCK, unknowns of the operator), a positive finite tol, "
                       "maxit >= 0 and lambda / relres arrays");
        return MG_ERR_BAD_ARG;
    }
    MG_TRY(driver_begin("mg_eig_solve", REFUSE_DIST | REFUSE_STAGE_CB));
    MG_TRY(eig_op_check("mg_eig_solve", true));
    if (mask == (d_.dim == 3 ? 63 : 15) && shift_ == 0.0) {
        set_last_error("mg_eig_solve: every face is Neumann and the shift is 0, so the operator has the eigenvalue 0 and relres divides "
                       "by it: set a positive shift (mg_set_shift) and subtract it from the eigenvalues");
        return MG_ERR_BAD_ARG;
    }
    MG_TRY(eig_resize(m));
    return d_.dtype == MG_F64 ? eig_t<double>(nev, tol, maxit, lambda, relres, hist, hist_cap, n_hist, st)
                              : eig_t<float>(nev, tol, maxit, lambda, relres, hist, hist_cap, n_hist, st);
}

int Solver::eig_check(const char *fn, int family, int j, bool may_grow)
{
    MG_TRY(driver_begin(fn, REFUSE_DIST));
    const int limit = may_grow && family == MG_EIG_X ? MG_EIG_MAX_BLOCK : eig_m_;
    if (family < 0 || family >= EIG_FAMILIES || j < 0 || j >= limit) {
        set_last_error(std::string(fn) + ": no such family / column (MG_EIG_X columns up to MG_EIG_MAX_BLOCK - 1 can be set, every "
                                         "other access lies inside the allocated block, see mg_eig_block)");
        return MG_ERR_BAD_ARG;
    }
    return MG_OK;
}

int Solver::eig_vector(int family, int j, void *host, bool to_handle)
{
    const char *fn = to_handle ? "mg_eig_set_vector" : "mg_eig_get_vector";
    MG_TRY(eig_check(fn, family, j, to_handle));
    if (!host) { set_last_error(std::string(fn) + ": null argument"); return MG_ERR_BAD_ARG; }
    if (j >= eig_m_) MG_TRY(eig_resize(j + 1));
    const Level &L0 = lv_[0];
    char *dev = reinterpret_cast<char *>(eig_[family][j]) + (size_t)L0.gh * (size_t)L0.g.plane * esize();
    return stage_copy(dev, L0.g, esize(), host, to_handle);
}

int Solver::eig_vector_device(int family, int j, void *dense, int dense_dtype, bool to_handle, hipStream_t caller)
{
    const char *fn = to_handle ? "mg_eig_set_vector_device" : "mg_eig_get_vector_device";
    MG_TRY(eig_check(fn, family, j, to_handle));
    const Level &L0 = lv_[0];
    MG_TRY(device_check(fn, dense, dense_dtype, L0.g));   // every refusal comes before the block grows
    if (j >= eig_m_) MG_TRY(eig_resize(j + 1));
    char *dev = reinterpret_cast<char *>(eig_[family][j]) + (size_t)L0.gh * (size_t)L0.g.plane * esize();
    return device_copy(fn, dev, L0.g, esize(), dense, dense_dtype, to_handle, caller);
}

int Solver::eig_kernel(int kernel, int nw, int np, const double *coef, const double *theta, double *G, double *H, double *sums)
{
    MG_TRY(driver_begin("mg_eig_kernel", REFUSE_DIST));
    MG_TRY(eig_take_operator("mg_eig_kernel", &kernel));
    const bool gram = kernel == MG_EIG_K_APPLY_GRAM;
    if ((!gram && kernel != MG_EIG_K_COMBINE) || eig_m_ == 0 || nw < 0 || nw > eig_m_ || (np != 0 && np != nw) ||
        (gram ? (!G || !H) : (!coef || !theta || !sums))) {
        set_last_error("mg_eig_kernel: unknown kernel, no block (mg_eig_block), nw outside [0, m], np not 0 or nw, or a null argument");
        return MG_ERR_BAD_ARG;
    }
    MG_TRY(eig_op_check("mg_eig_kernel", false));
    if (gram) return d_.dtype == MG_F64 ? eig_gram_t<double>(EIG_GRAM_FULL, nw, np, G, H) : eig_gram_t<float>(EIG_GRAM_FULL, nw, np, G, H);
    return d_.dtype == MG_F64 ? eig_combine_t<double>(nw, np, coef, theta, sums) : eig_combine_t<float>(nw, np, coef, theta, sums);
}

// ---------------------------------------------------------------- operator families (mg_vc_*, mg_bc_*, mg_fas_*), DESIGN.md sections 18 - 20
// Three operators that take the place of the handle's constant stencil in the smoother, the residual and the coarsest-grid
// solve. They share one driver skeleton, the fam_* templates below; a family is a policy F<T> that supplies exactly what
// differs: the four launches (with the family's plain flag), the precondition of the check, and what the cycle does on the
// way down to level l + 1 and back up. Everything goes launch by launch: no fused pairs, no LDS sub-cycle, no folded
// prolongation -- those kernels carry the constant stencil in registers.
//
// vc (section 18): L = sigma I - div(a grad .) with a nodal coefficient array per level (Level::vc_a; level l + 1 is the
// full-weighted level l). The kernels are in mg_vc.hip; the transfers are the handle's own. With a face mask (vc_mask_,
// section 22) the faces in it are zero-flux walls: the kernels mirror, and the restriction, the projection of the singular
// case and the Dirichlet copy are mg_bc.hip's with this mask. With mask 0 every launch is the one it was without it.
template <typename T>
struct Solver::VcFam {
    typedef T type;
    static int ready(Solver &s, const char *fn)
    {
        if (!s.vc_set_) { set_last_error(std::string(fn) + ": no coefficient set (call mg_vc_set_coefficient first)"); return MG_ERR_BAD_ARG; }
        return MG_OK;
    }
    static int residual(Solver &s, int l, const T *x, const T *b, T *r)
    {
        const Level &L = s.lv_[l];
        return launch_vc_residual<T>(s.stream_, L.g, L.coef, s.shift_, s.vc_mask_, FAS_LINEAR, (T)0, x, s.vcptr<T>(l), b, r, s.d_partials_, s.o4_partials_cap_, s.vc_plain_);
    }
    static void jacobi(Solver &s, int l, const T *x, const T *b, T *out)
    {
        const Level &L = s.lv_[l];
        launch_vc_jacobi<T>(s.stream_, L.g, L.coef, s.shift_, s.vc_mask_, FAS_LINEAR, (T)0, (T)s.d_.omega, x, s.vcptr<T>(l), b, out, s.vc_plain_);
    }
    static void rb_colour(Solver &s, int l, int colour, T *x, const T *b)
    {
        const Level &L = s.lv_[l];
        launch_vc_rb_colour<T>(s.stream_, L.g, L.coef, s.shift_, s.vc_mask_, FAS_LINEAR, (T)0, colour, x, s.vcptr<T>(l), b);
    }
    static void coarse(Solver &s, int l, T *x, T *tmp, const T *b)
    {
        const Level &L = s.lv_[l];
        launch_vc_coarse<T>(s.stream_, L.g, L.coef, s.shift_, s.vc_mask_, FAS_LINEAR, (T)0, (T)s.d_.omega, s.d_.smoother, x, tmp, b, s.vcptr<T>(l),
                            s.d_.coarse_maxit, s.d_.coarse_tol, s.d_.coarse_mode == MG_COARSE_FIXED ? 1 : 0, s.d_coarse_);
    }
    static void heat_rhs(Solver &s, double dt, double theta, const T *u, const T *f, T *out)
    {
        const Level &L = s.lv_[0];
        if (theta == 1.0 && s.vc_mask_) {   // the operator's value is multiplied by zero and the mask decides which nodes copy u:
            launch_bc_heat_rhs<T>(s.stream_, L.g, coef0_of<T>(L), s.vc_mask_, dt, theta, u, f, out, s.vc_plain_);   // mg_bc.hip's stencil-free form
            return;
        }
        if (theta == 1.0) {   // the operator's value is multiplied by zero: mg_heat.hip's stencil-free form, same Dirichlet nodes
            const double coef0[4] = {L.coef[0], L.coef[1], L.coef[2], L.cd0};
            launch_heat_rhs<T>(s.stream_, L.g, coef0, dt, theta, u, f, out);
            return;
        }
        launch_vc_heat_rhs<T>(s.stream_, L.g, L.coef, s.vc_mask_, FAS_LINEAR, (T)0, dt, theta, u, s.vcptr<T>(0), f, out, s.vc_plain_);
    }
    static int down(Solver &s, int l)
    {
        // injecting the residual at coarse nodes of a Neumann face makes the cycle diverge, as in section 19
        if (s.vc_mask_) MG_TRY(s.bc_restrict_t<T>(s.vc_mask_, l, s.d_.restriction, MG_ARR_TMP, MG_ARR_RHS));
        else MG_TRY(s.restrict_t<T>(l, s.d_.restriction, MG_ARR_TMP, MG_ARR_RHS));
        return s.zero_array(MG_ARR_U, l + 1);
    }
    static int up(Solver &s, int l) { return s.prolong_t<T>(l + 1, 1, MG_ARR_U, MG_ARR_U); }
    // mg_vc_solve: U = RHS on the Dirichlet nodes; all faces Neumann and no shift: RHS(0) is projected first, U(0) at the end
    static int solve_begin(Solver &s) { return s.vc_singular() ? s.bc_project_t<T>(s.vc_mask_, 0, MG_ARR_RHS, nullptr) : MG_OK; }
    static int solve_end(Solver &s) { return s.vc_singular() ? s.bc_project_t<T>(s.vc_mask_, 0, MG_ARR_U, nullptr) : MG_OK; }
    // mg_fmg on this operator: the mask of the interpolation, and RHS(l + 1) = R RHS(l) with the restriction down() uses
    static int mask(const Solver &s) { return s.vc_mask_; }
    static int restrict_rhs(Solver &s, int l)
    {
        return s.vc_mask_ ? s.bc_restrict_t<T>(s.vc_mask_, l, s.d_.restriction, MG_ARR_RHS, MG_ARR_RHS) : s.restrict_t<T>(l, s.d_.restriction, MG_ARR_RHS, MG_ARR_RHS);
    }
    static void dirichlet_copy(Solver &s)
    {
        T *const x = s.ptr<T>(MG_ARR_U, 0);
        const T *const b = s.ptr<T>(MG_ARR_RHS, 0);
        if (s.vc_mask_) launch_bc_dirichlet_copy<T>(s.stream_, s.lv_[0].g, s.vc_mask_, x, b);
        else launch_cg_boundary_copy<T>(s.stream_, s.lv_[0].g, x, b);
    }
};

// bc (section 19): the handle's constant operator with zero-flux walls on the faces of a mask (enum mg_face): nodes that lie
// only on Neumann faces are unknowns whose missing neighbours are mirror images. The kernels are in mg_bc.hip -- the
// restriction too, because injecting at coarse nodes of a Neumann face makes the cycle diverge; the prolongation is the
// handle's own. Nothing is allocated: the state is the mask.
template <typename T>
struct Solver::BcFam {
    typedef T type;
    static int ready(Solver &, const char *) { return MG_OK; }
    static int residual(Solver &s, int l, const T *x, const T *b, T *r)
    {
        const Level &L = s.lv_[l];
        return launch_bc_residual<T>(s.stream_, L.g, coef_of<T>(L), s.bc_mask_, x, b, r, s.d_partials_, s.o4_partials_cap_, s.bc_plain_);
    }
    static void jacobi(Solver &s, int l, const T *x, const T *b, T *out)
    {
        const Level &L = s.lv_[l];
        launch_bc_jacobi<T>(s.stream_, L.g, coef_of<T>(L), s.bc_mask_, (T)s.d_.omega, x, b, out, s.bc_plain_);
    }
    static void rb_colour(Solver &s, int l, int colour, T *x, const T *b)
    {
        const Level &L = s.lv_[l];
        launch_bc_rb_colour<T>(s.stream_, L.g, coef_of<T>(L), s.bc_mask_, colour, x, b);
    }
    static void coarse(Solver &s, int l, T *x, T *tmp, const T *b)
    {
        const Level &L = s.lv_[l];
        launch_bc_coarse<T>(s.stream_, L.g, coef_of<T>(L), s.bc_mask_, (T)s.d_.omega, s.d_.smoother, x, tmp, b, s.d_.coarse_maxit,
                            s.d_.coarse_tol, s.d_.coarse_mode == MG_COARSE_FIXED ? 1 : 0, s.d_coarse_);
    }
    static void heat_rhs(Solver &s, double dt, double theta, const T *u, const T *f, T *out)
    {
        const Level &L = s.lv_[0];   // the mask decides which nodes copy u, so theta == 1 has a form of its own in mg_bc.hip
        launch_bc_heat_rhs<T>(s.stream_, L.g, coef0_of<T>(L), s.bc_mask_, dt, theta, u, f, out, s.bc_plain_);
    }
    static int down(Solver &s, int l)
    {
        MG_TRY(s.bc_restrict_t<T>(s.bc_mask_, l, s.d_.restriction, MG_ARR_TMP, MG_ARR_RHS));
        return s.zero_array(MG_ARR_U, l + 1);
    }
    static int up(Solver &s, int l) { return s.prolong_t<T>(l + 1, 1, MG_ARR_U, MG_ARR_U); }
    // mg_bc_solve with all faces Neumann and no shift: the constants are the null space, RHS(0) is projected onto the range
    // first (it stays projected) and U(0) is projected at the end
    static int solve_begin(Solver &s) { return s.bc_singular() ? s.bc_project_t<T>(s.bc_mask_, 0, MG_ARR_RHS, nullptr) : MG_OK; }
    static int solve_end(Solver &s) { return s.bc_singular() ? s.bc_project_t<T>(s.bc_mask_, 0, MG_ARR_U, nullptr) : MG_OK; }
    static int mask(const Solver &s) { return s.bc_mask_; }
    static int restrict_rhs(Solver &s, int l) { return s.bc_restrict_t<T>(s.bc_mask_, l, s.d_.restriction, MG_ARR_RHS, MG_ARR_RHS); }
    static void dirichlet_copy(Solver &s)
    {
        launch_bc_dirichlet_copy<T>(s.stream_, s.lv_[0].g, s.bc_mask_, s.ptr<T>(MG_ARR_U, 0), s.ptr<T>(MG_ARR_RHS, 0));
    }
};

// fas (section 20): N(u) = (sigma I + A) u + gamma g(u) with the handle's constant operator, gamma the same on every level.
// All faces are Dirichlet unless the kind carries MG_FAS_ON_FACES (section 23): then the linear part is bc's operator with
// the handle's mg_bc_set_faces mask, read at call time (fas_mask()), and every launch below takes it; mask 0 is the
// mask-free launch. With MG_FAS_ON_COEFFICIENT (section 24, fas_coef_) the linear part is vc's operator instead: the launches
// are mg_vc.hip's with the reaction, the level's coefficient array, the shift and the mg_vc_set_faces mask, and ready() asks
// for a coefficient as VcFam's does. The cycle is the same recursion on the nonlinear problem itself: the coarse level starts from the
// INJECTED iterate (kept in E), its right-hand side is R r + N_c(injected iterate), and the correction is the difference to
// the kept copy. The kernels are in mg_fas.hip. Nothing is allocated: the state is the kind and gamma.
template <typename T>
struct Solver::FasFam {
    typedef T type;
    static int ready(Solver &s, const char *fn) { return s.fas_coef_ ? VcFam<T>::ready(s, fn) : MG_OK; }
    static int residual(Solver &s, int l, const T *x, const T *b, T *r)
    {
        const Level &L = s.lv_[l];
        if (s.fas_coef_)
            return launch_vc_residual<T>(s.stream_, L.g, L.coef, s.shift_, s.vc_mask_, s.fas_kind_, (T)s.fas_gamma_, x, s.vcptr<T>(l), b, r,
                                         s.d_partials_, s.o4_partials_cap_, s.fas_plain_);
        return launch_fas_residual<T>(s.stream_, L.g, coef_of<T>(L), s.fas_kind_, (T)s.fas_gamma_, s.fas_mask(), x, b, r, s.d_partials_,
                                      s.o4_partials_cap_, s.fas_plain_);
    }
    static void jacobi(Solver &s, int l, const T *x, const T *b, T *out)
    {
        const Level &L = s.lv_[l];
        if (s.fas_coef_) {
            launch_vc_jacobi<T>(s.stream_, L.g, L.coef, s.shift_, s.vc_mask_, s.fas_kind_, (T)s.fas_gamma_, (T)s.d_.omega, x, s.vcptr<T>(l), b, out,
                                s.fas_plain_);
            return;
        }
        launch_fas_jacobi<T>(s.stream_, L.g, coef_of<T>(L), s.fas_kind_, (T)s.fas_gamma_, s.fas_mask(), (T)s.d_.omega, x, b, out, s.fas_plain_);
    }
    static void rb_colour(Solver &s, int l, int colour, T *x, const T *b)
    {
        const Level &L = s.lv_[l];
        if (s.fas_coef_) {
            launch_vc_rb_colour<T>(s.stream_, L.g, L.coef, s.shift_, s.vc_mask_, s.fas_kind_, (T)s.fas_gamma_, colour, x, s.vcptr<T>(l), b);
            return;
        }
        launch_fas_rb_colour<T>(s.stream_, L.g, coef_of<T>(L), s.fas_kind_, (T)s.fas_gamma_, s.fas_mask(), colour, x, b);
    }
    static void coarse(Solver &s, int l, T *x, T *tmp, const T *b)
    {
        const Level &L = s.lv_[l];
        if (s.fas_coef_) {
            launch_vc_coarse<T>(s.stream_, L.g, L.coef, s.shift_, s.vc_mask_, s.fas_kind_, (T)s.fas_gamma_, (T)s.d_.omega, s.d_.smoother, x, tmp, b,
                                s.vcptr<T>(l), s.d_.coarse_maxit, s.d_.coarse_tol, s.d_.coarse_mode == MG_COARSE_FIXED ? 1 : 0, s.d_coarse_);
            return;
        }
        launch_fas_coarse<T>(s.stream_, L.g, coef_of<T>(L), s.fas_kind_, (T)s.fas_gamma_, s.fas_mask(), (T)s.d_.omega, s.d_.smoother, x, tmp, b,
                             s.d_.coarse_maxit, s.d_.coarse_tol, s.d_.coarse_mode == MG_COARSE_FIXED ? 1 : 0, s.d_coarse_);
    }
    static void heat_rhs(Solver &s, double dt, double theta, const T *u, const T *f, T *out)
    {
        const Level &L = s.lv_[0];
        if (theta == 1.0 && s.fas_mask()) {   // as VcFam::heat_rhs: the mask decides which nodes copy u, mg_bc.hip's stencil-free form
            launch_bc_heat_rhs<T>(s.stream_, L.g, coef0_of<T>(L), s.fas_mask(), dt, theta, u, f, out, s.fas_plain_);
            return;
        }
        if (theta == 1.0) {   // as VcFam::heat_rhs: the reaction is multiplied by zero too
            const double coef0[4] = {L.coef[0], L.coef[1], L.coef[2], L.cd0};
            launch_heat_rhs<T>(s.stream_, L.g, coef0, dt, theta, u, f, out);
            return;
        }
        if (s.fas_coef_) {
            launch_vc_heat_rhs<T>(s.stream_, L.g, L.coef, s.vc_mask_, s.fas_kind_, (T)s.fas_gamma_, dt, theta, u, s.vcptr<T>(0), f, out, s.fas_plain_);
            return;
        }
        launch_fas_heat_rhs<T>(s.stream_, L.g, coef0_of<T>(L), s.fas_kind_, (T)s.fas_gamma_, s.fas_mask(), dt, theta, u, f, out, s.fas_plain_);
    }
    static int down(Solver &s, int l) { return s.fas_coarse_rhs_t<T>(l); }   // U(l + 1) = E(l + 1) = the injected iterate, RHS(l + 1)
    static int up(Solver &s, int l) { return s.fas_correct_t<T>(l); }   // P writes face nodes already (mg_bc_cycle)
    // no projection: the nonlinear problem has no null space to take out (mg_fas_solve does none either)
    static int solve_begin(Solver &) { return MG_OK; }
    static int solve_end(Solver &) { return MG_OK; }
    // mg_fmg on this operator: f goes down by the weighting mg_fas_coarse_rhs gives the residual (mirrored by the mask, the
    // coarse Dirichlet nodes injected); no tau term -- these are the coarse problems
    static int mask(const Solver &s) { return s.fas_mask(); }
    static int restrict_rhs(Solver &s, int l) { return s.bc_restrict_t<T>(s.fas_mask(), l, s.d_.restriction, MG_ARR_RHS, MG_ARR_RHS); }
    static void dirichlet_copy(Solver &s)   // mg_fas_solve: U = RHS on the Dirichlet nodes
    {
        launch_bc_dirichlet_copy<T>(s.stream_, s.lv_[0].g, s.fas_mask(), s.ptr<T>(MG_ARR_U, 0), s.ptr<T>(MG_ARR_RHS, 0));
    }
};

template <template <typename> class F>
int Solver::fam_check(const char *fn, unsigned need)
{
    MG_TRY(driver_begin(fn, REFUSE_DIST | ((need & FAM_NEED_CYCLE) ? REFUSE_STAGE_CB : 0u)));
    MG_TRY(F<double>::ready(*this, fn));   // the precondition looks at handle state only: the same for either element type
    if ((need & FAM_NEED_CYCLE) && !is_vwf(d_.cycle)) {
        set_last_error(std::string(fn) + ": not on a sawtooth handle (the cycle must be MG_CYCLE_V, MG_CYCLE_W or MG_CYCLE_F)");
        return MG_ERR_BAD_ARG;
    }
    if ((need & (FAM_NEED_CYCLE | FAM_NEED_SMOOTHER)) && d_.smoother != MG_SMOOTH_JACOBI && d_.smoother != MG_SMOOTH_RBGS) {
        set_last_error(std::string(fn) + ": the handle's smoother must be MG_SMOOTH_JACOBI or MG_SMOOTH_RBGS");
        return MG_ERR_BAD_ARG;
    }
    return MG_OK;
}

int Solver::set_form(const char *fn, int form, bool *plain)
{
    if (form != 0 && form != 1) { set_last_error(std::string(fn) + ": form must be 0 (default) or 1 (the plain kernels everywhere)"); return MG_ERR_BAD_ARG; }
    *plain = form == 1;
    return MG_OK;
}

template <class F>
int Solver::fam_residual_t(int level, int ax, int ar, int arr_r, bool want_sum, int slot)
{
    typedef typename F::type T;
    Level &L = lv_[level];
    if (arr_r == MG_ARR_RHS) L.rhs_halo_ok = false;
    const int np = F::residual(*this, level, ptr<T>(ax, level), ptr<T>(ar, level), arr_r >= 0 ? ptr<T>(arr_r, level) : (T *)nullptr);
    if (want_sum) launch_reduce_final(stream_, d_partials_, np, d_scal_ + slot);
    MG_HIP(hipGetLastError());
    return MG_OK;
}

// residual -> reduce -> fetch -> value; synchronises
template <class F>
int Solver::fam_residual_sum_t(int level, int ax, int ar, int arr_r, double *sumsq_r)
{
    MG_TRY(fam_residual_t<F>(level, ax, ar, arr_r, true));
    MG_TRY(fetch_scalars(SC_FAM_SUM, d_scal_ + SC_FAM_SUM));
    *sumsq_r = h_scal_[SC_FAM_SUM];
    return MG_OK;
}

template <template <typename> class F>
int Solver::fam_residual(const char *fn, int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r)
{
    MG_TRY(fam_check<F>(fn, 0));
    if (!check_arr(arr_x, level, fn) || !check_arr(arr_rhs, level, fn)) return MG_ERR_BAD_ARG;
    if (arr_r >= 0 && (!check_arr(arr_r, level, fn) || arr_r == arr_x || arr_r == arr_rhs)) {
        set_last_error(std::string(fn) + ": bad output array");
        return MG_ERR_BAD_ARG;
    }
    if (!sumsq_r)   // the sum stays on the device: no synchronisation
        return d_.dtype == MG_F64 ? fam_residual_t<F<double>>(level, arr_x, arr_rhs, arr_r, true) : fam_residual_t<F<float>>(level, arr_x, arr_rhs, arr_r, true);
    return d_.dtype == MG_F64 ? fam_residual_sum_t<F<double>>(level, arr_x, arr_rhs, arr_r, sumsq_r)
                              : fam_residual_sum_t<F<float>>(level, arr_x, arr_rhs, arr_r, sumsq_r);
}

template <class F>
int Solver::fam_smooth_t(int level, int smoother, int sweeps, int ax, int ar)
{
    typedef typename F::type T;
    Level &L = lv_[level];
    if (ax == MG_ARR_RHS) L.rhs_halo_ok = false;
    for (int s = 0; s < sweeps; s++) {
        if (smoother == MG_SMOOTH_JACOBI) {   // out of place into TMP, then the two pointers are swapped (as smooth_t)
            F::jacobi(*this, level, ptr<T>(ax, level), ptr<T>(ar, level), ptr<T>(MG_ARR_TMP, level));
            std::swap(L.base[ax], L.base[MG_ARR_TMP]);
        } else {
            for (int colour = 0; colour < 2; colour++) F::rb_colour(*this, level, colour, ptr<T>(ax, level), ptr<T>(ar, level));
        }
    }
    MG_HIP(hipGetLastError());
    return MG_OK;
}

template <template <typename> class F>
int Solver::fam_smooth(const char *fn, int level, int smoother, int sweeps, int arr_x, int arr_rhs)
{
    MG_TRY(fam_check<F>(fn, 0));
    if (!check_arr(arr_x, level, fn) || !check_arr(arr_rhs, level, fn)) return MG_ERR_BAD_ARG;
    if (arr_x == MG_ARR_TMP || arr_rhs == MG_ARR_TMP || arr_x == arr_rhs || sweeps < 0 ||
        (smoother != MG_SMOOTH_JACOBI && smoother != MG_SMOOTH_RBGS)) {
        set_last_error(std::string(fn) + ": bad array / sweeps, or a smoother other than MG_SMOOTH_JACOBI / MG_SMOOTH_RBGS");
        return MG_ERR_BAD_ARG;
    }
    return d_.dtype == MG_F64 ? fam_smooth_t<F<double>>(level, smoother, sweeps, arr_x, arr_rhs)
                              : fam_smooth_t<F<float>>(level, smoother, sweeps, arr_x, arr_rhs);
}

template <class F>
int Solver::fam_coarse_t(int level, int ax, int ar)
{
    typedef typename F::type T;
    if (ax == MG_ARR_RHS) lv_[level].rhs_halo_ok = false;
    F::coarse(*this, level, ptr<T>(ax, level), ptr<T>(MG_ARR_TMP, level), ptr<T>(ar, level));
    MG_HIP(hipGetLastError());
    return MG_OK;
}

template <template <typename> class F>
int Solver::fam_coarse_solve(const char *fn, int level, int arr_x, int arr_rhs, mg_cycle_stats *st)
{
    MG_TRY(fam_check<F>(fn, FAM_NEED_SMOOTHER));
    if (!check_arr(arr_x, level, fn) || !check_arr(arr_rhs, level, fn)) return MG_ERR_BAD_ARG;
    if (arr_x == MG_ARR_TMP || arr_rhs == MG_ARR_TMP || arr_x == arr_rhs) { set_last_error(std::string(fn) + ": bad array"); return MG_ERR_BAD_ARG; }
    MG_TRY(d_.dtype == MG_F64 ? fam_coarse_t<F<double>>(level, arr_x, arr_rhs) : fam_coarse_t<F<float>>(level, arr_x, arr_rhs));
    return fetch_cycle_stats(st);
}

// cyc(l, kind) of mg_desc.h with the family's kernels, launch by launch
template <class F>
int Solver::fam_cycle_rec_t(int l, int kind)
{
    const int L = d_.levels;
    if (l == L - 1) {
        const long long pts = (long long)lv_[l].g.nx * lv_[l].g.ny * lv_[l].g.gnz;
        if (pts > 32768 && d_.coarse_mode == MG_COARSE_FIXED) {   // too big for one workgroup: chip-wide sweeps, as coarse_level_t
            MG_TRY(fam_smooth_t<F>(l, d_.smoother, d_.coarse_maxit, MG_ARR_U, MG_ARR_RHS));
            h_fixed_->iters = d_.coarse_maxit; h_fixed_->flag = 0;
            h_fixed_->relres = 0; h_fixed_->sumsq_rhs = 0; h_fixed_->sumsq_r = 0;   // not evaluated on this path
            MG_HIP(hipMemcpyAsync(d_coarse_, h_fixed_, sizeof(CoarseOut), hipMemcpyHostToDevice, stream_));
        } else {
            MG_TRY(fam_coarse_t<F>(l, MG_ARR_U, MG_ARR_RHS));
        }
        if (acc_stats_) { launch_coarse_accum(stream_, d_coarse_acc_, d_coarse_); MG_HIP(hipGetLastError()); }
        return MG_OK;
    }
    MG_TRY(fam_smooth_t<F>(l, d_.smoother, d_.nu_pre, MG_ARR_U, MG_ARR_RHS));
    MG_TRY(fam_residual_t<F>(l, MG_ARR_U, MG_ARR_RHS, MG_ARR_TMP, false));
    MG_TRY(F::down(*this, l));   // TMP(l) -> RHS(l + 1) and the start U(l + 1)
    MG_TRY(fam_cycle_rec_t<F>(l + 1, kind));
    if (l + 1 < L - 1 && kind == MG_CYCLE_W) MG_TRY(fam_cycle_rec_t<F>(l + 1, MG_CYCLE_W));   // continues from U(l + 1); RHS(l + 1) (fas: and E(l + 1)) unchanged
    if (l + 1 < L - 1 && kind == MG_CYCLE_F) MG_TRY(fam_cycle_rec_t<F>(l + 1, MG_CYCLE_V));
    MG_TRY(F::up(*this, l));
    return fam_smooth_t<F>(l, d_.smoother, d_.nu_post, MG_ARR_U, MG_ARR_RHS);
}

template <class F>
int Solver::fam_cycle_enqueue_t()
{
    if (d_.cycle == MG_CYCLE_V) return fam_cycle_rec_t<F>(0, MG_CYCLE_V);
    MG_TRY(stats_begin());   // W and F make several coarse solves: summed on the device, as cycle_from_t
    const int rc = fam_cycle_rec_t<F>(0, d_.cycle);
    acc_stats_ = false;
    MG_TRY(rc);
    return stats_end();
}

template <template <typename> class F>
int Solver::fam_cycle_enqueue() { return d_.dtype == MG_F64 ? fam_cycle_enqueue_t<F<double>>() : fam_cycle_enqueue_t<F<float>>(); }

template <template <typename> class F>
int Solver::fam_cycle(const char *fn, mg_cycle_stats *st)
{
    MG_TRY(fam_check<F>(fn, FAM_NEED_CYCLE));
    MG_TRY(fam_cycle_enqueue<F>());
    return fetch_cycle_stats(st);
}

// mg_solve's loop and history on the family's operator (vc, bc); desc.outer_pre_gs is ignored (the lexicographic sweep has
// no such form)
template <class F>
int Solver::fam_solve_t(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle)
{
    MG_TRY(F::solve_begin(*this));
    double nb = 0, rr = 0;
    MG_TRY(sumsq(0, MG_ARR_RHS, &nb));
    F::dirichlet_copy(*this);   // U = RHS on the Dirichlet nodes
    MG_HIP(hipGetLastError());
    int nh = 0;
    auto norm = [&]() -> int {
        MG_TRY(fam_residual_sum_t<F>(0, MG_ARR_U, MG_ARR_RHS, -1, &rr));
        if (hist && nh < hist_cap) hist[nh] = std::sqrt(rr / nb);
        nh++;
        return MG_OK;
    };
    MG_TRY(norm());
    for (int it = 0; it < maxit; it++) {
        MG_TRY(fam_cycle_enqueue_t<F>());
        MG_TRY(fetch_cycle_stats(per_cycle ? &per_cycle[it] : nullptr));
        MG_TRY(norm());
        if (std::sqrt(rr / nb) <= tol) break;
    }
    MG_TRY(F::solve_end(*this));
    if (n_hist) *n_hist = nh;
    return MG_OK;
}

template <template <typename> class F>
int Solver::fam_solve(const char *fn, double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle)
{
    MG_TRY(fam_check<F>(fn, FAM_NEED_CYCLE));
    if (maxit < 0) { set_last_error(std::string(fn) + ": negative maxit"); return MG_ERR_BAD_ARG; }
    return d_.dtype == MG_F64 ? fam_solve_t<F<double>>(tol, maxit, hist, hist_cap, n_hist, per_cycle)
                              : fam_solve_t<F<float>>(tol, maxit, hist, hist_cap, n_hist, per_cycle);
}

// ---------------------------------------------------------------- nested iteration on a family's operator (mg_fmg with MG_FMG_OPERATOR), DESIGN.md section 27
// fmg_t's pass with the family's launches: RHS goes down by the family's restriction, the coarsest level is solved as the
// cycle solves it, and per level U(l) = Pi_mask U(l + 1) (mg_fmg.hip with the family's mask: mirrored at the Neumann faces,
// RHS(l) on the mask's Dirichlet nodes) followed by count cycles started on level l. fam_cycle_rec_t started on level l only
// overwrites the levels below l, which the pass has finished with. In the singular case (linear families, every face Neumann,
// no shift) RHS(0) is projected first and U(0) last, as in fam_solve_t -- the projections are the only host synchronisations
// before the residual at the end.
template <class F>
int Solver::fam_fmg_t(int count, mg_fmg_stats *st)
{
    typedef typename F::type T;
    const int L = d_.levels, mask = F::mask(*this);
    MG_TRY(F::solve_begin(*this));
    for (int l = 0; l + 1 < L; l++) MG_TRY(F::restrict_rhs(*this, l));
    MG_TRY(zero_array(MG_ARR_U, L - 1));
    launch_bc_dirichlet_copy<T>(stream_, lv_[L - 1].g, mask, ptr<T>(MG_ARR_U, L - 1), ptr<T>(MG_ARR_RHS, L - 1));
    MG_HIP(hipGetLastError());
    MG_TRY(fam_cycle_rec_t<F>(L - 1, MG_CYCLE_V));   // the coarsest-grid solve: one workgroup or chip-wide sweeps, as in a cycle
    MG_HIP(hipMemcpyAsync(h_coarse_, d_coarse_, sizeof(CoarseOut), hipMemcpyDeviceToHost, stream_));   // of this first, true coarse solve
    for (int l = L - 2; l >= 0; l--) {
        launch_fmg_prolong<T>(stream_, lv_[l + 1].g, lv_[l].g, ptr<T>(MG_ARR_U, l + 1), ptr<T>(MG_ARR_U, l), ptr<T>(MG_ARR_RHS, l), mask);
        MG_HIP(hipGetLastError());
        for (int k = 0; k < count; k++) {
            if (d_.cycle == MG_CYCLE_V) { MG_TRY(fam_cycle_rec_t<F>(l, MG_CYCLE_V)); continue; }
            MG_TRY(stats_begin());   // W and F: as fam_cycle_enqueue_t
            const int rc = fam_cycle_rec_t<F>(l, d_.cycle);
            acc_stats_ = false;
            MG_TRY(rc);
            MG_TRY(stats_end());
        }
    }
    MG_TRY(F::solve_end(*this));
    double nb = 0, nr = 0;
    MG_TRY(sumsq(0, MG_ARR_RHS, &nb));
    MG_TRY(fam_residual_sum_t<F>(0, MG_ARR_U, MG_ARR_RHS, -1, &nr));   // synchronises: h_coarse_ is valid from here
    if (st) {
        st->levels = L;
        st->cycles_per_level = count;
        st->coarse_iters = h_coarse_->iters;
        st->coarse_flag = h_coarse_->flag;
        st->relres = std::sqrt(nr / nb);
    }
    return MG_OK;
}

template <template <typename> class F>
int Solver::fam_fmg(int count, mg_fmg_stats *st)
{
    MG_TRY(fam_check<F>("mg_fmg", FAM_NEED_CYCLE));
    if (count < 1) { set_last_error("mg_fmg: cycles_per_level (bits 0 .. 15) must be at least 1"); return MG_ERR_BAD_ARG; }
    return d_.dtype == MG_F64 ? fam_fmg_t<F<double>>(count, st) : fam_fmg_t<F<float>>(count, st);
}

template <template <typename> class F>
int Solver::fam_fmg_prolong(int coarse_level, int arr_src, int arr_dst, int arr_bnd)
{
    MG_TRY(fam_check<F>("mg_fmg_prolong", 0));   // single-GPU handles, and a coefficient where the family's mask goes with one
    return fmg_prolong_mask(F<double>::mask(*this), coarse_level, arr_src, arr_dst, arr_bnd);
}

// ---------------------------------------------------------------- implicit time steps on a family's operator (mg_*_heat_*), DESIGN.md section 21
// u_t = -N0(u) + f with N0 the family's operator WITHOUT the shift, f the source of mg_heat_set_source: mg_heat_step's loop
// with the family's right-hand side launch and the family's cycle on (1/(theta dt) I + N0) u' = rhs, warm-started from u.
template <class F>
int Solver::fam_heat_rhs_t(double dt, double theta, int arr_u, int arr_dst)
{
    typedef typename F::type T;
    Level &L0 = lv_[0];
    const T *f = heat_has_f_ ? reinterpret_cast<const T *>(heat_f_) + L0.gh * L0.g.plane : (const T *)nullptr;
    if (arr_dst == MG_ARR_RHS) L0.rhs_halo_ok = false;
    F::heat_rhs(*this, dt, theta, ptr<T>(arr_u, 0), f, ptr<T>(arr_dst, 0));
    MG_HIP(hipGetLastError());
    return MG_OK;
}

template <template <typename> class F>
int Solver::fam_heat_rhs(const char *fn, double dt, double theta, int arr_u, int arr_dst)
{
    MG_TRY(heat_check(fn, dt, theta));
    MG_TRY(fam_check<F>(fn, 0));
    if (!check_arr(arr_u, 0, fn) || !check_arr(arr_dst, 0, fn)) return MG_ERR_BAD_ARG;
    if (arr_u == arr_dst) { set_last_error(std::string(fn) + ": arr_dst must differ from arr_u"); return MG_ERR_BAD_ARG; }
    return d_.dtype == MG_F64 ? fam_heat_rhs_t<F<double>>(dt, theta, arr_u, arr_dst) : fam_heat_rhs_t<F<float>>(dt, theta, arr_u, arr_dst);
}

template <class F>
int Solver::fam_heat_step_t(double dt, double theta, int nsteps, int cycles_per_step)
{
    typedef typename F::type T;
    for (int n = 0; n < nsteps; n++) {
        MG_TRY(fam_heat_rhs_t<F>(dt, theta, MG_ARR_U, MG_ARR_RHS));
        for (int c = 0; c < cycles_per_step; c++) MG_TRY(fam_cycle_enqueue_t<F>());
    }
    MG_TRY(fam_residual_t<F>(0, MG_ARR_U, MG_ARR_RHS, -1, true, SC_RR));   // next to SC_BB: the two are fetched in one copy
    return sumsq_t<T>(0, MG_ARR_RHS);
}

template <template <typename> class F>
int Solver::fam_heat_step(const char *fn, double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st)
{
    MG_TRY(heat_check(fn, dt, theta));
    MG_TRY(fam_check<F>(fn, FAM_NEED_CYCLE));
    if (nsteps < 1) { set_last_error(std::string(fn) + ": nsteps must be at least 1"); return MG_ERR_BAD_ARG; }
    if (cycles_per_step < 1) { set_last_error(std::string(fn) + ": cycles_per_step must be at least 1"); return MG_ERR_BAD_ARG; }
    MG_TRY(set_shift(1.0 / (theta * dt)));
    MG_TRY(d_.dtype == MG_F64 ? fam_heat_step_t<F<double>>(dt, theta, nsteps, cycles_per_step)
                              : fam_heat_step_t<F<float>>(dt, theta, nsteps, cycles_per_step));
    // the one host synchronisation of the call: ||rhs - (sigma I + N0)(u)|| / ||rhs|| of the last step
    MG_TRY(fetch_scalars(SC_RR, d_scal_ + SC_RR, 2));   // SC_RR and SC_BB
    if (st) {
        st->steps = nsteps;
        st->cycles = nsteps * cycles_per_step;
        st->time = (double)nsteps * dt;
        st->relres = h_scal_[SC_RR] == 0.0 ? 0.0 : std::sqrt(h_scal_[SC_RR] / h_scal_[SC_BB]);
    }
    return MG_OK;
}

int Solver::vc_heat_rhs(double dt, double theta, int arr_u, int arr_dst) { return fam_heat_rhs<VcFam>("mg_vc_heat_rhs", dt, theta, arr_u, arr_dst); }
int Solver::bc_heat_rhs(double dt, double theta, int arr_u, int arr_dst) { return fam_heat_rhs<BcFam>("mg_bc_heat_rhs", dt, theta, arr_u, arr_dst); }
int Solver::fas_heat_rhs(double dt, double theta, int arr_u, int arr_dst) { return fam_heat_rhs<FasFam>("mg_fas_heat_rhs", dt, theta, arr_u, arr_dst); }
int Solver::vc_heat_step(double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st)
{
    return fam_heat_step<VcFam>("mg_vc_heat_step", dt, theta, nsteps, cycles_per_step, st);
}
int Solver::bc_heat_step(double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st)
{
    return fam_heat_step<BcFam>("mg_bc_heat_step", dt, theta, nsteps, cycles_per_step, st);
}
int Solver::fas_heat_step(double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st)
{
    return fam_heat_step<FasFam>("mg_fas_heat_step", dt, theta, nsteps, cycles_per_step, st);
}

// ---------------------------------------------------------------- what only mg_vc_* has
int Solver::vc_alloc()
{
    for (auto &L : lv_)   // slot by slot: a call that failed half way leaves the rest to the next one
        if (!L.vc_a) MG_TRY(alloc_zeroed(&L.vc_a, L.alloc_elems * esize()));
    return MG_OK;
}

template <typename T>
int Solver::vc_restrict_all_t()
{
    for (int l = 0; l + 1 < d_.levels; l++) {
        if (vc_mask_) launch_bc_restrict_fw<T>(stream_, lv_[l].g, lv_[l + 1].g, vc_mask_, vcptr<T>(l), vcptr<T>(l + 1));   // keeps a_min <= a_c <= a_max
        else launch_restrict_fw<T>(stream_, lv_[l].g, lv_[l + 1].g, vcptr<T>(l), vcptr<T>(l + 1));
    }
    MG_HIP(hipGetLastError());
    return MG_OK;
}

int Solver::vc_set_coefficient(const void *host)
{
    MG_TRY(driver_begin("mg_vc_set_coefficient", REFUSE_DIST));
    if (!host) { set_last_error("mg_vc_set_coefficient: null array"); return MG_ERR_BAD_ARG; }
    const Geom &g = lv_[0].g;
    const size_t n = (size_t)g.nx * (size_t)g.ny * (size_t)g.nz;
    bool ok = true;
    if (d_.dtype == MG_F64) { const double *a = static_cast<const double *>(host); for (size_t i = 0; i < n && ok; i++) ok = a[i] > 0.0 && std::isfinite(a[i]); }
    else { const float *a = static_cast<const float *>(host); for (size_t i = 0; i < n && ok; i++) ok = a[i] > 0.0f && std::isfinite(a[i]); }
    if (!ok) { set_last_error("mg_vc_set_coefficient: every value must be finite and > 0"); return MG_ERR_BAD_ARG; }
    MG_TRY(vc_alloc());
    MG_TRY(stage_copy(reinterpret_cast<char *>(lv_[0].vc_a) + (size_t)lv_[0].gh * (size_t)g.plane * esize(), g, esize(),
                      const_cast<void *>(host), true));
    MG_TRY(d_.dtype == MG_F64 ? vc_restrict_all_t<double>() : vc_restrict_all_t<float>());
    vc_set_ = true;
    return MG_OK;
}

int Solver::vc_set_coefficient_device(const void *dense, int dense_dtype, hipStream_t caller)
{
    const char *fn = "mg_vc_set_coefficient_device";
    MG_TRY(driver_begin(fn, REFUSE_DIST));
    const Geom &g = lv_[0].g;
    MG_TRY(device_check(fn, dense, dense_dtype, g));   // nothing is allocated for an array that is refused
    MG_TRY(vc_alloc());
    MG_TRY(device_copy(fn, reinterpret_cast<char *>(lv_[0].vc_a) + (size_t)lv_[0].gh * (size_t)g.plane * esize(), g, esize(),
                       const_cast<void *>(dense), dense_dtype, true, caller));
    MG_TRY(d_.dtype == MG_F64 ? vc_restrict_all_t<double>() : vc_restrict_all_t<float>());
    vc_set_ = true;
    return MG_OK;
}

int Solver::vc_get_coefficient(int level, void *host)
{
    MG_TRY(fam_check<VcFam>("mg_vc_get_coefficient", 0));
    if (!host || level < 0 || level >= d_.levels) { set_last_error("mg_vc_get_coefficient: bad level / null array"); return MG_ERR_BAD_ARG; }
    const Level &L = lv_[level];
    return stage_copy(reinterpret_cast<char *>(L.vc_a) + (size_t)L.gh * (size_t)L.g.plane * esize(), L.g, esize(), host, false);
}

int Solver::vc_set_form(int form) { return set_form("mg_vc_set_form", form, &vc_plain_); }
int Solver::vc_residual(int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r) { return fam_residual<VcFam>("mg_vc_residual", level, arr_x, arr_rhs, arr_r, sumsq_r); }
int Solver::vc_smooth(int level, int smoother, int sweeps, int arr_x, int arr_rhs) { return fam_smooth<VcFam>("mg_vc_smooth", level, smoother, sweeps, arr_x, arr_rhs); }
int Solver::vc_coarse_solve(int level, int arr_x, int arr_rhs, mg_cycle_stats *st) { return fam_coarse_solve<VcFam>("mg_vc_coarse_solve", level, arr_x, arr_rhs, st); }
int Solver::vc_cycle(mg_cycle_stats *st) { return fam_cycle<VcFam>("mg_vc_cycle", st); }
int Solver::vc_solve(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle)
{
    return fam_solve<VcFam>("mg_vc_solve", tol, maxit, hist, hist_cap, n_hist, per_cycle);
}

// pcg_body_t with A -> L and M r = one vc cycle from zero; the sum of the residual goes through launch_reduce_final into
// the families' slot
template <typename T>
int Solver::vc_pcg_t(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_krylov_stats *st)
{
    const Level &L0 = lv_[0];
    auto residual_sum = [&](T *r, double *v) -> int {
        const int np = VcFam<T>::residual(*this, 0, ptr<T>(MG_ARR_U, 0), ptr<T>(MG_ARR_RHS, 0), r);
        launch_reduce_final(stream_, d_partials_, np, d_scal_ + SC_FAM_SUM);
        MG_HIP(hipGetLastError());
        MG_TRY(fetch_scalars(SC_FAM_SUM, d_scal_ + SC_FAM_SUM));
        *v = h_scal_[SC_FAM_SUM];
        return MG_OK;
    };
    auto direction_apply = [&](const T *z, const T *p, T *pn, T *q) {
        return launch_vc_cg_direction<T>(stream_, L0.g, L0.coef, shift_, vc_mask_, z, p, vcptr<T>(0), pn, q, d_cg_, d_cg_part_);
    };
    return pcg_body_t<T>(true, residual_sum, direction_apply, tol, maxit, hist, hist_cap, n_hist, st, vc_mask_, vc_mask_ != 0 && vc_singular());
}

// the direction kernel alone on level-0 arrays (mg_vc_direction): kernel-level checks and measurements, as mg_pcg_kernel
template <typename T>
int Solver::vc_direction_t(double beta, const int *a, double *pq)
{
    const Level &L0 = lv_[0];
    *h_cg_ = CgScalars{};
    h_cg_->alpha = h_cg_->beta = beta;
    MG_HIP(hipMemcpyAsync(d_cg_, h_cg_, sizeof(CgScalars), hipMemcpyHostToDevice, stream_));
    const int np = launch_vc_cg_direction<T>(stream_, L0.g, L0.coef, shift_, vc_mask_, ptr<T>(a[0], 0), ptr<T>(a[1], 0), vcptr<T>(0),
                                             ptr<T>(a[2], 0), ptr<T>(a[3], 0), d_cg_, d_cg_part_);
    launch_reduce_final(stream_, d_cg_part_, np, d_cg_dot_);
    MG_HIP(hipGetLastError());
    if (pq) {
        MG_TRY(fetch_scalars(SC_CG_DOT, d_cg_dot_, 1));
        *pq = h_scal_[SC_CG_DOT];
    }
    return MG_OK;
}

int Solver::vc_direction(double beta, int arr_z, int arr_p, int arr_pn, int arr_q, double *pq)
{
    MG_TRY(fam_check<VcFam>("mg_vc_direction", 0));
    const int a[4] = {arr_z, arr_p, arr_pn, arr_q};
    for (int i = 0; i < 4; i++) {
        if (!check_arr(a[i], 0, "mg_vc_direction")) return MG_ERR_BAD_ARG;
        for (int j = 0; j < i; j++)
            if (a[i] == a[j]) { set_last_error("mg_vc_direction: the arrays must be distinct"); return MG_ERR_BAD_ARG; }
    }
    if (arr_pn == MG_ARR_RHS || arr_q == MG_ARR_RHS) lv_[0].rhs_halo_ok = false;
    MG_TRY(krylov_scalars_alloc());
    return d_.dtype == MG_F64 ? vc_direction_t<double>(beta, a, pq) : vc_direction_t<float>(beta, a, pq);
}

int Solver::vc_pcg_solve(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_krylov_stats *st)
{
    MG_TRY(fam_check<VcFam>("mg_vc_pcg_solve", FAM_NEED_CYCLE));
    MG_TRY(krylov_alloc());
    return d_.dtype == MG_F64 ? vc_pcg_t<double>(tol, maxit, hist, hist_cap, n_hist, st)
                              : vc_pcg_t<float>(tol, maxit, hist, hist_cap, n_hist, st);
}

// Neumann faces of the variable-coefficient operator (section 22). The mask is handle state like bc_mask_ and independent of
// it; with a coefficient set, the coarse levels are restricted again from the stored level 0 with the new mask.
int Solver::face_mask_check(const char *fn, int mask)
{
    if (mask < 0 || mask > 63) { set_last_error(std::string(fn) + ": the mask must be a combination of the six MG_FACE_* bits"); return MG_ERR_BAD_ARG; }
    if (d_.dim == 2 && (mask & (MG_FACE_ZLO | MG_FACE_ZHI))) { set_last_error(std::string(fn) + ": a 2-D handle has no z faces"); return MG_ERR_BAD_ARG; }
    return MG_OK;
}

int Solver::vc_set_faces(int mask)
{
    MG_TRY(driver_begin("mg_vc_set_faces", REFUSE_DIST));
    MG_TRY(face_mask_check("mg_vc_set_faces", mask));
    if (mask == vc_mask_) return MG_OK;
    const int old = vc_mask_;
    vc_mask_ = mask;
    if (vc_set_) {
        int rc = d_.dtype == MG_F64 ? vc_restrict_all_t<double>() : vc_restrict_all_t<float>();
        if (rc != MG_OK) {   // back to the mask the call found, and the coarse coefficients that go with it
            vc_mask_ = old;
            (void)(d_.dtype == MG_F64 ? vc_restrict_all_t<double>() : vc_restrict_all_t<float>());
            return rc;
        }
    }
    return MG_OK;
}

int Solver::vc_get_faces(int *mask) const
{
    if (!mask) return MG_ERR_BAD_ARG;
    *mask = vc_mask_;
    return MG_OK;
}

int Solver::vc_restrict(int fine_level, int kind, int arr_src, int arr_dst)
{
    MG_TRY(driver_begin("mg_vc_restrict", REFUSE_DIST));   // a transfer: no coefficient is needed
    return fam_restrict("mg_vc_restrict", vc_mask_, fine_level, kind, arr_src, arr_dst);
}

int Solver::vc_project(int level, int arr, double *mean)
{
    MG_TRY(driver_begin("mg_vc_project", REFUSE_DIST));
    if (!check_arr(arr, level, "mg_vc_project")) return MG_ERR_BAD_ARG;
    return d_.dtype == MG_F64 ? bc_project_t<double>(vc_mask_, level, arr, mean) : bc_project_t<float>(vc_mask_, level, arr, mean);
}

// ---------------------------------------------------------------- what only mg_bc_* has
int Solver::bc_set_faces(int mask)
{
    MG_TRY(driver_begin("mg_bc_set_faces", REFUSE_DIST));
    MG_TRY(face_mask_check("mg_bc_set_faces", mask));
    bc_mask_ = mask;
    return MG_OK;
}

int Solver::bc_get_faces(int *mask) const
{
    if (!mask) return MG_ERR_BAD_ARG;
    *mask = bc_mask_;
    return MG_OK;
}

template <typename T>
int Solver::bc_restrict_t(int mask, int fl, int kind, int as, int ad)
{
    if (ad == MG_ARR_RHS) lv_[fl + 1].rhs_halo_ok = false;
    if (kind == MG_RESTRICT_FULLW)
        launch_bc_restrict_fw<T>(stream_, lv_[fl].g, lv_[fl + 1].g, mask, ptr<T>(as, fl), ptr<T>(ad, fl + 1));
    else
        launch_inject<T>(stream_, lv_[fl].g, lv_[fl + 1].g, ptr<T>(as, fl), ptr<T>(ad, fl + 1));
    MG_HIP(hipGetLastError());
    return MG_OK;
}

int Solver::fam_restrict(const char *fn, int mask, int fine_level, int kind, int arr_src, int arr_dst)
{
    if (fine_level < 0 || fine_level + 1 >= d_.levels || !check_arr(arr_src, fine_level, fn) ||
        !check_arr(arr_dst, fine_level + 1, fn) || (kind != MG_RESTRICT_INJECT && kind != MG_RESTRICT_FULLW)) {
        set_last_error(std::string(fn) + ": bad level / array / kind");
        return MG_ERR_BAD_ARG;
    }
    return d_.dtype == MG_F64 ? bc_restrict_t<double>(mask, fine_level, kind, arr_src, arr_dst)
                              : bc_restrict_t<float>(mask, fine_level, kind, arr_src, arr_dst);
}

int Solver::bc_restrict(int fine_level, int kind, int arr_src, int arr_dst)
{
    MG_TRY(fam_check<BcFam>("mg_bc_restrict", 0));
    return fam_restrict("mg_bc_restrict", bc_mask_, fine_level, kind, arr_src, arr_dst);
}

// c = (sum w v) / (sum w), v -= (T)c. sum w is the product over the axes of (nodes - half a node per Neumann face): exact in double.
template <typename T>
int Solver::bc_project_ptr_t(int mask, const Geom &g, T *v, double *mean)
{
    const int np = launch_bc_wsum<T>(stream_, g, mask, v, d_partials_, o4_partials_cap_);
    launch_reduce_final(stream_, d_partials_, np, d_scal_ + SC_FAM_SUM);
    MG_HIP(hipGetLastError());
    MG_TRY(fetch_scalars(SC_FAM_SUM, d_scal_ + SC_FAM_SUM));
    auto halves = [&](int lo, int hi) { return 0.5 * (((mask & lo) ? 1 : 0) + ((mask & hi) ? 1 : 0)); };
    double sw = ((double)g.nx - halves(MG_FACE_XLO, MG_FACE_XHI)) * ((double)g.ny - halves(MG_FACE_YLO, MG_FACE_YHI));
    if (g.dim == 3) sw *= (double)g.gnz - halves(MG_FACE_ZLO, MG_FACE_ZHI);
    const double c = h_scal_[SC_FAM_SUM] / sw;
    launch_bc_shift<T>(stream_, g, (T)c, v);
    MG_HIP(hipGetLastError());
    if (mean) *mean = c;
    return MG_OK;
}

template <typename T>
int Solver::bc_project_t(int mask, int level, int arr, double *mean)
{
    Level &L = lv_[level];
    if (arr == MG_ARR_RHS) L.rhs_halo_ok = false;
    return bc_project_ptr_t<T>(mask, L.g, ptr<T>(arr, level), mean);
}

int Solver::bc_project(int level, int arr, double *mean)
{
    MG_TRY(fam_check<BcFam>("mg_bc_project", 0));
    if (!check_arr(arr, level, "mg_bc_project")) return MG_ERR_BAD_ARG;
    return d_.dtype == MG_F64 ? bc_project_t<double>(bc_mask_, level, arr, mean) : bc_project_t<float>(bc_mask_, level, arr, mean);
}

int Solver::bc_set_form(int form) { return set_form("mg_bc_set_form", form, &bc_plain_); }
int Solver::bc_residual(int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r) { return fam_residual<BcFam>("mg_bc_residual", level, arr_x, arr_rhs, arr_r, sumsq_r); }
int Solver::bc_smooth(int level, int smoother, int sweeps, int arr_x, int arr_rhs) { return fam_smooth<BcFam>("mg_bc_smooth", level, smoother, sweeps, arr_x, arr_rhs); }
int Solver::bc_coarse_solve(int level, int arr_x, int arr_rhs, mg_cycle_stats *st) { return fam_coarse_solve<BcFam>("mg_bc_coarse_solve", level, arr_x, arr_rhs, st); }
int Solver::bc_cycle(mg_cycle_stats *st) { return fam_cycle<BcFam>("mg_bc_cycle", st); }
int Solver::bc_solve(double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle)
{
    return fam_solve<BcFam>("mg_bc_solve", tol, maxit, hist, hist_cap, n_hist, per_cycle);
}

// ---------------------------------------------------------------- what only mg_fas_* has
int Solver::fas_set_reaction(int kind, double gamma)
{
    MG_TRY(driver_begin("mg_fas_set_reaction", REFUSE_DIST));
    const int flags = MG_FAS_ON_FACES | MG_FAS_ON_COEFFICIENT;
    const int base = kind & ~flags;
    if ((base != MG_FAS_CUBIC && base != MG_FAS_EXP) || (kind & flags) == flags) {
        set_last_error("mg_fas_set_reaction: the kind must be MG_FAS_CUBIC or MG_FAS_EXP, alone or OR-ed with one of MG_FAS_ON_FACES and "
                       "MG_FAS_ON_COEFFICIENT");
        return MG_ERR_BAD_ARG;
    }
    if (!std::isfinite(gamma)) { set_last_error("mg_fas_set_reaction: gamma must be finite"); return MG_ERR_BAD_ARG; }
    fas_kind_ = base;
    fas_faces_ = (kind & MG_FAS_ON_FACES) != 0;
    fas_coef_ = (kind & MG_FAS_ON_COEFFICIENT) != 0;
    fas_gamma_ = gamma;
    return MG_OK;
}

int Solver::fas_get_reaction(int *kind, double *gamma) const
{
    if (kind) *kind = fas_kind_ | (fas_faces_ ? MG_FAS_ON_FACES : 0) | (fas_coef_ ? MG_FAS_ON_COEFFICIENT : 0);
    if (gamma) *gamma = fas_gamma_;
    return MG_OK;
}

// TMP(fl) holds the residual of level fl: U, E and RHS of level fl + 1 in one launch
template <typename T>
int Solver::fas_coarse_rhs_t(int fl)
{
    lv_[fl + 1].rhs_halo_ok = false;
    if (fas_coef_)
        launch_vc_fas_coarse_rhs<T>(stream_, lv_[fl].g, lv_[fl + 1].g, lv_[fl + 1].coef, shift_, vc_mask_, fas_kind_, (T)fas_gamma_,
                                    d_.restriction == MG_RESTRICT_INJECT, ptr<T>(MG_ARR_U, fl), ptr<T>(MG_ARR_TMP, fl), vcptr<T>(fl + 1),
                                    ptr<T>(MG_ARR_U, fl + 1), ptr<T>(MG_ARR_E, fl + 1), ptr<T>(MG_ARR_RHS, fl + 1));
    else
        launch_fas_coarse_rhs<T>(stream_, lv_[fl].g, lv_[fl + 1].g, coef_of<T>(lv_[fl + 1]), fas_kind_, (T)fas_gamma_, fas_mask(),
                                 d_.restriction == MG_RESTRICT_INJECT, ptr<T>(MG_ARR_U, fl), ptr<T>(MG_ARR_TMP, fl), ptr<T>(MG_ARR_U, fl + 1),
                                 ptr<T>(MG_ARR_E, fl + 1), ptr<T>(MG_ARR_RHS, fl + 1));
    MG_HIP(hipGetLastError());
    return MG_OK;
}

int Solver::fas_coarse_rhs(int fine_level)
{
    MG_TRY(fam_check<FasFam>("mg_fas_coarse_rhs", 0));
    if (fine_level < 0 || fine_level + 1 >= d_.levels) { set_last_error("mg_fas_coarse_rhs: bad level"); return MG_ERR_BAD_ARG; }
    return d_.dtype == MG_F64 ? fas_coarse_rhs_t<double>(fine_level) : fas_coarse_rhs_t<float>(fine_level);
}

// E(fl + 1) = U(fl + 1) - E(fl + 1), then U(fl) += P E(fl + 1): E(fl + 1) holds the coarse correction afterwards
template <typename T>
int Solver::fas_correct_t(int fl)
{
    launch_fas_diff<T>(stream_, lv_[fl + 1].g, ptr<T>(MG_ARR_U, fl + 1), ptr<T>(MG_ARR_E, fl + 1));
    MG_HIP(hipGetLastError());
    return prolong_t<T>(fl + 1, 1, MG_ARR_E, MG_ARR_U);
}

int Solver::fas_correct(int fine_level)
{
    MG_TRY(fam_check<FasFam>("mg_fas_correct", 0));
    if (fine_level < 0 || fine_level + 1 >= d_.levels) { set_last_error("mg_fas_correct: bad level"); return MG_ERR_BAD_ARG; }
    return d_.dtype == MG_F64 ? fas_correct_t<double>(fine_level) : fas_correct_t<float>(fine_level);
}

int Solver::fas_set_form(int form) { return set_form("mg_fas_set_form", form, &fas_plain_); }
int Solver::fas_residual(int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r) { return fam_residual<FasFam>("mg_fas_residual", level, arr_x, arr_rhs, arr_r, sumsq_r); }
int Solver::fas_smooth(int level, int smoother, int sweeps, int arr_x, int arr_rhs) { return fam_smooth<FasFam>("mg_fas_smooth", level, smoother, sweeps, arr_x, arr_rhs); }
int Solver::fas_coarse_solve(int level, int arr_x, int arr_rhs, mg_cycle_stats *st) { return fam_coarse_solve<FasFam>("mg_fas_coarse_solve", level, arr_x, arr_rhs, st); }
int Solver::fas_cycle(mg_cycle_stats *st) { return fam_cycle<FasFam>("mg_fas_cycle", st); }

// hist[k] = sqrt(sum r^2) after k cycles, ABSOLUTE (b = 0 is an ordinary nonlinear problem); one synchronisation per cycle
template <typename T>
int Solver::fas_solve_t(double rtol, double atol, int maxit, double *hist, int hist_cap, int *n_hist, mg_fas_stats *st)
{
    FasFam<T>::dirichlet_copy(*this);   // U = RHS on the Dirichlet nodes
    MG_HIP(hipGetLastError());
    int nh = 0, status = 1;
    double first = 0, last = 0;
    auto norm = [&]() -> int {
        double rr = 0;
        MG_TRY(fam_residual_sum_t<FasFam<T>>(0, MG_ARR_U, MG_ARR_RHS, -1, &rr));
        last = std::sqrt(rr);
        if (nh == 0) first = last;
        if (hist && nh < hist_cap) hist[nh] = last;
        nh++;
        return MG_OK;
    };
    // 0 converged, 2 not finite, -1 go on
    auto verdict = [&]() { return !std::isfinite(last) ? 2 : (last <= std::max(atol, rtol * first) ? 0 : -1); };
    MG_TRY(norm());
    int v = verdict();
    int it = 0;
    for (; v < 0 && it < maxit; it++) {
        MG_TRY(fam_cycle_enqueue_t<FasFam<T>>());
        MG_TRY(norm());
        v = verdict();
    }
    if (v >= 0) status = v;
    if (n_hist) *n_hist = nh;
    if (st) { st->status = status; st->cycles = it; st->norm0 = first; st->norm = last; }
    return MG_OK;
}

int Solver::fas_solve(double rtol, double atol, int maxit, double *hist, int hist_cap, int *n_hist, mg_fas_stats *st)
{
    MG_TRY(fam_check<FasFam>("mg_fas_solve", FAM_NEED_CYCLE));
    if (!(rtol >= 0) || !(atol >= 0) || !std::isfinite(rtol) || !std::isfinite(atol) || maxit < 0) {
        set_last_error("mg_fas_solve: the tolerances must be finite and >= 0, maxit >= 0");
        return MG_ERR_BAD_ARG;
    }
    return d_.dtype == MG_F64 ? fas_solve_t<double>(rtol, atol, maxit, hist, hist_cap, n_hist, st)
                              : fas_solve_t<float>(rtol, atol, maxit, hist, hist_cap, n_hist, st);
}

}  // namespace mg
