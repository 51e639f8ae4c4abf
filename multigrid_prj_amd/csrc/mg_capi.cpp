// mg_capi.cpp -- extern "C" entry points declared in include/mg_hip.h.
// No exception crosses this boundary; every failure becomes a negative mg_status
// plus a message kept per host thread (mg_last_error).
#include <cstring>
#include <new>
#include <string>

#include "mg_solver.h"

struct mg_solver {
    mg::Solver *impl;
};

namespace {
int bad(const char *msg)
{
    mg::set_last_error(msg);
    return MG_ERR_BAD_ARG;
}
template <typename F>
int guarded(F &&f)
{
    try {
        return f();
    } catch (const std::bad_alloc &) {
        mg::set_last_error("host allocation failed");
        return MG_ERR_HIP;
    } catch (const std::exception &e) {
        mg::set_last_error(e.what());
        return MG_ERR_HIP;
    } catch (...) {
        mg::set_last_error("unknown C++ exception");
        return MG_ERR_HIP;
    }
}
}  // namespace

extern "C" {

const char *mg_last_error(void) { return mg::last_error().c_str(); }

int mg_device_count(int *count)
{
    if (!count) return bad("mg_device_count: null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return MG_OK;
}

int mg_create(const mg_desc *desc, int device, mg_handle *out)
{
    return guarded([&]() -> int {
        if (!out) return bad("mg_create: null output handle");
        *out = nullptr;
        std::string why;
        int rc = mg::validate_desc(desc, &why);
        if (rc) { mg::set_last_error("mg_create: " + why); return rc; }
        mg::Solver *s = new mg::Solver(*desc, device);
        rc = s->init();
        if (rc) { delete s; return rc; }
        *out = new mg_solver{s};
        return MG_OK;
    });
}

int mg_destroy(mg_handle h)
{
    if (!h) return MG_OK;
    delete h->impl;
    delete h;
    return MG_OK;
}

#define MG_H(h) do { if (!(h) || !(h)->impl) return bad("null handle"); } while (0)

int mg_level_n(mg_handle h, int level, int *n)
{
    MG_H(h);
    if (!n || level < 0 || level >= h->impl->nlevels()) return bad("mg_level_n: bad argument");
    *n = h->impl->level(level).g.nx;
    return MG_OK;
}

int mg_level_nz(mg_handle h, int level, int *nz)
{
    MG_H(h);
    if (!nz || level < 0 || level >= h->impl->nlevels()) return bad("mg_level_nz: bad argument");
    *nz = h->impl->level(level).present ? h->impl->level(level).g.nz : 0;
    return MG_OK;
}

int mg_level_coefficients(mg_handle h, int level, double out[4])
{
    MG_H(h);
    if (!out || level < 0 || level >= h->impl->nlevels()) return bad("mg_level_coefficients: bad argument");
    std::memcpy(out, h->impl->level(level).coef, 4 * sizeof(double));
    return MG_OK;
}

int mg_set_rhs(mg_handle h, const void *b) { MG_H(h); return guarded([&] { return h->impl->set_array(MG_ARR_RHS, 0, b); }); }
int mg_set_solution(mg_handle h, const void *u) { MG_H(h); return guarded([&] { return h->impl->set_array(MG_ARR_U, 0, u); }); }
int mg_get_solution(mg_handle h, void *u) { MG_H(h); return guarded([&] { return h->impl->get_array(MG_ARR_U, 0, u); }); }
int mg_set_array(mg_handle h, int which, int level, const void *host) { MG_H(h); return guarded([&] { return h->impl->set_array(which, level, host); }); }
int mg_get_array(mg_handle h, int which, int level, void *host) { MG_H(h); return guarded([&] { return h->impl->get_array(which, level, host); }); }
int mg_set_array_device(mg_handle h, int which, int level, const void *dev, int dtype, void *stream)
{
    MG_H(h);
    return guarded([&] { return h->impl->array_device(which, level, const_cast<void *>(dev), dtype, true, static_cast<hipStream_t>(stream)); });
}
int mg_get_array_device(mg_handle h, int which, int level, void *dev, int dtype, void *stream)
{
    MG_H(h);
    return guarded([&] { return h->impl->array_device(which, level, dev, dtype, false, static_cast<hipStream_t>(stream)); });
}
int mg_zero_array(mg_handle h, int which, int level) { MG_H(h); return guarded([&] { return h->impl->zero_array(which, level); }); }

int mg_smooth(mg_handle h, int level, int smoother, int sweeps, int arr_x, int arr_rhs)
{
    MG_H(h);
    return guarded([&] { return h->impl->smooth(level, smoother, sweeps, arr_x, arr_rhs); });
}
int mg_residual(mg_handle h, int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r)
{
    MG_H(h);
    return guarded([&] { return h->impl->residual(level, arr_x, arr_rhs, arr_r, sumsq_r); });
}
int mg_sumsq(mg_handle h, int level, int arr, double *sumsq)
{
    MG_H(h);
    return guarded([&] { return h->impl->sumsq(level, arr, sumsq); });
}
int mg_restrict(mg_handle h, int fine_level, int kind, int arr_src, int arr_dst)
{
    MG_H(h);
    return guarded([&] { return h->impl->restrict_to(fine_level, kind, arr_src, arr_dst); });
}
int mg_prolong(mg_handle h, int coarse_level, int add, int arr_src, int arr_dst)
{
    MG_H(h);
    return guarded([&] { return h->impl->prolong(coarse_level, add, arr_src, arr_dst); });
}
int mg_correct(mg_handle h, int arr_u, int arr_e)
{
    MG_H(h);
    return guarded([&] { return h->impl->correct(arr_u, arr_e); });
}
int mg_coarse_solve(mg_handle h, int level, int arr_x, int arr_rhs, mg_cycle_stats *st)
{
    MG_H(h);
    return guarded([&] { return h->impl->coarse_solve(level, arr_x, arr_rhs, st); });
}
int mg_coarse_solve_ex(mg_handle h, int level, int arr_x, int arr_rhs, int smoother, int maxit,
                       double tol, int fixed, mg_cycle_stats *st)
{
    MG_H(h);
    return guarded([&] { return h->impl->coarse_solve_ex(level, arr_x, arr_rhs, smoother, maxit, tol, fixed, st); });
}
int mg_cycle(mg_handle h, mg_cycle_stats *st) { MG_H(h); return guarded([&] { return h->impl->cycle(st); }); }
int mg_cycle_async(mg_handle h, int count) { MG_H(h); return guarded([&] { return h->impl->cycle_async(count); }); }
int mg_solve(mg_handle h, double tol, int maxit, double *hist, int hist_cap, int *n_hist,
             mg_cycle_stats *per_cycle)
{
    MG_H(h);
    if (maxit < 0) return bad("mg_solve: negative maxit");
    return guarded([&] { return h->impl->solve(tol, maxit, hist, hist_cap, n_hist, per_cycle); });
}
int mg_solve_lockstep(mg_handle h, double tol, int maxit, const int *coarse_counts, int n_counts,
                      double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle)
{
    MG_H(h);
    if (maxit < 0 || n_counts < 0 || (n_counts > 0 && !coarse_counts)) return bad("mg_solve_lockstep: bad argument");
    for (int i = 0; i < n_counts; i++)
        if (coarse_counts[i] < 0) return bad("mg_solve_lockstep: negative sweep count");
    return guarded([&] { return h->impl->solve(tol, maxit, hist, hist_cap, n_hist, per_cycle, coarse_counts, n_counts); });
}
int mg_pcg_solve(mg_handle h, double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_krylov_stats *st)
{
    MG_H(h);
    if (maxit < 0) return bad("mg_pcg_solve: negative maxit");
    if (hist_cap < 0 || (hist_cap > 0 && !hist)) return bad("mg_pcg_solve: bad history buffer");
    return guarded([&] { return h->impl->pcg_solve(tol, maxit, hist, hist_cap, n_hist, st); });
}
int mg_pcg_kernel(mg_handle h, int kernel, double scalar, const int *arrs, double dots[2])
{
    MG_H(h);
    if (!arrs || !dots) return bad("mg_pcg_kernel: null argument");
    return guarded([&] { return h->impl->pcg_kernel(kernel, scalar, arrs, dots); });
}
int mg_fmg(mg_handle h, int cycles_per_level, mg_fmg_stats *st)
{
    MG_H(h);
    return guarded([&] { return h->impl->fmg(cycles_per_level, st); });
}
int mg_subcycle(mg_handle h, int level, int kind, int path, mg_cycle_stats *st)
{
    MG_H(h);
    return guarded([&] { return h->impl->subcycle(level, kind, path, st); });
}
int mg_subcycle_root(mg_handle h, int *root)
{
    MG_H(h);
    if (!root) return bad("mg_subcycle_root: null argument");
    *root = h->impl->subcycle_root();
    return MG_OK;
}
int mg_fmg_prolong(mg_handle h, int coarse_level, int arr_src, int arr_dst, int arr_bnd)
{
    MG_H(h);
    return guarded([&] { return h->impl->fmg_prolong(coarse_level, arr_src, arr_dst, arr_bnd); });
}
int mg_mixed_set_rhs(mg_handle h, const double *host_b)
{
    MG_H(h);
    if (!host_b) return bad("mg_mixed_set_rhs: null argument");
    return guarded([&] { return h->impl->mixed_set(true, host_b); });
}
int mg_mixed_set_solution(mg_handle h, const double *host_u)
{
    MG_H(h);
    if (!host_u) return bad("mg_mixed_set_solution: null argument");
    return guarded([&] { return h->impl->mixed_set(false, host_u); });
}
int mg_mixed_get_solution(mg_handle h, double *host_u)
{
    MG_H(h);
    if (!host_u) return bad("mg_mixed_get_solution: null argument");
    return guarded([&] { return h->impl->mixed_get_solution(host_u); });
}
int mg_mixed_set_rhs_device(mg_handle h, const void *dev_b, int dtype, void *stream)
{
    MG_H(h);
    return guarded([&] { return h->impl->mixed_set_device(true, dev_b, dtype, static_cast<hipStream_t>(stream)); });
}
int mg_mixed_set_solution_device(mg_handle h, const void *dev_u, int dtype, void *stream)
{
    MG_H(h);
    return guarded([&] { return h->impl->mixed_set_device(false, dev_u, dtype, static_cast<hipStream_t>(stream)); });
}
int mg_mixed_get_solution_device(mg_handle h, void *dev_u, int dtype, void *stream)
{
    MG_H(h);
    return guarded([&] { return h->impl->mixed_get_solution_device(dev_u, dtype, static_cast<hipStream_t>(stream)); });
}
int mg_mixed_solve(mg_handle h, double tol, int maxit, int inner_cycles, double *hist, int hist_cap, int *n_hist, mg_mixed_stats *st)
{
    MG_H(h);
    if (hist_cap < 0 || (hist_cap > 0 && !hist)) return bad("mg_mixed_solve: bad history buffer");
    return guarded([&] { return h->impl->mixed_solve(tol, maxit, inner_cycles, hist, hist_cap, n_hist, st); });
}
int mg_mixed_kernel(mg_handle h, int kernel, double scale_in, double scale_out, int arr_e32, int arr_r32, double *sumsq_r)
{
    MG_H(h);
    return guarded([&] { return h->impl->mixed_kernel(kernel, scale_in, scale_out, arr_e32, arr_r32, sumsq_r); });
}
int mg_o4_residual(mg_handle h, int arr_u, int arr_b, int arr_r, double *sumsq_r)
{
    MG_H(h);
    return guarded([&] { return h->impl->o4_residual(arr_u, arr_b, arr_r, sumsq_r); });
}
int mg_o4_correct_residual(mg_handle h, int arr_u, int arr_e, int arr_b, int arr_unew, int arr_r, double *sumsq_r)
{
    MG_H(h);
    return guarded([&] { return h->impl->o4_correct_residual(arr_u, arr_e, arr_b, arr_unew, arr_r, sumsq_r); });
}
int mg_o4_solve(mg_handle h, double tol, int maxit, int inner_cycles, double *hist, int hist_cap, int *n_hist, mg_o4_stats *st)
{
    MG_H(h);
    if (hist_cap < 0 || (hist_cap > 0 && !hist)) return bad("mg_o4_solve: bad history buffer");
    return guarded([&] { return h->impl->o4_solve(tol, maxit, inner_cycles, hist, hist_cap, n_hist, st); });
}
int mg_vc_set_coefficient(mg_handle h, const void *host_a) { MG_H(h); return guarded([&] { return h->impl->vc_set_coefficient(host_a); }); }
int mg_vc_set_coefficient_device(mg_handle h, const void *dev_a, int dtype, void *stream)
{
    MG_H(h);
    return guarded([&] { return h->impl->vc_set_coefficient_device(dev_a, dtype, static_cast<hipStream_t>(stream)); });
}
int mg_vc_get_coefficient(mg_handle h, int level, void *host_a) { MG_H(h); return guarded([&] { return h->impl->vc_get_coefficient(level, host_a); }); }
int mg_vc_set_form(mg_handle h, int form) { MG_H(h); return guarded([&] { return h->impl->vc_set_form(form); }); }
int mg_vc_residual(mg_handle h, int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r)
{
    MG_H(h);
    return guarded([&] { return h->impl->vc_residual(level, arr_x, arr_rhs, arr_r, sumsq_r); });
}
int mg_vc_smooth(mg_handle h, int level, int smoother, int sweeps, int arr_x, int arr_rhs)
{
    MG_H(h);
    return guarded([&] { return h->impl->vc_smooth(level, smoother, sweeps, arr_x, arr_rhs); });
}
int mg_vc_coarse_solve(mg_handle h, int level, int arr_x, int arr_rhs, mg_cycle_stats *st)
{
    MG_H(h);
    return guarded([&] { return h->impl->vc_coarse_solve(level, arr_x, arr_rhs, st); });
}
int mg_vc_cycle(mg_handle h, mg_cycle_stats *st) { MG_H(h); return guarded([&] { return h->impl->vc_cycle(st); }); }
int mg_vc_solve(mg_handle h, double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle)
{
    MG_H(h);
    if (hist_cap < 0 || (hist_cap > 0 && !hist)) return bad("mg_vc_solve: bad history buffer");
    return guarded([&] { return h->impl->vc_solve(tol, maxit, hist, hist_cap, n_hist, per_cycle); });
}
int mg_vc_pcg_solve(mg_handle h, double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_krylov_stats *st)
{
    MG_H(h);
    if (maxit < 0) return bad("mg_vc_pcg_solve: negative maxit");
    if (hist_cap < 0 || (hist_cap > 0 && !hist)) return bad("mg_vc_pcg_solve: bad history buffer");
    return guarded([&] { return h->impl->vc_pcg_solve(tol, maxit, hist, hist_cap, n_hist, st); });
}
int mg_vc_direction(mg_handle h, double beta, int arr_z, int arr_p, int arr_pn, int arr_q, double *pq)
{
    MG_H(h);
    return guarded([&] { return h->impl->vc_direction(beta, arr_z, arr_p, arr_pn, arr_q, pq); });
}
int mg_vc_set_faces(mg_handle h, int mask) { MG_H(h); return guarded([&] { return h->impl->vc_set_faces(mask); }); }
int mg_vc_get_faces(mg_handle h, int *mask)
{
    MG_H(h);
    if (!mask) return bad("mg_vc_get_faces: null output");
    return h->impl->vc_get_faces(mask);
}
int mg_vc_restrict(mg_handle h, int fine_level, int kind, int arr_src, int arr_dst)
{
    MG_H(h);
    return guarded([&] { return h->impl->vc_restrict(fine_level, kind, arr_src, arr_dst); });
}
int mg_vc_project(mg_handle h, int level, int arr, double *mean) { MG_H(h); return guarded([&] { return h->impl->vc_project(level, arr, mean); }); }
int mg_bc_set_faces(mg_handle h, int mask) { MG_H(h); return guarded([&] { return h->impl->bc_set_faces(mask); }); }
int mg_bc_get_faces(mg_handle h, int *mask)
{
    MG_H(h);
    if (!mask) return bad("mg_bc_get_faces: null output");
    return h->impl->bc_get_faces(mask);
}
int mg_bc_set_form(mg_handle h, int form) { MG_H(h); return guarded([&] { return h->impl->bc_set_form(form); }); }
int mg_bc_residual(mg_handle h, int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r)
{
    MG_H(h);
    return guarded([&] { return h->impl->bc_residual(level, arr_x, arr_rhs, arr_r, sumsq_r); });
}
int mg_bc_smooth(mg_handle h, int level, int smoother, int sweeps, int arr_x, int arr_rhs)
{
    MG_H(h);
    return guarded([&] { return h->impl->bc_smooth(level, smoother, sweeps, arr_x, arr_rhs); });
}
int mg_bc_restrict(mg_handle h, int fine_level, int kind, int arr_src, int arr_dst)
{
    MG_H(h);
    return guarded([&] { return h->impl->bc_restrict(fine_level, kind, arr_src, arr_dst); });
}
int mg_bc_coarse_solve(mg_handle h, int level, int arr_x, int arr_rhs, mg_cycle_stats *st)
{
    MG_H(h);
    return guarded([&] { return h->impl->bc_coarse_solve(level, arr_x, arr_rhs, st); });
}
int mg_bc_project(mg_handle h, int level, int arr, double *mean) { MG_H(h); return guarded([&] { return h->impl->bc_project(level, arr, mean); }); }
int mg_bc_cycle(mg_handle h, mg_cycle_stats *st) { MG_H(h); return guarded([&] { return h->impl->bc_cycle(st); }); }
int mg_bc_solve(mg_handle h, double tol, int maxit, double *hist, int hist_cap, int *n_hist, mg_cycle_stats *per_cycle)
{
    MG_H(h);
    if (hist_cap < 0 || (hist_cap > 0 && !hist)) return bad("mg_bc_solve: bad history buffer");
    return guarded([&] { return h->impl->bc_solve(tol, maxit, hist, hist_cap, n_hist, per_cycle); });
}
int mg_fas_set_reaction(mg_handle h, int kind, double gamma) { MG_H(h); return guarded([&] { return h->impl->fas_set_reaction(kind, gamma); }); }
int mg_fas_get_reaction(mg_handle h, int *kind, double *gamma) { MG_H(h); return h->impl->fas_get_reaction(kind, gamma); }
int mg_fas_set_form(mg_handle h, int form) { MG_H(h); return guarded([&] { return h->impl->fas_set_form(form); }); }
int mg_fas_residual(mg_handle h, int level, int arr_x, int arr_rhs, int arr_r, double *sumsq_r)
{
    MG_H(h);
    return guarded([&] { return h->impl->fas_residual(level, arr_x, arr_rhs, arr_r, sumsq_r); });
}
int mg_fas_smooth(mg_handle h, int level, int smoother, int sweeps, int arr_x, int arr_rhs)
{
    MG_H(h);
    return guarded([&] { return h->impl->fas_smooth(level, smoother, sweeps, arr_x, arr_rhs); });
}
int mg_fas_coarse_rhs(mg_handle h, int fine_level) { MG_H(h); return guarded([&] { return h->impl->fas_coarse_rhs(fine_level); }); }
int mg_fas_correct(mg_handle h, int fine_level) { MG_H(h); return guarded([&] { return h->impl->fas_correct(fine_level); }); }
int mg_fas_coarse_solve(mg_handle h, int level, int arr_x, int arr_rhs, mg_cycle_stats *st)
{
    MG_H(h);
    return guarded([&] { return h->impl->fas_coarse_solve(level, arr_x, arr_rhs, st); });
}
int mg_fas_cycle(mg_handle h, mg_cycle_stats *st) { MG_H(h); return guarded([&] { return h->impl->fas_cycle(st); }); }
int mg_fas_solve(mg_handle h, double rtol, double atol, int maxit, double *hist, int hist_cap, int *n_hist, mg_fas_stats *st)
{
    MG_H(h);
    if (hist_cap < 0 || (hist_cap > 0 && !hist)) return bad("mg_fas_solve: bad history buffer");
    return guarded([&] { return h->impl->fas_solve(rtol, atol, maxit, hist, hist_cap, n_hist, st); });
}
int mg_set_shift(mg_handle h, double sigma) { MG_H(h); return guarded([&] { return h->impl->set_shift(sigma); }); }
int mg_get_shift(mg_handle h, double *sigma)
{
    MG_H(h);
    if (!sigma) return bad("mg_get_shift: null argument");
    *sigma = h->impl->shift();
    return MG_OK;
}
int mg_heat_set_source(mg_handle h, const void *host_f) { MG_H(h); return guarded([&] { return h->impl->heat_set_source(host_f); }); }
int mg_heat_set_source_device(mg_handle h, const void *dev_f, int dtype, void *stream)
{
    MG_H(h);
    return guarded([&] { return h->impl->heat_set_source_device(dev_f, dtype, static_cast<hipStream_t>(stream)); });
}
int mg_heat_step(mg_handle h, double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st)
{
    MG_H(h);
    return guarded([&] { return h->impl->heat_step(dt, theta, nsteps, cycles_per_step, st); });
}
int mg_heat_rhs(mg_handle h, double dt, double theta, int arr_u, int arr_dst)
{
    MG_H(h);
    return guarded([&] { return h->impl->heat_rhs(dt, theta, arr_u, arr_dst); });
}
#define MG_FAM_HEAT(fam)                                                                                                         \
    int mg_##fam##_heat_rhs(mg_handle h, double dt, double theta, int arr_u, int arr_dst)                                        \
    {                                                                                                                            \
        MG_H(h);                                                                                                                 \
        return guarded([&] { return h->impl->fam##_heat_rhs(dt, theta, arr_u, arr_dst); });                                      \
    }                                                                                                                            \
    int mg_##fam##_heat_step(mg_handle h, double dt, double theta, int nsteps, int cycles_per_step, mg_heat_stats *st)           \
    {                                                                                                                            \
        MG_H(h);                                                                                                                 \
        return guarded([&] { return h->impl->fam##_heat_step(dt, theta, nsteps, cycles_per_step, st); });                        \
    }
MG_FAM_HEAT(vc)
MG_FAM_HEAT(bc)
MG_FAM_HEAT(fas)
#undef MG_FAM_HEAT
int mg_eig_solve(mg_handle h, int m, int nev, double tol, int maxit, double *lambda, double *relres, double *hist, int hist_cap,
                 int *n_hist, mg_eig_stats *st)
{
    MG_H(h);
    if (hist_cap < 0 || (hist_cap > 0 && !hist)) return bad("mg_eig_solve: bad history buffer");
    return guarded([&] { return h->impl->eig_solve(m, nev, tol, maxit, lambda, relres, hist, hist_cap, n_hist, st); });
}
int mg_eig_set_vector(mg_handle h, int family, int j, const void *host)
{
    MG_H(h);
    return guarded([&] { return h->impl->eig_vector(family, j, const_cast<void *>(host), true); });
}
int mg_eig_get_vector(mg_handle h, int family, int j, void *host)
{
    MG_H(h);
    return guarded([&] { return h->impl->eig_vector(family, j, host, false); });
}
int mg_eig_set_vector_device(mg_handle h, int family, int j, const void *dev, int dtype, void *stream)
{
    MG_H(h);
    return guarded([&] { return h->impl->eig_vector_device(family, j, const_cast<void *>(dev), dtype, true, static_cast<hipStream_t>(stream)); });
}
int mg_eig_get_vector_device(mg_handle h, int family, int j, void *dev, int dtype, void *stream)
{
    MG_H(h);
    return guarded([&] { return h->impl->eig_vector_device(family, j, dev, dtype, false, static_cast<hipStream_t>(stream)); });
}
int mg_eig_block(mg_handle h, int *m)
{
    MG_H(h);
    if (!m) return bad("mg_eig_block: null argument");
    *m = h->impl->eig_block();
    return MG_OK;
}
int mg_eig_kernel(mg_handle h, int kernel, int nw, int np, const double *coef, const double *theta, double *G, double *H, double *sums)
{
    MG_H(h);
    return guarded([&] { return h->impl->eig_kernel(kernel, nw, np, coef, theta, G, H, sums); });
}
int mg_set_stage_callback(mg_handle h, mg_stage_fn fn, void *user)
{
    MG_H(h);
    return guarded([&] { return h->impl->set_stage_callback(fn, user); });
}
int mg_sync(mg_handle h) { MG_H(h); return guarded([&] { return h->impl->sync(); }); }
int mg_timer_start(mg_handle h) { MG_H(h); return guarded([&] { return h->impl->timer_start(); }); }
int mg_timer_stop(mg_handle h, double *ms) { MG_H(h); return guarded([&] { return h->impl->timer_stop(ms); }); }
int mg_profile_begin(mg_handle h) { MG_H(h); return guarded([&] { return h->impl->profile_begin(); }); }
int mg_profile_end(mg_handle h, double *ms, int *sweeps) { MG_H(h); return guarded([&] { return h->impl->profile_end(ms, sweeps); }); }
int mg_profile_fused(mg_handle h, double *ms, int *sweeps) { MG_H(h); return guarded([&] { return h->impl->profile_fused(ms, sweeps); }); }
int mg_profile_get(mg_handle h, int kind, double *ms, int *launches)
{
    MG_H(h);
    if (kind < 0 || kind >= MG_PROF_KINDS) return bad("mg_profile_get: unknown kind");
    return guarded([&] { return h->impl->profile_get(kind, ms, launches); });
}
int mg_comm_info(mg_handle h, int *rank, int *nranks, int *transport_ranks, const char **transport)
{
    MG_H(h);
    return guarded([&] { return h->impl->comm_info(rank, nranks, transport_ranks, transport); });
}
int mg_comm_stats(mg_handle h, long long *groups, long long *bytes_sent)
{
    MG_H(h);
    if (groups) *groups = h->impl->comm_groups();
    if (bytes_sent) *bytes_sent = h->impl->comm_bytes_sent();
    return MG_OK;
}
int mg_device_bytes(mg_handle h, size_t *bytes)
{
    MG_H(h);
    if (!bytes) return bad("mg_device_bytes: null argument");
    *bytes = h->impl->device_bytes();
    return MG_OK;
}

int mg_debug_raw_layout(mg_handle h, int space, int index, int level, mg_debug_raw_info *out)
{
    if (!h || !h->impl) return bad("mg_debug_raw_layout: null handle");
    return guarded([&] { return h->impl->raw_layout("mg_debug_raw_layout", space, index, level, out); });
}
int mg_debug_raw_copy(mg_handle h, int space, int index, int level, void *host, size_t bytes, int to_device)
{
    if (!h || !h->impl) return bad("mg_debug_raw_copy: null handle");
    return guarded([&] { return h->impl->raw_copy(space, index, level, host, bytes, to_device != 0); });
}

int mg_plan_slab(const mg_desc *desc, int nranks, int rank, int level, int *z0, int *nz,
                 int *first_gathered_level)
{
    std::string why;
    int rc = mg::validate_desc(desc, &why);
    if (rc) { mg::set_last_error("mg_plan_slab: " + why); return rc; }
    mg::SlabPlan p;
    rc = mg::plan_slab(*desc, nranks, rank, level, &p, &why);
    if (rc) { mg::set_last_error("mg_plan_slab: " + why); return rc; }
    if (z0) *z0 = p.z0;
    if (nz) *nz = p.nz;
    if (first_gathered_level) *first_gathered_level = p.first_gathered_level;
    return MG_OK;
}

int mg_comm_unique_id(void *id128)
{
    if (!id128) return bad("mg_comm_unique_id: null argument");
    std::string why;
    int rc = mg::rccl_unique_id(id128, &why);
    if (rc) mg::set_last_error("mg_comm_unique_id: " + why);
    return rc;
}

int mg_comm_selftest(size_t bytes)
{
    return guarded([&]() -> int {
        char id[MG_COMM_ID_BYTES];
        std::string why;
        int rc = mg::rccl_unique_id(id, &why);
        if (rc) { mg::set_last_error("mg_comm_selftest: " + why); return rc; }
        mg::Comm *c = mg::make_rccl_comm(0, 1, id, &why);
        if (!c) { mg::set_last_error("mg_comm_selftest: " + why); return MG_ERR_COMM; }
        struct Guard { mg::Comm *c; ~Guard() { delete c; } } g{c};
        hipStream_t s;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return bad("stream");
        char *a = nullptr, *b = nullptr;
        double *d = nullptr;
        if (hipMalloc((void **)&a, bytes) != hipSuccess || hipMalloc((void **)&b, bytes) != hipSuccess ||
            hipMalloc((void **)&d, sizeof(double)) != hipSuccess) return bad("alloc");
        (void)hipMemsetAsync(a, 0x5a, bytes, s);
        (void)hipMemsetAsync(b, 0, bytes, s);
        double one = 1.25;
        (void)hipMemcpyAsync(d, &one, sizeof(double), hipMemcpyHostToDevice, s);
        mg::P2POp ops[2] = {{0, true, a, bytes}, {0, false, b, bytes}};
        rc = c->batch(ops, 2, s);
        if (!rc) rc = c->allreduce_sum(d, 1, s);
        std::string hb(bytes, 0);
        double out = 0;
        (void)hipMemcpyAsync(&hb[0], b, bytes, hipMemcpyDeviceToHost, s);
        (void)hipMemcpyAsync(&out, d, sizeof(double), hipMemcpyDeviceToHost, s);
        (void)hipStreamSynchronize(s);
        (void)hipFree(a); (void)hipFree(b); (void)hipFree(d); (void)hipStreamDestroy(s);
        if (rc) { mg::set_last_error("mg_comm_selftest: transport call failed"); return rc; }
        for (size_t i = 0; i < bytes; i++)
            if (hb[i] != 0x5a) { mg::set_last_error("mg_comm_selftest: payload mismatch"); return MG_ERR_COMM; }
        if (out != 1.25) { mg::set_last_error("mg_comm_selftest: all-reduce mismatch"); return MG_ERR_COMM; }
        return MG_OK;
    });
}

// the gathered tail of a slab-decomposed hierarchy would be visited repeatedly: a schedule the library does not have
static int dist_cycle_check(const mg_desc *desc, int nranks, const char *fn)
{
    if (nranks > 1 && (desc->cycle == MG_CYCLE_W || desc->cycle == MG_CYCLE_F)) {
        mg::set_last_error(std::string(fn) + ": MG_CYCLE_W / MG_CYCLE_F run on single-GPU handles only");
        return MG_ERR_INVALID_DESC;
    }
    return MG_OK;
}

static int create_with_comm(const mg_desc *desc, int device, int rank, int nranks, mg::Comm *comm, mg_handle *out)
{
    (void)rank; (void)nranks;
    mg::Solver *s = new mg::Solver(*desc, device, comm);  // owns comm
    int rc = s->init();
    if (rc) { delete s; return rc; }
    *out = new mg_solver{s};
    return MG_OK;
}

int mg_create_distributed(const mg_desc *desc, int device, int rank, int nranks, const void *id128,
                          mg_handle *out)
{
    return guarded([&]() -> int {
        if (!out) return bad("mg_create_distributed: null output handle");
        *out = nullptr;
        if (nranks == 1 && rank == 0) return mg_create(desc, device, out);
        std::string why;
        int rc = mg::validate_desc(desc, &why);
        if (rc) { mg::set_last_error("mg_create_distributed: " + why); return rc; }
        if ((rc = dist_cycle_check(desc, nranks, "mg_create_distributed"))) return rc;
        mg::SlabPlan p;
        rc = mg::plan_slab(*desc, nranks, rank, 0, &p, &why);
        if (rc) { mg::set_last_error("mg_create_distributed: " + why); return rc; }
        if (device >= 0 && hipSetDevice(device) != hipSuccess) return bad("mg_create_distributed: bad device");
        mg::Comm *c = mg::make_rccl_comm(rank, nranks, id128, &why);
        if (!c) { mg::set_last_error("mg_create_distributed: " + why); return MG_ERR_COMM; }
        return create_with_comm(desc, device, rank, nranks, c, out);
    });
}

int mg_create_distributed_hostcomm(const mg_desc *desc, int device, int rank, int nranks,
                                   const mg_host_comm *comm, mg_handle *out)
{
    return guarded([&]() -> int {
        if (!out || !comm) return bad("mg_create_distributed_hostcomm: null argument");
        *out = nullptr;
        std::string why;
        int rc = mg::validate_desc(desc, &why);
        if (rc) { mg::set_last_error("mg_create_distributed_hostcomm: " + why); return rc; }
        if ((rc = dist_cycle_check(desc, nranks, "mg_create_distributed_hostcomm"))) return rc;
        mg::SlabPlan p;
        rc = mg::plan_slab(*desc, nranks, rank, 0, &p, &why);
        if (rc) { mg::set_last_error("mg_create_distributed_hostcomm: " + why); return rc; }
        mg::Comm *c = mg::make_host_comm(rank, nranks, *comm, &why);
        if (!c) { mg::set_last_error("mg_create_distributed_hostcomm: " + why); return MG_ERR_COMM; }
        return create_with_comm(desc, device, rank, nranks, c, out);
    });
}

int mg_create_distributed_dryrun(const mg_desc *desc, int device, int rank, int nranks, mg_handle *out)
{
    return guarded([&]() -> int {
        if (!out) return bad("mg_create_distributed_dryrun: null output handle");
        *out = nullptr;
        std::string why;
        int rc = mg::validate_desc(desc, &why);
        if (rc) { mg::set_last_error("mg_create_distributed_dryrun: " + why); return rc; }
        if ((rc = dist_cycle_check(desc, nranks, "mg_create_distributed_dryrun"))) return rc;
        mg::SlabPlan p;
        rc = mg::plan_slab(*desc, nranks, rank, 0, &p, &why);
        if (rc) { mg::set_last_error("mg_create_distributed_dryrun: " + why); return rc; }
        return create_with_comm(desc, device, rank, nranks, mg::make_dry_comm(rank, nranks), out);
    });
}

}  // extern "C"
