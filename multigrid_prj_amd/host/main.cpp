// main.cpp -- the `Multigrid` executable: same command line, stdout protocol and result
// files (MGGS4.txt, x.mtx) as /root/reference/GeometricMultigrid/src/main.cpp, with the
// whole solve resident on the GPU (MultiGrid::DeviceSolve -> mg_solve in libmg_hip.so).
#include <chrono>
#include <cmath>
#include <iostream>

#include "multigrid_hip.hpp"
#include "utilities.hpp"

int main(int argc, char **argv)
{
    Utils::Options opt;
    Utils::parse_command_line(argc, argv, opt);
    std::function<double(const double, const double)> f, g;
    Utils::init_test_functions(f, g, opt.test);

    auto start = std::chrono::high_resolution_clock::now();

    mg_desc d;
    // -smt 2 ("BiCGSTAB") runs the Jacobi cycle in the reference too (main.cpp:103-106)
    const int smoother = opt.zebrax ? MG_SMOOTH_ZEBRA_X : opt.zebra ? MG_SMOOTH_ZEBRA_Y
                                   : opt.rbgs ? MG_SMOOTH_RBGS : (opt.smoother == Gauss_Siedel ? MG_SMOOTH_GS_LEX : MG_SMOOTH_JACOBI);
    mg_desc_reference_defaults(&d, static_cast<int>(opt.N), opt.level, opt.width, opt.alpha, smoother);
    d.dim = opt.dim;
    d.omega = opt.omega;
    if (opt.fp32) d.dtype = MG_F32;
    if (opt.vcycle) {
        d.cycle = opt.cycle_kind;   // MG_CYCLE_V / _W / _F
        d.nu_pre = opt.nu1;
        d.nu_post = opt.nu2 >= 0 ? opt.nu2 : 2;
        d.outer_pre_gs = 0;
    } else if (opt.nu2 >= 0) {
        d.nu_post = opt.nu2;
    }
    if (opt.full_weighting) d.restriction = MG_RESTRICT_FULLW;
    if (opt.coarse_fixed >= 0) { d.coarse_mode = MG_COARSE_FIXED; d.coarse_maxit = opt.coarse_fixed; }
    if (opt.dim == 3) d.outer_pre_gs = 0;
    d.aniso[0] = opt.aniso_x; d.aniso[1] = opt.aniso_y; d.aniso[2] = opt.eps_z;
    d.semi_xy = opt.semi;

    // right-hand side: g on the boundary, f inside (DataVector)
    std::vector<double> b;
    size_t n = opt.N, total = (opt.dim == 3) ? n * n * n : n * n;
    if (opt.dim == 2) {
        MultiGrid::SquareDomain fine(opt.N, opt.width, 0);
        MultiGrid::DataVector<double> fvec(fine, f, g);
        b.assign(fvec.data(), fvec.data() + fvec.size());
    } else {
        // 3-D extension: the 2-D (f, g) pair extruded along z, g on all six faces
        const double h = opt.width / static_cast<double>(n - 1);
        b.resize(total);
        for (size_t k = 0; k < n; k++)
            for (size_t j = 0; j < n; j++)
                for (size_t i = 0; i < n; i++) {
                    bool bnd = i == 0 || j == 0 || k == 0 || i == n - 1 || j == n - 1 || k == n - 1;
                    double x = i * h, y = opt.width - j * h;
                    b[(k * n + j) * n + i] = bnd ? g(x, y) : f(x, y);
                }
    }
    std::vector<double> u(total, 0.);

    // Device setup belongs to the initialization phase, like the reference's construction of
    // domains / matrices / operators (main.cpp:25-67): create the HBM-resident hierarchy,
    // upload b and u = 0, and run one throw-away cycle so the code object is loaded.
    mg_handle h = nullptr;
    std::vector<float> bf, uf;
    try {
        MultiGrid::mg_check(mg_create(&d, -1, &h));
        if (opt.fp32) {
            bf.assign(b.begin(), b.end());
            uf.assign(total, 0.f);
            MultiGrid::mg_check(mg_set_rhs(h, bf.data()));
            MultiGrid::mg_check(mg_set_solution(h, uf.data()));
        } else {
            MultiGrid::mg_check(mg_set_rhs(h, b.data()));
            MultiGrid::mg_check(mg_set_solution(h, u.data()));
        }
        // one throw-away cycle from u = 0, then u = 0 again: every kernel of the cycle has been
        // loaded and the clocks are up before the solve is timed (u is the only state a cycle keeps)
        // (-cold skips it: the solve timer then includes the first, cold iteration like the reference's
        // does -- both figures are reported in DESIGN.md §6)
        if (!opt.cold) {
            MultiGrid::mg_check(mg_cycle(h, nullptr));
            if (opt.fp32) MultiGrid::mg_check(mg_set_solution(h, uf.data()));
            else MultiGrid::mg_check(mg_set_solution(h, u.data()));
            double warm = 0;
            MultiGrid::mg_check(mg_sumsq(h, 0, MG_ARR_RHS, &warm));
        }
    } catch (const MultiGrid::HipError &e) {
        // the reference does not validate n against levels and reads out of range; we stop
        std::cout << "Error: " << e.what() << std::endl;
        return 1;
    }

    auto end = std::chrono::high_resolution_clock::now();
    std::chrono::duration<double> init_time = end - start;
    std::cout << "Initialization time: " << init_time.count() << " seconds" << std::endl;
    start = std::chrono::high_resolution_clock::now();

    switch (opt.smoother) {
    case Gauss_Siedel: std::cout << "GS iters" << std::endl; break;
    case Jacobi: std::cout << "Jacobi iters" << std::endl; break;
    default: std::cout << "BiCGSTAB iters" << std::endl; break;
    }
    const int MaxIter = opt.maxit;
    std::vector<double> hist(static_cast<size_t>(MaxIter) + 1);
    std::vector<mg_cycle_stats> cycles(static_cast<size_t>(MaxIter > 0 ? MaxIter : 1));
    try {
        int nh = 0;
        MultiGrid::mg_check(mg_solve(h, TOL, MaxIter, hist.data(), MaxIter + 1, &nh, cycles.data()));
        hist.resize(static_cast<size_t>(nh));
        for (int i = 0; i + 1 < nh; i++)   // multigrid.hpp:131
            std::cout << "Achieved residual on coarse grid: " << cycles[i].coarse_relres << std::endl;
        if (opt.fp32) {
            MultiGrid::mg_check(mg_get_solution(h, uf.data()));
            u.assign(uf.begin(), uf.end());
        } else {
            MultiGrid::mg_check(mg_get_solution(h, u.data()));
        }
    } catch (const MultiGrid::HipError &e) {
        std::cout << "Error: " << e.what() << std::endl;
        mg_destroy(h);
        return 1;
    }
    // -eig m: the m smallest eigenvalues of the operator just solved with, by mg_eig_solve (tolerance 1e-8, 1e-3 in fp32);
    // printed after the report below
    std::vector<double> eig_lambda(static_cast<size_t>(opt.eig)), eig_relres(static_cast<size_t>(opt.eig));
    mg_eig_stats eig_st{};
    if (opt.eig > 0) {
        try {
            MultiGrid::mg_check(mg_eig_solve(h, opt.eig, opt.eig, opt.fp32 ? 1e-3 : 1e-8, 500, eig_lambda.data(), eig_relres.data(),
                                             nullptr, 0, nullptr, &eig_st));
        } catch (const MultiGrid::HipError &e) {
            std::cout << "Error: " << e.what() << std::endl;
            mg_destroy(h);
            return 1;
        }
    }

    // the reference stops its clock after the iteration loop (main.cpp:114); tearing the device
    // hierarchy down corresponds to its destructors at scope exit, after the report
    end = std::chrono::high_resolution_clock::now();
    mg_destroy(h);
    std::chrono::duration<double> solve_time = end - start;
    std::cout << "||Solving elapsed time: " << solve_time.count() << " sec<br>" << std::endl;
    std::cout << "Tol: " << TOL << "<br>" << std::endl;
    std::cout << "Max iter: " << MaxIter << "<br>" << std::endl;

    if (opt.eig > 0) {
        std::cout << "Eigenvalues: " << eig_st.iters << " LOBPCG iterations, " << eig_st.cycles << " cycles, status " << eig_st.status << std::endl;
        std::cout.precision(15);
        for (int j = 0; j < opt.eig; j++) std::cout << "eig " << j << " " << eig_lambda[j] << " " << eig_relres[j] << std::endl;
    }

    Utils::saveVectorOnFile(hist, "MGGS4.txt");
    Utils::saveVectorOnFile(u, "x.mtx");
    return 0;
}
