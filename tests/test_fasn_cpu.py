"""The semilinear operator with Neumann faces (mg_fas_* with MG_FAS_ON_FACES), numpy only: the numbers
of the design pinned from tests/fasn_ref.py -- the convergence table (the row whose residual is restricted as the mask-free
transition does it must grow), the manufactured solutions, the two bit-for-bit reductions (mask 0 is fas_ref, gamma 0 is
bc_ref), the fixed point of the coarse problem and the conservation identity of one theta step on an insulated box."""
import math

import numpy as np
import pytest

from tests import bc_ref as br
from tests import fas_ref as fr
from tests import fasn_ref as fn
from tests import npref, step_ref
from tests.npref_cycles import CYCLE_F, CYCLE_V, CYCLE_W

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


# ---------------------------------------------------------------- 1. the convergence table (n = 33, 4 levels, red-black V(2,2), 50 coarse sweeps, u = 0)
# The data are the issue's: b = s * default_rng(1).standard_normal with the DIRICHLET nodes set to 0 (the nodes that lie only
# on Neumann faces keep their data). Measured factors at cycle 10 (float64), written down in DESIGN.md section 23:
MEASURED = {
    "cubic-1e3-dirichlet": 0.2547, "cubic-1e3-xlo": 0.3186, "cubic-1e3-only-yhi-dirichlet": 0.5657, "cubic-1e3-all": 0.5657,
    "cubic-1-xlo": 0.1026, "cubic-1-xlo-today": 1.4805,
    "exp-100-dirichlet": 0.4463, "exp-100-xlo": 0.4454, "exp-100-only-yhi-dirichlet": 0.1962,
}


@pytest.mark.parametrize("name", list(fn.TABLE))
def test_table_factor_at_cycle_10(name):
    _, _, hist = fn.table_history(name, cycles=10)
    f = fn.factors(hist)
    print(name, f)
    assert len(hist) == 11 and np.isfinite(hist).all()
    assert f[9] == pytest.approx(fn.TABLE[name][5], rel=0.05)        # the prototype's value
    assert f[9] == pytest.approx(MEASURED[name], abs=2e-4)           # the value written down
    if name in fn.GPU_ROWS:
        assert f[9] <= 0.7
    if name == "cubic-1-xlo-today":   # the residual injected at the coarse nodes of the Neumann face: the cycle diverges
        assert f[9] > 1.0 and (f[5:] > 1.0).all() and hist[-1] > hist[5]


# ---------------------------------------------------------------- 2. the manufactured solutions
@pytest.mark.parametrize("name,want", [("cubic-all", (1.885e-3, 4.945e-4, 1.242e-4)), ("exp-all", (3.693e-2, 9.086e-3, 2.263e-3)),
                                       ("cubic-x", (None, 9.187e-5, 2.326e-5))])
def test_manufactured_solution_is_second_order(name, want):
    errs, cycles = [], []
    for n in (9, 17, 33):
        kind, gamma, mask, f, u = fn.manufactured(name, n)
        P = fn.problem(kind, gamma, mask, n=n, levels=fn.levels_for(n))
        x, hist, status = P.solve_history(np.zeros_like(f), f, 30, fn.TABLE_COARSE_SWEEPS, rtol=1e-12)
        assert status == 0
        errs.append(float(abs(x - u).max())); cycles.append(len(hist) - 1)
    print(name, errs, errs[0] / errs[1], errs[1] / errs[2], cycles)
    for e, w in zip(errs, want):
        if w is not None:
            assert e == pytest.approx(w, rel=1e-3)
    for ratio in (errs[0] / errs[1], errs[1] / errs[2]):
        assert 3.6 <= ratio <= 4.2
    assert cycles[1:] == {"cubic-all": [8, 9], "exp-all": [11, 12], "cubic-x": [9, 10]}[name]


# ---------------------------------------------------------------- 3. mask 0 is fas_ref, bit for bit
SMALL = [dict(dim=3, n=9, levels=2), dict(dim=2, n=17, levels=2), dict(dim=3, n=9, levels=3, semi_xy=1), dict(dim=3, n=9, levels=2, aniso=(1.0, 30.0, 0.05))]


def small_kw(case, prec, **more):
    kw = dict(length=1.0, alpha=1.3, smoother=npref.SMOOTH_RBGS, omega=6.0 / 7.0, nu_pre=2, nu_post=2, restriction=npref.RESTRICT_FULLW,
              outer_pre_gs=0, prec=prec)
    kw.update(case); kw.update(more)
    return kw


@DTYPES
@pytest.mark.parametrize("kind", [fr.CUBIC, fr.EXP], ids=["cubic", "exp"])
@pytest.mark.parametrize("case", SMALL, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items() if k != "aniso"))
def test_mask_zero_equals_fas_ref(case, kind, dtype):
    rng = np.random.default_rng(3)
    for restriction in (npref.RESTRICT_FULLW, npref.RESTRICT_INJECT):
        for cycle in (CYCLE_V, CYCLE_W, CYCLE_F):
            kw = small_kw(case, dtype, restriction=restriction, cycle=cycle)
            P = fn.FASNProblem(mask=0, kind=kind, gamma=0.7, sigma=3.0, **kw)
            Q = fr.FASProblem(kind=kind, gamma=0.7, sigma=3.0, **kw)
            for l in range(min(2, P.L)):
                u, b = (rng.standard_normal(P.shape(l)).astype(dtype) for _ in range(2))
                for got, ref in ((P.residual(u, b, l), Q.residual(u, b, l)), (P.jacobi(u, b, l), Q.jacobi(u, b, l)),
                                 (P.jacobi(u, b, l, 1.0), Q.jacobi(u, b, l, 1.0)), (P.rbgs(u, b, l), Q.rbgs(u, b, l)),
                                 (P.residual_mag(u, b, l), Q.residual_mag(u, b, l)), (P.point_solve_mag(u, b, l), Q.point_solve_mag(u, b, l))):
                    assert got.dtype == dtype and np.array_equal(got, ref)
                if l + 1 < P.L:
                    (uc0, rhs), (vc0, shs) = P.coarse_rhs(u, b, l), Q.coarse_rhs(u, b, l)
                    assert np.array_equal(uc0, vc0) and np.array_equal(rhs, shs) and rhs.dtype == dtype
                    assert np.array_equal(P.correct(u, rhs, uc0, l), Q.correct(u, rhs, uc0, l))
            u, b = (rng.standard_normal(P.shape(0)).astype(dtype) for _ in range(2))
            got, ref = P.vcycle(u, b, 6), Q.vcycle(u, b, 6)
            assert got.dtype == dtype and np.array_equal(got, ref) and P.visits == Q.visits


# ---------------------------------------------------------------- 4. gamma 0 is bc_ref, bit for bit
@DTYPES
@pytest.mark.parametrize("kind", [fr.CUBIC, fr.EXP], ids=["cubic", "exp"])
@pytest.mark.parametrize("case", SMALL, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items() if k != "aniso"))
def test_gamma_zero_equals_bc_ref(case, kind, dtype):
    """the residual, the Jacobi sweep, the red-black sweep and the transition's rc: num = b - s, den = cd"""
    rng = np.random.default_rng(4)
    dim = case["dim"]
    kw = small_kw(case, dtype)
    for mask in [br.all_faces(dim), fn.mixed_mask(dim)] + [1 << k for k in range(2 * dim)]:
        P = fn.FASNProblem(mask=mask, kind=kind, gamma=0.0, sigma=3.0, **kw)
        Q = br.BCProblem(mask=mask, sigma=3.0, **kw)
        for l in range(min(2, P.L)):
            u, b = (rng.standard_normal(P.shape(l)).astype(dtype) for _ in range(2))
            for got, ref in ((P.residual(u, b, l), Q.residual(u, b, l)), (P.jacobi(u, b, l), Q.jacobi(u, b, l)),
                             (P.jacobi(u, b, l, 1.0), Q.jacobi(u, b, l, 1.0)), (P.rbgs(u, b, l), Q.rbgs(u, b, l))):
                assert got.dtype == dtype and np.array_equal(got, ref), mask
            if l + 1 < P.L:
                rc = Q.restrict_fw(b, l)
                assert np.array_equal(P.restrict_fw(b, l), rc)
                uc0, rhs = P.coarse_rhs(u, b, l)
                dm = Q.dirichlet(uc0.shape)
                assert np.array_equal(uc0, Q.inject(u, l)) and np.array_equal(rhs, np.where(dm, uc0, rc + Q.apply_A(uc0, l + 1)))


# ---------------------------------------------------------------- 5. the coarse right-hand side
@pytest.mark.parametrize("kind,gamma,s", [(fr.CUBIC, 1e3, 1e3), (fr.EXP, 100.0, 1e4)], ids=["cubic", "exp"])
def test_exact_fine_solution_is_a_fixed_point_of_the_coarse_problem(kind, gamma, s):
    """n = 9, mixed mask: if u solves the fine problem (residual 1e-13 of the data), the coarse right-hand side is N_c(uc0) up to
    R r, so the coarse solve returns uc0 and the correction is below 1e-10 -- as pinned for fas_ref"""
    P = fn.problem(kind, gamma, fn.mixed_mask(3), n=9, levels=2, prec=np.longdouble)
    b = fn.noise(P, P.shape(0), s)
    u = P.as_prec(np.zeros_like(b))
    for _ in range(600):
        u = P.rbgs(u, b, 0)
    r = P.residual(u, b, 0)
    assert abs(r).max() <= 1e-13 * abs(b).max()
    uc0, rhs = P.coarse_rhs(u, r, 0)
    assert abs(P.residual(uc0, rhs, 1)).max() <= 1e-12 * abs(b).max()   # the coarse residual at uc0 is R r
    uc = P.coarse_solve(uc0, rhs, 1, 50)
    e = uc - uc0
    print(float(abs(e).max()))
    assert abs(e).max() <= 1e-10
    assert abs(P.correct(u, uc, uc0, 0) - u).max() <= 1e-10


# ---------------------------------------------------------------- 6. one theta step on an insulated box conserves what it should
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_theta_step_conserves_on_an_insulated_box(theta):
    n, dt, gamma = 17, 1e-3, 1e3
    u0, f = fn.step_case(n)
    P0 = fn.problem(fr.CUBIC, gamma, 63, n=n, levels=fn.levels_for(n))
    Ps = fn.problem(fr.CUBIC, gamma, 63, sigma=step_ref.shift_of(dt, theta), n=n, levels=fn.levels_for(n))
    assert step_ref.family_of(P0) == "bc" and not step_ref.fixed_nodes(P0, u0.shape).any()
    stepper = step_ref.FamilyStepper(P0, Ps, dt, theta, step_ref.converged_solver(fn.TABLE_COARSE_SWEEPS, 1e-13))
    u1, b = stepper.step(u0, f)
    resnorm = Ps.norm(u1, b)
    assert resnorm <= 1e-13 * float(np.sqrt(np.sum(b * b)))
    diff, bound, mag = fn.step_identity(P0, u0, u1, f, dt, theta, resnorm)
    print(f"theta {theta}: identity off by {diff:.3e} (relative {abs(diff) / mag:.1e}), bound {bound:.3e}")
    assert abs(diff) <= bound
    # the step's right-hand side in the working precision is the stepper's, one rounded operation at a time
    assert np.allclose(step_ref.step_rhs(P0, u0, f, dt, theta), b, rtol=1e-13, atol=0)


@DTYPES
@pytest.mark.parametrize("kind", [fr.CUBIC, fr.EXP])
def test_working_dtype_stays_in_its_dtype(kind, dtype):
    """every expression of the contract is evaluated in T: no silent promotion to float64"""
    P = fn.FASNProblem(mask=fn.mixed_mask(3), kind=kind, gamma=0.7, sigma=3.0, dim=3, n=9, levels=2, prec=dtype, omega=6.0 / 7.0,
                       restriction=npref.RESTRICT_FULLW)
    rng = np.random.default_rng(5)
    u, b = rng.standard_normal(P.shape(0)).astype(dtype), rng.standard_normal(P.shape(0)).astype(dtype)
    uc0, rhs = P.coarse_rhs(u, b, 0)
    for out in (P.residual(u, b, 0), P.jacobi(u, b, 0), P.jacobi(u, b, 0, 1.0), P.rbgs(u, b, 0), uc0, rhs, P.correct(u, rhs, uc0, 0),
                step_ref.step_rhs(P, u, b, 1e-3, 0.5), step_ref.step_rhs(P, u, None, 1e-3, 1.0)):
        assert out.dtype == dtype
