"""mg_set_shift and the implicit heat-equation stepper mg_heat_step / mg_heat_rhs (include/mg_hip.h) on the GPU.

* kernel level: mg_heat_rhs (mg_heat.hip) against its contract restated in numpy, bit for bit;
* the shift: every operator bit for bit against the CPU oracle's operator functions called with a shifted diagonal, whole
  cycles against the same cycle composed from those functions (bit for bit) and against npref with shifted coefficients
  (within cycle_bound), the solve drivers on the shifted operator;
* the stepper: against the same loop written out on a second handle (bit for bit), against an independent long-double
  stepper, against the closed-form decay of a sine mode and the two convergence orders; stats, isolation, determinism,
  refusals.
"""
import ctypes as C
import math
import threading

import numpy as np
import pytest

from multigrid_prj_amd import capi
from oracle import pyoracle as po
from tests import heat_ref as hr
from tests.npref import Problem, boundary_mask, fsum_sq
from tests.test_independent_reference import check_max, cycle_bound, sweep_scale

pytestmark = pytest.mark.gpu

V22 = dict(cycle=capi.CYCLE_V, smoother=capi.SMOOTH_JACOBI, nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW,
           outer_pre_gs=0)
FIXED = dict(coarse_mode=capi.COARSE_FIXED, coarse_maxit=20)
NP = {capi.MG_F64: np.float64, capi.MG_F32: np.float32}


def eps_of(dtype):
    return float(np.finfo(NP[dtype]).eps)


# ---------------------------------------------------------------- kernel level
KCASES = [(2, n) for n in (17, 97, 129, 385)] + [(3, n) for n in (17, 33, 97, 129)]


@pytest.mark.parametrize("dtype", [capi.MG_F64, capi.MG_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("dim,n", KCASES)
def test_heat_rhs_matches_contract(dim, n, dtype):
    rng = np.random.default_rng(100 * n + dim)
    aniso = (1.0, 3.0, 0.25) if (dim, n) == (3, 33) else (1.0, 1.0, 1.0)
    kw = dict(dim=dim, n=n, levels=2, length=1.0, alpha=1.3, aniso=aniso, dtype=dtype)
    dt = 2.5e-4
    with capi.Solver(capi.make_desc(**kw)) as s:
        shape = s.level_shape(0)
        coef0 = s.level_coefficients(0)
        assert coef0 == po.level_coef(po.make_desc(**kw), 0)
        u = rng.standard_normal(shape).astype(s.np)
        f = (rng.standard_normal(shape) * 1e3).astype(s.np)
        other = rng.standard_normal(shape).astype(s.np)
        s.set_array(capi.ARR_E, 0, u)
        s.set_shift(123.0)          # the assembly uses the UNSHIFTED diagonal whatever the shift
        for src in (None, f):
            s.heat_set_source(src)
            for theta in (1.0, 0.5, 0.75):
                s.set_array(capi.ARR_RES, 0, other)
                s.heat_rhs(dt, theta, capi.ARR_E, capi.ARR_RES)
                got = s.get_array(capi.ARR_RES, 0)
                ref = hr.heat_rhs_np(u, src, coef0, dt, theta)
                assert np.array_equal(got, ref), (theta, src is not None, int((got != ref).sum()))
                assert np.array_equal(got[boundary_mask(shape)], u[boundary_mask(shape)])
                if theta == 1.0:    # the stencil-free form is the general formula's value
                    assert np.array_equal(got, hr.heat_rhs_np(u, src, coef0, dt, theta, general=False))
                assert np.array_equal(s.get_array(capi.ARR_E, 0), u)
        assert s.get_shift() == 123.0


# ---------------------------------------------------------------- the shift, operator by operator
class ShiftedOracle:
    """the CPU oracle's operator functions (po.lib()) called with the diagonal cd + sigma on every level, and the two
    cycles composed from them as oracle/gmg_cycle.inc composes them"""

    def __init__(self, kw, sigma):
        self.d = po.make_desc(**kw)
        self.ops = po.Ops(self.d)
        self.sigma = sigma
        self.suf = self.ops.suf
        self.real = self.ops.real

    def coef(self, l):
        c = po.level_coef(self.d, l)
        return (po.CoefF64 if self.d.dtype == po.MG_F64 else po.CoefF32)(c[0], c[1], c[2], c[3] + self.sigma)

    def _f(self, name):
        return getattr(po.lib(), f"orc_{name}_{self.suf}")

    def smooth(self, l, smoother, sweeps, u, b, omega=None):
        out, tmp = u.copy(), np.empty_like(u)
        n, nz = po.Ops._nnz(u)
        self._f("smooth")(smoother, self.d.dim, n, nz, self.coef(l), self.real(self.d.omega if omega is None else omega), sweeps,
                          po._ptr(out), po._ptr(b), po._ptr(tmp))
        return out

    def residual(self, l, u, b):
        r = np.empty_like(u)
        n, nz = po.Ops._nnz(u)
        return r, self._f("residual")(self.d.dim, n, nz, self.coef(l), po._ptr(u), po._ptr(b), po._ptr(r))

    def coarse(self, l, smoother, e, b, maxit, tol, fixed):
        out, tmp = e.copy(), np.empty_like(e)
        flag, rel = C.c_int(0), C.c_double(0)
        n, nz = po.Ops._nnz(e)
        its = self._f("coarse_solve")(smoother, self.d.dim, n, nz, self.coef(l), self.real(self.d.omega), po._ptr(out), po._ptr(b),
                                      po._ptr(tmp), maxit, tol, int(fixed), C.byref(flag), C.byref(rel))
        return out, its, flag.value, rel.value

    def _coarse_of_cycle(self, l, e, b):
        d = self.d
        sm = po.SMOOTH_RBGS if d.smoother in (po.SMOOTH_ZEBRA_Y, po.SMOOTH_ZEBRA_X) else d.smoother
        return self.coarse(l, sm, e, b, d.coarse_maxit, d.coarse_tol, d.coarse_mode == po.COARSE_FIXED)[0]

    def vcycle(self, u, b, l=0):
        d = self.d
        if l == d.levels - 1:
            return self._coarse_of_cycle(l, u, b)
        u = self.smooth(l, d.smoother, d.nu_pre, u, b)
        r, _ = self.residual(l, u, b)
        rc = self.ops.restrict_fw(r) if d.restriction == po.RESTRICT_FULLW else self.ops.inject(r)
        ec = self.vcycle(np.zeros_like(rc), rc, l + 1)
        u = self.ops.prolong_add(ec, u)
        return self.smooth(l, d.smoother, d.nu_post, u, b)

    def sawtooth(self, u, b):
        d = self.d
        r = [self.residual(0, u, b)[0]]
        for l in range(d.levels - 1):
            r.append(self.ops.inject(r[-1]))
        e = self._coarse_of_cycle(d.levels - 1, np.zeros_like(r[-1]), r[-1])
        for l in range(d.levels - 2, -1, -1):
            e = self.smooth(l, d.smoother, d.nu_post, self.ops.prolong_overwrite(e), r[l])
        return self.ops.correct(u, e)[0]

    def cycle(self, u, b):
        return self.vcycle(u, b) if self.d.cycle == po.CYCLE_V else self.sawtooth(u, b)


GRIDS = {"2d65": dict(dim=2, n=65, levels=4, length=10.0, alpha=1.0), "3d33": dict(dim=3, n=33, levels=3, length=1.0, alpha=2.5),
         "3d49": dict(dim=3, n=49, levels=3, length=1.0, alpha=2.5)}   # 49, 25, 13: off 2^k + 1 (tests/size_table.py)
OPCFG = {
    "jacobi-omega1": dict(smoother=capi.SMOOTH_JACOBI, omega=1.0),
    "jacobi-omega0.8": dict(smoother=capi.SMOOTH_JACOBI, omega=0.8),
    "zebra-y": dict(smoother=capi.SMOOTH_ZEBRA_Y),
    "zebra-x": dict(smoother=capi.SMOOTH_ZEBRA_X),
}


@pytest.mark.parametrize("dtype", [capi.MG_F64, capi.MG_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("factor", [0.37, 50.0])
@pytest.mark.parametrize("cfg", list(OPCFG))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_shifted_operators_bit_exact_against_oracle(grid, cfg, factor, dtype):
    """sigma = factor * cd0 of level 0: 50 cd0 changes rcd and the outcome of make_coef's Markstein window test on the
    coarse levels. Levels 0 and 1; the descriptor's smoother on every configuration, and on the damped-Jacobi one also
    lexicographic GS, red-black, the residual + norm and the coarse solve in both modes."""
    kw = dict(GRIDS[grid], **OPCFG[cfg], dtype=dtype)
    rng = np.random.default_rng(5)
    rtol = 1e-12 if dtype == capi.MG_F64 else 1e-6
    with capi.Solver(capi.make_desc(**kw)) as s:
        cd0 = s.level_coefficients(0)[3]
        sigma = factor * cd0
        s.set_shift(sigma)
        assert s.get_shift() == sigma
        O = ShiftedOracle(kw, sigma)
        for l in (0, 1):
            c = s.level_coefficients(l)
            assert c[:3] == po.level_coef(O.d, l)[:3] and c[3] == po.level_coef(O.d, l)[3] + sigma
            shp = s.level_shape(l)
            u, b = rng.standard_normal(shp).astype(s.np), rng.standard_normal(shp).astype(s.np)
            s.set_array(capi.ARR_RHS, l, b)

            def run(smoother, sweeps):
                s.set_array(capi.ARR_E, l, u)
                s.smooth(l, smoother, sweeps, capi.ARR_E, capi.ARR_RHS)
                return s.get_array(capi.ARR_E, l)

            sm = kw["smoother"]
            for sweeps in (1, 3):
                assert np.array_equal(run(sm, sweeps), O.smooth(l, sm, sweeps, u, b)), (cfg, l, sweeps)
            if cfg != "jacobi-omega0.8":
                continue
            for other in (capi.SMOOTH_GS_LEX, capi.SMOOTH_RBGS):
                assert np.array_equal(run(other, 2), O.smooth(l, other, 2, u, b)), (other, l)
            s.set_array(capi.ARR_E, l, u)
            ss = s.residual(l, capi.ARR_E, capi.ARR_RHS, capi.ARR_TMP)
            r_ref, ss_ref = O.residual(l, u, b)
            assert np.array_equal(s.get_array(capi.ARR_TMP, l), r_ref)
            assert ss == pytest.approx(ss_ref, rel=rtol)
            assert s.residual(l, capi.ARR_E, capi.ARR_RHS, -1) == ss
            for csm in (capi.SMOOTH_JACOBI, capi.SMOOTH_RBGS):
                for fixed, maxit, tol in ((False, 2000, 0.1), (True, 7, 0.1)):
                    s.zero_array(capi.ARR_E, l)
                    st = s.coarse_solve_ex(l, capi.ARR_E, capi.ARR_RHS, csm, maxit, tol, fixed)
                    e, its, flag, rel = O.coarse(l, csm, np.zeros_like(b), b, maxit, tol, fixed)
                    assert (st.coarse_iters, st.coarse_flag) == (its, flag), (csm, fixed, l)
                    assert st.coarse_relres == pytest.approx(rel, rel=1e-10 if dtype == capi.MG_F64 else 1e-5)
                    assert np.array_equal(s.get_array(capi.ARR_E, l), e), (csm, fixed, l)


# ---------------------------------------------------------------- the shift, whole cycles
CYCLES = {"v22-fullw": dict(V22, omega=0.8), "sawtooth": dict(cycle=capi.CYCLE_SAWTOOTH, smoother=capi.SMOOTH_JACOBI, omega=0.8,
                                                              nu_pre=0, nu_post=3, restriction=capi.RESTRICT_INJECT)}


@pytest.mark.parametrize("cyc", list(CYCLES))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_shifted_cycle_against_oracle_composition_and_npref(grid, cyc):
    kw = dict(GRIDS[grid], **CYCLES[cyc], **FIXED)
    rng = np.random.default_rng(17)
    with capi.Solver(capi.make_desc(**kw)) as s:
        sigma = 0.37 * s.level_coefficients(0)[3]
        s.set_shift(sigma)
        shp = s.level_shape(0)
        b = rng.standard_normal(shp)
        u0 = 0.1 * rng.standard_normal(shp)
        s.set_rhs(b); s.set_solution(u0)
        st = s.cycle()
        got = s.get_solution()
    assert st.coarse_iters == FIXED["coarse_maxit"]
    assert np.array_equal(got, ShiftedOracle(kw, sigma).cycle(u0, b))
    P = hr.shifted_problem(kw, sigma)
    ref = P.cycle(u0, b, FIXED["coarse_maxit"])
    scale = float(np.abs(ref).max()) + sweep_scale(P, 0, b, u0)
    check_max(got, ref, cycle_bound(P, eps_of(capi.MG_F64), FIXED["coarse_maxit"], scale), f"{grid} {cyc}")


def test_shifted_vcycle_129_runs_the_fused_paths():
    """3-D n = 129, 4 levels, fp64, V(2,2) Jacobi full weighting: level 0 (129^3) runs the fused Jacobi pair k_jacobi2 (64
    vectors per row + the odd column) and the fused residual + restriction k_resid_restrict_fw, with the prolongation folded
    into the post-smoothing pair; the wide-tile kernels k_pairw / k_rrw need rows of 128 lanes and ny >= 200 and stay
    closed at this size; levels 1 and 2 (65^3, 33^3) run the small-level bricks of mg_small_levels.hip; 17^3 is the
    one-workgroup coarse solve."""
    kw = dict(dim=3, n=129, levels=4, length=1.0, alpha=1.0, **dict(V22, omega=6 / 7), **FIXED)
    rng = np.random.default_rng(23)
    with capi.Solver(capi.make_desc(**kw)) as s:
        sigma = 0.37 * s.level_coefficients(0)[3]
        s.set_shift(sigma)
        b = rng.standard_normal(s.level_shape(0))
        u0 = 0.1 * rng.standard_normal(s.level_shape(0))
        s.set_rhs(b); s.set_solution(u0)
        s.cycle()
        got = s.get_solution()
    assert np.array_equal(got, ShiftedOracle(kw, sigma).cycle(u0, b))


@pytest.mark.parametrize("smoother", [capi.SMOOTH_JACOBI, capi.SMOOTH_ZEBRA_Y], ids=["jacobi", "zebra-y"])
def test_shift_zero_restores_the_creation_state(smoother):
    kw = dict(dim=3, n=33, levels=3, length=1.0, **dict(V22, smoother=smoother, omega=0.8), **FIXED)
    rng = np.random.default_rng(29)
    b, u0 = rng.standard_normal((33,) * 3), rng.standard_normal((33,) * 3)
    out = []
    for shift_first in (False, True):
        with capi.Solver(capi.make_desc(**kw)) as s:
            c0 = [s.level_coefficients(l) for l in range(3)]
            if shift_first:
                s.set_shift(3.7 * c0[0][3])
                s.set_rhs(b); s.set_solution(u0)
                s.cycle()
                assert not np.array_equal(s.get_solution(), out[0])
                s.set_shift(0.0)
                assert [s.level_coefficients(l) for l in range(3)] == c0 and s.get_shift() == 0.0
            s.set_rhs(b); s.set_solution(u0)
            s.cycle()
            out.append(s.get_solution())
    assert np.array_equal(out[0], out[1])


# ---------------------------------------------------------------- the shift under the solve drivers
def shifted_coef(s, kw, sigma):
    """the handle's level-0 coefficients, checked to be the oracle's with ONE fp64 addition on the diagonal: the operator
    the numpy residuals below are taken with. (A diagonal summed in long double differs from it by up to half an ulp,
    1e-16 cd; that is a SYSTEMATIC difference delta_cd * u in the residual, and against a residual of 1e-11 |b| its
    correlation with r, delta_cd (r.u) / (r.r), reaches 1e-6: measured 1.08e-6 at 33^3.)"""
    c, o = s.level_coefficients(0), po.level_coef(po.make_desc(**kw), 0)
    assert c == (o[0], o[1], o[2], o[3] + sigma)
    return c


SOLVE_KW = dict(dim=3, n=33, levels=3, length=1.0, alpha=1.0, **dict(V22, omega=6 / 7))


def solve_rhs(seed):
    """random right-hand side with ZERO Dirichlet data. The drivers below are taken to residuals of 1e-10 .. 1e-11 of |b|
    and compared with a long-double residual; the fp64 residual the library evaluates carries a rounding of about
    eps * |cd u| per node, which has to stay well below that. With random O(1) boundary values the rows next to the
    boundary hold terms c * u_boundary ~ 1e3 |b| (rounding 5e-13 |b|, 5 % of a residual of 1e-11); with zero boundary
    values every term is O(|b|) and the rounding is 1e-16 |b|, 1e-5 of the residual, 1e-7 of its norm."""
    b = np.random.default_rng(seed).standard_normal((33,) * 3)
    b[boundary_mask(b.shape)] = 0.0
    return b


def start(b):
    u0 = np.zeros_like(b)
    u0[boundary_mask(b.shape)] = b[boundary_mask(b.shape)]
    return u0


def test_solve_on_the_shifted_operator():
    b = solve_rhs(31)
    with capi.Solver(capi.make_desc(**SOLVE_KW)) as s:
        s.set_rhs(b); s.set_solution(start(b))
        h0, _ = s.solve(1e-10, 100)
        sigma = 0.37 * s.level_coefficients(0)[3]
        s.set_shift(sigma)
        s.set_rhs(b); s.set_solution(start(b))
        h1, _ = s.solve(1e-10, 100)
        u = s.get_solution()
        coef = shifted_coef(s, SOLVE_KW, sigma)
    print("cycles unshifted", len(h0) - 1, "shifted", len(h1) - 1, "last", h1[-1], "numpy", hr.relres_ld(u, b, coef))
    assert h0[-1] <= 1e-10 and h1[-1] <= 1e-10
    assert len(h1) - 1 <= len(h0) - 1 + 2
    np.testing.assert_allclose(hr.relres_ld(u, b, coef), h1[-1], rtol=1e-6)


def test_pcg_on_the_shifted_operator():
    b = solve_rhs(37)
    with capi.Solver(capi.make_desc(**SOLVE_KW)) as s:
        sigma = 0.37 * s.level_coefficients(0)[3]
        s.set_shift(sigma)
        s.set_rhs(b); s.set_solution(np.zeros_like(b))
        hist, st = s.pcg_solve(1e-10, 60)
        u = s.get_solution()
        coef = shifted_coef(s, SOLVE_KW, sigma)
    assert st.status == capi.PCG_CONVERGED
    np.testing.assert_allclose(st.relres_true, hr.relres_ld(u, b, coef), rtol=1e-6)


def test_mixed_solve_on_the_shifted_operator():
    b = solve_rhs(41)
    with capi.Solver(capi.make_desc(**SOLVE_KW, dtype=capi.MG_F32)) as s:
        sigma = 0.37 * s.level_coefficients(0)[3]
        s.set_shift(sigma)
        s.mixed_set_rhs(b); s.mixed_set_solution(np.zeros_like(b))
        hist, st = s.mixed_solve(1e-11, 40, 4)
        u = s.mixed_get_solution()
        coef = shifted_coef(s, dict(SOLVE_KW, dtype=capi.MG_F32), sigma)
    assert st.status == capi.MIXED_CONVERGED and st.relres <= 1e-11
    # | ||r_gpu|| - ||r|| | <= ||r_gpu - r|| <= C_RESID eps || |A||u| + |b| ||  (the fp64 residual's rounding, node by node)
    P = hr.shifted_problem(SOLVE_KW, sigma)
    mag = P.apply_A(u, 0, absolute=True) + np.abs(b)
    bound = 16 * eps_of(capi.MG_F64) * math.sqrt(fsum_sq(mag) / fsum_sq(b))
    ref = hr.relres_ld(u, b, coef)
    print("mixed: relres", st.relres, "numpy", ref, "difference", abs(st.relres - ref), "bound", bound)
    assert abs(st.relres - ref) <= bound


def test_fmg_on_the_shifted_operator():
    b = np.random.default_rng(43).standard_normal((33,) * 3)
    with capi.Solver(capi.make_desc(**SOLVE_KW)) as s:
        sigma = 0.37 * s.level_coefficients(0)[3]
        s.set_shift(sigma)
        s.set_rhs(b)
        st = s.fmg(2)
        u = s.get_solution()
        coef = shifted_coef(s, SOLVE_KW, sigma)
    print("fmg relres", st.relres)
    assert st.relres > 0 and math.isfinite(st.relres)
    np.testing.assert_allclose(st.relres, hr.relres_ld(u, b, coef), rtol=1e-9)


# ---------------------------------------------------------------- the stepper
STEP_GRIDS = {"2d65": dict(dim=2, n=65, levels=4, length=1.0, alpha=1.0), "3d33": dict(dim=3, n=33, levels=3, length=1.0, alpha=1.0),
              "3d49": dict(dim=3, n=49, levels=3, length=1.0, alpha=1.0)}
STEP_CYCLES = {"v22": dict(V22, omega=0.8), "sawtooth": dict(cycle=capi.CYCLE_SAWTOOTH, smoother=capi.SMOOTH_JACOBI, omega=0.8,
                                                             nu_pre=0, nu_post=3, restriction=capi.RESTRICT_INJECT, outer_pre_gs=2)}


def heat_problem(shape, seed):
    """random initial state with non-constant Dirichlet data, random source"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), 10.0 * rng.standard_normal(shape)


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("cyc", list(STEP_CYCLES))
@pytest.mark.parametrize("grid", list(STEP_GRIDS))
def test_step_equals_the_loop_written_out(grid, cyc, theta):
    kw = dict(STEP_GRIDS[grid], **STEP_CYCLES[cyc], **FIXED)
    dt = 1e-3
    u0, f = heat_problem((kw["n"],) * kw["dim"], 47)
    with capi.Solver(capi.make_desc(**kw)) as s, capi.Solver(capi.make_desc(**kw)) as s2:
        s.heat_set_source(f); s.set_solution(u0)
        st = s.heat_step(dt, theta, 3, 2)
        s2.heat_set_source(f); s2.set_solution(u0)
        s2.set_shift(1.0 / (theta * dt))
        for _ in range(3):
            s2.heat_rhs(dt, theta, capi.ARR_U, capi.ARR_RHS)
            for _c in range(2):
                if kw["outer_pre_gs"]:
                    s2.smooth(0, capi.SMOOTH_GS_LEX, kw["outer_pre_gs"], capi.ARR_U, capi.ARR_RHS)
                s2.cycle()
        assert (st.steps, st.cycles) == (3, 6) and s.get_shift() == s2.get_shift() == 1.0 / (theta * dt)
        assert np.array_equal(s.get_solution(), s2.get_solution())
        assert np.array_equal(s.get_array(capi.ARR_RHS, 0), s2.get_array(capi.ARR_RHS, 0))


@pytest.mark.parametrize("dtype", [capi.MG_F64, capi.MG_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("grid", list(STEP_GRIDS))
def test_step_against_an_independent_stepper(grid, theta, dtype):
    """npref in long double runs the same sweep and cycle counts; bound: steps x cycle_bound"""
    kw = dict(STEP_GRIDS[grid], **STEP_CYCLES["v22"], **FIXED)
    dt, steps = 1e-3, 3
    u0, f = heat_problem((kw["n"],) * kw["dim"], 53)
    u0, f = u0.astype(NP[dtype]), f.astype(NP[dtype])
    with capi.Solver(capi.make_desc(**kw, dtype=dtype)) as s:
        s.heat_set_source(f); s.set_solution(u0)
        s.heat_step(dt, theta, steps, 1)
        got = s.get_solution()
    ref = hr.ThetaStepper(kw, dt, theta, hr.cycle_solver(1, FIXED["coarse_maxit"]))
    u, scale = ref.P0.as_prec(u0), 0.0
    for _ in range(steps):
        un, b = ref.step(u, f)
        scale = max(scale, float(np.abs(un).max()) + sweep_scale(ref.Ps, 0, b, u))
        u = un
    check_max(got, u, steps * cycle_bound(ref.Ps, eps_of(dtype), FIXED["coarse_maxit"], scale), f"{grid} theta {theta}")


# c of the rounding term c * eps * 8 * ||u0||: 8 x the largest error / (eps * 8 * ||u0||) observed over the first four cases below on
# MI355X. The algebraic term is an upper bound that exceeded the whole error in every case (error - algebraic < 0), so the
# WHOLE observed error is charged to rounding here, the conservative reading: 8 x 15.6 -> 125.
# (3d49, added with the grids off 2^k + 1, was measured after the constant was set: 5.48 and 2.83, below the largest)
PHYSICS_OBSERVED = {"2d65 theta 1": 15.65, "2d65 theta 0.5": 2.28, "3d33 theta 1": 3.65, "3d33 theta 0.5": 0.51,
                    "3d49 theta 1": 5.48, "3d49 theta 0.5": 2.83}
PHYSICS_C = 125.0
PHYSICS_CYCLES = 16


def physics_run(kw, theta, dt, steps):
    shape = (kw["n"],) * kw["dim"]
    u0 = hr.lowest_mode(shape)
    norms, rel = [], []
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_solution(u0)
        for _ in range(steps):
            norms.append(math.sqrt(fsum_sq(s.get_solution())))
            rel.append(s.heat_step(dt, theta, 1, PHYSICS_CYCLES).relres)
        return u0, s.get_solution(), np.array(norms), np.array(rel)


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("grid", list(STEP_GRIDS))
def test_decay_of_the_lowest_mode(grid, theta):
    kw = dict(STEP_GRIDS[grid], **STEP_CYCLES["v22"])
    lam, lam_max = hr.eigen_range(Problem(**kw))
    dt = 0.1 / lam
    u0, u, norms, rel = physics_run(kw, theta, dt, 8)
    print(grid, theta, "relres per step", rel)
    assert np.all(rel <= 1e-12)
    sigma = 1.0 / (theta * dt)
    kappa = (sigma + lam_max) / (sigma + lam)
    exact = (u0.astype(np.longdouble) * np.longdouble(hr.growth(theta, dt, lam)) ** 8)
    err = float(np.sqrt(np.sum((u - exact) ** 2)))
    algebraic = float(np.sum(kappa * rel * norms))
    unit = eps_of(capi.MG_F64) * 8 * math.sqrt(fsum_sq(u0))
    print(grid, theta, "error", err, "algebraic term", algebraic, "error / (eps 8 |u0|) =", err / unit,
          "(error - algebraic) / (eps 8 |u0|) =", (err - algebraic) / unit)
    assert PHYSICS_C <= 1000
    assert err <= algebraic + PHYSICS_C * unit


@pytest.mark.parametrize("theta,lo,hi", [(0.5, 3.0, 5.0), (1.0, 1.6, 2.4)])
@pytest.mark.parametrize("grid", list(STEP_GRIDS))
def test_convergence_order_in_time(grid, theta, lo, hi):
    """t_end = 0.8 / lam in 8 and in 16 steps: the time error (3e-4 and 1.7e-2 of |u0| at 8 steps, tests/test_heat_cpu.py)
    is more than 100 x the bound of the algebraic and rounding error, which is asserted"""
    kw = dict(STEP_GRIDS[grid], **STEP_CYCLES["v22"])
    lam, lam_max = hr.eigen_range(Problem(**kw))
    t_end = 0.8 / lam
    errs = []
    for steps in (8, 16):
        dt = t_end / steps
        u0, u, norms, rel = physics_run(kw, theta, dt, steps)
        sigma = 1.0 / (theta * dt)
        other = float(np.sum((sigma + lam_max) / (sigma + lam) * rel * norms)) + PHYSICS_C * eps_of(capi.MG_F64) * steps * math.sqrt(fsum_sq(u0))
        e = float(np.sqrt(np.sum((u - u0.astype(np.longdouble) * np.longdouble(math.exp(-lam * t_end))) ** 2)))
        assert e >= 100 * other, (e, other)
        errs.append(e)
    print(grid, theta, "errors", errs, "ratio", errs[0] / errs[1])
    assert lo <= errs[0] / errs[1] <= hi


def test_stats_isolation_determinism():
    kw = dict(STEP_GRIDS["3d33"], **STEP_CYCLES["v22"])
    u0, f = heat_problem((33,) * 3, 59)
    dt, theta = 2e-3, 0.5
    with capi.Solver(capi.make_desc(**kw)) as s:
        base = s.device_bytes()
        s.heat_set_source(None)
        assert s.device_bytes() == base
        s.heat_set_source(f)
        assert s.device_bytes() - base == 8 * (33 + 2) * 33 * 48     # one level-0 array: nz + 2 planes of 33 rows of 48 doubles
        s.heat_set_source(f)
        assert s.device_bytes() - base == 8 * 35 * 33 * 48
        s.set_solution(u0)
        st = s.heat_step(dt, theta, 5, 3)
        assert (st.steps, st.cycles) == (5, 15) and st.time == 5 * dt and s.get_shift() == 1.0 / (theta * dt)
        rr = s.residual(0, capi.ARR_U, capi.ARR_RHS, -1)
        bb = s.sumsq(0, capi.ARR_RHS)
        np.testing.assert_allclose(st.relres, math.sqrt(rr / bb), rtol=1e-12)
        u1 = s.get_solution()
        # the source survives the call: the same steps again give the same bits; without it they do not
        s.set_solution(u0)
        st2 = s.heat_step(dt, theta, 5, 3)
        assert np.array_equal(s.get_solution(), u1) and st2.relres == st.relres
        s.heat_set_source(None)
        s.set_solution(u0)
        s.heat_step(dt, theta, 5, 3)
        assert not np.array_equal(s.get_solution(), u1)
        assert s.device_bytes() - base == 8 * 35 * 33 * 48
        # the profile brackets keep timing the level-0 launches of the cycles inside: what two plain cycles report
        counts = []
        for run in (lambda: s.heat_step(dt, theta, 2, 1), lambda: s.cycle_async(2)):
            s.profile_begin()
            run()
            ms, sweeps = s.profile_end()
            ms_f, sweeps_f = s.profile_fused()
            assert ms + ms_f > 0
            counts.append((sweeps, sweeps_f))
        assert counts[0] == counts[1] and sum(counts[0]) == 2 * (kw["nu_pre"] + kw["nu_post"])


def refused(call, word=None):
    with pytest.raises(capi.MgError) as e:
        call()
    assert e.value.code == -4 and (word is None or word in str(e.value)), str(e.value)


def test_refusals():
    kw = dict(STEP_GRIDS["2d65"], **STEP_CYCLES["v22"])
    u0, _ = heat_problem((65, 65), 61)
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_solution(u0)
        s.set_shift(7.5)
        bad = [
            (lambda: s.set_shift(-1.0), "sigma"), (lambda: s.set_shift(math.inf), "sigma"), (lambda: s.set_shift(math.nan), "sigma"),
            (lambda: s.heat_step(0.0, 1.0, 1, 1), "dt"), (lambda: s.heat_step(-1e-3, 1.0, 1, 1), "dt"),
            (lambda: s.heat_step(math.inf, 1.0, 1, 1), "dt"), (lambda: s.heat_step(math.nan, 1.0, 1, 1), "dt"),
            (lambda: s.heat_step(1e-3, 0.0, 1, 1), "theta"), (lambda: s.heat_step(1e-3, 1.5, 1, 1), "theta"),
            (lambda: s.heat_step(1e-3, math.nan, 1, 1), "theta"),
            (lambda: s.heat_step(1e-3, 1.0, 0, 1), "nsteps"), (lambda: s.heat_step(1e-3, 1.0, 1, 0), "cycles_per_step"),
            (lambda: s.heat_rhs(1e-3, 1.0, capi.ARR_U, capi.ARR_U), "arr_dst"), (lambda: s.heat_rhs(0.0, 1.0), "dt"),
            (lambda: s.heat_rhs(1e-3, 2.0), "theta"),
        ]
        for call, word in bad:
            refused(call, word)
            assert s.get_shift() == 7.5 and np.array_equal(s.get_solution(), u0)
        s.set_stage_callback(lambda *a: None)
        refused(lambda: s.heat_step(1e-3, 1.0, 1, 1), "stage callback")
        assert s.get_shift() == 7.5 and np.array_equal(s.get_solution(), u0)
        s.set_stage_callback(None)
        assert s.heat_step(1e-3, 1.0, 1, 1).steps == 1


def test_refuses_distributed_handle():
    from tests.thread_ranks import ThreadWorld
    kw = dict(dim=3, n=33, levels=3, length=1.0, **dict(V22, omega=0.8), dist_min_n=9)
    desc = capi.make_desc(**kw)
    tw = ThreadWorld(2)
    res = [None, None]

    def calls(s, nz):
        return (lambda: s.set_shift(1.0), lambda: s.heat_set_source(np.ones((nz, 33, 33))), lambda: s.heat_step(1e-3, 1.0, 1, 1),
                lambda: s.heat_rhs(1e-3, 1.0))

    def rank_main(r):
        try:
            z0, nz, _ = capi.plan_slab(desc, 2, r, 0)
            s = capi.Solver(desc, device=0, rank=r, nranks=2, host_comm=tw.host_comm(r))
            try:
                got = []
                for call in calls(s, nz):
                    try:
                        call()
                        got.append("accepted")
                    except capi.MgError as e:
                        got.append((e.code, "distributed" in str(e)))
                got.append(s.get_shift())
                res[r] = got
            finally:
                s.close()
        except Exception as e:   # noqa: BLE001 -- reported below
            res[r] = repr(e)

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert res == [[(-4, True)] * 4 + [0.0]] * 2, res
    with capi.Solver(desc, device=0, rank=0, nranks=2, dry=True) as s:   # the dry-run measurement handle is distributed too
        for call in calls(s, s.level_shape(0)[0]):
            refused(call, "distributed")
        assert s.get_shift() == 0.0
