"""The full approximation scheme on the GPU (mg_fas_*, multigrid_prj_amd/csrc/mg_fas.hip) against tests/fas_ref.py: the cubic
kernels bit for bit (plain form and marching tile), gamma = 0 against the existing entry points bit for bit, the exp kernels
to the accuracy of the device's exp, the FAS transition and the correction bit for bit, the coarse solve, one cycle of each
kind against the long-double reference, the solves of DESIGN.md section 20 and the contracts of the C ABI."""
import functools

import numpy as np
import pytest

from multigrid_prj_amd import capi
from tests import npref
from tests import fas_ref as fr
from tests import tile_cases as tc

pytestmark = pytest.mark.gpu

NP = {capi.MG_F64: np.float64, capi.MG_F32: np.float32}
DTYPES = pytest.mark.parametrize("dtype", [capi.MG_F64, capi.MG_F32], ids=["f64", "f32"])
U, E, RHS, TMP, RES = capi.ARR_U, capi.ARR_E, capi.ARR_RHS, capi.ARR_TMP, capi.ARR_RES
JAC, RB = capi.SMOOTH_JACOBI, capi.SMOOTH_RBGS
INJECT, FULLW = capi.RESTRICT_INJECT, capi.RESTRICT_FULLW
CUBIC, EXP = capi.FAS_CUBIC, capi.FAS_EXP
LD = np.longdouble

# tests/test_vc_gpu.py's CASES: 9, 17 plain; 33, 35, 34 march in fp64; 65, 67 march in both (35: odd last column, not 2^k + 1;
# 67: a partial last vector in fp32; 34: an even row in fp64); 2-D always plain
CASES = [
    (3, 9, 2, {}), (3, 17, 2, {}), (3, 33, 2, {}), (3, 35, 2, {}), (3, 34, 1, {}), (3, 65, 2, {}), (3, 67, 2, {}),
    (2, 17, 2, {}), (2, 130, 1, {}),
    (3, 17, 2, {"aniso": (1.0, 30.0, 0.05)}), (3, 17, 3, {"semi_xy": 1}),
]
# ... on all of which the tile sees a cube with cx == cy == cz (the last two are plain). tests/tile_cases.py: a33, a65 put it on
# pairwise distinct axis coefficients, sa65, s67, s129 on a level with nz != nx (sa65: both at once; s67: an even row, 34 x 34 x 67;
# s129: the fp32 tile, level 1 only)
CASES += tc.CASES
case_id = tc.case_id


def desc_kw(dim, n, levels, extra, dtype, **more):
    kw = dict(dim=dim, n=n, levels=levels, length=1.0, alpha=1.3, dtype=dtype, cycle=capi.CYCLE_V, smoother=RB, nu_pre=2, nu_post=2,
              restriction=FULLW, outer_pre_gs=0, coarse_mode=capi.COARSE_FIXED, coarse_maxit=6)
    kw.update(extra); kw.update(more)
    return kw


def problem_of(s, kw, prec, kind, gamma, sigma=0.0):
    """the reference of a handle's descriptor in `prec`, with the handle's own level coefficients (shift included)"""
    P = fr.FASProblem(kind=kind, gamma=gamma, sigma=sigma, prec=prec, **{k: v for k, v in kw.items() if k != "dtype"})
    P.use_handle_coefs([s.level_coefficients(l) for l in range(kw["levels"])])
    return P


def sumsq(r):
    return npref.fsum_sq(r)


def is_march(dim, shape, T):
    return dim == 3 and fr.march_ok(3, shape[2], shape[1], shape[0], np.dtype(T).itemsize)


# ---------------------------------------------------------------- 1. the cubic kernels, bit for bit
@DTYPES
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cubic_kernels_bit_for_bit(case, dtype):
    """residual (saved and norm only), one Jacobi sweep (omega 1 and 6/7) and one red-black sweep on the case's levels to check
    (0 and 1; s129: 1), sigma 0 and 500, gamma 0.7 and -0.3, standard-normal data (den = cd + 3 G u^2 keeps its sign); where the
    marching tile takes the level the plain form is run too (mg_fas_set_form) against the same numbers. The inputs come back
    unmodified. The tile on distinct axis coefficients: a33, a65, sa65; on nz != nx: sa65, s67 (an even row), s129 (fp32)."""
    dim, n, levels, extra = case
    T = NP[dtype]
    rng = np.random.default_rng(100 * dim + n)
    check = tc.levels_to_check(case)
    forms_seen = {l: set() for l in check}
    for omega in (1.0, 6.0 / 7.0):
        kw = desc_kw(dim, n, levels, extra, dtype, omega=omega)
        with capi.Solver(capi.make_desc(**kw)) as s:
            for sigma in (0.0, 500.0):
                s.set_shift(sigma)
                for gamma in (0.7, -0.3):
                    s.fas_set_reaction(CUBIC, gamma)
                    assert s.fas_get_reaction() == (CUBIC, gamma)
                    P = problem_of(s, kw, T, fr.CUBIC, gamma, sigma)
                    for l in check:
                        shape = s.level_shape(l)
                        assert tuple(shape) == tc.level_shape(case, l)
                        u, b, other = (rng.standard_normal(shape).astype(T) for _ in range(3))
                        jac_ref = P.jacobi(u, b, l)
                        assert jac_ref.dtype == T
                        first = omega == 1.0   # the residual and the red-black sweep do not depend on omega
                        if first:
                            r_ref, rb_ref = P.residual(u, b, l), P.rbgs(u, b, l)
                            assert r_ref.dtype == T and rb_ref.dtype == T
                        march = is_march(dim, shape, T)
                        for form in ((0, 1) if march else (0,)):
                            s.fas_set_form(form)
                            forms_seen[l].add("march" if march and form == 0 else "plain")
                            tag = (l, sigma, omega, gamma, form)
                            s.set_array(RHS, l, b)
                            if first:
                                s.set_array(E, l, u); s.set_array(TMP, l, other)   # RES exists on level 0 only
                                ss = s.fas_residual(l, E, RHS, TMP)
                                got = s.get_array(TMP, l)
                                assert np.array_equal(got, r_ref), (tag, int((got != r_ref).sum()))
                                assert ss == pytest.approx(sumsq(r_ref), rel=1e-13) and s.fas_residual(l, E, RHS, -1) == ss
                                assert np.array_equal(s.get_array(E, l), u) and np.array_equal(s.get_array(RHS, l), b)
                                s.set_array(U, l, u)
                                s.fas_smooth(l, RB, 1, U, RHS)
                                got = s.get_array(U, l)
                                assert np.array_equal(got, rb_ref), (tag, int((got != rb_ref).sum()))
                            s.set_array(U, l, u)
                            s.fas_smooth(l, JAC, 1, U, RHS)
                            got = s.get_array(U, l)
                            assert np.array_equal(got, jac_ref), (tag, int((got != jac_ref).sum()))
                            assert np.array_equal(s.get_array(RHS, l), b)
                        s.fas_set_form(0)
    assert forms_seen == {l: tc.want_forms(case, l, np.dtype(T).itemsize) for l in check}   # per level: a semi level is no cube


# ---------------------------------------------------------------- 2. gamma = 0 is the existing entry points
@DTYPES
@pytest.mark.parametrize("kind", [CUBIC, EXP], ids=["cubic", "exp"])
@pytest.mark.parametrize("case", [(3, 17, 2, {}), (3, 35, 2, {}), (3, 65, 2, {}), (2, 130, 1, {}), tc.A65, tc.SA65], ids=case_id)
def test_gamma_zero_equals_the_existing_entry_points(case, kind, dtype):
    """mg_fas_residual / mg_fas_smooth with gamma = 0 against mg_residual / mg_smooth on the same random arrays, bit for bit, with
    and without a shift: num = b - s, den = cd, and the IEEE quotient is div_cd's. a65 and sa65 pin the tile to
    mg_jacobi_fast.hip's kernels on an operator with distinct axis coefficients (sa65: on a 33 x 33 x 65 level too)"""
    dim, n, levels, extra = case
    T = NP[dtype]
    kw = desc_kw(dim, n, levels, extra, dtype, omega=6.0 / 7.0)
    rng = np.random.default_rng(n)
    with capi.Solver(capi.make_desc(**kw)) as s:
        assert s.fas_get_reaction() == (CUBIC, 0.0)
        s.fas_set_reaction(kind, 0.0)
        for sigma in (0.0, 500.0):
            s.set_shift(sigma)
            for l in range(levels):
                shape = s.level_shape(l)
                u, b = (rng.standard_normal(shape).astype(T) for _ in range(2))
                s.set_array(E, l, u); s.set_array(RHS, l, b)
                n_const = s.residual(l, E, RHS, TMP); r_const = s.get_array(TMP, l)
                for form in ((0, 1) if is_march(dim, shape, T) else (0,)):
                    s.fas_set_form(form)
                    s.zero_array(TMP, l)
                    n_fas = s.fas_residual(l, E, RHS, TMP)
                    assert np.array_equal(s.get_array(TMP, l), r_const), (l, sigma, form)
                    assert n_fas == pytest.approx(n_const, rel=1e-13)   # the same squares added in another order
                    for sm in (JAC, RB):
                        s.set_array(U, l, u); s.smooth(l, sm, 1, U, RHS); x_const = s.get_array(U, l)
                        s.set_array(U, l, u); s.fas_smooth(l, sm, 1, U, RHS); x_fas = s.get_array(U, l)
                        assert np.array_equal(x_fas, x_const), (l, sigma, sm, form)
                s.fas_set_form(0)


# ---------------------------------------------------------------- 3. the exp kind
@DTYPES
@pytest.mark.parametrize("case", [(3, 17, 2, {}), (3, 35, 2, {}), (3, 67, 2, {}), (2, 130, 1, {}), (3, 17, 2, {"aniso": (1.0, 30.0, 0.05)}),
                                  tc.A65, tc.SA65], ids=case_id)
def test_exp_kernels_within_8_eps(case, dtype):
    """the same launches with g = exp(u), u uniform in [-2, 2], within 8 eps_T x magnitude: |b| + |A||u| + |G||g| for the residual,
    (|b| + |A - D||u| + |G|(|g| + |gp u|)) / |den| for the point solves. The device's exp is specified to 1 ulp and the
    reference's is rounded once, so g differs by at most 1.5 ulp; every other operation is the same in the same order. a65 and
    sa65: the exp tile on distinct axis coefficients (an exchanged pair is an error of order 1, not of 8 eps) and on nz != nx."""
    dim, n, levels, extra = case
    T = NP[dtype]
    eps = float(np.finfo(T).eps)
    rng = np.random.default_rng(7 * n + dim)
    worst = {"residual": 0.0, "jacobi": 0.0, "rb": 0.0}
    for omega in (1.0, 6.0 / 7.0):
        kw = desc_kw(dim, n, levels, extra, dtype, omega=omega)
        with capi.Solver(capi.make_desc(**kw)) as s:
            for sigma, gamma in ((0.0, 0.7), (500.0, -0.3)):
                s.set_shift(sigma); s.fas_set_reaction(EXP, gamma)
                P = problem_of(s, kw, T, fr.EXP, gamma, sigma)
                for l in range(min(levels, 2)):
                    shape = s.level_shape(l)
                    u = rng.uniform(-2.0, 2.0, shape).astype(T)
                    b = rng.standard_normal(shape).astype(T)
                    mag_r, mag_ps = P.residual_mag(u, b, l).astype(np.float64), P.point_solve_mag(u, b, l).astype(np.float64)
                    for form in ((0, 1) if is_march(dim, shape, T) else (0,)):
                        s.fas_set_form(form)
                        s.set_array(RHS, l, b)
                        if omega == 1.0:
                            s.set_array(E, l, u)
                            s.fas_residual(l, E, RHS, TMP)
                            d = abs(s.get_array(TMP, l).astype(np.float64) - P.residual(u, b, l).astype(np.float64)) / mag_r
                            worst["residual"] = max(worst["residual"], float(d.max()) / eps)
                            s.set_array(U, l, u); s.fas_smooth(l, RB, 1, U, RHS)
                            d = abs(s.get_array(U, l).astype(np.float64) - P.rbgs(u, b, l).astype(np.float64)) / mag_ps
                            worst["rb"] = max(worst["rb"], float(d.max()) / eps)
                        s.set_array(U, l, u); s.fas_smooth(l, JAC, 1, U, RHS)
                        d = abs(s.get_array(U, l).astype(np.float64) - P.jacobi(u, b, l).astype(np.float64)) / mag_ps
                        worst["jacobi"] = max(worst["jacobi"], float(d.max()) / eps)
                    s.fas_set_form(0)
    print(f"{case_id(case)} {T.__name__}: largest error in units of eps x magnitude: {worst}")
    assert max(worst.values()) <= 8.0


# ---------------------------------------------------------------- 4. the FAS transition and the correction, bit for bit
TRANSITIONS = [(3, 17, 2, {}), (3, 17, 3, {"semi_xy": 1}), (2, 17, 2, {}), (3, 35, 2, {})]


@DTYPES
@pytest.mark.parametrize("restriction", [FULLW, INJECT], ids=["fullw", "inject"])
@pytest.mark.parametrize("case", TRANSITIONS, ids=case_id)
def test_coarse_rhs_and_correct_bit_for_bit(case, restriction, dtype):
    """mg_fas_coarse_rhs: U, E and RHS of level 1 from U and TMP of level 0; mg_fas_correct: E(1) = U(1) - E(1), U(0) += P E(1).
    Every other array is unchanged."""
    dim, n, levels, extra = case
    T = NP[dtype]
    kw = desc_kw(dim, n, levels, extra, dtype, restriction=restriction)
    rng = np.random.default_rng(n + dim)
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_shift(500.0); s.fas_set_reaction(CUBIC, 0.7)
        P = problem_of(s, kw, T, fr.CUBIC, 0.7, 500.0)
        fs, cs = s.level_shape(0), s.level_shape(1)
        fine = {a: rng.standard_normal(fs).astype(T) for a in (U, E, RHS, TMP, RES)}
        coarse = {a: rng.standard_normal(cs).astype(T) for a in (U, E, RHS, TMP)}
        for a, v in fine.items():
            s.set_array(a, 0, v)
        for a, v in coarse.items():
            s.set_array(a, 1, v)
        uc0, rhs = P.coarse_rhs(fine[U], fine[TMP], 0)
        assert uc0.dtype == T and rhs.dtype == T
        s.fas_coarse_rhs(0)
        assert np.array_equal(s.get_array(U, 1), uc0) and np.array_equal(s.get_array(E, 1), uc0)
        got = s.get_array(RHS, 1)
        assert np.array_equal(got, rhs), int((got != rhs).sum())
        for a, v in fine.items():
            assert np.array_equal(s.get_array(a, 0), v), a
        assert np.array_equal(s.get_array(TMP, 1), coarse[TMP])
        # the correction: a coarse iterate that differs from the kept copy at the unknowns only, as after any coarse solve
        uc = uc0.copy()
        I = (slice(1, -1),) * len(cs)
        uc[I] = rng.standard_normal(uc[I].shape).astype(T)
        s.set_array(U, 1, uc)
        s.fas_correct(0)
        assert np.array_equal(s.get_array(E, 1), uc - uc0)
        got, want = s.get_array(U, 0), P.correct(fine[U], uc, uc0, 0)
        assert want.dtype == T and np.array_equal(got, want), int((got != want).sum())
        for a in (E, RHS, TMP, RES):
            assert np.array_equal(s.get_array(a, 0), fine[a]), a
        assert np.array_equal(s.get_array(U, 1), uc) and np.array_equal(s.get_array(RHS, 1), rhs)
        assert np.array_equal(s.get_array(TMP, 1), coarse[TMP])


# ---------------------------------------------------------------- 5. the coarse solve
@DTYPES
@pytest.mark.parametrize("smoother,omega", [(JAC, 6.0 / 7.0), (JAC, 1.0), (RB, 1.0)], ids=["jacobi67", "jacobi1", "rb"])
@pytest.mark.parametrize("dim,n", [(3, 9), (2, 17)])
def test_coarse_solve_fixed_bit_for_bit(dim, n, smoother, omega, dtype):
    """MG_COARSE_FIXED, cubic: 7 sweeps (odd: the Jacobi result is moved back) against coarse_loop in the working dtype"""
    T = NP[dtype]
    kw = desc_kw(dim, n, 1, {}, dtype, smoother=smoother, omega=omega, coarse_maxit=7)
    rng = np.random.default_rng(n)
    with capi.Solver(capi.make_desc(**kw)) as s:
        shape = s.level_shape(0)
        for gamma, sigma in ((0.7, 0.0), (-0.3, 10.0)):
            s.set_shift(sigma); s.fas_set_reaction(CUBIC, gamma)
            P = problem_of(s, kw, T, fr.CUBIC, gamma, sigma)
            u, b = (rng.standard_normal(shape).astype(T) for _ in range(2))
            ref, iters, flag, relres, _ = P.coarse_loop(u, b, 0, 7, 0.0, True)
            s.set_array(U, 0, u); s.set_array(RHS, 0, b)
            st = s.fas_coarse_solve(0, U, RHS)
            assert np.array_equal(s.get_array(U, 0), ref) and np.array_equal(s.get_array(RHS, 0), b)
            assert (st.coarse_iters, st.coarse_flag) == (7, 0) and st.coarse_relres == pytest.approx(relres, rel=1e-12)


@DTYPES
@pytest.mark.parametrize("smoother,omega", [(JAC, 6.0 / 7.0), (RB, 1.0)], ids=["jacobi67", "rb"])
@pytest.mark.parametrize("dim,n", [(3, 9), (2, 17)])
def test_coarse_solve_to_tolerance(dim, n, smoother, omega, dtype):
    """MG_COARSE_TOL, cubic: the reference runs in the working dtype, so its sweeps are the kernel's bit for bit and only the order
    in which the squares of the residual are added differs. No stopping decision of the reference is closer than 1e-6 to a
    tie (asserted), so that difference cannot move the stop: the sweep count and the flag are equal."""
    T = NP[dtype]
    tol = 3e-3
    rng = np.random.default_rng(n + 1)
    for maxit in (2000, 5):   # converges / runs out of sweeps
        kw = desc_kw(dim, n, 1, {}, dtype, smoother=smoother, omega=omega, coarse_mode=capi.COARSE_TOL, coarse_maxit=maxit, coarse_tol=tol)
        with capi.Solver(capi.make_desc(**kw)) as s:
            shape = s.level_shape(0)
            for sigma in (0.0, 10.0):
                s.set_shift(sigma); s.fas_set_reaction(CUBIC, 0.7)
                P = problem_of(s, kw, T, fr.CUBIC, 0.7, sigma)
                b = rng.standard_normal(shape).astype(T)
                ref, iters, flag, relres, tested = P.coarse_loop(np.zeros(shape, T), b, 0, maxit, tol, False)
                assert min(abs(t / tol - 1.0) for t in tested) > 1e-6
                s.zero_array(U, 0); s.set_array(RHS, 0, b)
                st = s.fas_coarse_solve(0, U, RHS)
                print(f"sigma {sigma} maxit {maxit}: gpu {st.coarse_iters} sweeps flag {st.coarse_flag}, reference {iters} flag {flag}")
                assert st.coarse_iters == iters and st.coarse_flag == flag
                assert st.coarse_relres == pytest.approx(relres, rel=1e-12)
                assert np.array_equal(s.get_array(U, 0), ref) and np.array_equal(s.get_array(RHS, 0), b)


# ---------------------------------------------------------------- 6. one cycle of each kind
CYCLE_KINDS = {
    "v-rb": dict(cycle=capi.CYCLE_V, smoother=RB), "w-rb": dict(cycle=capi.CYCLE_W, smoother=RB), "f-rb": dict(cycle=capi.CYCLE_F, smoother=RB),
    "v-jacobi": dict(cycle=capi.CYCLE_V, smoother=JAC, omega=6.0 / 7.0), "w-jacobi": dict(cycle=capi.CYCLE_W, smoother=JAC, omega=6.0 / 7.0),
    "f-jacobi": dict(cycle=capi.CYCLE_F, smoother=JAC, omega=6.0 / 7.0),
}
CYCLE_REACTIONS = {"cubic": (CUBIC, 50.0, 0.0), "exp": (EXP, 20.0, 10.0)}   # kind, gamma, sigma: gamma g' > 0 on standard-normal data


# (n, levels, extra) x kind x reaction; sa65 (tests/tile_cases.py): a V(2,2) cycle whose Jacobi sweeps and residuals go through
# the tile inside the driver's dispatch on 65^3 and on 33 x 33 x 65, both with pairwise distinct axis coefficients
CYCLE_GRIDS = {"17-3": (17, 3, {}), "35-2": (35, 2, {}), "sa65": tc.SA65[1:]}
CYCLE_PARAMS = [pytest.param(g, kind, r, id=f"{g}-{kind}-{r}") for g in ("17-3", "35-2") for kind in CYCLE_KINDS for r in CYCLE_REACTIONS]
CYCLE_PARAMS += [pytest.param("sa65", kind, "cubic", id=f"sa65-{kind}-cubic") for kind in ("v-rb", "v-jacobi")]


@functools.lru_cache(maxsize=None)
def cycle_inputs(n):
    """u0, b with float32 values: exact in both working dtypes, so the long-double reference is shared"""
    rng = np.random.default_rng(n)
    return rng.standard_normal((n, n, n)).astype(np.float32), rng.standard_normal((n, n, n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cycle_reference(grid, kind, reaction, prec, coefs):
    """coefs: mg_level_coefficients of every level (doubles, shift included) -- the contract casts THOSE to T"""
    rk, gamma, sigma = CYCLE_REACTIONS[reaction]
    n, levels, extra = CYCLE_GRIDS[grid]
    kw = desc_kw(3, n, levels, extra, capi.MG_F64, **CYCLE_KINDS[kind])
    u0, b = cycle_inputs(n)
    P = fr.FASProblem(kind=rk, gamma=gamma, sigma=sigma, prec=prec, **{k: v for k, v in kw.items() if k != "dtype"})
    P.use_handle_coefs(coefs)
    return P.vcycle(P.as_prec(u0), P.as_prec(b), kw["coarse_maxit"])


@DTYPES
@pytest.mark.parametrize("grid,kind,reaction", CYCLE_PARAMS)
def test_one_cycle_against_long_double(grid, kind, reaction, dtype):
    """mg_fas_cycle (V, W, F; red-black and Jacobi 6/7, V(2,2), 6 coarse sweeps) against the long-double reference cycle on the
    handle's level coefficients. The GPU's distance to it may be at most 4 x the distance of fas_ref run in the working dtype:
    both round the same arithmetic; the factor covers summation-order differences in the prolongation and the norms. sa65 (V
    red-black and V Jacobi, cubic): the tile on distinct axis coefficients and on nz != nx inside the driver. fas_ref's
    distance on sa65, from the reference alone on the CPU (max |u| = 4.5): V red-black fp64 4.3e-16, fp32 3.0e-07; V Jacobi fp64
    3.5e-16, fp32 2.3e-07 -- about half an eps_T x max |u|: the rule stays about rounding on this hierarchy."""
    T = NP[dtype]
    rk, gamma, sigma = CYCLE_REACTIONS[reaction]
    n, levels, extra = CYCLE_GRIDS[grid]
    u0, b = (a.astype(T) for a in cycle_inputs(n))
    kw = desc_kw(3, n, levels, extra, dtype, **CYCLE_KINDS[kind])
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_shift(sigma); s.fas_set_reaction(rk, gamma); s.set_solution(u0); s.set_rhs(b)
        coefs = tuple(s.level_coefficients(l) for l in range(levels))
        u_T, u_LD = cycle_reference(grid, kind, reaction, T, coefs), cycle_reference(grid, kind, reaction, LD, coefs)
        tol = 4 * float(abs(u_T.astype(LD) - u_LD).max())
        st = s.fas_cycle()
        got = s.get_solution().astype(LD)
        err = float(abs(got - u_LD).max())
        print(f"{grid} {kind} {reaction} {T.__name__}: |gpu - ld| = {err:.3e}, |fas_ref in T - ld| = {tol / 4:.3e}")
        assert err <= tol
        assert np.array_equal(s.get_array(RHS, 0), b)
        visits = {capi.CYCLE_V: 1, capi.CYCLE_W: 2 ** (levels - 2), capi.CYCLE_F: levels - 1}[kw["cycle"]]
        assert st.coarse_iters == visits * kw["coarse_maxit"] and st.coarse_flag == 0


@DTYPES
@pytest.mark.parametrize("smoother,omega", [(JAC, 6.0 / 7.0), (RB, 1.0)], ids=["jacobi67", "rb"])
def test_big_coarsest_level_is_smoothed_chip_wide(smoother, omega, dtype):
    """n = 65 on 2 levels: the coarsest level has 33^3 = 35937 > 32768 nodes, too many for the one-workgroup coarse kernel, so
    with MG_COARSE_FIXED the cycle runs coarse_maxit chip-wide sweeps there. One mg_fas_cycle (cubic, gamma = 1) equals, bit for
    bit, the same steps made through the public entry points on a second handle; the statistics report the fixed sweeps."""
    T = NP[dtype]
    kw = desc_kw(3, 65, 2, {}, dtype, smoother=smoother, omega=omega, coarse_maxit=3)
    rng = np.random.default_rng(65)
    with capi.Solver(capi.make_desc(**kw)) as s, capi.Solver(capi.make_desc(**kw)) as m:
        shape = s.level_shape(0)
        assert int(np.prod(s.level_shape(1))) == 33 ** 3 > 32768
        u0, b = rng.standard_normal(shape).astype(T), rng.standard_normal(shape).astype(T)
        for h in (s, m):
            h.fas_set_reaction(CUBIC, 1.0); h.set_solution(u0); h.set_rhs(b)
        st = s.fas_cycle()
        m.fas_smooth(0, smoother, kw["nu_pre"], U, RHS)
        m.fas_residual(0, U, RHS, TMP)
        m.fas_coarse_rhs(0)
        m.fas_smooth(1, smoother, kw["coarse_maxit"], U, RHS)
        m.fas_correct(0)
        m.fas_smooth(0, smoother, kw["nu_post"], U, RHS)
        got, want = s.get_solution(), m.get_solution()
        assert np.isfinite(want).all() and not np.array_equal(want, u0)
        assert np.array_equal(got, want), int((got != want).sum())
        for arr in (U, E, RHS):
            assert np.array_equal(s.get_array(arr, 1), m.get_array(arr, 1)), arr
        assert np.array_equal(s.get_array(RHS, 0), b)
        assert (st.coarse_iters, st.coarse_flag) == (3, 0)


# ---------------------------------------------------------------- 7. the solves (n = 33, 4 levels, red-black V(2,2), FULLW, 50 coarse sweeps)
ROWS = {   # the rows of DESIGN.md section 20 the GPU runs: kind, gamma, the size of the noise (None: b = 0)
    "cubic-noise": (fr.CUBIC, 1e3, 1e3),
    "bratu": (fr.EXP, -5.0, None),
}


def table_desc(dtype, n=33, levels=4):
    return dict(dim=3, n=n, levels=levels, length=1.0, alpha=1.0, dtype=dtype, cycle=capi.CYCLE_V, smoother=RB, nu_pre=2, nu_post=2,
                restriction=FULLW, outer_pre_gs=0, coarse_mode=capi.COARSE_FIXED, coarse_maxit=fr.TABLE_COARSE_SWEEPS)


def row_rhs(name):
    _, _, size = ROWS[name]
    return np.zeros((33,) * 3) if size is None else fr.noise((33,) * 3, size)


@functools.lru_cache(maxsize=None)
def row_reference(name, prec, cycles):
    kind, gamma, _ = ROWS[name]
    P = fr.table_problem(kind, gamma, prec=prec)
    b = row_rhs(name).astype(prec)
    _, hist, status = P.solve_history(np.zeros_like(b), b, cycles, fr.TABLE_COARSE_SWEEPS)
    return hist, status


@pytest.mark.parametrize("name", list(ROWS))
def test_solve_history_follows_the_reference(name):
    """fp64, 20 cycles with no tolerance: the factors of cycles 6 .. 10 match fas_ref's to 5 %, and the entries match to 1e-6
    relative while they are above 1e3 x the floor the float64 reference itself reaches"""
    ref, _ = row_reference(name, np.float64, 20)
    floor = float(ref.min())
    kind, gamma, _ = ROWS[name]
    b = row_rhs(name)
    with capi.Solver(capi.make_desc(**table_desc(capi.MG_F64))) as s:
        s.fas_set_reaction(kind, gamma); s.set_rhs(b); s.set_solution(np.zeros_like(b))
        hist, st = s.fas_solve(0.0, 0.0, 20)
        print("gpu", hist, "reference", ref)
        assert len(hist) == 21 and st.status == 1 and st.cycles == 20 and st.norm0 == hist[0] and st.norm == hist[-1]
        assert fr.factors(hist)[5:10] == pytest.approx(fr.factors(ref)[5:10], rel=0.05)
        above = ref > 1e3 * floor
        assert above.sum() >= 8 and hist[above] == pytest.approx(ref[above], rel=1e-6)
        assert np.array_equal(s.get_array(RHS, 0), b)


@pytest.mark.parametrize("name", list(ROWS))
def test_fp32_reaches_the_reference_floor(name):
    """fp32: the same solve stalls at a floor; the GPU gets within 10 x the floor fas_ref reaches in float32 (computed here)"""
    ref, _ = row_reference(name, np.float32, 14)
    floor = float(ref.min())
    kind, gamma, _ = ROWS[name]
    b = row_rhs(name).astype(np.float32)
    with capi.Solver(capi.make_desc(**table_desc(capi.MG_F32))) as s:
        s.fas_set_reaction(kind, gamma); s.set_rhs(b); s.set_solution(np.zeros_like(b))
        hist, st = s.fas_solve(0.0, 0.0, 14)
        print(f"{name}: float32 floor of the reference {floor:.3e}, gpu {hist.min():.3e}")
        assert len(hist) == 15 and st.status == 1 and hist.min() <= 10 * floor


def test_status_and_n_hist():
    """the stops: rtol, atol, maxit; b = 0 with u = 0 for the cubic (hist[0] = 0, status 0, no cycle); a far start (status 2)"""
    b = row_rhs("cubic-noise")
    ref, _ = row_reference("cubic-noise", np.float64, 20)
    with capi.Solver(capi.make_desc(**table_desc(capi.MG_F64))) as s:
        s.fas_set_reaction(CUBIC, 1e3)

        def solve(rtol, atol, maxit, rhs=b):
            s.set_rhs(rhs); s.set_solution(np.zeros_like(rhs))
            return s.fas_solve(rtol, atol, maxit)
        k = int(np.argmax(ref <= 1e-4 * ref[0]))   # the reference's first entry below rtol; not a tie (the rate is 0.25)
        assert k > 0 and abs(ref[k] / (1e-4 * ref[0]) - 1) > 1e-3 and abs(ref[k - 1] / (1e-4 * ref[0]) - 1) > 1e-3
        hist, st = solve(1e-4, 0.0, 20)
        assert (len(hist), st.status, st.cycles) == (k + 1, 0, k) and hist[-1] <= 1e-4 * hist[0] < hist[-2]
        atol = 1e-4 * ref[0]
        hist, st = solve(0.0, atol, 20)
        assert (len(hist), st.status, st.cycles) == (k + 1, 0, k) and hist[-1] <= atol < hist[-2]
        hist, st = solve(1e-4, 0.0, 3)
        assert (len(hist), st.status, st.cycles) == (4, 1, 3)
        hist, st = solve(1e-4, 0.0, 0)
        assert (len(hist), st.status, st.cycles) == (1, 1, 0) and hist[0] == pytest.approx(ref[0], rel=1e-12)
        hist, st = solve(0.0, 0.0, 5, np.zeros_like(b))
        assert (len(hist), st.status, st.cycles) == (1, 0, 0) and hist[0] == 0.0
        assert not s.get_solution().any()
        # FAS converges locally: noise of size 1e5 from u = 0 overflows (ordinary floating-point overflow) by cycle 3
        far = fr.noise((33,) * 3, 1e5)
        P = fr.table_problem(fr.CUBIC, 1e3)
        _, ref_far, status = P.solve_history(np.zeros_like(far), far, 6, fr.TABLE_COARSE_SWEEPS)
        assert status == 2 and len(ref_far) <= 4
        hist, st = solve(1e-8, 0.0, 6, far)
        print("far start: gpu", hist, "reference", ref_far)
        assert st.status == 2 and len(hist) <= 4 and not np.isfinite(hist[-1]) and np.isfinite(hist[:-1]).all()
        assert st.cycles == len(hist) - 1


@functools.lru_cache(maxsize=None)
def manufactured_reference(n, kind, gamma):
    f, u = fr.manufactured(n, kind, gamma)
    P = fr.table_problem(kind, gamma, n=n, levels=fr.levels_for(n))
    x, _, status = P.solve_history(np.zeros_like(f), f, 30, fr.TABLE_COARSE_SWEEPS, rtol=1e-12)
    assert status == 0
    return float(abs(x - u).max())


@pytest.mark.parametrize("kind,gamma", [(fr.CUBIC, 1e3), (fr.EXP, -5.0)], ids=["cubic", "exp"])
def test_manufactured_errors_match_the_reference(kind, gamma):
    """u = sin(pi x) sin(pi y) sin(pi z) at n = 17 and 33, solved to rtol 1e-12: the max errors are within 1 % of fas_ref's"""
    for n in (17, 33):
        f, u = fr.manufactured(n, kind, gamma)
        with capi.Solver(capi.make_desc(**table_desc(capi.MG_F64, n, fr.levels_for(n)))) as s:
            s.fas_set_reaction(kind, gamma); s.set_rhs(f); s.set_solution(np.zeros_like(f))
            hist, st = s.fas_solve(1e-12, 0.0, 30)
            err = float(abs(s.get_solution() - u).max())
            want = manufactured_reference(n, kind, gamma)
            print(f"n={n}: gpu {err:.4e}, reference {want:.4e}, {len(hist) - 1} cycles")
            assert st.status == 0 and err == pytest.approx(want, rel=0.01)


# ---------------------------------------------------------------- 8. contracts
def refused(call, word):
    with pytest.raises(capi.MgError) as e:
        call()
    assert e.value.code == -4 and word in str(e.value), str(e.value)


def test_refusals_change_nothing():
    rng = np.random.default_rng(5)
    base = desc_kw(3, 17, 3, {}, capi.MG_F64)

    def drivers(s):
        return [lambda: s.fas_cycle(), lambda: s.fas_solve(1e-8, 0.0, 3)]

    def snapshot(s):
        return [s.get_array(a, l) for l in range(3) for a in (U, E, RHS, TMP)] + [s.get_array(RES, 0)]

    def same(x, y):
        return all(np.array_equal(p, q) for p, q in zip(x, y))

    with capi.Solver(capi.make_desc(**base)) as s:
        for l in range(3):
            for a in (U, E, RHS, TMP):
                s.set_array(a, l, rng.standard_normal(s.level_shape(l)))
        s.fas_set_reaction(EXP, 0.25)
        before, nbytes = snapshot(s), s.device_bytes()
        nan, inf = float("nan"), float("inf")
        for call in (lambda: s.fas_set_reaction(2, 1.0), lambda: s.fas_set_reaction(-1, 1.0), lambda: s.fas_set_reaction(CUBIC, nan),
                     lambda: s.fas_set_reaction(CUBIC, inf), lambda: s.fas_set_reaction(EXP, -inf),
                     lambda: s.fas_residual(3, U, RHS, TMP), lambda: s.fas_residual(0, U, RHS, U), lambda: s.fas_residual(0, U, RHS, RHS),
                     lambda: s.fas_residual(0, 7, RHS, RES), lambda: s.fas_residual(1, U, RHS, RES),
                     lambda: s.fas_smooth(0, JAC, 1, U, U), lambda: s.fas_smooth(0, JAC, 1, TMP, RHS), lambda: s.fas_smooth(0, RB, 1, U, TMP),
                     lambda: s.fas_smooth(-1, RB, 1, U, RHS), lambda: s.fas_smooth(0, RB, -1, U, RHS),
                     lambda: s.fas_smooth(0, capi.SMOOTH_GS_LEX, 1, U, RHS), lambda: s.fas_smooth(0, capi.SMOOTH_ZEBRA_X, 1, U, RHS),
                     lambda: s.fas_smooth(0, 99, 1, U, RHS), lambda: s.fas_coarse_solve(2, U, TMP), lambda: s.fas_coarse_solve(2, U, U),
                     lambda: s.fas_coarse_solve(5, U, RHS), lambda: s.fas_coarse_rhs(2), lambda: s.fas_coarse_rhs(-1),
                     lambda: s.fas_correct(2), lambda: s.fas_correct(-1), lambda: s.fas_set_form(2),
                     lambda: s.fas_solve(-1e-3, 0.0, 3), lambda: s.fas_solve(0.0, -1.0, 3), lambda: s.fas_solve(nan, 0.0, 3),
                     lambda: s.fas_solve(0.0, inf, 3), lambda: s.fas_solve(1e-8, 0.0, -1)):
            with pytest.raises(capi.MgError) as e:
                call()
            assert e.value.code == -4
        # a stage callback
        s.set_stage_callback(lambda *a: None)
        for call in drivers(s):
            refused(call, "stage callback")
        s.set_stage_callback(None)
        assert s.fas_get_reaction() == (EXP, 0.25) and same(snapshot(s), before) and s.device_bytes() == nbytes
    # a sawtooth handle; a smoother the fas kernels do not have
    for more, word, extra_calls in ((dict(cycle=capi.CYCLE_SAWTOOTH), "sawtooth", 0), (dict(smoother=capi.SMOOTH_GS_LEX), "smoother", 1),
                                    (dict(smoother=capi.SMOOTH_ZEBRA_Y), "smoother", 1)):
        with capi.Solver(capi.make_desc(**dict(base, **more))) as s:
            u0 = rng.standard_normal(s.level_shape(0)); s.set_solution(u0); s.set_rhs(u0)
            s.fas_set_reaction(CUBIC, 2.0)
            for call in drivers(s) + [lambda: s.fas_coarse_solve(2, U, RHS)] * extra_calls:
                refused(call, word)
            assert np.array_equal(s.get_solution(), u0) and s.fas_get_reaction() == (CUBIC, 2.0)
    # distributed handles, the dry-run measurement handle included
    with capi.Solver(capi.make_desc(**base), device=0, rank=0, nranks=2, dry=True) as s:
        u0 = rng.standard_normal(s.level_shape(0)); s.set_solution(u0)
        before = s.device_bytes()
        for call in drivers(s) + [lambda: s.fas_set_reaction(EXP, 1.0), lambda: s.fas_residual(0, U, RHS, RES), lambda: s.fas_smooth(0, RB, 1, U, RHS),
                                  lambda: s.fas_coarse_rhs(0), lambda: s.fas_correct(0), lambda: s.fas_coarse_solve(2, U, RHS)]:
            refused(call, "distributed")
        assert np.array_equal(s.get_solution(), u0) and s.device_bytes() == before and s.fas_get_reaction() == (CUBIC, 0.0)
    # NULL handle
    L = capi.load()
    assert L.mg_fas_cycle(None, None) == -4 and L.mg_fas_set_reaction(None, 0, 0.0) == -4 and L.mg_fas_get_reaction(None, None, None) == -4
    assert L.mg_fas_solve(None, 0.0, 0.0, 1, None, 0, None, None) == -4 and L.mg_fas_coarse_rhs(None, 0) == -4
    assert L.mg_fas_correct(None, 0) == -4 and L.mg_fas_set_form(None, 0) == -4 and L.mg_fas_residual(None, 0, 0, 2, -1, None) == -4
    assert L.mg_fas_smooth(None, 0, 1, 1, 0, 2) == -4 and L.mg_fas_coarse_solve(None, 0, 0, 2, None) == -4


@DTYPES
def test_memory_determinism_and_isolation(dtype):
    T = NP[dtype]
    kw = desc_kw(3, 33, 4, {}, dtype, smoother=JAC, omega=6.0 / 7.0)
    rng = np.random.default_rng(8)
    with capi.Solver(capi.make_desc(**kw)) as s, capi.Solver(capi.make_desc(**kw)) as fresh:
        shape = s.level_shape(0)
        b = rng.standard_normal(shape).astype(T)
        before = s.device_bytes()
        assert before == fresh.device_bytes()
        runs = []
        for k in range(2):
            out = []
            for kind, gamma in ((CUBIC, 50.0), (EXP, 20.0)):
                s.fas_set_reaction(kind, gamma)
                s.set_rhs(b); s.set_solution(np.zeros_like(b))
                hist, _ = s.fas_solve(0.0, 0.0, 3)
                out += [hist, s.get_solution(), s.get_array(RHS, 0)]
                s.set_array(E, 0, b); s.fas_residual(0, E, RHS, RES); s.fas_smooth(0, RB, 1, E, RHS); s.fas_residual(0, U, RHS, TMP)
                s.fas_coarse_rhs(0); s.fas_correct(0); s.fas_coarse_solve(3, U, RHS); s.fas_cycle()
                out.append(s.get_solution())
                assert s.device_bytes() == before   # no mg_fas_* call allocates
            runs.append(out)
        for x, y in zip(*runs):
            assert np.array_equal(x, y)   # two runs give the same bits
        # a handle that ran mg_fas_solve gives mg_cycle / mg_solve results bit-identical to a fresh handle
        outs = []
        for h in (fresh, s):
            h.set_rhs(b); h.set_solution(np.zeros_like(b))
            h.cycle(); u1 = h.get_solution()
            hist, _ = h.solve(0.0, 2)
            outs.append((u1, hist, h.get_solution()))
        for x, y in zip(*outs):
            assert np.array_equal(x, y)
        assert s.device_bytes() == fresh.device_bytes() == before
