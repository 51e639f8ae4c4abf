"""Neumann faces on the GPU (mg_bc_*, multigrid_prj_amd/csrc/mg_bc.hip) against tests/bc_ref.py: the kernels bit for bit
(plain form and marching tile, the mirrored restriction included), mask 0 against the existing entry points bit for bit, the
coarse solve, one cycle of each kind against the long-double reference, convergence on the settings of DESIGN.md section 19
(the singular all-Neumann case included), a manufactured solution with an inhomogeneous flux, and the contracts of the C ABI."""
import functools

import numpy as np
import pytest

from multigrid_prj_amd import capi
from tests import npref
from tests import bc_ref as br
from tests import tile_cases as tc

pytestmark = pytest.mark.gpu

NP = {capi.MG_F64: np.float64, capi.MG_F32: np.float32}
DTYPES = pytest.mark.parametrize("dtype", [capi.MG_F64, capi.MG_F32], ids=["f64", "f32"])
U, E, RHS, TMP, RES = capi.ARR_U, capi.ARR_E, capi.ARR_RHS, capi.ARR_TMP, capi.ARR_RES
JAC, RB = capi.SMOOTH_JACOBI, capi.SMOOTH_RBGS
INJECT, FULLW = capi.RESTRICT_INJECT, capi.RESTRICT_FULLW
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


def mixed(dim):
    """Neumann faces that meet Dirichlet ones along edges: x-hi, y-hi, z-lo (2-D: x-hi, y-hi)"""
    return 0b011010 if dim == 3 else 0b1010


def desc_kw(dim, n, levels, extra, dtype, **more):
    kw = dict(dim=dim, n=n, levels=levels, length=1.0, alpha=1.3, dtype=dtype, cycle=capi.CYCLE_V, smoother=RB, nu_pre=2, nu_post=2,
              restriction=FULLW, outer_pre_gs=0, coarse_mode=capi.COARSE_FIXED, coarse_maxit=6)
    kw.update(extra); kw.update(more)
    return kw


def problem_of(s, kw, prec, mask, sigma=0.0):
    """the reference of a handle's descriptor in `prec`, with the handle's own level coefficients (shift included)"""
    P = br.BCProblem(mask=mask, sigma=sigma, prec=prec, **{k: v for k, v in kw.items() if k != "dtype"})
    P.use_handle_coefs([s.level_coefficients(l) for l in range(kw["levels"])])
    return P


def sumsq(r):
    return npref.fsum_sq(r)


# ---------------------------------------------------------------- 1. the kernels, bit for bit
@DTYPES
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernels_bit_for_bit(case, dtype):
    """residual (saved and norm only), one Jacobi sweep (omega 1 and 6/7), one red-black sweep and mg_bc_restrict (both kinds) on
    the case's levels to check (0 and 1; s129: 1), sigma 0 and 500, masks 0 / all faces / mixed (n = 9: every single face too);
    where the marching tile takes the level the plain form is run too (mg_bc_set_form) against the same numbers. The inputs come
    back unmodified. The tile on distinct axis coefficients: a33, a65, sa65; on nz != nx: sa65, s67 (an even row), s129 (fp32)."""
    dim, n, levels, extra = case
    T = NP[dtype]
    rng = np.random.default_rng(100 * dim + n)
    masks = [0, br.all_faces(dim), mixed(dim)] + ([1 << k for k in range(2 * dim)] if n == 9 else [])
    check = tc.levels_to_check(case)
    forms_seen = {l: set() for l in check}
    for omega in (1.0, 6.0 / 7.0):
        kw = desc_kw(dim, n, levels, extra, dtype, omega=omega)
        with capi.Solver(capi.make_desc(**kw)) as s:
            for sigma in (0.0, 500.0):
                s.set_shift(sigma)
                for mask in masks:
                    s.bc_set_faces(mask)
                    assert s.bc_get_faces() == mask
                    P = problem_of(s, kw, T, mask, sigma)
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
                        march = dim == 3 and br.march_ok(3, shape[2], shape[1], shape[0], np.dtype(T).itemsize)
                        for form in ((0, 1) if march else (0,)):
                            s.bc_set_form(form)
                            forms_seen[l].add("march" if march and form == 0 else "plain")
                            tag = (l, sigma, omega, mask, form)
                            s.set_array(RHS, l, b)
                            if first:
                                s.set_array(E, l, u); s.set_array(TMP, l, other)   # RES exists on level 0 only
                                ss = s.bc_residual(l, E, RHS, TMP)
                                got = s.get_array(TMP, l)
                                assert np.array_equal(got, r_ref), (tag, int((got != r_ref).sum()))
                                assert ss == pytest.approx(sumsq(r_ref), rel=1e-13) and s.bc_residual(l, E, RHS, -1) == ss
                                assert np.array_equal(s.get_array(E, l), u) and np.array_equal(s.get_array(RHS, l), b)
                                s.set_array(U, l, u)
                                s.bc_smooth(l, RB, 1, U, RHS)
                                got = s.get_array(U, l)
                                assert np.array_equal(got, rb_ref), (tag, int((got != rb_ref).sum()))
                            s.set_array(U, l, u)
                            s.bc_smooth(l, JAC, 1, U, RHS)
                            got = s.get_array(U, l)
                            assert np.array_equal(got, jac_ref), (tag, int((got != jac_ref).sum()))
                            assert np.array_equal(s.get_array(RHS, l), b)
                        s.bc_set_form(0)
                        if first and sigma == 0.0 and l + 1 < levels:   # the restriction knows neither omega nor sigma
                            s.set_array(E, l, u)
                            for kind, ref in ((FULLW, P.restrict_fw(u, l)), (INJECT, P.inject(u, l))):
                                assert ref.dtype == T
                                s.set_array(TMP, l + 1, np.full(s.level_shape(l + 1), 7, T))
                                s.bc_restrict(l, kind, E, TMP)
                                got = s.get_array(TMP, l + 1)
                                assert np.array_equal(got, ref), (l, mask, kind, int((got != ref).sum()))
                            assert np.array_equal(s.get_array(E, l), u)
    assert forms_seen == {l: tc.want_forms(case, l, np.dtype(T).itemsize) for l in check}   # per level: a semi level is no cube


# ---------------------------------------------------------------- 2. mask 0 is the existing entry points
@DTYPES
@pytest.mark.parametrize("case", [(3, 17, 2, {}), (3, 35, 2, {}), (3, 65, 2, {}), (2, 130, 1, {}), tc.A65, tc.SA65], ids=case_id)
def test_mask_zero_equals_the_existing_entry_points(case, dtype):
    """mg_bc_residual / mg_bc_smooth / mg_bc_restrict(FULLW) with mask 0 against mg_residual / mg_smooth / mg_restrict(FULLW) on
    the same random arrays, bit for bit, with and without a shift. a65 and sa65 pin the tile to mg_jacobi_fast.hip's kernels on an
    operator with distinct axis coefficients (sa65: on a 33 x 33 x 65 level too)"""
    dim, n, levels, extra = case
    T = NP[dtype]
    kw = desc_kw(dim, n, levels, extra, dtype, omega=6.0 / 7.0)
    rng = np.random.default_rng(n)
    with capi.Solver(capi.make_desc(**kw)) as s:
        assert s.bc_get_faces() == 0
        for sigma in (0.0, 500.0):
            s.set_shift(sigma)
            for l in range(levels):
                shape = s.level_shape(l)
                u, b = (rng.standard_normal(shape).astype(T) for _ in range(2))
                s.set_array(E, l, u); s.set_array(RHS, l, b)
                n_const = s.residual(l, E, RHS, TMP); r_const = s.get_array(TMP, l)
                n_bc = s.bc_residual(l, E, RHS, TMP); r_bc = s.get_array(TMP, l)
                assert np.array_equal(r_bc, r_const), (l, sigma)
                assert n_bc == pytest.approx(n_const, rel=1e-13)   # the same squares added in another order
                for sm in (JAC, RB):
                    s.set_array(U, l, u); s.smooth(l, sm, 1, U, RHS); x_const = s.get_array(U, l)
                    s.set_array(U, l, u); s.bc_smooth(l, sm, 1, U, RHS); x_bc = s.get_array(U, l)
                    assert np.array_equal(x_bc, x_const), (l, sigma, sm)
                if l + 1 < levels:
                    s.restrict(l, FULLW, E, TMP); c_const = s.get_array(TMP, l + 1)
                    s.zero_array(TMP, l + 1)
                    s.bc_restrict(l, FULLW, E, TMP)
                    assert np.array_equal(s.get_array(TMP, l + 1), c_const), (l, sigma)


# ---------------------------------------------------------------- 3. the coarse solve
def coarse_settings(dim):
    """(mask, sigma): the mixed mask on the plain operator, all faces Neumann with a shift (not singular)"""
    return [(mixed(dim), 0.0), (br.all_faces(dim), 10.0)]


@DTYPES
@pytest.mark.parametrize("smoother,omega", [(JAC, 6.0 / 7.0), (JAC, 1.0), (RB, 1.0)], ids=["jacobi67", "jacobi1", "rb"])
@pytest.mark.parametrize("dim,n", [(3, 9), (2, 17)])
def test_coarse_solve_fixed_bit_for_bit(dim, n, smoother, omega, dtype):
    T = NP[dtype]
    kw = desc_kw(dim, n, 1, {}, dtype, smoother=smoother, omega=omega, coarse_maxit=7)   # odd: the Jacobi result is moved back
    rng = np.random.default_rng(n)
    with capi.Solver(capi.make_desc(**kw)) as s:
        shape = s.level_shape(0)
        for mask, sigma in coarse_settings(dim) + [(br.all_faces(dim), 0.0)]:
            s.set_shift(sigma); s.bc_set_faces(mask)
            P = problem_of(s, kw, T, mask, sigma)
            u, b = (rng.standard_normal(shape).astype(T) for _ in range(2))
            ref, iters, flag, relres, _ = P.coarse_loop(u, b, 0, 7, 0.0, True)
            s.set_array(U, 0, u); s.set_array(RHS, 0, b)
            st = s.bc_coarse_solve(0, U, RHS)
            assert np.array_equal(s.get_array(U, 0), ref) and np.array_equal(s.get_array(RHS, 0), b)
            assert (st.coarse_iters, st.coarse_flag) == (7, 0) and st.coarse_relres == pytest.approx(relres, rel=1e-12)


@DTYPES
@pytest.mark.parametrize("smoother,omega", [(JAC, 6.0 / 7.0), (RB, 1.0)], ids=["jacobi67", "rb"])
@pytest.mark.parametrize("dim,n", [(3, 9), (2, 17)])
def test_coarse_solve_to_tolerance(dim, n, smoother, omega, dtype):
    """MG_COARSE_TOL: the reference runs in the working dtype, so its sweeps are the kernel's bit for bit and only the order in
    which the squares of the residual are added differs (about 1e-16 relative). No stopping decision of the reference is
    closer than 1e-6 to a tie (asserted), so that difference cannot move the stop: the sweep count and the flag are equal."""
    T = NP[dtype]
    tol = 3e-3
    rng = np.random.default_rng(n + 1)
    for maxit in (2000, 5):   # converges / runs out of sweeps
        kw = desc_kw(dim, n, 1, {}, dtype, smoother=smoother, omega=omega, coarse_mode=capi.COARSE_TOL, coarse_maxit=maxit, coarse_tol=tol)
        with capi.Solver(capi.make_desc(**kw)) as s:
            shape = s.level_shape(0)
            for mask, sigma in coarse_settings(dim):
                s.set_shift(sigma); s.bc_set_faces(mask)
                P = problem_of(s, kw, T, mask, sigma)
                b = rng.standard_normal(shape).astype(T)
                ref, iters, flag, relres, tested = P.coarse_loop(np.zeros(shape, T), b, 0, maxit, tol, False)
                assert min(abs(t / tol - 1.0) for t in tested) > 1e-6
                s.zero_array(U, 0); s.set_array(RHS, 0, b)
                st = s.bc_coarse_solve(0, U, RHS)
                print(f"mask {mask} sigma {sigma} maxit {maxit}: gpu {st.coarse_iters} sweeps flag {st.coarse_flag}, reference {iters} flag {flag}")
                assert st.coarse_iters == iters and st.coarse_flag == flag
                assert st.coarse_relres == pytest.approx(relres, rel=1e-10)
                assert np.array_equal(s.get_array(U, 0), ref) and np.array_equal(s.get_array(RHS, 0), b)


# ---------------------------------------------------------------- 4. one cycle of each kind
CYCLE_KINDS = {
    "v-rb": dict(cycle=capi.CYCLE_V, smoother=RB), "w-rb": dict(cycle=capi.CYCLE_W, smoother=RB), "f-rb": dict(cycle=capi.CYCLE_F, smoother=RB),
    "v-jacobi": dict(cycle=capi.CYCLE_V, smoother=JAC, omega=6.0 / 7.0), "w-jacobi": dict(cycle=capi.CYCLE_W, smoother=JAC, omega=6.0 / 7.0),
    "f-jacobi": dict(cycle=capi.CYCLE_F, smoother=JAC, omega=6.0 / 7.0),
}
CYCLE_SETTINGS = {"mixed": (mixed(3), 0.0), "all": (63, 10.0)}


# (n, levels, extra) x kind x setting; sa65 (tests/tile_cases.py): a V(2,2) cycle whose Jacobi sweeps and residuals go through
# the tile inside the driver's dispatch on 65^3 and on 33 x 33 x 65, both with pairwise distinct axis coefficients
CYCLE_GRIDS = {"17-3": (17, 3, {}), "33-4": (33, 4, {}), "sa65": tc.SA65[1:]}
CYCLE_PARAMS = [pytest.param(g, kind, setting, id=f"{g}-{kind}-{setting}") for g in ("17-3", "33-4") for kind in CYCLE_KINDS for setting in CYCLE_SETTINGS]
CYCLE_PARAMS += [pytest.param("sa65", kind, "mixed", id=f"sa65-{kind}-mixed") for kind in ("v-rb", "v-jacobi")]


@functools.lru_cache(maxsize=None)
def cycle_inputs(shape):
    """u0, b with float32 values: exact in both working dtypes, so the long-double reference is shared"""
    rng = np.random.default_rng(shape[-1])
    return rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cycle_reference(grid, kind, setting, prec, coefs):
    """coefs: mg_level_coefficients of every level (doubles, shift included) -- the contract casts THOSE to T, and in fp32 the
    cast diagonal is not exactly -2 x the sum of the cast off-diagonals, which a reference with coefficients of its own
    would not see (n = 17, V red-black, mixed: 8.6e-8 from long double with its own float32 coefficients, 7.2e-7 with these)"""
    mask, sigma = CYCLE_SETTINGS[setting]
    n, levels, extra = CYCLE_GRIDS[grid]
    kw = desc_kw(3, n, levels, extra, capi.MG_F64, **CYCLE_KINDS[kind])
    u0, b = cycle_inputs((n, n, n))
    P = br.BCProblem(mask=mask, sigma=sigma, prec=prec, **{k: v for k, v in kw.items() if k != "dtype"})
    P.use_handle_coefs(coefs)
    return P.vcycle(P.as_prec(u0), P.as_prec(b), kw["coarse_maxit"])


@DTYPES
@pytest.mark.parametrize("grid,kind,setting", CYCLE_PARAMS)
def test_one_cycle_against_long_double(grid, kind, setting, dtype):
    """mg_bc_cycle (V, W, F; red-black and Jacobi 6/7, V(2,2), 6 coarse sweeps) against the long-double reference cycle on the
    handle's level coefficients. Tolerance, as test_vc_gpu.py builds it: 4 x the largest difference between bc_ref run in the
    working dtype and in long double on the same input -- computed here, from the reference alone. sa65 (V red-black and V
    Jacobi, the mixed mask): the tile on distinct axis coefficients and on nz != nx inside the driver. That difference on sa65,
    from the reference alone on the CPU (max |u| = 4.5): V red-black fp64 8.3e-16, fp32 3.7e-07; V Jacobi fp64 6.8e-16, fp32
    3.0e-07 -- under one eps_T x max |u|, as at 17 and 33: the rule stays about rounding on this hierarchy."""
    T = NP[dtype]
    mask, sigma = CYCLE_SETTINGS[setting]
    n, levels, extra = CYCLE_GRIDS[grid]
    u0, b = (a.astype(T) for a in cycle_inputs((n, n, n)))
    kw = desc_kw(3, n, levels, extra, dtype, **CYCLE_KINDS[kind])
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_shift(sigma); s.bc_set_faces(mask); s.set_solution(u0); s.set_rhs(b)
        coefs = tuple(s.level_coefficients(l) for l in range(levels))
        u_T, u_LD = cycle_reference(grid, kind, setting, T, coefs), cycle_reference(grid, kind, setting, LD, coefs)
        tol = 4 * float(abs(u_T.astype(LD) - u_LD).max())
        st = s.bc_cycle()
        got = s.get_solution().astype(LD)
        err = float(abs(got - u_LD).max())
        print(f"{grid} {kind} {setting} {T.__name__}: |gpu - ld| = {err:.3e}, tolerance = {tol:.3e}")
        assert err <= tol
        assert np.array_equal(s.get_array(RHS, 0), b)
        visits = {capi.CYCLE_V: 1, capi.CYCLE_W: 2 ** (levels - 2), capi.CYCLE_F: levels - 1}[kw["cycle"]]
        assert st.coarse_iters == visits * kw["coarse_maxit"] and st.coarse_flag == 0


@DTYPES
@pytest.mark.parametrize("smoother,omega", [(JAC, 6.0 / 7.0), (RB, 1.0)], ids=["jacobi67", "rb"])
def test_big_coarsest_level_is_smoothed_chip_wide(smoother, omega, dtype):
    """n = 65 on 2 levels: the coarsest level has 33^3 = 35937 > 32768 nodes, too many for the one-workgroup coarse kernel, so
    with MG_COARSE_FIXED the cycle runs coarse_maxit chip-wide sweeps there. One mg_bc_cycle (Neumann x-lo and y-hi) equals, bit
    for bit, the same steps made through the public entry points on a second handle; the statistics report the fixed sweeps."""
    T = NP[dtype]
    mask = capi.FACE_XLO | capi.FACE_YHI
    kw = desc_kw(3, 65, 2, {}, dtype, smoother=smoother, omega=omega, coarse_maxit=3)
    rng = np.random.default_rng(65)
    with capi.Solver(capi.make_desc(**kw)) as s, capi.Solver(capi.make_desc(**kw)) as m:
        shape = s.level_shape(0)
        assert int(np.prod(s.level_shape(1))) == 33 ** 3 > 32768
        u0, b = rng.standard_normal(shape).astype(T), rng.standard_normal(shape).astype(T)
        for h in (s, m):
            h.bc_set_faces(mask); h.set_solution(u0); h.set_rhs(b)
        st = s.bc_cycle()
        m.bc_smooth(0, smoother, kw["nu_pre"], U, RHS)
        m.bc_residual(0, U, RHS, TMP)
        m.bc_restrict(0, kw["restriction"], TMP, RHS)
        m.zero_array(U, 1)
        m.bc_smooth(1, smoother, kw["coarse_maxit"], U, RHS)
        m.prolong(1, True, U, U)
        m.bc_smooth(0, smoother, kw["nu_post"], U, RHS)
        got, want = s.get_solution(), m.get_solution()
        assert np.isfinite(want).all() and not np.array_equal(want, u0)
        assert np.array_equal(got, want), int((got != want).sum())
        assert np.array_equal(s.get_array(U, 1), m.get_array(U, 1)) and np.array_equal(s.get_array(RHS, 0), b)
        assert (st.coarse_iters, st.coarse_flag) == (3, 0)


# ---------------------------------------------------------------- 5. convergence (n = 33, 4 levels, red-black V(2,2), FULLW, 50 coarse sweeps)
def conv_desc(name, dtype):
    mask, sigma = br.TABLE[name]
    return mask, sigma, dict(dim=3, n=33, levels=4, length=1.0, alpha=1.0, dtype=dtype, cycle=capi.CYCLE_V, smoother=RB, nu_pre=2, nu_post=2,
                             restriction=FULLW, outer_pre_gs=0, coarse_mode=capi.COARSE_FIXED, coarse_maxit=50)


@functools.lru_cache(maxsize=None)
def conv_reference(name, prec, ncycles, tol):
    P = br.convergence_problem(name, prec=prec)
    b = br.convergence_rhs(P.shape(0)).astype(prec)
    return (b,) + P.solve_history(np.zeros_like(b), b, ncycles, 50, tol=tol)


@pytest.mark.parametrize("name", ["only-y-hi-dirichlet", "all-neumann-singular"])
def test_solve_history_follows_the_reference(name):
    """fp64: the history follows bc_ref's float64 history to rel 1e-6 while the entries are above 1e-10 and reaches 1e-10 in at
    most the reference's count plus one; the singular case takes the w-weighted mean out of RHS(0) and of the result"""
    b, u_ref, ref, b_ref, mean_ref = conv_reference(name, np.float64, 25, 1e-10)
    mask, sigma, kw = conv_desc(name, capi.MG_F64)
    P = br.convergence_problem(name)
    w = P.weights(b.shape)
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_shift(sigma); s.bc_set_faces(mask)
        if P.singular():
            s.set_array(E, 0, b)
            mean = s.bc_project(0, E)
            scale = float((w * abs(b)).sum() / w.sum())
            print("mean of RHS(0): gpu", mean, "numpy", mean_ref)
            assert abs(mean - mean_ref) <= 1e-13 * scale
            assert abs(s.get_array(E, 0) - b_ref).max() <= 4 * np.finfo(np.float64).eps * abs(b).max()
        s.set_rhs(b); s.set_solution(np.zeros_like(b))
        hist, stats = s.bc_solve(1e-10, 25)
        print("gpu", hist, "reference", ref)
        assert ref[-1] <= 1e-10 and hist[-1] <= 1e-10 and len(hist) <= len(ref) + 1
        assert all(st.coarse_iters == 50 for st in stats)
        k = min(len(hist), len(ref))
        above = ref[:k] > 1e-10
        assert above.sum() >= 8 and hist[:k][above] == pytest.approx(ref[:k][above], rel=1e-6)
        u = s.get_solution()
        if P.singular():
            assert abs(s.get_array(RHS, 0) - b_ref).max() <= 4 * np.finfo(np.float64).eps * abs(b).max()   # the projected right-hand side
            assert abs((w * u).sum()) <= 1e-12 * (w * abs(u)).sum()
        else:
            assert np.array_equal(s.get_array(RHS, 0), b)
            dm = P.dirichlet(b.shape)
            assert np.array_equal(u[dm], b[dm])


@pytest.mark.parametrize("name", ["only-y-hi-dirichlet", "all-neumann-singular"])
def test_fp32_reaches_the_reference_floor(name):
    """fp32: the same solve stalls at a floor; the GPU gets within 10 x the floor bc_ref reaches in float32 (computed here)"""
    b, _, ref, _, _ = conv_reference(name, np.float32, 14, 0.0)
    floor = float(ref.min())
    mask, sigma, kw = conv_desc(name, capi.MG_F32)
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_shift(sigma); s.bc_set_faces(mask); s.set_rhs(b); s.set_solution(np.zeros_like(b))
        hist, _ = s.bc_solve(0.0, 14)
        print(f"{name}: float32 floor of the reference {floor:.3e}, gpu {hist.min():.3e}")
        assert len(hist) == 15 and hist.min() <= 10 * floor


# ---------------------------------------------------------------- 6. a manufactured solution with an inhomogeneous flux
def test_flux_solution_is_second_order():
    """2-D, u = sin(x + .3) cos(2y), the flux folded into b as include/mg_hip.h describes, n = 33 and 65, solved to 1e-11"""
    errs = []
    for n in (33, 65):
        mask, sigma, b, u = br.flux_case(n)
        kw = dict(dim=2, n=n, levels=br.levels_for(n), length=1.0, alpha=1.0, dtype=capi.MG_F64, cycle=capi.CYCLE_V, smoother=RB, nu_pre=2,
                  nu_post=2, restriction=FULLW, outer_pre_gs=0, coarse_mode=capi.COARSE_FIXED, coarse_maxit=50)
        with capi.Solver(capi.make_desc(**kw)) as s:
            s.bc_set_faces(mask); s.set_rhs(b); s.set_solution(np.zeros_like(b))
            hist, _ = s.bc_solve(1e-11, 40)
            assert hist[-1] <= 1e-11
            errs.append(float(abs(s.get_solution() - u).max()))
            assert np.array_equal(s.get_array(RHS, 0), b)
    print("errors", errs, "ratio", errs[0] / errs[1])
    assert 3.9 <= errs[0] / errs[1] <= 4.1


# ---------------------------------------------------------------- 7. contracts
def refused(call, word):
    with pytest.raises(capi.MgError) as e:
        call()
    assert e.value.code == -4 and word in str(e.value), str(e.value)


def test_refusals_leave_u_untouched():
    rng = np.random.default_rng(5)
    base = desc_kw(3, 17, 3, {}, capi.MG_F64)

    def drivers(s):
        return [lambda: s.bc_cycle(), lambda: s.bc_solve(1e-8, 3)]

    with capi.Solver(capi.make_desc(**base)) as s:
        u0 = rng.standard_normal(s.level_shape(0)); s.set_solution(u0); s.set_rhs(u0)
        s.bc_set_faces(mixed(3))
        # bad masks, arrays, levels, kinds and smoothers
        for call in (lambda: s.bc_set_faces(64), lambda: s.bc_set_faces(-1),
                     lambda: s.bc_residual(3, U, RHS, RES), lambda: s.bc_residual(0, U, RHS, U), lambda: s.bc_residual(0, 7, RHS, RES),
                     lambda: s.bc_smooth(0, JAC, 1, U, U), lambda: s.bc_smooth(0, JAC, 1, TMP, RHS), lambda: s.bc_smooth(-1, RB, 1, U, RHS),
                     lambda: s.bc_smooth(0, capi.SMOOTH_GS_LEX, 1, U, RHS), lambda: s.bc_smooth(0, capi.SMOOTH_ZEBRA_X, 1, U, RHS),
                     lambda: s.bc_smooth(0, 99, 1, U, RHS), lambda: s.bc_coarse_solve(2, U, TMP), lambda: s.bc_coarse_solve(5, U, RHS),
                     lambda: s.bc_restrict(2, FULLW, U, RHS), lambda: s.bc_restrict(-1, FULLW, U, RHS), lambda: s.bc_restrict(0, 5, U, RHS),
                     lambda: s.bc_restrict(0, FULLW, 9, RHS), lambda: s.bc_project(3, U), lambda: s.bc_project(0, 9),
                     lambda: s.bc_set_form(2)):
            with pytest.raises(capi.MgError) as e:
                call()
            assert e.value.code == -4
        assert s.bc_get_faces() == mixed(3)
        # a stage callback
        s.set_stage_callback(lambda *a: None)
        for call in drivers(s):
            refused(call, "stage callback")
        s.set_stage_callback(None)
        assert np.array_equal(s.get_solution(), u0)
    # z bits on a 2-D handle
    with capi.Solver(capi.make_desc(**desc_kw(2, 17, 2, {}, capi.MG_F64))) as s:
        s.bc_set_faces(0b1010)
        for m in (16, 32, 63):
            refused(lambda: s.bc_set_faces(m), "z faces")
        assert s.bc_get_faces() == 0b1010
    # a sawtooth handle; a smoother the bc kernels do not have
    for more, word, extra_calls in ((dict(cycle=capi.CYCLE_SAWTOOTH), "sawtooth", 0), (dict(smoother=capi.SMOOTH_GS_LEX), "smoother", 1),
                                    (dict(smoother=capi.SMOOTH_ZEBRA_Y), "smoother", 1)):
        with capi.Solver(capi.make_desc(**dict(base, **more))) as s:
            u0 = rng.standard_normal(s.level_shape(0)); s.set_solution(u0); s.set_rhs(u0)
            s.bc_set_faces(63)
            for call in drivers(s) + [lambda: s.bc_coarse_solve(2, U, RHS)] * extra_calls:
                refused(call, word)
            assert np.array_equal(s.get_solution(), u0)
    # distributed handles, the dry-run measurement handle included
    with capi.Solver(capi.make_desc(**base), device=0, rank=0, nranks=2, dry=True) as s:
        u0 = rng.standard_normal(s.level_shape(0)); s.set_solution(u0)
        before = s.device_bytes()
        for call in drivers(s) + [lambda: s.bc_set_faces(1), lambda: s.bc_residual(0, U, RHS, RES), lambda: s.bc_smooth(0, RB, 1, U, RHS),
                                  lambda: s.bc_restrict(0, FULLW, U, RHS), lambda: s.bc_coarse_solve(2, U, RHS), lambda: s.bc_project(0, U)]:
            refused(call, "distributed")
        assert np.array_equal(s.get_solution(), u0) and s.device_bytes() == before and s.bc_get_faces() == 0
    # NULL handle
    L = capi.load()
    assert L.mg_bc_cycle(None, None) == -4 and L.mg_bc_set_faces(None, 0) == -4 and L.mg_bc_get_faces(None, None) == -4
    assert L.mg_bc_solve(None, 0.0, 1, None, 0, None, None) == -4 and L.mg_bc_project(None, 0, 0, None) == -4


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
            for mask, sigma in ((mixed(3), 0.0), (63, 0.0)):
                s.set_shift(sigma); s.bc_set_faces(mask)
                s.set_rhs(b); s.set_solution(np.zeros_like(b))
                hist, _ = s.bc_solve(0.0, 3)
                out += [hist, s.get_solution(), s.get_array(RHS, 0)]
                s.set_array(E, 0, b); s.bc_residual(0, E, RHS, RES); s.bc_smooth(0, RB, 1, E, RHS); s.bc_restrict(0, FULLW, E, TMP)
                s.bc_coarse_solve(3, U, RHS); s.bc_project(0, E); s.bc_cycle()
                out.append(s.get_solution())
                assert s.device_bytes() == before   # no mg_bc_* call allocates
            runs.append(out)
        for x, y in zip(*runs):
            assert np.array_equal(x, y)   # two runs give the same bits
        # a handle that ran mg_bc_solve gives mg_cycle / mg_solve results bit-identical to a fresh handle
        outs = []
        for h in (fresh, s):
            h.set_rhs(b); h.set_solution(np.zeros_like(b))
            h.cycle(); u1 = h.get_solution()
            hist, _ = h.solve(0.0, 2)
            outs.append((u1, hist, h.get_solution()))
        for x, y in zip(*outs):
            assert np.array_equal(x, y)
        assert s.device_bytes() == fresh.device_bytes() == before
