"""Implicit time steps on the operator families on the GPU (mg_vc_heat_*, mg_bc_heat_*, mg_fas_heat_*)
against tests/step_ref.py: the right-hand side launch bit for bit (marching tile and plain form), the identities with
mg_heat_rhs, the step against the loop written out and against an independent long-double stepper, conservation with
every face Neumann, the refusals, determinism and isolation."""
import math
import threading

import numpy as np
import pytest

from multigrid_prj_amd import capi
from tests import bc_ref as br
from tests import fas_ref as fr
from tests import heat_ref as hr
from tests import npref
from tests import step_ref as sr
from tests import tile_cases as tc
from tests import vc_ref as vr
from tests.test_independent_reference import check_max, cycle_bound, sweep_scale

pytestmark = pytest.mark.gpu

NP = {capi.MG_F64: np.float64, capi.MG_F32: np.float32}
DTYPES = pytest.mark.parametrize("dtype", [capi.MG_F64, capi.MG_F32], ids=["f64", "f32"])
U, E, RHS, TMP, RES = capi.ARR_U, capi.ARR_E, capi.ARR_RHS, capi.ARR_TMP, capi.ARR_RES
JAC, RB = capi.SMOOTH_JACOBI, capi.SMOOTH_RBGS
LD = np.longdouble
MIXED = capi.FACE_XLO | capi.FACE_YHI | capi.FACE_ZLO | capi.FACE_ZHI   # in 2-D the z bits are dropped

# the shapes of tests/test_vc_gpu.py's CASES: 9, 17 plain; 33, 35 tile in fp64 (35: odd last column, not 2^k + 1), 34 an even
# row; 65, 67 tile in both dtypes (67: a partial last vector in fp32); 2-D always plain
SHAPES = [(3, 9, 2, {}), (3, 17, 2, {}), (3, 33, 2, {}), (3, 35, 2, {}), (3, 34, 1, {}), (3, 65, 2, {}), (3, 67, 2, {}), (2, 17, 2, {}),
          (2, 130, 1, {})]
# ... all with cx == cy == cz. tests/tile_cases.py's a33 (fp64) and a65 (both dtypes) put the OP_STEP tile, its no-neighbour
# theta == 1 form included, on pairwise distinct axis coefficients (the right-hand side is level 0 only: no semi-coarsened case)
SHAPES += [tc.A33, tc.A65]
# family settings: name -> (family, its parameter)
FAMS = {"vc": ("vc", None), "bc0": ("bc", 0), "bc-all": ("bc", 63), "bc-mixed": ("bc", MIXED), "cubic": ("fas", (fr.CUBIC, 50.0)),
        "exp": ("fas", (fr.EXP, 20.0))}


def shape_id(c):
    return tc.case_id(c) if len(c) == 4 and c[3] else f"{c[0]}d{c[1]}"


def desc_kw(dim, n, levels, dtype, **more):
    kw = dict(dim=dim, n=n, levels=levels, length=1.0, alpha=1.3, dtype=dtype, cycle=capi.CYCLE_V, smoother=RB, nu_pre=2, nu_post=2,
              restriction=capi.RESTRICT_FULLW, outer_pre_gs=0, coarse_mode=capi.COARSE_FIXED, coarse_maxit=6)
    kw.update(more)
    return kw


def mask_of(dim, mask):
    return mask & br.all_faces(dim)


def random_a(shape, seed):
    return np.random.default_rng(seed).uniform(0.5, 2.0, shape)


def configure(s, name, dim, a=None):
    """puts the family's state on the handle"""
    fam, par = FAMS[name]
    if fam == "vc":
        s.vc_set_coefficient(a)
    elif fam == "bc":
        s.bc_set_faces(mask_of(dim, par))
    else:
        s.fas_set_reaction(*par)
    return fam


def reference(name, kw, prec, coefs, sigma=0.0, a=None):
    """the family's problem in `prec` with the handle's level coefficients (coefs: read while the handle's shift was `sigma`)"""
    fam, par = FAMS[name]
    pk = {k: v for k, v in kw.items() if k != "dtype"}
    if fam == "vc":
        P = vr.VCProblem(prec=prec, sigma=sigma, **pk)
        P.use_handle_coefs(coefs)
        P.set_a(a)
    elif fam == "bc":
        P = br.BCProblem(mask=mask_of(kw["dim"], par), prec=prec, sigma=sigma, **pk)
        P.use_handle_coefs(coefs)
    else:
        P = fr.FASProblem(kind=par[0], gamma=par[1], prec=prec, sigma=sigma, **pk)
        P.use_handle_coefs(coefs)
    return P


def calls(s, fam):
    return {"rhs": getattr(s, fam + "_heat_rhs"), "step": getattr(s, fam + "_heat_step"), "cycle": getattr(s, fam + "_cycle"),
            "residual": getattr(s, fam + "_residual"), "form": getattr(s, fam + "_set_form")}


def is_tile(dim, n, T):
    return vr.march_side(dim, n, np.dtype(T).itemsize)


# ---------------------------------------------------------------- 1. the right-hand side launch, bit for bit
@DTYPES
@pytest.mark.parametrize("case", SHAPES, ids=shape_id)
def test_rhs_kernel_bit_for_bit(case, dtype):
    """every family, theta 1 / 0.5 / 0.75, with and without a source, tile and plain form, a handle shift that must be
    ignored and kept; cubic, vc and bc bit for bit, exp within 8 eps x magnitude (the device's exp is specified to 1 ulp). a33
    and a65: the tile with pairwise distinct axis coefficients, in every family setting"""
    dim, n, levels, extra = case
    T = NP[dtype]
    eps = float(np.finfo(T).eps)
    kw = desc_kw(dim, n, levels, dtype, **extra)
    rng = np.random.default_rng(1000 * dim + n)
    forms_seen, worst_exp = set(), 0.0
    with capi.Solver(capi.make_desc(**kw)) as s:
        shape = s.level_shape(0)
        coefs0 = [s.level_coefficients(l) for l in range(levels)]   # the unshifted operator
        a = random_a(shape, n).astype(T)
        f = (10.0 * rng.standard_normal(shape)).astype(T)
        other = rng.standard_normal(shape).astype(T)
        s.set_shift(123.0)
        for name in FAMS:
            fam = configure(s, name, dim, a)
            c = calls(s, fam)
            P = reference(name, kw, T, coefs0, a=a)
            u = (rng.uniform(-2.0, 2.0, shape) if name == "exp" else rng.standard_normal(shape)).astype(T)
            for src in (True, False):
                s.heat_set_source(f if src else None)
                for theta, dt, (au, ad) in ((1.0, 1e-3, (U, RHS)), (0.5, 2e-3, (E, TMP)), (0.75, 1e-3, (U, RHS))):
                    want = sr.step_rhs(P, u, f if src else None, dt, theta)
                    assert want.dtype == T
                    for form in ((0, 1) if is_tile(dim, n, T) else (0,)):
                        c["form"](form)
                        forms_seen.add("tile" if form == 0 and is_tile(dim, n, T) else "plain")
                        s.set_array(au, 0, u); s.set_array(ad, 0, other)
                        c["rhs"](dt, theta, au, ad)
                        got = s.get_array(ad, 0)
                        tag = (name, src, theta, form)
                        if name == "exp" and theta != 1.0:
                            mag = sr.step_rhs_mag(P, u, f if src else None, dt, theta).astype(np.float64)
                            d = float((abs(got.astype(np.float64) - want.astype(np.float64)) / mag).max()) / eps
                            worst_exp = max(worst_exp, d)
                            assert d <= 8.0, (tag, d)
                            fx = sr.fixed_nodes(P, shape)
                            assert np.array_equal(got[fx], u[fx]), tag
                        else:
                            assert np.array_equal(got, want), (tag, int((got != want).sum()))
                        assert np.array_equal(s.get_array(au, 0), u), tag
                        assert s.get_shift() == 123.0
                    c["form"](0)
    print(f"{shape_id(case)} {T.__name__}: exp, largest error in units of eps x magnitude: {worst_exp:.3f}")
    assert forms_seen == ({"tile", "plain"} if is_tile(dim, n, T) else {"plain"})


# ---------------------------------------------------------------- 2. the identities with mg_heat_rhs
@DTYPES
@pytest.mark.parametrize("case", [(3, 17, 2), (3, 35, 2), (3, 67, 2), (2, 130, 1)], ids=shape_id)
def test_identities_with_heat_rhs(case, dtype):
    """on the same random arrays: bc with mask 0 and fas with gamma 0 (both kinds) give mg_heat_rhs's bits; so do vc and fas
    with theta == 1; bc with theta == 1 is f + rdt u on the unknowns; vc with a == 1 agrees to 8 eps of npref's magnitudes"""
    dim, n, levels = case
    T = NP[dtype]
    eps = float(np.finfo(T).eps)
    kw = desc_kw(dim, n, levels, dtype)
    P = npref.Problem(**{k: v for k, v in kw.items() if k != "dtype"})
    rng = np.random.default_rng(n + 3)
    with capi.Solver(capi.make_desc(**kw)) as s:
        shape = s.level_shape(0)
        u, f = rng.standard_normal(shape).astype(T), (10.0 * rng.standard_normal(shape)).astype(T)
        s.set_solution(u)
        forms = (0, 1) if is_tile(dim, n, T) else (0,)

        def run(fam, dt, theta):
            out = []
            for form in forms:
                getattr(s, fam + "_set_form")(form)
                getattr(s, fam + "_heat_rhs")(dt, theta, U, RHS)
                out.append(s.get_array(RHS, 0))
            getattr(s, fam + "_set_form")(0)
            return out
        for src in (f, None):
            s.heat_set_source(src)
            for theta, dt in ((0.5, 2e-3), (0.75, 1e-3), (1.0, 1e-3)):
                s.heat_rhs(dt, theta, U, RHS)
                want = s.get_array(RHS, 0)
                s.bc_set_faces(0)
                assert all(np.array_equal(g, want) for g in run("bc", dt, theta)), ("bc mask 0", theta)
                for kind in (capi.FAS_CUBIC, capi.FAS_EXP):
                    s.fas_set_reaction(kind, 0.0)
                    assert all(np.array_equal(g, want) for g in run("fas", dt, theta)), ("fas gamma 0", kind, theta)
                s.vc_set_coefficient(np.ones(shape, T))
                mag = abs(T(1.0 / dt) * u) + abs(T(1.0 - theta)) * np.asarray(P.apply_A(u, 0, absolute=True), np.float64)
                bound = 8 * eps * (mag + (0 if src is None else abs(f))) * abs(T(1.0 / theta))
                for g in run("vc", dt, theta):
                    d = abs(g.astype(LD) - want.astype(LD))
                    assert (d <= bound).all(), ("vc a == 1", theta, float((d / bound).max()))
                if theta == 1.0:
                    s.vc_set_coefficient(random_a(shape, 5).astype(T))
                    assert all(np.array_equal(g, want) for g in run("vc", dt, theta))
                    s.fas_set_reaction(capi.FAS_CUBIC, 50.0)
                    assert all(np.array_equal(g, want) for g in run("fas", dt, theta))
                    t = T(1.0 / dt) * u
                    t = t if src is None else f + t
                    for mask in (br.all_faces(dim), mask_of(dim, MIXED)):
                        s.bc_set_faces(mask)
                        exp = np.where(br.BCProblem(mask=mask, dim=dim, n=n, levels=1).dirichlet(shape), u, t)
                        assert all(np.array_equal(g, exp) for g in run("bc", dt, theta)), ("bc theta 1", mask)
        assert np.array_equal(s.get_solution(), u)


# ---------------------------------------------------------------- 3. the step is the loop written out
STEP_CFG = {"v-rb": dict(cycle=capi.CYCLE_V, smoother=RB), "w-jac": dict(cycle=capi.CYCLE_W, smoother=JAC, omega=6.0 / 7.0)}


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("grid", [(17, 3), (33, 4)], ids=["17", "33"])
@pytest.mark.parametrize("cfg", list(STEP_CFG))
@pytest.mark.parametrize("name", ["vc", "bc-mixed", "cubic"])
def test_step_equals_the_loop_written_out(name, cfg, grid, theta):
    n, levels = grid
    kw = desc_kw(3, n, levels, capi.MG_F64, **STEP_CFG[cfg])
    dt, nsteps, ncyc = 1e-3, 3, 2
    rng = np.random.default_rng(47 + n)
    shape = (n,) * 3
    u0, f, a = rng.standard_normal(shape), 10.0 * rng.standard_normal(shape), random_a(shape, n)
    with capi.Solver(capi.make_desc(**kw)) as s, capi.Solver(capi.make_desc(**kw)) as s2:
        for h in (s, s2):
            fam = configure(h, name, 3, a)
            h.heat_set_source(f); h.set_solution(u0)
        st = calls(s, fam)["step"](dt, theta, nsteps, ncyc)
        c2 = calls(s2, fam)
        s2.set_shift(1.0 / (theta * dt))
        for _ in range(nsteps):
            c2["rhs"](dt, theta, U, RHS)
            for _c in range(ncyc):
                c2["cycle"]()
        assert (st.steps, st.cycles, st.time) == (nsteps, nsteps * ncyc, nsteps * dt)
        assert s.get_shift() == s2.get_shift() == 1.0 / (theta * dt)
        assert np.array_equal(s.get_solution(), s2.get_solution())
        assert np.array_equal(s.get_array(RHS, 0), s2.get_array(RHS, 0))
        rr, bb = c2["residual"](0, U, RHS, -1), s2.sumsq(0, RHS)
        assert st.relres == (0.0 if rr == 0.0 else math.sqrt(rr / bb))


# ---------------------------------------------------------------- 4. against an independent stepper
INDEP_MARGIN = 10.0   # the margin tests/test_independent_reference.py documents for its cycle bound ("about 10")
# error / (error of the same reference run in T) observed on MI355X over the 20 cases below: see DESIGN.md section 21
INDEP_CYCLES = {capi.MG_F64: 16, capi.MG_F32: 8}


def reference_run(name, kw, prec, coefs0, coefs_s, sigma, a_levels, a, u0, f, dt, theta, steps, solve):
    """the theta scheme over the family's reference in `prec` -> (u after `steps` steps, the scale of cycle_bound, Ps)"""
    P0, Ps = reference(name, kw, prec, coefs0, a=a), reference(name, kw, prec, coefs_s, sigma=sigma, a=a)
    if a_levels is not None:
        P0.a = Ps.a = [P0.as_prec(x) for x in a_levels]   # the coarse coefficients the handle holds (rounded in T)
    ref = sr.FamilyStepper(P0, Ps, dt, theta, solve)
    u, scale = P0.as_prec(u0), 0.0
    for _ in range(steps):
        un, b = ref.step(u, f)
        scale = max(scale, float(np.abs(un).max()) + sweep_scale(Ps, 0, b, u, un))
        u = un
    return u, scale, Ps


@DTYPES
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", ["vc", "bc-all", "bc-mixed", "cubic", "exp"])
def test_step_against_an_independent_stepper(name, theta, dtype):
    """The reference is the theta scheme in long double over vc_ref / bc_ref / fas_ref with every step solved to 1e-17; the
    GPU runs enough cycles per step to converge. 1/(theta dt) is the geometric mean of the extreme eigenvalues of A0, so
    that a cycle is far from exact and the test sees the solver.
    Tolerance: the SAME reference run in T (numpy, the cycle counts the GPU runs) misses the long-double one by its own
    rounding; the GPU may miss it by INDEP_MARGIN times that. The a-priori bound of tests/test_heat_gpu.py's test of the
    same name -- steps x cycle_bound with the scale of the reference run; vc's diagonal varies with a, so max a / min a
    goes in -- is asserted too; it is some 1e5 times wider."""
    T = NP[dtype]
    eps = float(np.finfo(T).eps)
    n, levels, steps = 17, 3, 3
    kw = desc_kw(3, n, levels, dtype)
    lo, hi = hr.eigen_range(npref.Problem(**{k: v for k, v in kw.items() if k != "dtype"}))
    dt = 1.0 / (theta * math.sqrt(lo * hi))
    sigma = 1.0 / (theta * dt)
    assert lo < sigma < hi
    rng = np.random.default_rng(53)
    shape = (n,) * 3
    u0 = rng.uniform(-1.0, 1.0, shape).astype(T)
    f = (10.0 * rng.standard_normal(shape)).astype(T)
    a = random_a(shape, 9).astype(T)
    with capi.Solver(capi.make_desc(**kw)) as s:
        coefs0 = [s.level_coefficients(l) for l in range(levels)]
        fam = configure(s, name, 3, a)
        s.heat_set_source(f); s.set_solution(u0)
        st = calls(s, fam)["step"](dt, theta, steps, INDEP_CYCLES[dtype])
        got = s.get_solution()
        coefs_s = [s.level_coefficients(l) for l in range(levels)]
        a_levels = [s.vc_get_coefficient(l) for l in range(levels)] if fam == "vc" else None
    args = (coefs0, coefs_s, sigma, a_levels, a, u0, f, dt, theta, steps)
    u, scale, Ps = reference_run(name, kw, LD, *args, sr.converged_solver(kw["coarse_maxit"], 1e-17))
    u_T, _, _ = reference_run(name, kw, T, *args, sr.cycle_solver(INDEP_CYCLES[dtype], kw["coarse_maxit"]))
    assert u_T.dtype == T
    own = float(np.abs(u_T.astype(LD) - u).max())
    amp = float(a.max() / a.min()) if fam == "vc" else 1.0
    bound = steps * amp * cycle_bound(Ps, eps, kw["coarse_maxit"], scale)
    err = float(np.abs(got.astype(LD) - u).max())
    print(f"{name} theta {theta} {T.__name__}: relres {st.relres:.2e}, error {err:.3e} = {err / own:.3g} x the reference's own in T, "
          f"= {err / bound:.3g} x the a-priori bound")
    # converged: what is left of the residual is its own rounding, 16 eps (|b| + |sigma I + A0||u|) per node
    # (tests/test_independent_reference.py's C_RESID), and |sigma I + A0| <= sigma + 2 cd0 = sigma + hi + lo
    assert st.relres <= 32 * eps * (2 + (hi + lo) / sigma)
    assert own > 0 and err <= INDEP_MARGIN * own, (err, own)
    check_max(got, u, bound, f"{name} theta {theta}")


# ---------------------------------------------------------------- 5. conservation with every face Neumann
def test_conservation_on_the_device():
    """mask 63, fp64, n = 33: the w-weighted mean (read through mg_bc_project on a copy) follows mean0 + t (w.f) / sum w to
    1e-12 relative when every step is converged; with ONE cycle per step the drift of a step is -theta dt (w.r) / sum w with r the
    saved mg_bc_residual. Bound of the second: the identity is exact for exact sums and an exact residual, so what is left is
    rounding -- of the two device means (N terms each, added in double: N eps mean|v| at the worst), of the right-hand side
    launch and of the residual (16 eps x their magnitudes per node, the per-operation constant of
    tests/test_independent_reference.py, weighted and scaled by theta dt)."""
    n, levels, theta = 33, 4, 0.5
    kw = desc_kw(3, n, levels, capi.MG_F64)
    shape = (n,) * 3
    lo, hi = hr.eigen_range(npref.Problem(**{k: v for k, v in kw.items() if k != "dtype"}))
    dt = 1.0 / (theta * math.sqrt(lo * hi))
    rng = np.random.default_rng(71)
    u0 = 1.0 + 0.3 * rng.standard_normal(shape)
    f = 50.0 + 10.0 * rng.standard_normal(shape)
    Pb = br.BCProblem(mask=63, prec=LD, dim=3, n=n, levels=1)
    w = Pb.weights(shape).astype(LD)
    sw, eps, N = float(w.sum()), float(np.finfo(np.float64).eps), u0.size
    wf = float(np.sum(w * f) / sw)
    assert abs(wf) > 1.0

    def mean(s):
        s.set_array(E, 0, s.get_solution())
        return s.bc_project(0, E)
    with capi.Solver(capi.make_desc(**kw)) as s:
        coefs0 = [s.level_coefficients(l) for l in range(levels)]
        s.bc_set_faces(63); s.heat_set_source(f); s.set_solution(u0)
        m0 = mean(s)
        assert abs(m0 - float(np.sum(w * u0) / sw)) <= N * eps * float(np.sum(w * abs(u0))) / sw
        for k in range(1, 6):
            st = s.bc_heat_step(dt, theta, 1, 20)
            assert st.relres <= 1e-12
            want = m0 + k * dt * wf
            assert abs(mean(s) - want) <= 1e-12 * abs(want), (k, mean(s), want)
        # one cycle per step: not converged, and the mean drifts by exactly what the residual says
        u = s.get_solution()
        m_before = mean(s)
        st = s.bc_heat_step(dt, theta, 1, 1)
        assert st.relres > 1e-6
        un, rhs = s.get_solution(), s.get_array(RHS, 0)
        ss = s.bc_residual(0, U, RHS, TMP)
        r = s.get_array(TMP, 0)
        assert st.relres == math.sqrt(ss / s.sumsq(0, RHS))
        m_after = mean(s)
        coefs_s = [s.level_coefficients(l) for l in range(levels)]
    drift = m_after - (m_before + dt * wf)
    want = -theta * dt * float(np.sum(w * r.astype(LD))) / sw
    pk = {k: v for k, v in kw.items() if k != "dtype"}
    P0 = br.BCProblem(mask=63, prec=np.float64, **pk); P0.use_handle_coefs(coefs0)
    Ps = br.BCProblem(mask=63, prec=np.float64, sigma=1.0 / (theta * dt), **pk); Ps.use_handle_coefs(coefs_s)
    mag_rhs = sr.step_rhs_mag(P0, u, f, dt, theta)
    mag_r = abs(rhs) + Ps.apply_A(un, 0, absolute=True)
    bound = eps * (N * (float(np.sum(w * abs(un))) + float(np.sum(w * abs(u)))) / sw
                   + theta * dt * 16 * float(np.sum(w * (mag_rhs + mag_r))) / sw)
    print(f"drift {drift:.6e}, -theta dt (w.r)/sum w {want:.6e}, difference / bound {abs(drift - want) / bound:.3g}")
    assert abs(want) > 1e3 * bound        # the check sees the drift
    assert abs(drift - want) <= bound


# ---------------------------------------------------------------- 6. refusals leave U, RHS and the shift untouched
def refused(call, word=None):
    with pytest.raises(capi.MgError) as e:
        call()
    assert e.value.code == -4 and (word is None or word in str(e.value)), str(e.value)


@pytest.mark.parametrize("name", ["vc", "bc-mixed", "cubic"])
def test_refusals(name):
    n = 17
    rng = np.random.default_rng(61)
    shape = (n,) * 3
    u0, b0, a = rng.standard_normal(shape), rng.standard_normal(shape), random_a(shape, 2)
    fam = FAMS[name][0]

    def check(s, bad):
        s.set_solution(u0); s.set_array(RHS, 0, b0); s.set_shift(7.5)
        for call, word in bad:
            refused(call, word)
            assert s.get_shift() == 7.5 and np.array_equal(s.get_solution(), u0) and np.array_equal(s.get_array(RHS, 0), b0), word
    with capi.Solver(capi.make_desc(**desc_kw(3, n, 3, capi.MG_F64))) as s:
        if fam == "vc":   # no coefficient yet
            check(s, [(lambda: s.vc_heat_step(1e-3, 1.0, 1, 1), "coefficient"), (lambda: s.vc_heat_rhs(1e-3, 1.0), "coefficient")])
        configure(s, name, 3, a)
        c = calls(s, fam)
        step, rhs = c["step"], c["rhs"]
        check(s, [
            (lambda: step(0.0, 1.0, 1, 1), "dt"), (lambda: step(-1e-3, 1.0, 1, 1), "dt"), (lambda: step(math.inf, 1.0, 1, 1), "dt"),
            (lambda: step(math.nan, 1.0, 1, 1), "dt"), (lambda: step(1e-3, 0.0, 1, 1), "theta"), (lambda: step(1e-3, 1.5, 1, 1), "theta"),
            (lambda: step(1e-3, math.nan, 1, 1), "theta"), (lambda: step(1e-3, 1.0, 0, 1), "nsteps"),
            (lambda: step(1e-3, 1.0, 1, 0), "cycles_per_step"), (lambda: rhs(1e-3, 1.0, U, U), "arr_dst"), (lambda: rhs(0.0, 1.0), "dt"),
            (lambda: rhs(1e-3, 2.0), "theta"),
        ])
        s.set_stage_callback(lambda *x: None)
        check(s, [(lambda: step(1e-3, 1.0, 1, 1), "stage callback")])
        s.set_stage_callback(None)
        assert step(1e-3, 1.0, 1, 1).steps == 1 and s.get_shift() == 1e3
    for more, word in ((dict(cycle=capi.CYCLE_SAWTOOTH, smoother=JAC), "sawtooth"), (dict(smoother=capi.SMOOTH_ZEBRA_Y), "smoother")):
        with capi.Solver(capi.make_desc(**desc_kw(3, n, 3, capi.MG_F64, **more))) as s:
            configure(s, name, 3, a)
            check(s, [(lambda: calls(s, fam)["step"](1e-3, 1.0, 1, 1), word)])


def test_refuses_distributed_handle():
    """as tests/test_heat_gpu.py::test_refuses_distributed_handle: two ranks on one device, and the dry-run handle"""
    from tests.thread_ranks import ThreadWorld
    kw = dict(dim=3, n=33, levels=3, length=1.0, cycle=capi.CYCLE_V, smoother=JAC, omega=0.8, nu_pre=2, nu_post=2,
              restriction=capi.RESTRICT_FULLW, outer_pre_gs=0, dist_min_n=9)
    desc = capi.make_desc(**kw)
    tw = ThreadWorld(2)
    res = [None, None]

    def new_calls(s):
        return [fn for fam in ("vc", "bc", "fas") for fn in (lambda fam=fam: getattr(s, fam + "_heat_step")(1e-3, 1.0, 1, 1),
                                                              lambda fam=fam: getattr(s, fam + "_heat_rhs")(1e-3, 1.0))]

    def rank_main(r):
        try:
            s = capi.Solver(desc, device=0, rank=r, nranks=2, host_comm=tw.host_comm(r))
            try:
                got = []
                for call in new_calls(s):
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
    assert res == [[(-4, True)] * 6 + [0.0]] * 2, res
    with capi.Solver(desc, device=0, rank=0, nranks=2, dry=True) as s:
        for call in new_calls(s):
            refused(call, "distributed")


# ---------------------------------------------------------------- 7. determinism and isolation
@pytest.mark.parametrize("name", ["vc", "bc-all", "cubic"])
def test_determinism_and_isolation(name):
    n, dt, theta = 33, 2e-3, 0.5
    kw = desc_kw(3, n, 3, capi.MG_F64)
    rng = np.random.default_rng(59)
    shape = (n,) * 3
    u0, f, a = rng.standard_normal(shape), 10.0 * rng.standard_normal(shape), random_a(shape, 4)
    with capi.Solver(capi.make_desc(**kw)) as fresh:
        fresh.heat_set_source(f); fresh.set_solution(u0)
        st_fresh = fresh.heat_step(dt, theta, 2, 2)
        u_fresh = fresh.get_solution()
    with capi.Solver(capi.make_desc(**kw)) as s:
        fam = configure(s, name, 3, a)
        c = calls(s, fam)
        s.heat_set_source(f)
        base = s.device_bytes()
        outs = []
        for _ in range(2):
            s.set_solution(u0)
            st = c["step"](dt, theta, 3, 2)
            outs.append((s.get_solution(), s.get_array(RHS, 0), st.relres))
            c["rhs"](dt, theta, U, TMP)
            outs[-1] += (s.get_array(TMP, 0),)
        assert all(np.array_equal(x, y) for x, y in zip(outs[0][:2] + outs[0][3:], outs[1][:2] + outs[1][3:])) and outs[0][2] == outs[1][2]
        assert s.device_bytes() == base          # the new entry points allocate nothing
        # mg_heat_step afterwards is what it is on a handle that never saw the family steppers
        s.set_solution(u0)
        st = s.heat_step(dt, theta, 2, 2)
        assert np.array_equal(s.get_solution(), u_fresh) and st.relres == st_fresh.relres
