"""W- and F-cycles on the GPU (MG_CYCLE_W, MG_CYCLE_F; include/mg_hip.h):
 1. the one-launch LDS sub-cycle (mg_subcycle.hip) against the launch-by-launch path, bit for bit;
 2. whole cycles and a short solve against the independent reference (tests/npref_cycles.py), the kernel on and off;
 3. W converges where V diverges (red-black V(1,1), injection, two coarse sweeps);
 4. the drivers that call "the handle's cycle" on W / F handles;
 5. the contract and the refusals.
The reference's bound per V-cycle (cycle_bound, tests/test_independent_reference.py) covers one visit of each of the L levels;
a cycle that makes v level visits gets v / L of it."""
import math
import os

import numpy as np
import pytest

from multigrid_prj_amd import build as mgbuild
from multigrid_prj_amd import capi
from tests import npref as npr
from tests import npref_cycles as nc
from tests import npref_fmg as nf
from tests.test_cli_and_mirror import run_cli
from tests.test_cycle_kinds_cpu import ROOTS, WEAK, WEAK_CASES, default_root, rate, weak_history
from tests.test_fmg_gpu import FMG_K, fmg_scale
from tests.test_independent_reference import C_RESID, check_max, cycle_bound, eps_of, np_of, sweep_scale

pytestmark = pytest.mark.gpu

LD = np.longdouble
KINDS = [capi.CYCLE_V, capi.CYCLE_W, capi.CYCLE_F]
KNAME = {capi.CYCLE_V: "V", capi.CYCLE_W: "W", capi.CYCLE_F: "F"}
ES = {capi.MG_F64: 8, capi.MG_F32: 4}


def planned_root(dim, n, levels, dtype, semi=0):
    """the finest admissible root, as tests/test_cycle_kinds_cpu.py pins the planner on these shapes"""
    return {r[:5]: r[5] for r in ROOTS}[(dim, n, levels, ES[dtype], semi)]


def coarse_solves(kind, nlev):
    """coarse solves of one cyc() over nlev levels"""
    return {capi.CYCLE_V: 1, capi.CYCLE_F: max(nlev - 1, 1), capi.CYCLE_W: 2 ** max(nlev - 2, 0)}[kind]


# ======================================================================= 1. the kernel against the launches
SHAPES = [
    dict(id="3d-17-L3-f64", dim=3, n=17, levels=3, dtype=capi.MG_F64),                      # root 9^3 over 5^3: the smallest
    dict(id="3d-33-L4-f64", dim=3, n=33, levels=4, dtype=capi.MG_F64),                      # root 17^3, at the LDS limit
    dict(id="3d-25-L3-f32", dim=3, n=25, levels=3, dtype=capi.MG_F32),                      # 13^3 -> 7^3, not 2^k + 1
    dict(id="3d-17-L4-semi-f64", dim=3, n=17, levels=4, dtype=capi.MG_F64, semi_xy=1, aniso=(1.0, 0.5, 0.05)),   # root 1 is 9 x 9 x 17
    dict(id="2d-129-L6-f64", dim=2, n=129, levels=6, dtype=capi.MG_F64),                    # root 65^2
    dict(id="2d-49-L4-f32", dim=2, n=49, levels=4, dtype=capi.MG_F32),                      # not 2^k + 1
]
# (smoother, omega, nu_pre, nu_post): even and odd numbers of out-of-place Jacobi sweeps, and red-black
SMOOTHERS = [
    ("jacobi-6/7", capi.SMOOTH_JACOBI, 6 / 7, 2, 2),
    ("jacobi-1", capi.SMOOTH_JACOBI, 1.0, 1, 2),
    ("rbgs", capi.SMOOTH_RBGS, 1.0, 1, 1),
]


def shape_kw(shape):
    return {k: v for k, v in shape.items() if k != "id"}


def both_paths(s, root, kind, u, b):
    out = []
    for path in (0, 1):
        s.set_array(capi.ARR_U, root, u); s.set_array(capi.ARR_RHS, root, b)
        st = s.subcycle(root, kind, path)
        out.append((st, s.get_array(capi.ARR_U, root)))
    return out


@pytest.mark.parametrize("sm", SMOOTHERS, ids=[s[0] for s in SMOOTHERS])
@pytest.mark.parametrize("shape", SHAPES, ids=[s["id"] for s in SHAPES])
def test_kernel_and_launches_give_the_same_bits(shape, sm):
    kw = shape_kw(shape)
    _, smoother, omega, nu1, nu2 = sm
    root = planned_root(kw["dim"], kw["n"], kw["levels"], kw["dtype"], kw.get("semi_xy", 0))
    dt = np_of(kw["dtype"])
    for restriction in (capi.RESTRICT_FULLW, capi.RESTRICT_INJECT):
        d = capi.make_desc(length=1.0, alpha=1.0, cycle=capi.CYCLE_V, smoother=smoother, omega=omega, nu_pre=nu1, nu_post=nu2,
                           restriction=restriction, coarse_mode=capi.COARSE_FIXED, coarse_maxit=3, outer_pre_gs=0, **kw)
        with capi.Solver(d) as s:
            assert s.subcycle_root() == -1   # a V handle keeps its launches unless MG_SUBCYCLE_LEVEL says otherwise
            # one handle of the sweep works on sigma I + A
            if shape["id"] == "3d-17-L3-f64" and smoother == capi.SMOOTH_RBGS and restriction == capi.RESTRICT_INJECT:
                s.set_shift(3.0)
            rng = np.random.default_rng(kw["n"] + 7 * restriction)
            u = rng.standard_normal(s.level_shape(root)).astype(dt)
            b = rng.standard_normal(s.level_shape(root)).astype(dt)
            for kind in KINDS:
                (st0, u0), (st1, u1) = both_paths(s, root, kind, u, b)
                what = (shape["id"], sm[0], restriction, KNAME[kind])
                assert st0.coarse_iters == st1.coarse_iters == 3 * coarse_solves(kind, kw["levels"] - root), what
                assert np.isfinite(u0).all() and not np.array_equal(u0, u), what
                assert np.array_equal(u0, u1), (what, float(np.abs(u0.astype(LD) - u1).max()))


TOL_CASES = [
    dict(id="3d-jacobi", dim=3, n=33, levels=4, dtype=capi.MG_F64, smoother=capi.SMOOTH_JACOBI, omega=6 / 7, nu_pre=2, nu_post=2,
         restriction=capi.RESTRICT_FULLW),
    dict(id="2d-rbgs", dim=2, n=33, levels=4, dtype=capi.MG_F64, smoother=capi.SMOOTH_RBGS, omega=1.0, nu_pre=1, nu_post=1,
         restriction=capi.RESTRICT_INJECT),
]


@pytest.mark.parametrize("case", TOL_CASES, ids=[c["id"] for c in TOL_CASES])
def test_kernel_and_launches_stop_alike_in_tolerance_mode(case):
    """MG_COARSE_TOL: the two paths sum their norms in different orders, which can move a stop only when a norm is within
    rounding of coarse_tol. The seed is the first one whose reference run keeps every deciding norm at least 1e-6 (relative)
    away from it; then the sweep counts and the bits must agree."""
    kw = {k: v for k, v in case.items() if k != "id"}
    tol, maxit, root, kind = 0.1, 200, 1, capi.CYCLE_W
    P = nc.CycleProblem(cycle=kind, length=1.0, alpha=1.0, prec=np.float64, **kw)
    for seed in range(20):
        rng = np.random.default_rng(seed)
        u = rng.standard_normal(P.shape(root)); b = rng.standard_normal(P.shape(root))
        P.tol, P.tol_sweeps, P.tol_margin = tol, [], float("inf")
        P.vcycle(u, b, maxit, root, kind)
        if P.tol_margin >= 1e-6:
            break
    else:
        pytest.fail("no seed keeps the coarse norms away from the tolerance")
    d = capi.make_desc(length=1.0, alpha=1.0, cycle=capi.CYCLE_V, coarse_mode=capi.COARSE_TOL, coarse_tol=tol, coarse_maxit=maxit,
                       outer_pre_gs=0, **kw)
    with capi.Solver(d) as s:
        (st0, u0), (st1, u1) = both_paths(s, root, kind, u, b)
    print(f"{case['id']}: seed {seed} margin {P.tol_margin:.2e} reference sweeps {P.tol_sweeps} launches {st0.coarse_iters} kernel {st1.coarse_iters}")
    assert st0.coarse_iters == st1.coarse_iters == sum(P.tol_sweeps)
    assert st0.coarse_flag == st1.coarse_flag == 0
    assert np.array_equal(u0, u1)


# ======================================================================= 2. whole cycles against the reference
CYCLE_SHAPES = [
    dict(id="3d-65-L5-jacobi-f64", dim=3, n=65, levels=5, dtype=capi.MG_F64, smoother=capi.SMOOTH_JACOBI, omega=6 / 7,
         nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW),   # brick kernels on 65^3 and 33^3, the kernel root at 17^3
    dict(id="3d-33-L4-rbgs-f32", dim=3, n=33, levels=4, dtype=capi.MG_F32, smoother=capi.SMOOTH_RBGS, omega=1.0,
         nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW),
    dict(id="2d-129-L6-jacobi-f64", dim=2, n=129, levels=6, dtype=capi.MG_F64, smoother=capi.SMOOTH_JACOBI, omega=6 / 7,
         nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW),
]
CM = 4   # fixed coarse sweeps


def visit_factor(P, kind):
    return sum(nc.expected_visits(kind, P.L)) / P.L


def run_cycles_and_solve(kw, kind, P, b, u0, refs, root_expected):
    """two mg_cycle calls and a three-iteration mg_solve on one handle -> the arrays and histories, each checked against refs"""
    eps = eps_of(kw["dtype"])
    dt = np_of(kw["dtype"])
    out = []
    with capi.Solver(capi.make_desc(**kw)) as s:
        assert s.subcycle_root() == root_expected
        s.set_rhs(b); s.set_solution(u0)
        for k in range(2):
            st = s.cycle()
            assert st.coarse_iters == CM * coarse_solves(kind, P.L) and st.coarse_flag == 0 and st.fine_sumsq_r == 0
            u = s.get_solution()
            scale = float(np.abs(refs["cycle"][k]).max()) + sweep_scale(P, 0, b, u0)
            check_max(u, refs["cycle"][k], visit_factor(P, kind) * cycle_bound(P, eps, CM, scale), f"cycle {k}")
            out.append(u)
        s.set_solution(np.zeros(P.shape(0), dt))
        hist, stats = s.solve(1e-30, 3)
        uref, href = refs["solve"]
        assert len(hist) == len(href) == 4 and [t.coarse_iters for t in stats] == [CM * coarse_solves(kind, P.L)] * 3
        scale = float(np.abs(uref).max()) + float(np.abs(b).max()) / float(abs(P.coef(0)[1]))
        dmax = 3 * visit_factor(P, kind) * cycle_bound(P, eps, CM, scale)
        usol = s.get_solution()
        check_max(usol, uref, dmax, "solve")
        nb = math.sqrt(npr.fsum_sq(b))
        mag = math.sqrt(npr.fsum_sq(np.abs(P.as_prec(b)) + P.apply_A(uref, 0, absolute=True)))
        atol = (C_RESID * eps * mag + 2 * float(abs(P.coef(0)[1])) * dmax * math.sqrt(b.size)) / nb
        np.testing.assert_allclose(hist, href, rtol=1e-9, atol=atol)
        out += [usol, hist]
    return out


@pytest.mark.parametrize("kind", [capi.CYCLE_W, capi.CYCLE_F], ids=["W", "F"])
@pytest.mark.parametrize("shape", CYCLE_SHAPES, ids=[s["id"] for s in CYCLE_SHAPES])
def test_cycles_and_solve_against_the_reference(shape, kind):
    kw = dict(shape_kw(shape), length=1.0, alpha=1.0, cycle=kind, coarse_mode=capi.COARSE_FIXED, coarse_maxit=CM, outer_pre_gs=0)
    dt = np_of(kw["dtype"])
    P = nc.CycleProblem(prec=LD if kw["n"] <= 129 else np.float64, **kw)
    rng = np.random.default_rng(kw["n"] + 3)
    b = rng.standard_normal(P.shape(0)).astype(dt)
    u0 = (0.1 * rng.standard_normal(P.shape(0))).astype(dt)
    refs = {"cycle": []}
    u = P.as_prec(u0)
    for k in range(2):
        u = P.cycle(u, b, CM)
        refs["cycle"].append(u)
    refs["solve"] = P.solve(np.zeros(P.shape(0)), b, [CM] * 3)
    finest = planned_root(kw["dim"], kw["n"], kw["levels"], kw["dtype"])
    with_kernel = run_cycles_and_solve(kw, kind, P, b, u0, refs, default_root(finest, kw["levels"]))
    # the same with the kernel rooted at the finest admissible level (17^3, 17^3, 65^2) and with the kernel off
    # (MG_SUBCYCLE_LEVEL is read when the handle is created): the same bits
    old = os.environ.get("MG_SUBCYCLE_LEVEL")
    try:
        for setting, root in ((finest, finest), (kw["levels"], -1)):
            os.environ["MG_SUBCYCLE_LEVEL"] = str(setting)
            other = run_cycles_and_solve(kw, kind, P, b, u0, refs, root)
            for a, c in zip(with_kernel, other):
                assert np.array_equal(a, c), setting
    finally:
        if old is None:
            del os.environ["MG_SUBCYCLE_LEVEL"]
        else:
            os.environ["MG_SUBCYCLE_LEVEL"] = old


def test_a_forced_root_serves_a_v_handle_too():
    """MG_SUBCYCLE_LEVEL = k >= 1 hands root k to the kernel for V handles as well: the V-cycle's bits, one launch below level 1"""
    kw = dict(dim=3, n=33, levels=4, dtype=capi.MG_F64, length=1.0, alpha=1.0, cycle=capi.CYCLE_V, smoother=capi.SMOOTH_JACOBI,
              omega=6 / 7, nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW, coarse_mode=capi.COARSE_FIXED, coarse_maxit=CM,
              outer_pre_gs=0)
    b = np.random.default_rng(1).standard_normal((33,) * 3)
    res = []
    for env in (None, "2", "1", "0"):
        old = os.environ.pop("MG_SUBCYCLE_LEVEL", None)
        if env is not None:
            os.environ["MG_SUBCYCLE_LEVEL"] = env
        try:
            with capi.Solver(capi.make_desc(**kw)) as s:
                assert s.subcycle_root() == {None: -1, "2": 2, "1": 1, "0": -1}[env]
                s.set_rhs(b); s.set_solution(np.zeros_like(b))
                st = s.cycle(); s.cycle()
                assert st.coarse_iters == CM
                res.append(s.get_solution())
        finally:
            os.environ.pop("MG_SUBCYCLE_LEVEL", None)
            if old is not None:
                os.environ["MG_SUBCYCLE_LEVEL"] = old
    assert all(np.array_equal(res[0], r) for r in res[1:])


# ======================================================================= 3. W does what V cannot
@pytest.mark.parametrize("case", WEAK_CASES, ids=["3d-33", "2d-65"])
def test_w_converges_where_v_diverges(case):
    eps = eps_of(capi.MG_F64)
    rates = {}
    for kind in KINDS:
        P, b, uref, href = weak_history(case, kind)
        rates[kind] = rate(href)
        kw = dict(WEAK, dtype=capi.MG_F64, cycle=kind, coarse_mode=capi.COARSE_FIXED, coarse_maxit=2, **case)
        with capi.Solver(capi.make_desc(**kw)) as s:
            s.set_rhs(b); s.set_solution(np.zeros_like(b))
            hist, stats = s.solve(1e-30, 6)
            u = s.get_solution()
        assert len(hist) == 7 and [t.coarse_iters for t in stats] == [2 * coarse_solves(kind, P.L)] * 6
        scale = float(np.abs(uref).max()) + float(np.abs(b).max()) / float(abs(P.coef(0)[1]))
        dmax = 6 * visit_factor(P, kind) * cycle_bound(P, eps, 2, scale)
        print(f"{case} {KNAME[kind]}: rate {rates[kind]:.3f} (device {float((hist[6] / hist[2]) ** 0.25):.3f}) "
              f"max error {float(np.abs(u.astype(LD) - uref).max()):.3e} bound {dmax:.3e}")
        check_max(u, uref, dmax, f"solve {KNAME[kind]}")
        nb = math.sqrt(npr.fsum_sq(b))
        mag = math.sqrt(npr.fsum_sq(np.abs(P.as_prec(b)) + P.apply_A(uref, 0, absolute=True)))
        atol = (C_RESID * eps * mag + 2 * float(abs(P.coef(0)[1])) * dmax * math.sqrt(b.size)) / nb
        np.testing.assert_allclose(hist, href, rtol=1e-9, atol=atol)
    assert rates[capi.CYCLE_V] > 1 and rates[capi.CYCLE_W] < 0.8
    if case["dim"] == 3:
        assert rates[capi.CYCLE_F] < 0.8


# ======================================================================= 4. the drivers compose
J33 = dict(dim=3, n=33, levels=4, length=1.0, alpha=1.0, smoother=capi.SMOOTH_JACOBI, omega=6 / 7, nu_pre=2, nu_post=2,
           restriction=capi.RESTRICT_FULLW, coarse_mode=capi.COARSE_FIXED, coarse_maxit=8, outer_pre_gs=0)


@pytest.mark.parametrize("kind", [capi.CYCLE_W, capi.CYCLE_F], ids=["W", "F"])
def test_fmg_runs_the_descriptors_kind(kind):
    kw = dict(J33, dtype=capi.MG_F64, cycle=kind)
    P = nc.CycleProblem(prec=LD, **kw)
    b = np.random.default_rng(33).standard_normal(P.shape(0))
    ref = nf.fmg(P, b, 1, 8)
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_rhs(b)
        st = s.fmg(1)
        u = s.get_solution()
    assert (st.levels, st.cycles_per_level, st.coarse_iters, st.coarse_flag) == (4, 1, 8, 0)
    bound = FMG_K * cycle_bound(P, eps_of(capi.MG_F64), 8, fmg_scale(P, b, ref))
    print(f"fmg {KNAME[kind]}: err {float(np.abs(u.astype(LD) - ref).max()):.3e} bound {bound:.3e}")
    check_max(u, ref, bound, "fmg(1)")
    # not the V-cycle's pass
    refv = nf.fmg(nc.CycleProblem(prec=LD, **dict(kw, cycle=capi.CYCLE_V)), b, 1, 8)
    assert float(np.abs(refv - ref).max()) > 100 * bound


def test_pcg_with_a_w_cycle_needs_no_more_iterations():
    b = np.random.default_rng(7).standard_normal((33,) * 3)
    iters = {}
    for kind in (capi.CYCLE_V, capi.CYCLE_W):
        with capi.Solver(capi.make_desc(**dict(J33, dtype=capi.MG_F64, cycle=kind))) as s:
            s.set_rhs(b); s.set_solution(np.zeros_like(b))
            hist, st = s.pcg_solve(1e-10, 60)
            assert st.status == capi.PCG_CONVERGED and hist[-1] <= 1e-10, (KNAME[kind], st.status, hist[-1])
            iters[kind] = st.iters
    print(f"pcg iterations: V {iters[capi.CYCLE_V]} W {iters[capi.CYCLE_W]}")
    assert iters[capi.CYCLE_W] <= iters[capi.CYCLE_V]


def test_heat_mixed_and_o4_run_on_a_w_handle():
    b = np.random.default_rng(9).standard_normal((33,) * 3)
    with capi.Solver(capi.make_desc(**dict(J33, dtype=capi.MG_F64, cycle=capi.CYCLE_W))) as s:
        s.set_solution(b)
        st = s.heat_step(1e-3, 1.0, 2, 2)
        assert st.steps == 2 and st.cycles == 4 and np.isfinite(st.relres) and st.relres < 1
        assert np.isfinite(s.get_solution()).all()
    with capi.Solver(capi.make_desc(**dict(J33, dtype=capi.MG_F64, cycle=capi.CYCLE_W))) as s:
        s.set_rhs(b); s.set_solution(np.zeros_like(b))
        hist, st = s.o4_solve(1e-30, 5, 1)
        assert st.status == capi.O4_MAXIT and len(hist) == 6 and np.isfinite(hist).all() and (np.diff(hist) < 0).all(), hist
    with capi.Solver(capi.make_desc(**dict(J33, dtype=capi.MG_F32, cycle=capi.CYCLE_W))) as s:
        s.mixed_set_rhs(b); s.mixed_set_solution(np.zeros_like(b))
        hist, st = s.mixed_solve(1e-30, 4, 2)
        assert st.status == capi.MIXED_MAXIT and len(hist) == 5 and np.isfinite(hist).all() and (np.diff(hist) < 0).all(), hist


# ======================================================================= 5. contract and refusals
def test_refusals_leave_u_untouched():
    kw = dict(J33, dtype=capi.MG_F64)

    def refused(s, level, kind, path, arr_level=1):
        s.set_array(capi.ARR_U, arr_level, np.random.default_rng(2).standard_normal(s.level_shape(arr_level)))
        before = s.get_array(capi.ARR_U, arr_level)
        with pytest.raises(capi.MgError) as e:
            s.subcycle(level, kind, path)
        assert e.value.code == -4 and "mg_subcycle" in str(e.value), str(e.value)   # MG_ERR_BAD_ARG
        assert np.array_equal(s.get_array(capi.ARR_U, arr_level), before)

    with capi.Solver(capi.make_desc(**dict(kw, cycle=capi.CYCLE_SAWTOOTH, nu_pre=0))) as s:
        assert s.subcycle_root() == -1
        refused(s, 1, capi.CYCLE_V, 0)
        with pytest.raises(capi.MgError) as e:
            s.fmg(1)
        assert e.value.code == -4 and "MG_CYCLE_V" in str(e.value)
    with capi.Solver(capi.make_desc(**dict(kw, cycle=capi.CYCLE_V))) as s:
        assert s.subcycle_root() == -1
        refused(s, 1, 0, 0)            # unknown kinds
        refused(s, 1, 4, 1)
        refused(s, 0, capi.CYCLE_W, 1)  # level 0 is never resident
        refused(s, 3, capi.CYCLE_W, 1)  # nor the coarsest alone
        refused(s, 4, capi.CYCLE_W, 0)  # levels that do not exist
        refused(s, -1, capi.CYCLE_W, 0)
        refused(s, 1, capi.CYCLE_W, 2)  # unknown path
    with capi.Solver(capi.make_desc(**dict(kw, cycle=capi.CYCLE_W, smoother=capi.SMOOTH_GS_LEX))) as s:
        assert s.subcycle_root() == -1  # lexicographic Gauss-Seidel: launches only
        refused(s, 1, capi.CYCLE_W, 1)
        assert s.subcycle(1, capi.CYCLE_W, 0).coarse_iters == 16
    with capi.Solver(capi.make_desc(**dict(kw, n=65, levels=3, cycle=capi.CYCLE_W))) as s:
        assert s.subcycle_root() == -1  # 33^3 does not fit
        refused(s, 1, capi.CYCLE_W, 1)


@pytest.mark.parametrize("kind", [capi.CYCLE_W, capi.CYCLE_F], ids=["W", "F"])
def test_distributed_handles_refuse_w_and_f(kind):
    d = capi.make_desc(**dict(J33, n=129, levels=4, dtype=capi.MG_F64, cycle=kind))
    with pytest.raises(capi.MgError) as e:
        capi.Solver(d, rank=0, nranks=2, dry=True)
    assert e.value.code == -1 and "single-GPU" in str(e.value), str(e.value)   # MG_ERR_INVALID_DESC
    capi.Solver(capi.make_desc(**dict(J33, n=129, levels=4, dtype=capi.MG_F64, cycle=capi.CYCLE_V)), rank=0, nranks=2, dry=True).close()


def test_cli_cycle_w(tmp_path):
    exe = mgbuild.build_cli()
    hists = {}
    for k in ("v", "w", "f"):
        rc, out = run_cli(exe, f"-n 33 -a 1 -w 1 -ml 4 -test 0 -smt 1 -dim 3 -cycle {k} -rbgs -nu1 1 -nu2 1 -coarse_fixed 2 -maxit 4".split(), tmp_path)
        assert rc == 0, out
        hists[k] = [float(x) for x in open(tmp_path / "MGGS4.txt").read().split()][1:]
        assert len(hists[k]) == 5 and np.isfinite(hists[k]).all()
    assert hists["w"] != hists["v"] and hists["f"] != hists["v"]
