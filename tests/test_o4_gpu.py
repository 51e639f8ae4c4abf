"""Fourth-order defect correction (mg_o4_residual, mg_o4_correct_residual, mg_o4_solve; include/mg_hip.h) on the GPU.

* kernel level: both kernels of mg_o4.hip, in both forms (marching tile / plain), bit for bit against the contract restated
  in numpy (tests/o4_ref.py);
* the driver on a manufactured problem: fourth order, the gain over mg_solve on the same grid, the outer contraction;
* contracts: RHS unchanged, memory, determinism, refusals, non-finite and zero right-hand sides.

Corrections mg_o4_solve(tol = 1e-10, from u = 0) took on an MI355X (printed by test_driver_fourth_order), inner_cycles 1 / 2:
  3-D V(2,2) red-black    n = 17: 20 / 20   n = 33: 21 / 21
  3-D V(2,2) Jacobi 6/7   n = 17: 23 / 19   n = 33: 26 / 21
  2-D sawtooth            n = 33: 27 / 21   n = 65: 27 / 22
Worst contraction from the third correction on: 0.32 - 0.34 (0.47 for the 2-D sawtooth cycle with inner_cycles = 1); errors
e4(17) = 1.794e-6, e4(33) = 1.300e-7 (ratio 13.80; 2-D 33 / 65: 15.5), e2(33) / e4(33) = 1763: the figures of the exact inner solve.
"""
import functools

import numpy as np
import pytest

from multigrid_prj_amd import capi
from tests import o4_ref as o4

pytestmark = pytest.mark.gpu

NP = {capi.MG_F64: np.float64, capi.MG_F32: np.float32}
U, E, RHS, TMP, RES = capi.ARR_U, capi.ARR_E, capi.ARR_RHS, capi.ARR_TMP, capi.ARR_RES


def case_id(c):
    dim, n, levels, extra = c
    return f"{dim}d{n}" + "".join("-" + k for k in extra) + ("-L4" if levels == 4 else "")


# ---------------------------------------------------------------- kernel level
@pytest.mark.parametrize("dtype", [capi.MG_F64, capi.MG_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", o4.KERNEL_CASES, ids=case_id)
def test_kernels_bit_for_bit(case, dtype):
    dim, n, levels, extra = case
    rng = np.random.default_rng(1000 * dim + n)
    kw = dict(dim=dim, n=n, levels=levels, length=1.0, alpha=1.3, dtype=dtype, **extra)
    with capi.Solver(capi.make_desc(**kw)) as s:
        shape = s.level_shape(0)
        T = s.np
        assert s.level_coefficients(0)[:3] == o4.level0_coef(dim, n, 1.0, 1.3, extra.get("aniso", (1.0, 1.0, 1.0)))[:3]
        bnd = o4.boundary_mask(shape)
        u, b, other = (rng.standard_normal(shape).astype(T) for _ in range(3))
        e = (rng.standard_normal(shape) * 0.1).astype(T)
        e[bnd] = np.where(rng.random(int(bnd.sum())) < 0.5, np.nan, 1e30).astype(T)   # garbage where e is not looked at
        for sigma in (0.0, 500.0):
            s.set_shift(sigma)
            coef = s.level_coefficients(0)
            assert coef[3] == o4.level0_coef(dim, n, 1.0, 1.3, extra.get("aniso", (1.0, 1.0, 1.0)))[3] + sigma
            # the residual, saved and norm only
            r_ref = o4.residual_np(u, b, coef, sigma)
            ss_ref = o4.sumsq(r_ref)
            s.set_array(E, 0, u); s.set_array(RHS, 0, b); s.set_array(RES, 0, other)
            ss = s.o4_residual(E, RHS, RES)
            got = s.get_array(RES, 0)
            side = o4.kernel_side(dim, n, np.dtype(T).itemsize)
            assert np.array_equal(got, r_ref), (side, sigma, int((got != r_ref).sum()))
            assert ss == pytest.approx(ss_ref, rel=1e-13) and s.o4_residual(E, RHS, -1) == ss
            assert np.array_equal(s.get_array(E, 0), u) and np.array_equal(s.get_array(RHS, 0), b)
            # the fused correction + residual
            un_ref = o4.correct_np(u, e)
            r2_ref = o4.residual_np(un_ref, b, coef, sigma)
            s.set_array(U, 0, u); s.set_array(E, 0, e); s.set_array(TMP, 0, other); s.set_array(RES, 0, other)
            ss2 = s.o4_correct_residual(U, E, RHS, TMP, RES)
            got_u, got_r = s.get_array(TMP, 0), s.get_array(RES, 0)
            assert np.array_equal(got_u, un_ref), (side, sigma, int((got_u != un_ref).sum()))
            assert np.array_equal(got_r, r2_ref), (side, sigma, int((got_r != r2_ref).sum()))
            assert ss2 == pytest.approx(o4.sumsq(r2_ref), rel=1e-13)
            assert np.array_equal(s.get_array(U, 0), u) and np.array_equal(s.get_array(RHS, 0), b)
            assert np.array_equal(s.get_array(E, 0), e, equal_nan=True)
            # the fused pass is the correction followed by the residual, and the residual of its output
            assert s.o4_residual(TMP, RHS, -1) == pytest.approx(ss2, rel=1e-13)


@pytest.mark.parametrize("dtype", [capi.MG_F64, capi.MG_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("dim,n", [(3, 33), (3, 65), (3, 67), (2, 129)])
@pytest.mark.parametrize("fused", [False, True], ids=["residual", "fused"])
def test_outputs_feed_the_other_kernels(fused, dim, n, dtype):
    """What mg_o4_residual / mg_o4_correct_residual leave in the handle's arrays is what an upload of the same values
    leaves, as far as the other kernels can tell: sweeps and a residual run on the outputs give the bits they give on a
    twin handle whose arrays were uploaded.
    That the padding columns (x >= nx) stay zero and the ghost planes untouched is checked in tests/test_storage_gpu.py
    (rows o4-residual and o4-correct-residual of tests/storage_table.py), on the whole allocations."""
    rng = np.random.default_rng(n)
    kw = dict(dim=dim, n=n, levels=2, length=1.0, dtype=dtype, cycle=capi.CYCLE_V, smoother=capi.SMOOTH_JACOBI, omega=6.0 / 7.0,
              nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW, outer_pre_gs=0)
    with capi.Solver(capi.make_desc(**kw)) as a, capi.Solver(capi.make_desc(**kw)) as t:
        shape = a.level_shape(0)
        u, e, b = (rng.standard_normal(shape).astype(a.np) for _ in range(3))
        if fused:
            a.set_array(TMP, 0, u); a.set_array(E, 0, e); a.set_array(RES, 0, b)
            a.o4_correct_residual(TMP, E, RES, U, RHS)
        else:
            a.set_array(U, 0, u); a.set_array(RES, 0, b)
            a.o4_residual(U, RES, RHS)
        t.set_array(U, 0, a.get_array(U, 0)); t.set_array(RHS, 0, a.get_array(RHS, 0))
        for s in (a, t):
            s.smooth(0, capi.SMOOTH_JACOBI, 2, U, RHS)
            s.smooth(0, capi.SMOOTH_RBGS, 1, U, RHS)
        assert np.array_equal(a.get_array(U, 0), t.get_array(U, 0))
        assert a.residual(0, U, RHS, E) == t.residual(0, U, RHS, E)
        assert np.array_equal(a.get_array(E, 0), t.get_array(E, 0))


# ---------------------------------------------------------------- the driver
V22 = dict(cycle=capi.CYCLE_V, nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW, outer_pre_gs=0, coarse_tol=1e-10)
CYCLES = {
    "v22-rb": dict(dim=3, smoother=capi.SMOOTH_RBGS, **V22),
    "v22-jacobi": dict(dim=3, smoother=capi.SMOOTH_JACOBI, omega=6.0 / 7.0, **V22),
    "2d-sawtooth": dict(dim=2),   # the reference's own cycle: make_desc's defaults
}
SIZES = {"v22-rb": (17, 33), "v22-jacobi": (17, 33), "2d-sawtooth": (33, 65)}


def levels_for(n):
    return int(np.log2(n - 1)) - 1   # coarsest grid: 5 nodes per axis


@functools.lru_cache(maxsize=None)
def driver_run(cycle, n, inner):
    kw = dict(CYCLES[cycle], n=n, levels=levels_for(n), length=1.0)
    M = o4.Manufactured(kw["dim"], n)
    b = np.asarray(M.b, np.float64)
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_rhs(b); s.set_solution(np.zeros_like(b))
        bytes0 = s.device_bytes()
        hist, st = s.o4_solve(1e-10, 60, inner)
        bytes1 = s.device_bytes()
        u4 = s.get_solution()
        rhs_after = s.get_array(RHS, 0)
        rel_check = float(np.sqrt(s.o4_residual(U, RHS, -1) / s.sumsq(0, RHS)))
        s.set_solution(np.zeros_like(b))
        hist_b, st_b = s.o4_solve(1e-10, 60, inner)
        bytes2 = s.device_bytes()
        s.set_solution(np.zeros_like(b))
        h2, _ = s.solve(1e-11, 200)
        u2 = s.get_solution()
    pitch = -(-n // 16) * 16
    one = ((n + 2) if kw["dim"] == 3 else 3) * n * pitch * 8
    return dict(M=M, b=b, hist=hist, st=(st.outer, st.cycles, st.status, st.relres), u4=u4, rhs_after=rhs_after, rel_check=rel_check,
                hist_b=hist_b, e4=M.err(u4), e2=M.err(u2), h2=h2, grew=(bytes1 - bytes0, bytes2 - bytes1), one=one)


@pytest.mark.parametrize("inner", [1, 2])
@pytest.mark.parametrize("cycle", list(CYCLES))
def test_driver_fourth_order(cycle, inner):
    small, large = (driver_run(cycle, n, inner) for n in SIZES[cycle])
    for n, R in zip(SIZES[cycle], (small, large)):
        outer, cycles, status, relres = R["st"]
        hist = R["hist"]
        rho = [hist[k + 1] / hist[k] for k in range(2, len(hist) - 1)]
        print(f"{cycle} n={n} inner={inner}: corrections {outer} status {status} relres {relres:.3e} e4 {R['e4']:.3e} e2 {R['e2']:.3e} "
              f"e2/e4 {R['e2'] / R['e4']:.0f} mg_solve cycles {len(R['h2']) - 1} contractions from the third: max {max(rho):.3f}")
        assert status == capi.O4_CONVERGED and outer == len(hist) - 1 and cycles == inner * outer and outer <= 60
        assert relres == hist[-1] and relres <= 1e-10
        assert all(hist[k + 1] <= hist[k] for k in range(1, len(hist) - 1)), hist
        assert R["rel_check"] == pytest.approx(relres, rel=1e-12)
        assert R["e4"] <= R["e2"] / 100
        if inner == 2:
            assert max(rho) <= 0.4, rho
    print(f"{cycle} inner={inner}: e4({SIZES[cycle][0]}) / e4({SIZES[cycle][1]}) = {small['e4'] / large['e4']:.2f}")
    assert small["e4"] / large["e4"] >= 10


@pytest.mark.parametrize("cycle,n", [("v22-rb", 17), ("v22-jacobi", 33), ("2d-sawtooth", 65)])
def test_driver_contracts(cycle, n):
    R = driver_run(cycle, n, 1)
    assert np.array_equal(R["rhs_after"], R["b"])                       # RHS(0) holds b, bit for bit
    assert R["grew"] == (3 * R["one"], 0)                               # b4 and two copies of u4, once
    assert np.array_equal(R["hist"], R["hist_b"])                       # two runs, the same bits
    assert np.array_equal(R["u4"][o4.boundary_mask(R["b"].shape)], R["b"][o4.boundary_mask(R["b"].shape)])


def test_fp32_reaches_its_floor():
    """status 0 or 1, never 2; the floor: an fp32 evaluation of r is off by at most C eps |A4||u| per node (C_ROUND of
    tests/test_o4_cpu.py: 16 roundings on any path) and the iterate by one rounding of u, another eps |A4||u|: twice that"""
    n = 33
    kw = dict(CYCLES["v22-rb"], n=n, levels=levels_for(n), length=1.0, dtype=capi.MG_F32)
    M = o4.Manufactured(3, n)
    b = np.asarray(M.b, np.float32)
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_rhs(b); s.set_solution(np.zeros_like(b))
        hist, st = s.o4_solve(1e-10, 30, 1)
        u = s.get_solution()
        mag = np.asarray(o4.a4_mag(u.astype(np.longdouble), s.level_coefficients(0), 0.0))
        floor = 2 * 16 * float(np.finfo(np.float32).eps) * float(np.sqrt(np.sum(mag * mag) / o4.sumsq(b)))
        print("fp32 hist", ["%.2e" % h for h in hist], "status", st.status, "floor bound %.2e" % floor, "error %.2e" % M.err(u))
        assert st.status in (capi.O4_CONVERGED, capi.O4_MAXIT) and np.isfinite(hist).all() and np.isfinite(u).all()
        assert st.relres <= floor


def test_refusals_leave_u_untouched():
    rng = np.random.default_rng(2)
    n = 17
    kw = dict(CYCLES["v22-rb"], n=n, levels=3, length=1.0)
    with capi.Solver(capi.make_desc(**kw)) as s:
        shape = s.level_shape(0)
        u0, b = rng.standard_normal(shape), rng.standard_normal(shape)
        s.set_solution(u0); s.set_rhs(b)
        for call, word in ((lambda: s.o4_solve(1e-8, 10, 0), "inner_cycles"), (lambda: s.o4_solve(1e-8, -1, 1), "maxit"),
                           (lambda: s.o4_residual(U, RHS, U), "output"), (lambda: s.o4_correct_residual(U, E, RHS, TMP, TMP), "distinct")):
            with pytest.raises(capi.MgError) as e:
                call()
            assert e.value.code == -4 and word in str(e.value)
            assert np.array_equal(s.get_solution(), u0) and np.array_equal(s.get_array(RHS, 0), b)
        s.set_stage_callback(lambda *a: None)
        with pytest.raises(capi.MgError) as e:
            s.o4_solve(1e-8, 10, 1)
        assert e.value.code == -4 and "stage callback" in str(e.value)
        assert np.array_equal(s.get_solution(), u0)
        s.set_stage_callback(None)
        before = s.device_bytes()
        assert s.o4_solve(1e-8, 2, 1)[1].status in (0, 1)
        assert s.device_bytes() > before
    assert capi.load().mg_o4_solve(None, 1e-8, 10, 1, None, 0, None, None) == -4
    assert capi.load().mg_o4_residual(None, U, RHS, -1, None) == -4
    assert capi.load().mg_o4_correct_residual(None, U, E, RHS, TMP, RES, None) == -4
    # n < 7
    with capi.Solver(capi.make_desc(dim=3, n=5, levels=2, length=1.0)) as s:
        u0 = rng.standard_normal(s.level_shape(0)); s.set_solution(u0)
        for call in (lambda: s.o4_solve(1e-8, 10, 1), lambda: s.o4_residual(U, RHS, -1), lambda: s.o4_correct_residual(U, E, RHS, TMP, RES)):
            with pytest.raises(capi.MgError) as e:
                call()
            assert e.value.code == -4 and "n >= 7" in str(e.value)
        assert np.array_equal(s.get_solution(), u0)
    # distributed handles, the dry-run measurement handle included
    with capi.Solver(capi.make_desc(dim=3, n=33, levels=3, length=1.0), device=0, rank=0, nranks=2, dry=True) as s:
        u0 = rng.standard_normal(s.level_shape(0)); s.set_solution(u0)
        before = s.device_bytes()
        for call in (lambda: s.o4_solve(1e-8, 10, 1), lambda: s.o4_residual(U, RHS, -1)):
            with pytest.raises(capi.MgError) as e:
                call()
            assert e.value.code == -4 and "distributed" in str(e.value)
        assert np.array_equal(s.get_solution(), u0) and s.device_bytes() == before


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_rhs_gives_status_2(bad):
    n = 17
    kw = dict(CYCLES["v22-rb"], n=n, levels=3, length=1.0)
    rng = np.random.default_rng(3)
    with capi.Solver(capi.make_desc(**kw)) as s:
        shape = s.level_shape(0)
        u0, b = rng.standard_normal(shape), rng.standard_normal(shape)
        b[n // 2, n // 2, 3] = bad
        s.set_solution(u0); s.set_rhs(b)
        hist, st = s.o4_solve(1e-8, 10, 1)
        assert st.status == capi.O4_NOT_FINITE and st.outer == 0 and len(hist) == 1 and not np.isfinite(hist[0])
        assert np.isfinite(s.get_solution()).all() and np.array_equal(s.get_solution(), u0)
        assert np.array_equal(s.get_array(RHS, 0), b, equal_nan=True)


def test_zero_rhs_needs_no_correction():
    kw = dict(CYCLES["v22-jacobi"], n=17, levels=3, length=1.0)
    with capi.Solver(capi.make_desc(**kw)) as s:
        z = np.zeros(s.level_shape(0))
        s.set_solution(z); s.set_rhs(z)
        hist, st = s.o4_solve(1e-8, 10, 1)
        assert (st.status, st.outer, st.cycles, st.relres) == (0, 0, 0, 0.0) and list(hist) == [0.0]
        assert not s.get_solution().any() and not s.get_array(RHS, 0).any()
