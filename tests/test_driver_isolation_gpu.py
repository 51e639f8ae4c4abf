"""The solve drivers share one preamble (Solver::driver_begin), one outer iteration (outer_iteration_enqueue) and one pinned
scalar buffer with named slots (mg_drivers.cpp, mg_solver.h): nothing one driver leaves behind may reach the next.

Every driver runs in sequence on ONE handle, each from the same initial u and b, and is compared bit for bit -- history,
stats struct and returned solution -- with the same call on a fresh handle created for that call alone. The comparison is
to the library itself, so it needs no tolerance. 3-D n = 33 with 3 levels is the smallest size at which every level type of
the cycle exists: level 0 (33) takes the streaming-sweep path, level 1 (17) is launch-bound, level 2 (9) is the LDS coarse
solve. (The fused-norm loop of mg_solve needs 257^3 and above: tests/test_gpu_parity.py runs it.)
"""
import numpy as np
import pytest

from multigrid_prj_amd import capi

pytestmark = pytest.mark.gpu

NP = {capi.MG_F64: np.float64, capi.MG_F32: np.float32}
SMOOTHERS = {"jacobi": dict(smoother=capi.SMOOTH_JACOBI, omega=6 / 7), "rbgs": dict(smoother=capi.SMOOTH_RBGS, omega=1.0)}
DT = 1e-3


def raw(x):
    """the bits of a history, a solution, a stats struct or a list of stats structs"""
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, float):
        return np.float64(x).tobytes()
    if isinstance(x, (list, tuple)):
        return tuple(raw(v) for v in x)
    return bytes(x)


# name -> call(handle, u0, b) -> everything the call returns, the solution included
def run_solve(s, u0, b):
    s.set_solution(u0); s.set_rhs(b)
    hist, stats = s.solve(1e-11, 3)
    return hist, stats, s.get_solution()


def run_pcg(s, u0, b):
    s.set_solution(u0); s.set_rhs(b)
    hist, st = s.pcg_solve(1e-11, 3)
    return hist, st, s.get_solution()


def run_mixed(s, u0, b):
    s.mixed_set_rhs(b.astype(np.float64)); s.mixed_set_solution(u0.astype(np.float64))
    hist, st = s.mixed_solve(1e-11, 2, 1)
    return hist, st, s.mixed_get_solution()


def run_fmg(s, u0, b):
    s.set_solution(u0); s.set_rhs(b)
    st = s.fmg(1)
    return st, s.get_solution()


def run_heat(s, u0, b):
    s.set_solution(u0); s.set_rhs(b)
    st = s.heat_step(DT, 1.0, 2, 1)
    out = st, s.get_solution(), s.get_shift()
    s.set_shift(0.0)
    return out


@pytest.mark.parametrize("pre_gs", [0, 2], ids=["gs0", "gs2"])
@pytest.mark.parametrize("dtype", [capi.MG_F64, capi.MG_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("sm", list(SMOOTHERS))
def test_drivers_in_sequence_equal_fresh_handles(sm, dtype, pre_gs):
    kw = dict(dim=3, n=33, levels=3, length=1.0, alpha=1.0, dtype=dtype, cycle=capi.CYCLE_V, nu_pre=2, nu_post=2,
              restriction=capi.RESTRICT_FULLW, coarse_mode=capi.COARSE_TOL, coarse_tol=0.1, coarse_maxit=2000,
              outer_pre_gs=pre_gs, **SMOOTHERS[sm])
    rng = np.random.default_rng(61)
    u0 = rng.standard_normal((33,) * 3).astype(NP[dtype])
    b = (10.0 * rng.standard_normal((33,) * 3)).astype(NP[dtype])
    steps = [("solve", run_solve), ("pcg_solve", run_pcg)]
    if dtype == capi.MG_F32:
        steps.append(("mixed_solve", run_mixed))
    steps += [("fmg", run_fmg), ("heat_step + set_shift(0)", run_heat), ("solve again", run_solve)]
    with capi.Solver(capi.make_desc(**kw)) as shared:
        got = []
        for name, run in steps:
            got.append(raw(run(shared, u0, b)))
            with capi.Solver(capi.make_desc(**kw)) as fresh:
                want = raw(run(fresh, u0, b))
            assert got[-1] == want, f"{name}: differs from the same call on a fresh handle"
        assert shared.get_shift() == 0.0
        assert got[-1] == got[0], "the second solve differs from the first"
    hist = np.frombuffer(got[0][0], np.float64)
    assert len(hist) == 4 and np.all(np.isfinite(hist)) and hist[-1] < hist[0]   # the drivers did run
