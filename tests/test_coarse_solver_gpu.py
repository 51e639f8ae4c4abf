"""Every coarse-grid solver kernel and its stopping logic against the oracle's Solver::Solve (oracle/gmg_ops.inc:
orc_coarse_solve), through mg_coarse_solve_ex: one case per row of tests/coarse_table.py -- every (kernel, DIM, SEG, overlap,
skip, dtype) mg::coarse_plan can return, at the smallest shape that reaches it -- plus the size edges of the kernels.

Compared per solve: the sweep count and the flag exactly, the iterate bit for bit, the relative residual to the bars of
test_gpu_parity.py::test_coarse_solver (rel 1e-10 fp64, 1e-5 fp32). The right-hand side is random with random Dirichlet
values (default_rng(nx + 31 * ny)); the solve starts from a zero array, from a random array whose boundary values differ
from the right-hand side's, and from a random array with the right-hand side's boundary values. Per row and guess:

 * the stopping sweep CHOSEN: with rel[k] the oracle's relative residual after k sweeps, tol = sqrt(rel[k-1] rel[k]) stops the
   reference loop at exactly k (tol = 2 rel[0] for k = 0). k = 0, 1, 2, 3 and 9 ... 26: with the Jacobi row kernel's window of
   8 sweeps these are all eight positions inside a window, the first and last sweep of two consecutive windows, and the sweeps
   before windows begin. A tie would make this fragile, so a target is kept only if rel[k] <= (1 - 1e-4) rel[k-1]: tol is then
   5e-5 relative away from both neighbours, 100 times the summation-order bar on these norms. Where the norm
   does not fall sweep by sweep, rel[k-1] is replaced by the smallest norm before sweep k (otherwise the loop would have
   stopped earlier). test_stopping_targets_are_well_separated checks on the CPU, with the oracle alone, which targets every
   row keeps: all of them from the random and the settled guess; from the zero guess all but the first sweeps (1 to 3 on the
   skip = 8 rows), because moving the Dirichlet values into x raises the norm above rel[0] = 1 and no tolerance can stop the
   loop until it is back below -- which is why a third guess, random with the right-hand side's boundary values, is run too.
   A degenerate shape (3^2, 3^3: one interior point, solved in one sweep) or an omega that does not converge keeps fewer.
 * the maxit cut: tol = 1e-300 with maxit in MAXITS, and maxit = k*, k* - 1 for two of the chosen stops (flag 0 and flag 1 one
   sweep apart);
 * fixed-sweep mode, maxit in FIXED;
 * a zero right-hand side: from the zero array a NaN norm, no sweep, flag 0, the array untouched; from a random array an
   infinite norm, maxit sweeps and flag 1, as the reference loop does it.
Jacobi rows run with omega = 1 and 6/7; the skip = 1 rows with omega = 1.2, which the descriptor admits (validate_desc does
not bound omega) and which does not converge, so few targets survive there; the one shape whose three LDS arrays do not fit
(skip = 1 for lack of room) runs with 1 and 6/7. The flagged zero guess is reachable only from a cycle: two V(1,1) cycles of a
two-level handle whose coarse U array is filled with NaN first. One child process per switch repeats the affected rows with
the switch at 0."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from multigrid_prj_amd import capi
from oracle import pyoracle as po
from tests import coarse_table as ct
from tests.switch_table import fallbacks

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

STOPS = (0, 1, 2, 3) + tuple(range(9, 27))
MAXITS = (0, 1, 2, 3, 8, 9, 10, 11, 17, 18, 25)
FIXED = (0, 1, 2, 3, 9)
K = max(STOPS)
# the size edges run a part of it (their grids are up to 139^2: the oracle's sweeps are what costs there)
EDGE_STOPS, EDGE_MAXITS, EDGE_FIXED = (0, 1, 2, 3, 9, 10), (0, 1, 3, 9), (0, 2, 9)
DT = {"f64": capi.MG_F64, "f32": capi.MG_F32}


def _rows():
    """(id, dim, dtype, shape, smoother, omega, part, switches off)"""
    out = []
    for v, (shape, sm, off) in ct.REACHABLE.items():
        kernel, dim, seg, overlap, skip, dtype = v
        name = f"{kernel}-{dim}d-seg{seg}{'-overlap' if overlap else ''}-skip{skip}-{dtype}"
        omegas = (1.2,) if skip == 1 else (1.0, 6 / 7) if kernel == "jacobi_rows" else (1.0,)
        out += [(f"{name}-om{om:.3g}", dim, dtype, shape, sm, om, "full", off) for om in omegas]
    for v, (shape, sm, off) in ct.SKIP1_FOR_LDS_ROOM.items():
        out += [(f"{v[0]}-{v[1]}d-seg{v[2]}-skip1-no-lds-room-{v[5]}-om{om:.3g}", v[1], v[5], shape, sm, om, "full", off) for om in (1.0, 6 / 7)]
    for kernel, dim, dtype, shape, sm in ct.EDGES:
        out.append((f"edge-{kernel}-{dim}d-{'x'.join(map(str, shape[3 - dim:]))}-{dtype}", dim, dtype, shape, sm, 1.0, "edge", ()))
    return out


ROWS = _rows()
DEFAULT_ROWS = [r for r in ROWS if not r[7]]
assert len(DEFAULT_ROWS) == len(ROWS)   # every variant is reachable with the switches at their defaults (coarse_table.py)


def desc_kw(dim, dtype, shape, smoother, omega):
    kw, level = ct.handle_kwargs(dim, shape)
    return dict(kw, dtype=DT[dtype], smoother=smoother, omega=omega), level


@functools.lru_cache(maxsize=None)
def problem(dim, dtype, shape):
    """(right-hand side with random Dirichlet values, random guess: its boundary values are other numbers)"""
    nz, ny, nx = shape
    rng = np.random.default_rng(nx + 31 * ny)
    shp, dt = shape[3 - dim:], np.float64 if dtype == "f64" else np.float32
    b, x0 = rng.standard_normal(shp).astype(dt), rng.standard_normal(shp).astype(dt)
    b.setflags(write=False); x0.setflags(write=False)
    return b, x0


GUESSES = ("zero", "random", "settled")


def start(b, x0, guess):
    """zero: a zero array; random: a random one whose boundary values differ from the right-hand side's; settled: the same with
    the right-hand side's boundary values, from which the norm falls from the first sweep on (from the other two the first
    sweep, which moves the Dirichlet values into x, raises it: no tolerance stops those at sweep 1)"""
    if guess == "zero":
        return np.zeros_like(b)
    x = x0.copy()
    if guess == "settled":
        for ax in range(b.ndim):
            for side in (0, -1):
                idx = [slice(None)] * b.ndim; idx[ax] = side
                x[tuple(idx)] = b[tuple(idx)]
    return x


@functools.lru_cache(maxsize=None)
def solve_cases(dim, dtype, shape, smoother, omega, part, guess):
    """[(label, maxit, tol, fixed, expected sweeps or None)] for one row and guess, from the oracle's residual history"""
    kw, lc = desc_kw(dim, dtype, shape, smoother, omega)
    ops = po.Ops(po.make_desc(**kw))
    b, x0 = problem(dim, dtype, shape)
    x = start(b, x0, guess)
    rel = [ops.coarse_solve(lc, smoother, x, b, maxit=0, fixed=True)[3]]
    for _ in range(K):
        x, _, _, r = ops.coarse_solve(lc, smoother, x, b, maxit=1, fixed=True)
        rel.append(r)
    stops, maxits, fixed = (STOPS, MAXITS, FIXED) if part == "full" else (EDGE_STOPS, EDGE_MAXITS, EDGE_FIXED)
    cases, chosen, lo = [("stop0", 1000, 2 * rel[0], 0, 0)], [0], rel[0]
    for k in range(1, K + 1):   # lo: the smallest norm before sweep k, which is rel[k-1] once the norm falls sweep by sweep
        if k in stops and 0 < rel[k] <= (1 - 1e-4) * lo:
            cases.append((f"stop{k}", 1000, math.sqrt(lo * rel[k]), 0, k)); chosen.append(k)
        lo = min(lo, rel[k])
    cases += [(f"maxit{m}", m, 1e-300, 0, None) for m in maxits]
    for ks in sorted(set(chosen[-1:] + [k for k in chosen if k in (2, 13)])):   # before windows, inside one, and the last one kept
        if ks > 0:
            tol = cases[chosen.index(ks)][2]
            cases += [(f"stop{ks}-maxit{ks}", ks, tol, 0, ks), (f"stop{ks}-maxit{ks - 1}", ks - 1, tol, 0, ks - 1)]
    cases += [(f"fixed{m}", m, 0.1, 1, m) for m in fixed]
    return tuple(cases), tuple(chosen), tuple(rel)


def windows_covered(chosen):
    """all eight positions inside a window of 8, over two consecutive windows and their first and last sweeps"""
    return {k % 8 for k in chosen if k >= 9} == set(range(8)) and sum(k >= 9 for k in chosen) >= 16


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_stopping_targets_are_well_separated(row):
    """CPU, the oracle alone: the precondition of the chosen stops, before anything runs on the GPU"""
    name, dim, dtype, shape, sm, om, part, off = row
    for guess in GUESSES:
        cases, chosen, rel = solve_cases(dim, dtype, shape, sm, om, part, guess)
        nz, ny, nx = shape
        if om <= 1 and nx > 3:
            want = STOPS if part == "full" else EDGE_STOPS
            # zero guess: the first sweep moves the Dirichlet values into x and RAISES the norm (by 2.5 to 23 times here); until it is
            # back under rel[0] = 1 no tolerance stops the loop, so those early sweeps are not targets. Never a window position.
            back = next(k for k in range(1, K + 1) if rel[k] <= (1 - 1e-4) * rel[0]) if guess == "zero" else 1
            assert chosen == tuple(k for k in want if k == 0 or k >= back), (name, guess, chosen, rel)
            assert part != "full" or "skip8" not in name or (back <= 9 and windows_covered(chosen)), (name, guess, chosen)
        assert chosen[0] == 0 and all(t > 0 and math.isfinite(t) for _, _, t, _, _ in cases)
        labels = [c[0] for c in cases]
        assert len(set(labels)) == len(labels)


def compare(s, ops, lc, sm, b, x, cases, dtype, what):
    counts = {}
    for label, maxit, tol, fixed, want in cases:
        s.set_array(capi.ARR_E, lc, x)
        st = s.coarse_solve_ex(lc, capi.ARR_E, capi.ARR_RHS, sm, maxit, tol, fixed)
        e, its, flag, rel = ops.coarse_solve(lc, sm, x, b, maxit=maxit, tol=tol, fixed=bool(fixed))
        if want is not None:
            assert its == want, (what, label, "the oracle stopped elsewhere", its, want)
        if label.startswith("maxit") and rel > 0:
            assert (its, flag) == (maxit, 1), (what, label, its, flag)
        assert (st.coarse_iters, st.coarse_flag) == (its, flag), (what, label, (st.coarse_iters, st.coarse_flag), (its, flag))
        got = s.get_array(capi.ARR_E, lc)
        assert np.array_equal(got, e), (what, label, its, int(np.sum(got != e)), "values differ")
        assert st.coarse_relres == pytest.approx(rel, rel=1e-10 if dtype == "f64" else 1e-5), (what, label)
        kind = label.rstrip("0123456789") if "-" not in label else "stop/maxit pair"
        counts[kind] = counts.get(kind, 0) + 1
    return counts


def run_row(row, only_stops=False):
    name, dim, dtype, shape, sm, om, part, off = row
    kw, lc = desc_kw(dim, dtype, shape, sm, om)
    ops = po.Ops(po.make_desc(**kw))
    b, x0 = problem(dim, dtype, shape)
    nx = shape[2]
    with capi.Solver(capi.make_desc(**kw)) as s:
        assert s.level_shape(lc) == b.shape
        s.set_array(capi.ARR_RHS, lc, b)
        for guess in GUESSES:
            cases, chosen, rel = solve_cases(dim, dtype, shape, sm, om, part, guess)
            if only_stops:
                cases = [c for c in cases if c[0].startswith("stop")]
            counts = compare(s, ops, lc, sm, b, start(b, x0, guess), cases, dtype, (name, guess + " guess"))
            print(name, guess, "guess: stops", chosen, counts)
        if only_stops:
            return
        # zero right-hand side. From the zero array Norm() is 0 / 0 = NaN, `NaN > tol` is false and the loop never starts; from any
        # other array it is x / 0 = inf, which no sweep brings under the tolerance: maxit sweeps, flag 1 (orc_coarse_solve)
        zb = np.zeros_like(b)
        s.set_array(capi.ARR_RHS, lc, zb)
        for x in (zb, x0):
            s.set_array(capi.ARR_E, lc, x)
            st = s.coarse_solve_ex(lc, capi.ARR_E, capi.ARR_RHS, sm, 19, 0.1, 0)
            e, its, flag, rel = ops.coarse_solve(lc, sm, x, zb, maxit=19, tol=0.1)
            if x is zb:
                assert (its, flag) == (0, 0) and math.isnan(rel) and np.array_equal(e, x)
            else:   # (one interior point: x is exactly 0 after two sweeps, and 0 / 0 stops the loop there)
                assert ((its, flag) == (19, 1) and rel == math.inf) or (nx == 3 and (its, flag) == (2, 0) and math.isnan(rel))
            assert (st.coarse_iters, st.coarse_flag) == (its, flag), (name, "zero rhs", st.coarse_iters, st.coarse_flag)
            assert (math.isnan(st.coarse_relres) and math.isnan(rel)) or st.coarse_relres == rel, (name, "zero rhs", st.coarse_relres, rel)
            assert np.array_equal(s.get_array(capi.ARR_E, lc), e), (name, "zero rhs")
        print(name, "zero rhs: 2")


@pytest.mark.gpu
@pytest.mark.parametrize("row", DEFAULT_ROWS, ids=[r[0] for r in DEFAULT_ROWS])
def test_table_row_equals_the_oracle(row):
    run_row(row)


def _zero_flag_rows():
    """one shape per (kernel, DIM, SEG): the smallest fp64 one of the table that a two-level hierarchy can end in (a square, a
    cube, or the box (2 (n - 1) + 1, n, n); that leaves out the 3-D global loop, reached at 65 x 9 x 9, whose x the launcher clears
    like the generic LDS kernel's)"""
    best = {}
    for v, (shape, sm, off) in ct.REACHABLE.items():
        if shape[0] not in (1, shape[2], 2 * (shape[2] - 1) + 1):
            continue
        if v[5] == "f64" and v[4] != 1 and not off and (v[:3] not in best or math.prod(shape) < math.prod(best[v[:3]][0])):
            best[v[:3]] = (shape, sm)
    return [(f"{k[0]}-{k[1]}d-seg{k[2]}", k[1], shape, sm) for k, (shape, sm) in best.items()]


@pytest.mark.gpu
@pytest.mark.parametrize("row", _zero_flag_rows(), ids=[r[0] for r in _zero_flag_rows()])
def test_flagged_zero_guess_from_a_cycle(row):
    """zero_x = 1: the V-cycle hands the coarsest solve an array it has NOT cleared. Two-level V(1,1) with this coarse shape;
    the coarse U array is filled with NaN before each cycle, so a kernel that reads x despite the flag cannot pass."""
    name, dim, shape, sm = row
    nz, ny, nx = shape
    semi = 1 if dim == 3 and nz != nx else 0
    n = 2 * (nx - 1) + 1
    assert not semi or nz == n
    kw = dict(dim=dim, n=n, levels=2, dtype=capi.MG_F64, smoother=sm, omega=1.0 if sm != capi.SMOOTH_JACOBI else 6 / 7, cycle=capi.CYCLE_V,
              nu_pre=1, nu_post=1, restriction=capi.RESTRICT_FULLW, coarse_mode=capi.COARSE_TOL, coarse_tol=0.1, semi_xy=semi)
    rng = np.random.default_rng(nx + 31 * ny)
    so = po.Solver(po.make_desc(**kw))
    with capi.Solver(capi.make_desc(**kw)) as sg:
        assert sg.level_shape(1) == shape[3 - dim:]
        u, b = rng.standard_normal(sg.level_shape(0)), rng.standard_normal(sg.level_shape(0))
        sg.set_solution(u); sg.set_rhs(b); so.set_solution(u); so.set_rhs(b)
        for cyc in range(2):
            sg.set_array(capi.ARR_U, 1, np.full(sg.level_shape(1), np.nan))
            st_g, st_o = sg.cycle(), so.cycle()
            print(name, "cycle", cyc, "coarse sweeps", st_g.coarse_iters, st_o.coarse_iters)
            assert (st_g.coarse_iters, st_g.coarse_flag) == (st_o.coarse_iters, st_o.coarse_flag), (name, cyc)
            assert np.array_equal(sg.get_solution(), so.get_solution()), (name, cyc)
    so.close()


# the rows whose kernel a switch at 0 replaces (by the generic LDS kernel or the global loop: coarse_table.py says which side is which)
FAMILY = {"MG_COARSE_ROWS": "jacobi_rows", "MG_COARSE_RB_ROWS": "rb_rows", "MG_COARSE_GS_ROWS": "gs_rows2d"}


def fallback_rows(var):
    rows = [r for r in DEFAULT_ROWS if r[0].startswith(FAMILY[var]) or r[0].startswith("edge-" + FAMILY[var])]
    rows += [(f"off-{kernel}-{'x'.join(map(str, shape[1:]))}-{dtype}", 2, dtype, shape, sm, 1.0, "edge", (sw,))
             for kernel, dtype, shape, sm, sw in ct.EDGES_SWITCH_OFF if sw == var]
    return rows


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tests import test_coarse_solver_gpu as t
rows = t.fallback_rows(sys.argv[2])
assert len(rows) > 2
for row in rows:
    t.run_row(row, only_stops=True)
print("child ok", len(rows))
"""


@pytest.mark.gpu
@pytest.mark.parametrize("var", fallbacks(*FAMILY))
def test_fallback_switch_keeps_counts_and_bits(var):
    """The switch is read once per process: a child repeats the tolerance-mode solves of the family's rows with it at 0, and
    the 2-D size edge of the generic LDS kernel, which only a switch at 0 leads to."""
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, var], env=dict(os.environ, **{var: "0"}), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
