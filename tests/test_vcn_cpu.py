"""Neumann faces of the variable-coefficient operator (mg_vc_set_faces), the part that needs no GPU: tests/vcn_ref.py against
tests/vc_ref.py (mask 0, bit for bit) and tests/bc_ref.py (a == 1), the properties the design rests on (diag(w) L symmetric for
any a, constants in the null space, the mirrored full weighting keeps the coefficient's bounds and the weights), the
convergence table of DESIGN.md section 22 and the dispatch rule of the marching tile."""
import os
import subprocess

import numpy as np
import pytest

from tests import npref
from tests import bc_ref as br
from tests import vc_ref as vr
from tests import vcn_ref as vn

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multigrid_prj_amd", "csrc")
LD = np.longdouble


def random_a(shape, seed):
    return np.exp(np.random.default_rng(seed).standard_normal(shape))


# ---------------------------------------------------------------- mask 0 is vc_ref
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kw", [dict(dim=3, n=9, levels=2), dict(dim=3, n=9, levels=2, aniso=(1.0, 30.0, 0.05)), dict(dim=2, n=9, levels=2)],
                         ids=["3d", "aniso", "2d"])
def test_mask_zero_is_vc_ref_bit_for_bit(kw, dtype):
    """residual, Jacobi (omega 1 and 6/7) and red-black on levels 0 and 1, sigma 0 and 500, on the same coefficient arrays"""
    rng = np.random.default_rng(9)
    for sigma in (0.0, 500.0):
        common = dict(length=1.0, alpha=1.3, omega=6.0 / 7.0, sigma=sigma, prec=dtype, **kw)
        V, N = vr.VCProblem(**common), vn.VCNProblem(mask=0, **common)
        V.set_a(random_a(V.shape(0), 1).astype(dtype))
        N.a = V.a
        for l in range(2):
            u, b = (rng.standard_normal(V.shape(l)).astype(dtype) for _ in range(2))
            assert np.array_equal(N.dirichlet(u.shape), npref.boundary_mask(u.shape))
            for got, want in ((N.residual(u, b, l), V.residual(u, b, l)), (N.jacobi(u, b, l), V.jacobi(u, b, l)),
                              (N.jacobi(u, b, l, 1.0), V.jacobi(u, b, l, 1.0)), (N.rbgs(u, b, l), V.rbgs(u, b, l))):
                assert got.dtype == dtype and np.array_equal(got, want), (l, sigma)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_working_dtype_stays_in_its_dtype(dtype):
    N = vn.VCNProblem(mask=vn.MIXED, dim=3, n=9, levels=2, prec=dtype, sigma=3.0, omega=6.0 / 7.0)
    N.set_a(random_a(N.shape(0), 2).astype(dtype))
    rng = np.random.default_rng(5)
    u, b = rng.standard_normal(N.shape(0)).astype(dtype), rng.standard_normal(N.shape(0)).astype(dtype)
    for out in (N.a[1], N.residual(u, b, 0), N.jacobi(u, b, 0), N.jacobi(u, b, 0, 1.0), N.rbgs(u, b, 0), N.restrict_fw(u, 0), N.project(u)[0],
                N.step_rhs(u, b, 1e-3, 0.5), N.step_rhs(u, None, 1e-3, 1.0)):
        assert out.dtype == dtype


# ---------------------------------------------------------------- a == 1 is bc_ref
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mask", [0, 63, vn.MIXED, vn.XLO, 63 & ~vn.YHI])
def test_unit_coefficient_agrees_with_bc_ref(mask, dtype):
    """the two add the same terms in different orders: 8 eps_T of the magnitude of the terms (tests/test_vc_gpu.py's bound for
    a == 1, with bc_ref's apply_A(absolute=True) and point_solve_mag); the same Dirichlet nodes"""
    eps = float(np.finfo(dtype).eps)
    rng = np.random.default_rng(mask)
    for sigma in (0.0, 500.0):
        common = dict(dim=3, n=9, levels=2, length=1.0, alpha=1.3, omega=6.0 / 7.0, sigma=sigma, mask=mask, aniso=(1.0, 3.0, 0.4))
        N, B = vn.VCNProblem(prec=dtype, **common), br.BCProblem(prec=LD, **common)
        N.set_a(np.ones(N.shape(0), dtype))
        for l in range(2):
            assert np.array_equal(N.a[l], np.ones(N.shape(l), dtype))
            u, b = (rng.standard_normal(N.shape(l)).astype(dtype) for _ in range(2))
            dm = N.dirichlet(u.shape)
            assert np.array_equal(dm, B.dirichlet(u.shape))
            bound = 8 * eps * np.asarray(abs(B.as_prec(b)) + B.apply_A(u, l, absolute=True))
            diff = abs(N.residual(u, b, l).astype(LD) - B.residual(u, b, l))
            assert (diff <= bound).all(), (l, sigma, float((diff / bound).max()))
            bound = 8 * eps * np.asarray(abs(B.as_prec(u)) + B.point_solve_mag(u, b, l))
            for om in (1.0, 6.0 / 7.0):
                diff = abs(N.jacobi(u, b, l, om).astype(LD) - B.jacobi(u, b, l, om))
                assert (diff <= bound).all(), (l, sigma, om, float((diff / bound).max()))
            assert (abs(N.rbgs(u, b, l).astype(LD) - B.rbgs(u, b, l)) <= 2 * bound).all()   # two colour passes


# ---------------------------------------------------------------- symmetry, null space, the coarse coefficients
MASKS = {3: [0, 63, vn.MIXED, vn.XLO, vn.ZHI, 63 & ~vn.YHI], 2: [0, 15, vn.XHI | vn.YHI, vn.XLO, vn.YHI, 15 & ~vn.YHI]}


@pytest.mark.parametrize("sigma", [0.0, 500.0])
@pytest.mark.parametrize("dim,k", [(d, k) for d in (3, 2) for k in range(6)])
def test_weighted_operator_is_symmetric(dim, k, sigma):
    """diag(w) L is symmetric on the unknowns for a random positive a, and L 1 = sigma 1 on unknown rows"""
    mask = MASKS[dim][k]
    N = vn.VCNProblem(mask=mask, sigma=sigma, dim=dim, n=7, levels=1, prec=np.float64, aniso=(1.0, 3.0, 0.4))
    shape = N.shape(0)
    N.set_a(random_a(shape, 7 + k))
    A = N.matrix(0)
    unk = ~N.dirichlet(shape).ravel()
    w = N.node_weights(shape).ravel()
    WA = (w[:, None] * A)[np.ix_(unk, unk)]
    tol = 8 * np.finfo(np.float64).eps * abs(A).max()
    assert abs(WA - WA.T).max() <= tol
    assert abs(A[np.ix_(unk, unk)] - A[np.ix_(unk, unk)].T).max() > 1e3 * tol or mask == 0   # without w it is not
    row = N.apply_A(np.ones(shape), 0).ravel()[unk]
    assert abs(row - sigma).max() <= tol


@pytest.mark.parametrize("dim", [3, 2])
def test_constants_span_the_null_space(dim):
    """every face Neumann, sigma = 0: L applied to a constant vanishes at every node, to rounding"""
    N = vn.VCNProblem(mask=vn.all_faces(dim), dim=dim, n=9, levels=1, prec=np.float64)
    N.set_a(random_a(N.shape(0), 3))
    assert N.singular() and not N.dirichlet(N.shape(0)).any()
    out = N.apply_A(np.full(N.shape(0), 2.5), 0)
    assert abs(out).max() <= 8 * np.finfo(np.float64).eps * 2.5 * abs(N.parts(np.ones(N.shape(0)), 0)[1]).max()


@pytest.mark.parametrize("kw", [dict(dim=3, n=9, levels=3), dict(dim=3, n=9, levels=3, semi_xy=1), dict(dim=2, n=17, levels=3)],
                         ids=["3d", "semi", "2d"])
def test_mirrored_full_weighting_keeps_bounds_and_weights(kw):
    """min a <= a_coarse <= max a on every level for every mask (a convex combination: non-negative weights that add up to 1,
    so only the rounding of three sums can leave the interval), and R^T w_coarse = w_fine / 2^(coarsened axes) exactly"""
    dim = kw["dim"]
    for mask in MASKS[dim]:
        N = vn.VCNProblem(mask=mask, prec=np.float64, **kw)
        a0 = np.where(np.random.default_rng(mask).random(N.shape(0)) < 0.5, 1.0, 1000.0)
        N.set_a(a0)
        for l in range(1, N.L):
            assert N.a[l].min() >= 1.0 * (1 - 1e-14) and N.a[l].max() <= 1000.0 * (1 + 1e-14), (mask, l)
    N = vn.VCNProblem(mask=vn.all_faces(dim), prec=np.float64, **kw)
    R = N.restriction_matrix(0)
    wf, wc = N.node_weights(N.shape(0)).ravel(), N.node_weights(N.shape(1)).ravel()
    assert np.array_equal(R.T @ wc, wf / 2 ** len(N._coarsened_axes(0)))


# ---------------------------------------------------------------- the table of DESIGN.md section 22
def factor(field, faces, **kw):
    hist, f = vn.cycle_factor(vn.convergence_problem(field, faces, **{k: v for k, v in kw.items() if k != "ncycles"}), ncycles=kw.get("ncycles", 12))
    print(field, faces, kw, "factors per cycle", np.round(hist[1:] / hist[:-1], 4), "last residual", hist[-1])
    return f, hist


# (field, faces) -> (factor of the 12th cycle, flexible CG iterations to 1e-8 with w-weighted dots, with plain dots): the rows of
# the table in DESIGN.md section 22 and the figures of the README row, as tests/vcn_ref.py gives them in float64
TABLE = {
    ("smooth", "x-lo"): (0.156, 6, 6),
    ("smooth", "mixed"): (0.261, 8, 8),
    ("smooth", "only-y-hi-dirichlet"): (0.363, 8, 9),
    ("smooth", "all-neumann-singular"): (0.295, 8, 8),
    ("smooth", "all-neumann-sigma10"): (0.222, None, None),
    ("aligned", "x-lo"): (0.992, 20, 24),
    ("aligned", "mixed"): (0.991, 22, 37),
    ("aligned", "only-y-hi-dirichlet"): (0.991, 28, 47),
    ("aligned", "all-neumann-singular"): (0.679, 16, 16),
    ("offgrid", "x-lo"): (0.991, 24, 28),
    ("offgrid", "mixed"): (0.951, 27, 38),
    ("offgrid", "all-neumann-singular"): (0.785, 21, 22),
}


@pytest.mark.parametrize("field,faces", list(TABLE), ids=["-".join(k) for k in TABLE])
def test_convergence_table(field, faces):
    """3-D, n = 33, 4 levels, red-black V(2,2), mirrored full weighting of residuals and coefficients, 50 coarse sweeps, seeded
    standard-normal right-hand side, float64: deterministic, so every row of the documented table is pinned -- the factor to
    the three digits the table prints, the iteration counts exactly. The smooth field converges with every mask; on the jumps
    the cycle stalls (or crawls) and the w-weighted dots never cost more iterations than plain ones."""
    want_f, want_w, want_p = TABLE[field, faces]
    P = vn.convergence_problem(field, faces)
    hist, f = vn.cycle_factor(P)
    print(field, faces, "factor", f, "after 12 cycles", hist[-1])
    assert f == pytest.approx(want_f, abs=0.003)
    if field == "smooth":
        assert hist[-1] < 1e-5
    if want_w is not None:
        kw, hw = vn.fcg_iterations(P, True)
        kp, hp = vn.fcg_iterations(P, False)
        print("flexible CG iterations: weighted", kw, "to", hw[-1], "(before:", hw[-2], ") plain", kp, "to", hp[-1], "(before:", hp[-2], ")")
        assert hw[-1] <= 1e-8 and hp[-1] <= 1e-8
        assert (kw, kp) == (want_w, want_p) and kw <= kp


def test_todays_restriction_diverges_on_a_neumann_face():
    """full weighting that injects at the coarse nodes of the x-lo Neumann face (coefficients and residuals): after the first
    cycles the residual grows, by 1.03 at cycle 5 up to 1.5 per cycle at cycle 12, where the relative residual has passed
    2.8, 4.0, 5.9 and reached 8.9 (the diverging row of the table in DESIGN.md section 22)"""
    f, hist = factor("smooth", "x-lo", restriction_mode="today")
    growth = hist[1:] / hist[:-1]
    assert f > 1.2 and (growth[4:] > 1.0).all()
    assert hist[-4:] == pytest.approx([2.8, 4.0, 5.9, 8.9], rel=0.02)


# ---------------------------------------------------------------- which form a shape takes
MAIN = r"""
#include <cstdio>
#include "mg_geom.h"
int main()
{
    int dim, nx, ny, nz, es;
    while (scanf("%d %d %d %d %d", &dim, &nx, &ny, &nz, &es) == 5) printf("%d\n", mg::vc_march_ok(dim, nx, ny, nz, es) ? 1 : 0);
    return 0;
}
"""


def test_dispatch_rule(tmp_path):
    """march_side / march_ok of vcn_ref agree with mg_geom.h on the shapes of tests/test_vcn_gpu.py and around the thresholds"""
    src, exe = tmp_path / "vcn_gate.cpp", tmp_path / "vcn_gate"
    src.write_text(MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], check=True)
    cases = []
    for n in (3, 5, 7, 9, 17, 31, 32, 33, 34, 35, 63, 64, 65, 67, 130, 513, 1025):
        for es in (8, 4):
            cases += [(3, n, n, n, es), (2, n, n, 1, es)]
            assert vn.march_ok(3, n, n, n, es) == vn.march_side(3, n, es)
    cases += [(3, 33, 33, 5, 8), (3, 33, 33, 7, 8), (3, 17, 17, 513, 8), (3, 64, 6, 64, 4)]
    want = [int(vn.march_ok(*c)) for c in cases]
    text = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == want
    by = dict(zip(cases, want))
    assert by[3, 9, 9, 9, 8] == 0 and by[3, 17, 17, 17, 4] == 0 and by[3, 33, 33, 33, 8] == 1 and by[3, 35, 35, 35, 8] == 1
    assert by[3, 34, 34, 34, 8] == 1 and by[3, 33, 33, 33, 4] == 0 and by[3, 65, 65, 65, 4] == 1 and by[3, 67, 67, 67, 4] == 1
    assert not any(w for c, w in by.items() if c[0] == 2)


# ---------------------------------------------------------------- an inhomogeneous flux
def flux_case(n, form, wall_flat):
    """2-D, u = sin(x + .3) cos(2y) on the unit square, -div(a grad u) = f; x-lo, x-hi and y-hi carry the exact outward normal
    derivative g, folded into b at the face's nodes (a corner takes one term per face); y-lo is Dirichlet.
    form "wall": + (2 alpha / h) a_i g, the flux through the wall with the coefficient AT the wall;
    form "half": + (alpha / h) (a_i + a_i+) g, the coefficient of the mirrored slot (half a cell inside).
    wall_flat: a has zero normal derivative on the three Neumann faces, where the two forms differ by O(h^2) only."""
    X, Y = br.grid(n, 2)
    u = np.sin(X + 0.3) * np.cos(2 * Y)
    ux, uy = np.cos(X + 0.3) * np.cos(2 * Y), -2 * np.sin(X + 0.3) * np.sin(2 * Y)
    if wall_flat:
        a = 1.5 + 0.5 * np.cos(np.pi * X) * np.cos(np.pi * Y)
        ax, ay = -0.5 * np.pi * np.sin(np.pi * X) * np.cos(np.pi * Y), -0.5 * np.pi * np.cos(np.pi * X) * np.sin(np.pi * Y)
    else:
        a = 1.0 + 0.5 * X + 0.3 * np.sin(2 * Y)
        ax, ay = 0.5 + 0 * X, 0.6 * np.cos(2 * Y)
    b = -(ax * ux + a * (-u) + ay * uy + a * (-4 * u))
    h = 1.0 / (n - 1)
    for here, inside, g in (((slice(None), 0), (slice(None), 1), -ux[:, 0]), ((slice(None), -1), (slice(None), -2), ux[:, -1]),
                            ((-1, slice(None)), (-2, slice(None)), uy[-1, :])):
        b[here] += (2.0 / h) * a[here] * g if form == "wall" else (1.0 / h) * (a[here] + a[inside]) * g
    b[0, :] = u[0, :]   # Dirichlet data
    return a, b, u


def flux_errors(form, wall_flat):
    errs = []
    for n in (17, 33, 65):
        a, b, u = flux_case(n, form, wall_flat)
        P = vn.VCNProblem(mask=br.FLUX_MASK, dim=2, n=n, levels=br.levels_for(n), length=1.0, alpha=1.0, smoother=npref.SMOOTH_RBGS,
                          nu_pre=2, nu_post=2, restriction=npref.RESTRICT_FULLW, outer_pre_gs=0, prec=np.float64)
        P.set_a(a)
        x, hist, _, _ = P.solve_history(np.zeros_like(b), b, 80, 50, tol=1e-12)
        assert hist[-1] <= 1e-12
        errs.append(float(abs(x - u).max()))
    print(form, "wall-flat a" if wall_flat else "general a", "errors", errs, "ratios", errs[0] / errs[1], errs[1] / errs[2])
    return errs


def test_inhomogeneous_flux_is_second_order():
    """the wall form is second-order accurate for any a (measured 3.90e-3 / 9.74e-4 / 2.44e-4: ratios 4.00, 4.00)"""
    e = flux_errors("wall", False)
    assert 3.9 <= e[0] / e[1] <= 4.1 and 3.9 <= e[1] / e[2] <= 4.1


def test_half_node_flux_form_needs_a_flat_coefficient_at_the_wall():
    """(alpha / h)(a_i + a_i+) g takes a half a cell inside the wall: it imposes the flux with a relative error (h/2) a'/a. Second
    order where a has zero normal derivative on the Neumann faces; first order otherwise (measured 1.13e-2 / 4.95e-3 / 2.30e-3:
    ratios 2.29, 2.16) -- INTEGRATION.md gives the wall form for that reason"""
    e = flux_errors("half", True)
    assert 3.8 <= e[0] / e[1] <= 4.2 and 3.8 <= e[1] / e[2] <= 4.2
    e = flux_errors("half", False)
    assert e[1] / e[2] < 3.0 and e[2] > 5 * flux_errors("wall", False)[2]
