"""tests/fmgop_ref.py on its own (no GPU): the mirrored FMG interpolation reproduces the polynomials it should, keeps the
one-sided rule at Dirichlet ends and is npref_fmg's with mask 0; the reference pass has the FMG property on the cases the GPU
test reuses -- this is where their inputs are chosen -- and handles the singular all-Neumann case."""
import functools

import numpy as np
import pytest

from tests import bc_ref as br
from tests import fmgop_ref as fo
from tests import npref
from tests import npref_fmg as nf

EPS = float(np.finfo(np.float64).eps)


def row_problem(nc, dim=2):
    return npref.Problem(dim=dim, n=2 * nc - 1, levels=2, prec=np.float64)


def prolong_row(c, lo, hi):
    return fo.rule_last_axis(np.asarray(c, np.float64)[None, :], lo, hi)[0]


# ---------------------------------------------------------------- the 1-D rule
@pytest.mark.parametrize("nc", [3, 4, 5, 9, 17])
def test_even_polynomials_at_a_neumann_lo_end(nc):
    """x = 0 is the Neumann end: an even polynomial is its own mirror image there, so the cubic rule on the extended row is
    exact for it up to degree 3 -- at every fine node, node 1 included. The hi end is Dirichlet: the one-sided quadratic
    rule is exact for degree 2."""
    xc, xf = np.arange(nc, dtype=np.float64), 0.5 * np.arange(2 * nc - 1)
    for p in (lambda x: 1 + 0 * x, lambda x: 1 + 3 * x * x, lambda x: 2 - 0.75 * x * x):
        got = prolong_row(p(xc), True, False)
        assert abs(got - p(xf)).max() <= 8 * EPS * abs(p(xf)).max()
    # the same at a Neumann hi end, mirrored about x = nc - 1
    q = lambda x: 1 + 3 * (x - (nc - 1)) ** 2
    assert abs(prolong_row(q(xc), False, True) - q(xf)).max() <= 8 * EPS * abs(q(xf)).max()
    # both ends Neumann: cos-like even data about both ends, exact for constants; node 1 and node 2nc-3 take the cubic rule
    c = np.random.default_rng(nc).standard_normal(nc)
    got = prolong_row(c, True, True)
    ext = np.concatenate(([c[1]], c, [c[-2]]))
    want = (9 * ext[1:-2] + 9 * ext[2:-1] - ext[:-3] - ext[3:]) / 16
    assert abs(got[1::2] - want).max() <= 8 * EPS * abs(c).max() and np.array_equal(got[::2], c)


@pytest.mark.parametrize("nc", [3, 4, 9])
def test_dirichlet_ends_keep_the_one_sided_rule(nc):
    c = np.random.default_rng(10 + nc).integers(-50, 50, nc).astype(np.float64)   # integers: every order of operations is exact
    for lo, hi in ((False, False), (True, False), (False, True)):
        got = prolong_row(c, lo, hi)
        if not lo:
            assert got[1] == (3 * c[0] + 6 * c[1] - c[2]) / 8
        if not hi and not (nc == 3 and not lo):
            assert got[-2] == (3 * c[-1] + 6 * c[-2] - c[-3]) / 8
        if lo:
            assert got[1] == (-c[1] + 9 * c[0] + 9 * c[1] - c[2]) / 16
        if hi:
            assert got[-2] == (-c[-2] + 9 * c[-1] + 9 * c[-2] - c[-3]) / 16


@pytest.mark.parametrize("case", [dict(dim=2, n=33, levels=2), dict(dim=3, n=17, levels=2), dict(dim=3, n=17, levels=2, semi_xy=1),
                                  dict(dim=3, n=5, levels=2), dict(dim=3, n=13, levels=2)],
                         ids=lambda c: f"{c['dim']}d{c['n']}s{c.get('semi_xy', 0)}")
def test_mask_zero_is_npref_fmg(case):
    """integer-valued arrays: both references' orders of operations are exact on them, so the two agree bit for bit"""
    P = npref.Problem(prec=np.float64, **case)
    rng = np.random.default_rng(3)
    c = rng.integers(-100, 100, P.shape(1)).astype(np.float64)
    bnd = rng.integers(-100, 100, P.shape(0)).astype(np.float64)
    assert np.array_equal(fo.prolong(P, c, 0, 0), nf.cubic_prolong(P, c, 0))
    assert np.array_equal(fo.prolong(P, c, 0, 0, bnd=bnd), nf.cubic_prolong(P, c, 0, bnd=bnd))
    # and on random data to rounding
    c = rng.standard_normal(P.shape(1))
    assert abs(fo.prolong(P, c, 0, 0) - nf.cubic_prolong(P, c, 0)).max() <= 16 * EPS * abs(c).max()


@pytest.mark.parametrize("mask", [1, 2, 4, 16, 32, 55, 63])
def test_tensor_product_with_a_mask(mask):
    """3-D: Dirichlet nodes take bnd, every other node is interpolated -- a product of per-axis polynomials that are even
    about their Neumann ends and of degree <= 2 otherwise is reproduced at every node"""
    P = npref.Problem(dim=3, n=9, levels=2, prec=np.float64)
    nc, n = 5, 9

    def poly(ax, x, last):
        lo, hi = bool(mask & br.face_bit(3, ax, 0)), bool(mask & br.face_bit(3, ax, 1))
        if lo and hi:
            return 1 + 0 * x
        if lo:
            return 1 + 0.5 * x * x
        if hi:
            return 2 - 0.25 * (x - last) ** 2
        return 1 + 0.3 * x - 0.2 * x * x
    fc = [poly(ax, np.arange(nc, dtype=np.float64), nc - 1.0) for ax in range(3)]
    ff = [poly(ax, 0.5 * np.arange(n), nc - 1.0) for ax in range(3)]
    c = fc[0][:, None, None] * fc[1][None, :, None] * fc[2][None, None, :]
    f = ff[0][:, None, None] * ff[1][None, :, None] * ff[2][None, None, :]
    got = fo.prolong(P, c, 0, mask)
    assert abs(got - f).max() <= 32 * EPS * abs(f).max()
    bnd = np.full(P.shape(0), 7.0)
    got = fo.prolong(P, c, 0, mask, bnd=bnd)
    dm = fo.dirichlet_nodes(P.shape(0), mask)
    assert np.array_equal(dm, br.BCProblem(mask=mask, dim=3, n=9, levels=2).dirichlet(P.shape(0)))
    assert (got[dm] == 7.0).all() and abs(got - f)[~dm].max(initial=0.0) <= 32 * EPS * abs(f).max()


# ---------------------------------------------------------------- the FMG property of the reference pass
@functools.lru_cache(maxsize=None)
def property_figures(name):
    """-> (||u_fmg - u_h||, ||u_h - u*||, relres) in the max norm: one red-black V(2,2) per level, float64"""
    P, b, ustar, _ = fo.case_problem(name)
    uh = fo.discrete_solution(P, b)
    u, relres, _ = fo.fmg_pass(P, b, 1, fo.COARSE_SWEEPS)
    return float(abs(u - uh).max()), float(abs(uh - ustar).max()), relres


@pytest.mark.parametrize("name", fo.PROPERTY_CASES)
def test_reference_pass_has_the_fmg_property(name):
    e_alg, e_disc, relres = property_figures(name)
    print(f"{name}: ||u_fmg - u_h|| {e_alg:.3e}  ||u_h - u*|| {e_disc:.3e}  ratio {e_alg / e_disc:.3f}  relres {relres:.2e}")
    assert e_alg <= e_disc


def test_the_dropped_case_is_the_only_one_and_misses_in_the_reference():
    assert len(fo.DROPPED) <= 1 and set(fo.PROPERTY_CASES) | set(fo.DROPPED) == set(fo.CASES)
    for name, ratio in fo.DROPPED.items():
        e_alg, e_disc, _ = property_figures(name)
        print(f"{name}: ratio {e_alg / e_disc:.3f}")
        assert e_alg > e_disc and e_alg / e_disc == pytest.approx(ratio, rel=5e-3)


def test_cases_cover_the_issue():
    fams = {fo.CASES[n][0] for n in fo.CASES}
    assert fams == {"bc", "vc", "fas", "fasn", "fasvc"}
    assert {fo.CASES[n][4] for n in fo.CASES if fo.CASES[n][0] in ("bc", "vc")} == {fo.X_LO, fo.ALL_BUT_Y_HI}
    assert any(fo.CASES[n][1] == 2 and fo.CASES[n][2] == 65 for n in fo.CASES)
    assert all((fo.CASES[n][2], fo.CASES[n][3]) == (33, 4) for n in fo.CASES if fo.CASES[n][1] == 3)


# ---------------------------------------------------------------- the singular case
def test_singular_all_neumann_pass():
    """mask 63, no shift: b is projected first and u last; relres is measured against the projected b, and the w-weighted
    mean of the result is zero"""
    P = br.convergence_problem("all-neumann-singular", n=17, levels=3)
    b = br.convergence_rhs(P.shape(0), seed=5)
    u, relres, bp = fo.fmg_pass(P, b, 1, 30)
    w = P.weights(b.shape)
    assert abs((w * u).sum()) <= 1e-12 * (w * abs(u)).sum()
    assert abs((w * bp).sum()) <= 1e-12 * (w * abs(bp)).sum() and not np.array_equal(bp, b)
    assert relres == pytest.approx(P.rel_residual(u, bp), rel=1e-12) and relres < 0.2
    # two cycles per level do better than one
    assert fo.fmg_pass(P, b, 2, 30)[1] < relres
