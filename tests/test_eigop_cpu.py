"""The numpy side of the operator families of mg_eig_solve (MG_EIG_OPERATOR), no GPU: tests/eigop_ref.py against dense matrices.

* diag(w) L is symmetric for both families and every mask: the reason the eigenproblem is solved in the w inner product;
* the closed form of the constant operator's spectrum with Neumann faces equals the dense eigenvalues;
* the reference weighted LOBPCG converges on every whole-solve case of tests/test_eigop_gpu.py.

Iteration counts of the reference LOBPCG at tol = 1e-8, m = 4, nev = 3, start vectors eig_ref.start_vectors (REF_ITERS
below; tests/test_eigop_gpu.py allows the GPU two more). With the exact inverse as M the 9 x 9 x 5 coefficient case below needs
EXACT_INVERSE_ITERS iterations; the cycle-preconditioned counts are of that order (20 .. 37), except where the off-grid jump
of 1000 meets the x-lo Neumann face (52, 55): the two-level Jacobi cycle is a weaker preconditioner there.
"""
import numpy as np
import pytest

from tests import eig_ref as er
from tests import eigop_ref as eo

TOL = 1e-8
REF_ITERS = {
    "faces-9-xlo": 35, "faces-9-mixed": 20, "faces-9-all-but-yhi": 25,
    "faces-17-xlo": 37, "faces-17-mixed": 22, "faces-17-all-but-yhi": 21,
    "faces-9-all-sigma10": 24,
    "coef-9-smooth-dirichlet": 21, "coef-9-smooth-xlo": 28, "coef-9-smooth-all-but-yhi": 22,
    "coef-9-offgrid-dirichlet": 25, "coef-9-offgrid-xlo": 52, "coef-9-offgrid-all-but-yhi": 32,
    "coef-13-smooth-dirichlet": 24, "coef-13-smooth-xlo": 31, "coef-13-smooth-all-but-yhi": 22,
    "coef-13-offgrid-dirichlet": 35, "coef-13-offgrid-xlo": 55, "coef-13-offgrid-all-but-yhi": 34,
}
EXACT_INVERSE_ITERS = 19

SHAPES = [(9, 9, 9), (5, 9, 9)]   # (nz, ny, nx): 9^3 and 9 x 9 x 5
MASKS = list(eo.masks(3))


def random_field(shape, seed=3):
    """a random positive field spanning a factor of 100"""
    return 10.0 ** np.random.default_rng(seed).uniform(-1.0, 1.0, shape)


def dense_problem(family, shape, mask_name):
    mask, sigma = eo.masks(3)[mask_name]
    P = eo.problem(family, eo.desc_kw(9, 1), mask, sigma, a0=np.ones((9, 9, 9)))
    if family == eo.ON_COEFFICIENT:
        P.a = [random_field(shape)]
    return P, mask


@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=["9x9x9", "9x9x5"])
@pytest.mark.parametrize("family", [eo.ON_FACES, eo.ON_COEFFICIENT], ids=["faces", "coefficient"])
def test_weighted_operator_is_symmetric(family, shape, mask_name):
    P, mask = dense_problem(family, shape, mask_name)
    Lm, unk, w = eo.dense_operator(P, shape)
    axis = lambda n, ax: n - (0 if mask & eo.face_bit(3, ax, 0) else 1) - (0 if mask & eo.face_bit(3, ax, 1) else 1)
    assert Lm.shape[0] == int(np.prod([axis(n, ax) for ax, n in enumerate(shape)]))
    WL = w[:, None] * Lm
    assert np.max(np.abs(WL - WL.T)) <= 4 * np.finfo(np.float64).eps * np.max(np.abs(WL))
    if mask:
        assert np.max(np.abs(Lm - Lm.T)) > 1e-3 * np.max(np.abs(Lm))   # L itself is not symmetric with a Neumann face


@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=["9x9x9", "9x9x5"])
def test_closed_form_matches_dense_eigenvalues(shape, mask_name):
    P, mask = dense_problem(eo.ON_FACES, shape, mask_name)
    Lm, unk, w = eo.dense_operator(P, shape)
    S = eo.symmetrised(Lm, w)
    dense = np.linalg.eigvalsh(0.5 * (S + S.T))
    exact, idx = eo.closed_form(eo.level0_coef(P), shape, mask, dense.size)
    assert len(idx) == dense.size
    np.testing.assert_allclose(dense, exact, rtol=0, atol=1e-12 * abs(exact).max())
    # the modes are eigenvectors, of w-norm 1
    for k in (0, 1, 5):
        v = eo.mode(shape, mask, idx[k])
        np.testing.assert_allclose(eo.apply(P, v), exact[k] * v, atol=1e-10 * abs(exact).max())
        np.testing.assert_allclose(eo.ld_wdot(eo.node_weights(P, shape), v, v), 1.0, rtol=1e-13)
    if mask_name == "all-sigma10":
        np.testing.assert_allclose(exact[0], 10.0, rtol=1e-13)


def test_exact_inverse_iterations():
    """3 of 4 pairs at 1e-8 on the 9 x 9 x 5 coefficient case with M = L^-1: the count the cycle-preconditioned ones are
    measured against"""
    shape = SHAPES[1]
    P, mask = dense_problem(eo.ON_COEFFICIENT, shape, "xlo")
    Lm, unk, w = eo.dense_operator(P, shape)
    Li = np.linalg.inv(Lm)

    def M(r):
        z = np.zeros(shape)
        z[unk] = Li @ r[unk]
        return z
    out = eo.lobpcg(P, er.start_vectors(shape, 4), 3, TOL, 80, M)
    print("exact-inverse iterations", out["iters"])
    assert out["status"] == 0 and abs(out["iters"] - EXACT_INVERSE_ITERS) <= 2
    lam = np.linalg.eigvalsh(0.5 * (eo.symmetrised(Lm, w) + eo.symmetrised(Lm, w).T))
    np.testing.assert_allclose(out["lam"][:3], lam[:3], rtol=2 * TOL)


@pytest.fixture(scope="module")
def reference_runs():
    out = {}
    for name in eo.SOLVE_CASES:
        P = eo.case_problem(name)
        out[name] = (P, eo.lobpcg(P, er.start_vectors(P.shape(0), eo.SOLVE_M), eo.SOLVE_NEV, TOL, 80))
    return out


@pytest.mark.parametrize("name", list(eo.SOLVE_CASES))
def test_reference_lobpcg_converges(reference_runs, name):
    P, out = reference_runs[name]
    family, n, levels, mk, fd = eo.SOLVE_CASES[name]
    mask = P.mask
    print(name, "iters", out["iters"], "cycles", out["cycles"], "restarts", out["restarts"], "lambda", out["lam"])
    assert out["status"] == 0 and out["hist"][-1] <= TOL
    assert abs(out["iters"] - REF_ITERS[name]) <= 1   # numpy's own eigh / cholesky may round differently from build to build
    if family == eo.ON_FACES:
        exact, _ = eo.closed_form(eo.level0_coef(P), P.shape(0), mask, eo.SOLVE_M)
    else:
        exact, _ = eo.dense_eigh(P, P.shape(0), eo.SOLVE_M)
    nev = eo.SOLVE_NEV
    assert np.all(np.abs(out["lam"][:nev] - exact[:nev]) <= 2 * TOL * np.abs(exact[:nev])), (out["lam"], exact)
    w = eo.node_weights(P, P.shape(0))
    G = np.array([[eo.ld_wdot(w, a, b) for b in out["X"]] for a in out["X"]])
    np.testing.assert_allclose(G, np.eye(eo.SOLVE_M), atol=1e-12)

