"""numpy references for mg_eig_solve with an operator family, MG_EIG_OPERATOR (include/mg_hip.h): the eigenproblem
L x = lambda x of the two operator families on the unknowns of a face mask,

    ON_FACES        the constant stencil with Neumann faces (tests/bc_ref.py holds its node classes, weights and cycle),
    ON_COEFFICIENT  sigma u - div(a grad u) with Neumann faces (tests/vcn_ref.py),

in the inner product of the weights w = 1/2 per Neumann face a node lies on, in which L is self-adjoint.

 * apply: L b element by element in T, b taken as 0 on the Dirichlet nodes of the mask and the result 0 there -- what the
   role-1 half of k_eig_gram makes (mg_eig.hip), restated on bc_ref's / vcn_ref's expressions;
 * weighted long-double dots;
 * lobpcg: tests/eig_ref.py's reference LOBPCG with w in G, H and the norms and the family's numpy cycle as M;
 * the closed form of the constant operator's spectrum and modes for every mask, and the dense operator on the unknowns.

Helper module (no tests of its own): tests/test_eigop_cpu.py and tests/test_eigop_gpu.py import it.
"""
import numpy as np

from tests import bc_ref as br
from tests import eig_ref as er
from tests import npref
from tests import vc_ref as vr
from tests import vcn_ref as vn
from tests.bc_ref import XLO, XHI, YLO, YHI, ZLO, ZHI, all_faces, face_bit   # noqa: F401

ON_CONSTANT, ON_FACES, ON_COEFFICIENT = 0, 1, 2   # enum mg_eig_operator


def masks(dim):
    """name -> (mask, sigma): the five settings of the issue (2-D: without the z faces)"""
    full = all_faces(dim)
    mixed = vn.MIXED & full
    return {"dirichlet": (0, 0.0), "xlo": (XLO, 0.0), "mixed": (mixed, 0.0), "all-but-yhi": (full & ~YHI, 0.0),
            "all-sigma10": (full, 10.0)}


# ---------------------------------------------------------------- the problems
V22 = dict(cycle=1, smoother=npref.SMOOTH_JACOBI, nu_pre=2, nu_post=2, restriction=npref.RESTRICT_FULLW, outer_pre_gs=0,
           coarse_mode=1, coarse_maxit=20, length=1.0, alpha=1.0)   # make_desc keywords: V(2,2), full weighting, 20 fixed coarse sweeps
COARSE_SWEEPS = 20


def desc_kw(n, levels, dim=3):
    return dict(dim=dim, n=n, levels=levels, aniso=(1.0, 0.7, 0.3) if dim == 3 else (1.0, 0.6, 1.0), omega=6 / 7 if dim == 3 else 0.8, **V22)


def field_smooth100(n):
    """a smooth field spanning a factor of 100 (vc_ref.field_smooth: 10^-1 .. 10^1)"""
    return vr.field_smooth(n)


FIELDS = {"smooth": field_smooth100, "offgrid": vr.field_jump_offgrid, "one": lambda n: np.ones((n, n, n))}

# the whole-solve cases of both test files: name -> (family, n, levels, mask name, field or None); m = 4, nev = 3
SOLVE_M, SOLVE_NEV = 4, 3
SOLVE_CASES = {}
for _n, _lv in ((9, 2), (17, 3)):
    for _mk in ("xlo", "mixed", "all-but-yhi"):
        SOLVE_CASES[f"faces-{_n}-{_mk}"] = (ON_FACES, _n, _lv, _mk, None)
SOLVE_CASES["faces-9-all-sigma10"] = (ON_FACES, 9, 2, "all-sigma10", None)
for _n in (9, 13):
    for _fd in ("smooth", "offgrid"):
        for _mk in ("dirichlet", "xlo", "all-but-yhi"):
            SOLVE_CASES[f"coef-{_n}-{_fd}-{_mk}"] = (ON_COEFFICIENT, _n, 2, _mk, _fd)


def problem(family, kw, mask, sigma, a0=None, prec=np.float64, handle_coefs=None):
    """the numpy problem of a family on the descriptor keywords kw; handle_coefs: [mg_level_coefficients(l)] -- for ON_FACES
    taken AFTER mg_set_shift (cd carries sigma), as the kernels take them"""
    kw = {k: v for k, v in kw.items() if k != "dtype"}
    if family == ON_COEFFICIENT:
        P = vn.VCNProblem(mask=mask, sigma=sigma, prec=prec, **kw)
        if handle_coefs is not None:
            P.use_handle_coefs(handle_coefs)
        P.set_a(a0)
    else:
        P = br.BCProblem(mask=mask, sigma=sigma, prec=prec, **kw)
        if handle_coefs is not None:
            P.use_handle_coefs(handle_coefs)
    return P


def case_problem(name, prec=np.float64):
    family, n, levels, mk, fd = SOLVE_CASES[name]
    mask, sigma = masks(3)[mk]
    return problem(family, desc_kw(n, levels), mask, sigma, FIELDS[fd](n) if fd else None, prec)


def level0_coef(P):
    """(cx, cy, cz, cd) of level 0 as the closed form takes them (cd with the shift)"""
    c = [float(x) for x in P.c_axes[0]]
    cd = float(P.cd[0]) if hasattr(P, "cd") else None
    return (c[-1], c[-2], c[0] if len(c) == 3 else 0.0, cd)


# ---------------------------------------------------------------- the apply, element by element in T
def apply(P, u):
    """L u on level 0 in P.prec, every operation rounded as the kernel rounds it: u counts as 0 on the Dirichlet nodes of
    the mask and the result is 0 there; a mirrored neighbour stands in the slot of the missing one"""
    u = P.as_prec(u)
    dm = P.dirichlet(u.shape)
    u0 = np.where(dm, P.prec(0), u)
    if isinstance(P, vn.VCNProblem):
        s, d = P.parts(u0, 0)
        out = d * u0 - s
    else:
        out = P._row_sum(u0, 0, True)
    return np.where(dm, P.prec(0), out)


def node_weights(P, shape):
    return P.node_weights(shape) if isinstance(P, vn.VCNProblem) else P.weights(shape)


def ld_wdot(w, a, b):
    """sum w a b in long double"""
    return float(np.sum(w.astype(np.longdouble) * a.astype(np.longdouble) * b.astype(np.longdouble)))


# ---------------------------------------------------------------- closed form of the constant operator
def _axis_angles(n, lo_neumann, hi_neumann):
    """the angles phi_k = 2 theta_k of one axis, so that the axis contributes 2 c cos(phi_k) beside cd, and the kind of its modes"""
    if lo_neumann and hi_neumann:
        return np.arange(0, n) * np.pi / (n - 1), "cos"
    if not lo_neumann and not hi_neumann:
        return np.arange(1, n - 1) * np.pi / (n - 1), "sin"
    return (np.arange(0, n - 1) + 0.5) * np.pi / (n - 1), "cos" if lo_neumann else "sin"


def closed_form(coef, shape, mask, count):
    """the `count` smallest eigenvalues of the constant operator with the Neumann faces of `mask`, ascending, with their
    mode indices (one index per ARRAY axis into that axis' table of angles):
        lambda = cd + sum over the axes of 2 c_a cos(2 theta_k),   i.e. sigma + sum (-c_a) 4 sin^2(theta_k),
    theta_k = k pi h / 2 with k = 1 .. n-2 (Dirichlet-Dirichlet), k = 0 .. n-1 (Neumann-Neumann), and (k + 1/2) pi h / 2 with
    k = 0 .. n-2 (mixed), h = 1 / (n - 1) -> (values, [index tuples])"""
    cx, cy, cz, cd = coef
    nd = len(shape)
    axes_c = (cz, cy, cx) if nd == 3 else (cy, cx)
    per_axis = []
    for ax, (c, n) in enumerate(zip(axes_c, shape)):
        phi, _ = _axis_angles(n, bool(mask & face_bit(nd, ax, 0)), bool(mask & face_bit(nd, ax, 1)))
        per_axis.append(2.0 * c * np.cos(phi))
    lam = cd + sum(np.reshape(v, [-1 if a == i else 1 for a in range(nd)]) for i, v in enumerate(per_axis))
    order = np.argsort(lam, axis=None, kind="stable")[:count]
    idx = [tuple(int(k) for k in np.unravel_index(o, lam.shape)) for o in order]
    return lam.ravel()[order], idx


def mode(shape, mask, idx):
    """the eigenvector of mode `idx`: a product of sines, cosines and quarter-wave cosines / sines, 0 on Dirichlet nodes,
    of norm 1 in the w inner product"""
    nd = len(shape)
    v = np.ones(shape)
    w = np.ones(shape)
    for ax, (n, k) in enumerate(zip(shape, idx)):
        lo, hi = bool(mask & face_bit(nd, ax, 0)), bool(mask & face_bit(nd, ax, 1))
        phi, kind = _axis_angles(n, lo, hi)
        s = (np.cos if kind == "cos" else np.sin)(np.arange(n) * phi[k])
        wa = np.ones(n)
        if lo:
            wa[0] = 0.5
        else:
            s[0] = 0.0
        if hi:
            wa[-1] = 0.5
        else:
            s[-1] = 0.0
        rs = [-1 if b == ax else 1 for b in range(nd)]
        v = v * np.reshape(s, rs)
        w = w * np.reshape(wa, rs)
    return v / np.sqrt(np.sum(w * v * v))


# ---------------------------------------------------------------- the dense operator on the unknowns
def dense_operator(P, shape):
    """-> (Lm, unk, w): Lm[i, j] = (L e_j)_i over the unknowns (row-major order of the level), the boolean array of the
    unknowns and their weights; P's level-0 expressions on an array of `shape` (small shapes only)"""
    unk = ~P.dirichlet(shape)
    idx = np.flatnonzero(unk.ravel())
    Lm = np.empty((idx.size, idx.size))
    e = np.zeros(shape, P.prec)
    for j, q in enumerate(idx):
        e.flat[q] = 1
        Lm[:, j] = apply(P, e).ravel()[idx]
        e.flat[q] = 0
    return Lm, unk, node_weights(P, shape).ravel()[idx]


def symmetrised(Lm, w):
    """w^1/2 L w^-1/2: symmetric when diag(w) L is, with L's eigenvalues; its eigenvectors y give x = w^-1/2 y, w-orthonormal"""
    r = np.sqrt(w)
    return Lm * np.outer(r, 1.0 / r)


def dense_eigh(P, shape, count):
    """the `count` lowest eigenpairs from numpy.linalg.eigh of the symmetrised dense operator -> (values, [w-orthonormal
    vectors as level arrays])"""
    Lm, unk, w = dense_operator(P, shape)
    S = symmetrised(Lm, w)
    lam, Y = np.linalg.eigh(0.5 * (S + S.T))
    vecs = []
    for j in range(count):
        x = np.zeros(shape)
        x[unk] = Y[:, j] / np.sqrt(w)
        vecs.append(x)
    return lam[:count], vecs


# ---------------------------------------------------------------- reference weighted LOBPCG
def cycle_preconditioner(P):
    """M r = one cycle of the family's numpy reference from zero, COARSE_SWEEPS fixed sweeps on the coarsest level"""
    return lambda r: P.vcycle(np.zeros_like(r), P.as_prec(r), COARSE_SWEEPS)


def lobpcg(P, X0, nev, tol, maxit, M=None):
    """tests/eig_ref.py::lobpcg on P's operator in the w inner product: G = S^T diag(w) S, H = S^T diag(w) L S and
    relres_j = ||R_j||_w / (|theta_j| ||X_j||_w); M defaults to P's cycle. fp64.
    -> dict(lam, relres, X, iters, cycles, restarts, status, hist)"""
    shape = X0[0].shape
    dm = P.dirichlet(shape)
    w = node_weights(P, shape).ravel()[:, None]
    m = len(X0)
    M = cycle_preconditioner(P) if M is None else M
    A = lambda v: apply(P, v).astype(np.float64)
    flat = lambda cols: np.stack([c.ravel() for c in cols], axis=1)
    unflat = lambda Mx: [Mx[:, j].reshape(shape) for j in range(Mx.shape[1])]
    wnorm = lambda Mx: np.sqrt(np.sum(w * Mx * Mx, axis=0))

    X = flat([np.where(dm, 0.0, x) for x in X0])
    AX = flat([A(x) for x in unflat(X)])
    rr = er.rayleigh_ritz(X.T @ (w * X), X.T @ (w * AX), m)
    if rr is None:
        return dict(status=2, iters=0, cycles=0, restarts=0, hist=[])
    theta, C = rr
    X, AX = X @ C, AX @ C
    P_ = AP = None
    p_cols = []
    iters = cycles = restarts = 0
    hist, status = [], 1
    while True:
        R = AX - X * theta
        relres = wnorm(R) / (np.abs(theta) * wnorm(X))
        hist.append(float(relres[:nev].max()))
        if hist[-1] <= tol:
            status = 0
            break
        if iters == maxit:
            break
        act = [j for j in range(m) if relres[j] > tol]
        if P_ is not None and all(j in p_cols for j in act):
            keep = [p_cols.index(j) for j in act]
            P_, AP = P_[:, keep], AP[:, keep]
        else:
            P_ = AP = None   # first iteration, after a restart, or a column came back from the locked set
        W = flat([np.where(dm, 0.0, np.asarray(M(r), np.float64)) for r in unflat(R[:, act])])
        cycles += len(act)
        AW = flat([A(x) for x in unflat(W)])
        for attempt in range(2):
            S = np.hstack([X, W] + ([P_] if P_ is not None else []))
            AS = np.hstack([AX, AW] + ([AP] if P_ is not None else []))
            G, H = S.T @ (w * S), S.T @ (w * AS)
            G[:m, :m], H[:m, :m] = np.eye(m), np.diag(theta)   # what X's orthonormality already gives
            rr = er.rayleigh_ritz(G, 0.5 * (H + H.T), m)
            if rr is not None or P_ is None:
                break
            P_ = AP = None
            restarts += 1
        if rr is None:
            status = 2
            break
        theta, C = rr
        Cp = C[m:, :][:, act]
        P_, AP = S[:, m:] @ Cp, AS[:, m:] @ Cp
        X, AX = S @ C, AS @ C
        p_cols = list(act)
        iters += 1
    AX = flat([A(x) for x in unflat(X)])
    lam, C = er.rayleigh_ritz(X.T @ (w * X), X.T @ (w * AX), m)
    X, AX = X @ C, AX @ C
    relres = wnorm(AX - X * lam) / np.abs(lam)
    return dict(lam=lam, relres=relres, X=unflat(X), iters=iters, cycles=cycles, restarts=restarts, status=status, hist=hist)


def subspace_sine(x, basis, w):
    """sine of the angle, in the w inner product, between x and the span of the w-orthonormal `basis` vectors"""
    r = np.sqrt(w).ravel()
    return er.subspace_sine(r * x.ravel(), [r * b.ravel() for b in basis])
