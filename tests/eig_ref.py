"""numpy references for mg_eig_solve (include/mg_hip.h): the closed-form spectrum of the level-0 operator, a dense
restatement of it, the element-wise formulas of the two block kernels of mg_eig.hip, and an independent LOBPCG that
follows the same algorithm with the CPU oracle's cycle as preconditioner.

Helper module (no tests of its own): tests/test_eig_cpu.py and tests/test_eig_gpu.py import it.
"""
import numpy as np

from oracle import pyoracle as po

PIVOT_MIN = 1e-10   # mg_dense.h::DENSE_PIVOT_MIN


def interior(ndim):
    return (slice(1, -1),) * ndim


def boundary_mask(shape):
    m = np.ones(shape, bool)
    m[interior(len(shape))] = False
    return m


# ---------------------------------------------------------------- the whole-solve cases of both test files
V22 = dict(cycle=po.CYCLE_V, smoother=po.SMOOTH_JACOBI, nu_pre=2, nu_post=2, restriction=po.RESTRICT_FULLW, outer_pre_gs=0,
           coarse_mode=po.COARSE_FIXED, coarse_maxit=20, length=1.0)
# name -> (descriptor keywords, m, nev)
SOLVE_CASES = {
    "3d9": (dict(dim=3, n=9, levels=2, aniso=(1.0, 0.7, 0.3), omega=6 / 7, **V22), 4, 4),
    "3d33": (dict(dim=3, n=33, levels=4, aniso=(1.0, 0.7, 0.3), omega=6 / 7, **V22), 4, 4),
    "2d65": (dict(dim=2, n=65, levels=4, aniso=(1.0, 0.6, 1.0), omega=0.8, **V22), 5, 3),
    "3d25-degenerate": (dict(dim=3, n=25, levels=3, omega=6 / 7, **V22), 6, 4),   # lambda_2 = lambda_3 = lambda_4
}


def start_vectors(shape, m, seed=2001):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(shape) for _ in range(m)]


# ---------------------------------------------------------------- closed form
def closed_form(coef, shape, count):
    """the `count` smallest eigenvalues of the interior operator, ascending, with their mode indices:
    lambda(p, q, r) = cd + 2 cx cos(p pi / (nx-1)) + 2 cy cos(q pi / (ny-1)) + 2 cz cos(r pi / (nz-1)), indices 1 .. n-2
    (shape is (nz, ny, nx) or (ny, nx); the z term is dropped in 2-D). -> (values, [(r, q, p) or (q, p)])"""
    cx, cy, cz, cd = coef
    axes_c = (cz, cy, cx) if len(shape) == 3 else (cy, cx)
    per_axis = [2.0 * c * np.cos(np.arange(1, n - 1) * np.pi / (n - 1)) for c, n in zip(axes_c, shape)]
    lam = cd + sum(np.reshape(v, [-1 if a == i else 1 for a in range(len(shape))]) for i, v in enumerate(per_axis))
    order = np.argsort(lam, axis=None, kind="stable")[:count]
    idx = [tuple(int(k) + 1 for k in np.unravel_index(o, lam.shape)) for o in order]
    return lam.ravel()[order], idx


def mode(shape, idx):
    """the normalised eigenvector of mode `idx` (a product of sines, 0 on Dirichlet nodes)"""
    v = np.ones(shape)
    for a, (n, k) in enumerate(zip(shape, idx)):
        s = np.sin(np.arange(n) * k * np.pi / (n - 1))
        s[0] = s[-1] = 0.0
        v = v * np.reshape(s, [-1 if b == a else 1 for b in range(len(shape))])
    return v / np.linalg.norm(v)


def dense_matrix(coef, shape):
    """the interior operator as a dense matrix (small shapes only)"""
    cx, cy, cz, cd = coef
    axes_c = (cz, cy, cx) if len(shape) == 3 else (cy, cx)
    m = [n - 2 for n in shape]
    A = cd * np.eye(int(np.prod(m)))
    for a, c in enumerate(axes_c):
        mats = [np.eye(k, k=1) + np.eye(k, k=-1) if i == a else np.eye(k) for i, k in enumerate(m)]
        K = mats[0]
        for M_ in mats[1:]:
            K = np.kron(K, M_)
        A += c * K
    return A


# ---------------------------------------------------------------- element-wise formulas of the kernels
def apply_A(w, coef, T=np.float64):
    """A w in the row order of k_cg_direction_apply, every operation rounded in T; w is taken as 0 on Dirichlet nodes and
    the result is 0 there"""
    cx, cy, cz, cd = (T(c) for c in coef)
    p = np.array(w, dtype=T)
    p[boundary_mask(p.shape)] = 0
    I = interior(p.ndim)
    q = np.zeros_like(p)

    def nb(axis, off):
        sl = [slice(1, -1)] * p.ndim
        sl[axis] = slice(1 + off, p.shape[axis] - 1 + off)
        return p[tuple(sl)]

    ax_z, ax_y, ax_x = (0, 1, 2) if p.ndim == 3 else (None, 0, 1)
    s = np.zeros_like(p[I])
    if p.ndim == 3:
        s = s + cz * nb(ax_z, -1)
    s = s + cy * nb(ax_y, -1)
    s = s + cx * nb(ax_x, -1)
    s = s + cd * p[I]
    s = s + cx * nb(ax_x, +1)
    s = s + cy * nb(ax_y, +1)
    if p.ndim == 3:
        s = s + cz * nb(ax_z, +1)
    q[I] = s
    return q


def combine_formula(S, C, T):
    """columns of S C by the kernel's contract: each element starts at 0.0 in double, adds (double) S_i * C_ij for i in the
    column order of S (product and sum rounded separately), and is rounded once to T"""
    out = []
    for j in range(C.shape[1]):
        acc = np.zeros(S[0].shape, np.float64)
        for i, s in enumerate(S):
            acc = acc + s.astype(np.float64) * np.float64(C[i, j])
        out.append(acc.astype(T))
    return out


def ld_dot(a, b):
    return float(np.sum(a.astype(np.longdouble) * b.astype(np.longdouble)))


# ---------------------------------------------------------------- the reduced problem
def rayleigh_ritz(G, H, nvec, pivot_min=PIVOT_MIN):
    """the nvec smallest eigenpairs of H c = theta G c by the route of mg_dense.h (diagonal scaling, Cholesky with a pivot
    floor, standard symmetric eigenproblem) with numpy's factorisations -> (theta, C) or None when G is not safely
    positive definite"""
    g = np.diag(G)
    if not (np.all(np.isfinite(G)) and np.all(np.isfinite(H)) and np.all(g > 0)):
        return None
    d = 1.0 / np.sqrt(g)
    Gs, Hs = G * np.outer(d, d), H * np.outer(d, d)
    try:
        L = np.linalg.cholesky(Gs)
    except np.linalg.LinAlgError:
        return None
    if np.min(np.diag(L)) ** 2 <= pivot_min:
        return None
    Li = np.linalg.inv(L)
    As = Li @ Hs @ Li.T
    w, Q = np.linalg.eigh(0.5 * (As + As.T))
    C = (d[:, None] * (Li.T @ Q))[:, :nvec]
    return w[:nvec], C


# ---------------------------------------------------------------- reference LOBPCG
def oracle_preconditioner(kw):
    """M r = one outer iteration of the CPU oracle's mg_solve from zero (as tests/test_pcg_gpu.py::ref_fcg)"""
    S = po.Solver(po.make_desc(**kw))
    pre_gs = kw.get("outer_pre_gs", 2)

    def M(r):
        S.set_rhs(r)
        S.set_solution(np.zeros_like(r))
        if pre_gs:
            S.smooth_fine(po.SMOOTH_GS_LEX, pre_gs)
        S.cycle()
        return S.get_solution()
    return M, S


def lobpcg(coef, X0, nev, tol, maxit, M):
    """The algorithm of mg_eig_solve in numpy, fp64. X0: list of m start vectors.
    -> dict(lam, relres, X, iters, cycles, restarts, status, hist)"""
    shape = X0[0].shape
    bnd = boundary_mask(shape)
    m = len(X0)
    A = lambda v: apply_A(v, coef)
    flat = lambda cols: np.stack([c.ravel() for c in cols], axis=1)
    unflat = lambda Mx: [Mx[:, j].reshape(shape) for j in range(Mx.shape[1])]

    X = flat([np.where(bnd, 0.0, x) for x in X0])
    AX = flat([A(x) for x in unflat(X)])
    rr = rayleigh_ritz(X.T @ X, X.T @ AX, m)
    if rr is None:
        return dict(status=2, iters=0, cycles=0, restarts=0, hist=[])
    theta, C = rr
    X, AX = X @ C, AX @ C
    P = AP = None
    p_cols = []
    iters = cycles = restarts = 0
    hist, status = [], 1
    while True:
        R = AX - X * theta
        relres = np.linalg.norm(R, axis=0) / (np.abs(theta) * np.linalg.norm(X, axis=0))
        hist.append(float(relres[:nev].max()))
        if hist[-1] <= tol:
            status = 0
            break
        if iters == maxit:
            break
        act = [j for j in range(m) if relres[j] > tol]
        if P is not None and all(j in p_cols for j in act):
            keep = [p_cols.index(j) for j in act]
            P, AP = P[:, keep], AP[:, keep]
        else:
            P = AP = None   # first iteration, after a restart, or a column came back from the locked set
        W = flat([np.where(bnd, 0.0, M(r)) for r in unflat(R[:, act])])
        cycles += len(act)
        AW = flat([A(w) for w in unflat(W)])
        for attempt in range(2):
            S = np.hstack([X, W] + ([P] if P is not None else []))
            AS = np.hstack([AX, AW] + ([AP] if P is not None else []))
            G, H = S.T @ S, S.T @ AS
            G[:m, :m], H[:m, :m] = np.eye(m), np.diag(theta)   # what X's orthonormality already gives
            rr = rayleigh_ritz(G, 0.5 * (H + H.T), m)
            if rr is not None or P is None:
                break
            P = AP = None
            restarts += 1
        if rr is None:
            status = 2
            break
        theta, C = rr
        Cp = C[m:, :][:, act]
        P, AP = S[:, m:] @ Cp, AS[:, m:] @ Cp
        X, AX = S @ C, AS @ C
        p_cols = list(act)
        iters += 1
    AX = flat([A(x) for x in unflat(X)])
    rr = rayleigh_ritz(X.T @ X, X.T @ AX, m)
    lam, C = rr
    X, AX = X @ C, AX @ C
    relres = np.linalg.norm(AX - X * lam, axis=0) / np.abs(lam)
    return dict(lam=lam, relres=relres, X=unflat(X), iters=iters, cycles=cycles, restarts=restarts, status=status, hist=hist)


def subspace_sine(x, basis):
    """sine of the angle between the vector x and the span of the orthonormal `basis` vectors"""
    x = x.ravel() / np.linalg.norm(x)
    B = np.stack([b.ravel() for b in basis], axis=1)
    return float(np.linalg.norm(x - B @ (B.T @ x)))
