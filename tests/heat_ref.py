"""heat_ref -- numpy references of the implicit heat-equation stepper (TEST INFRASTRUCTURE; mg_heat_step, include/mg_hip.h).

* heat_rhs_np: the arithmetic contract of mg_heat.hip restated in the working dtype, one rounding per operation;
* ThetaStepper: the theta scheme for u_t = -A0 u + f on tests/npref.Problem in high precision, its linear solves done by a
  callback (dense, or a fixed number of npref sweeps and cycles);
* the lowest discrete sine mode, its eigenvalue and the extreme eigenvalues of A0, for closed-form checks.
"""
from __future__ import annotations

import math

import numpy as np

from tests.npref import Problem, boundary_mask, SMOOTH_GS_LEX


def interior(ndim):
    return (slice(1, -1),) * ndim


def _nb(u, axis, off):
    sl = [slice(1, -1)] * u.ndim
    sl[axis] = slice(1 + off, u.shape[axis] - 1 + off)
    return u[tuple(sl)]


def stencil_np(u, coef):
    """(((((((0 + cz u[k-1]) + cy u[j-1]) + cx u[i-1]) + cd u) + cx u[i+1]) + cy u[j+1]) + cz u[k+1]) at the interior nodes, in
    u's dtype, every operation rounded separately (cz terms absent in 2-D)"""
    dt = u.dtype.type
    cx, cy, cz, cd = (dt(c) for c in coef)
    I = interior(u.ndim)
    ax_z, ax_y, ax_x = (0, 1, 2) if u.ndim == 3 else (None, 0, 1)
    s = np.zeros_like(u[I])
    if u.ndim == 3:
        s = s + cz * _nb(u, ax_z, -1)
    s = s + cy * _nb(u, ax_y, -1)
    s = s + cx * _nb(u, ax_x, -1)
    s = s + cd * u[I]
    s = s + cx * _nb(u, ax_x, +1)
    s = s + cy * _nb(u, ax_y, +1)
    if u.ndim == 3:
        s = s + cz * _nb(u, ax_z, +1)
    return s


def relres_ld(u, b, coef):
    """||b - A u|| / ||b|| over all nodes in long double, A given by coef = (cx, cy, cz, cd) exactly as passed (the fp64
    values a handle reports: the operator the library applies, its shifted diagonal being ONE fp64 addition)"""
    LD = np.longdouble
    u, b = np.asarray(u).astype(LD), np.asarray(b).astype(LD)
    r = b - u                                   # Dirichlet rows are identity rows
    I = interior(u.ndim)
    r[I] = b[I] - stencil_np(u, coef)
    return float(np.sqrt(np.sum(r * r) / np.sum(b * b)))


def heat_rhs_np(u, f, coef0, dt, theta, general=True):
    """the contract of mg_heat_rhs: rhs = ((f + rdt u) - omt s) rth inside (f may be None), u on Dirichlet nodes;
    general=False: the stencil-free form of theta == 1, f + rdt u"""
    T = u.dtype.type
    rdt, omt, rth = T(1.0 / dt), T(1.0 - theta), T(1.0 / theta)
    I = interior(u.ndim)
    t = rdt * u[I]
    if f is not None:
        t = f[I] + t
    if general:
        t = (t - omt * stencil_np(u, coef0)) * rth
    out = u.copy()
    out[I] = t
    return out


def lowest_mode(shape, dtype=np.float64):
    """prod_axes sin(pi i / (n - 1)): the eigenvector of A0 with the smallest eigenvalue; zero on the boundary"""
    u = np.ones(shape, np.longdouble)
    for a, n in enumerate(shape):
        s = np.sin(np.pi * np.arange(n, dtype=np.longdouble) / (n - 1))
        s[0] = s[-1] = 0
        u = u * s.reshape([-1 if i == a else 1 for i in range(len(shape))])
    return u.astype(dtype)


def eigen_range(P: Problem, l=0):
    """(lam_min, lam_max) of the interior block of A0 on level l: sum_axes 4 |c_a| sin^2(k pi / (2 (n_a - 1))), k = 1, n_a - 2"""
    ca, _ = P.coef(l)
    shape = P.shape(l)
    lo = sum(4 * abs(float(c)) * math.sin(math.pi / (2 * (n - 1))) ** 2 for c, n in zip(ca, shape))
    hi = sum(4 * abs(float(c)) * math.sin((n - 2) * math.pi / (2 * (n - 1))) ** 2 for c, n in zip(ca, shape))
    return lo, hi


def growth(theta, dt, lam):
    """amplification of an eigenmode per theta-scheme step"""
    return (1 - (1 - theta) * dt * lam) / (1 + theta * dt * lam)


def shifted_problem(kw, sigma, prec=np.longdouble):
    """npref.Problem of sigma I + A on every level: coefs[l] = (ax, cd + sigma)"""
    P = Problem(**kw, prec=prec)
    P.coefs = [(ax, cd + prec(sigma)) for ax, cd in P.coefs]
    return P


class ThetaStepper:
    """u_t = -A0 u + f by the theta scheme on npref.Problem(**kw); solve(Ps, u, rhs) -> u' returns the (approximate)
    solution of (sigma I + A0) u' = rhs started from u, Ps = shifted_problem(kw, sigma)"""

    def __init__(self, kw, dt, theta, solve, prec=np.longdouble):
        self.P0 = Problem(**kw, prec=prec)
        self.dt, self.theta, self.prec = prec(dt), prec(theta), prec
        self.sigma = 1.0 / (float(theta) * float(dt))   # the fp64 value the library uses
        self.Ps = shifted_problem(kw, self.sigma, prec)
        self.solve = solve

    def rhs(self, u, f):
        u = self.P0.as_prec(u)
        I = interior(u.ndim)
        out = u.copy()
        t = u[I] / self.dt - (1 - self.theta) * self.P0.apply_A(u, 0)[I]
        if f is not None:
            t = t + self.P0.as_prec(f)[I]
        out[I] = t / self.theta
        return out

    def step(self, u, f=None):
        b = self.rhs(u, f)
        return self.solve(self.Ps, self.P0.as_prec(u), b), b


def dense_solver(Ps, u, b):
    """exact solve of the interior block (float64 LAPACK), Dirichlet values from b"""
    ax, cd = Ps.coef(0)
    shp = b.shape
    m = [s - 2 for s in shp]
    eye = [np.eye(k) for k in m]
    off = [np.eye(k, k=1) + np.eye(k, k=-1) for k in m]
    A = float(cd) * np.eye(int(np.prod(m)))
    for a in range(len(shp)):
        mats = [off[i] if i == a else eye[i] for i in range(len(shp))]
        K = mats[0]
        for M_ in mats[1:]:
            K = np.kron(K, M_)
        A += float(ax[a]) * K
    xb = np.where(boundary_mask(shp), b, 0)
    r = np.asarray(b - Ps.apply_A(xb, 0), np.float64)[interior(len(shp))].ravel()
    x = np.asarray(xb, np.float64).copy()
    x[interior(len(shp))] = np.linalg.solve(A, r).reshape(m)
    return Ps.as_prec(x)


def cycle_solver(cycles, coarse_sweeps):
    """`cycles` outer iterations of mg_solve: outer_pre_gs lexicographic GS sweeps + one cycle with coarse_sweeps coarse sweeps"""
    def solve(Ps, u, b):
        for _ in range(cycles):
            u = Ps.smooth(SMOOTH_GS_LEX, Ps.outer_pre_gs, u, b, 0)
            u = Ps.cycle(u, b, coarse_sweeps)
        return u
    return solve
