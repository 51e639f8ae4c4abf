"""vc_ref -- numpy reference of the variable-coefficient operator of mg_vc_* (TEST INFRASTRUCTURE, numpy only).

    (L u)_i = sigma u_i + sum over axes a of (-c_a / 2) [ (a_i + a_i+)(u_i - u_i+) + (a_i + a_i-)(u_i - u_i-) ]

One class does both jobs the tests have:

 * In a working precision (prec = np.float32 / np.float64, the level coefficients taken from the handle with
   use_handle_coefs) every numpy call below is ONE rounded operation of the arithmetic contract of
   multigrid_prj_amd/csrc/mg_vc.hip, in its order: w_a = (T)(-c_a / 2); s = 0, d = (T)sigma; for the neighbours q in the
   order z-, y-, x-, x+, y+, z+:  g = w_a * (a_i + a_q);  s = s + g * u_q;  d = d + g;  then  r = b - (d * u_i - s),
   ps = (b + s) / d,  Jacobi u' = ps (omega == 1) or u_i + omega * (ps - u_i),  red-black in place with colour
   (i + j + k) & 1. The kernels are compared with it bit for bit.
 * In np.longdouble / np.float64 it is the reference of cycles, of the coarse loop and of the flexible CG: the same
   expressions, the transfers and the cycle recursion of tests/npref.py and tests/npref_cycles.py.

Coarse coefficients: level l + 1 = full weighting of level l (mode="fw", what the library does) or injection
(mode="inject", kept to show why not: it diverges on a jump that is off the coarse grids).
"""
from __future__ import annotations

import math

import numpy as np

from tests import npref
from tests.npref import _interior, _nb, boundary_mask
from tests.npref_cycles import CycleProblem


def neighbour_order(ndim):
    """(array axis, offset) of the neighbours in the residual kernel's row order: z-, y-, x-, x+, y+, z+"""
    return [(ax, -1) for ax in range(ndim)] + [(ax, 1) for ax in reversed(range(ndim))]


class VCProblem(CycleProblem):
    def __init__(self, sigma=0.0, **kw):
        super().__init__(**kw)
        self.sigma = sigma
        self.a = None
        # c_a by array axis as python floats / longdoubles; use_handle_coefs replaces them with the handle's doubles
        self.c_axes = [list(self.coefs[l][0]) for l in range(self.L)]

    def use_handle_coefs(self, per_level):
        """per_level[l] = (cx, cy, cz, cd) of mg_level_coefficients: the doubles the kernels cast to T"""
        for l, c in enumerate(per_level):
            self.c_axes[l] = [c[2], c[1], c[0]] if self.dim == 3 else [c[1], c[0]]

    def set_a(self, a0, mode="fw"):
        self.a = [self.as_prec(a0)]
        for l in range(self.L - 1):
            self.a.append(self.inject(self.a[-1], l) if mode == "inject" else self.restrict_fw(self.a[-1], l))

    def weights(self, l):
        """w_a = (T)(-c_a / 2): the division in the coefficient's own precision (fp64 for the handle's), then the cast"""
        return [self.prec(-c / 2) for c in self.c_axes[l]]

    # -- the contract
    def parts(self, u, l):
        """(s, d) at the interior nodes"""
        a, w, I = self.a[l], self.weights(l), _interior(u.ndim)
        ai = a[I]
        s = np.zeros_like(ai)
        d = np.full_like(ai, self.prec(self.sigma))
        for ax, off in neighbour_order(u.ndim):
            g = w[ax] * (ai + _nb(a, ax, off))
            s = s + g * _nb(u, ax, off)
            d = d + g
        return s, d

    def apply_A(self, u, l, absolute=False):
        u = self.as_prec(u)
        if absolute:
            u = abs(u)
        out = u.copy()
        I = _interior(u.ndim)
        s, d = self.parts(u, l)
        out[I] = d * u[I] + s if absolute else d * u[I] - s
        return out

    def point_solve(self, u, b, l):
        u, b = self.as_prec(u), self.as_prec(b)
        out = b.copy()
        I = _interior(u.ndim)
        s, d = self.parts(u, l)
        out[I] = (b[I] + s) / d
        return out

    def point_solve_mag(self, u, b, l):
        u, b = abs(self.as_prec(u)), abs(self.as_prec(b))
        out = b.copy()
        I = _interior(u.ndim)
        s, d = self.parts(u, l)
        out[I] = (b[I] + s) / d
        return out

    def jacobi(self, u, b, l, omega=None):
        om = self.omega if omega is None else self.prec(omega)
        u = self.as_prec(u)
        ps = self.point_solve(u, b, l)
        if om == 1:
            return ps
        out = ps.copy()
        I = _interior(u.ndim)
        out[I] = u[I] + om * (ps[I] - u[I])
        return out

    # -- the interior matrix (small grids only): column j = L e_j
    def interior_matrix(self, l):
        shape = self.shape(l)
        I = _interior(len(shape))
        m = int(np.prod([n - 2 for n in shape]))
        A = np.empty((m, m), self.prec)
        e = np.zeros(shape, self.prec)
        ei = e[I]
        for j in range(m):
            ei.flat[j] = 1
            A[:, j] = self.apply_A(e, l)[I].ravel()
            ei.flat[j] = 0
        return A

    # -- the coarse loop (Solver::Solve with maxit, tol, fixed), every norm it tests recorded
    def coarse_loop(self, u, rhs, l, maxit, tol, fixed):
        """-> (u, iters, flag, relres, [relres tested])"""
        nb2 = npref.fsum_sq(rhs)
        rel = lambda v: math.sqrt(npref.fsum_sq(self.residual(v, rhs, l)) / nb2)
        u = self.as_prec(u)
        sm = self.coarse_smoother()
        if fixed:
            u = self.smooth(sm, maxit, u, rhs, l)
            r = rel(u)
            return u, maxit, 0, r, [r]
        tested = [rel(u)]
        iters, counter, flag = 0, maxit, 0
        while tested[-1] > tol:
            if counter == 0:
                flag = 1
                break
            u = self.smooth(sm, 1, u, rhs, l)
            counter -= 1
            iters += 1
            tested.append(rel(u))
        return u, iters, flag, tested[-1], tested

    # -- the outer loops
    def cycle_history(self, u, b, ncycles, coarse_sweeps):
        """mg_vc_solve: U = RHS on the Dirichlet nodes, hist[0], one cycle per entry -> (u, hist)"""
        u, b = self.as_prec(u).copy(), self.as_prec(b)
        bm = boundary_mask(b.shape)
        u[bm] = b[bm]
        nb2 = npref.fsum_sq(b)
        hist = [self.rel_residual(u, b, nb2)]
        for _ in range(ncycles):
            u = self.vcycle(u, b, coarse_sweeps)
            hist.append(self.rel_residual(u, b, nb2))
        return u, np.array(hist)

    def fcg(self, x, b, tol, maxit, coarse_sweeps):
        """mg_vc_pcg_solve: flexible CG (Polak-Ribiere beta) on L, M r = one cycle from zero -> (x, hist)"""
        x, b = self.as_prec(x).copy(), self.as_prec(b)
        bm = boundary_mask(b.shape)
        x[bm] = b[bm]
        nb = math.sqrt(npref.fsum_sq(b))
        M = lambda r: self.vcycle(np.zeros_like(r), r, coarse_sweeps)
        r = self.residual(x, b, 0)
        hist = [math.sqrt(npref.fsum_sq(r)) / nb]
        p = np.zeros_like(b)
        beta, gamma = self.prec(0), None
        for k in range(maxit):
            z = M(r)
            g2 = (z * r).sum()
            if k > 0:
                beta = -alpha * (z * q).sum() / gamma
            gamma = g2
            p = z + beta * p
            p[bm] = 0
            q = self.apply_A(p, 0)
            q[bm] = 0
            alpha = gamma / (p * q).sum()
            x = x + alpha * p
            r = r - alpha * q
            hist.append(math.sqrt(npref.fsum_sq(r)) / nb)
            if hist[-1] <= tol:
                break
        return x, np.array(hist)


# ---------------------------------------------------------------- the fields of the convergence tests (level-0 node coordinates in [0, 1])
def grid(n, dim=3):
    x = np.linspace(0.0, 1.0, n)
    return np.meshgrid(*([x] * dim), indexing="ij")[::-1]   # X (fast axis), Y, Z


def field_smooth(n):
    X, Y, Z = grid(n)
    return np.exp(math.log(10.0) * np.sin(2 * np.pi * X) * np.cos(2 * np.pi * Y) * np.cos(np.pi * Z))


def field_jump_aligned(n, c=1000.0):
    X, Y, Z = grid(n)
    return np.where((abs(X - .5) <= .25) & (abs(Y - .5) <= .25) & (abs(Z - .5) <= .25), c, 1.0)


def field_jump_offgrid(n, c=1000.0):
    X, Y, Z = grid(n)
    return np.where((abs(X - .47) <= .2) & (abs(Y - .5) <= .27) & (abs(Z - .55) <= .22), c, 1.0)


def convergence_problem(smoother=npref.SMOOTH_RBGS, omega=1.0, n=33, levels=5, prec=np.float64):
    """the setting of the convergence table: 3-D, V(2,2), full weighting, unit cube, alpha = 1"""
    return VCProblem(dim=3, n=n, levels=levels, length=1.0, alpha=1.0, smoother=smoother, omega=omega, nu_pre=2, nu_post=2,
                     restriction=npref.RESTRICT_FULLW, outer_pre_gs=0, prec=prec)


def convergence_rhs(shape, seed=1, zero_boundary=False):
    """standard normal values; the cycle histories keep them on the Dirichlet nodes too (boundary data), the Krylov runs
    take homogeneous boundary data"""
    b = np.random.default_rng(seed).standard_normal(shape)
    if zero_boundary:
        b[boundary_mask(shape)] = 0
    return b


def march_side(dim, n, elem_size):
    """mg::vc_march_ok (mg_geom.h) for a cubic level: 3-D, at least 16 full 16-byte vectors per row"""
    return dim == 3 and n // (16 // elem_size) >= 16 and n >= 7
