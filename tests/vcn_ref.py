"""vcn_ref -- numpy reference of the variable-coefficient operator with Neumann faces (TEST INFRASTRUCTURE, numpy only):
mg_vc_* after mg_vc_set_faces, multigrid_prj_amd/csrc/mg_vc.hip, DESIGN.md section 22.

    (L u)_i = sigma u_i + sum over the slots z-, y-, x-, x+, y+, z+ of (-c_a / 2) (a_i + a_q)(u_i - u_q)

with q the neighbour, or its MIRROR IMAGE inside the box when the neighbour falls outside through a Neumann face -- for a and
for u alike, so a mirrored slot counts twice. The node classes are tests/bc_ref.py's: a node on at least one face that is not
in the mask (mg_face bits, bc_ref.XLO ...) is a Dirichlet node with an identity row, every other node is an unknown.

As tests/vc_ref.py and tests/bc_ref.py, one class does both jobs:

 * In a working precision (np.float32 / np.float64, the level coefficients taken from the handle with use_handle_coefs)
   every numpy call is ONE rounded operation of the contract, in vc_ref's order: w_a = (T)(-c_a / 2); s = 0, d = (T)sigma;
   per slot g = w_a * (a_i + a_q); s = s + g * u_q; d = d + g; then r = b - (d * u_i - s), ps = (b + s) / d, Jacobi, red-black.
   The kernels are compared with it bit for bit. With mask 0 these are vc_ref's numbers bit for bit.
 * In np.float64 / np.longdouble it is the reference of the cycle, the coarse loop, mg_vc_solve (the singular projection
   included), the weighted flexible CG of mg_vc_pcg_solve and the theta step.

Coarse coefficients and residuals go down by bc_ref's mirrored full weighting (restriction_mode="mirror", what the library
does with a non-zero mask) or by npref's, which injects on every coarse boundary node (restriction_mode="today": kept to
show that the cycle then diverges on a Neumann face).
"""
from __future__ import annotations

import math

import numpy as np

from tests import bc_ref as br
from tests import npref
from tests import vc_ref as vr
from tests.bc_ref import XLO, XHI, YLO, YHI, ZLO, ZHI, all_faces   # noqa: F401  (re-exported: the mask names of the tests)
from tests.step_ref import scalars
from tests.vc_ref import neighbour_order

MIXED = XHI | YHI | ZLO   # Neumann faces that meet Dirichlet ones along edges


def march_side(dim, n, elem_size):
    """mg::march_ok (mg_geom.h) for a cubic level: 3-D, at least 16 full 16-byte vectors per row"""
    return dim == 3 and n // (16 // elem_size) >= 16 and n >= 7


def march_ok(dim, nx, ny, nz, elem_size):
    """mg::march_ok restated"""
    return dim == 3 and nx // (16 // elem_size) >= 16 and ny >= 7 and nz >= 7


class VCNProblem(vr.VCProblem):
    def __init__(self, mask=0, restriction_mode="mirror", **kw):
        super().__init__(**kw)
        assert 0 <= mask <= all_faces(self.dim) and restriction_mode in ("mirror", "today")
        self.mask, self.restriction_mode = mask, restriction_mode

    # -- which nodes are what: bc_ref's definitions, written on self.mask
    dirichlet = br.BCProblem.dirichlet
    node_weights = br.BCProblem.weights   # w = 1/2 per Neumann face of the node (vc_ref's weights(l) are the w_a)
    singular = br.BCProblem.singular

    # -- the contract
    def parts(self, u, l, sigma=None):
        """(s, d) at EVERY node with mirrored neighbours (meaningful at the unknowns), in the kernel's order"""
        a, w, nd = self.a[l], self.weights(l), u.ndim
        up, ap = np.pad(u, 1, mode="reflect"), np.pad(a, 1, mode="reflect")   # index -1 -> 1, n -> n - 2: the mirror image

        def nb(p, ax, off):
            sl = [slice(1, -1)] * nd
            sl[ax] = slice(1 + off, p.shape[ax] - 1 + off)
            return p[tuple(sl)]
        s = np.zeros_like(u)
        d = np.full_like(u, self.prec(self.sigma if sigma is None else sigma))
        for ax, off in neighbour_order(nd):
            g = w[ax] * (a + nb(ap, ax, off))
            s = s + g * nb(up, ax, off)
            d = d + g
        return s, d

    def apply_A(self, u, l, absolute=False, sigma=None):
        u = self.as_prec(u)
        if absolute:
            u = abs(u)
        s, d = self.parts(u, l, sigma)
        return np.where(self.dirichlet(u.shape), u, d * u + s if absolute else d * u - s)

    def point_solve(self, u, b, l):
        u, b = self.as_prec(u), self.as_prec(b)
        s, d = self.parts(u, l)
        return np.where(self.dirichlet(u.shape), b, (b + s) / d)

    def point_solve_mag(self, u, b, l):
        return self.point_solve(abs(self.as_prec(u)), abs(self.as_prec(b)), l)

    def jacobi(self, u, b, l, omega=None):
        om = self.omega if omega is None else self.prec(omega)
        u = self.as_prec(u)
        ps = self.point_solve(u, b, l)
        if om == 1:
            return ps
        return np.where(self.dirichlet(u.shape), ps, u + om * (ps - u))

    # residual, rbgs, smooth, prolong, inject, vcycle, coarse_loop: inherited (written on apply_A / point_solve / restrict_fw)

    def restrict_fw(self, fine, l):
        if self.restriction_mode == "today":
            return npref.Problem.restrict_fw(self, fine, l)
        return br.BCProblem.restrict_fw(self, fine, l)   # mirrored fine neighbours, coarse Dirichlet nodes injected

    def set_a(self, a0, mode="fw"):
        """level l + 1 = the mirrored full weighting of level l with this mask (what mg_vc_set_coefficient / mg_vc_set_faces do)"""
        assert mode == "fw"
        self.a = [self.as_prec(a0)]
        for l in range(self.L - 1):
            self.a.append(self.restrict_fw(self.a[-1], l))

    def project(self, v):
        """mg_vc_project -> (v - (T)c, c), c = sum w v / sum w in double"""
        v = self.as_prec(v)
        w = self.node_weights(v.shape)
        c = math.fsum((w * v.astype(np.float64)).ravel().tolist()) / math.fsum(w.ravel().tolist())
        return v - self.prec(c), c

    def wdot(self, x, y, weighted=True):
        """sum w x y in double (weighted=False: the plain dot)"""
        p = x.astype(np.float64) * y.astype(np.float64)
        return float(np.sum(self.node_weights(x.shape) * p if weighted else p))

    # -- dense matrix of the operator over all nodes (small grids only): column j = L e_j
    def matrix(self, l):
        shape = self.shape(l)
        m = int(np.prod(shape))
        A = np.empty((m, m), self.prec)
        e = np.zeros(shape, self.prec)
        for j in range(m):
            e.flat[j] = 1
            A[:, j] = self.apply_A(e, l).ravel()
            e.flat[j] = 0
        return A

    restriction_matrix = br.BCProblem.restriction_matrix

    # -- the theta step (mg_vc_heat_rhs): tests/step_ref.py's expression with this operator's Dirichlet nodes
    def step_rhs(self, u, f, dt, theta):
        """rhs = ((f + rdt*u) - omt*n0) * rth at the unknowns, u at the Dirichlet nodes; n0 = the UNSHIFTED operator (d from 0)"""
        u = self.as_prec(u)
        rdt, omt, rth = scalars(self.prec, dt, theta)
        t = rdt * u
        if f is not None:
            t = self.as_prec(f) + t
        t = t - omt * self.apply_A(u, 0, sigma=0.0)
        return np.where(self.dirichlet(u.shape), u, t * rth)

    # -- mg_vc_solve
    def solve_history(self, u, b, ncycles, coarse_sweeps, tol=0.0):
        """the singular case projects b first and u last; U = RHS on the Dirichlet nodes; hist[0]; one cycle per entry,
        stopping at <= tol -> (u, hist, b as the solve leaves it, the mean taken out of b or None)"""
        u, b = self.as_prec(u).copy(), self.as_prec(b)
        mean = None
        if self.singular():
            b, mean = self.project(b)
        dm = self.dirichlet(b.shape)
        u[dm] = b[dm]
        nb2 = npref.fsum_sq(b)
        hist = [self.rel_residual(u, b, nb2)]
        for _ in range(ncycles):
            u = self.vcycle(u, b, coarse_sweeps)
            hist.append(self.rel_residual(u, b, nb2))
            if hist[-1] <= tol:
                break
        if self.singular():
            u = self.project(u)[0]
        return u, np.array(hist), b, mean

    # -- mg_vc_pcg_solve
    def fcg(self, x, b, tol, maxit, coarse_sweeps, weighted=True):
        """flexible CG (Polak-Ribiere beta) on L, M r = one cycle from zero, every inner product sum w x y (weighted=False:
        plain dots, kept to show what the weights buy); the stopping test is the plain norm. Singular: b is projected first,
        z after each M, x at the end -> (x, hist)"""
        x, b = self.as_prec(x).copy(), self.as_prec(b)
        sing = self.singular()
        if sing:
            b = self.project(b)[0]
        dm = self.dirichlet(b.shape)
        x[dm] = b[dm]
        nb = math.sqrt(npref.fsum_sq(b))
        dot = lambda p, q: self.prec(self.wdot(p, q, weighted))
        r = self.residual(x, b, 0)
        hist = [math.sqrt(npref.fsum_sq(r)) / nb]
        p = np.zeros_like(b)
        beta, gamma = self.prec(0), None
        for k in range(maxit):
            z = self.vcycle(np.zeros_like(r), r, coarse_sweeps)
            if sing:
                z = self.project(z)[0]
            g2 = dot(z, r)
            if k > 0:
                beta = -alpha * dot(z, q) / gamma
            gamma = g2
            p = z + beta * p
            p[dm] = 0
            q = self.apply_A(p, 0)
            q[dm] = 0
            alpha = gamma / dot(p, q)
            x = x + alpha * p
            r = r - alpha * q
            hist.append(math.sqrt(npref.fsum_sq(r)) / nb)
            if hist[-1] <= tol:
                break
        if sing:
            x = self.project(x)[0]
        return x, np.array(hist)


# ---------------------------------------------------------------- the settings of the convergence table
FIELDS = {"smooth": vr.field_smooth, "aligned": vr.field_jump_aligned, "offgrid": vr.field_jump_offgrid}
FACES = {   # name -> (mask, sigma)
    "x-lo": (XLO, 0.0),
    "mixed": (MIXED, 0.0),
    "only-y-hi-dirichlet": (63 & ~YHI, 0.0),
    "all-neumann-singular": (63, 0.0),
    "all-neumann-sigma10": (63, 10.0),
}


def convergence_problem(field, faces, n=33, levels=4, prec=np.float64, restriction_mode="mirror", smoother=npref.SMOOTH_RBGS, omega=1.0):
    """3-D, red-black V(2,2), full weighting, unit cube, alpha = 1; the coefficient hierarchy is set"""
    mask, sigma = FACES[faces]
    P = VCNProblem(mask=mask, sigma=sigma, restriction_mode=restriction_mode, dim=3, n=n, levels=levels, length=1.0, alpha=1.0,
                   smoother=smoother, omega=omega, nu_pre=2, nu_post=2, restriction=npref.RESTRICT_FULLW, outer_pre_gs=0, prec=prec)
    P.set_a(FIELDS[field](n))
    return P


def convergence_rhs(shape, seed=1):
    return np.random.default_rng(seed).standard_normal(shape)


def cycle_factor(P, ncycles=12, coarse_sweeps=50):
    """(history, the reduction factor of the last cycle) of mg_vc_solve's loop from zero on the standard-normal right-hand side"""
    b = convergence_rhs(P.shape(0)).astype(P.prec)
    hist = P.solve_history(np.zeros_like(b), b, ncycles, coarse_sweeps)[1]
    return hist, float(hist[-1] / hist[-2])


def fcg_iterations(P, weighted, tol=1e-8, maxit=80, coarse_sweeps=50):
    """iterations of the flexible CG to tol; homogeneous Dirichlet data, as vc_ref's Krylov runs"""
    b = convergence_rhs(P.shape(0)).astype(P.prec)
    b[P.dirichlet(b.shape)] = 0
    hist = P.fcg(np.zeros_like(b), b, tol, maxit, coarse_sweeps, weighted=weighted)[1]
    return len(hist) - 1, hist
