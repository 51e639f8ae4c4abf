"""bc_ref -- numpy reference of the constant operator with Neumann faces of mg_bc_* (TEST INFRASTRUCTURE, numpy only).

A mask of mg_face bits (x-lo 1, x-hi 2, y-lo 4, y-hi 8, z-lo 16, z-hi 32; x is the fast index) names the Neumann faces. A node
on at least one face that is not in the mask is a Dirichlet node (identity row); every other node is an unknown whose
missing neighbours are mirror images, axis by axis.

One class does both jobs the tests have, as tests/vc_ref.py does:

 * In a working precision (prec = np.float32 / np.float64, the level coefficients taken from the handle with
   use_handle_coefs) every numpy call below is ONE rounded operation of the arithmetic contract of
   multigrid_prj_amd/csrc/mg_bc.hip, in its order:
       residual     sum = 0; sum += cz u(z-); += cy u(y-); += cx u(x-); += cd u_i; += cx u(x+); += cy u(y+); += cz u(z+); r = b - sum
       point solve  the same sum without the diagonal term, ps = (b - sum) / cd
       Jacobi       u' = ps (omega == 1) or u_i + omega * (ps - u_i);  red-black in place with colour (i + j + k) & 1
       restriction  [q hlf q] along x, then y, then z (q * lo + hlf * mid + q * hi), fine neighbours mirrored, coarse
                    Dirichlet nodes injected
   The kernels are compared with it bit for bit.
 * In np.longdouble / np.float64 it is the reference of cycles, of the coarse loop and of mg_bc_solve: the same expressions,
   the prolongation and the cycle recursion of tests/npref.py and tests/npref_cycles.py.

restriction_mode="today" swaps in npref's full weighting (every coarse boundary node injected, which is what mg_restrict
does): kept to show why mg_bc_restrict exists -- the red-black cycle diverges with it.
"""
from __future__ import annotations

import math

import numpy as np

from tests import npref
from tests.npref import parity
from tests.npref_cycles import CycleProblem

XLO, XHI, YLO, YHI, ZLO, ZHI = 1, 2, 4, 8, 16, 32


def all_faces(dim):
    return 63 if dim == 3 else 15


def face_bit(ndim, axis, side):
    """the mg_face bit of the face at the low (side 0) or high (side 1) end of ARRAY axis `axis` (x is the last one)"""
    return 1 << (2 * (ndim - 1 - axis) + side)


def march_side(dim, n, elem_size):
    """mg::bc_march_ok (mg_geom.h) for a cubic level: 3-D, at least 16 full 16-byte vectors per row"""
    return dim == 3 and n // (16 // elem_size) >= 16 and n >= 7


def march_ok(dim, nx, ny, nz, elem_size):
    """mg::bc_march_ok restated"""
    return dim == 3 and nx // (16 // elem_size) >= 16 and ny >= 7 and nz >= 7


class BCProblem(CycleProblem):
    def __init__(self, mask=0, sigma=0.0, restriction_mode="mirror", **kw):
        super().__init__(**kw)
        assert 0 <= mask <= all_faces(self.dim)
        self.mask, self.sigma, self.restriction_mode = mask, sigma, restriction_mode
        # c_a by array axis and the diagonal (shift included); use_handle_coefs replaces them with the handle's doubles
        self.c_axes = [list(self.coefs[l][0]) for l in range(self.L)]
        self.cd = [self.coefs[l][1] + self.prec(sigma) for l in range(self.L)]

    def use_handle_coefs(self, per_level):
        """per_level[l] = (cx, cy, cz, cd) of mg_level_coefficients (cd with the shift): the doubles the kernels cast to T"""
        for l, c in enumerate(per_level):
            self.c_axes[l] = [c[2], c[1], c[0]] if self.dim == 3 else [c[1], c[0]]
            self.cd[l] = c[3]

    def singular(self):
        return self.mask == all_faces(self.dim) and self.sigma == 0

    # -- which nodes are what
    def dirichlet(self, shape):
        """True at the Dirichlet nodes: on at least one face that is not in the mask"""
        nd = len(shape)
        m = np.zeros(shape, bool)
        for ax in range(nd):
            for side in (0, 1):
                if not self.mask & face_bit(nd, ax, side):
                    sl = [slice(None)] * nd
                    sl[ax] = 0 if side == 0 else -1
                    m[tuple(sl)] = True
        return m

    def weights(self, shape):
        """w = product over the axes of 1/2 for each Neumann face the node lies on (float64, exact)"""
        nd = len(shape)
        w = np.ones(shape, np.float64)
        for ax in range(nd):
            v = np.ones(shape[ax])
            if self.mask & face_bit(nd, ax, 0):
                v[0] *= 0.5
            if self.mask & face_bit(nd, ax, 1):
                v[-1] *= 0.5
            w = w * v.reshape([-1 if a == ax else 1 for a in range(nd)])
        return w

    # -- the contract
    def _row_sum(self, u, l, diag, absolute=False):
        """the row's sum at EVERY node with mirrored neighbours (meaningful at the unknowns), in the kernel's order"""
        nd = u.ndim
        up = np.pad(u, 1, mode="reflect")   # index -1 -> 1, n -> n-2: the mirror image
        c = [self.prec(abs(x) if absolute else x) for x in self.c_axes[l]]
        cd = self.prec(abs(self.cd[l]) if absolute else self.cd[l])

        def nb(ax, off):
            sl = [slice(1, -1)] * nd
            sl[ax] = slice(1 + off, up.shape[ax] - 1 + off)
            return up[tuple(sl)]
        s = np.zeros_like(u)
        for ax in range(nd):
            s = s + c[ax] * nb(ax, -1)
        if diag:
            s = s + cd * u
        for ax in reversed(range(nd)):
            s = s + c[ax] * nb(ax, 1)
        return s

    def apply_A(self, u, l, absolute=False):
        u = self.as_prec(u)
        if absolute:
            u = abs(u)
        dm = self.dirichlet(u.shape)
        return np.where(dm, u, self._row_sum(u, l, True, absolute))

    def residual(self, u, b, l):
        return self.as_prec(b) - self.apply_A(u, l)

    def point_solve(self, u, b, l):
        u, b = self.as_prec(u), self.as_prec(b)
        ps = (b - self._row_sum(u, l, False)) / self.prec(self.cd[l])
        return np.where(self.dirichlet(u.shape), b, ps)

    def point_solve_mag(self, u, b, l):
        u, b = abs(self.as_prec(u)), abs(self.as_prec(b))
        ps = (b + self._row_sum(u, l, False, True)) / self.prec(abs(self.cd[l]))
        return np.where(self.dirichlet(u.shape), b, ps)

    def jacobi(self, u, b, l, omega=None):
        om = self.omega if omega is None else self.prec(omega)
        u = self.as_prec(u)
        ps = self.point_solve(u, b, l)
        if om == 1:
            return ps
        return np.where(self.dirichlet(u.shape), ps, u + om * (ps - u))

    # rbgs, smooth, prolong, inject: npref's (rbgs is written on self.point_solve)

    def restrict_fw(self, fine, l):
        if self.restriction_mode == "today":
            return super().restrict_fw(fine, l)
        f = self.as_prec(fine)
        q, h = self.prec(0.25), self.prec(0.5)
        for a in reversed(self._coarsened_axes(l)):   # x first, then y, then z: restrict_fw_point's order
            pw = [(0, 0)] * f.ndim
            pw[a] = (1, 1)
            fp = np.moveaxis(np.pad(f, pw, mode="reflect"), a, -1)
            w = q * fp[..., 0:-2:2] + h * fp[..., 1:-1:2] + q * fp[..., 2::2]
            f = np.moveaxis(w, -1, a)
        inj = self.inject(fine, l)
        dm = self.dirichlet(inj.shape)
        return np.where(dm, inj, f)

    def project(self, v):
        """mg_bc_project -> (v - (T)c, c), c = sum w v / sum w in double"""
        v = self.as_prec(v)
        w = self.weights(v.shape)
        c = math.fsum((w * v.astype(np.float64)).ravel().tolist()) / math.fsum(w.ravel().tolist())
        return v - self.prec(c), c

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

    def restriction_matrix(self, l):
        fs, cs = self.shape(l), self.shape(l + 1)
        R = np.empty((int(np.prod(cs)), int(np.prod(fs))), self.prec)
        e = np.zeros(fs, self.prec)
        for j in range(R.shape[1]):
            e.flat[j] = 1
            R[:, j] = self.restrict_fw(e, l).ravel()
            e.flat[j] = 0
        return R

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

    # -- mg_bc_solve
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


# ---------------------------------------------------------------- the settings of the convergence table
TABLE = {   # name -> (mask, sigma)
    "dirichlet": (0, 0.0),
    "x-lo": (XLO, 0.0),
    "only-y-hi-dirichlet": (63 & ~YHI, 0.0),
    "all-neumann-sigma10": (63, 10.0),
    "all-neumann-singular": (63, 0.0),
}


def convergence_problem(name, smoother=npref.SMOOTH_RBGS, omega=1.0, n=33, levels=4, prec=np.float64, restriction_mode="mirror"):
    """3-D, V(2,2), full weighting, unit cube, alpha = 1"""
    mask, sigma = TABLE[name]
    return BCProblem(mask=mask, sigma=sigma, restriction_mode=restriction_mode, dim=3, n=n, levels=levels, length=1.0, alpha=1.0,
                     smoother=smoother, omega=omega, nu_pre=2, nu_post=2, restriction=npref.RESTRICT_FULLW, outer_pre_gs=0, prec=prec)


def convergence_rhs(shape, seed=1):
    return np.random.default_rng(seed).standard_normal(shape)


# ---------------------------------------------------------------- manufactured solutions (unit box, alpha = 1)
def grid(n, dim):
    x = np.linspace(0.0, 1.0, n)
    return np.meshgrid(*([x] * dim), indexing="ij")[::-1]   # X (fast axis), Y(, Z)


def homogeneous_case(n):
    """all faces Neumann, sigma = 7: u = cos(pi x) cos(2 pi y) cos(pi z) has zero normal derivative on every face -> (mask, sigma, b, u)"""
    X, Y, Z = grid(n, 3)
    u = np.cos(np.pi * X) * np.cos(2 * np.pi * Y) * np.cos(np.pi * Z)
    return 63, 7.0, (7.0 + 6.0 * np.pi ** 2) * u, u


FLUX_MASK = XLO | XHI | YHI   # y-lo stays Dirichlet


def flux_case(n):
    """2-D, u = sin(x + .3) cos(2y), -lap u = 5u; x-lo, x-hi and y-hi carry the exact outward normal derivative g, folded into
    b as +(2 alpha / h) g at the face's nodes (a corner takes one term per face); y-lo is Dirichlet -> (mask, sigma, b, u)"""
    X, Y = grid(n, 2)
    u = np.sin(X + 0.3) * np.cos(2 * Y)
    ux, uy = np.cos(X + 0.3) * np.cos(2 * Y), -2 * np.sin(X + 0.3) * np.sin(2 * Y)
    h = 1.0 / (n - 1)
    b = 5.0 * u
    b[:, 0] += (2.0 / h) * -ux[:, 0]
    b[:, -1] += (2.0 / h) * ux[:, -1]
    b[-1, :] += (2.0 / h) * uy[-1, :]
    b[0, :] = u[0, :]   # Dirichlet data
    return FLUX_MASK, 0.0, b, u


def levels_for(n):
    """down to a 3-point grid"""
    return int(round(math.log2(n - 1)))
