"""npref -- an independent high-precision reference of every multigrid operator (TEST INFRASTRUCTURE, numpy only).

Written from the definitions (include/mg_desc.h, DESIGN.md §2, the mathematics of each operator), not from the CPU
oracle's loops, and with whole-array slicing instead of point loops, so that a transcription error shared with the
oracle or the kernels is unlikely. It imports nothing from oracle/ and nothing from the product package.

Conventions (mg_desc.h): a level is an array of shape (n, n) in 2-D, indexed [j, i], or (nz, n, n) in 3-D, indexed
[k, j, i]; x is the fast axis i, z the slow axis k. Nodes with an index 0 or last on any axis are Dirichlet nodes, whose
matrix rows are identity rows. Interior rows of A are  cd u + sum_axes c_a (u[-1] + u[+1])  with
    c_a = -alpha aniso_a / h_a^2,   cd = -2 sum_a c_a,
h_a the level's mesh width along axis a: h = length/(n-1) * 2^l in x and y, and in z h_z = length/(n-1) * 2^(l - s)
(0 while l <= s) for s = semi_xy leading semi-coarsenings (transitions l -> l+1 with l < s keep z).

Precision: everything is computed in `prec` (np.longdouble by default, float64 for large grids); inputs are cast
exactly from their working dtype.
"""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
SMOOTH_GS_LEX, SMOOTH_JACOBI, SMOOTH_RBGS, SMOOTH_ZEBRA_Y, SMOOTH_ZEBRA_X = 0, 1, 2, 3, 4
CYCLE_SAWTOOTH, CYCLE_V = 0, 1
RESTRICT_INJECT, RESTRICT_FULLW = 0, 1


# ---------------------------------------------------------------- array helpers
def _interior(ndim):
    return (slice(1, -1),) * ndim


def _nb(a, axis, off):
    """the neighbour at offset `off` along `axis` of every interior node (shape of the interior)"""
    sl = [slice(1, -1)] * a.ndim
    sl[axis] = slice(1 + off, a.shape[axis] - 1 + off)
    return a[tuple(sl)]


_PAR = {}


def parity(shape, axes=None):
    """(sum of the indices over `axes`, all axes by default) & 1"""
    key = (tuple(shape), None if axes is None else tuple(axes))
    if key not in _PAR:
        idx = np.indices(shape)
        ax = range(len(shape)) if axes is None else axes
        _PAR[key] = (sum(idx[a] for a in ax) & 1).astype(np.int8)
    return _PAR[key]


def boundary_mask(shape):
    m = np.ones(shape, bool)
    m[_interior(len(shape))] = False
    return m


def fsum_sq(a) -> float:
    """sum of squares, exactly rounded once (math.fsum over the squares taken in the array's precision)"""
    return math.fsum((np.asarray(a).ravel().astype(LD) ** 2).astype(np.float64).tolist())


# ---------------------------------------------------------------- the problem
class Problem:
    """Level geometry, coefficients and every operator of one descriptor (the keyword arguments of make_desc;
    dtype / coarse_mode / coarse_tol / dist_min_n are accepted and ignored: counts of coarse sweeps are explicit)."""

    def __init__(self, dim=2, n=17, levels=2, length=10.0, alpha=1.0, cycle=CYCLE_SAWTOOTH, smoother=SMOOTH_JACOBI,
                 omega=1.0, nu_pre=0, nu_post=5, restriction=RESTRICT_INJECT, coarse_maxit=2000, outer_pre_gs=2,
                 aniso=(1.0, 1.0, 1.0), semi_xy=0, prec=LD, **_ignored):
        assert dim in (2, 3) and levels >= 1 and (n - 1) % (1 << (levels - 1)) == 0
        assert 0 <= semi_xy <= levels - 1 and (semi_xy == 0 or dim == 3)
        self.dim, self.L, self.prec = dim, levels, prec
        self.cycle_kind, self.smoother, self.restriction = cycle, smoother, restriction
        self.nu_pre, self.nu_post, self.coarse_maxit, self.outer_pre_gs = nu_pre, nu_post, coarse_maxit, outer_pre_gs
        self.omega = prec(omega)
        self.n, self.nz, self.semi = [], [], []
        nl, nzl = n, n
        for l in range(levels):
            self.n.append(nl)
            self.nz.append(nzl if dim == 3 else 1)
            semi = dim == 3 and l < semi_xy
            self.semi.append(semi)
            nl = (nl - 1) // 2 + 1
            if not semi:
                nzl = (nzl - 1) // 2 + 1
        h0 = prec(length) / prec(n - 1)
        a = [prec(x) for x in aniso]
        self.coefs = []
        for l in range(levels):
            h = h0 * prec(2 ** l)
            hz = h0 * prec(2 ** max(l - semi_xy, 0))
            cx = -prec(alpha) * a[0] / (h * h)
            cy = -prec(alpha) * a[1] / (h * h)
            cz = -prec(alpha) * a[2] / (hz * hz)
            ax = [cz, cy, cx] if dim == 3 else [cy, cx]   # by array axis
            self.coefs.append((ax, -2 * sum(ax)))

    # -- geometry
    def shape(self, l):
        return (self.n[l], self.n[l]) if self.dim == 2 else (self.nz[l], self.n[l], self.n[l])

    def coef(self, l):
        """(off-diagonals by array axis, diagonal)"""
        return self.coefs[l]

    def as_prec(self, a):
        return np.asarray(a).astype(self.prec)

    # -- the operator
    def offdiag(self, u, l, axes=None, absolute=False):
        """sum over `axes` (all by default) of c_a (u[-1] + u[+1]) at the interior nodes"""
        ca, _ = self.coefs[l]
        s = 0
        for a in (range(u.ndim) if axes is None else axes):
            c = abs(ca[a]) if absolute else ca[a]
            s = s + c * (_nb(u, a, -1) + _nb(u, a, 1))
        return s

    def apply_A(self, u, l, absolute=False):
        """A u; absolute=True: |A| |u|, the magnitude that bounds the rounding of any evaluation of A u"""
        u = self.as_prec(u)
        if absolute:
            u = abs(u)
        cd = self.coefs[l][1]
        out = u.copy()
        I = _interior(u.ndim)
        out[I] = (abs(cd) if absolute else cd) * u[I] + self.offdiag(u, l, absolute=absolute)
        return out

    def residual(self, u, b, l):
        return self.as_prec(b) - self.apply_A(u, l)

    def point_solve(self, u, b, l):
        """the value of every node that satisfies its own row with all neighbours at u: D^-1 (b - (A - D) u)"""
        u, b = self.as_prec(u), self.as_prec(b)
        out = b.copy()
        I = _interior(u.ndim)
        out[I] = (b[I] - self.offdiag(u, l)) / self.coefs[l][1]
        return out

    def point_solve_mag(self, u, b, l):
        """|D|^-1 (|b| + |A - D| |u|): bounds the rounding of point_solve"""
        u, b = abs(self.as_prec(u)), abs(self.as_prec(b))
        out = b.copy()
        I = _interior(u.ndim)
        out[I] = (b[I] + self.offdiag(u, l, absolute=True)) / abs(self.coefs[l][1])
        return out

    # -- smoothers (one sweep each)
    def jacobi(self, u, b, l, omega=None):
        om = self.omega if omega is None else self.prec(omega)
        u = self.as_prec(u)
        ps = self.point_solve(u, b, l)
        out = ps.copy()
        I = _interior(u.ndim)
        out[I] = u[I] + om * (ps[I] - u[I])
        return out

    def rbgs(self, u, b, l):
        """red-black Gauss-Seidel: colour (i+j+k) & 1, colour 0 first; Dirichlet nodes take b with their colour"""
        u = self.as_prec(u).copy()
        par = parity(u.shape)
        for colour in (0, 1):
            u = np.where(par == colour, self.point_solve(u, b, l), u)
        return u

    def gs_lex(self, u, b, l):
        """lexicographic Gauss-Seidel. A node reads its lower neighbours (index - 1 on some axis) new and its upper ones
        old, so the lexicographic order gives the same values as the order of diagonal planes sum(index) = s, which is
        what is vectorised here."""
        u = self.as_prec(u).copy()
        b = self.as_prec(b)
        ca, cd = self.coefs[l]
        shape = u.shape
        strides = [int(np.prod(shape[a + 1:])) for a in range(len(shape))]
        idx = np.indices(shape).reshape(len(shape), -1)
        diag = idx.sum(0)
        bnd = boundary_mask(shape).ravel()
        order = np.argsort(diag, kind="stable")
        cuts = np.searchsorted(diag[order], np.arange(diag.max() + 2))
        uf, bf = u.ravel(), b.ravel()
        for s in range(diag.max() + 1):
            p = order[cuts[s]:cuts[s + 1]]
            pb, pi = p[bnd[p]], p[~bnd[p]]
            uf[pb] = bf[pb]
            acc = 0
            for a, st in enumerate(strides):
                acc = acc + ca[a] * (uf[pi - st] + uf[pi + st])
            uf[pi] = (bf[pi] - acc) / cd
        return uf.reshape(shape)

    def zebra(self, u, b, l, line_axis):
        """zebra line Gauss-Seidel: every line along `line_axis` (array axis) whose other indices have parity `colour`
        is solved exactly for its own nodes (colour 0 first), the nodes off the line held at their current values.
        Lines that lie in the boundary and the two end nodes of every line are Dirichlet nodes (= b)."""
        u = self.as_prec(u).copy()
        b = self.as_prec(b)
        ca, cd = self.coefs[l]
        cl = ca[line_axis]
        others = [a for a in range(u.ndim) if a != line_axis]
        par = parity(u.shape, others)
        I = _interior(u.ndim)
        for colour in (0, 1):
            r = b[I] - self.offdiag(u, l, axes=others)
            # the known end values move to the right-hand side
            first = [slice(1, -1)] * u.ndim; first[line_axis] = slice(0, 1)
            last = [slice(1, -1)] * u.ndim; last[line_axis] = slice(-1, None)
            r = np.moveaxis(r, line_axis, -1).copy()
            r[..., 0] -= cl * np.moveaxis(b[tuple(first)], line_axis, -1)[..., 0]
            r[..., -1] -= cl * np.moveaxis(b[tuple(last)], line_axis, -1)[..., 0]
            x = tridiag_solve_const(cl, cd, r)
            new = b.copy()
            new[I] = np.moveaxis(x, -1, line_axis)
            u = np.where(par == colour, new, u)
        return u

    def smooth(self, smoother, sweeps, u, b, l, omega=None):
        u = self.as_prec(u)
        for _ in range(sweeps):
            if smoother == SMOOTH_JACOBI:
                u = self.jacobi(u, b, l, omega)
            elif smoother == SMOOTH_RBGS:
                u = self.rbgs(u, b, l)
            elif smoother == SMOOTH_ZEBRA_Y:
                u = self.zebra(u, b, l, u.ndim - 2)
            elif smoother == SMOOTH_ZEBRA_X:
                u = self.zebra(u, b, l, u.ndim - 1)
            elif smoother == SMOOTH_GS_LEX:
                u = self.gs_lex(u, b, l)
            else:
                raise ValueError(smoother)
        return u

    def coarse_smoother(self):
        """the coarsest-grid solver of a zebra hierarchy smooths with red-black GS (mg_desc.h)"""
        return SMOOTH_RBGS if self.smoother in (SMOOTH_ZEBRA_Y, SMOOTH_ZEBRA_X) else self.smoother

    # -- transfers between level l (fine) and l + 1 (coarse)
    def _coarsened_axes(self, l):
        nd = self.dim
        return [a for a in range(nd) if not (self.semi[l] and a == 0)]

    def inject(self, fine, l):
        sl = tuple(slice(None, None, 2) if a in self._coarsened_axes(l) else slice(None) for a in range(fine.ndim))
        return self.as_prec(fine)[sl].copy()

    def restrict_fw(self, fine, l):
        """tensor product of [1 2 1]/4 along the coarsened axes at interior coarse nodes, injection on the coarse
        boundary"""
        f = self.as_prec(fine)
        q, h = self.prec(0.25), self.prec(0.5)
        for a in self._coarsened_axes(l):
            f = np.moveaxis(f, a, -1)
            w = f[..., ::2].copy()
            w[..., 1:-1] = q * f[..., 1:-2:2] + h * f[..., 2:-1:2] + q * f[..., 3::2]
            f = np.moveaxis(w, -1, a)
        inj = self.inject(fine, l)
        bm = boundary_mask(inj.shape)
        f[bm] = inj[bm]
        return f

    def prolong(self, coarse, l):
        """P coarse on level l: tensor-product linear interpolation along the coarsened axes"""
        c = self.as_prec(coarse)
        h = self.prec(0.5)
        for a in self._coarsened_axes(l):
            c = np.moveaxis(c, a, -1)
            nc = c.shape[-1]
            f = np.empty(c.shape[:-1] + (2 * nc - 1,), c.dtype)
            f[..., ::2] = c
            f[..., 1::2] = h * (c[..., :-1] + c[..., 1:])
            c = np.moveaxis(f, -1, a)
        return c

    # -- cycles (u, b on level 0; `counts` = coarse sweeps, an int or a per-call iterator)
    def coarse_solve(self, e, rhs, l, sweeps):
        return self.smooth(self.coarse_smoother(), sweeps, e, rhs, l)

    def vcycle(self, u, b, coarse_sweeps, l=0):
        if l == self.L - 1:
            return self.coarse_solve(u, b, l, coarse_sweeps)
        u = self.smooth(self.smoother, self.nu_pre, u, b, l)
        r = self.residual(u, b, l)
        rc = self.restrict_fw(r, l) if self.restriction == RESTRICT_FULLW else self.inject(r, l)
        ec = self.vcycle(np.zeros(self.shape(l + 1), self.prec), rc, coarse_sweeps, l + 1)
        u = u + self.prolong(ec, l)
        return self.smooth(self.smoother, self.nu_post, u, b, l)

    def sawtooth(self, u, b, coarse_sweeps):
        """the reference cycle: fine residual injected to every level, coarse solve from zero, then coarse to fine
        e_l = P e_{l+1} followed by nu_post sweeps on A_l e_l = r_l, finally u += e_0"""
        u = self.as_prec(u)
        r = [self.residual(u, b, 0)]
        for l in range(self.L - 1):
            r.append(self.inject(r[-1], l))
        e = self.coarse_solve(np.zeros(self.shape(self.L - 1), self.prec), r[-1], self.L - 1, coarse_sweeps)
        for l in range(self.L - 2, -1, -1):
            e = self.smooth(self.smoother, self.nu_post, self.prolong(e, l), r[l], l)
        return u + e

    def cycle(self, u, b, coarse_sweeps):
        return self.vcycle(self.as_prec(u), self.as_prec(b), coarse_sweeps) if self.cycle_kind == CYCLE_V \
            else self.sawtooth(u, b, coarse_sweeps)

    def rel_residual(self, u, b, nb2=None) -> float:
        nb2 = fsum_sq(b) if nb2 is None else nb2
        return math.sqrt(fsum_sq(self.residual(u, b, 0)) / nb2)

    def solve(self, u, b, coarse_counts, tol=0.0):
        """outer loop: hist[0] = |r(u)|/|b|; per trip outer_pre_gs lexicographic GS sweeps on level 0, one cycle whose
        coarse solve spends coarse_counts[trip] sweeps, hist += |r|/|b|; stops at <= tol or after len(coarse_counts)
        trips. Norms are sums of squares over every node, boundary included."""
        u, b = self.as_prec(u), self.as_prec(b)
        nb2 = fsum_sq(b)
        hist = [self.rel_residual(u, b, nb2)]
        for cnt in coarse_counts:
            u = self.smooth(SMOOTH_GS_LEX, self.outer_pre_gs, u, b, 0)
            u = self.cycle(u, b, int(cnt))
            hist.append(self.rel_residual(u, b, nb2))
            if hist[-1] <= tol:
                break
        return u, np.array(hist)


def tridiag_solve_const(off, diag, r):
    """solves, along the last axis of r and for every line at once, the system with `diag` on the diagonal and `off`
    on both off-diagonals (Thomas algorithm: elimination downwards, substitution upwards)"""
    m = r.shape[-1]
    cp = np.empty(m, r.dtype)
    dp = np.empty_like(r)
    piv = diag
    cp[0] = off / piv
    dp[..., 0] = r[..., 0] / piv
    for j in range(1, m):
        piv = diag - off * cp[j - 1]
        cp[j] = off / piv
        dp[..., j] = (r[..., j] - off * dp[..., j - 1]) / piv
    x = np.empty_like(r)
    x[..., -1] = dp[..., -1]
    for j in range(m - 2, -1, -1):
        x[..., j] = dp[..., j] - cp[j] * x[..., j + 1]
    return x


def line_amplification(P: Problem, l, line_axis):
    """|D| / (|D| - 2|c_line|): bound of the max-norm growth of a line solve relative to a point solve"""
    ca, cd = P.coef(l)
    return float(abs(cd) / (abs(cd) - 2 * abs(ca[line_axis])))
