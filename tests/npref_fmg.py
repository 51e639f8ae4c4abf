"""npref_fmg -- independent reference of full multigrid (mg_fmg) and of its interpolation (TEST INFRASTRUCTURE, numpy only).

Restates include/mg_hip.h's description of mg_fmg / mg_fmg_prolong on top of npref.Problem: whole-array slicing, computed
in the Problem's precision (long double by default). Imports nothing from oracle/ and nothing from the product package.

The FMG interpolation Pi is the tensor product, over the axes a transition coarsens, of the 1-D rule on a coarse row
c[0..nc-1], fine row f[0..2nc-2]:
    f[2m]   = c[m]
    f[2m+1] = (-c[m-1] + 9 c[m] + 9 c[m+1] - c[m+2]) / 16      where all four exist (cubic Lagrange at the midpoint)
    f[1]    = (3 c[0] + 6 c[1] - c[2]) / 8, mirrored at the other end   (quadratic Lagrange through the three end nodes)
Axes a transition keeps (z of a semi-coarsened one) are copied.
"""
from __future__ import annotations

import numpy as np

from tests.npref import RESTRICT_FULLW, Problem, boundary_mask


def _rule_last_axis(c, absolute):
    nc = c.shape[-1]
    assert nc >= 3
    s = -1 if not absolute else 1
    f = np.empty(c.shape[:-1] + (2 * nc - 1,), c.dtype)
    f[..., ::2] = c
    odd = np.empty(c.shape[:-1] + (nc - 1,), c.dtype)
    if nc >= 4:
        odd[..., 1:-1] = (s * c[..., :-3] + 9 * c[..., 1:-2] + 9 * c[..., 2:-1] + s * c[..., 3:]) / 16
    odd[..., 0] = (3 * c[..., 0] + 6 * c[..., 1] + s * c[..., 2]) / 8
    odd[..., -1] = (3 * c[..., -1] + 6 * c[..., -2] + s * c[..., -3]) / 8
    f[..., 1::2] = odd
    return f


def cubic_prolong(P: Problem, coarse, l, bnd=None, absolute=False):
    """Pi coarse on level l (coarse lives on level l + 1). bnd: an array of level l whose values the fine Dirichlet nodes
    take instead of being interpolated. absolute=True: |Pi| |coarse|, the weights' magnitudes applied to the values'
    magnitudes -- what bounds the rounding of any evaluation of Pi coarse."""
    c = P.as_prec(coarse)
    if absolute:
        c = abs(c)
    for a in P._coarsened_axes(l):
        c = np.moveaxis(_rule_last_axis(np.moveaxis(c, a, -1), absolute), -1, a)
    c = np.ascontiguousarray(c)
    assert c.shape == P.shape(l)
    if bnd is not None:
        bm = boundary_mask(c.shape)
        c[bm] = (abs(P.as_prec(bnd)) if absolute else P.as_prec(bnd))[bm]
    return c


def restrict_rhs(P: Problem, b):
    """[f_0, ..., f_{L-1}]: f_{l+1} = R f_l with the Problem's restriction (injection on the coarse boundary either way)"""
    f = [P.as_prec(b)]
    for l in range(P.L - 1):
        f.append(P.restrict_fw(f[-1], l) if P.restriction == RESTRICT_FULLW else P.inject(f[-1], l))
    return f


def fmg(P: Problem, b, cycles_per_level, coarse_sweeps, interp="cubic"):
    """the FMG iterate on level 0: coarse solve (coarse_sweeps sweeps from 0 inside / f on the Dirichlet nodes), then per
    level the interpolated solution (Dirichlet nodes from f_l) and cycles_per_level V-cycles started on that level.
    interp="linear" swaps Pi for the V-cycle's own (bi/tri)linear prolongation, for comparison only."""
    f = restrict_rhs(P, b)
    lc = P.L - 1
    u = np.zeros(P.shape(lc), P.prec)
    bm = boundary_mask(u.shape)
    u[bm] = f[lc][bm]
    u = P.coarse_solve(u, f[lc], lc, coarse_sweeps)
    for l in range(P.L - 2, -1, -1):
        if interp == "cubic":
            u = cubic_prolong(P, u, l, bnd=f[l])
        else:
            u = P.prolong(u, l).copy()
            bm = boundary_mask(u.shape)
            u[bm] = f[l][bm]
        for _ in range(cycles_per_level):
            u = P.vcycle(u, f[l], coarse_sweeps, l)
    return u


def manufactured(P: Problem, length=1.0, alpha=1.0):
    """(u_exact, b) on level 0 of an isotropic Problem: u = sin(a x + p) sin(b y + q) [sin(c z + r)], b = -alpha Laplace(u)
    inside and u on the Dirichlet nodes"""
    n = P.n[0]
    t = np.linspace(0, length, n).astype(P.prec)
    fx, fy, fz = np.sin(3.1 * t + 0.4), np.sin(2.3 * t + 1.1), np.sin(1.7 * t + 0.2)
    if P.dim == 2:
        u = fy[:, None] * fx[None, :]
        lam = 3.1 ** 2 + 2.3 ** 2
    else:
        u = fz[:, None, None] * fy[None, :, None] * fx[None, None, :]
        lam = 3.1 ** 2 + 2.3 ** 2 + 1.7 ** 2
    b = P.prec(alpha * lam) * u
    bm = boundary_mask(u.shape)
    b[bm] = u[bm]
    return u, b
