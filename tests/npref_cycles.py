"""npref_cycles -- the W- and F-cycle on top of the independent reference (TEST INFRASTRUCTURE, numpy only).

include/mg_hip.h defines one cycle of kind V, W or F started on level l, with L the number of levels:

    cyc(l, kind):
      if l == L-1:  coarse solve of A U = RHS;  return
      nu_pre sweeps;  RHS(l+1) = R (RHS(l) - A U(l));  U(l+1) = 0
      cyc(l+1, kind)
      if l+1 < L-1:                      the coarsest grid is solved once per visit of its parent
          kind == W: cyc(l+1, W)         the second visit continues from U(l+1), RHS(l+1) unchanged
          kind == F: cyc(l+1, V)
      U(l) += P U(l+1);  nu_post sweeps

CycleProblem.vcycle is that recursion, written with the operators of npref.Problem; Problem.cycle, Problem.solve and
npref_fmg.fmg call vcycle and so work unchanged. visits[l] counts the calls per level since the last reset_visits().
"""
from __future__ import annotations

import numpy as np

from tests import npref

CYCLE_V, CYCLE_W, CYCLE_F = 1, 2, 3


def expected_visits(kind, levels, start=0):
    """visits per level of one cyc(start, kind): 1 on the start level; V: 1 everywhere; W: twice the parent's; F: the
    parent's visits plus one per F-visit of the parent -- and the coarsest level once per visit of its parent"""
    v = [0] * levels

    def rec(l, k):
        v[l] += 1
        if l == levels - 1:
            return
        rec(l + 1, k)
        if l + 1 < levels - 1 and k != CYCLE_V:
            rec(l + 1, CYCLE_W if k == CYCLE_W else CYCLE_V)
    rec(start, kind)
    return v


def closed_form_visits(kind, levels):
    """the same without recursion: level l < L-1 is visited 1 (V), l + 1 (F), 2^l (W) times; the coarsest as often as its parent"""
    per = {CYCLE_V: lambda l: 1, CYCLE_F: lambda l: l + 1, CYCLE_W: lambda l: 2 ** l}[kind]
    v = [per(l) for l in range(levels - 1)]
    return v + [v[-1] if v else 1]


class CycleProblem(npref.Problem):
    def __init__(self, cycle=CYCLE_V, **kw):
        assert cycle in (CYCLE_V, CYCLE_W, CYCLE_F)
        super().__init__(cycle=npref.CYCLE_V, **kw)
        self.kind = cycle
        self.tol = None            # a number: the coarsest solve iterates to this tolerance (see coarse_solve_tol)
        self.tol_sweeps, self.tol_margin = [], float("inf")
        self.reset_visits()

    def reset_visits(self):
        self.visits = [0] * self.L

    def vcycle(self, u, b, coarse_sweeps, l=0, kind=None):
        kind = self.kind if kind is None else kind
        self.visits[l] += 1
        if l == self.L - 1:
            if self.tol is not None:   # coarse_sweeps is then the sweep limit
                u, sweeps, margin = self.coarse_solve_tol(u, b, l, self.tol, coarse_sweeps)
                self.tol_sweeps.append(sweeps)
                self.tol_margin = min(self.tol_margin, margin)
                return u
            return self.coarse_solve(u, b, l, coarse_sweeps)
        u = self.smooth(self.smoother, self.nu_pre, u, b, l)
        r = self.residual(u, b, l)
        rc = self.restrict_fw(r, l) if self.restriction == npref.RESTRICT_FULLW else self.inject(r, l)
        ec = self.vcycle(np.zeros(self.shape(l + 1), self.prec), rc, coarse_sweeps, l + 1, kind)
        if l + 1 < self.L - 1:
            if kind == CYCLE_W:
                ec = self.vcycle(ec, rc, coarse_sweeps, l + 1, CYCLE_W)
            elif kind == CYCLE_F:
                ec = self.vcycle(ec, rc, coarse_sweeps, l + 1, CYCLE_V)
        u = u + self.prolong(ec, l)
        return self.smooth(self.smoother, self.nu_post, u, b, l)

    # -- the iterate-to-tolerance coarse solve (MG_COARSE_TOL), for choosing inputs whose stopping decisions are robust
    def coarse_solve_tol(self, u, rhs, l, tol, maxit):
        """Solver::Solve: sweep while sqrt(sum r^2 / sum rhs^2) > tol, at most maxit sweeps -> (u, sweeps, margin); margin
        is the smallest |relres / tol - 1| over the tests taken: how far every stopping decision was from flipping"""
        nb2 = npref.fsum_sq(rhs)
        u = self.as_prec(u)
        sweeps, margin = 0, float("inf")
        while True:
            rel = (npref.fsum_sq(self.residual(u, rhs, l)) / nb2) ** 0.5
            margin = min(margin, abs(rel / tol - 1.0))
            if not rel > tol or sweeps == maxit:
                return u, sweeps, margin
            u = self.smooth(self.coarse_smoother(), 1, u, rhs, l)
            sweeps += 1

    def level_visits(self, kind=None):
        """total level visits of one cycle from level 0 (what a rounding bound per cycle scales with)"""
        return sum(expected_visits(self.kind if kind is None else kind, self.L))
