"""step_ref -- numpy reference of the implicit time steps on the operator families (TEST INFRASTRUCTURE; numpy, and scipy's
sparse LU for the direct solves of the small CPU tests; mg_vc_heat_*, mg_bc_heat_*, mg_fas_heat_*, include/mg_hip.h).

    u_t = -N0(u) + f,     (1/(theta dt)) u' + N0(u') = (f + u/dt - (1 - theta) N0(u)) / theta

N0 is the family's operator on level 0 WITHOUT the shift: a tests/vc_ref.VCProblem, tests/bc_ref.BCProblem or
tests/fas_ref.FASProblem built with sigma = 0 (and, for a handle, with the level coefficients read BEFORE any shift is set).

 * In a working precision every numpy call of step_rhs is ONE rounded operation of the kernels' contract:
       rdt = (T)(1/dt), omt = (T)(1 - theta), rth = (T)(1/theta)
       rhs = ((f + rdt*u) - omt*n0) * rth   at the unknowns (without a source: (rdt*u - omt*n0) * rth);  rhs = u at Dirichlet nodes
   with n0 the family's residual expression with the shift taken out (n0 below).
 * FamilyStepper is the theta scheme in any precision (long double for the tests), its solves done by a callback; the direct
   solver below serves the small CPU tests.
"""
from __future__ import annotations

import copy

import numpy as np

from tests.bc_ref import BCProblem
from tests.fas_ref import FASProblem
from tests.npref import boundary_mask
from tests.vc_ref import VCProblem


def family_of(P):
    return "vc" if isinstance(P, VCProblem) else "bc" if isinstance(P, BCProblem) else "fas" if isinstance(P, FASProblem) else None


def fixed_nodes(P, shape):
    """True at the Dirichlet nodes: bc's are the nodes on a face that is not in the mask, vc's and fas's the box boundary"""
    return P.dirichlet(shape) if family_of(P) == "bc" else boundary_mask(shape)


def n0(P, u):
    """the operator's value at every node (u itself at the Dirichlet nodes), in P.prec and in the kernels' order:
    vc d*u_i - s with d started from 0, bc the row sum with the diagonal of P, fas that sum + G*g"""
    return P.apply_N(u, 0) if family_of(P) == "fas" else P.apply_A(u, 0)


def scalars(T, dt, theta):
    return T(1.0 / dt), T(1.0 - theta), T(1.0 / theta)


def step_rhs(P, u, f, dt, theta):
    """the contract of mg_X_heat_rhs in P.prec; P carries the UNSHIFTED operator; f may be None"""
    T = P.prec
    u = P.as_prec(u)
    rdt, omt, rth = scalars(T, dt, theta)
    t = rdt * u
    if f is not None:
        t = P.as_prec(f) + t
    t = t - omt * n0(P, u)
    t = t * rth
    return np.where(fixed_nodes(P, u.shape), u, t)


def step_rhs_mag(P, u, f, dt, theta):
    """|f| + |rdt u| + |omt| (the magnitudes of n0's terms), times |rth|: what bounds the rounding of step_rhs"""
    T = P.prec
    u = P.as_prec(u)
    rdt, omt, rth = scalars(T, dt, theta)
    if family_of(P) == "fas":
        mag = P.residual_mag(u, np.zeros_like(u), 0)
    else:
        mag = P.apply_A(u, 0, absolute=True)
    t = abs(rdt * u) + abs(omt) * mag
    if f is not None:
        t = t + abs(P.as_prec(f))
    return t * abs(rth)


class FamilyStepper:
    """the theta scheme on P0 (sigma = 0) and Ps (the same problem with sigma = 1/(theta dt), the fp64 value the library
    uses); solve(Ps, u, rhs) -> u' returns the (approximate) solution of (sigma I + N0)(u') = rhs started from u"""

    def __init__(self, P0, Ps, dt, theta, solve):
        self.P0, self.Ps, self.solve = P0, Ps, solve
        self.dt, self.theta = P0.prec(dt), P0.prec(theta)

    def rhs(self, u, f):
        u = self.P0.as_prec(u)
        t = u / self.dt - (1 - self.theta) * n0(self.P0, u)
        if f is not None:
            t = t + self.P0.as_prec(f)
        return np.where(fixed_nodes(self.P0, u.shape), u, t / self.theta)

    def step(self, u, f=None):
        b = self.rhs(u, f)
        return self.solve(self.Ps, self.P0.as_prec(u), b), b


def shift_of(dt, theta):
    return 1.0 / (float(theta) * float(dt))


def cycle_solver(cycles, coarse_sweeps):
    """`cycles` cycles of the family (what mg_X_heat_step runs per step)"""
    def solve(Ps, u, b):
        for _ in range(cycles):
            u = Ps.vcycle(u, b, coarse_sweeps)
        return u
    return solve


def converged_solver(coarse_sweeps, rtol, maxcycles=60):
    """cycles until ||b - (sigma I + N0)(u)|| <= rtol ||b||"""
    def solve(Ps, u, b):
        nb = float(np.sqrt(np.sum(b * b)))
        for _ in range(maxcycles):
            r = b - n0(Ps, u)
            if float(np.sqrt(np.sum(r * r))) <= rtol * nb:
                return u
            u = Ps.vcycle(u, b, coarse_sweeps)
        raise AssertionError("the reference solve did not converge")
    return solve


# ---------------------------------------------------------------- direct solves (small grids: scipy's sparse LU in float64 + refinement)
def linear_matrix(P, shape):
    """the dense float64 matrix of u -> n0(P, u) over ALL nodes (identity rows at the Dirichlet nodes); P must be linear"""
    m = int(np.prod(shape))
    A = np.empty((m, m), np.float64)
    e = np.zeros(shape, P.prec)
    for j in range(m):
        e.flat[j] = 1
        A[:, j] = np.asarray(n0(P, e), np.float64).ravel()
        e.flat[j] = 0
    return A


def dense_solver(newton=12):
    """solves (sigma I + N0)(u') = b at the unknowns, u' = b at the Dirichlet nodes, by Newton steps with a float64 LU of the
    Jacobian (the first step solves a linear family; the rest is iterative refinement in P.prec)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    cache = {}

    def solve(Ps, u, b):
        shape = b.shape
        fx = fixed_nodes(Ps, shape).ravel()
        fas = family_of(Ps) == "fas" and Ps.gamma != 0
        if id(Ps) not in cache:
            lin = Ps
            if family_of(Ps) == "fas":
                lin = copy.copy(Ps)   # the linear part: the same problem without the reaction
                lin.gamma, lin.G = 0.0, Ps.prec(0)
            A = sp.csc_matrix(linear_matrix(lin, shape))
            cache[id(Ps)] = (A, None if fas else spl.splu(A))
        A, lu = cache[id(Ps)]
        x = np.where(fx.reshape(shape), b, u).astype(Ps.prec)
        for _ in range(newton):
            r = np.asarray(b - n0(Ps, x), np.float64).ravel()
            if fas:
                _, gp = Ps.react(x)
                d = np.where(fx, 0.0, float(Ps.gamma) * np.asarray(gp, np.float64).ravel())
                lu = spl.splu((A + sp.diags(d)).tocsc())
            x = x + Ps.as_prec(lu.solve(r).reshape(shape))
        return x
    return solve
