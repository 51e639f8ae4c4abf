"""fasvc_ref -- numpy reference of the semilinear operator on the VARIABLE-COEFFICIENT operator: mg_fas_* with
MG_FAS_ON_COEFFICIENT, the handle's mg_vc_set_coefficient hierarchy and its mg_vc_set_faces mask (TEST INFRASTRUCTURE, numpy
only).

    N(u) = sigma u - div(a grad u) + gamma g(u),   the linear part vcn_ref's: s, d of mg_vc.hip with mirrored neighbours (for a
                                                   and u alike) on the faces of the mask, Dirichlet nodes on a face outside it

FASVCProblem stands on vcn_ref.VCNProblem (the coefficient hierarchy, parts, the mask, the mirrored restriction, the step) and
takes fas_ref.FASProblem's reaction, correction and FAS recursion; neither parent is edited.

 * In a working precision (prec = np.float32 / np.float64, the level coefficients taken from the handle with
   use_handle_coefs, the coefficient hierarchy with set_a) every numpy call below is ONE rounded operation of the contract
   of include/mg_hip.h, in its order, G = prec(gamma):
       residual     r = b - ((d*u_i - s) + G*g); Dirichlet nodes: r = b - u
       point solve  num = (b + s) - G*(g - gp*u_i); den = d + G*gp; ps = num / den; Dirichlet nodes: b
       Jacobi       u' = ps (omega == 1) or u_i + omega * (ps - u_i);  red-black in place with colour (i + j + k) & 1
       transition   uc = u injected; rc = the mirrored [q hlf q] weighting of r with the mask (the plain one for mask 0, or r
                    injected); rhs_c = rc + ((d_c*uc - s_c) + G*g(uc)) at the coarse unknowns, uc at the coarse Dirichlet nodes
       correction   e = uc_new - uc (rounded); u += P e
       step         n0 = (d0*u_i - s) + G*g with d0 started from 0; vcn_ref's step_rhs on it
   With gamma 0 every one of these is vcn_ref's expression: the same bits (tests/test_fasvc_cpu.py).
 * In np.longdouble / np.float64 it is the reference of cycles, of the coarse loop, of mg_fas_solve and of the steps.

apply_A IS THE NONLINEAR OPERATOR HERE: the inherited residual, step_rhs and coarse loop call it.
"""
from __future__ import annotations

import math

import numpy as np

from tests import npref
from tests import vc_ref as vr
from tests.fas_ref import CUBIC, EXP, FASProblem
from tests.fasn_ref import FASNProblem, factors, grid, levels_for   # noqa: F401  (re-exported)
from tests.npref_cycles import CYCLE_V
from tests.step_ref import scalars
from tests.vcn_ref import MIXED, XLO, YHI, VCNProblem, all_faces   # noqa: F401

LD = np.longdouble
ON_COEFFICIENT = 1024   # MG_FAS_ON_COEFFICIENT


class FASVCProblem(VCNProblem):
    """keywords: kind, gamma (the reaction), mask, sigma, restriction_mode (VCNProblem), the rest npref_cycles.CycleProblem's"""

    def __init__(self, kind=CUBIC, gamma=0.0, **kw):
        super().__init__(**kw)
        assert kind in (CUBIC, EXP)
        self.react_kind, self.gamma = kind, gamma
        self.G = self.prec(gamma)

    def singular(self):
        return False   # no projection is done (include/mg_hip.h)

    # -- FASProblem's reaction, correction, recursion and norm; FASNProblem's solve loop (the mask's Dirichlet nodes)
    react = FASProblem.react
    correct = FASProblem.correct
    vcycle = FASProblem.vcycle
    norm = FASProblem.norm
    solve_history = FASNProblem.solve_history

    # -- the contract
    def apply_A(self, u, l, absolute=False, sigma=None):
        """N(u) at the unknowns, u at the Dirichlet nodes; absolute: |d||u| + |s| + |G||g| with |u| in s, what bounds its rounding"""
        u = self.as_prec(u)
        with np.errstate(over="ignore"):
            g, _ = self.react(u)
        dm = self.dirichlet(u.shape)
        if absolute:
            au = abs(u)
            s, d = self.parts(au, l, sigma)
            return np.where(dm, au, (d * au + s) + abs(self.G) * abs(g))
        s, d = self.parts(u, l, sigma)
        return np.where(dm, u, (d * u - s) + self.G * g)

    def apply_N(self, u, l):
        return self.apply_A(u, l)

    def residual_mag(self, u, b, l):
        """|b| + |d||u| + |s|(|u|) + |G||g| (Dirichlet nodes: |b| + |u|)"""
        return abs(self.as_prec(b)) + self.apply_A(u, l, absolute=True)

    def _newton(self, u, b, l):
        """(num, den, s, g, gp) at every node (meaningful at the unknowns)"""
        s, d = self.parts(u, l)
        g, gp = self.react(u)
        num = (b + s) - self.G * (g - gp * u)
        den = d + self.G * gp
        return num, den, s, g, gp

    def point_solve(self, u, b, l):
        u, b = self.as_prec(u), self.as_prec(b)
        num, den, _, _, _ = self._newton(u, b, l)
        return np.where(self.dirichlet(u.shape), b, num / den)

    def point_solve_mag(self, u, b, l):
        """(|b| + s(|u|) + |G|(|g| + |gp u|)) / |den|: bounds the rounding of the point solve"""
        u, b = self.as_prec(u), self.as_prec(b)
        _, den, _, g, gp = self._newton(u, b, l)
        s_abs, _ = self.parts(abs(u), l)
        mag = (abs(b) + s_abs + abs(self.G) * (abs(g) + abs(gp * u))) / abs(den)
        return np.where(self.dirichlet(u.shape), abs(b), mag)

    # jacobi, rbgs, smooth, residual, restrict_fw (by the mask), set_a, step_rhs, coarse_loop: inherited

    def coarse_rhs(self, u, r, l):
        """mg_fas_coarse_rhs with the flag: (u, r on level l) -> (uc0, rhs_c) on level l + 1"""
        uc0 = self.inject(u, l)
        # restrict_fw: bc_ref's mirrored weighting by the mask; with mask 0 its interior expression is restrict_fw_point's
        rc = self.restrict_fw(r, l) if self.restriction == npref.RESTRICT_FULLW else self.inject(r, l)
        return uc0, np.where(self.dirichlet(uc0.shape), uc0, rc + self.apply_A(uc0, l + 1))

    def step_rhs_mag(self, u, f, dt, theta):
        """|f| + |rdt u| + |omt| (the magnitudes of n0's terms), times |rth|: what bounds the rounding of step_rhs"""
        u = self.as_prec(u)
        rdt, omt, rth = scalars(self.prec, dt, theta)
        t = abs(rdt * u) + abs(omt) * self.apply_A(u, 0, absolute=True, sigma=0.0)
        if f is not None:
            t = t + abs(self.as_prec(f))
        return t * abs(rth)


# ---------------------------------------------------------------- the settings of the convergence table
TABLE_COARSE_SWEEPS = 50
ONLY_YHI_DIRICHLET = 63 & ~YHI

TABLE = {   # name -> (kind, gamma, s, mask, the factor of cycle 10 over cycle 9 measured with this file in float64)
    "cubic-1e3-dirichlet": (CUBIC, 1e3, 1e3, 0, 0.204),
    "cubic-1e3-xlo": (CUBIC, 1e3, 1e3, XLO, 0.258),
    "cubic-1e3-only-yhi-dirichlet": (CUBIC, 1e3, 1e3, ONLY_YHI_DIRICHLET, 0.378),
    "cubic-1e3-all": (CUBIC, 1e3, 1e3, 63, 0.377),
    "cubic-1-dirichlet": (CUBIC, 1.0, 1.0, 0, 0.158),
    "cubic-1-xlo": (CUBIC, 1.0, 1.0, XLO, 0.163),
    "cubic-1-only-yhi-dirichlet": (CUBIC, 1.0, 1.0, ONLY_YHI_DIRICHLET, 0.362),
    "exp-100-dirichlet": (EXP, 100.0, 1e3, 0, 0.119),
    "exp-100-xlo": (EXP, 100.0, 1e3, XLO, 0.127),
    "exp-100-only-yhi-dirichlet": (EXP, 100.0, 1e3, ONLY_YHI_DIRICHLET, 0.297),
}
# the rows the GPU test reuses: the three cubic 1e3 rows with a non-zero mask and the exp x-lo row
GPU_ROWS = ("cubic-1e3-xlo", "cubic-1e3-only-yhi-dirichlet", "cubic-1e3-all", "exp-100-xlo")


def problem(kind, gamma, mask, a0=None, sigma=0.0, n=33, levels=4, prec=np.float64, smoother=npref.SMOOTH_RBGS, omega=1.0, cycle=CYCLE_V,
            restriction=npref.RESTRICT_FULLW, dim=3, **kw):
    """V(2,2), unit cube, alpha = 1, full weighting by the mask; a0: the level-0 coefficient (default vc_ref.field_smooth)"""
    P = FASVCProblem(kind=kind, gamma=gamma, mask=mask, sigma=sigma, dim=dim, n=n, levels=levels, length=1.0, alpha=1.0, smoother=smoother,
                     omega=omega, nu_pre=2, nu_post=2, restriction=restriction, outer_pre_gs=0, prec=prec, cycle=cycle, **kw)
    P.set_a(vr.field_smooth(n) if a0 is None else a0)
    return P


def table_problem(name, n=33, levels=4, prec=np.float64):
    kind, gamma, _, mask, _ = TABLE[name]
    return problem(kind, gamma, mask, n=n, levels=levels, prec=prec)


def noise(P, shape, s, seed=1):
    """b = s * standard normal, the DIRICHLET nodes of P set to 0"""
    b = s * np.random.default_rng(seed).standard_normal(shape)
    b[P.dirichlet(shape)] = 0.0
    return b


def table_history(name, cycles=10, n=33, levels=4, prec=np.float64):
    """-> (P, b, hist) of `cycles` cycles from u = 0"""
    P = table_problem(name, n, levels, prec)
    b = noise(P, P.shape(0), TABLE[name][2])
    _, hist, _ = P.solve_history(np.zeros(P.shape(0), prec), b, cycles, TABLE_COARSE_SWEEPS)
    return P, b, hist


# ---------------------------------------------------------------- manufactured solutions (unit cube, alpha = 1, a = vc_ref.field_smooth)
MANUFACTURED = {   # name -> (kind, gamma, mask, (max error at n = 9, 17, 33), (cycles to rtol 1e-12 at 17, 33)) measured with this file
    "neumann-cubic": (CUBIC, 1e3, 63, (4.12e-2, 9.73e-3, 2.42e-3), (32, 31)),
    "neumann-exp": (EXP, 20.0, 63, (1.03e-1, 2.81e-2, 7.18e-3), (14, 15)),
    "dirichlet-cubic": (CUBIC, 1e3, 0, (1.52e-2, 3.94e-3, 9.94e-4), (10, 11)),
    "dirichlet-exp": (EXP, 20.0, 0, (2.31e-2, 5.82e-3, 1.47e-3), (13, 14)),
}
MANUFACTURED_MAXIT = 40


def manufactured(name, n):
    """a = exp(ln10 p), p = sin(2 pi x) cos(2 pi y) cos(pi z); f = -(a lap u + grad a . grad u) + gamma g(u) with the analytic
    derivatives. All faces Neumann: u = cos(pi x) cos(2 pi y) cos(pi z); all Dirichlet: u = sin(pi x) sin(pi y) sin(pi z) and
    f = u = 0 on the boundary -> (kind, gamma, mask, a, f, u)"""
    kind, gamma, mask = MANUFACTURED[name][:3]
    X, Y, Z = grid(n)
    pi, ln10 = np.pi, math.log(10.0)
    sx, cx, cy, sy, cz, sz = np.sin(2 * pi * X), np.cos(2 * pi * X), np.cos(2 * pi * Y), np.sin(2 * pi * Y), np.cos(pi * Z), np.sin(pi * Z)
    a = np.exp(ln10 * sx * cy * cz)
    ax, ay, az = a * ln10 * 2 * pi * cx * cy * cz, -a * ln10 * 2 * pi * sx * sy * cz, -a * ln10 * pi * sx * cy * sz
    if mask == 63:
        u = np.cos(pi * X) * np.cos(2 * pi * Y) * np.cos(pi * Z)
        ux = -pi * np.sin(pi * X) * np.cos(2 * pi * Y) * np.cos(pi * Z)
        uy = -2 * pi * np.cos(pi * X) * np.sin(2 * pi * Y) * np.cos(pi * Z)
        uz = -pi * np.cos(pi * X) * np.cos(2 * pi * Y) * np.sin(pi * Z)
        lap = -6 * pi ** 2 * u
    else:
        u = np.sin(pi * X) * np.sin(pi * Y) * np.sin(pi * Z)
        ux = pi * np.cos(pi * X) * np.sin(pi * Y) * np.sin(pi * Z)
        uy = pi * np.sin(pi * X) * np.cos(pi * Y) * np.sin(pi * Z)
        uz = pi * np.sin(pi * X) * np.sin(pi * Y) * np.cos(pi * Z)
        lap = -3 * pi ** 2 * u
    g = u ** 3 if kind == CUBIC else np.exp(u)
    f = -(a * lap + ax * ux + ay * uy + az * uz) + gamma * g
    if mask != 63:
        bm = npref.boundary_mask(u.shape)
        u[bm] = 0.0
        f[bm] = 0.0
    return kind, gamma, mask, a, f, u


def manufactured_levels(n):
    """down to a 5-point grid (33: the 4 levels of the convergence table): with all faces Neumann a 3-point coarsest grid slows
    the cycle down to 0.8 per cycle"""
    return levels_for(n) - 1


def manufactured_solve(name, n):
    """-> (max error, cycles) of the float64 reference solved to rtol 1e-12"""
    kind, gamma, mask, a, f, u = manufactured(name, n)
    P = problem(kind, gamma, mask, a0=a, n=n, levels=manufactured_levels(n))
    x, hist, status = P.solve_history(np.zeros_like(f), f, MANUFACTURED_MAXIT, TABLE_COARSE_SWEEPS, rtol=1e-12)
    assert status == 0
    return float(abs(x - u).max()), len(hist) - 1


# ---------------------------------------------------------------- one theta step on an insulated box (all faces Neumann, cubic)
def step_case(n=17):
    """u0 and the source f of the step tests (all faces Neumann, cubic, gamma 1e3, dt 1e-3)"""
    X, Y, Z = grid(n)
    u0 = 0.2 + 0.5 * np.cos(np.pi * X) * np.cos(2 * np.pi * Y) * np.cos(np.pi * Z)
    f = 10.0 * np.random.default_rng(6).standard_normal(u0.shape)
    return u0, f


def step_identity(P0, u0, u1, f, dt, theta, resnorm):
    """-> (lhs - rhs, bound, magnitude) of sum w (u1 - u0)/dt = sum w f - gamma (theta sum w g(u1) + (1 - theta) sum w g(u0)): with
    every face Neumann diag(w) L is symmetric with zero row sums for mg_vc's operator too, so sum w L u = 0
    and theta * sum w r is all the solve leaves behind"""
    w = P0.node_weights(u0.shape)
    fs = lambda a: math.fsum(np.asarray(a, np.float64).ravel().tolist())
    g0, g1 = u0 ** 3, u1 ** 3
    terms = [fs(w * (u1 - u0)) / dt, -fs(w * f), P0.gamma * theta * fs(w * g1), P0.gamma * (1 - theta) * fs(w * g0)]
    mags = [fs(w * abs(u1 - u0)) / dt, fs(w * abs(f)), abs(P0.gamma) * theta * fs(w * abs(g1)), abs(P0.gamma) * (1 - theta) * fs(w * abs(g0))]
    bound = float(np.sqrt(fs(w * w))) * resnorm + 64 * np.finfo(np.float64).eps * sum(mags)
    return sum(terms), bound, sum(mags)


def mixed_mask(dim):
    """tests/test_vcn_gpu.py's mixed mask, Neumann faces that meet Dirichlet ones along edges: x-hi, y-hi, z-lo (2-D: x-hi, y-hi)"""
    return MIXED if dim == 3 else 0b1010
