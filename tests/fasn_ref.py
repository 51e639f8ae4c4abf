"""fasn_ref -- numpy reference of the semilinear operator with NEUMANN faces: mg_fas_* with MG_FAS_ON_FACES and a non-zero
mg_bc_set_faces mask (TEST INFRASTRUCTURE, numpy only).

    N(u) = (sigma I + A) u + gamma g(u),   A = mg_bc_*'s operator: the faces of the mask are zero-flux walls (mirror images),
                                           a node on a face outside the mask is a Dirichlet node

FASNProblem stands on bc_ref.BCProblem (the mask, the mirrored row sum, the mirrored restriction, the Dirichlet nodes) and
takes fas_ref.FASProblem's reaction, transition, correction and FAS recursion; neither parent is edited.

 * In a working precision (prec = np.float32 / np.float64, the level coefficients taken from the handle with
   use_handle_coefs) every numpy call below is ONE rounded operation of the arithmetic contract of
   multigrid_prj_amd/csrc/mg_fas.hip with a mask, in its order, G = prec(gamma), u(q) the neighbour or its mirror image:
       residual     sum = bc_ref's row sum; r = b - (sum + G*g); Dirichlet nodes: r = b - u
       point solve  s = bc_ref's off-diagonal sum; num = (b - s) - G*(g - gp*u); den = cd + G*gp; ps = num / den; Dirichlet: b
       Jacobi       u' = ps (omega == 1) or u_i + omega * (ps - u_i);  red-black in place with colour (i + j + k) & 1
       transition   uc = u injected; rc = bc_ref's mirrored [q hlf q] weighting of r (or r injected);
                    rhs_c = rc + (sum_c(uc) + G*g(uc)) at the coarse unknowns, uc at the coarse Dirichlet nodes
       correction   e = uc_new - uc (rounded); u += P e
   With mask 0 every one of these is fas_ref's expression and with gamma 0 bc_ref's: the same bits (tests/test_fasn_cpu.py).
 * In np.longdouble / np.float64 it is the reference of cycles, of the coarse loop, of mg_fas_solve and of the steps.

apply_A IS THE NONLINEAR OPERATOR HERE: BCProblem.residual and tests/step_ref.py (which sees a BCProblem) call it, so the
residual, n0 of the time steps and their magnitudes come out of the one override.

restriction_mode="today" restricts the RESIDUAL as mg_fas_coarse_rhs does without a mask (every coarse boundary node
injected): kept to show why the residual must go down mirrored -- the cycle diverges with it.
"""
from __future__ import annotations

import math

import numpy as np

from tests import npref
from tests.bc_ref import XHI, XLO, YHI, BCProblem, all_faces
from tests.fas_ref import CUBIC, EXP, FASProblem
from tests.npref_cycles import CYCLE_V

LD = np.longdouble
ON_FACES = 256   # MG_FAS_ON_FACES


class FASNProblem(BCProblem, FASProblem):
    """keywords: mask, sigma, restriction_mode (BCProblem), kind, gamma (FASProblem), the rest npref_cycles.CycleProblem's"""

    def __init__(self, **kw):
        assert kw.get("iterate_mode", "inject") == "inject"
        super().__init__(**kw)   # BCProblem takes mask / sigma and sets cd last, FASProblem the reaction

    def singular(self):
        return False   # no projection is done (include/mg_hip.h)

    # -- the contract (react, correct, vcycle, norm: FASProblem's; _row_sum, dirichlet, restrict_fw, jacobi: BCProblem's)
    def apply_A(self, u, l, absolute=False):
        """N(u) at the unknowns, u at the Dirichlet nodes; absolute: |A||u| + |G||g|, what bounds its rounding"""
        u = self.as_prec(u)
        with np.errstate(over="ignore"):
            g, _ = self.react(u)
        dm = self.dirichlet(u.shape)
        if absolute:
            return np.where(dm, abs(u), self._row_sum(abs(u), l, True, absolute=True) + abs(self.G) * abs(g))
        return np.where(dm, u, self._row_sum(u, l, True) + self.G * g)

    def apply_N(self, u, l):
        return self.apply_A(u, l)

    def residual_mag(self, u, b, l):
        """|b| + |A||u| + |G||g| (Dirichlet nodes: |b| + |u|)"""
        u, b = self.as_prec(u), abs(self.as_prec(b))
        g, _ = self.react(u)
        return np.where(self.dirichlet(u.shape), b + abs(u), b + self._row_sum(abs(u), l, True, absolute=True) + abs(self.G) * abs(g))

    def _newton(self, u, b, l):
        """(num, den, g, gp) at every node (meaningful at the unknowns)"""
        g, gp = self.react(u)
        num = (b - self._row_sum(u, l, False)) - self.G * (g - gp * u)
        den = self.prec(self.cd[l]) + self.G * gp
        return num, den, g, gp

    def point_solve(self, u, b, l):
        u, b = self.as_prec(u), self.as_prec(b)
        num, den, _, _ = self._newton(u, b, l)
        return np.where(self.dirichlet(u.shape), b, num / den)

    def point_solve_mag(self, u, b, l):
        """(|b| + |A - D||u| + |G|(|g| + |gp u|)) / |den|: bounds the rounding of the point solve"""
        u, b = self.as_prec(u), self.as_prec(b)
        _, den, g, gp = self._newton(u, b, l)
        mag = (abs(b) + self._row_sum(abs(u), l, False, absolute=True) + abs(self.G) * (abs(g) + abs(gp * u))) / abs(den)
        return np.where(self.dirichlet(u.shape), abs(b), mag)

    def coarse_rhs(self, u, r, l):
        """mg_fas_coarse_rhs with a mask: (u, r on level l) -> (uc0, rhs_c) on level l + 1"""
        uc0 = self.inject(u, l)
        rc = self.restrict_fw(r, l) if self.restriction == npref.RESTRICT_FULLW else self.inject(r, l)
        return uc0, np.where(self.dirichlet(uc0.shape), uc0, rc + self.apply_A(uc0, l + 1))

    # -- mg_fas_solve
    def solve_history(self, u, b, maxit, coarse_sweeps, rtol=0.0, atol=0.0):
        """FASProblem.solve_history with the mask's Dirichlet nodes -> (u, hist of ABSOLUTE norms, status)"""
        u, b = self.as_prec(u).copy(), self.as_prec(b)
        dm = self.dirichlet(b.shape)
        u[dm] = b[dm]
        hist = [self.norm(u, b)]

        def verdict():
            if not math.isfinite(hist[-1]):
                return 2
            return 0 if hist[-1] <= max(atol, rtol * hist[0]) else -1
        v = verdict()
        while v < 0 and len(hist) - 1 < maxit:
            with np.errstate(all="ignore"):
                u = self.vcycle(u, b, coarse_sweeps)
            hist.append(self.norm(u, b))
            v = verdict()
        return u, np.array(hist), (1 if v < 0 else v)


# ---------------------------------------------------------------- the settings of the convergence table
TABLE_COARSE_SWEEPS = 50
ONLY_YHI_DIRICHLET = 63 & ~YHI

TABLE = {   # name -> (kind, gamma, s, mask, restriction_mode, the prototype's factor at cycle 10)
    "cubic-1e3-dirichlet": (CUBIC, 1e3, 1e3, 0, "mirror", 0.255),
    "cubic-1e3-xlo": (CUBIC, 1e3, 1e3, XLO, "mirror", 0.319),
    "cubic-1e3-only-yhi-dirichlet": (CUBIC, 1e3, 1e3, ONLY_YHI_DIRICHLET, "mirror", 0.566),
    "cubic-1e3-all": (CUBIC, 1e3, 1e3, 63, "mirror", 0.566),
    "cubic-1-xlo": (CUBIC, 1.0, 1.0, XLO, "mirror", 0.103),
    "cubic-1-xlo-today": (CUBIC, 1.0, 1.0, XLO, "today", 1.48),
    "exp-100-dirichlet": (EXP, 100.0, 1e4, 0, "mirror", 0.446),
    "exp-100-xlo": (EXP, 100.0, 1e4, XLO, "mirror", 0.445),
    "exp-100-only-yhi-dirichlet": (EXP, 100.0, 1e4, ONLY_YHI_DIRICHLET, "mirror", 0.196),
}
GPU_ROWS = ("cubic-1e3-xlo", "cubic-1e3-only-yhi-dirichlet", "cubic-1e3-all")   # the convergence rows the GPU test reuses


def problem(kind, gamma, mask, sigma=0.0, n=33, levels=4, prec=np.float64, restriction_mode="mirror", smoother=npref.SMOOTH_RBGS,
            omega=1.0, cycle=CYCLE_V, restriction=npref.RESTRICT_FULLW, dim=3, **kw):
    """V(2,2), unit cube, alpha = 1, the residual restricted with the (mirrored) full weighting"""
    return FASNProblem(kind=kind, gamma=gamma, mask=mask, sigma=sigma, restriction_mode=restriction_mode, dim=dim, n=n, levels=levels,
                       length=1.0, alpha=1.0, smoother=smoother, omega=omega, nu_pre=2, nu_post=2, restriction=restriction,
                       outer_pre_gs=0, prec=prec, cycle=cycle, **kw)


def table_problem(name, n=33, levels=4, prec=np.float64):
    kind, gamma, _, mask, mode, _ = TABLE[name]
    return problem(kind, gamma, mask, n=n, levels=levels, prec=prec, restriction_mode=mode)


def noise(P, shape, s, seed=1):
    """b = s * standard normal, the DIRICHLET nodes of P set to 0 (the nodes of a Neumann face keep their data)"""
    b = s * np.random.default_rng(seed).standard_normal(shape)
    b[P.dirichlet(shape)] = 0.0
    return b


def table_history(name, cycles=10, n=33, levels=4, prec=np.float64):
    """-> (P, b, hist) of `cycles` cycles from u = 0"""
    P = table_problem(name, n, levels, prec)
    b = noise(P, P.shape(0), TABLE[name][2])
    _, hist, _ = P.solve_history(np.zeros(P.shape(0), prec), b, cycles, TABLE_COARSE_SWEEPS)
    return P, b, hist


def factors(hist):
    h = np.asarray(hist, float)
    return h[1:] / h[:-1]


# ---------------------------------------------------------------- manufactured solutions (unit cube, alpha = 1)
def grid(n, dim=3):
    x = np.linspace(0.0, 1.0, n)
    return np.meshgrid(*([x] * dim), indexing="ij")[::-1]   # X (fast axis), Y(, Z)


MANUFACTURED = {   # name -> (kind, gamma, mask)
    "cubic-all": (CUBIC, 1e3, 63),
    "exp-all": (EXP, 20.0, 63),
    "cubic-x": (CUBIC, 1e3, XLO | XHI),
}


def manufactured(name, n):
    """all faces Neumann: u = cos(pi x) cos(2 pi y) cos(pi z), f = 6 pi^2 u + gamma g(u); x faces Neumann, the rest Dirichlet:
    u = cos(pi x) sin(pi y) sin(pi z), f = 3 pi^2 u + gamma g(u), f = u on the Dirichlet nodes -> (kind, gamma, mask, f, u)"""
    kind, gamma, mask = MANUFACTURED[name]
    X, Y, Z = grid(n)
    pi = np.pi
    if mask == 63:
        u, lam = np.cos(pi * X) * np.cos(2 * pi * Y) * np.cos(pi * Z), 6 * pi ** 2
    else:
        u, lam = np.cos(pi * X) * np.sin(pi * Y) * np.sin(pi * Z), 3 * pi ** 2
    g = u ** 3 if kind == CUBIC else np.exp(u)
    f = lam * u + gamma * g
    if mask != 63:
        P = problem(kind, gamma, mask, n=n, levels=2)
        dm = P.dirichlet(u.shape)
        u[dm] = 0.0
        f[dm] = 0.0
    return kind, gamma, mask, f, u


# ---------------------------------------------------------------- one theta step on an insulated box (all faces Neumann, cubic)
def step_case(n=17):
    """u0 and the source f of the step tests (all faces Neumann, cubic, gamma 1e3, dt 1e-3)"""
    X, Y, Z = grid(n)
    u0 = 0.2 + 0.5 * np.cos(np.pi * X) * np.cos(2 * np.pi * Y) * np.cos(np.pi * Z)
    f = 10.0 * np.random.default_rng(6).standard_normal(u0.shape)
    return u0, f


def step_identity(P0, u0, u1, f, dt, theta, resnorm):
    """-> (lhs - rhs, bound) of sum w (u1 - u0)/dt = sum w f - gamma (theta sum w g(u1) + (1 - theta) sum w g(u0)): with every face
    Neumann w A is symmetric with zero row sums, so sum w A u = 0 and theta * sum w r is all the solve leaves behind"""
    w = P0.weights(u0.shape)
    fs = lambda a: math.fsum(np.asarray(a, np.float64).ravel().tolist())
    g0, g1 = u0 ** 3, u1 ** 3
    terms = [fs(w * (u1 - u0)) / dt, -fs(w * f), P0.gamma * theta * fs(w * g1), P0.gamma * (1 - theta) * fs(w * g0)]
    mags = [fs(w * abs(u1 - u0)) / dt, fs(w * abs(f)), abs(P0.gamma) * theta * fs(w * abs(g1)), abs(P0.gamma) * (1 - theta) * fs(w * abs(g0))]
    bound = float(np.sqrt(fs(w * w))) * resnorm + 64 * np.finfo(np.float64).eps * sum(mags)
    return sum(terms), bound, sum(mags)


def levels_for(n):
    """down to a 3-point grid"""
    return int(round(math.log2(n - 1)))


def mixed_mask(dim):
    """tests/test_bc_gpu.py's mixed mask, Neumann faces that meet Dirichlet ones along edges: x-hi, y-hi, z-lo (2-D: x-hi, y-hi)"""
    return 0b011010 if dim == 3 else 0b1010
