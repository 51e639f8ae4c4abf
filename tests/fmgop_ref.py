"""fmgop_ref -- numpy reference of nested iteration on the operator families: mg_fmg / mg_fmg_prolong with
MG_FMG_OPERATOR(op) (TEST INFRASTRUCTURE, numpy only; include/mg_hip.h).

The interpolation. Pi_mask is the tensor product, over the axes a transition coarsens, of the 1-D rule of tests/npref_fmg.py
on a coarse row c[0..nc-1] that is EXTENDED BY ITS MIRROR IMAGE at an end whose face is in the mask (mg_face bits,
bc_ref.XLO ...): c[-1] = c[1], c[nc] = c[nc-2]. The odd fine node next to such an end then takes the cubic rule; the
one-sided quadratic rule stays at an end whose face is Dirichlet. Every call below is ONE rounded operation of
mg_fmg.hip's rule(), ((wb b + wc c) - (a + d)) * 2^-k with an operand a one-sided rule does not use replaced by 0, applied
along x first, then y, then z -- in a working precision (np.float32 / np.float64) the kernels are compared with it bit for
bit. Fine nodes on at least one face that is not in the mask (bc_ref's Dirichlet nodes) take bnd.

The pass. fmg_pass composes the family references of tests/ (bc_ref, vcn_ref, fas_ref, fasn_ref, fasvc_ref): their
restriction carries the right-hand side down, their coarse solve, cycle and projection do the rest. For the nonlinear
families the restricted f IS the coarse right-hand side: these are the coarse problems, not coarse corrections.
"""
from __future__ import annotations

import math

import numpy as np

from tests import bc_ref as br
from tests import fas_ref as fr
from tests import fasn_ref as fnr
from tests import fasvc_ref as fvr
from tests import npref
from tests import vcn_ref as vnr
from tests.bc_ref import face_bit
from tests.npref_cycles import CYCLE_V

ON_CONSTANT, ON_FACES, ON_COEFFICIENT, ON_REACTION = 0, 1, 2, 3
RULE_CUBIC, RULE_LEFT, RULE_RIGHT = 0, 1, 2


def operator_flag(op):
    """MG_FMG_OPERATOR(op)"""
    return op << 16


def dirichlet_nodes(shape, mask):
    """True on the nodes that lie on at least one face that is not in the mask (bc_ref.BCProblem.dirichlet)"""
    nd = len(shape)
    m = np.zeros(shape, bool)
    for ax in range(nd):
        for side in (0, 1):
            if not mask & face_bit(nd, ax, side):
                sl = [slice(None)] * nd
                sl[ax] = 0 if side == 0 else -1
                m[tuple(sl)] = True
    return m


def rule_last_axis(c, lo, hi):
    """the 1-D rule along the last axis; lo / hi: that end's face is in the mask (the row is mirrored there)"""
    nc = c.shape[-1]
    assert nc >= 3
    T = c.dtype.type
    m = np.arange(nc - 1)
    ia, idd = m - 1, m + 2
    ia[0] = 1 if lo else 0              # the mirror image c[-1] = c[1] (Dirichlet: any node, the one-sided rule ignores it)
    idd[-1] = nc - 2 if hi else nc - 1  # c[nc] = c[nc-2]
    kind = np.full(nc - 1, RULE_CUBIC)
    kind[-1] = RULE_CUBIC if hi else RULE_RIGHT
    kind[0] = RULE_CUBIC if lo else RULE_LEFT   # m == 0 decides first, as rule_kind() does (nc = 3)
    wb = np.where(kind == RULE_LEFT, 3, np.where(kind == RULE_RIGHT, 6, 9)).astype(T)
    wc = np.where(kind == RULE_LEFT, 6, np.where(kind == RULE_RIGHT, 3, 9)).astype(T)
    sc = np.where(kind == RULE_CUBIC, 0.0625, 0.125).astype(T)
    zero = T(0)
    a = np.where(kind == RULE_LEFT, zero, c[..., ia])
    d = np.where(kind == RULE_RIGHT, zero, c[..., idd])
    f = np.empty(c.shape[:-1] + (2 * nc - 1,), c.dtype)
    f[..., ::2] = c
    f[..., 1::2] = ((wb * c[..., :-1] + wc * c[..., 1:]) - (a + d)) * sc
    return f


def prolong(P, coarse, l, mask, bnd=None):
    """Pi_mask coarse on level l of the Problem (coarse lives on level l + 1), in P.prec; bnd: an array of level l whose
    values the Dirichlet nodes of the mask take (None: they are interpolated like every other node)"""
    c = P.as_prec(coarse)
    nd = c.ndim
    for a in reversed(P._coarsened_axes(l)):   # x (the last array axis) first, then y, then z
        lo, hi = bool(mask & face_bit(nd, a, 0)), bool(mask & face_bit(nd, a, 1))
        c = np.moveaxis(rule_last_axis(np.ascontiguousarray(np.moveaxis(c, a, -1)), lo, hi), -1, a)
    c = np.ascontiguousarray(c)
    assert c.shape == P.shape(l)
    if bnd is not None:
        dm = dirichlet_nodes(c.shape, mask)
        c[dm] = P.as_prec(bnd)[dm]
    return c


def mask_of(P):
    return getattr(P, "mask", 0)


def is_singular(P):
    return bool(getattr(P, "singular", lambda: False)())


def restrict_rhs(P, b):
    """[f_0, ..., f_{L-1}]: f_{l+1} = R f_l with the family's restriction (Dirichlet data travels by injection)"""
    f = [P.as_prec(b)]
    for l in range(P.L - 1):
        f.append(P.restrict_fw(f[-1], l) if P.restriction == npref.RESTRICT_FULLW else P.inject(f[-1], l))
    return f


def fmg_pass(P, b, count, coarse_sweeps):
    """mg_fmg(h, count | MG_FMG_OPERATOR(op)) on the family Problem P (its cycle kind, smoother and sweeps) ->
    (u on level 0, relres = ||b - L u|| / ||b|| (fas: ||f - N(u)|| / ||f||), b as the pass leaves it)"""
    mask = mask_of(P)
    b = P.as_prec(b)
    if is_singular(P):
        b = P.project(b)[0]
    f = restrict_rhs(P, b)
    lc = P.L - 1
    u = np.zeros(P.shape(lc), P.prec)
    dm = dirichlet_nodes(u.shape, mask)
    u[dm] = f[lc][dm]
    with np.errstate(over="ignore", invalid="ignore"):
        u = P.coarse_solve(u, f[lc], lc, coarse_sweeps)
        for l in range(P.L - 2, -1, -1):
            u = prolong(P, u, l, mask, bnd=f[l])
            for _ in range(count):
                u = P.vcycle(u, f[l], coarse_sweeps, l)
        if is_singular(P):
            u = P.project(u)[0]
        relres = math.sqrt(npref.fsum_sq(P.residual(u, b, 0)) / npref.fsum_sq(b))
    return u, relres, b


# ---------------------------------------------------------------- the cases of the FMG property (unit box, alpha = 1)
X_LO, ALL_BUT_Y_HI = br.XLO, 63 & ~br.YHI
LN10 = math.log(10.0)


def _factor(t, lo, hi, j=1):
    """a factor on [0, 1] with f' = 0 at a Neumann end and f = 0 at a Dirichlet end, j = 1, 2, ... its wave number
    -> (f, f', k^2) with f'' = -k^2 f"""
    if lo == hi:
        k = j * np.pi
        return (np.cos(k * t), -k * np.sin(k * t), k * k) if lo else (np.sin(k * t), k * np.cos(k * t), k * k)
    k = (j - 0.5) * np.pi
    return (np.cos(k * t), -k * np.sin(k * t), k * k) if lo else (np.sin(k * t), k * np.cos(k * t), k * k)


OFFSET = 0.3   # the Dirichlet data: u* = OFFSET on every Dirichlet face


def smooth_solution(n, dim, mask, amp=1.0, wave=1):
    """u* = OFFSET + the product over the axes of a factor with zero slope at the Neumann ends and zero value at the
    Dirichlet ends -> (u*, -lap u*, [d u* / d axis by array axis])"""
    t = np.linspace(0.0, 1.0, n)
    fs, ks, ds = [], [], []
    for ax in range(dim):
        lo, hi = bool(mask & face_bit(dim, ax, 0)), bool(mask & face_bit(dim, ax, 1))
        f, df, k2 = _factor(t, lo, hi, wave)
        sh = [1] * dim
        sh[ax] = n
        fs.append(f.reshape(sh)); ks.append(k2); ds.append(df.reshape(sh))
    prod = np.ones((n,) * dim)
    for f in fs:
        prod = prod * f
    grads = []
    for ax in range(dim):
        g = np.ones((n,) * dim)
        for bx in range(dim):
            g = g * (ds[bx] if bx == ax else fs[bx])
        grads.append(g)
    return amp * (OFFSET + prod), amp * sum(ks) * prod, [amp * g for g in grads]


def field_factor100(n, dim=3):
    """a = 10^(cos(pi x) cos(pi y) cos(pi z)): between 0.1 and 10, even about every face (a mirrored coefficient is smooth)
    -> (a, [d a / d axis by array axis])"""
    t = np.linspace(0.0, 1.0, n)
    cs, sn = [], []
    for ax in range(dim):
        sh = [1] * dim
        sh[ax] = n
        cs.append(np.cos(np.pi * t).reshape(sh)); sn.append((-np.pi * np.sin(np.pi * t)).reshape(sh))
    p = np.ones((n,) * dim)
    for c in cs:
        p = p * c
    a = np.exp(LN10 * p)
    grads = []
    for ax in range(dim):
        g = np.ones((n,) * dim)
        for bx in range(dim):
            g = g * (sn[bx] if bx == ax else cs[bx])
        grads.append(a * LN10 * g)
    return a, grads


# name -> (family, dim, n, levels, mask, reaction kind, gamma)
CASES = {
    "bc-xlo": ("bc", 3, 33, 4, X_LO, None, 0.0),
    "bc-allbutyhi": ("bc", 3, 33, 4, ALL_BUT_Y_HI, None, 0.0),
    "bc-2d-xlo": ("bc", 2, 65, 5, X_LO, None, 0.0),
    "vc-xlo": ("vc", 3, 33, 4, X_LO, None, 0.0),
    "vc-allbutyhi": ("vc", 3, 33, 4, ALL_BUT_Y_HI, None, 0.0),
    "fas-cubic": ("fas", 3, 33, 4, 0, fr.CUBIC, 1e3),
    "fas-exp": ("fas", 3, 33, 4, 0, fr.EXP, 20.0),
    "fasn-cubic-xlo": ("fasn", 3, 33, 4, X_LO, fr.CUBIC, 1e3),
    "fasn-cubic-allbutyhi": ("fasn", 3, 33, 4, ALL_BUT_Y_HI, fr.CUBIC, 1e3),
    "fasn-exp-xlo": ("fasn", 3, 33, 4, X_LO, fr.EXP, 20.0),
    "fasn-exp-allbutyhi": ("fasn", 3, 33, 4, ALL_BUT_Y_HI, fr.EXP, 20.0),
    "fasvc-cubic-xlo": ("fasvc", 3, 33, 4, X_LO, fr.CUBIC, 1e3),
    "fasvc-cubic-allbutyhi": ("fasvc", 3, 33, 4, ALL_BUT_Y_HI, fr.CUBIC, 1e3),
    "fasvc-exp-xlo": ("fasvc", 3, 33, 4, X_LO, fr.EXP, 20.0),
    "fasvc-exp-allbutyhi": ("fasvc", 3, 33, 4, ALL_BUT_Y_HI, fr.EXP, 20.0),
}
COARSE_SWEEPS = 50
# (amplitude, wave number) of u*, 1.0 / 1 unless named here. With gamma = 1e3 and |u*| ~ 1 the reaction's slope 3 gamma u^2
# is a hundred times the Laplacian's lowest eigenvalue: it divides the discretisation error by that much and the inequality
# of the FMG property has nothing to stand on (reference ratios 4.5 ... 31), so the cubic cases take |u*| <= 0.13.
INPUTS = {name: (0.1, 1) for name in ("fas-cubic", "fasn-cubic-xlo", "fasn-cubic-allbutyhi", "fasvc-cubic-xlo", "fasvc-cubic-allbutyhi")}
# the one case whose REFERENCE misses ||u_fmg - u_h|| <= ||u_h - u*|| with one red-black V(2,2) per level, and the ratio it
# reached (the same with vc_ref.field_smooth as the coefficient, and for every amplitude: the problem is linear); its pass
# is still compared with the reference's, only the inequality is not asked of it
DROPPED = {"vc-allbutyhi": 1.208}
PROPERTY_CASES = [name for name in CASES if name not in DROPPED]


def case_problem(name, prec=np.float64, smoother=npref.SMOOTH_RBGS, omega=1.0, cycle=CYCLE_V, coefs=None, amp=None, wave=None):
    """-> (P, b, u*, a or None): V(2,2) (or `cycle`), full weighting; coefs: the handle's mg_level_coefficients per level"""
    fam, dim, n, levels, mask, kind, gamma = CASES[name]
    kw = dict(dim=dim, n=n, levels=levels, length=1.0, alpha=1.0, smoother=smoother, omega=omega, nu_pre=2, nu_post=2,
              restriction=npref.RESTRICT_FULLW, outer_pre_gs=0, prec=prec, cycle=cycle)
    damp, dwave = INPUTS.get(name, (1.0, 1))
    ustar, mlap, grads = smooth_solution(n, dim, mask, damp if amp is None else amp, dwave if wave is None else wave)
    a = None
    if fam == "bc":
        P = br.BCProblem(mask=mask, **kw)
    elif fam == "vc":
        P = vnr.VCNProblem(mask=mask, **kw)
    elif fam == "fas":
        P = fr.FASProblem(kind=kind, gamma=gamma, **kw)
    elif fam == "fasn":
        P = fnr.FASNProblem(kind=kind, gamma=gamma, mask=mask, **kw)
    else:
        P = fvr.FASVCProblem(kind=kind, gamma=gamma, mask=mask, **kw)
    if coefs is not None:
        P.use_handle_coefs(coefs)
    if fam in ("vc", "fasvc"):
        a, ga = field_factor100(n, dim)
        b = a * mlap - sum(g * h for g, h in zip(ga, grads))
        P.set_a(a)
    else:
        b = mlap.copy()
    if kind is not None:
        b = b + gamma * (ustar ** 3 if kind == fr.CUBIC else np.exp(ustar))
    dm = dirichlet_nodes(ustar.shape, mask)
    b[dm] = ustar[dm]
    return P, b, ustar, a


def discrete_solution(P, b, maxit=80):
    """the reference solve to 1e-12 from zero -> u_h"""
    z = np.zeros(P.shape(0), P.prec)
    if hasattr(P, "react_kind"):
        u, hist, status = P.solve_history(z, b, maxit, COARSE_SWEEPS, rtol=1e-12)
        assert status == 0, hist
        return u
    out = P.solve_history(z, b, maxit, COARSE_SWEEPS, tol=1e-12)
    assert out[1][-1] <= 1e-12, out[1]
    return out[0]
