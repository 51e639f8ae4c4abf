"""The time steppers of the operator families on the CPU: tests/step_ref.py alone (no GPU, no library call).

 * the four bit-for-bit identities of DESIGN.md section 21 against tests/heat_ref.heat_rhs_np;
 * conservation with every face Neumann: w.A0 = 0 and w.u' = w.u + dt w.f - theta dt w.r for ANY approximate u';
 * the order in time of the theta scheme on the vc and the fas operator (dense solves, n = 9).
"""
import functools
import math

import numpy as np
import pytest

from tests import bc_ref as br
from tests import fas_ref as fr
from tests import heat_ref as hr
from tests import step_ref as sr
from tests import vc_ref as vr
from tests.npref import Problem, boundary_mask

LD = np.longdouble
GEOM = {"3d9": dict(dim=3, n=9, levels=1, length=1.0, alpha=1.3), "2d17": dict(dim=2, n=17, levels=1, length=2.0, alpha=0.7),
        "3d9-aniso": dict(dim=3, n=9, levels=1, length=1.0, alpha=1.0, aniso=(1.0, 30.0, 0.05))}
DT = 2e-3


def coef0(P):
    """(cx, cy, cz, cd0) as heat_rhs_np takes them, from a BCProblem's / FASProblem's own numbers (sigma = 0)"""
    ax = P.c_axes[0]
    return (ax[-1], ax[-2], ax[0] if len(ax) == 3 else 0.0, P.cd[0])


def fields(shape, T, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape).astype(T), (10.0 * rng.standard_normal(shape)).astype(T)


@pytest.mark.parametrize("T", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("src", [True, False], ids=["f", "nof"])
@pytest.mark.parametrize("geom", list(GEOM))
def test_identities_against_the_constant_stepper(geom, src, T):
    kw = GEOM[geom]
    shape = Problem(**kw).shape(0)
    u, f = fields(shape, T, 7)
    f = f if src else None
    bc0 = br.BCProblem(mask=0, prec=T, **kw)
    c0 = coef0(bc0)
    for theta in (0.5, 0.75, 1.0):
        want = hr.heat_rhs_np(u, f, c0, DT, theta)
        assert want.dtype == T
        # 1. bc with mask 0
        assert np.array_equal(sr.step_rhs(bc0, u, f, DT, theta), want)
        # 2. fas with gamma 0, both kinds
        for kind in (fr.CUBIC, fr.EXP):
            assert np.array_equal(sr.step_rhs(fr.FASProblem(kind=kind, gamma=0.0, prec=T, **kw), u, f, DT, theta), want)
    # 3. theta == 1: vc and fas (any a, any gamma) give the stencil-free form of mg_heat_rhs
    want = hr.heat_rhs_np(u, f, c0, DT, 1.0, general=False)
    assert np.array_equal(want, hr.heat_rhs_np(u, f, c0, DT, 1.0))
    vc = vr.VCProblem(prec=T, **kw)
    vc.set_a(np.random.default_rng(3).uniform(0.5, 2.0, shape))
    assert np.array_equal(sr.step_rhs(vc, u, f, DT, 1.0), want)
    assert np.array_equal(sr.step_rhs(fr.FASProblem(kind=fr.CUBIC, gamma=50.0, prec=T, **kw), u, f, DT, 1.0), want)
    # 4. theta == 1: bc is f + rdt u on the unknowns and u on the Dirichlet nodes, whatever the mask
    rdt = T(1.0 / DT)
    for mask in (br.all_faces(kw["dim"]), br.XLO | br.YHI):
        P = br.BCProblem(mask=mask, prec=T, **kw)
        t = rdt * u
        if f is not None:
            t = f + t
        assert np.array_equal(sr.step_rhs(P, u, f, DT, 1.0), np.where(P.dirichlet(shape), u, t))


@pytest.mark.parametrize("T", [np.float64, np.float32], ids=["f64", "f32"])
def test_unit_coefficient_is_the_constant_stepper_to_rounding(T):
    """a == 1: the vc expression differs from the constant one by its order of operations only -- 8 eps of the magnitudes"""
    kw = GEOM["3d9"]
    shape = Problem(**kw).shape(0)
    u, f = fields(shape, T, 11)
    vc = vr.VCProblem(prec=T, **kw)
    vc.set_a(np.ones(shape))
    c0 = coef0(br.BCProblem(mask=0, prec=T, **kw))
    for theta in (0.5, 0.75):
        got, want = sr.step_rhs(vc, u, f, DT, theta).astype(LD), hr.heat_rhs_np(u, f, c0, DT, theta).astype(LD)
        bound = 8 * float(np.finfo(T).eps) * sr.step_rhs_mag(vc, u, f, DT, theta).astype(LD)
        assert (abs(got - want) <= bound).all(), float((abs(got - want) / bound).max())


@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_conservation_with_every_face_neumann(theta):
    """w = BCProblem.weights: w.A0 = 0, so sigma w.u' = w.rhs - w.r and, with sigma = 1/(theta dt),
    w.u' = w.u + dt w.f - theta dt w.r for any u' with residual r = rhs - (sigma I + A0) u' -- converged or not.
    Long double; the bound is the rounding of the four weighted sums and of A0 u, A0 u': (N + 16) eps times the
    magnitudes, N = 729 the number of terms of a sum."""
    kw = dict(dim=3, n=9, levels=1, length=1.0, alpha=1.0)
    P0 = br.BCProblem(mask=63, prec=LD, **kw)
    lo, hi = hr.eigen_range(Problem(**kw))
    dt = 1.0 / (theta * math.sqrt(max(lo, 1.0) * hi))    # sigma between the extreme eigenvalues
    sigma = sr.shift_of(dt, theta)
    assert lo < sigma < hi
    Ps = br.BCProblem(mask=63, sigma=sigma, prec=LD, **kw)
    shape = P0.shape(0)
    w = P0.weights(shape).astype(LD)
    rng = np.random.default_rng(5)
    u, f = rng.standard_normal(shape).astype(LD), (10 * rng.standard_normal(shape) + 3.0).astype(LD)
    eps, N = float(np.finfo(LD).eps), u.size
    # w.A0 = 0: column sums of the weighted matrix, and on a random vector
    A = sr.linear_matrix(br.BCProblem(mask=63, prec=np.float64, **kw), shape)
    assert abs(w.astype(np.float64).ravel() @ A).max() <= 16 * np.finfo(np.float64).eps * abs(A).sum(axis=0).max()
    assert abs(np.sum(w * sr.n0(P0, u))) <= (N + 16) * eps * float(np.sum(w * P0.apply_A(u, 0, absolute=True)))
    st = sr.FamilyStepper(P0, Ps, dt, theta, sr.dense_solver())
    exact, rhs = st.step(u, f)
    for un in (exact, exact + LD(0.1) * rng.standard_normal(shape).astype(LD), u):
        r = rhs - sr.n0(Ps, un)
        lhs = np.sum(w * un)
        want = np.sum(w * u) + LD(dt) * np.sum(w * f) - LD(theta) * LD(dt) * np.sum(w * r)
        mag = np.sum(w * (abs(un) + abs(u) + LD(dt) * abs(f) + LD(theta * dt) * abs(r)
                          + LD(dt) * (P0.apply_A(u, 0, absolute=True) + Ps.apply_A(un, 0, absolute=True))))
        assert abs(lhs - want) <= (N + 16) * eps * float(mag), (float(abs(lhs - want)), float(mag))
    assert float(np.sqrt(np.sum((rhs - sr.n0(Ps, exact)) ** 2) / np.sum(rhs ** 2))) < 1e-15


def smooth_start(n):
    X, Y, Z = vr.grid(n)
    u = np.sin(np.pi * X) * np.sin(np.pi * Y) * np.sin(np.pi * Z)
    u[boundary_mask(u.shape)] = 0.0
    return u, 5.0 * np.sin(np.pi * X) * np.sin(2 * np.pi * Y) * np.sin(np.pi * Z)


def family_pair(fam, sigma):
    kw = dict(dim=3, n=9, levels=1, length=1.0, alpha=1.0, prec=np.float64)
    if fam == "vc":
        out = [vr.VCProblem(sigma=s, **kw) for s in (0.0, sigma)]
        for P in out:
            P.set_a(vr.field_smooth(9))
        return out
    return [fr.FASProblem(kind=fr.CUBIC, gamma=50.0, sigma=s, **kw) for s in (0.0, sigma)]


@functools.lru_cache(maxsize=None)
def run_to(fam, theta, t_end, steps):
    dt = t_end / steps
    P0, Ps = family_pair(fam, sr.shift_of(dt, theta))
    st = sr.FamilyStepper(P0, Ps, dt, theta, sr.dense_solver(newton=4))
    u, f = smooth_start(9)
    for _ in range(steps):
        u, _ = st.step(u, f)
    return u


@pytest.mark.parametrize("theta, lo, hi", [(0.5, 3.0, 5.0), (1.0, 1.6, 2.4)])
@pytest.mark.parametrize("fam", ["vc", "fas"])
def test_order_in_time(fam, theta, lo, hi):
    """halving dt divides the error at t_end by 4 (theta = 1/2) or 2 (theta = 1); the reference is the trapezoidal rule
    with a 16 times finer step than the finer run. The windows are those of tests/test_heat_gpu.py."""
    t_end = 0.02
    ref = run_to(fam, 0.5, t_end, 256)
    e = [float(np.abs(run_to(fam, theta, t_end, k) - ref).max()) for k in (8, 16)]
    assert lo < e[0] / e[1] < hi, (e, e[0] / e[1])
