"""Nested iteration on the operator families on the GPU: mg_fmg / mg_fmg_prolong with MG_FMG_OPERATOR(op) (include/mg_hip.h,
DESIGN.md section 27) against tests/fmgop_ref.py.

 a. the mirrored interpolation (mg_fmg.hip, both kernel forms) bit for bit, every op, masks 0, 1, 2, 4, 16, 32, 55, 63;
 b. the padding columns and ghost planes after each of those launches (tests/test_storage_gpu.py's checker);
 c. the whole pass against the reference pass, and the FMG property on the cases chosen in tests/test_fmgop_cpu.py;
 d. what it is for: mg_vc_solve and mg_fas_solve need fewer cycles from the FMG iterate than from zero;
 e. refusals, and the unflagged calls."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from multigrid_prj_amd import capi
from tests import fas_ref as fr
from tests import fmgop_ref as fo
from tests import npref
from tests import npref_fmg as nf
from tests import storage_table as st
from tests import test_storage_gpu as sg
from tests.test_fmg_gpu import COARSE_SWEEPS as PLAIN_SWEEPS
from tests.test_fmg_gpu import FMG_K, fmg_kw, fmg_rhs, fmg_scale
from tests.test_independent_reference import check_max, cycle_bound

pytestmark = pytest.mark.gpu

NP = {capi.MG_F64: np.float64, capi.MG_F32: np.float32}
LD = np.longdouble
U, E, RHS = capi.ARR_U, capi.ARR_E, capi.ARR_RHS
JAC, RB = capi.SMOOTH_JACOBI, capi.SMOOTH_RBGS
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MASKS = (0, 1, 2, 4, 16, 32, 55, 63)
OPS = (capi.FMG_ON_FACES, capi.FMG_ON_COEFFICIENT, capi.FMG_ON_REACTION)


def test_the_interface_constants():
    assert (capi.FMG_ON_CONSTANT, capi.FMG_ON_FACES, capi.FMG_ON_COEFFICIENT, capi.FMG_ON_REACTION) == (0, 1, 2, 3)
    assert capi.fmg_operator(3) == 3 << 16 == fo.operator_flag(fo.ON_REACTION)


# ---------------------------------------------------------------- a. the interpolation, bit for bit
# 17 -> 33: the streaming kernel in both dtypes; 9 -> 17, 5 -> 9, 3 -> 5: the gather kernel; 2-D; a semi-coarsened transition
# (z kept: 33 planes of 17 x 17 -> 33 x 33); grids that are not 2^k + 1 (tests/size_table.py: 97 -> 49 -> 25, 77 -> 39): 25 -> 49
# streams with partial waves, 14 -> 27 gathers with an even coarse row
TRANSITIONS = [dict(dim=3, n=33, levels=2), dict(dim=3, n=17, levels=2), dict(dim=3, n=9, levels=2), dict(dim=3, n=5, levels=2),
               dict(dim=2, n=33, levels=2), dict(dim=3, n=33, levels=2, semi_xy=1), dict(dim=3, n=49, levels=2), dict(dim=3, n=27, levels=2)]


def tid(c):
    return f"{c['dim']}d{c['n']}" + ("-semi" if c.get("semi_xy") else "")


def masks_of(dim):
    return tuple(m for m in MASKS if dim == 3 or not m & 48) + ((7, 15) if dim == 2 else ())


def set_mask(s, op, mask):
    """the mask where `op` reads it; ON_REACTION: through MG_FAS_ON_FACES for masks with x-lo in them, through MG_FAS_ON_COEFFICIENT for the others"""
    if op == capi.FMG_ON_FACES:
        s.bc_set_faces(mask)
    elif op == capi.FMG_ON_COEFFICIENT:
        s.vc_set_faces(mask)
    elif mask & 1:
        s.fas_set_reaction(capi.FAS_CUBIC | capi.FAS_ON_FACES, 1.0); s.bc_set_faces(mask); s.vc_set_faces(0)
    else:
        s.fas_set_reaction(capi.FAS_EXP | capi.FAS_ON_COEFFICIENT, 1.0); s.vc_set_faces(mask); s.bc_set_faces(0)


def interp_inputs(P, T, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(P.shape(1)).astype(T), rng.standard_normal(P.shape(0)).astype(T)


@pytest.mark.parametrize("dtype", [capi.MG_F64, capi.MG_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", TRANSITIONS, ids=tid)
def test_interpolation_bit_for_bit(case, dtype):
    T = NP[dtype]
    P = npref.Problem(prec=T, **case)
    c, bnd = interp_inputs(P, T, case["n"])
    with capi.Solver(capi.make_desc(dtype=dtype, **case)) as s:
        s.vc_set_coefficient(np.full(P.shape(0), 1.5))
        s.set_array(U, 1, c); s.set_array(RHS, 0, bnd)
        plain = {}
        for ab in (RHS, -1):
            s.set_array(E, 0, np.full(P.shape(0), np.nan, T))
            s.fmg_prolong(1, U, E, ab)
            plain[ab] = s.get_array(E, 0)
        for k, mask in enumerate(masks_of(case["dim"])):
            for op in OPS:
                set_mask(s, op, mask)
                for ab in ((RHS, -1) if (k + op) % 2 == 0 or mask in (0, 55) else (RHS,)):   # arr_bnd < 0 in some
                    s.set_array(E, 0, np.full(P.shape(0), np.nan, T))
                    s.fmg_prolong(1, U, E, ab, op=op)
                    got = s.get_array(E, 0)
                    want = fo.prolong(P, c, 0, mask, bnd=bnd if ab >= 0 else None)
                    bad = np.argwhere(got != want)
                    assert np.array_equal(got, want), f"mask {mask} op {op} bnd {ab}: {len(bad)} nodes differ, first {bad[:3].tolist()}"
                    if mask == 0:
                        assert np.array_equal(got, plain[ab]), "mask 0 with an op: the unflagged call's bits"
        assert np.array_equal(s.get_array(RHS, 0), bnd) and np.array_equal(s.get_array(U, 1), c)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from multigrid_prj_amd import capi
dim, n, dtype, semi, masks = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), [int(m) for m in sys.argv[6].split(",")]
T = np.float64 if dtype == capi.MG_F64 else np.float32
out = {}
with capi.Solver(capi.make_desc(dim=dim, n=n, levels=2, dtype=dtype, semi_xy=semi)) as s:
    rng = np.random.default_rng(n)
    s.set_array(capi.ARR_U, 1, rng.standard_normal(s.level_shape(1)).astype(T))
    s.set_array(capi.ARR_RHS, 0, rng.standard_normal(s.level_shape(0)).astype(T))
    for mask in masks:
        s.bc_set_faces(mask)
        for ab in (capi.ARR_RHS, -1):
            s.fmg_prolong(1, capi.ARR_U, capi.ARR_E, ab, op=capi.FMG_ON_FACES)
            out[f"m{mask}b{ab}"] = s.get_array(capi.ARR_E, 0)
np.savez(sys.argv[7], **out)
print("child ok")
"""


@pytest.mark.parametrize("n,dtype,semi", [(33, capi.MG_F64, 0), (33, capi.MG_F32, 0), (33, capi.MG_F64, 1), (49, capi.MG_F32, 0)])
def test_both_kernel_forms_give_the_same_bits(n, dtype, semi, tmp_path):
    """MG_FMG_FAST=0 (read once per process: a child each) sends these transitions to the gather kernel; same bits for every mask,
    and both are the reference's"""
    T = NP[dtype]
    outs = {}
    for tag, env in (("fast", {}), ("gather", {"MG_FMG_FAST": "0"})):
        path = str(tmp_path / (tag + ".npz"))
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, "3", str(n), str(dtype), str(semi), ",".join(map(str, MASKS)), path],
                           env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "child ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
        outs[tag] = dict(np.load(path))
    case = dict(dim=3, n=n, levels=2, semi_xy=semi)
    P = npref.Problem(prec=T, **case)
    c, bnd = interp_inputs(P, T, n)
    for mask in MASKS:
        for ab in (RHS, -1):
            k = f"m{mask}b{ab}"
            assert np.array_equal(outs["fast"][k], outs["gather"][k]), k
            assert np.array_equal(outs["gather"][k], fo.prolong(P, c, 0, mask, bnd=bnd if ab >= 0 else None)), k


# ---------------------------------------------------------------- b. storage
def _storage_setup(x, v):
    x.s.bc_set_faces(v["mask"])


def _storage_call(x, v):
    x.s.fmg_prolong(1, U, E, v["bnd"], op=capi.FMG_ON_FACES)   # the checker resets the mask before the next variant
    return ()


STORAGE_CASES = [st.C(3, 33, 2), st.C(3, 17, 2), st.C(3, 9, 2), st.C(3, 5, 2), st.C(2, 33, 2), st.C(3, 33, 2, semi_xy=1), st.C(3, 49, 2),
                 st.C(3, 27, 2), st.C(3, 67, 2)]   # 67: the tail line of the streaming kernel next to a partial fp32 vector
STORAGE_ROW = st.Row("fmg-prolong-op", ("mg_fmg_prolong",), tuple(STORAGE_CASES), tuple(st.BOTH),
                     lambda case, dtype: st.product(mask=masks_of(case.dim)[1:], bnd=(RHS, -1)), _storage_setup, _storage_call,
                     lambda x, v: st.lv(0, E), ())
STORAGE_PAIRS = [(STORAGE_ROW, c, dt) for c in STORAGE_CASES for dt in st.BOTH]


@pytest.fixture(scope="module")
def _storage_handles():
    sg.close_handles()
    yield
    sg.close_handles()


@pytest.mark.parametrize("p", STORAGE_PAIRS, ids=st.pair_id)
def test_storage_after_the_mirrored_interpolation(p, _storage_handles):
    """check a: padding columns and ghost planes of arr_dst hold what they held, nothing but arr_dst is written; check b: nothing
    written depends on what lies outside the dense grid"""
    fails_a, fails_b = sg.run(*p)
    assert not fails_a and not fails_b, f"{len(fails_a)} + {len(fails_b)} failures:\n" + "\n".join((fails_a + fails_b)[:12])


# ---------------------------------------------------------------- c. the pass
KINDS = {"v-rb-1": (capi.CYCLE_V, RB, 1.0, 1), "w-rb-2": (capi.CYCLE_W, RB, 1.0, 2), "v-jac-2": (capi.CYCLE_V, JAC, 6.0 / 7.0, 2),
         "w-jac-1": (capi.CYCLE_W, JAC, 6.0 / 7.0, 1)}
F32_CASES = ("bc-allbutyhi", "vc-xlo", "fasn-cubic-xlo", "fasvc-exp-allbutyhi")
PASS_PARAMS = [(name, kind, capi.MG_F64) for name in fo.CASES for kind in KINDS] + [(name, "v-rb-1", capi.MG_F32) for name in F32_CASES]


def case_desc(name, kind, dtype):
    fam, dim, n, levels, mask, rk, gamma = fo.CASES[name]
    cycle, smoother, omega, count = KINDS[kind]
    kw = dict(dim=dim, n=n, levels=levels, length=1.0, alpha=1.0, dtype=dtype, cycle=cycle, smoother=smoother, omega=omega, nu_pre=2, nu_post=2,
              restriction=capi.RESTRICT_FULLW, outer_pre_gs=0, coarse_mode=capi.COARSE_FIXED, coarse_maxit=fo.COARSE_SWEEPS)
    return kw, count


def setup_family(s, name, a, T):
    """the handle's state for the case -> the op of the flagged calls"""
    fam, dim, n, levels, mask, rk, gamma = fo.CASES[name]
    kind = None if rk is None else (capi.FAS_CUBIC if rk == fr.CUBIC else capi.FAS_EXP)
    if fam == "bc":
        s.bc_set_faces(mask)
        return capi.FMG_ON_FACES
    if fam == "vc":
        s.vc_set_coefficient(a.astype(T)); s.vc_set_faces(mask)
        return capi.FMG_ON_COEFFICIENT
    if fam == "fas":
        s.fas_set_reaction(kind, gamma)
    elif fam == "fasn":
        s.fas_set_reaction(kind | capi.FAS_ON_FACES, gamma); s.bc_set_faces(mask)
    else:
        s.vc_set_coefficient(a.astype(T)); s.vc_set_faces(mask); s.fas_set_reaction(kind | capi.FAS_ON_COEFFICIENT, gamma)
    return capi.FMG_ON_REACTION


@functools.lru_cache(maxsize=None)
def pass_reference(name, kind, prec, T, coefs):
    """the reference pass in `prec` on the inputs rounded to T, with the handle's level coefficients"""
    cycle, smoother, omega, count = KINDS[kind]
    P, b, _, a = fo.case_problem(name, prec=prec, smoother=smoother, omega=omega, cycle=cycle, coefs=coefs)
    if a is not None:
        P.set_a(a.astype(T))
    u, relres, _ = fo.fmg_pass(P, b.astype(T), count, fo.COARSE_SWEEPS)
    return u, relres, P


@functools.lru_cache(maxsize=None)
def discrete_solution(name):
    P, b, ustar, _ = fo.case_problem(name)
    uh = fo.discrete_solution(P, b)
    return uh, float(abs(uh - ustar).max())


def operator_norm(name, coefs, a, u):
    """a bound of the max row sum of the Jacobian at u: 2 |cd| max(a) + |gamma| max |g'(u)| (relres tolerance below)"""
    fam, dim, n, levels, mask, rk, gamma = fo.CASES[name]
    lin = 2.0 * abs(coefs[0][3]) * (float(a.max()) if a is not None else 1.0)
    if rk is None:
        return lin
    return lin + abs(gamma) * float((3 * u * u).max() if rk == fr.CUBIC else np.exp(u).max())


@pytest.mark.parametrize("name,kind,dtype", PASS_PARAMS, ids=[f"{n}-{k}-{'f64' if d == capi.MG_F64 else 'f32'}" for n, k, d in PASS_PARAMS])
def test_pass_against_the_reference(name, kind, dtype):
    """U(0) against the long-double reference pass on the handle's level coefficients, with the tolerance of the families' cycle
    tests (test_bc_gpu.py, test_vcn_gpu.py, test_fas_gpu.py, test_fasn_gpu.py, test_fasvc_gpu.py: 4 x the distance of the
    reference run in the working dtype from the one in long double); stats.relres against the reference's, where a
    difference d in u moves the residual norm by at most ||J|| d sqrt(N) -- a weak bound in fp32, so stats.relres is also held
    to the long-double residual OF THE U(0) RETURNED, within the rounding of one residual evaluation in the working dtype
    (16 eps || |b| + |A||u| + |gamma g| || / ||b||); RHS(0) bit-identical; the FMG property where the CPU test kept the case
    (one red-black V(2,2) per level, fp64)"""
    T = NP[dtype]
    kw, count = case_desc(name, kind, dtype)
    _, b, _, a = fo.case_problem(name)
    b = b.astype(T)
    with capi.Solver(capi.make_desc(**kw)) as s:
        op = setup_family(s, name, a, T)
        coefs = tuple(s.level_coefficients(l) for l in range(kw["levels"]))
        (u_T, rr_T, _), (u_LD, rr_LD, P_LD) = pass_reference(name, kind, T, T, coefs), pass_reference(name, kind, LD, T, coefs)
        tol = 4 * float(abs(u_T.astype(LD) - u_LD).max())
        s.set_rhs(b); s.set_solution(np.full(b.shape, np.nan, T))   # the incoming U(0) is ignored
        stats = s.fmg(count, op=op)
        got = s.get_solution()
        err = float(abs(got.astype(LD) - u_LD).max())
        rr_tol = operator_norm(name, coefs, a, np.asarray(u_LD, np.float64)) * tol * math.sqrt(b.size) / math.sqrt(npref.fsum_sq(b)) \
            + 4 * abs(rr_T - rr_LD)
        print(f"{name} {kind} {T.__name__}: |gpu - ld| {err:.3e} tolerance {tol:.3e}; relres gpu {stats.relres:.6e} ld {rr_LD:.6e} tolerance {rr_tol:.1e}")
        assert err <= tol
        assert abs(stats.relres - rr_LD) <= rr_tol
        nb = math.sqrt(npref.fsum_sq(b))
        rr_got = math.sqrt(npref.fsum_sq(P_LD.residual(got, b, 0))) / nb
        mag = P_LD.residual_mag(got, b, 0) if hasattr(P_LD, "residual_mag") else abs(P_LD.as_prec(b)) + P_LD.apply_A(got, 0, absolute=True)
        rr_eps = 16 * float(np.finfo(T).eps) * math.sqrt(npref.fsum_sq(mag)) / nb
        print(f"    relres of the U(0) returned, in long double: {rr_got:.9e}; gpu - that {stats.relres - rr_got:.2e}, rounding bound {rr_eps:.2e}")
        assert abs(stats.relres - rr_got) <= rr_eps
        assert (stats.levels, stats.cycles_per_level, stats.coarse_iters, stats.coarse_flag) == (kw["levels"], count, fo.COARSE_SWEEPS, 0)
        assert np.array_equal(s.get_array(RHS, 0), b), "RHS(0) is unchanged"
        dm = fo.dirichlet_nodes(b.shape, fo.CASES[name][4])
        assert np.array_equal(got[dm], b[dm])
        if kind == "v-rb-1" and dtype == capi.MG_F64 and name in fo.PROPERTY_CASES:
            uh, e_disc = discrete_solution(name)
            e_alg = float(abs(got - uh).max())
            print(f"{name}: ||u_fmg - u_h|| {e_alg:.3e} ||u_h - u*|| {e_disc:.3e}")
            assert e_alg <= e_disc


def test_singular_all_neumann_pass():
    """mask 63, no shift: RHS(0) is projected and stays projected, the weighted mean of U(0) is zero, relres is the reference's"""
    from tests import bc_ref as br
    kw = dict(dim=3, n=17, levels=3, length=1.0, alpha=1.0, dtype=capi.MG_F64, cycle=capi.CYCLE_V, smoother=RB, omega=1.0, nu_pre=2, nu_post=2,
              restriction=capi.RESTRICT_FULLW, outer_pre_gs=0, coarse_mode=capi.COARSE_FIXED, coarse_maxit=30)
    P = br.convergence_problem("all-neumann-singular", n=17, levels=3)
    b = br.convergence_rhs(P.shape(0), seed=5)
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.bc_set_faces(63)
        P.use_handle_coefs([s.level_coefficients(l) for l in range(3)])
        u_ref, rr_ref, b_ref = fo.fmg_pass(P, b, 1, 30)
        s.set_rhs(b); s.set_solution(np.zeros_like(b))
        stats = s.fmg(1, op=capi.FMG_ON_FACES)
        u, w = s.get_solution(), P.weights(b.shape)
        print(f"relres gpu {stats.relres:.12e} reference {rr_ref:.12e}")
        assert stats.relres == pytest.approx(rr_ref, rel=1e-9)
        assert abs((w * u).sum()) <= 1e-12 * (w * abs(u)).sum()
        assert abs(s.get_array(RHS, 0) - b_ref).max() <= 4 * np.finfo(np.float64).eps * abs(b).max()
        assert abs(u - u_ref).max() <= 1e-10 * abs(u_ref).max()


# ---------------------------------------------------------------- d. what it is for
def test_vc_solve_needs_fewer_cycles_from_the_fmg_iterate():
    name, tol, maxit = "vc-xlo", 1e-8, 40
    kw, _ = case_desc(name, "v-rb-1", capi.MG_F64)
    _, b, _, a = fo.case_problem(name)
    with capi.Solver(capi.make_desc(**kw)) as s:
        op = setup_family(s, name, a, np.float64)
        P, _, _, _ = fo.case_problem(name, coefs=[s.level_coefficients(l) for l in range(kw["levels"])])
        ref_zero = len(P.solve_history(np.zeros_like(b), b, maxit, fo.COARSE_SWEEPS, tol=tol)[1]) - 1
        ref_fmg = len(P.solve_history(fo.fmg_pass(P, b, 1, fo.COARSE_SWEEPS)[0], b, maxit, fo.COARSE_SWEEPS, tol=tol)[1]) - 1
        s.set_rhs(b); s.set_solution(np.zeros_like(b))
        zero = len(s.vc_solve(tol, maxit)[0]) - 1
        st_ = s.fmg(1, op=op)
        hist = s.vc_solve(tol, maxit)[0]
        print(f"mg_vc_solve to {tol}: {zero} cycles from zero, {len(hist) - 1} from the FMG iterate (reference {ref_zero}, {ref_fmg})")
        assert hist[0] == pytest.approx(st_.relres, rel=1e-9)
        assert (zero, len(hist) - 1) == (ref_zero, ref_fmg) and len(hist) - 1 < zero


def test_fas_solve_needs_fewer_cycles_from_the_fmg_iterate():
    name, maxit = "fasvc-exp-xlo", 40
    kw, _ = case_desc(name, "v-rb-1", capi.MG_F64)
    _, b, _, a = fo.case_problem(name)
    atol = 1e-8 * math.sqrt(npref.fsum_sq(b))
    with capi.Solver(capi.make_desc(**kw)) as s:
        op = setup_family(s, name, a, np.float64)
        P, _, _, _ = fo.case_problem(name, coefs=[s.level_coefficients(l) for l in range(kw["levels"])])
        ref_zero = len(P.solve_history(np.zeros_like(b), b, maxit, fo.COARSE_SWEEPS, atol=atol)[1]) - 1
        ref_fmg = len(P.solve_history(fo.fmg_pass(P, b, 1, fo.COARSE_SWEEPS)[0], b, maxit, fo.COARSE_SWEEPS, atol=atol)[1]) - 1
        s.set_rhs(b); s.set_solution(np.zeros_like(b))
        h0, st0 = s.fas_solve(0.0, atol, maxit)
        s.fmg(1, op=op)
        h1, st1 = s.fas_solve(0.0, atol, maxit)
        print(f"mg_fas_solve to {atol:.3e}: {st0.cycles} cycles from zero, {st1.cycles} from the FMG iterate (reference {ref_zero}, {ref_fmg})")
        assert st0.status == 0 and st1.status == 0
        assert (st0.cycles, st1.cycles) == (ref_zero, ref_fmg) and st1.cycles < st0.cycles


# ---------------------------------------------------------------- e. refusals and the unflagged calls
def _refused(s, call):
    u0 = s.get_solution()
    with pytest.raises(capi.MgError) as e:
        call()
    assert e.value.code == -4, e.value
    assert np.array_equal(s.get_solution(), u0)


def test_refusals_leave_u_untouched():
    kw = dict(dim=3, n=17, levels=3, length=1.0, alpha=1.0, dtype=capi.MG_F64, cycle=capi.CYCLE_V, smoother=JAC, omega=6 / 7, nu_pre=2,
              nu_post=2, restriction=capi.RESTRICT_FULLW, outer_pre_gs=0)
    rng = np.random.default_rng(6)
    b, u = rng.standard_normal((17,) * 3), rng.standard_normal((17,) * 3)
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_rhs(b); s.set_solution(u); s.bc_set_faces(capi.FACE_XLO)
        _refused(s, lambda: capi._check(s.lib.mg_fmg(s.h, 1 | (4 << 16), None)))           # unknown op bits
        _refused(s, lambda: capi._check(s.lib.mg_fmg(s.h, 1 | capi.fmg_operator(capi.FMG_ON_FACES) | (1 << 20), None)))
        _refused(s, lambda: capi._check(s.lib.mg_fmg_prolong(s.h, 1 | (1 << 18), U, E, -1)))
        for op in OPS[:1] + OPS[2:]:
            _refused(s, lambda: s.fmg(0, op=op))                     # count 0
        _refused(s, lambda: s.fmg(1, op=capi.FMG_ON_COEFFICIENT))    # no coefficient
        _refused(s, lambda: s.fmg_prolong(1, U, E, -1, op=capi.FMG_ON_COEFFICIENT))
        s.fas_set_reaction(capi.FAS_CUBIC | capi.FAS_ON_COEFFICIENT, 1.0)
        _refused(s, lambda: s.fmg(1, op=capi.FMG_ON_REACTION))
        s.fas_set_reaction(capi.FAS_CUBIC, 1.0)
        s.set_stage_callback(lambda *a: None)
        for op in OPS[:1] + OPS[2:]:
            _refused(s, lambda: s.fmg(1, op=op))
        s.set_stage_callback(None)
        _refused(s, lambda: s.fmg_prolong(3, U, E, -1, op=capi.FMG_ON_FACES))     # a bad level
        _refused(s, lambda: s.fmg_prolong(0, U, E, -1, op=capi.FMG_ON_FACES))
        _refused(s, lambda: s.fmg_prolong(1, U, E, E, op=capi.FMG_ON_FACES))
        s.fmg(1, op=capi.FMG_ON_FACES)   # and the handle still works
        assert np.isfinite(s.get_solution()).all()
    for bad in (dict(cycle=capi.CYCLE_SAWTOOTH, nu_pre=0, restriction=capi.RESTRICT_INJECT), dict(smoother=capi.SMOOTH_GS_LEX, omega=1.0)):
        with capi.Solver(capi.make_desc(**dict(kw, **bad))) as s:
            s.set_rhs(b); s.set_solution(u)
            for op in OPS[:1] + OPS[2:]:
                _refused(s, lambda: s.fmg(1, op=op))
    with capi.Solver(capi.make_desc(**dict(kw, n=65, levels=3)), rank=0, nranks=2, dry=True) as s:
        _refused(s, lambda: s.fmg(1, op=capi.FMG_ON_FACES))
        _refused(s, lambda: s.fmg_prolong(1, U, E, -1, op=capi.FMG_ON_FACES))


@pytest.mark.parametrize("row", [dict(id="3d-f64-33-jacobi", dim=3, n=33, levels=3, dtype=capi.MG_F64, smoother=JAC, omega=6 / 7),
                                 dict(id="3d-f32-65-rbgs", dim=3, n=65, levels=4, dtype=capi.MG_F32, smoother=RB, omega=1.0),
                                 dict(id="2d-f64-65-jacobi", dim=2, n=65, levels=5, dtype=capi.MG_F64, smoother=JAC, omega=0.8)],
                         ids=lambda r: r["id"])
def test_unflagged_fmg_is_what_it_was(row):
    """mg_fmg without a flag on a plain handle against npref_fmg's pass, with tests/test_fmg_gpu.py's bound; MG_FMG_ON_CONSTANT
    and a Neumann mask left on the handle change no bit of it"""
    kw = fmg_kw(row)
    T = NP[kw["dtype"]]
    P = npref.Problem(prec=LD, **kw)
    b = fmg_rhs(P, T, kw["n"])
    with capi.Solver(capi.make_desc(**kw)) as s:
        for k in (1, 2):
            s.set_rhs(b)
            st_ = s.fmg(k)
            got = s.get_solution()
            ref = nf.fmg(P, b, k, PLAIN_SWEEPS)
            check_max(got, ref, FMG_K * cycle_bound(P, float(np.finfo(T).eps), PLAIN_SWEEPS, fmg_scale(P, b, ref)), f"fmg({k})")
            s.bc_set_faces(63 if kw["dim"] == 3 else 15)
            st2 = s.fmg(k, op=capi.FMG_ON_CONSTANT)
            assert np.array_equal(s.get_solution(), got) and st2.relres == st_.relres
            s.bc_set_faces(0)
