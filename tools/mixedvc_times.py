"""mixedvc_times -- the mixed-precision defect correction on the variable-coefficient operator (mg_mixed_solve / mg_mixed_kernel
with MG_MIXED_OPERATOR(MG_MIXED_ON_COEFFICIENT)) against its yardsticks, one part per process so that each can run under a
time limit of its own:

    python tools/mixedvc_times.py --part kernel     # the fused correct + residual launch: tile against the plain form, mask 0 and
                                                    # all faces Neumann; an fp64 handle's mg_vc_residual tile (32 B per node) and the
                                                    # constant k_mixed_correct_residual (32 B per node) as bandwidth yardsticks
    python tools/mixedvc_times.py --part smooth     # smooth factor-100 field, all faces Neumann, shift 10, tol 1e-10: mixed with
                                                    # 1 / 2 / 4 cycles per correction against mg_vc_solve on an fp64 handle
    python tools/mixedvc_times.py --part jump       # aligned jump of 1000, only y-hi Dirichlet, to 1e-8: mixed with 8 CG iterations
                                                    # per correction against mg_vc_pcg_solve on an fp64 handle
    python tools/mixedvc_times.py --n 257 --levels 5 --repeats 7

513^3, 6 levels, red-black V(2,2), full weighting, 50 fixed coarse sweeps by default; the right-hand side is the benchmark's
(bench.py: hash_rhs), the first guess zero. Every solver is warmed up once, then the timed runs alternate between the solvers
`--repeats` times; the tables give the median and the spread (min .. max) of the host wall clock around the call (the calls end
in a device synchronisation) and of the HIP-event time on the handle's stream. The fused launch moves 8 (u) + 4 (e) + 4 (a) +
8 (b) bytes in and 8 (u') + 4 (r32) out per node: 36 B, on which its rate is given.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0
ALL_FACES, ONLY_YHI_DIRICHLET = 63, 63 & ~8


def grid(n):
    t = np.linspace(0.0, 1.0, n)
    return np.meshgrid(t, t, t, indexing="ij", sparse=True)   # z, y, x


def field_smooth(n):
    """10^(sin 2 pi x cos 2 pi y cos pi z): between 0.1 and 10"""
    Z, Y, X = grid(n)
    return np.exp(math.log(10.0) * np.sin(2 * np.pi * X) * np.cos(2 * np.pi * Y) * np.cos(np.pi * Z))


def field_jump_aligned(n, c=1000.0):
    Z, Y, X = grid(n)
    return np.where((abs(X - .5) <= .25) & (abs(Y - .5) <= .25) & (abs(Z - .5) <= .25), c, 1.0)


def timed(s, fn):
    t0 = time.perf_counter(); s.timer_start()
    out = fn()
    ms = s.timer_stop(); wall = (time.perf_counter() - t0) * 1e3
    return out, wall, ms


def med(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:9.3f} ({v[0]:.3f} .. {v[-1]:.3f})"


def alternate(runs, repeats):
    for fn in runs.values():   # warm-up: every kernel of every solver once
        fn()
    res = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            res[k].append(fn())
    return res


def table(res, base):
    print(f"{'solver':30s} {'cycles':>6s} {'corr.':>5s} {'true relres':>11s} {'reached':>7s}  {'host wall ms: median (min .. max)':>38s}  "
          f"{'device ms: median (min .. max)':>38s}")
    for k, rs in res.items():
        r = rs[0]
        assert all(x["cycles"] == r["cycles"] and x["true"] == r["true"] for x in rs), "runs of one solver differ"
        print(f"{k:30s} {r['cycles']:6d} {r.get('outer', 0):5d} {r['true']:11.3e} {str(bool(r['reached'])):>7s}  {spread([x['wall'] for x in rs]):>38s}  "
              f"{spread([x['ms'] for x in rs]):>38s}", flush=True)
    b = sorted(x["wall"] for x in res[base])
    for k, rs in res.items():
        if k == base:
            continue
        w = sorted(x["wall"] for x in rs)
        verdict = "faster beyond the spread" if w[-1] < b[0] else ("slower beyond the spread" if w[0] > b[-1] else "within the spread")
        print(f"{k:30s} median wall / {base} median wall = {med(w) / med(b):.3f}  ({verdict})")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=("kernel", "smooth", "jump"), default="kernel")
    ap.add_argument("--n", type=int, default=513)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--maxit", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=9)
    a = ap.parse_args()

    from bench import hash_rhs
    from multigrid_prj_amd import capi
    COEF = capi.MIXED_ON_COEFFICIENT
    kw = dict(dim=3, n=a.n, levels=a.levels, length=1.0, alpha=1.0, cycle=capi.CYCLE_V, smoother=capi.SMOOTH_RBGS, nu_pre=2, nu_post=2,
              restriction=capi.RESTRICT_FULLW, coarse_mode=capi.COARSE_FIXED, coarse_maxit=50, outer_pre_gs=0)
    pts = a.n ** 3
    print(f"# part {a.part}: 3-D {a.n}^3, {a.levels} levels, red-black V(2,2), full weighting, 50 coarse sweeps; benchmark right-hand side, "
          f"zero first guess; {a.repeats} alternating repeats after one warm-up", flush=True)
    b = hash_rhs(a.n, np.float64)
    zero = np.zeros_like(b)
    s32 = capi.Solver(capi.make_desc(**kw, dtype=capi.MG_F32))
    s64 = capi.Solver(capi.make_desc(**kw))

    if a.part == "kernel":
        af = field_smooth(a.n)
        s32.vc_set_coefficient(af.astype(np.float32)); s64.vc_set_coefficient(af)
        s32.mixed_set_rhs(b); s32.mixed_set_solution(zero)
        s64.set_rhs(b); s64.set_solution(zero)
        e = np.random.default_rng(1).standard_normal(b.shape).astype(np.float32)
        s32.set_array(capi.ARR_E, 0, e)
        del e
        K = capi.MIXED_K_CORRECT_RESIDUAL

        def fused(form, op):
            def f():
                s32.vc_set_form(form)
                return timed(s32, lambda: s32.mixed_kernel(K, 2.0 ** 20, 1.0, capi.ARR_E, capi.ARR_RHS, op=op))[2]
            return f

        def vc64(form):
            def f():
                s64.vc_set_form(form)
                return timed(s64, lambda: s64.vc_residual(0, capi.ARR_U, capi.ARR_RHS, capi.ARR_TMP))[2]
            return f

        for mask, name in ((0, "mask 0"), (ALL_FACES, "all faces Neumann")):
            s32.vc_set_faces(mask); s64.vc_set_faces(mask)
            runs = {"fused vc tile": fused(0, COEF), "fused vc plain form": fused(1, COEF), "fp64 mg_vc_residual tile": vc64(0),
                    "constant k_mixed_correct_residual": fused(0, capi.MIXED_ON_CONSTANT)}
            res = alternate(runs, a.kreps)
            print(f"-- {name}; device ms of the launch + the sum of its partials + the copy of the norm: median (min .. max)")
            for k, v in res.items():
                bpn = 36 if k.startswith("fused") else 32
                gb = bpn * pts / 1e9
                print(f"{k:36s} {spread(v)} ms; {bpn} B/node = {gb:.2f} GB -> {gb / med(v):.2f} TB/s = {gb / med(v) / PEAK_TBS:.1%} of the "
                      f"{PEAK_TBS:g} TB/s peak", flush=True)
        s32.vc_set_form(0); s64.vc_set_form(0)

    elif a.part == "smooth":
        tol = 1e-10
        af = field_smooth(a.n)
        for s, arr in ((s32, af.astype(np.float32)), (s64, af)):
            s.set_shift(10.0); s.vc_set_coefficient(arr); s.vc_set_faces(ALL_FACES)
        s32.mixed_set_rhs(b); s64.set_rhs(b)
        bb = float(np.sum(b.astype(np.longdouble) ** 2))

        def run64():
            s64.set_solution(zero)
            (hist, _), wall, ms = timed(s64, lambda: s64.vc_solve(tol, 4 * a.maxit))
            true = math.sqrt(s64.vc_residual(0, capi.ARR_U, capi.ARR_RHS) / bb)
            return dict(cycles=len(hist) - 1, true=true, wall=wall, ms=ms, reached=hist[-1] <= tol)

        def run_mixed(count):
            s32.mixed_set_solution(zero)
            (hist, st), wall, ms = timed(s32, lambda: s32.mixed_solve(tol, a.maxit, count, op=COEF))
            return dict(cycles=st.cycles, outer=st.outer, true=st.relres, wall=wall, ms=ms, reached=st.status == 0)

        runs = {"mg_vc_solve fp64": run64}
        for m in (1, 2, 4):
            runs[f"mixed vc, {m} cycles per corr."] = (lambda m=m: run_mixed(m))
        print(f"-- smooth factor-100 field, all faces Neumann, shift 10, tol {tol:g}")
        table(alternate(runs, a.repeats), "mg_vc_solve fp64")

    else:
        tol = 1e-8
        af = field_jump_aligned(a.n)
        for s, arr in ((s32, af.astype(np.float32)), (s64, af)):
            s.vc_set_coefficient(arr); s.vc_set_faces(ONLY_YHI_DIRICHLET)
        s32.mixed_set_rhs(b); s64.set_rhs(b)

        def run64():
            s64.set_solution(zero)
            (hist, st), wall, ms = timed(s64, lambda: s64.vc_pcg_solve(tol, 8 * a.maxit))
            return dict(cycles=st.iters, true=st.relres_true, wall=wall, ms=ms, reached=st.status == 0)

        def run_mixed():
            s32.mixed_set_solution(zero)
            (hist, st), wall, ms = timed(s32, lambda: s32.mixed_solve(tol, a.maxit, 8, op=COEF, inner_pcg=True))
            return dict(cycles=st.cycles, outer=st.outer, true=st.relres, wall=wall, ms=ms, reached=st.status == 0)

        print(f"-- aligned jump of 1000, only y-hi Dirichlet, tol {tol:g}; cycles = CG iterations")
        table(alternate({"mg_vc_pcg_solve fp64": run64, "mixed vc, 8 CG per corr.": run_mixed}, a.repeats), "mg_vc_pcg_solve fp64")

    b64, b32 = s64.device_bytes(), s32.device_bytes()
    print(f"mg_device_bytes: fp64 handle {b64 / 1e9:.3f} GB = {b64 / pts:.1f} B/node; MG_F32 handle with the fp64 outer arrays "
          f"{b32 / 1e9:.3f} GB = {b32 / pts:.1f} B/node")
    s64.close(); s32.close()


if __name__ == "__main__":
    main()
