"""fmgop_times -- what a face mask costs the level-0 FMG interpolation launch (mg_fmg_prolong with MG_FMG_OPERATOR, DESIGN.md
section 27): the streaming 3-D kernel with a mask against (a) its own mask-free launch of the same shape in the same run and
(b) the gather kernel with the same mask.

    python tools/fmgop_times.py                                  # 257^3 -> 513^3 fp64 and 513^3 -> 1025^3 fp32
    python tools/fmgop_times.py --n 513 --dtype f64 --reps 9
    python tools/fmgop_times.py --pass                           # instead: mg_fmg(1) on mg_bc_*'s operator against the unflagged mg_fmg(1), 513^3 fp64

Times come from HIP events on the handle's stream (mg_timer_*) around ONE launch, after a warm-up of every launch timed; each
figure is the median of --reps timings, the masks alternating inside a repetition. MG_FMG_FAST is read once per process, so the
two kernel forms run in a child process each (the same command with --inner). arr_bnd = RHS(0) in every launch. Compulsory
bytes: the fine array written once, the coarse array read once, the Dirichlet nodes of RHS(0) read.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MASKS = (0, 1, 55, 63)   # mask-free, x-lo, all but y-hi, every face


def inner(a):
    from multigrid_prj_amd import capi
    n = a.n
    T = np.float64 if a.dtype == "f64" else np.float32
    kw = dict(dim=3, n=n, levels=2, dtype=capi.MG_F64 if a.dtype == "f64" else capi.MG_F32, length=1.0, alpha=1.0, cycle=capi.CYCLE_V,
              smoother=capi.SMOOTH_JACOBI, omega=6.0 / 7.0, nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW, outer_pre_gs=0)
    nc = (n - 1) // 2 + 1
    t = np.linspace(0.0, 1.0, nc).astype(T)
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_array(capi.ARR_U, 1, np.cos(3 * t)[:, None, None] * np.sin(2 * t + 1)[None, :, None] * np.cos(t)[None, None, :])
        times = {m: [] for m in MASKS}
        for rep in range(a.reps + 1):   # the first repetition is the warm-up
            for m in MASKS:
                s.bc_set_faces(m)
                s.timer_start()
                if m == 0:
                    s.fmg_prolong(1, capi.ARR_U, capi.ARR_E, capi.ARR_RHS)
                else:
                    s.fmg_prolong(1, capi.ARR_U, capi.ARR_E, capi.ARR_RHS, op=capi.FMG_ON_FACES)
                ms = s.timer_stop()
                if rep:
                    times[m].append(ms)
    print(json.dumps({str(m): [statistics.median(v), min(v)] for m, v in times.items()}))


def run_inner(a, n, dtype, fast):
    env = dict(os.environ)
    if not fast:
        env["MG_FMG_FAST"] = "0"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--inner", "--n", str(n), "--dtype", dtype, "--reps", str(a.reps)],
                       env=env, cwd=ROOT, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(p.stdout[-2000:] + p.stderr[-4000:])
    return {int(k): v for k, v in json.loads(p.stdout.strip().splitlines()[-1]).items()}


def whole_pass(a):
    from multigrid_prj_amd import capi
    n = 513
    kw = dict(dim=3, n=n, levels=6, dtype=capi.MG_F64, length=1.0, alpha=1.0, cycle=capi.CYCLE_V, smoother=capi.SMOOTH_JACOBI, omega=6.0 / 7.0,
              nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW, coarse_mode=capi.COARSE_TOL, coarse_maxit=2000, coarse_tol=0.1, outer_pre_gs=0)
    t = np.linspace(0.0, 1.0, n)
    b = np.cos(np.pi * t)[:, None, None] * np.sin(np.pi * t)[None, :, None] * np.cos(np.pi * t)[None, None, :]
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_rhs(b)
        s.bc_set_faces(55)
        rows = []
        for name, call in (("mg_fmg(1), constant operator (fused level kernels)", lambda: s.fmg(1)),
                           ("mg_fmg(1 | ON_FACES), all faces but y-hi Neumann", lambda: s.fmg(1, op=capi.FMG_ON_FACES))):
            call()
            out = []
            for _ in range(a.reps):
                s.timer_start(); st = call(); out.append(s.timer_stop())
            rows.append((name, statistics.median(out), st.relres, st.coarse_iters))
        s.set_solution(np.zeros_like(b))
        s.bc_cycle()
        out = []
        for _ in range(a.reps):
            s.timer_start(); s.bc_cycle(); out.append(s.timer_stop())
        print(f"# {n}^3 fp64, 6 levels, V(2,2) Jacobi 6/7, coarse to 0.1; medians of {a.reps}, device ms (the final residual included)")
        for name, ms, rr, ci in rows:
            print(f"{name:58s} {ms:9.3f} ms  relres {rr:.3e}  sweeps of the first coarse solve {ci}")
        print(f"{'one mg_bc_cycle (with its statistics fetch)':58s} {statistics.median(out):9.3f} ms")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--dtype", choices=["f64", "f32"], default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--pass", action="store_true", dest="whole_pass")
    a = ap.parse_args()
    if a.inner:
        return inner(a)
    if a.whole_pass:
        return whole_pass(a)
    shapes = [(a.n or 513, a.dtype or "f64")] if (a.n or a.dtype) else [(513, "f64"), (1025, "f32")]
    for n, dtype in shapes:
        es = 8 if dtype == "f64" else 4
        nc = (n - 1) // 2 + 1
        gb = (n ** 3 + nc ** 3 + (n ** 3 - (n - 2) ** 3)) * es / 1e9
        fast, gather = run_inner(a, n, dtype, True), run_inner(a, n, dtype, False)
        print(f"# level-0 interpolation {nc}^3 -> {n}^3 {dtype}, arr_bnd = RHS(0); compulsory {gb:.3f} GB; medians of {a.reps} (min), ms per launch")
        print(f"{'mask':>5s} {'streaming':>18s} {'TB/s':>6s} {'x mask 0':>9s} {'gather':>18s} {'streaming / gather':>19s}")
        for m in MASKS:
            f, g = fast[m], gather[m]
            print(f"{m:5d} {f[0]:9.3f} ({f[1]:6.3f}) {gb / f[0]:6.2f} {f[0] / fast[0][0]:9.3f} {g[0]:9.3f} ({g[1]:6.3f}) {f[0] / g[0]:19.3f}")


if __name__ == "__main__":
    main()
