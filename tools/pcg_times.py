"""pcg_times -- mg_solve against mg_pcg_solve on one configuration (iterations and device time to `tol`), and the
per-iteration cost of the three vector kernels of the flexible CG loop.

    python tools/pcg_times.py --case headline                 # 513^3 fp64, 6 levels, Jacobi V(2,2) omega 6/7, FW, tol coarse
    python tools/pcg_times.py --case config1                  # BASELINE config 1: 257^2, 3 levels, sawtooth, -smt 1 defaults
    python tools/pcg_times.py --case config5 --smoother rbgs  # eps = 0.01 in z, 3 semi-coarsenings, 8 levels
    python tools/pcg_times.py --case aniso-std                # eps = 0.01 in z on standard coarsening
    python tools/pcg_times.py --parse-stats X_kernel_stats.csv --n 513 --dim 3 --dtype f64

Times come from HIP events on the handle's stream (mg_timer_*), after one warm-up solve of each kind. Kernel times come
from a separate `rocprofv3 --kernel-trace --stats` run of the same command: --parse-stats reads its kernel_stats.csv
and prints each new kernel's average time, its compulsory bytes (table in DESIGN.md) and their rate as a fraction of
the 8 TB/s HBM peak.
"""
from __future__ import annotations

import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0
# compulsory passes over one level-0 array (reads + writes) per launch
KERNELS = {"k_cg_update": 6, "k_cg_dots": 3, "k_cg_direction_apply": 4}

SMOOTHERS = {"gs": 0, "jacobi": 1, "rbgs": 2, "zebra": 3, "zebrax": 4}


def case_desc(a):
    from multigrid_prj_amd import capi
    sm = SMOOTHERS[a.smoother] if a.smoother else None
    if a.case == "config1":   # Multigrid -n 257 -a 1 -w 10 -ml 3 -test 1 -smt 1
        kw = dict(dim=2, n=257, levels=3, length=10.0, alpha=1.0, smoother=capi.SMOOTH_JACOBI)
        return kw, "2-D 257^2, 3 levels, sawtooth, Jacobi, 2 GS pre-sweeps, coarse to 0.1 (BASELINE config 1)"
    kw = dict(dim=3, n=a.n or 513, levels=6, dtype=capi.MG_F64 if a.dtype == "f64" else capi.MG_F32, length=1.0, alpha=1.0,
              cycle=capi.CYCLE_V, smoother=capi.SMOOTH_JACOBI, nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW,
              coarse_mode=capi.COARSE_TOL, coarse_maxit=2000, coarse_tol=0.1, outer_pre_gs=0)
    if a.case == "config5":
        kw.update(levels=8, aniso=(1.0, 1.0, 0.01), semi_xy=3)
    elif a.case == "aniso-std":
        kw.update(aniso=(1.0, 1.0, 0.01))
    if sm is not None:
        kw["smoother"] = sm
    kw["omega"] = a.omega if a.omega is not None else (6.0 / 7.0 if kw["smoother"] == capi.SMOOTH_JACOBI else 1.0)
    name = {v: k for k, v in SMOOTHERS.items()}[kw["smoother"]]
    what = (f"3-D {kw['n']}^3 {a.dtype}, {kw['levels']} levels, V(2,2) {name} omega={kw['omega']:.4g}, full weighting, "
            f"coarse to 0.1, aniso={kw.get('aniso', (1.0, 1.0, 1.0))}, semi_xy={kw.get('semi_xy', 0)}")
    return kw, what


def rhs_for(kw, seed=0):
    from oracle import pyoracle as po
    if kw["dim"] == 2:
        return po.fill_rhs_2d(kw["n"], kw["length"], 1)
    n = kw["n"]
    b = np.zeros((n, n, n), np.float64 if kw.get("dtype", 0) == 0 else np.float32)
    rng = np.random.default_rng(seed)
    for k in range(1, n - 1):   # random interior, zero boundary; plane by plane to bound host memory
        b[k, 1:-1, 1:-1] = rng.standard_normal((n - 2, n - 2))
    return b


def run(a):
    from multigrid_prj_amd import capi
    kw, what = case_desc(a)
    b = rhs_for(kw)
    tol = a.tol if a.tol is not None else (1e-6 if a.case == "config1" else 1e-8)
    print(f"# {what}; tol {tol:g}", flush=True)
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_rhs(b)
        zero = np.zeros_like(b)
        # warm-up: every kernel of both solvers once
        s.set_solution(zero); s.solve(tol, 2)
        s.set_solution(zero); s.pcg_solve(tol, 2)
        s.set_solution(zero)
        t0 = time.perf_counter(); s.timer_start()
        hmg, _ = s.solve(tol, a.maxit)
        ms_mg = s.timer_stop(); wall_mg = (time.perf_counter() - t0) * 1e3
        cyc = len(hmg) - 1
        true_mg = np.sqrt(s.residual(0, capi.ARR_U, capi.ARR_RHS) / s.sumsq(0, capi.ARR_RHS))
        s.set_solution(zero)
        t0 = time.perf_counter(); s.timer_start()
        hp, st = s.pcg_solve(tol, a.maxit)
        ms_p = s.timer_stop(); wall_p = (time.perf_counter() - t0) * 1e3
    ok_mg = hmg[-1] <= tol
    print(f"mg_solve     : {cyc:4d} cycles     {'reached' if ok_mg else 'NOT reached'} tol (last {hmg[-1]:.3e}, true {true_mg:.3e})  "
          f"{ms_mg:9.2f} ms device  {wall_mg:9.2f} ms host  {ms_mg / max(cyc, 1):7.3f} ms/cycle", flush=True)
    status = {0: "converged", 1: "hit maxit", 2: "breakdown"}[st.status]
    print(f"mg_pcg_solve : {st.iters:4d} iterations {status} (last {st.relres:.3e}, true {st.relres_true:.3e})  "
          f"{ms_p:9.2f} ms device  {wall_p:9.2f} ms host  {ms_p / max(st.iters, 1):7.3f} ms/iteration", flush=True)
    if ok_mg and st.status == 0:
        print(f"pcg / mg_solve wall time to tol: {ms_p / ms_mg:.3f}  ({'PCG wins' if ms_p < ms_mg else 'PCG loses'})")
    elif st.status == 0:
        print(f"only PCG reached tol (mg_solve stopped at {a.maxit} cycles)")
    print("hist_mg  " + " ".join(f"{v:.3e}" for v in hmg))
    print("hist_pcg " + " ".join(f"{v:.3e}" for v in hp))


def parse_stats(a):
    """rocprofv3 --stats kernel_stats.csv -> per-launch time and HBM fraction of the three CG kernels"""
    n, dim = a.n, a.dim
    es = 8 if a.dtype == "f64" else 4
    pts = n ** dim
    with open(a.parse_stats) as f:
        rows = list(csv.DictReader(f))
    print(f"# level 0: {n}^{dim} {a.dtype} = {pts * es / 1e9:.3f} GB per array; peak {PEAK_TBS} TB/s")
    print(f"{'kernel':24s} {'calls':>6s} {'avg us':>9s} {'bytes GB':>9s} {'TB/s':>6s} {'of peak':>7s}")
    tot = 0.0
    for k, passes in KERNELS.items():
        sel = [r for r in rows if k in r["Name"]]
        if not sel:
            print(f"{k:24s} (not in the trace)")
            continue
        calls = sum(int(r["Calls"]) for r in sel)
        tot_ns = sum(float(r["TotalDurationNs"]) for r in sel)
        avg_us = tot_ns / calls / 1e3
        gb = passes * pts * es / 1e9
        tbs = gb / (avg_us * 1e-6) / 1e3
        tot += avg_us
        print(f"{k:24s} {calls:6d} {avg_us:9.1f} {gb:9.3f} {tbs:6.2f} {tbs / PEAK_TBS:7.1%}")
    tails = [r for r in rows if "k_cg_tail" in r["Name"]]
    if tails:
        c = sum(int(r["Calls"]) for r in tails)
        print(f"{'k_cg_tail':24s} {c:6d} {sum(float(r['TotalDurationNs']) for r in tails) / c / 1e3:9.1f}")
    print(f"three streaming kernels per iteration: {tot / 1e3:.3f} ms")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", choices=["headline", "config1", "config5", "aniso-std"], default="headline")
    ap.add_argument("--smoother", choices=list(SMOOTHERS), default=None)
    ap.add_argument("--omega", type=float, default=None)
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--tol", type=float, default=None)
    ap.add_argument("--maxit", type=int, default=300)
    ap.add_argument("--parse-stats", default=None)
    a = ap.parse_args()
    if a.parse_stats:
        a.n = a.n or 513
        parse_stats(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
