"""heat_times -- the right-hand-side kernel of mg_heat_step (mg_heat.hip) against the saved residual of the same handle, and
a whole implicit step against the handle's cycle.

    python tools/heat_times.py                              # every part below
    python tools/heat_times.py --parts kernel64 step        # 513^3 fp64 kernel table, the step table
    python tools/heat_times.py --parts kernel32 --n32 513   # the fp32 kernel table on a smaller grid

Parts:
  kernel64 / kernel32   mg_heat_rhs in its four forms at --n64^3 fp64 / --n32^3 fp32 next to mg_residual with the residual
                        saved (arr_r = TMP; the norm's reduction launch included, as the entry point runs it): HIP events on
                        the handle's stream around --kreps back-to-back launches, --samples samples after a warm-up, median
                        (min .. max). Compulsory traffic: u read, f read when there is a source, rhs written; the residual
                        reads u and rhs and writes r. The general form with a source moves 4/3 of the residual's bytes; the
                        yardstick is time <= 1.15 x 4/3 x the residual's median.
  step                  --n64^3 fp64, --levels levels, V(2,2) Jacobi omega 6/7, full weighting, one cycle per step, backward
                        Euler and Crank-Nicolson: ms per step from the difference of a 40-step and a 20-step call (the one
                        residual + synchronisation at the end of a call drops out) next to mg_cycle_async's ms per cycle.
  check                 3 Crank-Nicolson steps of 2 cycles at --n64^3: the returned relres and mg_residual / mg_sumsq after.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0


def med(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:8.4f} ({v[0]:.4f} .. {v[-1]:.4f})"


def field(n, dtype, phase):
    """a smooth, cheap-to-build n^3 field (the kernels' time does not depend on the values)"""
    x = np.linspace(0.0, 1.0, n)
    a, b, c = np.sin(3 * x + phase), np.cos(5 * x - phase), np.sin(7 * x + 2 * phase)
    return (a[:, None, None] * b[None, :, None] + c[None, None, :]).astype(dtype)


def sample(s, fn, kreps, samples):
    fn(); s.sync()
    out = []
    for _ in range(samples):
        s.timer_start()
        for _k in range(kreps):
            fn()
        out.append(s.timer_stop() / kreps)
    return out


def kernel_table(capi, n, dtype, a):
    es = 8 if dtype == capi.MG_F64 else 4
    name = "fp64" if es == 8 else "fp32"
    pts = n ** 3
    kw = dict(dim=3, n=n, levels=2, length=1.0, alpha=1.0, dtype=dtype)
    npdt = np.float64 if es == 8 else np.float32
    print(f"# kernel, {n}^3 {name}: {a.kreps} back-to-back launches per sample, {a.samples} samples after a warm-up; ms per launch, "
          f"median (min .. max)", flush=True)
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_array(capi.ARR_U, 0, field(n, npdt, 0.3))
        s.set_array(capi.ARR_RHS, 0, field(n, npdt, 1.1))
        dt = 1e-3
        rows = []
        res = sample(s, lambda: s.residual_async(0, capi.ARR_U, capi.ARR_RHS, capi.ARR_TMP), a.kreps, a.samples)
        rows.append(("mg_residual, r saved (yardstick)", res, 3 * es))
        for src in (True, False):
            s.heat_set_source(field(n, npdt, 2.0) if src else None)
            for theta, form in ((0.5, "general"), (1.0, "stencil-free")):
                t = sample(s, lambda: s.heat_rhs(dt, theta, capi.ARR_U, capi.ARR_RES), a.kreps, a.samples)
                rows.append((f"mg_heat_rhs {form}, {'source' if src else 'no source'}", t, (3 if src else 2) * es))
        res2 = sample(s, lambda: s.residual_async(0, capi.ARR_U, capi.ARR_RHS, capi.ARR_TMP), a.kreps, a.samples)
        rows.append(("mg_residual, r saved (again, after)", res2, 3 * es))
        for label, t, bpp in rows:
            gb = bpp * pts / 1e9
            print(f"{label:40s} {spread(t)} ms  {bpp:2d} B/node = {gb:6.3f} GB -> {gb / med(t):5.2f} TB/s = {gb / med(t) / PEAK_TBS:5.1%} of "
                  f"{PEAK_TBS:g} TB/s", flush=True)
        yard = 1.15 * (4.0 / 3.0) * med(res)
        got = med(rows[1][1])
        print(f"target: general form with source <= 1.15 x 4/3 x residual = {yard:.4f} ms; measured {got:.4f} ms = "
              f"{got / (4.0 / 3.0 * med(res)):.3f} x (4/3 x residual): {'MET' if got <= yard else 'MISSED'}", flush=True)


def step_kw(capi, n, levels):
    return dict(dim=3, n=n, levels=levels, length=1.0, alpha=1.0, cycle=capi.CYCLE_V, smoother=capi.SMOOTH_JACOBI, omega=6.0 / 7.0,
                nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW, coarse_mode=capi.COARSE_TOL, coarse_maxit=2000, coarse_tol=0.1,
                outer_pre_gs=0)


def step_table(capi, a):
    n = a.n64
    print(f"# step, {n}^3 fp64, {a.levels} levels, V(2,2) Jacobi omega 6/7, full weighting, one cycle per step, with a source; "
          f"ms per step = (40-step call - 20-step call) / 20, {a.samples} samples; mg_cycle_async: 20 cycles per sample", flush=True)
    with capi.Solver(capi.make_desc(**step_kw(capi, n, a.levels))) as s:
        u0 = field(n, np.float64, 0.3)
        s.heat_set_source(field(n, np.float64, 2.0))
        s.set_solution(u0)
        dt = 1e-4
        for theta, label in ((1.0, "backward Euler"), (0.5, "Crank-Nicolson")):
            s.heat_step(dt, theta, 2, 1)
            per, k20 = [], []
            for _ in range(a.samples):
                s.timer_start(); s.heat_step(dt, theta, 20, 1); t20 = s.timer_stop()
                s.timer_start(); s.heat_step(dt, theta, 40, 1); t40 = s.timer_stop()
                per.append((t40 - t20) / 20); k20.append(t20 / 20)
            s.cycle_async(2); s.sync()
            cyc = []
            for _ in range(a.samples):
                s.timer_start(); s.cycle_async(20); cyc.append(s.timer_stop() / 20)
            ker = sample(s, lambda: s.heat_rhs(dt, theta, capi.ARR_U, capi.ARR_RES), a.kreps, a.samples)
            extra = med(per) - med(cyc)
            print(f"{label:15s} step {spread(per)} ms (20-step call / 20, tail included: {med(k20):.4f}); cycle {spread(cyc)} ms; "
                  f"assembly kernel alone {spread(ker)} ms; step - cycle = {extra:.4f} ms = {extra / med(ker):.3f} x the kernel", flush=True)


def check(capi, a):
    n = a.n64
    with capi.Solver(capi.make_desc(**step_kw(capi, n, a.levels))) as s:
        s.heat_set_source(field(n, np.float64, 2.0))
        s.set_solution(field(n, np.float64, 0.3))
        st = s.heat_step(1e-4, 0.5, 3, 2)
        rr = s.residual(0, capi.ARR_U, capi.ARR_RHS, -1)
        bb = s.sumsq(0, capi.ARR_RHS)
        after = math.sqrt(rr / bb)
        print(f"# check, {n}^3 fp64: 3 Crank-Nicolson steps of 2 cycles: steps {st.steps} cycles {st.cycles} time {st.time:g} relres "
              f"{st.relres:.6e}; mg_residual / mg_sumsq afterwards {after:.6e}; relative difference {abs(after - st.relres) / after:.2e} "
              f"({'agree' if abs(after - st.relres) <= 1e-12 * after else 'DISAGREE'} to rtol 1e-12); shift {s.get_shift():g}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parts", nargs="+", default=["kernel64", "kernel32", "step", "check"], choices=["kernel64", "kernel32", "step", "check"])
    ap.add_argument("--n64", type=int, default=513)
    ap.add_argument("--n32", type=int, default=1025)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--kreps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=9)
    a = ap.parse_args()
    from multigrid_prj_amd import capi
    if "kernel64" in a.parts:
        kernel_table(capi, a.n64, capi.MG_F64, a)
    if "kernel32" in a.parts:
        kernel_table(capi, a.n32, capi.MG_F32, a)
    if "step" in a.parts:
        step_table(capi, a)
    if "check" in a.parts:
        check(capi, a)


if __name__ == "__main__":
    main()
