"""eigop_times -- what an operator family (MG_EIG_OPERATOR) costs mg_eig_solve: the Gram + apply launches, one whole mg_eig_solve iteration and its split
into preconditioning cycles and block kernels, for MG_EIG_ON_FACES and MG_EIG_ON_COEFFICIENT against MG_EIG_ON_CONSTANT in
the same run (modelled on tools/eig_times.py, whose conventions it keeps).

    python tools/eigop_times.py                     # 513^3 fp64, 6 levels, V(2,2) Jacobi omega 6/7, m = 4, all faces Neumann, shift 10
    python tools/eigop_times.py --dtype f32
    python tools/eigop_times.py --n 129 --levels 4

Times come from HIP events on the handle's stream (mg_timer_*), after a warm-up of everything that is timed; each figure is
the median of --repeat timings. The solve is timed at a tolerance it cannot meet, so it runs exactly --iters iterations
with every column active; a solve with maxit = 0 (start-up and exit only) is timed separately and subtracted. The cycles are
timed the way the solve's preconditioner runs them: m times a zeroing of U(0) and ONE cycle of the family from that zero
(mg_cycle_async / mg_bc_cycle / mg_vc_cycle; the last two also fetch their statistics, a host synchronisation per cycle that the
solve does not have). "block" is the iteration less those. Every face of the box is Neumann for
the two families -- every mirror select is live -- and the shift keeps the operator regular. Bytes are counted in passes
over one level-0 array, the stencil's neighbour reads not counted: with m = 4 the apply launch (rows X, W against the W
columns) reads 2m + m arrays and writes m, and the coefficient family reads a once more.
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(s, fn, repeat, setup=None):
    out = []
    for _ in range(repeat):
        if setup:
            setup()
        s.timer_start()
        fn()
        out.append(s.timer_stop())
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=513)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--shift", type=float, default=10.0)
    a = ap.parse_args()
    import torch
    from multigrid_prj_amd import capi
    m, n = a.m, a.n
    kw = dict(dim=3, n=n, levels=a.levels, dtype=capi.MG_F64 if a.dtype == "f64" else capi.MG_F32, length=1.0, alpha=1.0,
              cycle=capi.CYCLE_V, smoother=capi.SMOOTH_JACOBI, omega=6.0 / 7.0, nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW,
              coarse_mode=capi.COARSE_TOL, coarse_maxit=2000, coarse_tol=0.1, outer_pre_gs=0)
    es = 8 if a.dtype == "f64" else 4
    gb = n ** 3 * es / 1e9
    print(f"# 3-D {n}^3 {a.dtype}, {a.levels} levels, V(2,2) Jacobi omega 6/7, full weighting; m = {m}, all columns active, all faces "
          f"Neumann, shift {a.shift:g}; one level-0 array = {gb:.3f} GB; medians of {a.repeat}", flush=True)
    tdt = torch.float64 if a.dtype == "f64" else torch.float32
    x0 = [torch.rand((n,) * 3, dtype=tdt, device="cuda") for _ in range(m)]
    t = torch.linspace(0.0, 1.0, n, dtype=torch.float64, device="cuda")
    coef = torch.exp(math.log(10.0) * torch.sin(2 * math.pi * t)[None, None, :] * torch.cos(2 * math.pi * t)[None, :, None]
                     * torch.cos(math.pi * t)[:, None, None]).to(tdt).contiguous()   # vc_ref.field_smooth: a factor of 100
    torch.cuda.synchronize()
    tiny = 1e-300
    rows = {}
    with capi.Solver(capi.make_desc(**kw)) as s:
        s.set_shift(a.shift)
        s.bc_set_faces(63)
        s.vc_set_faces(63)
        s.vc_set_coefficient_device(coef)
        s.sync()

        def restart():
            for j in range(m):
                s.eig_set_vector_device(capi.EIG_X, j, x0[j])
            s.sync()

        def cycles_of(op):   # as Solver::precondition: per column a zeroed start and one cycle from it
            for _ in range(m):
                s.zero_array(capi.ARR_U, 0)
                if op == capi.EIG_ON_CONSTANT:
                    s.cycle_async(1)
                else:
                    (s.bc_cycle if op == capi.EIG_ON_FACES else s.vc_cycle)()

        for name, op in (("constant", capi.EIG_ON_CONSTANT), ("faces", capi.EIG_ON_FACES), ("coefficient", capi.EIG_ON_COEFFICIENT)):
            s.eig_set_operator(op)
            restart()
            s.eig_solve(m, m, tol=tiny, maxit=2)                     # warm-up: every kernel of the solve
            cycles_of(op); s.sync()
            t_edge = timed(s, lambda: s.eig_solve(m, m, tol=tiny, maxit=0), a.repeat, restart)
            t_solve = timed(s, lambda: s.eig_solve(m, m, tol=tiny, maxit=a.iters), a.repeat, restart)
            restart()
            lam, rel, hist, st = s.eig_solve(m, m, tol=tiny, maxit=a.iters)
            assert st.iters == a.iters and st.cycles == a.iters * m, (st.iters, st.cycles, st.status)
            t_iter = (t_solve - t_edge) / a.iters
            t_cyc = timed(s, lambda: cycles_of(op), a.repeat)
            s.eig_kernel_gram(m, m); s.eig_kernel_gram(m, 0)
            t_gram_w = timed(s, lambda: s.eig_kernel_gram(m, 0), a.repeat)      # X columns (read AX) + the W columns with the apply
            t_gram_full = timed(s, lambda: s.eig_kernel_gram(m, m), a.repeat)   # + the P columns
            cx = np.vstack([np.eye(m), 1e-3 * np.ones((2 * m, m))]); cp = 1e-3 * np.ones((2 * m, m)) + np.vstack([np.eye(m), np.eye(m)])
            s.eig_kernel_combine(m, m, cx, cp, np.ones(m))
            t_comb = timed(s, lambda: s.eig_kernel_combine(m, m, cx, cp, np.ones(m)), a.repeat)
            rows[name] = dict(gram_w=t_gram_w, gram_full=t_gram_full, comb=t_comb, iter=t_iter, cyc=t_cyc, block=t_iter - t_cyc, lam0=lam[0])
        s.eig_set_operator(capi.EIG_ON_CONSTANT)

    tiles = -(-m // 4)
    p_w = tiles * (2 * m) + m + tiles * m + m            # eig_times.py's count of the np = 0 entry: the X tile and the W tile with the apply
    p_apply = tiles * (2 * m) + m + m                    # the apply launch alone: rows X, W; b read, A b written
    print(f"counted passes of the apply launch: constant / faces {p_apply} (reads {p_apply - m}), coefficient {p_apply + 1} (reads {p_apply - m + 1})")
    print(f"{'operator':12s} {'Gram+apply np=0':>16s} {'Gram+apply all':>15s} {'combine':>9s} {'iteration':>10s} {'= cycles':>9s} {'+ block':>9s}   ms")
    for name, r in rows.items():
        print(f"{name:12s} {r['gram_w']:16.3f} {r['gram_full']:15.3f} {r['comb']:9.3f} {r['iter']:10.2f} {r['cyc']:9.2f} {r['block']:9.2f}")
    c = rows["constant"]
    for name in ("faces", "coefficient"):
        r = rows[name]
        print(f"{name:12s} {r['gram_w'] / c['gram_w']:16.2f} {r['gram_full'] / c['gram_full']:15.2f} {r['comb'] / c['comb']:9.2f} {r['iter'] / c['iter']:10.2f} "
              f"{r['cyc'] / c['cyc']:9.2f} {r['block'] / c['block']:9.2f}   x constant")
    print(f"Gram + apply, np = 0, counted bytes: constant {p_w * gb / c['gram_w']:.2f} TB/s, faces {p_w * gb / rows['faces']['gram_w']:.2f} TB/s, "
          f"coefficient {(p_w + 1) * gb / rows['coefficient']['gram_w']:.2f} TB/s")
    print("lowest Ritz value after the timed iterations: " + ", ".join(f"{k} {v['lam0']:.6g}" for k, v in rows.items()))


if __name__ == "__main__":
    main()
