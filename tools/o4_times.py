"""o4_times -- the fourth-order defect correction (mg_o4_*) measured on one handle per configuration, in one process:

 1. mg_o4_residual (saving) against mg_residual (saving): both move 24 B per fp64 node, so the second-order kernel is the
    yardstick for the radius-2 tile;
 2. mg_o4_correct_residual (40 B per fp64 node) against mg_correct + mg_o4_residual, the two passes it replaces;
 3. mg_o4_solve from mg_fmg's iterate and from zero, inner_cycles 1 and 2: the corrections and the milliseconds until the
    error against a manufactured solution stops falling (within 5 % of the smallest error seen in --maxcorr corrections),
    next to mg_solve to 1e-10 on the same right-hand side and its (second-order) error.

    python tools/o4_times.py                 # 257^3 and 513^3 fp64, 513^3 fp32, 2049^2 fp64
    python tools/o4_times.py --only 3d257f64

Kernels: HIP events on the handle's stream around --kreps back-to-back launches (no norm fetched), the two sides of a
comparison alternating --repeats times; median (min .. max). Solves: host wall clock around the call, which ends in a
device synchronisation. V(2,2) Jacobi omega 6/7, full weighting, coarse solve to 0.1 -- the benchmark's cycle. The
manufactured solution is sin(2.3x + 0.4) exp(1.1y) cos(1.7z - 0.2) + xyz on the unit cube, evaluated in fp64; errors are
max norms taken on the device (torch), so the arrays never cross to the host.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0
CONFIGS = {
    "3d257f64": dict(dim=3, n=257, levels=6, f32=False),
    "3d513f64": dict(dim=3, n=513, levels=7, f32=False),
    "3d513f32": dict(dim=3, n=513, levels=7, f32=True),
    "2d2049f64": dict(dim=2, n=2049, levels=9, f32=False),
}


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def spread(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:8.3f} ({v[0]:.3f} .. {v[-1]:.3f})"


def manufactured(dim, n):
    """(u*, b) in fp64: b = -Laplace u* inside, u* on the Dirichlet nodes"""
    t = np.arange(n, dtype=np.float64) / (n - 1)
    sx, ey = np.sin(2.3 * t + 0.4), np.exp(1.1 * t)
    if dim == 3:
        cz = np.cos(1.7 * t - 0.2)
        P = cz[:, None, None] * ey[None, :, None] * sx[None, None, :]
        u = P + t[:, None, None] * t[None, :, None] * t[None, None, :]
        f = (2.3 ** 2 - 1.1 ** 2 + 1.7 ** 2) * P
        I = (slice(1, -1),) * 3
    else:
        P = np.cos(-0.2) * ey[:, None] * sx[None, :]
        u = P.copy()
        f = (2.3 ** 2 - 1.1 ** 2) * P
        I = (slice(1, -1),) * 2
    b = u.copy()
    b[I] = f[I]
    return u, b


def run(name, cfg, a):
    import torch
    from multigrid_prj_amd import capi
    dim, n = cfg["dim"], cfg["n"]
    dtype = capi.MG_F32 if cfg["f32"] else capi.MG_F64
    es = 4 if cfg["f32"] else 8
    kw = dict(dim=dim, n=n, levels=cfg["levels"], length=1.0, alpha=1.0, dtype=dtype, cycle=capi.CYCLE_V, smoother=capi.SMOOTH_JACOBI,
              omega=6.0 / 7.0, nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW, coarse_mode=capi.COARSE_TOL, coarse_maxit=2000,
              coarse_tol=0.1, outer_pre_gs=0)
    pts = n ** dim
    print(f"\n## {name}: {dim}-D n = {n}, {cfg['levels']} levels, {'fp32' if cfg['f32'] else 'fp64'}, V(2,2) Jacobi omega 6/7, FW, coarse to 0.1",
          flush=True)
    ustar, b = manufactured(dim, n)
    s = capi.Solver(capi.make_desc(**kw))
    U, E, RHS, TMP, RES = capi.ARR_U, capi.ARR_E, capi.ARR_RHS, capi.ARR_TMP, capi.ARR_RES
    tdt = torch.float32 if cfg["f32"] else torch.float64
    ustar_d = torch.from_numpy(ustar).to("cuda")
    b_d = torch.from_numpy(b).to("cuda", dtype=tdt)
    zero_d = torch.zeros_like(b_d)
    out_d = torch.empty_like(b_d)
    torch.cuda.synchronize()
    s.set_rhs_device(b_d); s.set_solution_device(zero_d); s.sync()
    bytes0 = s.device_bytes()

    def error():
        s.get_solution_device(out_d); s.sync(); torch.cuda.synchronize()
        return float((out_d.to(torch.float64) - ustar_d).abs().max().item())

    # ---- 1, 2: the kernels
    def k_events(fn):
        s.sync(); s.timer_start()
        for _ in range(a.kreps):
            fn()
        return s.timer_stop() / a.kreps

    lib, h = s.lib, s.h
    o4r = lambda: lib.mg_o4_residual(h, U, RHS, RES, None)
    a2r = lambda: s.residual_async(0, U, RHS, RES)
    o4cr = lambda: lib.mg_o4_correct_residual(h, U, E, RHS, TMP, RES, None)
    two = lambda: (s.correct(U, E), lib.mg_o4_residual(h, U, RHS, RES, None))
    for fn in (o4r, a2r, o4cr, two):
        fn()
    t = {k: [] for k in ("o4r", "a2r", "o4cr", "two")}
    for _ in range(a.repeats):
        t["a2r"].append(k_events(a2r)); t["o4r"].append(k_events(o4r))
        t["two"].append(k_events(two)); t["o4cr"].append(k_events(o4cr))
    gb_r, gb_c = 3 * es * pts / 1e9, 5 * es * pts / 1e9
    for key, label, gb in (("a2r", "mg_residual (saving)", gb_r), ("o4r", "mg_o4_residual (saving)", gb_r),
                           ("two", "mg_correct + mg_o4_residual", 2 * gb_r), ("o4cr", "mg_o4_correct_residual", gb_c)):
        m = med(t[key])
        print(f"{label:30s} {spread(t[key])} ms; {gb:.3f} GB compulsory -> {gb / m:.2f} TB/s, frac {gb / m / PEAK_TBS:.3f} of {PEAK_TBS:g} TB/s")
    print(f"ratio 1: mg_o4_residual / mg_residual = {med(t['o4r']) / med(t['a2r']):.3f}")
    print(f"ratio 2: mg_o4_correct_residual / (mg_correct + mg_o4_residual) = {med(t['o4cr']) / med(t['two']):.3f}", flush=True)

    # ---- 3: the solves
    def start(from_fmg):
        s.set_rhs_device(b_d); s.set_solution_device(zero_d)
        if from_fmg:
            s.fmg(1)

    def timed(fn):
        s.sync(); t0 = time.perf_counter()
        out = fn()
        return out, (time.perf_counter() - t0) * 1e3

    start(False)
    (h2, _), _ = timed(lambda: s.solve(1e-10, 100))   # warm-up
    w2 = []
    for _ in range(a.repeats):
        start(False)
        (h2, _), w = timed(lambda: s.solve(1e-10, 100)); w2.append(w)
    e2 = error()
    print(f"mg_solve to 1e-10 from zero: {len(h2) - 1} cycles, relres {h2[-1]:.2e}, wall {spread(w2)} ms, error {e2:.3e} (second order)")
    for from_fmg in (True, False):
        for inner in (1, 2):
            # the error after each correction: one correction per call, warm-started (the iterates are those of one long call)
            start(from_fmg)
            errs, rel = [error()], []
            for _ in range(a.maxcorr):
                hist, st = s.o4_solve(0.0, 1, inner)
                rel.append(hist[-1]); errs.append(error())
                if st.status == 2:
                    break
            lim = min(errs)
            need = next(k for k, e in enumerate(errs) if e <= 1.05 * lim)
            start(from_fmg); s.o4_solve(0.0, max(need, 1), inner)   # warm-up
            ws = []
            for _ in range(a.repeats):
                start(False)
                _, w = timed(lambda: ((s.fmg(1) if from_fmg else None), s.o4_solve(0.0, need, inner)))
                ws.append(w)
            print(f"mg_o4_solve from {'mg_fmg' if from_fmg else 'zero  '} inner_cycles {inner}: {need:2d} corrections ({need * inner} cycles) until the error "
                  f"is within 5 % of its limit {lim:.3e} (second order / fourth order = {e2 / lim:.0f}); wall {spread(ws)} ms"
                  f"{' incl. mg_fmg' if from_fmg else ''}; / mg_solve = {med(ws) / med(w2):.2f}")
            print("    error by correction: " + " ".join(f"{e:.2e}" for e in errs[:need + 3]))
            print("    relres by correction: " + " ".join(f"{r:.2e}" for r in rel[:need + 3]), flush=True)
    print(f"mg_device_bytes: {bytes0 / 1e9:.3f} GB before the first mg_o4_solve, {s.device_bytes() / 1e9:.3f} GB after "
          f"(+{(s.device_bytes() - bytes0) / pts:.1f} B/node)")
    s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--maxcorr", type=int, default=14)
    a = ap.parse_args()
    print(f"# o4_times: {a.repeats} alternating repeats, {a.kreps} back-to-back launches per kernel timing, at most {a.maxcorr} corrections")
    for name in a.only:
        run(name, CONFIGS[name], a)


if __name__ == "__main__":
    main()
