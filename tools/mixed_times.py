"""mixed_times -- the fp64 handle's mg_solve against mg_mixed_solve (fp64 defect correction over fp32 cycles) on one
configuration: wall time from the first launch to the last synchronisation, to the same true fp64 residual.

    python tools/mixed_times.py                       # 513^3, 6 levels, Jacobi V(2,2) omega 6/7, FW, coarse to 0.1, tol 1e-9
    python tools/mixed_times.py --n 257 --levels 5 --tol 1e-10 --repeats 7
    python tools/mixed_times.py --inner 1 2 4 6 8

The right-hand side is the benchmark's (bench.py: hash_rhs), the first guess zero. Every solver is warmed up once, then
the timed solves alternate between the solvers `--repeats` times; the table gives the median and the spread (min .. max)
of the host wall clock around the call (the calls end in a device synchronisation) and the HIP-event time on the
handle's stream. The fp32 cycle and the fused correction launch are timed apart on the same handle (HIP events around
`--kreps` back-to-back launches); the correction's compulsory traffic is 32 B per node (u64 and b64 read, e32 read, u64 and
r32 written) and its rate is given against the 8 TB/s HBM peak and the streaming rate the project's own calibration
reaches (profiles/r01_kbench_stream_calibration.log).
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


def timed(s, fn):
    t0 = time.perf_counter(); s.timer_start()
    out = fn()
    ms = s.timer_stop(); wall = (time.perf_counter() - t0) * 1e3
    return out, wall, ms


def spread(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:9.2f} ({v[0]:.2f} .. {v[-1]:.2f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=513)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--tol", type=float, default=1e-9)
    ap.add_argument("--maxit", type=int, default=60)
    ap.add_argument("--inner", type=int, nargs="+", default=[1, 2, 4, 6])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=10)
    a = ap.parse_args()

    from bench import hash_rhs
    from multigrid_prj_amd import capi
    kw = dict(dim=3, n=a.n, levels=a.levels, length=1.0, alpha=1.0, cycle=capi.CYCLE_V, smoother=capi.SMOOTH_JACOBI, omega=6.0 / 7.0,
              nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW, coarse_mode=capi.COARSE_TOL, coarse_maxit=2000, coarse_tol=0.1,
              outer_pre_gs=0)
    pts = a.n ** 3
    print(f"# 3-D {a.n}^3, {a.levels} levels, V(2,2) Jacobi omega=6/7, full weighting, coarse to 0.1; benchmark right-hand side, "
          f"zero first guess; tol {a.tol:g}; {a.repeats} alternating repeats after one warm-up of each solver", flush=True)
    b = hash_rhs(a.n, np.float64)
    zero = np.zeros_like(b)
    bb = float(np.sum(b.astype(np.longdouble) ** 2))

    s64 = capi.Solver(capi.make_desc(**kw))
    s32 = capi.Solver(capi.make_desc(**kw, dtype=capi.MG_F32))
    s64.set_rhs(b)
    s32.mixed_set_rhs(b)
    bytes64 = s64.device_bytes(); bytes32 = s32.device_bytes()

    def run64():
        s64.set_solution(zero)
        (hist, _), wall, ms = timed(s64, lambda: s64.solve(a.tol, a.maxit * max(a.inner)))
        true = np.sqrt(s64.residual(0, capi.ARR_U, capi.ARR_RHS) / bb)
        return dict(cycles=len(hist) - 1, last=hist[-1], true=true, wall=wall, ms=ms, reached=hist[-1] <= a.tol)

    def run_mixed(inner):
        s32.mixed_set_solution(zero)
        (hist, st), wall, ms = timed(s32, lambda: s32.mixed_solve(a.tol, a.maxit, inner))
        return dict(cycles=st.cycles, outer=st.outer, last=st.relres, true=st.relres, wall=wall, ms=ms, reached=st.status == 0, hist=hist)

    runs = {"mg_solve fp64": run64}
    for m in a.inner:
        runs[f"mixed, {m} per corr."] = (lambda m=m: run_mixed(m))
    for fn in runs.values():   # warm-up: every kernel of every solver once
        fn()
    res = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, fn in runs.items():
            res[k].append(fn())
    print(f"{'solver':22s} {'cycles':>6s} {'corr.':>5s} {'true relres':>11s} {'reached':>7s}  {'host wall ms: median (min .. max)':>36s}  "
          f"{'device ms: median (min .. max)':>34s} {'ms/cycle':>8s}")
    for k, rs in res.items():
        r = rs[0]
        assert all(x["cycles"] == r["cycles"] and x["true"] == r["true"] for x in rs), "runs of one solver differ"
        med = sorted(x["wall"] for x in rs)[len(rs) // 2]
        print(f"{k:22s} {r['cycles']:6d} {r.get('outer', 0):5d} {r['true']:11.3e} {str(bool(r['reached'])):>7s}  {spread([x['wall'] for x in rs]):>36s}  "
              f"{spread([x['ms'] for x in rs]):>34s} {med / max(r['cycles'], 1):8.3f}", flush=True)
    base = sorted(x["wall"] for x in res["mg_solve fp64"])
    for k, rs in res.items():
        if k == "mg_solve fp64":
            continue
        w = sorted(x["wall"] for x in rs)
        verdict = "faster beyond the spread" if w[-1] < base[0] else ("slower beyond the spread" if w[0] > base[-1] else "within the spread")
        print(f"{k:22s} median wall / fp64 median wall = {w[len(w) // 2] / base[len(base) // 2]:.3f}  ({verdict}: "
              f"mixed {w[0]:.2f} .. {w[-1]:.2f} ms, fp64 {base[0]:.2f} .. {base[-1]:.2f} ms)")
    for k, rs in res.items():
        if "hist" in rs[0]:
            print(f"hist {k:20s} " + " ".join(f"{v:.2e}" for v in rs[0]["hist"]))

    # the pieces: one fp32 cycle, one fp64 cycle, the fused correction launch
    s32.sync(); s32.timer_start(); s32.cycle_async(a.kreps); ms_c32 = s32.timer_stop() / a.kreps
    s64.sync(); s64.timer_start(); s64.cycle_async(a.kreps); ms_c64 = s64.timer_stop() / a.kreps
    s32.mixed_kernel(capi.MIXED_K_CORRECT_RESIDUAL, 1.0, 1.0, capi.ARR_U, capi.ARR_RHS)   # warm
    ms_k = []
    for _ in range(a.kreps):
        _, _, ms = timed(s32, lambda: s32.mixed_kernel(capi.MIXED_K_CORRECT_RESIDUAL, 1.0, 1.0, capi.ARR_U, capi.ARR_RHS))
        ms_k.append(ms)
    ms_r = []
    for _ in range(a.kreps):
        _, _, ms = timed(s32, lambda: s32.mixed_kernel(capi.MIXED_K_RESIDUAL, 1.0, 1.0, capi.ARR_U, capi.ARR_RHS))
        ms_r.append(ms)
    gb_k, gb_r = 32 * pts / 1e9, 20 * pts / 1e9
    mk, mr = sorted(ms_k)[len(ms_k) // 2], sorted(ms_r)[len(ms_r) // 2]
    print(f"fp32 cycle {ms_c32:.3f} ms, fp64 cycle {ms_c64:.3f} ms (mean of {a.kreps} back-to-back, no norm)")
    print(f"k_mixed_correct_residual + sum + copy of the norm: {spread(ms_k)} ms; {gb_k:.2f} GB compulsory -> {gb_k / mk:.2f} TB/s "
          f"= {gb_k / mk / PEAK_TBS:.1%} of the {PEAK_TBS:g} TB/s peak")
    print(f"k_mixed_residual         + sum + copy of the norm: {spread(ms_r)} ms; {gb_r:.2f} GB compulsory -> {gb_r / mr:.2f} TB/s "
          f"= {gb_r / mr / PEAK_TBS:.1%} of the {PEAK_TBS:g} TB/s peak")
    print(f"mg_device_bytes: fp64 handle {bytes64 / 1e9:.3f} GB = {bytes64 / pts:.1f} B/node; MG_F32 handle with the fp64 outer arrays "
          f"{bytes32 / 1e9:.3f} GB = {bytes32 / pts:.1f} B/node")
    s64.close(); s32.close()


if __name__ == "__main__":
    main()
