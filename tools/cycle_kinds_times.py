"""cycle_kinds_times -- device time per V-, F- and W-cycle with the one-launch LDS sub-cycle (mg_subcycle.hip) rooted at every
admissible level and switched off, and the residual reduction each kind buys per millisecond.

    python tools/cycle_kinds_times.py --case bench513            # 513^3 fp64, 8 levels, V(2,2), full weighting (bench.py's grid)
    python tools/cycle_kinds_times.py --case bench1025           # 1025^3 fp32, 9 levels
    python tools/cycle_kinds_times.py --case weak129             # 129^3 fp64, 6 levels, red-black V(1,1), injection, 2 coarse sweeps
    python tools/cycle_kinds_times.py --case bench513 --smoother rbgs --rates

One process. MG_SUBCYCLE_LEVEL is a HANDLE switch, so every setting gets a handle of its own (created, measured, destroyed in
turn). Times come from HIP events on the handle's stream (mg_timer_*) around `--cycles` back-to-back mg_cycle_async cycles,
after a warm-up of the same length; the figure is the median over `--reps` such batches, with the spread (min .. max).
"launch visits" are the level visits per cycle that run launch by launch (every level above the root, each visit five or six
launches), "kernel launches" the k_subcycle launches, one per visit of the root's parent. --rates adds a six-iteration mg_solve from
u = 0 on a random right-hand side: rate = (h[6] / h[2])^(1/4) per cycle and the decimal digits gained per millisecond.
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

KINDS = {"V": 1, "F": 3, "W": 2}


def case_kw(a):
    from multigrid_prj_amd import capi
    f64 = capi.MG_F64
    base = dict(dim=3, length=1.0, alpha=1.0, nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW, coarse_mode=capi.COARSE_FIXED,
                coarse_maxit=20, outer_pre_gs=0)
    if a.case == "bench513":
        kw = dict(base, n=513, levels=8, dtype=f64)
    elif a.case == "bench1025":
        kw = dict(base, n=1025, levels=9, dtype=capi.MG_F32)
    elif a.case == "iso129":
        kw = dict(base, n=129, levels=6, dtype=f64)
    else:   # weak129: what W and F are for
        kw = dict(base, n=129, levels=6, dtype=f64, nu_pre=1, nu_post=1, restriction=capi.RESTRICT_INJECT, coarse_maxit=2)
        a.smoother = a.smoother or "rbgs"
    kw["smoother"] = capi.SMOOTH_RBGS if a.smoother == "rbgs" else capi.SMOOTH_JACOBI
    kw["omega"] = 6.0 / 7.0 if kw["smoother"] == capi.SMOOTH_JACOBI else 1.0
    return kw


def visits(kind, levels):
    v = [0] * levels

    def rec(l, k):
        v[l] += 1
        if l == levels - 1:
            return
        rec(l + 1, k)
        if l + 1 < levels - 1 and k != 1:
            rec(l + 1, 2 if k == 2 else 1)
    rec(0, kind)
    return v


def measure(kw, kind, setting, b, a):
    """-> (root the handle reports, [ms per cycle of every batch], history or None)"""
    from multigrid_prj_amd import capi
    old = os.environ.pop("MG_SUBCYCLE_LEVEL", None)
    if setting is not None:
        os.environ["MG_SUBCYCLE_LEVEL"] = str(setting)
    try:
        s = capi.Solver(capi.make_desc(cycle=kind, **kw))
    finally:
        os.environ.pop("MG_SUBCYCLE_LEVEL", None)
        if old is not None:
            os.environ["MG_SUBCYCLE_LEVEL"] = old
    with s:
        root = s.subcycle_root()
        if setting is not None and setting < kw["levels"] and root != setting:
            return root, None, None   # not admissible: such a handle runs its launches, which `levels` measures
        s.set_rhs(b)
        s.zero_array(capi.ARR_U, 0)
        s.cycle_async(a.cycles); s.sync()
        ms = []
        for _ in range(a.reps):
            s.timer_start(); s.cycle_async(a.cycles); ms.append(s.timer_stop() / a.cycles)
        hist = None
        if a.rates:
            s.zero_array(capi.ARR_U, 0)
            hist, _ = s.solve(0.0, 6)
    return root, ms, hist


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", choices=["bench513", "bench1025", "iso129", "weak129"], default="bench513")
    ap.add_argument("--smoother", choices=["jacobi", "rbgs"], default=None)
    ap.add_argument("--kinds", default="V,F,W")
    ap.add_argument("--cycles", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rates", action="store_true")
    ap.add_argument("--only-default", action="store_true", help="the library's rule and the launches only, no sweep over the roots")
    a = ap.parse_args()
    from multigrid_prj_amd import capi
    kw = case_kw(a)
    L, n = kw["levels"], kw["n"]
    dt = np.float64 if kw["dtype"] == capi.MG_F64 else np.float32
    b = np.zeros((n, n, n), dt)
    rng = np.random.default_rng(5)
    for k in range(1, n - 1):
        b[k, 1:-1, 1:-1] = rng.standard_normal((n - 2, n - 2))
    print(f"# {a.case}: 3-D {n}^3 {'fp64' if dt == np.float64 else 'fp32'}, {L} levels, {'red-black' if a.smoother == 'rbgs' else 'Jacobi 6/7'} "
          f"({kw['nu_pre']},{kw['nu_post']}), {'full weighting' if kw['restriction'] else 'injection'}, {kw['coarse_maxit']} fixed coarse sweeps; "
          f"{a.cycles} cycles per batch, median of {a.reps} batches", flush=True)
    v_ms = None
    for name in a.kinds.split(","):
        kind = KINDS[name]
        settings = [None, L] if a.only_default else [None] + list(range(1, L - 1)) + [L]
        seen = set()
        for setting in settings:
            root, ms, hist = measure(kw, kind, setting, b, a)
            if ms is None:
                continue
            if setting is None and kind == 1:
                root = -1
            key = (root,)
            if key in seen and setting is not None and setting < L:
                continue
            seen.add(key)
            med = statistics.median(ms)
            if kind == 1 and root < 0 and v_ms is None:
                v_ms = med
            vis = visits(kind, L)
            by_launch = sum(vis[:root]) if root >= 0 else sum(vis)
            kern = vis[root - 1] if root >= 0 else 0   # one launch per visit of the root's parent
            label = "default" if setting is None else ("launches" if setting >= L else f"root {setting}")
            line = (f"{name} {label:9s} root {root:2d}: {med:8.3f} ms/cycle (min {min(ms):.3f} max {max(ms):.3f})  launch visits {by_launch:4d}  "
                    f"kernel launches {kern:3d}")
            if v_ms:
                line += f"  x V {med / v_ms:5.3f}"
            if hist is not None:
                r = (hist[6] / hist[2]) ** 0.25 if len(hist) > 6 and hist[2] > 0 and math.isfinite(hist[6]) else float("nan")
                line += f"  rate {r:7.4f}  digits/ms {(-math.log10(r) / med if r > 0 else float('nan')):7.4f}"
            print(line, flush=True)


if __name__ == "__main__":
    main()
