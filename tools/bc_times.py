"""bc_times -- the Neumann-face kernels (mg_bc_*) measured next to the constant all-Dirichlet ones, in one process, per launch:

 the bc residual (saving) and the bc Jacobi sweep, marching tile and plain form; one red-black colour pass; mg_bc_restrict
 (full weighting with mirrored neighbours); next to mg_residual (saving), one unfused mg_smooth Jacobi sweep, mg_restrict
 and the rate mg_io's copy kernel streams (mg_set_array_device: one element in, one out per node).

The bc residual and the bc Jacobi sweep move u, b in and r or u' out: 3 elements per node of compulsory traffic, what
mg_residual moves. The expectation to check is a ratio near 1 against the constant kernels in the same run.

    python tools/bc_times.py                 # 513^3 fp64 and 1025^3 fp32, all faces Neumann
    python tools/bc_times.py --only 3d257f64 --mask 0

HIP events on the handle's stream around --kreps back-to-back launches (no norm fetched), --repeats times; median
(min .. max). Right-hand side: standard normal values. The report goes to stdout and to --log (profiles/bc_times.log).
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "3d257f64": dict(n=257, levels=6, f32=False),
    "3d513f64": dict(n=513, levels=7, f32=False),
    "3d1025f32": dict(n=1025, levels=8, f32=True),
}
LOG = None


def say(text=""):
    print(text, flush=True)
    if LOG:
        LOG.write(text + "\n"); LOG.flush()


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def spread(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:8.3f} ({v[0]:.3f} .. {v[-1]:.3f})"


def run(name, cfg, a):
    import torch
    from multigrid_prj_amd import capi
    n, levels = cfg["n"], cfg["levels"]
    dtype = capi.MG_F32 if cfg["f32"] else capi.MG_F64
    tdt = torch.float32 if cfg["f32"] else torch.float64
    es = 4 if cfg["f32"] else 8
    pts = n ** 3
    U, E, RHS, TMP, RES = capi.ARR_U, capi.ARR_E, capi.ARR_RHS, capi.ARR_TMP, capi.ARR_RES
    JAC, RB, FW = capi.SMOOTH_JACOBI, capi.SMOOTH_RBGS, capi.RESTRICT_FULLW
    say(f"\n## {name}: 3-D n = {n}, {levels} levels, {'fp32' if cfg['f32'] else 'fp64'}, Neumann mask {a.mask:#08b}")
    b_d = torch.randn((n, n, n), dtype=tdt, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    torch.cuda.synchronize()
    kw = dict(dim=3, n=n, levels=levels, length=1.0, alpha=1.0, dtype=dtype, cycle=capi.CYCLE_V, smoother=JAC, omega=6.0 / 7.0,
              nu_pre=2, nu_post=2, restriction=FW, coarse_mode=capi.COARSE_TOL, coarse_maxit=2000, coarse_tol=0.1, outer_pre_gs=0)
    s = capi.Solver(capi.make_desc(**kw))
    lib, h = s.lib, s.h
    s.set_rhs_device(b_d); s.set_array_device(E, 0, b_d); s.zero_array(U, 0)
    s.bc_set_faces(a.mask); s.sync()

    def k_events(fn, reps):
        s.sync(); s.timer_start()
        for _ in range(reps):
            fn()
        return s.timer_stop() / reps

    def measure(fns, reps):
        for fn in fns.values():
            fn()
        out = {k: [] for k in fns}
        for _ in range(a.repeats):
            for k, fn in fns.items():
                out[k].append(k_events(fn, reps))
        return out

    form = lambda f: lib.mg_bc_set_form(h, f)
    fns = {
        "mg_io copy (set_array_device)": lambda: s.set_array_device(RES, 0, b_d),
        "mg_residual (saving)": lambda: s.residual_async(0, U, RHS, RES),
        "mg_smooth Jacobi, 1 sweep": lambda: s.smooth(0, JAC, 1, U, RHS),
        "mg_restrict (full weighting)": lambda: s.restrict(0, FW, E, TMP),
        "bc residual (saving), march": lambda: (form(0), lib.mg_bc_residual(h, 0, U, RHS, RES, None)),
        "bc residual (saving), plain": lambda: (form(1), lib.mg_bc_residual(h, 0, U, RHS, RES, None), form(0)),
        "bc residual (norm only), march": lambda: (form(0), lib.mg_bc_residual(h, 0, U, RHS, -1, None)),
        "bc Jacobi sweep, march": lambda: (form(0), s.bc_smooth(0, JAC, 1, U, RHS)),
        "bc Jacobi sweep, plain": lambda: (form(1), s.bc_smooth(0, JAC, 1, U, RHS), form(0)),
        "bc red-black colour pass (half a sweep)": lambda: s.bc_smooth(0, RB, 1, U, RHS),
        "mg_bc_restrict (mirrored full weighting)": lambda: s.bc_restrict(0, FW, E, TMP),
    }
    tk = measure(fns, a.kreps)
    tk["bc red-black colour pass (half a sweep)"] = [x / 2 for x in tk["bc red-black colour pass (half a sweep)"]]
    io = 2 * es * pts / 1e9 / med(tk["mg_io copy (set_array_device)"])
    say(f"mg_io streams {io:.2f} TB/s (2 elements per node)")
    for k, ts in tk.items():
        if k.startswith("mg_io"):
            continue
        elems = 1.125 if "restrict" in k else (2 if "norm only" in k else 3)   # restriction: the fine array in, 1/8 of it out
        g = elems * es * pts / 1e9
        say(f"{k:42s} {spread(ts)} ms; {g:.3f} GB compulsory -> {g / med(ts):.2f} TB/s = {g / med(ts) / io:.2f} of mg_io")
    r = lambda x, y: med(tk[x]) / med(tk[y])
    say(f"ratio: bc residual (march) / mg_residual = {r('bc residual (saving), march', 'mg_residual (saving)'):.2f}; "
        f"bc Jacobi (march) / mg_smooth = {r('bc Jacobi sweep, march', 'mg_smooth Jacobi, 1 sweep'):.2f}; "
        f"mg_bc_restrict / mg_restrict = {r('mg_bc_restrict (mirrored full weighting)', 'mg_restrict (full weighting)'):.2f}")
    say(f"ratio: bc residual plain / march = {r('bc residual (saving), plain', 'bc residual (saving), march'):.2f}; "
        f"bc Jacobi plain / march = {r('bc Jacobi sweep, plain', 'bc Jacobi sweep, march'):.2f}")
    s.close()
    del b_d
    torch.cuda.empty_cache()


def main():
    global LOG
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", nargs="+", default=["3d513f64", "3d1025f32"], choices=list(CONFIGS))
    ap.add_argument("--mask", type=lambda v: int(v, 0), default=63, help="the Neumann faces (mg_face bits), default all six")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "bc_times.log"))
    a = ap.parse_args()
    LOG = open(a.log, "w") if a.log else None
    say(f"# bc_times: {a.repeats} repeats, {a.kreps} back-to-back launches per kernel timing")
    for name in a.only:
        run(name, CONFIGS[name], a)


if __name__ == "__main__":
    main()
