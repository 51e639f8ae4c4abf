"""vc_times -- the variable-coefficient kernels and cycle (mg_vc_*) measured next to the constant-coefficient ones, in one process:

 1. per launch: the vc residual (saving) and the vc Jacobi sweep, marching tile and plain form; one red-black colour pass;
    the direction kernel of mg_vc_pcg_solve; next to mg_residual (saving) and one unfused mg_smooth Jacobi sweep;
 2. per cycle: mg_vc_cycle V(2,2) with Jacobi (omega 6/7) and with red-black, next to mg_cycle on the same handle.

The vc residual and the vc Jacobi sweep move u, a, b in and r or u' out: 4 elements per node of compulsory traffic (32 B in
fp64). Each launch is reported as the fraction of the rate mg_io's copy kernel streams in the same run (mg_set_array_device:
one element in, one out per node).

    python tools/vc_times.py                 # 513^3 fp64 and 1025^3 fp32
    python tools/vc_times.py --only 3d257f64

HIP events on the handle's stream around --kreps back-to-back launches (no norm fetched), --repeats times; median
(min .. max). Coefficient: 10^(sin 2 pi x cos 2 pi y cos pi z), contrast 100; right-hand side: standard normal values.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "3d257f64": dict(n=257, levels=6, f32=False),
    "3d513f64": dict(n=513, levels=7, f32=False),
    "3d1025f32": dict(n=1025, levels=8, f32=True),
}


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
    print(f"\n## {name}: 3-D n = {n}, {levels} levels, {'fp32' if cfg['f32'] else 'fp64'}, V(2,2), FW, coarse to 0.1", flush=True)
    t = torch.linspace(0.0, 1.0, n, dtype=torch.float64, device="cuda")
    expo = torch.cos(math.pi * t)[:, None, None] * torch.cos(2 * math.pi * t)[None, :, None] * torch.sin(2 * math.pi * t)[None, None, :]
    a_d = torch.pow(10.0, expo).to(tdt).contiguous()
    del expo
    b_d = torch.randn((n, n, n), dtype=tdt, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    torch.cuda.synchronize()
    v = 16 // es
    print("form by level: " + ", ".join(f"{l}: {(n - 1) // 2 ** l + 1}^3 {'march' if ((n - 1) // 2 ** l + 1) // v >= 16 else 'plain'}"
                                        for l in range(levels)) + " (residual and Jacobi sweep; red-black passes are plain on every level)")
    gb = 4 * es * pts / 1e9
    cyc = {}
    for smoother, sname in ((capi.SMOOTH_JACOBI, "jacobi"), (capi.SMOOTH_RBGS, "red-black")):
        kw = dict(dim=3, n=n, levels=levels, length=1.0, alpha=1.0, dtype=dtype, cycle=capi.CYCLE_V, smoother=smoother, omega=6.0 / 7.0,
                  nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW, coarse_mode=capi.COARSE_TOL, coarse_maxit=2000, coarse_tol=0.1,
                  outer_pre_gs=0)
        s = capi.Solver(capi.make_desc(**kw))
        lib, h = s.lib, s.h
        s.set_rhs_device(b_d); s.set_array_device(E, 0, b_d); s.zero_array(U, 0)
        s.vc_set_coefficient_device(a_d); s.sync()

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

        if smoother == capi.SMOOTH_JACOBI:
            form = lambda f: lib.mg_vc_set_form(h, f)
            fns = {
                "mg_io copy (set_array_device)": lambda: s.set_array_device(RES, 0, b_d),
                "mg_residual (saving)": lambda: s.residual_async(0, U, RHS, RES),
                "mg_smooth Jacobi, 1 sweep": lambda: s.smooth(0, capi.SMOOTH_JACOBI, 1, U, RHS),
                "vc residual (saving), march": lambda: (form(0), lib.mg_vc_residual(h, 0, U, RHS, RES, None)),
                "vc residual (saving), plain": lambda: (form(1), lib.mg_vc_residual(h, 0, U, RHS, RES, None), form(0)),
                "vc residual (norm only), march": lambda: (form(0), lib.mg_vc_residual(h, 0, U, RHS, -1, None)),
                "vc Jacobi sweep, march": lambda: (form(0), s.vc_smooth(0, capi.SMOOTH_JACOBI, 1, U, RHS)),
                "vc Jacobi sweep, plain": lambda: (form(1), s.vc_smooth(0, capi.SMOOTH_JACOBI, 1, U, RHS), form(0)),
                "vc red-black colour pass (half a sweep)": lambda: s.vc_smooth(0, capi.SMOOTH_RBGS, 1, U, RHS),
                "vc direction kernel": lambda: lib.mg_vc_direction(h, 0.5, U, E, TMP, RES, None),
            }
            tk = measure(fns, a.kreps)
            tk["vc red-black colour pass (half a sweep)"] = [x / 2 for x in tk["vc red-black colour pass (half a sweep)"]]
            io = 2 * es * pts / 1e9 / med(tk["mg_io copy (set_array_device)"])
            print(f"mg_io streams {io:.2f} TB/s (2 elements per node)")
            for k, ts in tk.items():
                if k.startswith("mg_io"):
                    continue
                elems = 3 if k.startswith("mg_") or "norm only" in k else (5 if "direction" in k else 4)
                g = elems * es * pts / 1e9
                print(f"{k:42s} {spread(ts)} ms; {g:.3f} GB compulsory -> {g / med(ts):.2f} TB/s = {g / med(ts) / io:.2f} of mg_io")
            print(f"ratio: vc residual / mg_residual = {med(tk['vc residual (saving), march']) / med(tk['mg_residual (saving)']):.2f}; "
                  f"vc Jacobi / mg_smooth = {med(tk['vc Jacobi sweep, march']) / med(tk['mg_smooth Jacobi, 1 sweep']):.2f}", flush=True)
        # the cycles
        s.set_rhs_device(b_d); s.zero_array(U, 0)
        fns = {"mg_cycle": lambda: s.cycle_async(1), "mg_vc_cycle": lambda: lib.mg_vc_cycle(h, None)}
        tc = measure(fns, a.creps)
        for k, ts in tc.items():
            print(f"{k:12s} V(2,2) {sname:9s} {spread(ts)} ms per cycle")
        print(f"ratio: mg_vc_cycle / mg_cycle ({sname}) = {med(tc['mg_vc_cycle']) / med(tc['mg_cycle']):.2f}", flush=True)
        cyc[sname] = med(tc["mg_vc_cycle"])
        s.close()
    del a_d, b_d
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", nargs="+", default=["3d513f64", "3d1025f32"], choices=list(CONFIGS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--creps", type=int, default=5)
    a = ap.parse_args()
    print(f"# vc_times: {a.repeats} repeats, {a.kreps} back-to-back launches per kernel timing, {a.creps} cycles per cycle timing")
    for name in a.only:
        run(name, CONFIGS[name], a)


if __name__ == "__main__":
    main()
