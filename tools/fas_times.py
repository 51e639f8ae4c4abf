"""fas_times -- the kernels of the full approximation scheme (mg_fas_*) measured next to the constant ones, in one process, per
launch:

 the fas residual (saving) and the fas Jacobi sweep, marching tile and plain form, cubic and exp; one red-black colour pass;
 mg_fas_coarse_rhs (the FAS transition) against mg_restrict; one mg_fas_cycle against mg_cycle and mg_bc_cycle with mask 0;
 next to mg_residual (saving), one unfused mg_smooth Jacobi sweep and the rate mg_io's copy kernel streams
 (mg_set_array_device: one element in, one out per node).

The fas residual and the fas Jacobi sweep move u, b in and r or u' out: 3 elements per node of compulsory traffic, what
mg_residual and the bc tile move. The expectation to check is the bc tile's time for the cubic tile.

    python tools/fas_times.py                 # 513^3 fp64 and 1025^3 fp32
    python tools/fas_times.py --only 3d257f64

HIP events on the handle's stream around --kreps back-to-back launches (no norm fetched), --repeats times; median
(min .. max). A cycle is timed around --creps calls, each with its one fetch of the coarse statistics. Right-hand side:
standard normal values; gamma = 1. The report goes to stdout and to --log (profiles/fas_times.log).
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
    CUBIC, EXP = capi.FAS_CUBIC, capi.FAS_EXP
    say(f"\n## {name}: 3-D n = {n}, {levels} levels, {'fp32' if cfg['f32'] else 'fp64'}, gamma = {a.gamma}")
    b_d = torch.randn((n, n, n), dtype=tdt, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    torch.cuda.synchronize()
    kw = dict(dim=3, n=n, levels=levels, length=1.0, alpha=1.0, dtype=dtype, cycle=capi.CYCLE_V, smoother=JAC, omega=6.0 / 7.0,
              nu_pre=2, nu_post=2, restriction=FW, coarse_mode=capi.COARSE_FIXED, coarse_maxit=50, outer_pre_gs=0)
    s = capi.Solver(capi.make_desc(**kw))
    lib, h = s.lib, s.h
    s.set_rhs_device(b_d); s.set_array_device(E, 0, b_d); s.zero_array(U, 0)
    s.sync()

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

    form = lambda f: lib.mg_fas_set_form(h, f)
    kind = lambda k: s.fas_set_reaction(k, a.gamma)
    fns = {
        "mg_io copy (set_array_device)": lambda: s.set_array_device(RES, 0, b_d),
        "mg_residual (saving)": lambda: s.residual_async(0, U, RHS, RES),
        "mg_smooth Jacobi, 1 sweep": lambda: s.smooth(0, JAC, 1, U, RHS),
        "mg_restrict (full weighting)": lambda: s.restrict(0, FW, E, TMP),
        "bc residual (saving), march, mask 0": lambda: lib.mg_bc_residual(h, 0, U, RHS, RES, None),
        "bc Jacobi sweep, march, mask 0": lambda: s.bc_smooth(0, JAC, 1, U, RHS),
    }
    for kname, k in (("cubic", CUBIC), ("exp", EXP)):
        fns.update({
            f"fas residual (saving), march, {kname}": lambda k=k: (kind(k), form(0), lib.mg_fas_residual(h, 0, U, RHS, RES, None)),
            f"fas residual (saving), plain, {kname}": lambda k=k: (kind(k), form(1), lib.mg_fas_residual(h, 0, U, RHS, RES, None), form(0)),
            f"fas residual (norm only), march, {kname}": lambda k=k: (kind(k), form(0), lib.mg_fas_residual(h, 0, U, RHS, -1, None)),
            f"fas Jacobi sweep, march, {kname}": lambda k=k: (kind(k), form(0), s.fas_smooth(0, JAC, 1, U, RHS)),
            f"fas Jacobi sweep, plain, {kname}": lambda k=k: (kind(k), form(1), s.fas_smooth(0, JAC, 1, U, RHS), form(0)),
            f"fas red-black colour pass (half a sweep), {kname}": lambda k=k: (kind(k), s.fas_smooth(0, RB, 1, U, RHS)),
            f"mg_fas_coarse_rhs, {kname}": lambda k=k: (kind(k), s.fas_coarse_rhs(0)),
        })
    tk = measure(fns, a.kreps)
    for k in tk:
        if "colour pass" in k:
            tk[k] = [x / 2 for x in tk[k]]
    io = 2 * es * pts / 1e9 / med(tk["mg_io copy (set_array_device)"])
    say(f"mg_io streams {io:.2f} TB/s (2 elements per node)")
    for k, ts in tk.items():
        if k.startswith("mg_io"):
            continue
        # restriction: the fine array in, 1/8 of it out; the FAS transition: two fine arrays in, 3/8 out
        elems = 1.125 if "mg_restrict" in k else (2.375 if "coarse_rhs" in k else (2 if "norm only" in k else 3))
        g = elems * es * pts / 1e9
        say(f"{k:50s} {spread(ts)} ms; {g:.3f} GB compulsory -> {g / med(ts):.2f} TB/s = {g / med(ts) / io:.2f} of mg_io")
    r = lambda x, y: med(tk[x]) / med(tk[y])
    for kname in ("cubic", "exp"):
        say(f"ratio, {kname}: fas residual (march) / mg_residual = {r(f'fas residual (saving), march, {kname}', 'mg_residual (saving)'):.2f}, "
            f"/ bc tile = {r(f'fas residual (saving), march, {kname}', 'bc residual (saving), march, mask 0'):.2f}; "
            f"fas Jacobi (march) / mg_smooth = {r(f'fas Jacobi sweep, march, {kname}', 'mg_smooth Jacobi, 1 sweep'):.2f}, "
            f"/ bc tile = {r(f'fas Jacobi sweep, march, {kname}', 'bc Jacobi sweep, march, mask 0'):.2f}; "
            f"plain / march = {r(f'fas residual (saving), plain, {kname}', f'fas residual (saving), march, {kname}'):.2f} (residual), "
            f"{r(f'fas Jacobi sweep, plain, {kname}', f'fas Jacobi sweep, march, {kname}'):.2f} (Jacobi); "
            f"mg_fas_coarse_rhs / mg_restrict = {r(f'mg_fas_coarse_rhs, {kname}', 'mg_restrict (full weighting)'):.2f}")

    # one cycle of each family from u = 0 (Jacobi 6/7 V(2,2), 50 coarse sweeps), each call with its fetch of the coarse statistics
    def fresh(fn):
        def go():
            s.zero_array(U, 0)
            fn()
        return go
    cyc = {"mg_cycle": fresh(s.cycle), "mg_bc_cycle, mask 0": fresh(s.bc_cycle),
           "mg_fas_cycle, cubic": fresh(lambda: (kind(CUBIC), s.fas_cycle())), "mg_fas_cycle, exp": fresh(lambda: (kind(EXP), s.fas_cycle()))}
    tc = measure(cyc, a.creps)
    for k, ts in tc.items():
        say(f"{k:50s} {spread(ts)} ms per cycle (the zeroing of U included)")
    rc = lambda x, y: med(tc[x]) / med(tc[y])
    say(f"ratio: mg_fas_cycle (cubic) / mg_cycle = {rc('mg_fas_cycle, cubic', 'mg_cycle'):.2f}, / mg_bc_cycle = {rc('mg_fas_cycle, cubic', 'mg_bc_cycle, mask 0'):.2f}; "
        f"mg_fas_cycle (exp) / mg_bc_cycle = {rc('mg_fas_cycle, exp', 'mg_bc_cycle, mask 0'):.2f}")
    s.close()
    del b_d
    torch.cuda.empty_cache()


def main():
    global LOG
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", nargs="+", default=["3d513f64", "3d1025f32"], choices=list(CONFIGS))
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--creps", type=int, default=3)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "fas_times.log"))
    a = ap.parse_args()
    LOG = open(a.log, "w") if a.log else None
    say(f"# fas_times: {a.repeats} repeats, {a.kreps} back-to-back launches per kernel timing, {a.creps} cycles per cycle timing")
    for name in a.only:
        run(name, CONFIGS[name], a)


if __name__ == "__main__":
    main()
