"""step_times -- the right-hand side launch of the family time steppers (mg_vc_heat_rhs, mg_bc_heat_rhs, mg_fas_heat_rhs)
measured in one process, per launch, next to what it is compared with:

 each family's launch in the marching tile and in the plain form, with and without a source (theta = 1/2), and bc's
 stencil-free form (theta = 1); mg_heat_rhs; the family's SAVING residual tile, which moves the same arrays (f for b, out
 for r) and is the yardstick; the composed alternative the launch replaces -- the family's residual launch with b = 0 plus
 the torch passes that form the same array from it; one mg_X_heat_step with one cycle per step against one mg_X_cycle.

fp64 vc moves u, a, f in and rhs out (4 elements per node, 3 without a source); bc and fas move 3 (2 without a source).

    python tools/step_times.py                 # 513^3 fp64 and 1025^3 fp32
    python tools/step_times.py --only 3d257f64

HIP events on the handle's stream around --kreps back-to-back launches, --repeats times; median (min .. max). A step / a
cycle is timed around --creps calls, each with its one host synchronisation. The report goes to stdout and to --log
(profiles/step_times.log).
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
    JAC, FW = capi.SMOOTH_JACOBI, capi.RESTRICT_FULLW
    dt, theta = 1e-3, 0.5
    rdt, omt, rth = 1.0 / dt, 1.0 - theta, 1.0 / theta
    say(f"\n## {name}: 3-D n = {n}, {levels} levels, {'fp32' if cfg['f32'] else 'fp64'}, dt = {dt}, theta = {theta}")
    gen = torch.Generator(device="cuda").manual_seed(1)
    u_d = torch.randn((n, n, n), dtype=tdt, device="cuda", generator=gen)
    f_d = torch.randn((n, n, n), dtype=tdt, device="cuda", generator=gen)
    r_d = torch.empty_like(u_d)
    torch.cuda.synchronize()
    kw = dict(dim=3, n=n, levels=levels, length=1.0, alpha=1.0, dtype=dtype, cycle=capi.CYCLE_V, smoother=JAC, omega=6.0 / 7.0,
              nu_pre=2, nu_post=2, restriction=FW, coarse_mode=capi.COARSE_FIXED, coarse_maxit=50, outer_pre_gs=0)
    s = capi.Solver(capi.make_desc(**kw))
    lib, h = s.lib, s.h
    s.set_array_device(U, 0, u_d); s.set_array_device(E, 0, u_d); s.zero_array(RHS, 0)
    s.vc_set_coefficient_device(torch.rand((n, n, n), dtype=tdt, device="cuda", generator=gen) * 1.5 + 0.5)
    s.bc_set_faces(63); s.fas_set_reaction(capi.FAS_CUBIC, 1.0)
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

    src = lambda on: s.heat_set_source_device(f_d if on else None)   # a device copy when on: never inside a timed region
    FAM = ("vc", "bc", "fas")
    rhs = {x: getattr(lib, f"mg_{x}_heat_rhs") for x in FAM}
    res = {x: getattr(lib, f"mg_{x}_residual") for x in FAM}
    form = {x: getattr(lib, f"mg_{x}_set_form") for x in FAM}

    def composed(x):
        # -N0(u) by the family's residual launch with b = 0 (the handle's shift is 0 here), then the passes that form
        # (f + rdt u + omt r) rth from dense device arrays and hand it back; the Dirichlet nodes are left as they come
        res[x](h, 0, E, RHS, RES, None)
        s.get_array_device(RES, 0, r_d)
        t = torch.add(f_d, u_d, alpha=rdt)
        t.add_(r_d, alpha=omt).mul_(rth)
        s.set_array_device(TMP, 0, t)

    with_f = {
        "mg_io copy (set_array_device)": lambda: s.set_array_device(RES, 0, u_d),
        "mg_heat_rhs, source": lambda: lib.mg_heat_rhs(h, dt, theta, U, RES),
        "mg_heat_rhs, theta 1, source": lambda: lib.mg_heat_rhs(h, dt, 1.0, U, RES),
        "mg_bc_heat_rhs, theta 1, tile, source": lambda: rhs["bc"](h, dt, 1.0, U, RES),
    }
    no_f = {
        "mg_heat_rhs, no source": lambda: lib.mg_heat_rhs(h, dt, theta, U, RES),
        "mg_bc_heat_rhs, theta 1, tile, no source": lambda: rhs["bc"](h, dt, 1.0, U, RES),
    }
    for x in FAM:
        with_f.update({
            f"mg_{x}_residual (saving), tile": lambda x=x: res[x](h, 0, E, RHS, RES, None),
            f"mg_{x}_heat_rhs, tile, source": lambda x=x: rhs[x](h, dt, theta, U, RES),
            f"mg_{x}_heat_rhs, plain, source": lambda x=x: (form[x](h, 1), rhs[x](h, dt, theta, U, RES), form[x](h, 0)),
            f"composed: mg_{x}_residual + torch passes": lambda x=x: composed(x),
        })
        no_f.update({
            f"mg_{x}_heat_rhs, tile, no source": lambda x=x: rhs[x](h, dt, theta, U, RES),
            f"mg_{x}_heat_rhs, plain, no source": lambda x=x: (form[x](h, 1), rhs[x](h, dt, theta, U, RES), form[x](h, 0)),
        })
    src(True)
    tk = measure(with_f, a.kreps)
    src(False)
    tk.update(measure(no_f, a.kreps))
    io = 2 * es * pts / 1e9 / med(tk["mg_io copy (set_array_device)"])
    say(f"mg_io streams {io:.2f} TB/s (2 elements per node)")
    for k, ts in tk.items():
        if k.startswith("mg_io"):
            continue
        if k.startswith("composed"):
            say(f"{k:50s} {spread(ts)} ms")
            continue
        elems = (3 if "no source" not in k else 2) + (1 if "_vc_" in k else 0)
        g = elems * es * pts / 1e9
        say(f"{k:50s} {spread(ts)} ms; {g:.3f} GB compulsory -> {g / med(ts):.2f} TB/s = {g / med(ts) / io:.2f} of mg_io")
    r = lambda p, q: med(tk[p]) / med(tk[q])
    for x in FAM:
        say(f"ratio, {x}: rhs tile (source) / saving residual tile = {r(f'mg_{x}_heat_rhs, tile, source', f'mg_{x}_residual (saving), tile'):.2f}, "
            f"/ mg_heat_rhs = {r(f'mg_{x}_heat_rhs, tile, source', 'mg_heat_rhs, source'):.2f}; "
            f"no source / mg_heat_rhs no source = {r(f'mg_{x}_heat_rhs, tile, no source', 'mg_heat_rhs, no source'):.2f}; "
            f"plain / tile = {r(f'mg_{x}_heat_rhs, plain, source', f'mg_{x}_heat_rhs, tile, source'):.2f}; "
            f"composed / rhs tile = {r(f'composed: mg_{x}_residual + torch passes', f'mg_{x}_heat_rhs, tile, source'):.2f}")
    say(f"ratio, bc theta 1 (stencil-free tile) / mg_heat_rhs theta 1 = {r('mg_bc_heat_rhs, theta 1, tile, source', 'mg_heat_rhs, theta 1, source'):.2f}")

    # one step with one cycle against one cycle of the family (Jacobi 6/7 V(2,2), 50 coarse sweeps), each call with its one
    # host synchronisation; both on the shifted operator the step leaves behind
    src(True)
    s.set_shift(1.0 / (theta * dt))
    cyc = {}
    for x in FAM:
        cyc[f"mg_{x}_cycle"] = getattr(s, f"{x}_cycle")
        cyc[f"mg_{x}_heat_step, 1 step, 1 cycle"] = lambda x=x: getattr(s, f"{x}_heat_step")(dt, theta, 1, 1)
    tc = measure(cyc, a.creps)
    for k, ts in tc.items():
        say(f"{k:50s} {spread(ts)} ms per call")
    for x in FAM:
        say(f"ratio, {x}: heat_step(1, 1) / cycle = {med(tc[f'mg_{x}_heat_step, 1 step, 1 cycle']) / med(tc[f'mg_{x}_cycle']):.3f}")
    s.close()
    del u_d, f_d, r_d
    torch.cuda.empty_cache()


def main():
    global LOG
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", nargs="+", default=["3d513f64", "3d1025f32"], choices=list(CONFIGS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--creps", type=int, default=3)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "step_times.log"))
    a = ap.parse_args()
    LOG = open(a.log, "w") if a.log else None
    say(f"# step_times: {a.repeats} repeats, {a.kreps} back-to-back launches per kernel timing, {a.creps} calls per step / cycle timing")
    for name in a.only:
        run(name, CONFIGS[name], a)


if __name__ == "__main__":
    main()
