"""fasn_times -- the semilinear kernels with Neumann faces (mg_fas_* with MG_FAS_ON_FACES and a mg_bc_set_faces mask) measured in
one process, per launch, next to the same kernels with mask 0:

 the fas residual (saving) and the fas Jacobi sweep, cubic: the mirrored marching tile, the mask-0 marching tile and the plain
 form with the same mask; mg_fas_coarse_rhs with and without the mask; and one mg_fas_cycle with the flag next to one
 mg_bc_cycle with the same mask.

The residual and the Jacobi sweep move u, b in and r or u' out: 3 elements per node of compulsory traffic. The transition reads
the fine residual, every other row of every other plane of the fine iterate (whole lines) and writes three coarse arrays:
(1 + 1/4 + 3/8) elements per fine node. The condition for shipping the tile is that the mirrored tile is faster than the plain
form with the same mask in the same run; its ratio to the mask-0 tile is reported.

    python tools/fasn_times.py                 # 513^3 fp64 and 1025^3 fp32, all faces Neumann
    python tools/fasn_times.py --only 3d257f64 --mask 0x1a

HIP events on the handle's stream around --kreps back-to-back launches (no norm fetched), --repeats times after one warm-up
launch of each; median (min .. max). Right-hand side: standard normal values. The report goes to stdout and to --log
(profiles/fasn_times.log).
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
    U, RHS, RES = capi.ARR_U, capi.ARR_RHS, capi.ARR_RES
    JAC, FW = capi.SMOOTH_JACOBI, capi.RESTRICT_FULLW
    say(f"\n## {name}: 3-D n = {n}, {levels} levels, {'fp32' if cfg['f32'] else 'fp64'}, cubic gamma {a.gamma}, Neumann mask {a.mask:#08b}")
    gen = torch.Generator(device="cuda").manual_seed(1)
    b_d = torch.randn((n, n, n), dtype=tdt, device="cuda", generator=gen)
    torch.cuda.synchronize()
    kw = dict(dim=3, n=n, levels=levels, length=1.0, alpha=1.0, dtype=dtype, cycle=capi.CYCLE_V, smoother=JAC, omega=6.0 / 7.0,
              nu_pre=2, nu_post=2, restriction=FW, coarse_mode=capi.COARSE_FIXED, coarse_maxit=50, outer_pre_gs=0)
    s = capi.Solver(capi.make_desc(**kw))
    lib, h = s.lib, s.h
    s.set_rhs_device(b_d); s.zero_array(U, 0); s.sync()
    s.fas_set_reaction(capi.FAS_CUBIC | capi.FAS_ON_FACES, a.gamma)
    s.set_shift(1.0)   # regular for mg_bc_cycle with every face in the mask too

    def k_events(fn, reps):
        s.sync(); s.timer_start()
        for _ in range(reps):
            fn()
        return s.timer_stop() / reps

    def measure(fns, reps):
        for fn in fns.values():   # warm-up: one launch of each
            fn()
        out = {k: [] for k in fns}
        for _ in range(a.repeats):
            for k, fn in fns.items():
                out[k].append(k_events(fn, reps))
        return out

    form = lambda f: lib.mg_fas_set_form(h, f)
    res = lambda: lib.mg_fas_residual(h, 0, U, RHS, RES, None)
    jac = lambda: s.fas_smooth(0, JAC, 1, U, RHS)
    tk = {}
    for label, mask in (("mask 0", 0), ("mirrored", a.mask)):
        s.bc_set_faces(mask); s.sync()
        fns = {
            f"fas residual (saving), march, {label}": lambda: (form(0), res()),
            f"fas Jacobi sweep, march, {label}": lambda: (form(0), jac()),
            f"mg_fas_coarse_rhs, {label}": lambda: s.fas_coarse_rhs(0),
        }
        if mask:
            fns[f"fas residual (saving), plain, {label}"] = lambda: (form(1), res(), form(0))
            fns[f"fas Jacobi sweep, plain, {label}"] = lambda: (form(1), jac(), form(0))
        tk.update(measure(fns, a.kreps))
        s.zero_array(U, 0)
        if mask:
            tk.update(measure({"mg_fas_cycle, flag and mask": lambda: s.fas_cycle()}, 1))
            s.zero_array(U, 0)
            tk.update(measure({"mg_bc_cycle, the same mask": lambda: s.bc_cycle()}, 1))
            s.zero_array(U, 0)
    for k, ts in tk.items():
        if "cycle" in k:
            say(f"{k:48s} {spread(ts)} ms")
            continue
        g = (1.625 if "coarse_rhs" in k else 3.0) * es * pts / 1e9
        say(f"{k:48s} {spread(ts)} ms; {g:.3f} GB compulsory -> {g / med(ts):.2f} TB/s")
    r = lambda x, y: med(tk[x]) / med(tk[y])
    for kern in ("fas residual (saving)", "fas Jacobi sweep"):
        say(f"ratio, {kern}: plain / mirrored tile = {r(kern + ', plain, mirrored', kern + ', march, mirrored'):.2f} (must be > 1); "
            f"mirrored tile / mask-0 tile = {r(kern + ', march, mirrored', kern + ', march, mask 0'):.2f}")
    say(f"ratio, mg_fas_coarse_rhs: mirrored / mask 0 = {r('mg_fas_coarse_rhs, mirrored', 'mg_fas_coarse_rhs, mask 0'):.2f}; "
        f"mg_fas_cycle with the flag / mg_bc_cycle = {r('mg_fas_cycle, flag and mask', 'mg_bc_cycle, the same mask'):.2f}")
    s.close()
    del b_d
    torch.cuda.empty_cache()


def main():
    global LOG
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", nargs="+", default=["3d513f64", "3d1025f32"], choices=list(CONFIGS))
    ap.add_argument("--mask", type=lambda v: int(v, 0), default=63, help="the Neumann faces (mg_face bits), default all six")
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "fasn_times.log"))
    a = ap.parse_args()
    LOG = open(a.log, "w") if a.log else None
    say(f"# fasn_times: {a.repeats} repeats, {a.kreps} back-to-back launches per kernel timing")
    for name in a.only:
        run(name, CONFIGS[name], a)


if __name__ == "__main__":
    main()
