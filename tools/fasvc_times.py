"""fasvc_times -- the semilinear kernels on the variable-coefficient operator (mg_fas_* with MG_FAS_ON_COEFFICIENT, the handle's
mg_vc_set_coefficient hierarchy and mg_vc_set_faces mask) measured in one process, per launch, next to (a) the mg_vc_* launch
with the same mask and (b) the plain form (mg_fas_set_form(1)) with the same mask:

 the residual (saving), the Jacobi sweep and the right-hand side of a theta step with a source (theta 0.5), each for the cubic
 and the exp reaction, mask 0 and all six faces; mg_fas_coarse_rhs; and one mg_fas_cycle next to one mg_vc_cycle.

The residual and the Jacobi sweep move u, a, b in and r or u' out: 4 elements per node of compulsory traffic, the step with a
source 5. The transition reads the fine residual, every other row of every other plane of the fine iterate (whole lines), the
coarse coefficient and writes three coarse arrays: (1 + 1/4 + 4/8) elements per fine node. A (kind, element type, mirrored)
combination runs the marching tile only where the tile is faster than the plain form in the same run:
the report ends with that decision per combination.

    python tools/fasvc_times.py                 # 513^3 fp64 and 1025^3 fp32
    python tools/fasvc_times.py --only 3d257f64

HIP events on the handle's stream around --kreps back-to-back launches (no norm fetched), --repeats times after one warm-up
launch of each; median (min .. max). Right-hand side and source: standard normal values; coefficient: uniform in [0.5, 2].
The report goes to stdout and to --log (profiles/fasvc_times.log).
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


def run(name, cfg, a, decisions):
    import torch
    from multigrid_prj_amd import capi
    n, levels = cfg["n"], cfg["levels"]
    dtype = capi.MG_F32 if cfg["f32"] else capi.MG_F64
    tdt = torch.float32 if cfg["f32"] else torch.float64
    tname = "fp32" if cfg["f32"] else "fp64"
    es = 4 if cfg["f32"] else 8
    pts = n ** 3
    U, RHS, RES, TMP = capi.ARR_U, capi.ARR_RHS, capi.ARR_RES, capi.ARR_TMP
    JAC, FW = capi.SMOOTH_JACOBI, capi.RESTRICT_FULLW
    say(f"\n## {name}: 3-D n = {n}, {levels} levels, {tname}, gamma {a.gamma}, shift 1")
    gen = torch.Generator(device="cuda").manual_seed(1)
    b_d = torch.randn((n, n, n), dtype=tdt, device="cuda", generator=gen)
    a_d = torch.rand((n, n, n), dtype=tdt, device="cuda", generator=gen) * 1.5 + 0.5
    torch.cuda.synchronize()
    kw = dict(dim=3, n=n, levels=levels, length=1.0, alpha=1.0, dtype=dtype, cycle=capi.CYCLE_V, smoother=JAC, omega=6.0 / 7.0,
              nu_pre=2, nu_post=2, restriction=FW, coarse_mode=capi.COARSE_FIXED, coarse_maxit=50, outer_pre_gs=0)
    s = capi.Solver(capi.make_desc(**kw))
    lib, h = s.lib, s.h
    s.set_rhs_device(b_d); s.zero_array(U, 0)
    s.vc_set_coefficient_device(a_d); s.heat_set_source_device(b_d); s.sync()
    del a_d
    s.set_shift(1.0)   # regular with every face in the mask and gamma g' >= 0

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

    OPS = ("residual (saving)", "Jacobi sweep", "theta step with source")
    traffic = {OPS[0]: 4.0, OPS[1]: 4.0, OPS[2]: 5.0, "mg_fas_coarse_rhs": 1.75}
    fam_calls = lambda fam: {
        OPS[0]: lambda: getattr(lib, f"mg_{fam}_residual")(h, 0, U, RHS, RES, None),
        OPS[1]: lambda: getattr(s, f"{fam}_smooth")(0, JAC, 1, U, RHS),
        OPS[2]: lambda: getattr(s, f"{fam}_heat_rhs")(1e-3, 0.5, U, TMP),
    }
    tk = {}
    for mlabel, mask in (("mask 0", 0), ("all six faces", 63)):
        s.vc_set_faces(mask); s.zero_array(U, 0); s.sync()
        fns = {f"vc {op}, tile, {mlabel}": fn for op, fn in fam_calls("vc").items()}
        tk.update(measure(fns, a.kreps))
        s.zero_array(U, 0)
        tk.update(measure({f"mg_vc_cycle, {mlabel}": lambda: s.vc_cycle()}, 1))
        for klabel, kind in (("cubic", capi.FAS_CUBIC), ("exp", capi.FAS_EXP)):
            s.fas_set_reaction(kind | capi.FAS_ON_COEFFICIENT, a.gamma)
            s.zero_array(U, 0); s.sync()
            fns = {}
            for form, flabel in ((0, "tile"), (1, "plain")):
                for op, fn in fam_calls("fas").items():
                    fns[f"fas {klabel} {op}, {flabel}, {mlabel}"] = (lambda fn=fn, form=form: (lib.mg_fas_set_form(h, form), fn(), lib.mg_fas_set_form(h, 0)))
            fns[f"fas {klabel} mg_fas_coarse_rhs, {mlabel}"] = lambda: s.fas_coarse_rhs(0)
            tk.update(measure(fns, a.kreps))
            s.zero_array(U, 0)
            tk.update(measure({f"mg_fas_cycle {klabel}, {mlabel}": lambda: s.fas_cycle()}, 1))
            s.zero_array(U, 0)
    for k, ts in tk.items():
        if "cycle" in k:
            say(f"{k:56s} {spread(ts)} ms")
            continue
        g = next(v for op, v in traffic.items() if op in k) * es * pts / 1e9
        say(f"{k:56s} {spread(ts)} ms; {g:.3f} GB compulsory -> {g / med(ts):.2f} TB/s")
    r = lambda x, y: med(tk[x]) / med(tk[y])
    for mlabel in ("mask 0", "all six faces"):
        for klabel in ("cubic", "exp"):
            ratios = []
            for op in OPS:
                pt = r(f"fas {klabel} {op}, plain, {mlabel}", f"fas {klabel} {op}, tile, {mlabel}")
                tv = r(f"fas {klabel} {op}, tile, {mlabel}", f"vc {op}, tile, {mlabel}")
                ratios.append(pt)
                say(f"ratio, {klabel}, {mlabel}, {op}: plain / tile = {pt:.2f}; tile / mg_vc tile = {tv:.2f}")
            say(f"ratio, {klabel}, {mlabel}: mg_fas_cycle / mg_vc_cycle = {r(f'mg_fas_cycle {klabel}, {mlabel}', f'mg_vc_cycle, {mlabel}'):.2f}")
            decisions.append((klabel, tname, "mirrored" if mlabel != "mask 0" else "not mirrored", min(ratios)))
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
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "fasvc_times.log"))
    a = ap.parse_args()
    LOG = open(a.log, "w") if a.log else None
    say(f"# fasvc_times: {a.repeats} repeats, {a.kreps} back-to-back launches per kernel timing")
    decisions = []
    for name in a.only:
        run(name, CONFIGS[name], a, decisions)
    say("\n## tile or plain (the smallest plain / tile ratio of the three modes; the tile runs where it is > 1)")
    for klabel, tname, mir, worst in decisions:
        say(f"{klabel:6s} {tname} {mir:13s}: plain / tile >= {worst:.2f} -> {'tile' if worst > 1 else 'plain form'}")


if __name__ == "__main__":
    main()
