"""One row per compute entry point of include/mg_hip.h: how to call it, which allocations it may write, and the shapes to run
it on. tests/test_storage_gpu.py holds every row to the layout's invariant through the raw window
mg_debug_raw_*: padding columns (x >= nx) and ghost planes are +0 before and after every call, arrays a call does not write
keep every word, and no result depends on what lies outside the dense grid. tests/test_storage_cpu.py checks that every
function the header declares has a row here or a line in NO_KERNEL. Nothing here needs a GPU or the HIP library.

Which kernel file is reached by which rows and cases (3-D, n^3; "tail" = the hand-written tail-line store of an odd last
column, mg_device.h; a reverted store that wrote its value into the following padding word would leave a non-zero padding
word in an array of the row's written set, which check (a) reports):
  mg_jacobi_fast.hip   k_jacobi (tail 1): smooth[jac-1], cycle at 65, 97, 129, 131 (fp64: n % 2 == 1; fp32: 65, 97, 129: n % 4 == 1);
                       k_jacobi2 fused pair (tail 2) and the folding pair, rows of exactly 64 vectors + 1: smooth[jac-2],
                       cycle[V-jac], solve, fmg, pcg-solve, heat-step at 129 fp64; smooth-wide, cycle-wide at 257 fp32;
                       the one-pass red-black sweep: smooth[rb], cycle[V-rb] at the same sizes;
                       k_resid_restrict_fw: cycle, solve, fmg at 65 .. 131 (tests/size_table.py: resid_restrict_fast_ok)
  mg_pair_wide.hip     k_pairw (tail): smooth-wide[jac-2], cycle-wide[V-jac] at 257 fp64 (128 lanes); 513 fp32: tools/pairbench
  mg_rr_wide.hip       k_rrw: cycle-wide[V-jac] at 257 fp64
  mg_transfer_fast.hip prolong, restrict, cycle at 65, 97, 129 (nf % V == 1, nc >= 17)
  mg_small_levels.hip  brick kernels: cycle[V-jac], solve, fmg at 65 and 97 (levels of at most 129^3, V(2,2), full weighting)
  mg_kernels.hip       every base row at 17 (plain kernels), the coarse solves, zebra and lexicographic sweeps
  mg_subcycle.hip      subcycle[path 1], cycle[W], cycle[F] at 17 (L = 3) and 33 (L = 4)
  mg_fmg.hip           fmg_prolong, fmg: the line store up to line_end <= pitch, every base case
  mg_krylov.hip        pcg_kernel[*], pcg_solve          mg_mixed.hip   mixed_kernel[*], mixed_solve (fp32 handles)
  mg_io.hip            set_array_device, get_array_device
  mg_eig.hip           eig-gram, eig-combine
  mg_heat.hip          heat_rhs, heat_step (tail): 33, 35 fp64; 65, 67 both; the two non-isotropic family cases below on level 0
  mg_o4.hip            o4_residual, o4_correct_residual (tail): 33, 35 fp64; 65 both; 67 fp64; the same two cases on level 0
  mg_vc.hip            vc_* rows, form 0 (marching tile, mirrored with a mask; tail): 33, 35 fp64; 65 both; 67 fp64 (fp32:
                       67 % 4 == 3, the partial last vector); form 1 and n = 9, 17, 2-D: the plain kernels.
                       3d67L2-semi_xy1 (tests/tile_cases.py's s67): the cycle rows run the fp64 tile on level 1, 34 x 34 x 67 --
                       an even row (no tail line) on a level with nz != nx, under checks (a) and (b); the restrict, coarse-rhs
                       and correct rows cross the semi-coarsened transition. 3d65L2-aniso1.0_2.5_0.3 (a65): every row's tile
                       with pairwise distinct axis coefficients; the cycle rows run the fp64 tile on level 1 (33^3, tail) too
  mg_bc.hip, mg_fas.hip  bc_* / fas_* rows, the same cases and forms
An odd n that takes NO tail-line store: 9 and 17 (plain kernels) in every row, 35 and 67 in fp32 (n % 4 == 3).
"""
from collections import namedtuple

import numpy as np

from multigrid_prj_amd import capi

F64, F32 = capi.MG_F64, capi.MG_F32
U, E, RHS, TMP, RES = capi.ARR_U, capi.ARR_E, capi.ARR_RHS, capi.ARR_TMP, capi.ARR_RES
JAC, RB, LEX, ZY, ZX = capi.SMOOTH_JACOBI, capi.SMOOTH_RBGS, capi.SMOOTH_GS_LEX, capi.SMOOTH_ZEBRA_Y, capi.SMOOTH_ZEBRA_X
INJ, FW = capi.RESTRICT_INJECT, capi.RESTRICT_FULLW
LEVEL, VC, KRYLOV, MIXED, EIG, HEAT, O4 = (capi.RAW_LEVEL, capi.RAW_VC, capi.RAW_KRYLOV, capi.RAW_MIXED, capi.RAW_EIG,
                                           capi.RAW_HEAT, capi.RAW_O4)
SPACE_NAME = {LEVEL: "level", VC: "vc_a", KRYLOV: "kry", MIXED: "mx", EIG: "eig", HEAT: "heat_f", O4: "o4"}
SPACE_INDICES = {LEVEL: 5, VC: 1, KRYLOV: 5, MIXED: 3, EIG: 6 * capi.EIG_MAX_BLOCK, HEAT: 1, O4: 3}
LEVEL0_ONLY = (KRYLOV, MIXED, EIG, HEAT, O4)
EIG_M = 3   # block size of the eig rows


# ---------------------------------------------------------------- the padded layout (mg_geom.h)
Layout = namedtuple("Layout", "es nx ny nz pitch gh")


def pitch_of(nx, es):
    """rows are rounded up to 128 bytes (mg_solver.cpp, Solver::init)"""
    epl = 128 // es
    return (nx + epl - 1) // epl * epl


def layout_of(dim, n, nz, es, gh=1):
    return Layout(es, n, n, nz if dim == 3 else 1, pitch_of(n, es), gh)


def raw_shape(lay):
    return (lay.nz + 2 * lay.gh, lay.ny, lay.pitch)


def padding_mask(lay):
    """True on the padding columns x >= nx of the dense planes"""
    m = np.zeros(raw_shape(lay), bool)
    m[lay.gh:lay.gh + lay.nz, :, lay.nx:] = True
    return m


def ghost_mask(lay):
    """True on every word of the ghost planes (their padding columns included)"""
    m = np.zeros(raw_shape(lay), bool)
    m[:lay.gh] = True
    m[lay.gh + lay.nz:] = True
    return m


def dense_view(raw, lay):
    """the (nz, ny, nx) dense part of a raw allocation, a view"""
    return raw[lay.gh:lay.gh + lay.nz, :, :lay.nx]


def fill_outside(raw, lay, value):
    """`value` into every padding column and ghost plane of a raw allocation, in place"""
    raw[lay.gh:lay.gh + lay.nz, :, lay.nx:] = value
    raw[:lay.gh] = value
    raw[lay.gh + lay.nz:] = value


def bits(a):
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def first_outside_nonzero(raw, lay):
    """the comparison of check (a): (count, kind, (z, y, x)) of the words outside the dense grid that are not +0 by bit
    pattern, z counted from the first dense plane (ghost planes: z < 0 or z >= nz); (0, None, None) when all are +0"""
    b = bits(raw)
    if not (b[lay.gh:lay.gh + lay.nz, :, lay.nx:].any() or b[:lay.gh].any() or b[lay.gh + lay.nz:].any()):
        return 0, None, None
    bad = (b != 0) & (padding_mask(lay) | ghost_mask(lay))
    count = int(bad.sum())
    z, y, x = (int(v) for v in np.argwhere(bad)[0])
    kind = "ghost" if z < lay.gh or z >= lay.gh + lay.nz else "padding"
    return count, kind, (z - lay.gh, y, x)


# ---------------------------------------------------------------- cases
Case = namedtuple("Case", "id dim n levels extra")


def C(dim, n, levels, **extra):
    word = lambda v: "_".join(str(x) for x in v) if isinstance(v, tuple) else str(v)   # aniso=(1.0, 2.5, 0.3) -> aniso1.0_2.5_0.3
    return Case(f"{dim}d{n}L{levels}" + "".join(f"-{k}{word(v)}" for k, v in extra.items()), dim, n, levels, extra)


# operator families (tests/test_bc_gpu.py CASES, vcn_ref.march_ok): 9, 17 plain; 33, 34, 35 the fp64 marching tile (2^k + 1,
# an even row, an odd row that is not 2^k + 1); 65, 67 the tile in both precisions (67: a partial last fp32 vector)
FAM3 = [C(3, 9, 2), C(3, 17, 2), C(3, 33, 2), C(3, 34, 1), C(3, 35, 2), C(3, 65, 2), C(3, 67, 2)]
# ... all isotropic cubes. tests/tile_cases.py's s67 and a65: the tile's stores on a level with nz != nx (34 x 34 x 67, level 1 of
# the family cycle rows) and with pairwise distinct axis coefficients. march() below is about level 0, a cube in both
FAM3 += [C(3, 67, 2, semi_xy=1), C(3, 65, 2, aniso=(1.0, 2.5, 0.3))]
D2 = [C(2, 17, 2), C(2, 130, 1), C(2, 129, 2)]
FAM = FAM3 + D2
FAM_2LEVEL = [c for c in FAM if c.levels >= 2]
# base path (tests/size_table.py): 17 plain; 65 the brick kernels; 97, 129, 131 mg_jacobi_fast.hip's single sweep, fused pair,
# folding pair and k_resid_restrict_fw; one semi_xy hierarchy (nz != nx on the coarse levels)
SEMI = C(3, 33, 3, semi_xy=2)
BASE_SMALL = [C(3, 17, 2), C(3, 65, 3), SEMI] + D2
BASE_FAST = [C(3, 97, 3), C(3, 129, 3), C(3, 131, 2)]
BASE = BASE_SMALL + BASE_FAST
BASE_2LEVEL = [c for c in BASE if c.levels >= 2]
WIDE = C(3, 257, 2)            # fp64: k_pairw, k_rrw (128 lanes); fp32: the fused and folding pairs of mg_jacobi_fast.hip (64 vectors + 1)
SUBCYCLE_CASES = [C(3, 17, 3), C(3, 33, 4)]   # tests/test_cycle_kinds_gpu.py SHAPES: root 1 fits one CU's LDS
BOTH = (F64, F32)


def base_desc(case, dtype, **more):
    kw = dict(dim=case.dim, n=case.n, levels=case.levels, dtype=dtype, length=1.0, alpha=1.0, cycle=capi.CYCLE_V, smoother=JAC,
              omega=6 / 7, nu_pre=2, nu_post=2, restriction=FW, coarse_mode=capi.COARSE_FIXED, coarse_maxit=4, outer_pre_gs=0)
    kw.update(case.extra)
    kw.update(more)
    return kw


# ---------------------------------------------------------------- rows
# entries: the functions of mg_hip.h the row runs. variants(case, dtype) -> [dict]: "desc" overrides base_desc (variants
# with equal "desc" share a handle), "id" names the variant. setup(x, v): state the call needs (masks, forms, allocations,
# arrays of other spaces), before the level arrays are filled. call(x, v) -> tuple of the returned scalars.
# writes(x, v) -> {(space, index, level)}: every allocation the call MAY write, scratch included, named AFTER the call
# (out-of-place sweeps swap the U and TMP buffers: both are listed). relies_on_zero: [(space, index, "file:line -- reason")]
# the arrays check (b) must not poison.
Row = namedtuple("Row", "id entries cases dtypes variants setup call writes relies_on_zero")
ROWS = []


def row(id, entries, cases, call, writes, variants=None, setup=None, dtypes=BOTH, relies_on_zero=()):
    entries = (entries,) if isinstance(entries, str) else tuple(entries)
    ROWS.append(Row(id, entries, tuple(cases), tuple(dtypes), variants or (lambda case, dtype: [dict(id="", desc={})]),
                    setup or (lambda x, v: None), call, writes, tuple(relies_on_zero)))


def lv(level, *arrs):
    return {(LEVEL, a, level) for a in arrs}


def all_levels(x, keep=()):
    """every level array of the hierarchy (RES exists on level 0 only) but `keep`"""
    out = set()
    for l in range(x.case.levels):
        out |= lv(l, U, E, RHS, TMP)
    out |= lv(0, RES)
    return out - set(keep)


def product(**axes):
    out = [dict(id="", desc={})]
    for k, vals in axes.items():
        out = [dict(o, **{k: v}, id=(o["id"] + "," if o["id"] else "") + f"{k}={v}") for o in out for v in vals]
    return out


def levels_of(case):
    return (0, 1) if case.levels >= 2 and case.n <= 65 else (0,)


def stats(st):
    return tuple(getattr(st, f) for f, _ in st._fields_)


def digest(a):
    """a returned array as scalars of the call: its bytes"""
    return (np.ascontiguousarray(a).tobytes(),)


# ---- base operators
def _smooth_variants(case, dtype):
    out = []
    for l in levels_of(case):
        out += [dict(id=f"jac-{k}@{l}", desc={}, sm=JAC, sweeps=k, l=l) for k in (1, 2)]
        out += [dict(id=f"rb@{l}", desc={}, sm=RB, sweeps=1, l=l)]
        if case.n <= 33 or case.dim == 2:   # one workgroup walks the whole level
            out += [dict(id=f"lex@{l}", desc={}, sm=LEX, sweeps=1, l=l)]
        if case.n <= 131:
            out += [dict(id=f"zebra-y@{l}", desc=dict(smoother=ZY, omega=1.0), sm=ZY, sweeps=1, l=l),
                    dict(id=f"zebra-x@{l}", desc=dict(smoother=ZX, omega=1.0), sm=ZX, sweeps=1, l=l)]
    return out


row("smooth", "mg_smooth", BASE, variants=_smooth_variants,
    call=lambda x, v: (x.s.smooth(v["l"], v["sm"], v["sweeps"], U, RHS),) and (),
    writes=lambda x, v: lv(v["l"], U, TMP))
row("smooth-wide", "mg_smooth", [WIDE],
    variants=lambda case, dtype: [dict(id="jac-2@0", desc={}, sm=JAC, sweeps=2, l=0), dict(id="jac-1@0", desc={}, sm=JAC, sweeps=1, l=0),
                                  dict(id="rb@0", desc={}, sm=RB, sweeps=1, l=0)],
    call=lambda x, v: (x.s.smooth(0, v["sm"], v["sweeps"], U, RHS),) and (), writes=lambda x, v: lv(0, U, TMP))
row("residual-save", "mg_residual", BASE,
    variants=lambda case, dtype: [dict(id=f"@{l}", desc={}, l=l) for l in levels_of(case)],
    call=lambda x, v: (x.s.residual(v["l"], U, RHS, RES if v["l"] == 0 else TMP),),
    writes=lambda x, v: lv(v["l"], RES if v["l"] == 0 else TMP))
row("residual-norm", "mg_residual", BASE,
    variants=lambda case, dtype: [dict(id=f"@{l}", desc={}, l=l) for l in levels_of(case)],
    call=lambda x, v: (x.s.residual(v["l"], U, RHS, -1),), writes=lambda x, v: set())
row("sumsq", "mg_sumsq", BASE,
    variants=lambda case, dtype: [dict(id=f"@{l}", desc={}, l=l) for l in levels_of(case)],
    call=lambda x, v: (x.s.sumsq(v["l"], RHS),), writes=lambda x, v: set())
row("restrict", "mg_restrict", BASE_2LEVEL, variants=lambda case, dtype: product(kind=(INJ, FW)),
    call=lambda x, v: (x.s.restrict(0, v["kind"], TMP, RHS),) and (), writes=lambda x, v: lv(1, RHS))
row("prolong", "mg_prolong", BASE_2LEVEL, variants=lambda case, dtype: product(add=(0, 1)),
    call=lambda x, v: (x.s.prolong(1, v["add"], U, E),) and (), writes=lambda x, v: lv(0, E))
row("correct", "mg_correct", BASE, call=lambda x, v: (x.s.correct(U, E),) and (), writes=lambda x, v: lv(0, U, E))
row("coarse-solve", "mg_coarse_solve", BASE_SMALL,
    variants=lambda case, dtype: [dict(id="jac", desc={}), dict(id="rb", desc=dict(smoother=RB, omega=1.0)),
                                  dict(id="tol", desc=dict(coarse_mode=capi.COARSE_TOL, coarse_maxit=7))],
    call=lambda x, v: stats(x.s.coarse_solve(x.case.levels - 1, E, RHS)),
    writes=lambda x, v: lv(x.case.levels - 1, E, TMP))
row("coarse-solve-ex", "mg_coarse_solve_ex", BASE_SMALL,
    variants=lambda case, dtype: product(sm=(JAC, RB, LEX), fixed=(0, 1)),
    call=lambda x, v: stats(x.s.coarse_solve_ex(x.case.levels - 1, E, RHS, v["sm"], 5, 0.1, v["fixed"])),
    writes=lambda x, v: lv(x.case.levels - 1, E, TMP))
row("zero-array", "mg_zero_array", BASE_SMALL, call=lambda x, v: (x.s.zero_array(E, 0),) and (), writes=lambda x, v: lv(0, E))
row("set-array", ("mg_set_array", "mg_set_solution", "mg_set_rhs"), BASE_SMALL,
    call=lambda x, v: (x.s.set_array(E, 0, x.extra(0)), x.s.set_solution(x.extra(1)), x.s.set_rhs(x.extra(2))) and (),
    writes=lambda x, v: lv(0, E, U, RHS))
row("get-array", ("mg_get_array", "mg_get_solution"), BASE_SMALL,
    call=lambda x, v: digest(x.s.get_array(E, 0)) + digest(x.s.get_solution()), writes=lambda x, v: set())


def _set_device(x, v):
    import torch
    for k, dt in enumerate((torch.float64, torch.float32)):   # both element types of the dense array: the kernel converts
        t = torch.from_numpy(np.ascontiguousarray(x.extra(k), np.float64)).to("cuda", dt)
        x.s.set_array_device((E, TMP)[k], 0, t)
    x.s.sync()
    return ()


def _get_device(x, v):
    import torch
    out = ()
    for k, dt in enumerate((torch.float64, torch.float32)):
        t = torch.zeros(x.s.level_shape(0), dtype=dt, device="cuda")
        x.s.get_array_device((E, TMP)[k], 0, t)
        x.s.sync()
        out += digest(t.cpu().numpy())
    return out


row("set-array-device", "mg_set_array_device", BASE_SMALL, call=_set_device, writes=lambda x, v: lv(0, E, TMP))
row("get-array-device", "mg_get_array_device", BASE_SMALL, call=_get_device, writes=lambda x, v: set())

# ---- cycles and solves
SAW = dict(cycle=capi.CYCLE_SAWTOOTH, omega=1.0, restriction=INJ, nu_pre=0, nu_post=3)


def _cycle_variants(case, dtype):
    out = [dict(id="V-jac", desc={}), dict(id="V-rb", desc=dict(smoother=RB, omega=1.0))]
    if case.n <= 65:
        out += [dict(id="W", desc=dict(cycle=capi.CYCLE_W)), dict(id="F", desc=dict(cycle=capi.CYCLE_F)),
                dict(id="sawtooth", desc=SAW), dict(id="V11-inj", desc=dict(nu_pre=1, nu_post=1, restriction=INJ))]
    return out


row("cycle", "mg_cycle", BASE + SUBCYCLE_CASES, variants=_cycle_variants,
    call=lambda x, v: stats(x.s.cycle()), writes=lambda x, v: all_levels(x, keep=lv(0, RHS)))
row("cycle-wide", "mg_cycle", [WIDE],
    variants=lambda case, dtype: [dict(id="V-jac", desc=dict(coarse_maxit=2)), dict(id="V-rb", desc=dict(coarse_maxit=2, smoother=RB, omega=1.0))],
    call=lambda x, v: stats(x.s.cycle()), writes=lambda x, v: all_levels(x, keep=lv(0, RHS)))
row("solve", "mg_solve", BASE_SMALL + [C(3, 129, 3)],
    variants=lambda case, dtype: [dict(id="V", desc={})] + ([dict(id="sawtooth", desc=SAW)] if case.n <= 65 else []),
    call=lambda x, v: tuple(x.s.solve(1e-30, 2)[0]), writes=lambda x, v: all_levels(x, keep=lv(0, RHS)))
row("subcycle", "mg_subcycle", SUBCYCLE_CASES, variants=lambda case, dtype: product(kind=(capi.CYCLE_V, capi.CYCLE_W, capi.CYCLE_F), path=(0, 1)),
    call=lambda x, v: stats(x.s.subcycle(1, v["kind"], v["path"])),
    writes=lambda x, v: {k for k in all_levels(x) if k[2] >= 1} - lv(1, RHS))

# ---- full multigrid
row("fmg", "mg_fmg", BASE_SMALL + [C(3, 129, 3)],
    variants=lambda case, dtype: [dict(id="V", desc={})] + ([dict(id="W-rb", desc=dict(cycle=capi.CYCLE_W, smoother=RB, omega=1.0))] if case.n <= 65 else []),
    call=lambda x, v: stats(x.s.fmg(1)), writes=lambda x, v: all_levels(x, keep=lv(0, RHS)))
row("fmg-prolong", "mg_fmg_prolong", BASE_2LEVEL, variants=lambda case, dtype: product(bnd=(-1, RHS)),
    call=lambda x, v: (x.s.fmg_prolong(1, U, E, v["bnd"]),) and (), writes=lambda x, v: lv(0, E))

# ---- Krylov
PCG_ARRS = {capi.PCG_K_UPDATE: ([U, E, RHS, TMP], (U, RHS)), capi.PCG_K_DOTS: ([E, RES, TMP], ()),
            capi.PCG_K_DIRECTION: ([E, RES, U, TMP], (U, TMP))}
row("pcg-kernel", "mg_pcg_kernel", BASE_SMALL + [C(3, 129, 3)],
    variants=lambda case, dtype: product(kernel=(capi.PCG_K_UPDATE, capi.PCG_K_DOTS, capi.PCG_K_DIRECTION)),
    call=lambda x, v: tuple(x.s.pcg_kernel(v["kernel"], 0.37, PCG_ARRS[v["kernel"]][0])),
    writes=lambda x, v: lv(0, *PCG_ARRS[v["kernel"]][1]))


def _pcg_setup(x, v):   # the first call allocates the five Krylov buffers
    if not x.s.debug_raw_layout(KRYLOV, 0, 0).allocated:
        x.s.set_rhs(x.extra(0))
        x.s.pcg_solve(1e-30, 1)


row("pcg-solve", "mg_pcg_solve", BASE_SMALL + [C(3, 129, 3)], setup=_pcg_setup,
    call=lambda x, v: tuple(x.s.pcg_solve(1e-30, 2)[0]),
    writes=lambda x, v: all_levels(x, keep=lv(0, RHS)) | {(KRYLOV, k, 0) for k in range(5)})


# ---- mixed precision (fp32 handles)
def _mixed_setup(x, v):
    x.s.mixed_set_rhs(x.extra(0, np.float64))
    x.s.mixed_set_solution(x.extra(1, np.float64))


row("mixed-kernel", "mg_mixed_kernel", BASE_SMALL + [C(3, 129, 3)], dtypes=(F32,), setup=_mixed_setup,
    variants=lambda case, dtype: product(kernel=(capi.MIXED_K_RESIDUAL, capi.MIXED_K_CORRECT_RESIDUAL)),
    call=lambda x, v: (x.s.mixed_kernel(v["kernel"], 8.0, 0.5, E, RES),),
    writes=lambda x, v: lv(0, RES) | ({(MIXED, 1, 0), (MIXED, 2, 0)} if v["kernel"] == capi.MIXED_K_CORRECT_RESIDUAL else set()))
row("mixed-solve", "mg_mixed_solve", BASE_SMALL + [C(3, 129, 3)], dtypes=(F32,), setup=_mixed_setup,
    call=lambda x, v: tuple(x.s.mixed_solve(1e-30, 2, 1)[0]),
    writes=lambda x, v: all_levels(x) | {(MIXED, 1, 0), (MIXED, 2, 0)})

# ---- fourth order (level 0, n >= 7; the marching tile where mg_geom.h's march_ok says so)
row("o4-residual", "mg_o4_residual", FAM, variants=lambda case, dtype: product(r=(RES, -1)),
    call=lambda x, v: (x.s.o4_residual(U, RHS, v["r"]),), writes=lambda x, v: lv(0, RES) if v["r"] >= 0 else set())
row("o4-correct-residual", "mg_o4_correct_residual", FAM,
    call=lambda x, v: (x.s.o4_correct_residual(U, E, RHS, TMP, RES),), writes=lambda x, v: lv(0, TMP, RES))


# ---- heat
def _heat_setup(x, v):
    x.s.set_shift(0.0)
    x.s.heat_set_source(x.extra(0) if v.get("src") else None)


row("heat-rhs", "mg_heat_rhs", FAM + BASE_FAST[:2], setup=_heat_setup, variants=lambda case, dtype: product(theta=(1.0, 0.5), src=(0, 1)),
    call=lambda x, v: (x.s.heat_rhs(1e-3, v["theta"], U, RHS),) and (), writes=lambda x, v: lv(0, RHS))
row("heat-step", "mg_heat_step", BASE_SMALL + [C(3, 129, 3)], setup=_heat_setup, variants=lambda case, dtype: product(src=(0, 1)),
    call=lambda x, v: stats(x.s.heat_step(1e-3, 0.5, 1, 1)), writes=lambda x, v: all_levels(x))


# ---- eigen block
def _eig_setup(x, v):
    for f in range(6):   # X first: it makes the block
        for j in range(EIG_M):
            x.s.eig_set_vector(f, j, x.extra(f * EIG_M + j))


def _eig_call(x, v):
    if v["kernel"] == "gram":
        G, H = x.s.eig_kernel_gram(2, v["np"])
        return digest(G) + digest(H)
    n = EIG_M + 2 + v["np"]
    rng = np.random.default_rng(5)
    return digest(x.s.eig_kernel_combine(2, v["np"], rng.standard_normal((n, EIG_M)), rng.standard_normal((2 + v["np"], 2)),
                                         rng.uniform(1.0, 50.0, EIG_M)))


def _eig_writes(x, v):
    fams = (capi.EIG_W, capi.EIG_AW) if v["kernel"] == "gram" else (capi.EIG_X, capi.EIG_AX, capi.EIG_W, capi.EIG_P, capi.EIG_AP)
    return {(EIG, f * capi.EIG_MAX_BLOCK + j, 0) for f in fams for j in range(EIG_M)}


# k_eig_gram zeroes its ROW operands at e >= valid and multiplies them with COLUMN operands it has not masked there: the product
# is 0 only while the columns' padding words are finite
EIG_GRAM_ZERO = "mg_eig.hip:241 -- acc += av * cv with av zeroed in the padding columns (line 232) and cv as loaded: 0 * padding"
row("eig-gram", "mg_eig_kernel", BASE_SMALL, setup=_eig_setup, variants=lambda case, dtype: product(kernel=("gram",), np=(0, 2)),
    call=_eig_call, writes=_eig_writes,
    relies_on_zero=[(EIG, f * capi.EIG_MAX_BLOCK + j, EIG_GRAM_ZERO) for f in range(6) for j in range(EIG_M)])
row("eig-combine", "mg_eig_kernel", BASE_SMALL, setup=_eig_setup, variants=lambda case, dtype: product(kernel=("combine",), np=(0, 2)),
    call=_eig_call, writes=_eig_writes)


# ---- operator families: masks 0 / all faces / mixed, both forms where the marching tile takes level 0
def fam_masks(dim):
    return (0, 63 if dim == 3 else 15, 0b011010 if dim == 3 else 0b1010)


def march(case, dtype):
    """level 0 (a cube) takes the marching tile; not for the levels of a semi-coarsened hierarchy"""
    return case.dim == 3 and case.n // (16 // (8 if dtype == F64 else 4)) >= 16 and case.n >= 7


def _forms(case, dtype):
    return (0, 1) if march(case, dtype) else (0,)


def _fam_variants(fam, **axes):
    def f(case, dtype):
        first = dict(reaction=((capi.FAS_CUBIC, 0.7), (capi.FAS_EXP, 0.7))) if fam == "fas" else dict(mask=fam_masks(case.dim))
        return product(**first, form=_forms(case, dtype), **axes)
    return f


def _fam_setup(fam):
    def f(x, v):
        s = x.s
        s.set_shift(0.0)
        s.heat_set_source(None)
        if fam == "vc":
            if not s.debug_raw_layout(VC, 0, 0).allocated or x.coef_dirty:
                s.vc_set_faces(0)
                s.vc_set_coefficient(1.0 + np.abs(x.extra(0)))
                x.coef_dirty = False
            s.vc_set_faces(v["mask"]); s.vc_set_form(v["form"])
        elif fam == "bc":
            s.bc_set_faces(v["mask"]); s.bc_set_form(v["form"])
        else:
            s.fas_set_reaction(*v["reaction"]); s.fas_set_form(v["form"])
    return f


RBD = dict(smoother=RB, omega=1.0)   # the families' cycles and coarse solves want a Jacobi or red-black handle


def fam_rows(fam):
    m = lambda name: lambda x: getattr(x.s, f"{fam}_{name}")
    su, va = _fam_setup(fam), lambda **axes: _fam_variants(fam, **axes)
    row(f"{fam}-residual", f"mg_{fam}_residual", FAM, setup=su, variants=va(r=(TMP, -1)),
        call=lambda x, v: (m("residual")(x)(0, U, RHS, v["r"]),), writes=lambda x, v: lv(0, TMP) if v["r"] >= 0 else set())
    row(f"{fam}-smooth", f"mg_{fam}_smooth", FAM, setup=su, variants=va(sm=(JAC, RB)),
        call=lambda x, v: (m("smooth")(x)(0, v["sm"], 1, U, RHS),) and (), writes=lambda x, v: lv(0, U, TMP))
    row(f"{fam}-coarse-solve", f"mg_{fam}_coarse_solve", [c for c in FAM_2LEVEL if c.n <= 35], setup=su,
        variants=lambda case, dtype: [dict(o, desc=d, id=o["id"] + "," + n) for o in va()(case, dtype) for n, d in (("jac", {}), ("rb", RBD))],
        call=lambda x, v: stats(m("coarse_solve")(x)(1, E, RHS)), writes=lambda x, v: lv(1, E, TMP))
    row(f"{fam}-cycle", f"mg_{fam}_cycle", FAM, setup=su,
        variants=lambda case, dtype: [dict(o, desc=d, id=o["id"] + "," + n) for o in va()(case, dtype)
                                      for n, d in (("jac", {}), ("rb-W", dict(RBD, cycle=capi.CYCLE_W)))],
        call=lambda x, v: stats(m("cycle")(x)()), writes=lambda x, v: all_levels(x, keep=lv(0, RHS)))
    row(f"{fam}-heat-rhs", f"mg_{fam}_heat_rhs", FAM, setup=su, variants=va(theta=(1.0, 0.5)),
        call=lambda x, v: (m("heat_rhs")(x)(1e-3, v["theta"], U, RHS),) and (), writes=lambda x, v: lv(0, RHS))
    if fam in ("vc", "bc"):
        row(f"{fam}-restrict", f"mg_{fam}_restrict", FAM_2LEVEL, setup=su,
            variants=lambda case, dtype: product(mask=fam_masks(case.dim), kind=(INJ, FW), form=(0,)),
            call=lambda x, v: (m("restrict")(x)(0, v["kind"], TMP, RHS),) and (), writes=lambda x, v: lv(1, RHS))
        row(f"{fam}-project", f"mg_{fam}_project", FAM, setup=su,
            variants=lambda case, dtype: product(mask=fam_masks(case.dim), form=(0,)),
            call=lambda x, v: (m("project")(x)(0, E),), writes=lambda x, v: lv(0, E))


fam_rows("vc")


def _vc_set_coefficient(x, v):
    x.coef_dirty = True
    x.s.vc_set_coefficient(1.5 + np.abs(x.extra(1)))
    return ()


row("vc-set-coefficient", "mg_vc_set_coefficient", FAM, setup=_fam_setup("vc"),
    variants=lambda case, dtype: product(mask=fam_masks(case.dim), form=(0,)),
    call=_vc_set_coefficient, writes=lambda x, v: {(VC, 0, l) for l in range(x.case.levels)})
row("vc-direction", "mg_vc_direction", FAM, setup=_fam_setup("vc"), variants=_fam_variants("vc"),
    call=lambda x, v: (x.s.vc_direction(0.37, E, RES, U, TMP),), writes=lambda x, v: lv(0, U, TMP))
fam_rows("bc")
fam_rows("fas")
row("fas-coarse-rhs", "mg_fas_coarse_rhs", FAM_2LEVEL, setup=_fam_setup("fas"),
    variants=lambda case, dtype: [dict(o, desc=d, id=o["id"] + "," + n) for o in _fam_variants("fas")(case, dtype)
                                  for n, d in (("fw", {}), ("inj", dict(restriction=INJ)))],
    call=lambda x, v: (x.s.fas_coarse_rhs(0),) and (), writes=lambda x, v: lv(1, U, E, RHS))
row("fas-correct", "mg_fas_correct", FAM_2LEVEL, setup=_fam_setup("fas"), variants=_fam_variants("fas"),
    call=lambda x, v: (x.s.fas_correct(0),) and (), writes=lambda x, v: lv(1, E) | lv(0, U))

ROW = {r.id: r for r in ROWS}
assert len(ROW) == len(ROWS)

# ---------------------------------------------------------------- functions of mg_hip.h without a row, and why
NO_KERNEL = {
    "mg_last_error": "query", "mg_device_count": "query", "mg_create": "allocates and clears; every row starts from it",
    "mg_destroy": "frees", "mg_level_n": "query", "mg_level_nz": "query", "mg_level_coefficients": "query",
    "mg_subcycle_root": "query", "mg_get_shift": "query", "mg_vc_get_faces": "query", "mg_bc_get_faces": "query",
    "mg_fas_get_reaction": "query", "mg_eig_block": "query", "mg_comm_info": "query", "mg_comm_stats": "query",
    "mg_device_bytes": "query", "mg_profile_fused": "query", "mg_profile_get": "query",
    "mg_set_shift": "host coefficients (a zebra handle re-tabulates its line factors, which are not level-shaped); set by the rows heat-rhs, heat-step and the family rows",
    "mg_vc_set_form": "a flag; both values run in every vc-* row", "mg_bc_set_form": "a flag; both values run in every bc-* row",
    "mg_fas_set_form": "a flag; both values run in every fas-* row",
    "mg_bc_set_faces": "a mask; three values run in every bc-* row",
    "mg_vc_set_faces": "the mask, then vc-set-coefficient's restriction of the stored level 0; three values run in every vc-* row",
    "mg_fas_set_reaction": "two scalars; both kinds run in every fas-* row",
    "mg_set_stage_callback": "host state", "mg_sync": "waits", "mg_timer_start": "event", "mg_timer_stop": "event",
    "mg_profile_begin": "events", "mg_profile_end": "events",
    "mg_comm_unique_id": "comm", "mg_comm_selftest": "comm, no level array", "mg_create_distributed": "distributed handle: tests/test_distributed.py",
    "mg_create_distributed_hostcomm": "distributed handle: tests/test_distributed.py",
    "mg_create_distributed_dryrun": "distributed handle: tests/test_distributed.py", "mg_plan_slab": "host-only plan",
    "mg_debug_raw_layout": "the window itself, no kernel", "mg_debug_raw_copy": "the window itself, no kernel",
    "mg_cycle_async": "mg_cycle without the fetch of its statistics: row cycle",
    "mg_solve_lockstep": "mg_solve's unfused loop with the coarse sweep count given: rows solve, cycle, coarse-solve-ex",
    "mg_o4_solve": "composition: rows o4-residual, o4-correct-residual, cycle",
    "mg_eig_solve": "composition: rows eig-gram, eig-combine, cycle",
    "mg_vc_solve": "composition: rows vc-residual, vc-cycle, vc-project", "mg_vc_pcg_solve": "composition: rows vc-direction, vc-cycle, vc-project, pcg-kernel",
    "mg_bc_solve": "composition: rows bc-residual, bc-cycle, bc-project", "mg_fas_solve": "composition: rows fas-residual, fas-cycle",
    "mg_vc_heat_step": "composition: rows vc-heat-rhs, vc-cycle, vc-residual", "mg_bc_heat_step": "composition: rows bc-heat-rhs, bc-cycle, bc-residual",
    "mg_fas_heat_step": "composition: rows fas-heat-rhs, fas-cycle, fas-residual",
    "mg_heat_set_source": "mg_set_array's host staging copy into the source array: row set-array; used by heat-rhs, heat-step",
    "mg_mixed_set_rhs": "mg_set_array's host staging copy with the fp64 geometry: row set-array; used by mixed-kernel",
    "mg_mixed_set_solution": "as mg_mixed_set_rhs", "mg_mixed_get_solution": "mg_get_array's staging copy: row get-array",
    "mg_eig_set_vector": "mg_set_array's host staging copy: row set-array; used by eig-kernel", "mg_eig_get_vector": "row get-array's copy",
    "mg_vc_get_coefficient": "row get-array's copy",
    "mg_heat_set_source_device": "the copy kernel of row set-array-device on the same geometry",
    "mg_mixed_set_rhs_device": "the copy kernel of row set-array-device", "mg_mixed_set_solution_device": "the copy kernel of row set-array-device",
    "mg_mixed_get_solution_device": "the copy kernel of row get-array-device",
    "mg_eig_set_vector_device": "the copy kernel of row set-array-device", "mg_eig_get_vector_device": "the copy kernel of row get-array-device",
    "mg_vc_set_coefficient_device": "the copy kernel of row set-array-device, then vc-set-coefficient's restriction",
}


def pairs():
    """every (row, case, dtype) the GPU test runs"""
    return [(r, c, dt) for r in ROWS for c in r.cases for dt in r.dtypes]


def pair_id(p):
    r, c, dt = p
    return f"{r.id}-{c.id}-{'f64' if dt == F64 else 'f32'}"
