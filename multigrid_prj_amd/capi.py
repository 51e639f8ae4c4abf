"""ctypes binding of libmg_hip.so (include/mg_hip.h) -- the host-side mirror used by
tests and bench.py.  There is no CPU fallback: loading fails loudly when the HIP
library is missing, and Solver() fails loudly when no GPU is present.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

MG_F64, MG_F32 = 0, 1
SMOOTH_GS_LEX, SMOOTH_JACOBI, SMOOTH_RBGS, SMOOTH_ZEBRA_Y, SMOOTH_ZEBRA_X = 0, 1, 2, 3, 4
CYCLE_SAWTOOTH, CYCLE_V = 0, 1
CYCLE_W, CYCLE_F = 2, 3
RESTRICT_INJECT, RESTRICT_FULLW = 0, 1
FACE_XLO, FACE_XHI, FACE_YLO, FACE_YHI, FACE_ZLO, FACE_ZHI = 1, 2, 4, 8, 16, 32   # enum mg_face: the Neumann faces of mg_bc_*
FAS_CUBIC, FAS_EXP = 0, 1   # enum mg_fas_kind: the reaction g of mg_fas_* (u^3, exp(u))
FAS_ON_FACES = 256          # OR-ed into the kind: the linear part is mg_bc_*'s operator with the mg_bc_set_faces mask
FAS_ON_COEFFICIENT = 1024   # OR-ed into the kind (not with 256; 512 stays refused): the linear part is mg_vc_*'s operator
COARSE_TOL, COARSE_FIXED = 0, 1
ARR_U, ARR_E, ARR_RHS, ARR_TMP, ARR_RES = 0, 1, 2, 3, 4
MG_COMM_ID_BYTES = 128
PROF_SMOOTH, PROF_SMOOTH_PROLONG, PROF_RESID_RESTRICT, PROF_PROLONG = 0, 1, 2, 3
PCG_K_UPDATE, PCG_K_DOTS, PCG_K_DIRECTION = 0, 1, 2
PCG_CONVERGED, PCG_MAXIT, PCG_BREAKDOWN = 0, 1, 2
MIXED_K_RESIDUAL, MIXED_K_CORRECT_RESIDUAL = 0, 1
MIXED_CONVERGED, MIXED_MAXIT, MIXED_NOT_FINITE = 0, 1, 2
MIXED_ON_CONSTANT, MIXED_ON_COEFFICIENT = 0, 2   # enum mg_mixed_operator (1 is kept for a faces-only operator and refused)
MIXED_INNER_PCG = 1 << 20                        # OR-ed into mg_mixed_solve's inner_cycles, only with MIXED_ON_COEFFICIENT
O4_CONVERGED, O4_MAXIT, O4_NOT_FINITE = 0, 1, 2
EIG_MAX_BLOCK = 8
EIG_X, EIG_AX, EIG_W, EIG_AW, EIG_P, EIG_AP = 0, 1, 2, 3, 4, 5
EIG_K_APPLY_GRAM, EIG_K_COMBINE = 0, 1
EIG_CONVERGED, EIG_MAXIT, EIG_NOT_FINITE = 0, 1, 2
EIG_ON_CONSTANT, EIG_ON_FACES, EIG_ON_COEFFICIENT = 0, 1, 2   # enum mg_eig_operator


def eig_operator(op):
    """include/mg_hip.h::MG_EIG_OPERATOR: what is OR-ed into mg_eig_solve's m or mg_eig_kernel's kernel"""
    return op << 8

def mixed_operator(op):
    """include/mg_hip.h::MG_MIXED_OPERATOR: what is OR-ed into mg_mixed_solve's inner_cycles or mg_mixed_kernel's kernel"""
    return op << 16

FMG_ON_CONSTANT, FMG_ON_FACES, FMG_ON_COEFFICIENT, FMG_ON_REACTION = 0, 1, 2, 3   # enum mg_fmg_operator


def fmg_operator(op):
    """include/mg_hip.h::MG_FMG_OPERATOR: what is OR-ed into mg_fmg's cycles_per_level or mg_fmg_prolong's coarse_level"""
    return op << 16

# enum mg_raw_space: the arrays mg_debug_raw_* (a test and debugging window, not a data path) can look at
RAW_LEVEL, RAW_VC, RAW_KRYLOV, RAW_MIXED, RAW_EIG, RAW_HEAT, RAW_O4 = 0, 1, 2, 3, 4, 5, 6


class MgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libmg_hip error {code}: {msg}")
        self.code = code


class MgDesc(C.Structure):
    """include/mg_desc.h::mg_desc"""

    _fields_ = [
        ("dim", C.c_int32), ("n", C.c_int32), ("levels", C.c_int32), ("dtype", C.c_int32),
        ("length", C.c_double), ("alpha", C.c_double),
        ("cycle", C.c_int32), ("smoother", C.c_int32),
        ("omega", C.c_double),
        ("nu_pre", C.c_int32), ("nu_post", C.c_int32),
        ("restriction", C.c_int32), ("coarse_mode", C.c_int32),
        ("coarse_maxit", C.c_int32), ("outer_pre_gs", C.c_int32),
        ("coarse_tol", C.c_double),
        ("aniso", C.c_double * 3),
        ("dist_min_n", C.c_int32), ("semi_xy", C.c_int32),
    ]


class MgCycleStats(C.Structure):
    _fields_ = [
        ("coarse_iters", C.c_int32), ("coarse_flag", C.c_int32),
        ("coarse_relres", C.c_double), ("fine_sumsq_r", C.c_double),
    ]


class MgFmgStats(C.Structure):
    """include/mg_hip.h::mg_fmg_stats (mg_fmg)"""

    _fields_ = [
        ("levels", C.c_int32), ("cycles_per_level", C.c_int32), ("coarse_iters", C.c_int32), ("coarse_flag", C.c_int32),
        ("relres", C.c_double),
    ]


class MgFasStats(C.Structure):
    """include/mg_hip.h::mg_fas_stats (mg_fas_solve)"""

    _fields_ = [
        ("status", C.c_int32), ("cycles", C.c_int32),
        ("norm0", C.c_double), ("norm", C.c_double),
    ]


class MgKrylovStats(C.Structure):
    """include/mg_hip.h::mg_krylov_stats (mg_pcg_solve)"""

    _fields_ = [
        ("iters", C.c_int32), ("status", C.c_int32),
        ("relres", C.c_double), ("relres_true", C.c_double),
    ]


class MgMixedStats(C.Structure):
    """include/mg_hip.h::mg_mixed_stats (mg_mixed_solve)"""

    _fields_ = [
        ("outer", C.c_int32), ("cycles", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32),
        ("relres", C.c_double),
    ]


class MgO4Stats(C.Structure):
    """include/mg_hip.h::mg_o4_stats (mg_o4_solve)"""

    _fields_ = [
        ("outer", C.c_int32), ("cycles", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32),
        ("relres", C.c_double),
    ]


class MgHeatStats(C.Structure):
    """include/mg_hip.h::mg_heat_stats (mg_heat_step)"""

    _fields_ = [("steps", C.c_int32), ("cycles", C.c_int32), ("time", C.c_double), ("relres", C.c_double)]


class MgDebugRawInfo(C.Structure):
    """include/mg_hip.h::mg_debug_raw_info (mg_debug_raw_layout)"""

    _fields_ = [("elem_size", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("pitch", C.c_int32),
                ("ghost", C.c_int32), ("allocated", C.c_int32), ("reserved", C.c_int32), ("elems", C.c_uint64)]


class MgEigStats(C.Structure):
    """include/mg_hip.h::mg_eig_stats (mg_eig_solve)"""

    _fields_ = [("iters", C.c_int32), ("status", C.c_int32), ("cycles", C.c_int32), ("restarts", C.c_int32),
                ("max_relres", C.c_double)]


def make_desc(dim=2, n=17, levels=2, dtype=MG_F64, length=10.0, alpha=1.0,
              cycle=CYCLE_SAWTOOTH, smoother=SMOOTH_JACOBI, omega=1.0, nu_pre=0, nu_post=5,
              restriction=RESTRICT_INJECT, coarse_mode=COARSE_TOL, coarse_maxit=2000,
              outer_pre_gs=2, coarse_tol=1e-1, aniso=(1.0, 1.0, 1.0), dist_min_n=0, semi_xy=0) -> MgDesc:
    """Defaults are the reference program's hard-coded values (include/mg_desc.h)."""
    d = MgDesc()
    d.dim, d.n, d.levels, d.dtype = dim, n, levels, dtype
    d.length, d.alpha = length, alpha
    d.cycle, d.smoother, d.omega = cycle, smoother, omega
    d.nu_pre, d.nu_post = nu_pre, nu_post
    d.restriction, d.coarse_mode = restriction, coarse_mode
    d.coarse_maxit, d.outer_pre_gs, d.coarse_tol = coarse_maxit, outer_pre_gs, coarse_tol
    d.aniso[0], d.aniso[1], d.aniso[2] = aniso
    d.dist_min_n = dist_min_n
    d.semi_xy = semi_xy
    return d


class MgP2POp(C.Structure):
    _fields_ = [("peer", C.c_int32), ("is_send", C.c_int32), ("buf", C.c_void_p), ("bytes", C.c_size_t)]


STAGE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p)
BATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(MgP2POp), C.c_int)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int)


class MgHostComm(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("batch", BATCH_FN), ("allreduce_sum", ALLREDUCE_FN)]


# every symbol include/mg_hip.h declares (tests check the library exports them all)
EXPORTS = [
    "mg_last_error", "mg_device_count", "mg_create", "mg_destroy", "mg_level_n", "mg_level_nz",
    "mg_level_coefficients", "mg_set_rhs", "mg_set_solution", "mg_get_solution", "mg_set_array",
    "mg_get_array", "mg_zero_array", "mg_set_array_device", "mg_get_array_device", "mg_smooth", "mg_residual", "mg_sumsq", "mg_restrict",
    "mg_prolong", "mg_correct", "mg_coarse_solve", "mg_coarse_solve_ex", "mg_cycle", "mg_cycle_async", "mg_solve", "mg_solve_lockstep",
    "mg_pcg_solve", "mg_pcg_kernel", "mg_fmg", "mg_fmg_prolong", "mg_subcycle", "mg_subcycle_root",
    "mg_mixed_set_rhs", "mg_mixed_set_solution", "mg_mixed_get_solution", "mg_mixed_solve", "mg_mixed_kernel",
    "mg_mixed_set_rhs_device", "mg_mixed_set_solution_device", "mg_mixed_get_solution_device",
    "mg_o4_residual", "mg_o4_correct_residual", "mg_o4_solve",
    "mg_vc_set_coefficient", "mg_vc_set_coefficient_device", "mg_vc_get_coefficient", "mg_vc_set_form", "mg_vc_residual", "mg_vc_smooth",
    "mg_vc_coarse_solve", "mg_vc_cycle", "mg_vc_solve", "mg_vc_pcg_solve", "mg_vc_direction",
    "mg_vc_set_faces", "mg_vc_get_faces", "mg_vc_restrict", "mg_vc_project",
    "mg_bc_set_faces", "mg_bc_get_faces", "mg_bc_set_form", "mg_bc_residual", "mg_bc_smooth", "mg_bc_restrict", "mg_bc_coarse_solve",
    "mg_bc_project", "mg_bc_cycle", "mg_bc_solve",
    "mg_fas_set_reaction", "mg_fas_get_reaction", "mg_fas_set_form", "mg_fas_residual", "mg_fas_smooth", "mg_fas_coarse_rhs", "mg_fas_correct",
    "mg_fas_coarse_solve", "mg_fas_cycle", "mg_fas_solve",
    "mg_set_shift", "mg_get_shift", "mg_heat_set_source", "mg_heat_set_source_device", "mg_heat_step", "mg_heat_rhs",
    "mg_vc_heat_rhs", "mg_bc_heat_rhs", "mg_fas_heat_rhs", "mg_vc_heat_step", "mg_bc_heat_step", "mg_fas_heat_step",
    "mg_eig_solve", "mg_eig_set_vector", "mg_eig_get_vector", "mg_eig_set_vector_device", "mg_eig_get_vector_device",
    "mg_eig_block", "mg_eig_kernel",
    "mg_set_stage_callback", "mg_sync", "mg_timer_start", "mg_timer_stop", "mg_profile_begin", "mg_profile_end", "mg_profile_fused", "mg_profile_get", "mg_comm_info", "mg_comm_stats", "mg_device_bytes",
    "mg_debug_raw_layout", "mg_debug_raw_copy", "mg_comm_unique_id", "mg_comm_selftest",
    "mg_create_distributed", "mg_create_distributed_hostcomm", "mg_create_distributed_dryrun", "mg_plan_slab",
]

_lib = None


def load(build_if_missing: bool = True) -> C.CDLL:
    """Loads (building first if stale) the in-tree libmg_hip.so."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB_PATH
    if build_if_missing:
        path = _build.build()
    if not os.path.exists(path):
        raise MgError(-2, f"{path} is missing: build it with `python -m multigrid_prj_amd.build`")
    L = C.CDLL(path)
    vp, i, dp = C.c_void_p, C.c_int, C.POINTER(C.c_double)
    L.mg_last_error.restype = C.c_char_p
    L.mg_device_count.argtypes = [C.POINTER(i)]
    L.mg_create.argtypes = [C.POINTER(MgDesc), i, C.POINTER(vp)]
    L.mg_destroy.argtypes = [vp]
    L.mg_level_n.argtypes = [vp, i, C.POINTER(i)]
    L.mg_level_nz.argtypes = [vp, i, C.POINTER(i)]
    L.mg_level_coefficients.argtypes = [vp, i, dp]
    L.mg_set_rhs.argtypes = [vp, vp]
    L.mg_set_solution.argtypes = [vp, vp]
    L.mg_get_solution.argtypes = [vp, vp]
    L.mg_set_array.argtypes = [vp, i, i, vp]
    L.mg_get_array.argtypes = [vp, i, i, vp]
    L.mg_zero_array.argtypes = [vp, i, i]
    L.mg_set_array_device.argtypes = [vp, i, i, vp, i, vp]
    L.mg_get_array_device.argtypes = [vp, i, i, vp, i, vp]
    L.mg_smooth.argtypes = [vp, i, i, i, i, i]
    L.mg_residual.argtypes = [vp, i, i, i, i, dp]
    L.mg_sumsq.argtypes = [vp, i, i, dp]
    L.mg_restrict.argtypes = [vp, i, i, i, i]
    L.mg_prolong.argtypes = [vp, i, i, i, i]
    L.mg_correct.argtypes = [vp, i, i]
    L.mg_coarse_solve.argtypes = [vp, i, i, i, C.POINTER(MgCycleStats)]
    L.mg_coarse_solve_ex.argtypes = [vp, i, i, i, i, i, C.c_double, i, C.POINTER(MgCycleStats)]
    L.mg_cycle.argtypes = [vp, C.POINTER(MgCycleStats)]
    L.mg_cycle_async.argtypes = [vp, i]
    L.mg_solve.argtypes = [vp, C.c_double, i, dp, i, C.POINTER(i), C.POINTER(MgCycleStats)]
    L.mg_solve_lockstep.argtypes = [vp, C.c_double, i, C.POINTER(i), i, dp, i, C.POINTER(i), C.POINTER(MgCycleStats)]
    L.mg_pcg_solve.argtypes = [vp, C.c_double, i, dp, i, C.POINTER(i), C.POINTER(MgKrylovStats)]
    L.mg_pcg_kernel.argtypes = [vp, i, C.c_double, C.POINTER(i), dp]
    L.mg_fmg.argtypes = [vp, i, C.POINTER(MgFmgStats)]
    L.mg_fmg_prolong.argtypes = [vp, i, i, i, i]
    L.mg_subcycle.argtypes = [vp, i, i, i, C.POINTER(MgCycleStats)]
    L.mg_subcycle_root.argtypes = [vp, C.POINTER(i)]
    L.mg_mixed_set_rhs.argtypes = [vp, vp]
    L.mg_mixed_set_solution.argtypes = [vp, vp]
    L.mg_mixed_get_solution.argtypes = [vp, vp]
    L.mg_mixed_set_rhs_device.argtypes = [vp, vp, i, vp]
    L.mg_mixed_set_solution_device.argtypes = [vp, vp, i, vp]
    L.mg_mixed_get_solution_device.argtypes = [vp, vp, i, vp]
    L.mg_mixed_solve.argtypes = [vp, C.c_double, i, i, dp, i, C.POINTER(i), C.POINTER(MgMixedStats)]
    L.mg_mixed_kernel.argtypes = [vp, i, C.c_double, C.c_double, i, i, dp]
    L.mg_o4_residual.argtypes = [vp, i, i, i, dp]
    L.mg_o4_correct_residual.argtypes = [vp, i, i, i, i, i, dp]
    L.mg_o4_solve.argtypes = [vp, C.c_double, i, i, dp, i, C.POINTER(i), C.POINTER(MgO4Stats)]
    L.mg_vc_set_coefficient.argtypes = [vp, vp]
    L.mg_vc_set_coefficient_device.argtypes = [vp, vp, i, vp]
    L.mg_vc_get_coefficient.argtypes = [vp, i, vp]
    L.mg_vc_set_form.argtypes = [vp, i]
    L.mg_vc_residual.argtypes = [vp, i, i, i, i, dp]
    L.mg_vc_smooth.argtypes = [vp, i, i, i, i, i]
    L.mg_vc_coarse_solve.argtypes = [vp, i, i, i, C.POINTER(MgCycleStats)]
    L.mg_vc_cycle.argtypes = [vp, C.POINTER(MgCycleStats)]
    L.mg_vc_solve.argtypes = [vp, C.c_double, i, dp, i, C.POINTER(i), C.POINTER(MgCycleStats)]
    L.mg_vc_pcg_solve.argtypes = [vp, C.c_double, i, dp, i, C.POINTER(i), C.POINTER(MgKrylovStats)]
    L.mg_vc_direction.argtypes = [vp, C.c_double, i, i, i, i, dp]
    L.mg_vc_set_faces.argtypes = [vp, i]
    L.mg_vc_get_faces.argtypes = [vp, C.POINTER(i)]
    L.mg_vc_restrict.argtypes = [vp, i, i, i, i]
    L.mg_vc_project.argtypes = [vp, i, i, dp]
    L.mg_bc_set_faces.argtypes = [vp, i]
    L.mg_bc_get_faces.argtypes = [vp, C.POINTER(i)]
    L.mg_bc_set_form.argtypes = [vp, i]
    L.mg_bc_residual.argtypes = [vp, i, i, i, i, dp]
    L.mg_bc_smooth.argtypes = [vp, i, i, i, i, i]
    L.mg_bc_restrict.argtypes = [vp, i, i, i, i]
    L.mg_bc_coarse_solve.argtypes = [vp, i, i, i, C.POINTER(MgCycleStats)]
    L.mg_bc_project.argtypes = [vp, i, i, dp]
    L.mg_bc_cycle.argtypes = [vp, C.POINTER(MgCycleStats)]
    L.mg_bc_solve.argtypes = [vp, C.c_double, i, dp, i, C.POINTER(i), C.POINTER(MgCycleStats)]
    L.mg_fas_set_reaction.argtypes = [vp, i, C.c_double]
    L.mg_fas_get_reaction.argtypes = [vp, C.POINTER(i), dp]
    L.mg_fas_set_form.argtypes = [vp, i]
    L.mg_fas_residual.argtypes = [vp, i, i, i, i, dp]
    L.mg_fas_smooth.argtypes = [vp, i, i, i, i, i]
    L.mg_fas_coarse_rhs.argtypes = [vp, i]
    L.mg_fas_correct.argtypes = [vp, i]
    L.mg_fas_coarse_solve.argtypes = [vp, i, i, i, C.POINTER(MgCycleStats)]
    L.mg_fas_cycle.argtypes = [vp, C.POINTER(MgCycleStats)]
    L.mg_fas_solve.argtypes = [vp, C.c_double, C.c_double, i, dp, i, C.POINTER(i), C.POINTER(MgFasStats)]
    L.mg_set_shift.argtypes = [vp, C.c_double]
    L.mg_get_shift.argtypes = [vp, dp]
    L.mg_heat_set_source.argtypes = [vp, vp]
    L.mg_heat_set_source_device.argtypes = [vp, vp, i, vp]
    L.mg_heat_step.argtypes = [vp, C.c_double, C.c_double, i, i, C.POINTER(MgHeatStats)]
    L.mg_heat_rhs.argtypes = [vp, C.c_double, C.c_double, i, i]
    for fam in ("vc", "bc", "fas"):
        getattr(L, f"mg_{fam}_heat_rhs").argtypes = [vp, C.c_double, C.c_double, i, i]
        getattr(L, f"mg_{fam}_heat_step").argtypes = [vp, C.c_double, C.c_double, i, i, C.POINTER(MgHeatStats)]
    L.mg_eig_solve.argtypes = [vp, i, i, C.c_double, i, dp, dp, dp, i, C.POINTER(i), C.POINTER(MgEigStats)]
    L.mg_eig_set_vector.argtypes = [vp, i, i, vp]
    L.mg_eig_get_vector.argtypes = [vp, i, i, vp]
    L.mg_eig_set_vector_device.argtypes = [vp, i, i, vp, i, vp]
    L.mg_eig_get_vector_device.argtypes = [vp, i, i, vp, i, vp]
    L.mg_eig_block.argtypes = [vp, C.POINTER(i)]
    L.mg_eig_kernel.argtypes = [vp, i, i, i, dp, dp, dp, dp, dp]
    L.mg_set_stage_callback.argtypes = [vp, STAGE_FN, vp]
    L.mg_sync.argtypes = [vp]
    L.mg_timer_start.argtypes = [vp]
    L.mg_timer_stop.argtypes = [vp, dp]
    L.mg_profile_begin.argtypes = [vp]
    L.mg_profile_end.argtypes = [vp, dp, C.POINTER(i)]
    L.mg_profile_fused.argtypes = [vp, dp, C.POINTER(i)]
    L.mg_profile_get.argtypes = [vp, i, dp, C.POINTER(i)]
    L.mg_comm_info.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(C.c_char_p)]
    L.mg_comm_stats.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.mg_device_bytes.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.mg_debug_raw_layout.argtypes = [vp, i, i, i, C.POINTER(MgDebugRawInfo)]
    L.mg_debug_raw_copy.argtypes = [vp, i, i, i, vp, C.c_size_t, i]
    L.mg_comm_unique_id.argtypes = [vp]
    L.mg_comm_selftest.argtypes = [C.c_size_t]
    L.mg_create_distributed.argtypes = [C.POINTER(MgDesc), i, i, i, vp, C.POINTER(vp)]
    L.mg_create_distributed_hostcomm.argtypes = [C.POINTER(MgDesc), i, i, i, C.POINTER(MgHostComm), C.POINTER(vp)]
    L.mg_create_distributed_dryrun.argtypes = [C.POINTER(MgDesc), i, i, i, C.POINTER(vp)]
    L.mg_plan_slab.argtypes = [C.POINTER(MgDesc), i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise MgError(rc, load().mg_last_error().decode())


def device_count() -> int:
    n = C.c_int(0)
    _check(load().mg_device_count(C.byref(n)))
    return n.value


def plan_slab(desc: MgDesc, nranks: int, rank: int, level: int):
    """Host-only: (z0, nz, first_gathered_level) of `rank` on `level`."""
    z0, nz, fg = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(load().mg_plan_slab(C.byref(desc), nranks, rank, level, C.byref(z0), C.byref(nz), C.byref(fg)))
    return z0.value, nz.value, fg.value


def comm_selftest(nbytes: int = 1 << 20):
    """RCCL transport smoke test on the current device (one rank, send/recv to self)."""
    _check(load().mg_comm_selftest(nbytes))


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(MG_COMM_ID_BYTES)
    _check(load().mg_comm_unique_id(buf))
    return buf.raw


def device_view(obj, shape, writable=False):
    """(pointer, MG_F64 | MG_F32) of a dense device array that exposes __cuda_array_interface__ (a torch-ROCm tensor does; so
    does anything else that follows the protocol -- the package itself imports none of them). ValueError, before any
    library call, unless it is a C-contiguous float64 / float32 array of exactly `shape` with a data pointer (and not
    read-only where `writable` is asked for)."""
    cai = getattr(obj, "__cuda_array_interface__", None)
    if not isinstance(cai, dict):
        raise ValueError(f"{type(obj).__name__} has no __cuda_array_interface__: a device array (a torch tensor in HBM) is expected")
    dtype = {"<f8": MG_F64, "<f4": MG_F32}.get(cai.get("typestr"))
    if dtype is None:
        raise ValueError(f"typestr {cai.get('typestr')!r}: only '<f8' and '<f4' device arrays can be copied")
    got = tuple(int(v) for v in cai.get("shape", ()))
    if got != tuple(int(v) for v in shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {got}")
    strides = cai.get("strides")
    if strides is not None:
        want, step = [], 8 if dtype == MG_F64 else 4
        for extent in reversed(got):
            want.append(step); step *= extent
        if tuple(int(v) for v in strides) != tuple(reversed(want)):
            raise ValueError(f"strides {tuple(strides)} are not C-contiguous (expected {tuple(reversed(want))}): pass a contiguous array")
    ptr, readonly = cai.get("data", (0, True))
    if not ptr:
        raise ValueError("null data pointer")
    if writable and readonly:
        raise ValueError("the device array is read-only")
    return int(ptr), dtype


class Solver:
    """One GPU-resident hierarchy. Mirrors the operator vocabulary of the reference
    (`x * smoother`, `x * RES`, interpolate, Solve, SawtoothMGIteration, main loop)."""

    def __init__(self, desc: MgDesc, device: int = -1, rank: int = 0, nranks: int = 1, comm_id: bytes | None = None,
                 host_comm: "MgHostComm | None" = None, dry: bool = False):
        self.lib = load()
        self.d = desc
        self.np = np.float64 if desc.dtype == MG_F64 else np.float32
        self.h = C.c_void_p()
        self.rank, self.nranks = rank, nranks
        self._host_comm = host_comm  # keep the callbacks alive
        if nranks > 1 and dry:   # measurement only: no peers, nothing moves
            _check(self.lib.mg_create_distributed_dryrun(C.byref(desc), device, rank, nranks, C.byref(self.h)))
        elif nranks > 1 and host_comm is not None:
            _check(self.lib.mg_create_distributed_hostcomm(C.byref(desc), device, rank, nranks, C.byref(host_comm), C.byref(self.h)))
        elif nranks > 1:
            buf = C.create_string_buffer(comm_id, MG_COMM_ID_BYTES)
            _check(self.lib.mg_create_distributed(C.byref(desc), device, rank, nranks, buf, C.byref(self.h)))
        else:
            _check(self.lib.mg_create(C.byref(desc), device, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- geometry
    def level_n(self, level: int) -> int:
        n = C.c_int(0); _check(self.lib.mg_level_n(self.h, level, C.byref(n))); return n.value

    def level_nz(self, level: int) -> int:
        n = C.c_int(0); _check(self.lib.mg_level_nz(self.h, level, C.byref(n))); return n.value

    def level_shape(self, level: int):
        """Host shape of this rank's part of a level (the local z-slab when distributed)."""
        n = self.level_n(level)
        return (n, n) if self.d.dim == 2 else (self.level_nz(level), n, n)

    def level_coefficients(self, level: int):
        out = (C.c_double * 4)(); _check(self.lib.mg_level_coefficients(self.h, level, out)); return tuple(out)

    # -- data movement
    def _host(self, a, level):
        a = np.ascontiguousarray(a, self.np)
        if a.shape != self.level_shape(level):
            raise ValueError(f"expected shape {self.level_shape(level)}, got {a.shape}")
        return a

    def set_array(self, which, level, a):
        a = self._host(a, level); _check(self.lib.mg_set_array(self.h, which, level, a.ctypes.data_as(C.c_void_p)))

    def get_array(self, which, level):
        a = np.empty(self.level_shape(level), self.np)
        _check(self.lib.mg_get_array(self.h, which, level, a.ctypes.data_as(C.c_void_p))); return a

    def zero_array(self, which, level):
        _check(self.lib.mg_zero_array(self.h, which, level))

    def set_rhs(self, b): self.set_array(ARR_RHS, 0, b)
    def set_solution(self, u): self.set_array(ARR_U, 0, u)
    def get_solution(self): return self.get_array(ARR_U, 0)

    # -- the same from / into dense DEVICE arrays (torch tensors in HBM, ...), ordered against the caller's stream: `stream` is
    # the integer handle of a HIP stream (torch.cuda.current_stream().cuda_stream); 0 = the default stream, torch's default.
    # No host synchronisation: a set may be followed at once by work on `stream` that overwrites the source, a get by work
    # on `stream` that reads `out`; host code synchronises the stream (or calls sync()) before it looks at `out`.
    def set_array_device(self, which, level, obj, stream=0):
        ptr, dt = device_view(obj, self.level_shape(level))
        _check(self.lib.mg_set_array_device(self.h, which, level, ptr, dt, stream or None))

    def get_array_device(self, which, level, out, stream=0):
        ptr, dt = device_view(out, self.level_shape(level), writable=True)
        _check(self.lib.mg_get_array_device(self.h, which, level, ptr, dt, stream or None))

    def set_rhs_device(self, b, stream=0): self.set_array_device(ARR_RHS, 0, b, stream)
    def set_solution_device(self, u, stream=0): self.set_array_device(ARR_U, 0, u, stream)
    def get_solution_device(self, out, stream=0): self.get_array_device(ARR_U, 0, out, stream)

    # -- operators
    def smooth(self, level, smoother, sweeps, arr_x, arr_rhs):
        _check(self.lib.mg_smooth(self.h, level, smoother, sweeps, arr_x, arr_rhs))

    def residual(self, level, arr_x, arr_rhs, arr_r=-1) -> float:
        s = C.c_double(0); _check(self.lib.mg_residual(self.h, level, arr_x, arr_rhs, arr_r, C.byref(s))); return s.value

    def residual_async(self, level, arr_x, arr_rhs, arr_r=-1):
        _check(self.lib.mg_residual(self.h, level, arr_x, arr_rhs, arr_r, None))

    def sumsq(self, level, arr) -> float:
        s = C.c_double(0); _check(self.lib.mg_sumsq(self.h, level, arr, C.byref(s))); return s.value

    def restrict(self, fine_level, kind, arr_src, arr_dst):
        _check(self.lib.mg_restrict(self.h, fine_level, kind, arr_src, arr_dst))

    def prolong(self, coarse_level, add, arr_src, arr_dst):
        _check(self.lib.mg_prolong(self.h, coarse_level, int(add), arr_src, arr_dst))

    def correct(self, arr_u=ARR_U, arr_e=ARR_E):
        _check(self.lib.mg_correct(self.h, arr_u, arr_e))

    def coarse_solve(self, level, arr_x, arr_rhs) -> MgCycleStats:
        st = MgCycleStats(); _check(self.lib.mg_coarse_solve(self.h, level, arr_x, arr_rhs, C.byref(st))); return st

    def coarse_solve_ex(self, level, arr_x, arr_rhs, smoother, maxit, tol, fixed=False) -> MgCycleStats:
        st = MgCycleStats()
        _check(self.lib.mg_coarse_solve_ex(self.h, level, arr_x, arr_rhs, smoother, maxit, tol, int(fixed), C.byref(st))); return st

    def cycle(self) -> MgCycleStats:
        st = MgCycleStats(); _check(self.lib.mg_cycle(self.h, C.byref(st))); return st

    def cycle_async(self, count=1):
        _check(self.lib.mg_cycle_async(self.h, count))

    def solve(self, tol=1e-11, maxit=1000):
        hist = (C.c_double * (maxit + 1))(); nh = C.c_int(0)
        stats = (MgCycleStats * max(maxit, 1))()
        _check(self.lib.mg_solve(self.h, tol, maxit, hist, maxit + 1, C.byref(nh), stats))
        return np.array(hist[:nh.value]), list(stats[:nh.value - 1])

    def solve_lockstep(self, coarse_counts, tol=1e-11, maxit=1000):
        """mg_solve with outer iteration i's coarse solve spending exactly coarse_counts[i] sweeps"""
        hist = (C.c_double * (maxit + 1))(); nh = C.c_int(0)
        stats = (MgCycleStats * max(maxit, 1))()
        cnt = (C.c_int * max(len(coarse_counts), 1))(*[int(c) for c in coarse_counts])
        _check(self.lib.mg_solve_lockstep(self.h, tol, maxit, cnt, len(coarse_counts), hist, maxit + 1, C.byref(nh), stats))
        return np.array(hist[:nh.value]), list(stats[:nh.value - 1])

    def pcg_solve(self, tol=1e-11, maxit=1000):
        """mg_pcg_solve: multigrid-preconditioned flexible CG on level 0 (b = RHS, x0 = U; U holds x on return)
        -> (hist, MgKrylovStats); hist[k] = ||r_k|| / ||b||"""
        hist = (C.c_double * (maxit + 1))(); nh = C.c_int(0); st = MgKrylovStats()
        _check(self.lib.mg_pcg_solve(self.h, tol, maxit, hist, maxit + 1, C.byref(nh), C.byref(st)))
        return np.array(hist[:min(nh.value, maxit + 1)]), st

    def pcg_kernel(self, kernel, scalar, arrs):
        """mg_pcg_kernel: one vector kernel of pcg_solve on level-0 arrays (PCG_K_*) -> (dot0, dot1)"""
        a = (C.c_int * 4)(*(list(arrs) + [0] * (4 - len(arrs)))); dots = (C.c_double * 2)()
        _check(self.lib.mg_pcg_kernel(self.h, kernel, scalar, a, dots))
        return dots[0], dots[1]

    def fmg(self, cycles_per_level=1, op=None):
        """mg_fmg: full multigrid (nested iteration) from the coarsest grid up, cubic interpolation of the solution and
        cycles_per_level cycles of the descriptor's kind (V, W or F) per level; U(0) holds the iterate on return (its incoming content is ignored)
        -> MgFmgStats. op (FMG_ON_*): the pass on a family's operator as the handle holds it at the call -- FMG_ON_FACES
        mg_bc_*'s, FMG_ON_COEFFICIENT mg_vc_*'s, FMG_ON_REACTION mg_fas_*'s -- OR-ed into cycles_per_level as MG_FMG_OPERATOR
        does; None passes cycles_per_level as it is"""
        st = MgFmgStats()
        _check(self.lib.mg_fmg(self.h, cycles_per_level if op is None else cycles_per_level | fmg_operator(op), C.byref(st)))
        return st

    def fmg_prolong(self, coarse_level, arr_src, arr_dst, arr_bnd=-1, op=None):
        """mg_fmg_prolong: arr_dst(coarse_level - 1) = Pi arr_src(coarse_level), the FMG (cubic) interpolation; fine
        Dirichlet nodes from arr_bnd (< 0: interpolated too). op (FMG_ON_*): mirrored at the Neumann faces of that family's
        mask, arr_bnd on the mask's Dirichlet nodes; OR-ed into coarse_level as MG_FMG_OPERATOR does"""
        _check(self.lib.mg_fmg_prolong(self.h, coarse_level if op is None else coarse_level | fmg_operator(op), arr_src, arr_dst, arr_bnd))

    def subcycle(self, level, kind, path=0) -> MgCycleStats:
        """mg_subcycle: one cyc(level, kind) (CYCLE_V / _W / _F) on U(level), RHS(level) from the U it holds; path 0: launch
        by launch, path 1: the one-launch LDS kernel rooted at `level`"""
        st = MgCycleStats(); _check(self.lib.mg_subcycle(self.h, level, kind, path, C.byref(st))); return st

    def subcycle_root(self) -> int:
        """mg_subcycle_root: the level the handle's cycles hand to the LDS kernel, -1: none"""
        r = C.c_int(0); _check(self.lib.mg_subcycle_root(self.h, C.byref(r))); return r.value

    # -- mixed-precision defect correction: fp64 u / b beside an MG_F32 hierarchy (float64 arrays whatever the handle's dtype)
    def _host64(self, a):
        a = np.ascontiguousarray(a, np.float64)
        if a.shape != self.level_shape(0):
            raise ValueError(f"expected shape {self.level_shape(0)}, got {a.shape}")
        return a

    def mixed_set_rhs(self, b):
        b = self._host64(b); _check(self.lib.mg_mixed_set_rhs(self.h, b.ctypes.data_as(C.c_void_p)))

    def mixed_set_solution(self, u):
        u = self._host64(u); _check(self.lib.mg_mixed_set_solution(self.h, u.ctypes.data_as(C.c_void_p)))

    def mixed_get_solution(self):
        u = np.empty(self.level_shape(0), np.float64)
        _check(self.lib.mg_mixed_get_solution(self.h, u.ctypes.data_as(C.c_void_p))); return u

    def mixed_set_rhs_device(self, b, stream=0):
        ptr, dt = device_view(b, self.level_shape(0))
        _check(self.lib.mg_mixed_set_rhs_device(self.h, ptr, dt, stream or None))

    def mixed_set_solution_device(self, u, stream=0):
        ptr, dt = device_view(u, self.level_shape(0))
        _check(self.lib.mg_mixed_set_solution_device(self.h, ptr, dt, stream or None))

    def mixed_get_solution_device(self, out, stream=0):
        ptr, dt = device_view(out, self.level_shape(0), writable=True)
        _check(self.lib.mg_mixed_get_solution_device(self.h, ptr, dt, stream or None))

    def mixed_solve(self, tol=1e-11, maxit=100, inner_cycles=4, op=MIXED_ON_CONSTANT, inner_pcg=False):
        """mg_mixed_solve: fp64 defect correction over the fp32 cycles of this (MG_F32) handle, `maxit` corrections of
        `inner_cycles` cycles at most -> (hist, MgMixedStats); hist[k] = the true fp64 ||b - A u_k|| / ||b||.
        op=MIXED_ON_COEFFICIENT: on mg_vc_*'s operator as the handle holds it (coefficient, shift, vc_set_faces mask);
        inner_pcg: `inner_cycles` iterations of vc_pcg_solve's CG per correction instead of cycles. Both are OR-ed into
        inner_cycles as MG_MIXED_OPERATOR / MG_MIXED_INNER_PCG do; the defaults pass inner_cycles as it is"""
        cap = max(maxit, 0) + 1
        hist = (C.c_double * cap)(); nh = C.c_int(0); st = MgMixedStats()
        arg = inner_cycles | mixed_operator(op) | (MIXED_INNER_PCG if inner_pcg else 0)
        _check(self.lib.mg_mixed_solve(self.h, tol, maxit, arg, hist, cap, C.byref(nh), C.byref(st)))
        return np.array(hist[:min(nh.value, cap)]), st

    def mixed_kernel(self, kernel, scale_in, scale_out, arr_e32, arr_r32, op=MIXED_ON_CONSTANT) -> float:
        """mg_mixed_kernel: one of the two fp64-in / fp32-out kernels of mixed_solve (MIXED_K_*) -> sum r^2; op as in mixed_solve"""
        s = C.c_double(0)
        _check(self.lib.mg_mixed_kernel(self.h, kernel | mixed_operator(op), scale_in, scale_out, arr_e32, arr_r32, C.byref(s))); return s.value

    # -- fourth-order defect correction on level 0
    def o4_residual(self, arr_u, arr_b, arr_r=-1) -> float:
        """mg_o4_residual: arr_r(0) = arr_b(0) - (sigma I + A4) arr_u(0) with the fourth-order operator (arr_r < 0: norm
        only) -> sum r^2"""
        s = C.c_double(0); _check(self.lib.mg_o4_residual(self.h, arr_u, arr_b, arr_r, C.byref(s))); return s.value

    def o4_correct_residual(self, arr_u, arr_e, arr_b, arr_unew, arr_r) -> float:
        """mg_o4_correct_residual: arr_unew = arr_u + arr_e (interior nodes), arr_r = arr_b - (sigma I + A4) arr_unew in
        one launch; five distinct level-0 arrays -> sum r^2"""
        s = C.c_double(0)
        _check(self.lib.mg_o4_correct_residual(self.h, arr_u, arr_e, arr_b, arr_unew, arr_r, C.byref(s))); return s.value

    def o4_solve(self, tol=1e-10, maxit=60, inner_cycles=1):
        """mg_o4_solve: fourth-order defect correction over this handle's cycles (b = RHS, first iterate = U; U holds the
        answer on return), `maxit` corrections of `inner_cycles` cycles at most -> (hist, MgO4Stats);
        hist[k] = ||b - (sigma I + A4) u_k|| / ||b||"""
        cap = max(maxit, 0) + 1
        hist = (C.c_double * cap)(); nh = C.c_int(0); st = MgO4Stats()
        _check(self.lib.mg_o4_solve(self.h, tol, maxit, inner_cycles, hist, cap, C.byref(nh), C.byref(st)))
        return np.array(hist[:min(nh.value, cap)]), st

    # -- diagonal shift and the implicit heat-equation stepper
    def set_shift(self, sigma: float):
        """mg_set_shift: the handle works on sigma I + A from here on (sigma >= 0; 0 restores the creation state)"""
        _check(self.lib.mg_set_shift(self.h, sigma))

    def get_shift(self) -> float:
        s = C.c_double(0); _check(self.lib.mg_get_shift(self.h, C.byref(s))); return s.value

    # -- variable-coefficient diffusion sigma u - div(a grad u) (mg_vc_*, include/mg_hip.h)
    def vc_set_coefficient(self, a):
        """mg_vc_set_coefficient: the nodal coefficient a > 0 of level 0 (coarser levels: its full weighting)"""
        a = self._host(a, 0); _check(self.lib.mg_vc_set_coefficient(self.h, a.ctypes.data_as(C.c_void_p)))

    def vc_set_coefficient_device(self, a, stream=0):
        """mg_vc_set_coefficient_device: the same from a dense device array on the caller's stream"""
        ptr, dt = device_view(a, self.level_shape(0))
        _check(self.lib.mg_vc_set_coefficient_device(self.h, ptr, dt, stream or None))

    def vc_get_coefficient(self, level):
        a = np.empty(self.level_shape(level), self.np)
        _check(self.lib.mg_vc_get_coefficient(self.h, level, a.ctypes.data_as(C.c_void_p))); return a

    def vc_set_form(self, form):
        """mg_vc_set_form (tests and measurement tools): 1 = the plain kernels on every level, 0 = the default"""
        _check(self.lib.mg_vc_set_form(self.h, int(form)))

    def vc_residual(self, level, arr_x, arr_rhs, arr_r=-1) -> float:
        s = C.c_double(0); _check(self.lib.mg_vc_residual(self.h, level, arr_x, arr_rhs, arr_r, C.byref(s))); return s.value

    def vc_smooth(self, level, smoother, sweeps, arr_x, arr_rhs):
        _check(self.lib.mg_vc_smooth(self.h, level, smoother, sweeps, arr_x, arr_rhs))

    def vc_coarse_solve(self, level, arr_x, arr_rhs) -> MgCycleStats:
        st = MgCycleStats(); _check(self.lib.mg_vc_coarse_solve(self.h, level, arr_x, arr_rhs, C.byref(st))); return st

    def vc_cycle(self) -> MgCycleStats:
        st = MgCycleStats(); _check(self.lib.mg_vc_cycle(self.h, C.byref(st))); return st

    def vc_solve(self, tol=1e-11, maxit=1000):
        """mg_vc_solve -> (hist, per-cycle MgCycleStats)"""
        hist = (C.c_double * (maxit + 1))(); nh = C.c_int(0)
        stats = (MgCycleStats * max(maxit, 1))()
        _check(self.lib.mg_vc_solve(self.h, tol, maxit, hist, maxit + 1, C.byref(nh), stats))
        return np.array(hist[:nh.value]), list(stats[:nh.value - 1])

    def vc_pcg_solve(self, tol=1e-11, maxit=1000):
        """mg_vc_pcg_solve: flexible CG on L preconditioned by one mg_vc_cycle -> (hist, MgKrylovStats)"""
        hist = (C.c_double * (maxit + 1))(); nh = C.c_int(0); st = MgKrylovStats()
        _check(self.lib.mg_vc_pcg_solve(self.h, tol, maxit, hist, maxit + 1, C.byref(nh), C.byref(st)))
        return np.array(hist[:min(nh.value, maxit + 1)]), st

    def vc_direction(self, beta, arr_z, arr_p, arr_pn, arr_q) -> float:
        """mg_vc_direction: arr_pn = arr_z + beta arr_p, arr_q = L arr_pn (both 0 on Dirichlet nodes) -> sum pn.q"""
        s = C.c_double(0); _check(self.lib.mg_vc_direction(self.h, beta, arr_z, arr_p, arr_pn, arr_q, C.byref(s))); return s.value

    # Neumann faces of the variable-coefficient operator: a face mask of its own (mg_vc_set_faces, include/mg_hip.h)
    def vc_set_faces(self, mask):
        """mg_vc_set_faces: the Neumann faces (FACE_* bits) of mg_vc_*, 0 = all Dirichlet; independent of bc_set_faces"""
        _check(self.lib.mg_vc_set_faces(self.h, int(mask)))

    def vc_get_faces(self) -> int:
        """mg_vc_get_faces: the mask of vc_set_faces"""
        m = C.c_int(0); _check(self.lib.mg_vc_get_faces(self.h, C.byref(m))); return m.value

    def vc_restrict(self, fine_level, kind, arr_src, arr_dst):
        """mg_vc_restrict: bc_restrict with the vc mask"""
        _check(self.lib.mg_vc_restrict(self.h, fine_level, kind, arr_src, arr_dst))

    def vc_project(self, level, arr) -> float:
        """mg_vc_project: subtracts the w-weighted mean (the vc mask's weights) from every node and returns it"""
        m = C.c_double(0); _check(self.lib.mg_vc_project(self.h, level, arr, C.byref(m))); return m.value

    # -- Neumann faces: the constant operator with zero-flux walls on the faces of a mask (mg_bc_*, include/mg_hip.h)
    def bc_set_faces(self, mask):
        """mg_bc_set_faces: the set of Neumann faces (FACE_* bits), 0 = all Dirichlet"""
        _check(self.lib.mg_bc_set_faces(self.h, int(mask)))

    def bc_get_faces(self) -> int:
        m = C.c_int(0); _check(self.lib.mg_bc_get_faces(self.h, C.byref(m))); return m.value

    def bc_set_form(self, form):
        """mg_bc_set_form (tests and measurement tools): 1 = the plain kernels on every level, 0 = the default"""
        _check(self.lib.mg_bc_set_form(self.h, int(form)))

    def bc_residual(self, level, arr_x, arr_rhs, arr_r=-1) -> float:
        s = C.c_double(0); _check(self.lib.mg_bc_residual(self.h, level, arr_x, arr_rhs, arr_r, C.byref(s))); return s.value

    def bc_smooth(self, level, smoother, sweeps, arr_x, arr_rhs):
        _check(self.lib.mg_bc_smooth(self.h, level, smoother, sweeps, arr_x, arr_rhs))

    def bc_restrict(self, fine_level, kind, arr_src, arr_dst):
        _check(self.lib.mg_bc_restrict(self.h, fine_level, kind, arr_src, arr_dst))

    def bc_coarse_solve(self, level, arr_x, arr_rhs) -> MgCycleStats:
        st = MgCycleStats(); _check(self.lib.mg_bc_coarse_solve(self.h, level, arr_x, arr_rhs, C.byref(st))); return st

    def bc_project(self, level, arr) -> float:
        """mg_bc_project: subtracts the w-weighted mean from every node and returns it"""
        m = C.c_double(0); _check(self.lib.mg_bc_project(self.h, level, arr, C.byref(m))); return m.value

    def bc_cycle(self) -> MgCycleStats:
        st = MgCycleStats(); _check(self.lib.mg_bc_cycle(self.h, C.byref(st))); return st

    def bc_solve(self, tol=1e-11, maxit=1000):
        """mg_bc_solve -> (hist, per-cycle MgCycleStats)"""
        hist = (C.c_double * (maxit + 1))(); nh = C.c_int(0)
        stats = (MgCycleStats * max(maxit, 1))()
        _check(self.lib.mg_bc_solve(self.h, tol, maxit, hist, maxit + 1, C.byref(nh), stats))
        return np.array(hist[:nh.value]), list(stats[:nh.value - 1])

    # -- nonlinear solves by the full approximation scheme: (sigma I + A) u + gamma g(u) = f (mg_fas_*, include/mg_hip.h)
    def fas_set_reaction(self, kind, gamma):
        """mg_fas_set_reaction: g = u^3 (FAS_CUBIC) or exp(u) (FAS_EXP) and its factor gamma. The kind alone: the handle's constant
        operator, all faces Dirichlet; OR-ed with FAS_ON_FACES: Neumann faces by bc_set_faces; OR-ed with FAS_ON_COEFFICIENT:
        sigma u - div(a grad u) + gamma g(u) with the coefficient of vc_set_coefficient, the shift and the faces of vc_set_faces,
        all read at call time (a compute call without a coefficient raises MgError -4). The two flags exclude each other."""
        _check(self.lib.mg_fas_set_reaction(self.h, int(kind), float(gamma)))

    def fas_get_reaction(self):
        """-> (kind, gamma)"""
        k = C.c_int(0); g = C.c_double(0); _check(self.lib.mg_fas_get_reaction(self.h, C.byref(k), C.byref(g))); return k.value, g.value

    def fas_set_form(self, form):
        """mg_fas_set_form (tests and measurement tools): 1 = the plain kernels on every level, 0 = the default"""
        _check(self.lib.mg_fas_set_form(self.h, int(form)))

    def fas_residual(self, level, arr_x, arr_rhs, arr_r=-1) -> float:
        s = C.c_double(0); _check(self.lib.mg_fas_residual(self.h, level, arr_x, arr_rhs, arr_r, C.byref(s))); return s.value

    def fas_smooth(self, level, smoother, sweeps, arr_x, arr_rhs):
        _check(self.lib.mg_fas_smooth(self.h, level, smoother, sweeps, arr_x, arr_rhs))

    def fas_coarse_rhs(self, fine_level):
        """mg_fas_coarse_rhs: TMP(l), U(l) -> U, E, RHS of level l + 1"""
        _check(self.lib.mg_fas_coarse_rhs(self.h, fine_level))

    def fas_correct(self, fine_level):
        """mg_fas_correct: U(l) += P (U(l+1) - E(l+1)); E(l+1) holds the difference afterwards"""
        _check(self.lib.mg_fas_correct(self.h, fine_level))

    def fas_coarse_solve(self, level, arr_x, arr_rhs) -> MgCycleStats:
        st = MgCycleStats(); _check(self.lib.mg_fas_coarse_solve(self.h, level, arr_x, arr_rhs, C.byref(st))); return st

    def fas_cycle(self) -> MgCycleStats:
        st = MgCycleStats(); _check(self.lib.mg_fas_cycle(self.h, C.byref(st))); return st

    def fas_solve(self, rtol=1e-10, atol=0.0, maxit=50):
        """mg_fas_solve -> (hist of absolute residual norms, MgFasStats)"""
        hist = (C.c_double * (maxit + 1))(); nh = C.c_int(0); st = MgFasStats()
        _check(self.lib.mg_fas_solve(self.h, rtol, atol, maxit, hist, maxit + 1, C.byref(nh), C.byref(st)))
        return np.array(hist[:nh.value]), st

    def heat_set_source(self, f):
        """mg_heat_set_source: the source term f of u_t = -A0 u + f (level-0 array of the handle's dtype); None: f = 0"""
        if f is None:
            _check(self.lib.mg_heat_set_source(self.h, None))
        else:
            f = self._host(f, 0); _check(self.lib.mg_heat_set_source(self.h, f.ctypes.data_as(C.c_void_p)))

    def heat_set_source_device(self, f, stream=0):
        """mg_heat_set_source_device: f from a dense device array on the caller's stream; None: f = 0"""
        if f is None:
            _check(self.lib.mg_heat_set_source_device(self.h, None, self.d.dtype, stream or None))
        else:
            ptr, dt = device_view(f, self.level_shape(0))
            _check(self.lib.mg_heat_set_source_device(self.h, ptr, dt, stream or None))

    def heat_step(self, dt, theta=1.0, nsteps=1, cycles_per_step=1) -> MgHeatStats:
        """mg_heat_step: nsteps theta-scheme steps of u_t = -A0 u + f from U, cycles_per_step cycles each, no host
        synchronisation in between; U holds the result, the shift 1 / (theta dt) stays set -> MgHeatStats"""
        st = MgHeatStats()
        _check(self.lib.mg_heat_step(self.h, dt, theta, nsteps, cycles_per_step, C.byref(st)))
        return st

    def heat_rhs(self, dt, theta, arr_u=ARR_U, arr_dst=ARR_RHS):
        """mg_heat_rhs: arr_dst(0) = the right-hand side of one theta-scheme step built from arr_u(0)"""
        _check(self.lib.mg_heat_rhs(self.h, dt, theta, arr_u, arr_dst))

    # -- the same steps of u_t = -N0(u) + f on a family's operator (N0 without the shift; f: the handle's one source)
    def _fam_heat_step(self, fam, dt, theta, nsteps, cycles_per_step) -> MgHeatStats:
        st = MgHeatStats()
        _check(getattr(self.lib, f"mg_{fam}_heat_step")(self.h, dt, theta, nsteps, cycles_per_step, C.byref(st)))
        return st

    def vc_heat_step(self, dt, theta=1.0, nsteps=1, cycles_per_step=1) -> MgHeatStats:
        """mg_vc_heat_step: mg_heat_step for u_t = div(a grad u) + f with mg_vc_cycle as the step's cycle"""
        return self._fam_heat_step("vc", dt, theta, nsteps, cycles_per_step)

    def bc_heat_step(self, dt, theta=1.0, nsteps=1, cycles_per_step=1) -> MgHeatStats:
        """mg_bc_heat_step: mg_heat_step with zero-flux walls on the faces of the mask, mg_bc_cycle as the step's cycle"""
        return self._fam_heat_step("bc", dt, theta, nsteps, cycles_per_step)

    def fas_heat_step(self, dt, theta=1.0, nsteps=1, cycles_per_step=1) -> MgHeatStats:
        """mg_fas_heat_step: mg_heat_step for u_t = -(A0 u + gamma g(u)) + f with mg_fas_cycle as the step's cycle"""
        return self._fam_heat_step("fas", dt, theta, nsteps, cycles_per_step)

    def vc_heat_rhs(self, dt, theta, arr_u=ARR_U, arr_dst=ARR_RHS):
        """mg_vc_heat_rhs: arr_dst(0) = the right-hand side of one theta step of the unshifted vc operator from arr_u(0)"""
        _check(self.lib.mg_vc_heat_rhs(self.h, dt, theta, arr_u, arr_dst))

    def bc_heat_rhs(self, dt, theta, arr_u=ARR_U, arr_dst=ARR_RHS):
        """mg_bc_heat_rhs: the same with the Neumann faces of the mask; Dirichlet nodes take u"""
        _check(self.lib.mg_bc_heat_rhs(self.h, dt, theta, arr_u, arr_dst))

    def fas_heat_rhs(self, dt, theta, arr_u=ARR_U, arr_dst=ARR_RHS):
        """mg_fas_heat_rhs: the same with N0(u) = A0 u + gamma g(u)"""
        _check(self.lib.mg_fas_heat_rhs(self.h, dt, theta, arr_u, arr_dst))

    # -- lowest eigenpairs of sigma I + A on level 0 (multigrid-preconditioned LOBPCG)
    def eig_solve(self, m, nev=None, tol=1e-8, maxit=200, op=None):
        """mg_eig_solve: the nev (default m) smallest eigenpairs on a block of m vectors, warm-started from the X columns the
        handle holds -> (lambda[m], relres[m], hist, MgEigStats); the vectors come from eig_get_vector(EIG_X, j).
        op: the operator of this call (EIG_ON_*; default: the one of eig_set_operator), OR-ed into m as MG_EIG_OPERATOR does"""
        nev = m if nev is None else nev
        marg = m | eig_operator(self._eig_op if op is None else op)
        cap = max(maxit, 0) + 1
        lam = (C.c_double * max(m, 1))(); rel = (C.c_double * max(m, 1))()
        hist = (C.c_double * cap)(); nh = C.c_int(0); st = MgEigStats()
        _check(self.lib.mg_eig_solve(self.h, marg, nev, tol, maxit, lam, rel, hist, cap, C.byref(nh), C.byref(st)))
        return np.array(lam[:m]), np.array(rel[:m]), np.array(hist[:min(nh.value, cap)]), st

    def eig_set_vector(self, family, j, a):
        """mg_eig_set_vector: column j of a family (EIG_*) from a level-0 host array; EIG_X columns beyond the block grow it"""
        a = self._host(a, 0); _check(self.lib.mg_eig_set_vector(self.h, family, j, a.ctypes.data_as(C.c_void_p)))

    def eig_get_vector(self, family, j):
        a = np.empty(self.level_shape(0), self.np)
        _check(self.lib.mg_eig_get_vector(self.h, family, j, a.ctypes.data_as(C.c_void_p))); return a

    def eig_set_vector_device(self, family, j, obj, stream=0):
        ptr, dt = device_view(obj, self.level_shape(0))
        _check(self.lib.mg_eig_set_vector_device(self.h, family, j, ptr, dt, stream or None))

    def eig_get_vector_device(self, family, j, out, stream=0):
        ptr, dt = device_view(out, self.level_shape(0), writable=True)
        _check(self.lib.mg_eig_get_vector_device(self.h, family, j, ptr, dt, stream or None))

    def eig_block(self) -> int:
        """mg_eig_block: the block size currently allocated, 0: none"""
        m = C.c_int(0); _check(self.lib.mg_eig_block(self.h, C.byref(m))); return m.value

    _eig_op = EIG_ON_CONSTANT

    def eig_set_operator(self, op):
        """The operator eig_solve / eig_kernel_* pass on when they are given none: EIG_ON_CONSTANT (default), EIG_ON_FACES
        (mg_bc_*'s operator) or EIG_ON_COEFFICIENT (mg_vc_*'s). One integer kept by THIS OBJECT -- the C interface has no
        setter, every mg_eig_solve / mg_eig_kernel call names its operator (MG_EIG_OPERATOR); the mask, the shift and the
        coefficient are read by the library at that call"""
        if op not in (EIG_ON_CONSTANT, EIG_ON_FACES, EIG_ON_COEFFICIENT):
            raise MgError(-4, "eig_set_operator: the operator must be EIG_ON_CONSTANT, EIG_ON_FACES or EIG_ON_COEFFICIENT")
        self._eig_op = op

    def eig_get_operator(self) -> int:
        return self._eig_op

    def eig_kernel_gram(self, nw, np_, op=None):
        """mg_eig_kernel(EIG_K_APPLY_GRAM): AW = A W on the first nw W columns, then (G, H) over [X, W, P]; op as in eig_solve"""
        s = self.eig_block() + nw + np_
        G = np.zeros((s, s)); H = np.zeros((s, s)); dp = C.POINTER(C.c_double)
        _check(self.lib.mg_eig_kernel(self.h, EIG_K_APPLY_GRAM | eig_operator(self._eig_op if op is None else op), nw, np_, None, None, G.ctypes.data_as(dp), H.ctypes.data_as(dp), None))
        return G, H

    def eig_kernel_combine(self, nw, np_, cx, cp, theta, op=None):
        """mg_eig_kernel(EIG_K_COMBINE): the in-place block update with Cx (s x m), Cp ((nw + np) x nw), theta (m) -> sums r^2
        (weighted with an operator family); op as in eig_solve"""
        m = self.eig_block(); dp = C.POINTER(C.c_double)
        coef = np.concatenate([np.ascontiguousarray(cx, np.float64).ravel(), np.ascontiguousarray(cp, np.float64).ravel()])
        th = np.ascontiguousarray(theta, np.float64); sums = np.zeros(m)
        assert coef.size == (m + nw + np_) * m + (nw + np_) * nw and th.size == m
        _check(self.lib.mg_eig_kernel(self.h, EIG_K_COMBINE | eig_operator(self._eig_op if op is None else op), nw, np_, coef.ctypes.data_as(dp), th.ctypes.data_as(dp), None, None,
                                      sums.ctypes.data_as(dp)))
        return sums

    def set_stage_callback(self, fn):
        """fn(stage, level, array) after every stage of the sawtooth cycle (CREATE_GIF dumps); None removes it"""
        if fn is None:
            self._stage_cb = STAGE_FN(0)
        else:
            def tramp(user, stage, level, n, nz, ptr):
                shape = (n, n) if self.d.dim == 2 else (nz, n, n)
                cnt = int(np.prod(shape))
                buf = (C.c_double if self.d.dtype == MG_F64 else C.c_float) * cnt
                fn(stage, level, np.ctypeslib.as_array(buf.from_address(ptr)).reshape(shape).copy())
            self._stage_cb = STAGE_FN(tramp)
        _check(self.lib.mg_set_stage_callback(self.h, self._stage_cb, None))

    def sync(self): _check(self.lib.mg_sync(self.h))
    def timer_start(self): _check(self.lib.mg_timer_start(self.h))

    def timer_stop(self) -> float:
        ms = C.c_double(0); _check(self.lib.mg_timer_stop(self.h, C.byref(ms))); return ms.value

    def profile_begin(self): _check(self.lib.mg_profile_begin(self.h))

    def profile_end(self):
        """-> (summed ms of the finest-grid smoother calls, number of sweeps)"""
        ms = C.c_double(0); n = C.c_int(0)
        _check(self.lib.mg_profile_end(self.h, C.byref(ms), C.byref(n))); return ms.value, n.value

    def profile_fused(self):
        """-> (summed ms, sweeps) of the finest-grid launches that also carried the prolongation
        (valid after profile_end)"""
        ms = C.c_double(0); n = C.c_int(0)
        _check(self.lib.mg_profile_fused(self.h, C.byref(ms), C.byref(n))); return ms.value, n.value

    def profile_get(self, kind):
        """-> (summed ms, launches) of one kind of finest-level launch (PROF_*; valid after profile_end)"""
        ms = C.c_double(0); n = C.c_int(0)
        _check(self.lib.mg_profile_get(self.h, kind, C.byref(ms), C.byref(n))); return ms.value, n.value

    def comm_info(self):
        """-> (rank, nranks, ranks the transport reports, transport name)"""
        r, n, t = C.c_int(0), C.c_int(0), C.c_int(0); name = C.c_char_p()
        _check(self.lib.mg_comm_info(self.h, C.byref(r), C.byref(n), C.byref(t), C.byref(name)))
        return r.value, n.value, t.value, name.value.decode()

    def comm_stats(self):
        """-> (message groups posted, bytes sent) by this rank since creation"""
        g, b = C.c_longlong(0), C.c_longlong(0)
        _check(self.lib.mg_comm_stats(self.h, C.byref(g), C.byref(b))); return g.value, b.value

    def device_bytes(self) -> int:
        b = C.c_size_t(0); _check(self.lib.mg_device_bytes(self.h, C.byref(b))); return b.value

    # -- test and debugging window (mg_debug_raw_*): whole allocations, ghost planes and padding columns included
    def debug_raw_layout(self, space, index=0, level=0) -> MgDebugRawInfo:
        """mg_debug_raw_layout: element size, extents, pitch, ghost planes and size of one allocation (RAW_* spaces)"""
        info = MgDebugRawInfo(); _check(self.lib.mg_debug_raw_layout(self.h, space, index, level, C.byref(info))); return info

    def debug_raw_get(self, space, index=0, level=0):
        """mg_debug_raw_copy, device -> host: the allocation as an array of shape (nz + 2 ghost, ny, pitch)"""
        info = self.debug_raw_layout(space, index, level)
        a = np.empty((info.nz + 2 * info.ghost, info.ny, info.pitch), np.float64 if info.elem_size == 8 else np.float32)
        _check(self.lib.mg_debug_raw_copy(self.h, space, index, level, a.ctypes.data_as(C.c_void_p), a.nbytes, 0)); return a

    def debug_raw_set(self, space, index, level, a):
        """mg_debug_raw_copy, host -> device: every word of the allocation from an array shaped as debug_raw_get returns it"""
        info = self.debug_raw_layout(space, index, level)
        want = (info.nz + 2 * info.ghost, info.ny, info.pitch)
        a = np.ascontiguousarray(a, np.float64 if info.elem_size == 8 else np.float32)
        if a.shape != want:
            raise ValueError(f"expected shape {want}, got {a.shape}")
        _check(self.lib.mg_debug_raw_copy(self.h, space, index, level, a.ctypes.data_as(C.c_void_p), a.nbytes, 1))
