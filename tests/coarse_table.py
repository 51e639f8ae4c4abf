"""What mg::coarse_plan (multigrid_prj_amd/csrc/mg_geom.h) can return, derived by tests/test_coarse_plan_cpu.py from its sweep over
every shape a descriptor can make coarsest (that test fails when the planner and this file disagree) and run row by row on
the GPU by tests/test_coarse_solver_gpu.py.

A variant is (kernel, DIM, SEG, overlap, skip, dtype):
  kernel   one of KERNELS, the order of mg::CoarseKernel
  SEG      run length of the row kernels (0: not a row kernel)
  overlap  the last run of a row shares one point with its neighbour (dup0 in k_coarse_jacobi_rows)
  skip     sweeps between two norm tests of the Jacobi row kernel: 8, or 1 (omega outside (0, 1], or no LDS room); 0 elsewhere
Each maps to ((nz, ny, nx), smoother, switches off): the smallest shape that reaches it with every switch at its default --
all of them are reachable that way -- and the smoother (0 lexicographic Gauss-Seidel, 1 Jacobi, 2 red-black) that does."""
from collections import namedtuple

Plan = namedtuple("Plan", "kernel seg overlap skip threads lds_bytes zero_x memset")
KERNELS = ("jacobi_rows", "rb_rows", "gs_rows2d", "lds", "global")
SWITCHES = ("MG_COARSE_ROWS", "MG_COARSE_RB_ROWS", "MG_COARSE_GS_ROWS")   # coarse_plan's last three arguments

REACHABLE = {
    ('jacobi_rows', 2, 4, False, 8, 'f32'): ((1, 26, 26), 1, ()),
    ('jacobi_rows', 2, 4, False, 8, 'f64'): ((1, 26, 26), 1, ()),
    ('jacobi_rows', 2, 4, False, 1, 'f32'): ((1, 26, 26), 1, ()),
    ('jacobi_rows', 2, 4, False, 1, 'f64'): ((1, 26, 26), 1, ()),
    ('jacobi_rows', 2, 4, True, 8, 'f32'): ((1, 25, 25), 1, ()),
    ('jacobi_rows', 2, 4, True, 8, 'f64'): ((1, 25, 25), 1, ()),
    ('jacobi_rows', 2, 4, True, 1, 'f32'): ((1, 25, 25), 1, ()),
    ('jacobi_rows', 2, 4, True, 1, 'f64'): ((1, 25, 25), 1, ()),
    ('jacobi_rows', 2, 5, False, 8, 'f32'): ((1, 32, 32), 1, ()),
    ('jacobi_rows', 2, 5, False, 8, 'f64'): ((1, 32, 32), 1, ()),
    ('jacobi_rows', 2, 5, False, 1, 'f32'): ((1, 32, 32), 1, ()),
    ('jacobi_rows', 2, 5, False, 1, 'f64'): ((1, 32, 32), 1, ()),
    ('jacobi_rows', 2, 5, True, 8, 'f32'): ((1, 31, 31), 1, ()),
    ('jacobi_rows', 2, 5, True, 8, 'f64'): ((1, 31, 31), 1, ()),
    ('jacobi_rows', 2, 5, True, 1, 'f32'): ((1, 31, 31), 1, ()),
    ('jacobi_rows', 2, 5, True, 1, 'f64'): ((1, 31, 31), 1, ()),
    ('jacobi_rows', 2, 7, False, 8, 'f32'): ((1, 44, 44), 1, ()),
    ('jacobi_rows', 2, 7, False, 8, 'f64'): ((1, 44, 44), 1, ()),
    ('jacobi_rows', 2, 7, False, 1, 'f32'): ((1, 44, 44), 1, ()),
    ('jacobi_rows', 2, 7, False, 1, 'f64'): ((1, 44, 44), 1, ()),
    ('jacobi_rows', 2, 7, True, 8, 'f32'): ((1, 36, 36), 1, ()),
    ('jacobi_rows', 2, 7, True, 8, 'f64'): ((1, 36, 36), 1, ()),
    ('jacobi_rows', 2, 7, True, 1, 'f32'): ((1, 36, 36), 1, ()),
    ('jacobi_rows', 2, 7, True, 1, 'f64'): ((1, 36, 36), 1, ()),
    ('jacobi_rows', 2, 8, False, 8, 'f32'): ((1, 34, 34), 1, ()),
    ('jacobi_rows', 2, 8, False, 8, 'f64'): ((1, 34, 34), 1, ()),
    ('jacobi_rows', 2, 8, False, 1, 'f32'): ((1, 34, 34), 1, ()),
    ('jacobi_rows', 2, 8, False, 1, 'f64'): ((1, 34, 34), 1, ()),
    ('jacobi_rows', 2, 8, True, 8, 'f32'): ((1, 41, 41), 1, ()),
    ('jacobi_rows', 2, 8, True, 8, 'f64'): ((1, 41, 41), 1, ()),
    ('jacobi_rows', 2, 8, True, 1, 'f32'): ((1, 41, 41), 1, ()),
    ('jacobi_rows', 2, 8, True, 1, 'f64'): ((1, 41, 41), 1, ()),
    ('jacobi_rows', 3, 4, False, 8, 'f32'): ((10, 10, 10), 1, ()),
    ('jacobi_rows', 3, 4, False, 8, 'f64'): ((10, 10, 10), 1, ()),
    ('jacobi_rows', 3, 4, False, 1, 'f32'): ((10, 10, 10), 1, ()),
    ('jacobi_rows', 3, 4, False, 1, 'f64'): ((10, 10, 10), 1, ()),
    ('jacobi_rows', 3, 4, True, 8, 'f32'): ((17, 9, 9), 1, ()),
    ('jacobi_rows', 3, 4, True, 8, 'f64'): ((17, 9, 9), 1, ()),
    ('jacobi_rows', 3, 4, True, 1, 'f32'): ((17, 9, 9), 1, ()),
    ('jacobi_rows', 3, 4, True, 1, 'f64'): ((17, 9, 9), 1, ()),
    ('jacobi_rows', 3, 5, False, 8, 'f32'): ((12, 12, 12), 1, ()),
    ('jacobi_rows', 3, 5, False, 8, 'f64'): ((12, 12, 12), 1, ()),
    ('jacobi_rows', 3, 5, False, 1, 'f32'): ((12, 12, 12), 1, ()),
    ('jacobi_rows', 3, 5, False, 1, 'f64'): ((12, 12, 12), 1, ()),
    ('jacobi_rows', 3, 5, True, 8, 'f32'): ((11, 11, 11), 1, ()),
    ('jacobi_rows', 3, 5, True, 8, 'f64'): ((11, 11, 11), 1, ()),
    ('jacobi_rows', 3, 5, True, 1, 'f32'): ((11, 11, 11), 1, ()),
    ('jacobi_rows', 3, 5, True, 1, 'f64'): ((11, 11, 11), 1, ()),
    ('jacobi_rows', 3, 7, True, 8, 'f32'): ((15, 15, 15), 1, ()),
    ('jacobi_rows', 3, 7, True, 8, 'f64'): ((15, 15, 15), 1, ()),
    ('jacobi_rows', 3, 7, True, 1, 'f32'): ((15, 15, 15), 1, ()),
    ('jacobi_rows', 3, 7, True, 1, 'f64'): ((15, 15, 15), 1, ()),
    ('rb_rows', 2, 4, False, 0, 'f32'): ((1, 26, 26), 2, ()),
    ('rb_rows', 2, 4, False, 0, 'f64'): ((1, 26, 26), 2, ()),
    ('rb_rows', 2, 4, True, 0, 'f32'): ((1, 25, 25), 2, ()),
    ('rb_rows', 2, 4, True, 0, 'f64'): ((1, 25, 25), 2, ()),
    ('rb_rows', 2, 5, False, 0, 'f32'): ((1, 32, 32), 2, ()),
    ('rb_rows', 2, 5, False, 0, 'f64'): ((1, 32, 32), 2, ()),
    ('rb_rows', 2, 5, True, 0, 'f32'): ((1, 31, 31), 2, ()),
    ('rb_rows', 2, 5, True, 0, 'f64'): ((1, 31, 31), 2, ()),
    ('rb_rows', 3, 4, False, 0, 'f32'): ((10, 10, 10), 2, ()),
    ('rb_rows', 3, 4, False, 0, 'f64'): ((10, 10, 10), 2, ()),
    ('rb_rows', 3, 4, True, 0, 'f32'): ((17, 9, 9), 2, ()),
    ('rb_rows', 3, 4, True, 0, 'f64'): ((17, 9, 9), 2, ()),
    ('rb_rows', 3, 5, False, 0, 'f32'): ((12, 12, 12), 2, ()),
    ('rb_rows', 3, 5, False, 0, 'f64'): ((12, 12, 12), 2, ()),
    ('rb_rows', 3, 5, True, 0, 'f32'): ((11, 11, 11), 2, ()),
    ('rb_rows', 3, 5, True, 0, 'f64'): ((11, 11, 11), 2, ()),
    ('gs_rows2d', 2, 0, False, 0, 'f32'): ((1, 3, 3), 0, ()),
    ('gs_rows2d', 2, 0, False, 0, 'f64'): ((1, 3, 3), 0, ()),
    ('lds', 2, 0, False, 0, 'f32'): ((1, 3, 3), 1, ()),
    ('lds', 2, 0, False, 0, 'f64'): ((1, 3, 3), 1, ()),
    ('lds', 3, 0, False, 0, 'f32'): ((3, 3, 3), 0, ()),
    ('lds', 3, 0, False, 0, 'f64'): ((3, 3, 3), 0, ()),
    ('global', 2, 0, False, 0, 'f32'): ((1, 73, 73), 1, ()),
    ('global', 2, 0, False, 0, 'f64'): ((1, 73, 73), 1, ()),
    ('global', 3, 0, False, 0, 'f32'): ((65, 9, 9), 0, ()),
    ('global', 3, 0, False, 0, 'f64'): ((65, 9, 9), 0, ()),
}
SKIP1_FOR_LDS_ROOM = {
    ('jacobi_rows', 3, 5, False, 1, 'f64'): ((45, 12, 12), 1, ()),
}

# (kernel, DIM, SEG) the planner's orders of preference name and no shape reaches: not instantiated in mg_kernels.hip
UNREACHABLE = {
    ("jacobi_rows", 3, 8): "a row that admits runs of 8 within 512 threads admits runs of 4 within 1024, and 4 comes first in the 3-D order",
}
# (3-D Jacobi runs of 7 without overlap are a variant no shape reaches either: an interior width of 7 takes runs of 4, 14 runs
# of 5, and from 21 on the interior rows of a cube or a box exceed 512 threads)

# size edges, every switch at its default: the last shape on a kernel and the first one off it
#   (kernel, DIM, dtype, (nz, ny, nx), smoother)
EDGES = [
    ("gs_rows2d", 2, "f64", (1, 97, 97), 0), ("global", 2, "f64", (1, 98, 98), 0),      # two LDS copies within 150 KiB
    ("gs_rows2d", 2, "f32", (1, 138, 138), 0), ("global", 2, "f32", (1, 139, 139), 0),
    ("lds", 3, "f64", (17, 17, 17), 0), ("global", 3, "f64", (18, 18, 18), 0),          # 5 points per thread of 1024
    ("lds", 3, "f32", (17, 17, 17), 0), ("global", 3, "f32", (18, 18, 18), 0),
]
# the same for the generic LDS kernel in 2-D, where only a switch at 0 leads to it: (kernel, dtype, shape, smoother, switch)
EDGES_SWITCH_OFF = [
    ("lds", "f64", (1, 71, 71), 1, "MG_COARSE_ROWS"), ("global", "f64", (1, 72, 72), 1, "MG_COARSE_ROWS"),
    ("lds", "f32", (1, 71, 71), 2, "MG_COARSE_RB_ROWS"), ("global", "f32", (1, 72, 72), 2, "MG_COARSE_RB_ROWS"),
    ("lds", "f64", (1, 71, 71), 0, "MG_COARSE_GS_ROWS"), ("global", "f64", (1, 72, 72), 0, "MG_COARSE_GS_ROWS"),
]


def handle_kwargs(dim, shape):
    """descriptor arguments of the smallest hierarchy whose LAST level has this shape, and that level's index: a single level
    for squares and cubes; for a box (nz, n, n), nz = (n - 1) 2^k + 1, a cube of nz semi-coarsened k times"""
    nz, ny, nx = shape
    assert ny == nx and (nz == nx if dim == 3 else nz == 1) or dim == 3
    if dim == 2 or nz == nx:
        return dict(dim=dim, n=nx, levels=1), 0
    k = ((nz - 1) // (nx - 1)).bit_length() - 1
    assert (nx - 1) << k == nz - 1
    return dict(dim=3, n=nz, levels=k + 1, semi_xy=k), k
