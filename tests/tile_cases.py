"""The cases that put the marching tile of the operator families on a level with unequal axis coefficients (TEST
INFRASTRUCTURE, numpy only; nothing here needs a GPU or the HIP library).

The residual, the Jacobi sweep and the theta-step right-hand side of mg_vc_*, mg_bc_* and mg_fas_* (MG_FAS_ON_FACES and
MG_FAS_ON_COEFFICIENT included) have a plain form and a marching tile (k_vc_march, k_bc_march, the tile of mg_fas.hip, the fused
tile of mg_vc_mixed.hip). mg_geom.h's march_ok hands a level to the tile when it is 3-D and a row holds at least 16 full
16-byte vectors: nx >= 32 in fp64, nx >= 64 in fp32. On a cube with cx == cy == cz a tile that exchanged two axis coefficients,
or took a face test or a plane count from the wrong extent, computes the same bits. The classes below are the ones in which it
does not:

    distinct   cx, cy, cz pairwise distinct on a level the tile takes
    nz != nx   a semi-coarsened level the tile takes (the z-face test, the z-chunk count)
    even       an even row (no tail-line store) on a level that is not a cube

    id     desc                                    levels   what it reaches
    a33    3-D 33,  2 levels, aniso=ANISO          0, 1     fp64 tile on level 0, distinct (fp32: plain)
    a65    3-D 65,  2 levels, aniso=ANISO          0, 1     tile in both precisions on level 0, fp64 tile on level 1 (33^3), distinct
    sa65   3-D 65,  2 levels, semi_xy=1, ANISO     0, 1     level 1 is 33 x 33 x 65: fp64 tile, nz != nx AND distinct
    s67    3-D 67,  2 levels, semi_xy=1            0, 1     level 1 is 34 x 34 x 67: fp64 tile, even, nz != nx, cx == cy != cz
    s129   3-D 129, 2 levels, semi_xy=1            1        level 1 is 65 x 65 x 129: the fp32 tile with nz != nx; more than one
                                                            z chunk per column. Level 0 (129^3) is never referenced in numpy.

ANISO is tests/o4_ref.py's: three distinct entries, no ratio a power of two (an exchanged pair changes the bits of every
product), and mild enough that point smoothers converge on it. tests/test_tile_cases_cpu.py proves the column on the right.
"""
from collections import namedtuple

import numpy as np

from tests import npref

ANISO = (1.0, 2.5, 0.3)

TileCase = namedtuple("TileCase", "id dim n levels extra check")   # check: the levels a kernel test looks at

TABLE = [
    TileCase("a33", 3, 33, 2, {"aniso": ANISO}, (0, 1)),
    TileCase("a65", 3, 65, 2, {"aniso": ANISO}, (0, 1)),
    TileCase("sa65", 3, 65, 2, {"semi_xy": 1, "aniso": ANISO}, (0, 1)),
    TileCase("s67", 3, 67, 2, {"semi_xy": 1}, (0, 1)),
    TileCase("s129", 3, 129, 2, {"semi_xy": 1}, (1,)),
]
# as the kernel tests spell a case: (dim, n, levels, extra)
CASES = [(t.dim, t.n, t.levels, t.extra) for t in TABLE]
A33, A65, SA65, S67, S129 = CASES


def find(case):
    """the table's entry of a (dim, n, levels, extra) case, None for a case of another list"""
    for t in TABLE:
        if (t.dim, t.n, t.levels, t.extra) == tuple(case):
            return t
    return None


def case_id(case):
    """the table's id, or the spelling the kernel tests have always used: 3d65, 3d17-aniso, 3d17-semi_xy"""
    t = find(case)
    dim, n, levels, extra = case
    return t.id if t else f"{dim}d{n}" + "".join("-" + k for k in extra)


def levels_to_check(case):
    """a table case: its own levels; any other case: levels 0 and 1, as the kernel tests have always looked at"""
    t = find(case)
    return t.check if t else tuple(range(min(case[2], 2)))


def _problem(case):
    dim, n, levels, extra = case
    return npref.Problem(dim=dim, n=n, levels=levels, length=1.0, alpha=1.3, prec=np.float64, **extra)


def level_shape(case, l):
    """the level's array shape, (nz, ny, nx) in 3-D and (ny, nx) in 2-D"""
    return _problem(case).shape(l)


def level_coefs(case, l):
    """(cx, cy, cz) as the references compute them without a handle (npref.Problem.coefs); 2-D: (cx, cy)"""
    by_axis, _ = _problem(case).coefs[l]
    return tuple(float(c) for c in reversed(by_axis))


def march_ok(dim, nx, ny, nz, elem_size):
    """mg::march_ok (mg_geom.h) restated"""
    return dim == 3 and nx // (16 // elem_size) >= 16 and ny >= 7 and nz >= 7


def takes_tile(case, l, elem_size):
    shape = level_shape(case, l)
    return case[0] == 3 and march_ok(3, shape[2], shape[1], shape[0], elem_size)


def want_forms(case, l, elem_size):
    """the forms a kernel test must have run on the level: both where the tile takes it, the plain one elsewhere"""
    return {"march", "plain"} if takes_tile(case, l, elem_size) else {"plain"}


def tile_levels(cases):
    """every (case, level, element size) of `cases`, over the levels the kernel tests check, that the tile takes ->
    [dict(id, level, es, shape, coefs, distinct, nz_ne_nx, even)]"""
    out = []
    for case in cases:
        for l in levels_to_check(case):
            for es in (8, 4):
                if not takes_tile(case, l, es):
                    continue
                nz, ny, nx = level_shape(case, l)
                cx, cy, cz = level_coefs(case, l)
                out.append(dict(id=case_id(case), level=l, es=es, shape=(nz, ny, nx), coefs=(cx, cy, cz),
                                distinct=len({cx, cy, cz}) == 3, nz_ne_nx=nz != nx, even=nx % 2 == 0))
    return out
