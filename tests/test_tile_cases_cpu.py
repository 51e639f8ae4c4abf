"""The table of tile cases (tests/tile_cases.py) reaches every class it is there for -- from its computed columns, no GPU.

A bit-for-bit case proves something about the marching tile's axis handling only if the tile takes a level on which the axes
differ. The assertions below work from pure restatements of the level geometry, the level coefficients (npref.Problem.coefs)
and mg_geom.h's march_ok; they fail when a gate or a row changes so that a class is no longer run, and they state the gap the
table closes: no case the kernel tests had before it reaches any of the classes.
"""
import math

import pytest

from tests import tile_cases as tc

NEW = tc.tile_levels(tc.CASES)


def test_the_table_is_the_issue_s():
    assert tc.ANISO == (1.0, 2.5, 0.3)
    from tests import o4_ref
    assert tc.ANISO == o4_ref.ANISO
    assert [(t.id, t.n, t.levels, t.check) for t in tc.TABLE] == [("a33", 33, 2, (0, 1)), ("a65", 65, 2, (0, 1)), ("sa65", 65, 2, (0, 1)),
                                                                  ("s67", 67, 2, (0, 1)), ("s129", 129, 2, (1,))]
    assert all(t.dim == 3 for t in tc.TABLE)
    assert [t.extra for t in tc.TABLE] == [dict(aniso=tc.ANISO), dict(aniso=tc.ANISO), dict(semi_xy=1, aniso=tc.ANISO), dict(semi_xy=1),
                                           dict(semi_xy=1)]
    # distinct entries, and no ratio a power of two: an exchanged pair changes the bits of a product
    a = tc.ANISO
    for i in range(3):
        for j in range(i + 1, 3):
            assert math.frexp(a[i] / a[j])[0] != 0.5, (i, j)
    for case, t in zip(tc.CASES, tc.TABLE):
        assert tc.find(case) is t and tc.case_id(case) == t.id and tc.levels_to_check(case) == t.check
    assert tc.find((3, 65, 2, {})) is None and tc.case_id((3, 17, 2, {"aniso": (1.0, 30.0, 0.05)})) == "3d17-aniso"
    assert tc.levels_to_check((3, 17, 3, {"semi_xy": 1})) == (0, 1) and tc.levels_to_check((3, 34, 1, {})) == (0,)


def test_level_shapes_and_coefficients():
    assert [tc.level_shape(tc.SA65, l) for l in (0, 1)] == [(65, 65, 65), (65, 33, 33)]
    assert [tc.level_shape(tc.S67, l) for l in (0, 1)] == [(67, 67, 67), (67, 34, 34)]
    assert tc.level_shape(tc.S129, 1) == (129, 65, 65) and tc.level_shape(tc.A65, 1) == (33, 33, 33)
    assert tc.level_shape((2, 130, 1, {}), 0) == (130, 130)
    # c_a = -alpha aniso_a / h_a^2; a semi-coarsened level keeps h_z
    h = 1.0 / 64
    cx, cy, cz = tc.level_coefs(tc.SA65, 1)
    assert (cx, cy, cz) == pytest.approx((-1.3 / (2 * h) ** 2, -1.3 * 2.5 / (2 * h) ** 2, -1.3 * 0.3 / h ** 2), rel=1e-14)
    cx, cy, cz = tc.level_coefs(tc.S67, 1)
    assert cx == cy and cz == pytest.approx(4 * cx, rel=1e-14)
    cx, cy, cz = tc.level_coefs((3, 65, 2, {}), 1)
    assert cx == cy == cz


def test_march_gate_is_the_references():
    from tests import bc_ref, fas_ref, vcn_ref
    for nx in (9, 17, 31, 32, 33, 34, 35, 63, 64, 65, 67, 129):
        for nz in (5, 7, nx, 2 * nx - 1):
            for es in (8, 4):
                want = tc.march_ok(3, nx, nx, nz, es)
                assert want == (nx >= (32 if es == 8 else 64) and nz >= 7)
                assert want == bc_ref.march_ok(3, nx, nx, nz, es) == vcn_ref.march_ok(3, nx, nx, nz, es) == fas_ref.march_ok(3, nx, nx, nz, es)
                assert not tc.march_ok(2, nx, nx, 1, es)


def test_each_case_reaches_what_its_row_says():
    hit = {(x["id"], x["level"], x["es"]) for x in NEW}
    assert hit == {("a33", 0, 8), ("a65", 0, 8), ("a65", 0, 4), ("a65", 1, 8), ("sa65", 0, 8), ("sa65", 0, 4), ("sa65", 1, 8),
                   ("s67", 0, 8), ("s67", 0, 4), ("s67", 1, 8), ("s129", 1, 8), ("s129", 1, 4)}
    by = {(x["id"], x["level"], x["es"]): x for x in NEW}
    assert all(by[k]["distinct"] and not by[k]["nz_ne_nx"] for k in (("a33", 0, 8), ("a65", 0, 4), ("a65", 1, 8)))
    x = by[("sa65", 1, 8)]
    assert x["shape"] == (65, 33, 33) and x["distinct"] and x["nz_ne_nx"] and not x["even"]
    x = by[("s67", 1, 8)]
    assert x["shape"] == (67, 34, 34) and x["even"] and x["nz_ne_nx"] and not x["distinct"] and x["coefs"][0] == x["coefs"][1]
    x = by[("s129", 1, 4)]
    assert x["shape"] == (129, 65, 65) and x["nz_ne_nx"]
    assert ("s129", 0, 8) not in hit   # level 0 of s129 is never referenced


def test_the_table_reaches_every_class():
    for es in (8, 4):
        assert any(x["distinct"] for x in NEW if x["es"] == es), es
        assert any(x["nz_ne_nx"] for x in NEW if x["es"] == es), es
    assert any(x["even"] and x["nz_ne_nx"] for x in NEW if x["es"] == 8)
    assert any(x["distinct"] and x["nz_ne_nx"] for x in NEW)


def old_lists():
    """the case lists of the families' kernel tests without the table's entries: what the suite had before"""
    from tests import test_bc_gpu, test_fas_gpu, test_fasn_gpu, test_fasvc_gpu, test_vc_gpu, test_vcn_gpu
    out = {}
    for mod in (test_bc_gpu, test_fas_gpu, test_fasn_gpu, test_fasvc_gpu, test_vc_gpu, test_vcn_gpu):
        assert all(c in mod.CASES for c in tc.CASES), mod.__name__   # the table is in every list
        out[mod.__name__] = [c for c in mod.CASES if tc.find(c) is None]
    return out


def test_no_earlier_case_reaches_any_class():
    """the statement of the gap: the anisotropic and the semi-coarsened entries the lists had run the plain kernels (n = 17), and
    every level the tile took was a cube with cx == cy == cz (an even row among them: 34^3)"""
    for name, cases in old_lists().items():
        assert len(cases) == 11 and any("aniso" in c[3] for c in cases) and any("semi_xy" in c[3] for c in cases), name
        old = tc.tile_levels(cases)
        assert {x["id"] for x in old} == {"3d33", "3d34", "3d35", "3d65", "3d67"}, name   # the tile did run, on cubes
        for x in old:
            assert not x["distinct"] and not x["nz_ne_nx"], (name, x)
            assert x["coefs"][0] == x["coefs"][1] == x["coefs"][2] and x["shape"][0] == x["shape"][2], (name, x)


def test_the_other_lists_carry_the_cases_the_issue_names():
    from tests import storage_table as st
    from tests import test_mixedvc_gpu, test_step_gpu
    assert [(c[0], c[1], c[2], c[3]) for c in test_step_gpu.SHAPES if c[3]] == [tc.A33, tc.A65]
    assert [k for k in test_mixedvc_gpu.KSHAPES if k[2]] == [(3, 33, dict(aniso=tc.ANISO)), (3, 65, dict(aniso=tc.ANISO))]
    extra = [c for c in st.FAM3 if c.extra]
    assert [(c.dim, c.n, c.levels, c.extra) for c in extra] == [tc.S67, tc.A65]
