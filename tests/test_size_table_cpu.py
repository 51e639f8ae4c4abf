"""The table of odd sizes (tests/size_table.py) reaches every class it is there for -- from its computed columns, no GPU.

A row of tests/test_odd_sizes_gpu.py proves something only if its shape really takes the kernel it was written for. The
columns of size_table.plan() are computed from Python statements of the dispatch gates; the assertions below fail when a gate
(or a row) changes so that a class of tail lanes, partial waves, short bricks or mixed hierarchies is no longer run by any
row whose n is not 2^k + 1.
"""
import pytest

from oracle import pyoracle as po
from tests import size_table as st

ODD = [r for r in st.ROWS if not st.is_pow2_plus_1(r["n"])]
PLANS = [(r, st.plan(r)) for r in ODD]
LEVELS = [(r, x) for r, p in PLANS for x in p["levels"]]
TRANS = [(r, l, t) for r, p in PLANS for l, t in enumerate(p["transitions"])]


def test_every_row_is_admissible_and_outside_the_power_of_two_family():
    assert ODD == st.ROWS, "the table is about n = m * 2^j + 1 with m not a power of two"
    for r in st.ROWS:
        assert (r["n"] - 1) % (1 << (r["levels"] - 1)) == 0, r["id"]
        assert r["dim"] == 2 or r["n"] <= 225, r["id"]
        assert st.shapes(r)[-1][0] >= 3, r["id"]


def test_the_issue_sizes_run_in_both_precisions_with_both_point_smoothers():
    for n, levels, semi in [(37, 3, 0), (45, 3, 0), (97, 5, 0), (133, 3, 0), (161, 5, 0), (193, 4, 0), (225, 5, 0), (97, 4, 1)]:
        for dtype in (po.MG_F64, po.MG_F32):
            for sm in (po.SMOOTH_JACOBI, po.SMOOTH_RBGS):
                hit = [r for r in st.ROWS if (r["n"], r["levels"], r["semi_xy"], r["dtype"], r["smoother"]) == (n, levels, semi, dtype, sm)
                       and r["nu"] == (2, 2) and r["restriction"] == po.RESTRICT_FULLW and r["cycle"] == po.CYCLE_V]
                assert hit, (n, levels, semi, dtype, sm)
    jac = [r for r in st.ROWS if r["smoother"] == po.SMOOTH_JACOBI and r["cycle"] == po.CYCLE_V]
    assert any(r["nu"] == (1, 1) and r["n"] == 97 for r in jac) and any(r["nu"] == (2, 1) and r["n"] == 45 for r in jac)
    assert any(r["restriction"] == po.RESTRICT_INJECT and r["cycle"] == po.CYCLE_V for r in st.ROWS)
    saw = [r for r in st.ROWS if r["cycle"] == po.CYCLE_SAWTOOTH and r["dim"] == 3]
    assert any(r["smoother"] == po.SMOOTH_JACOBI and (r["n"], r["levels"], r["omega"], r["nu"][1]) == (49, 3, 1.0, 3) for r in saw)
    assert any(r["smoother"] == po.SMOOTH_GS_LEX and (r["n"], r["levels"]) == (25, 2) for r in saw)
    for sm, line in ((po.SMOOTH_ZEBRA_Y, 1), (po.SMOOTH_ZEBRA_X, 0)):
        for dtype in (po.MG_F64, po.MG_F32):
            assert any(r["smoother"] == sm and r["dtype"] == dtype and r["dim"] == 3 and (r["n"], r["levels"]) == (97, 4)
                       and r["aniso"][line] == 100.0 for r in st.ROWS), (sm, dtype)
    assert any(r["smoother"] == po.SMOOTH_ZEBRA_X and r["dim"] == 2 and r["n"] == 97 for r in st.ROWS)


@pytest.mark.parametrize("dtype", [po.MG_F64, po.MG_F32], ids=["f64", "f32"])
def test_four_gates_are_seen_from_both_sides(dtype):
    lv = [x for r, x in LEVELS if r["dtype"] == dtype and r["dim"] == 3]
    tr = [t for r, _, t in TRANS if r["dtype"] == dtype and r["dim"] == 3]
    assert {x["fast_path_ok"] for x in lv} == {True, False}
    for gate in ("prolong_fast_ok", "resid_restrict_fast_ok", "small_fused_ok"):
        assert {t[gate] for t in tr} == {True, False}, gate
    # ... and not only as gates: the kernels behind them run, and so do the ones they fall back to
    assert {t["rr_fused"] for t in tr} == {True, False} and {t["prolong_fast"] for t in tr} == {True, False}
    assert {t["small_post"] for t in tr} == {True, False} and {t["small_pre"] for t in tr} == {True, False}
    # small_fused_ok is false for its size on a standard transition (161^3 and up) and for a semi-coarsened one
    assert any(not t["small_fused_ok"] for r, l, t in TRANS if r["dtype"] == dtype and not r["semi_xy"] and r["dim"] == 3)
    assert any(not t["small_fused_ok"] for r, l, t in TRANS if r["dtype"] == dtype and l < r["semi_xy"])


def test_jacobi2_ok_is_out_of_reach_of_this_family():
    """The fifth gate: rows of 64, 128, 192 ... vectors plus one column are n = 129, 257, 385 (fp64) and 257, 513, 769
    (fp32): no level of a 3-D grid of at most 225 points a side has such rows unless n = 2^k + 1 (129 = (n - 1) / 2^l + 1
    gives n = 2^(7 + l) + 1). The fused pair keeps its own tests (n = 385 among them); here every row must take the single
    sweeps, and this fails if the pair's widths ever grow into the family."""
    for n in range(3, 226):
        if st.is_pow2_plus_1(n):
            continue
        for dtype in (po.MG_F64, po.MG_F32):
            l = 0
            while (n - 1) % (1 << l) == 0 and (n - 1) // (1 << l) + 1 >= 3:
                assert not st.jacobi2_ok((n - 1) // (1 << l) + 1, dtype), (n, l, dtype)
                l += 1
    assert not any(x["jacobi2_ok"] for _, x in LEVELS)
    assert any(st.jacobi2_ok(n, po.MG_F64) for n in (129, 385)) and st.jacobi2_ok(257, po.MG_F32)   # the statement is alive


def test_fused_residual_restriction_runs_with_partial_waves():
    for dtype in (po.MG_F64, po.MG_F32):
        lanes = {t["rr_lanes"] for r, _, t in TRANS if t["rr_fused"] and r["dtype"] == dtype}
        one = {x for x in lanes if x < 64}
        # one wave that is not full, and neither 16 nor 32 lanes: widths between and beyond them
        assert {24, 40, 48, 56} <= one, (dtype, sorted(one))
        assert any(x % 2 == 1 for x in one), (dtype, sorted(one))
        if dtype == po.MG_F32:   # (a coarse row of >= 17 columns is >= 16 lanes in fp64, >= 8 in fp32)
            assert any(x < 16 for x in one), sorted(one)
    # a full wave next to a partial one (the wave-edge mailbox's last lane is not lane 63): fp64 rows up to 225 reach it
    two = {t["rr_lanes"] for r, _, t in TRANS if t["rr_fused"] and t["rr_waves"] == 2}
    assert {64 + 16, 64 + 32, 64 + 48} <= two, sorted(two)
    assert any(64 < x < 64 + 16 for x in two), sorted(two)
    # ... in a standard and in a semi-coarsened transition
    assert any(t["rr_fused"] for r, l, t in TRANS if l < r["semi_xy"])


def test_small_level_kernels_run_with_every_last_brick_width():
    post = {t["last_brick"][2] for _, _, t in TRANS if t["small_post"]}
    pre = {t["last_brick"][2] for _, _, t in TRANS if t["small_pre"]}
    assert post == {1, 2, 3, 4}, post
    # k_small_pre_rr needs the zero guess as a flag: a level below the finest that passes fast_path_ok. In fp32 those have
    # n % 4 == 1, whose coarse level has nc % 4 in {1, 3}
    assert pre == {1, 2, 3, 4}, pre
    for dtype, want in ((po.MG_F64, {1, 2, 3, 4}), (po.MG_F32, {1, 3})):
        assert {t["last_brick"][2] for r, _, t in TRANS if t["small_pre"] and r["dtype"] == dtype} == want, dtype
        assert {t["last_brick"][2] for r, _, t in TRANS if t["small_post"] and r["dtype"] == dtype} == {1, 2, 3, 4}, dtype
    # the post kernel without the pre kernel before it on the same level (real zeroing, sweeps, then the brick kernel)
    assert any(t["small_post"] and not t["small_pre"] and l > 0 for _, l, t in TRANS)
    # on the standard transitions of a semi-coarsened hierarchy (nz != nx), with and without the pre kernel
    assert {t["small_pre"] for r, _, t in TRANS if t["small_post"] and r["semi_xy"]} == {True, False}


def test_kernel_families_alternate_within_a_hierarchy():
    # a generic level of rows >= 33 between fast transfers, below a fast level
    def mixed(r, p):
        lv, tr = p["levels"], p["transitions"]
        return any(lv[l]["n"] >= 33 and lv[l]["family"] == "generic" and lv[l - 1]["family"] == "fast"
                   and tr[l - 1]["prolong_fast"] and (tr[l - 1]["rr_fused"] or r["restriction"] == po.RESTRICT_INJECT)
                   for l in range(1, len(lv)))
    hits = [r for r, p in PLANS if mixed(r, p)]
    assert {r["smoother"] for r in hits} >= {po.SMOOTH_JACOBI, po.SMOOTH_RBGS}, [r["id"] for r in hits]
    assert any(p["transitions"][0]["rr_fused"] for r, p in PLANS if r in hits and r["smoother"] == po.SMOOTH_JACOBI)
    # the zero-guess flag handed from one family to another, and withheld: fast -> small with the flag, fast -> generic
    # and fast -> small without it
    pairs = {(p["levels"][l - 1]["family"], p["levels"][l]["family"], p["levels"][l]["u_zero"])
             for _, p in PLANS for l in range(1, len(p["levels"]) - 1)}
    assert {("fast", "small", True), ("fast", "small", False), ("fast", "generic", False), ("fast", "fast", True),
            ("fast", "fast", False), ("small", "small", True), ("small", "small", False)} <= pairs, pairs
    # a level with nx % V == 0, in both precisions
    for dtype in (po.MG_F64, po.MG_F32):
        assert any(x["n"] % st._V(dtype) == 0 for r, x in LEVELS if r["dtype"] == dtype), dtype
    # the coarsest grid swept by the level kernels (fixed sweeps on more points than the one-workgroup solver takes)
    assert {p["coarse_swept"] for _, p in PLANS} == {True, False}


def test_expected_launches_agree_with_the_sweep_count_table():
    """the launch counts this table predicts are the ones tests/test_sweep_counts_gpu.py states for its own rows"""
    from tests import test_sweep_counts_gpu as sc
    for row in sc.ROWS:
        d = row["desc"]
        for nu in row["nus"]:
            r = st.make_row(row["id"], d["n"], d["levels"], d["dtype"], d["smoother"], omega=d["omega"], restriction=d["restriction"],
                        nu=nu, dim=d["dim"], semi_xy=d.get("semi_xy", 0), aniso=d.get("aniso", st.ISO))
            for off in ((), ("MG_FUSED_PAIR",), ("MG_FUSED_RB",), ("MG_FUSED_PROLONG",), ("MG_SMALL_FUSED",)):
                assert st.expected_launches(r, off) == sc.expected(row, nu, off), (row["id"], nu, off)
