"""The storage around the dense grids, after every kernel entry point (tests/storage_table.py has the rows and the cases).

Every level-shaped array is (nz + 2 ghost) planes x ny rows x pitch elements; mg_get_array returns the
dense part only, so the bit-pinned tests of the other files cannot see a tail-line store that puts a value into a padding
column, a store one plane too low that lands in a ghost plane, or a kernel that reads a word out there without masking it.
mg_debug_raw_* returns whole allocations. For every (row, case, dtype):

 (a) from a clean state -- dense inputs filled with seeded normals through the ordinary setters -- every padding word and
     every ghost-plane word of every array is +0 by bit pattern after the call, every array outside the row's written set
     keeps every word, and the dense part of the raw copy is what mg_get_array returns;
 (b) with a quiet NaN in every padding column and ghost plane of every array, the dense outputs and the returned scalars
     are those of (a) bit for bit, and the arrays outside the written set keep every word, sentinels included;
 (c) the comparison of (a) finds a single planted word, in a padding column and in a ghost plane, at its coordinate.
"""
import struct
import zlib

import numpy as np
import pytest
import torch  # noqa: F401  (first: the device rows' tensors and the library must find the same HIP runtime)

from multigrid_prj_amd import capi
from tests import storage_table as st
from tests.storage_table import LEVEL, VC, EIG

pytestmark = pytest.mark.gpu


class Ctx:
    """one handle of a (case, dtype) with its seeded inputs"""

    def __init__(self, s, case, dtype):
        self.s, self.case, self.dtype = s, case, dtype
        self.T = np.float64 if dtype == capi.MG_F64 else np.float32
        self.seed = zlib.crc32(case.id.encode())
        self.coef_dirty = False
        self._extra, self._fill = {}, {}

    def extra(self, k, T=None):
        """the k-th spare level-0 array of normals (the same in every run of the case)"""
        T = T or self.T
        if (k, T) not in self._extra:
            self._extra[(k, T)] = np.random.default_rng([self.seed, 1000 + k]).standard_normal(self.s.level_shape(0)).astype(T)
        return self._extra[(k, T)]

    def fill_levels(self):
        for l in range(self.case.levels):
            for a in range(5):
                if not self.s.debug_raw_layout(LEVEL, a, l).allocated:
                    continue
                if (a, l) not in self._fill:
                    self._fill[(a, l)] = np.random.default_rng([self.seed, a, l]).standard_normal(self.s.level_shape(l)).astype(self.T)
                self.s.set_array(a, l, self._fill[(a, l)])


def layouts(x):
    out = {}
    for space, count in st.SPACE_INDICES.items():
        for l in range(1 if space in st.LEVEL0_ONLY else x.case.levels):
            for idx in range(count):
                i = x.s.debug_raw_layout(space, idx, l)
                if i.allocated:
                    out[(space, idx, l)] = st.Layout(i.elem_size, i.nx, i.ny, i.nz, i.pitch, i.ghost)
    return out


def snapshot(x):
    return {k: (lay, x.s.debug_raw_get(*k)) for k, lay in layouts(x).items()}


def poison(x, skip):
    """a quiet NaN in every padding column and ghost plane of every allocated array but those of `skip`; -> what was uploaded"""
    out = {}
    for k, (lay, raw) in snapshot(x).items():
        if (k[0], k[1]) not in skip:
            st.fill_outside(raw, lay, np.nan)
            x.s.debug_raw_set(*k, raw)
        out[k] = (lay, raw)
    return out


def name(k):
    space, idx, l = k
    what = ("U", "E", "RHS", "TMP", "RES")[idx] if space == LEVEL else f"{st.SPACE_NAME[space]}[{idx}]"
    return f"{what}({l})"


def first_diff(a, b):
    d = st.bits(a) != st.bits(b)
    return int(d.sum()), tuple(int(v) for v in np.argwhere(d)[0])


def dense_getter(x, k):
    space, idx, l = k
    if space == LEVEL:
        return x.s.get_array(idx, l)
    if space == VC:
        return x.s.vc_get_coefficient(l)
    if space == EIG:
        return x.s.eig_get_vector(idx // capi.EIG_MAX_BLOCK, idx % capi.EIG_MAX_BLOCK)
    return None


def same_scalars(a, b):
    enc = lambda t: [e if isinstance(e, bytes) else struct.pack("d", float(e)) for e in t]
    return enc(a) == enc(b)


def reset(x):
    """the handle-wide settings of the extension families back to their defaults (handles are shared between rows)"""
    s = x.s
    s.set_shift(0.0); s.heat_set_source(None)
    s.bc_set_faces(0); s.bc_set_form(0); s.vc_set_faces(0); s.vc_set_form(0)
    s.fas_set_reaction(capi.FAS_CUBIC, 0.0); s.fas_set_form(0)


def scrub(x):
    """+0 back into every padding column and ghost plane, and level arrays without NaNs: the state a handle starts from"""
    for k, (lay, raw) in snapshot(x).items():
        finite = bool(np.isfinite(st.dense_view(raw, lay)).all())
        if st.first_outside_nonzero(raw, lay)[0] or not finite:
            if not finite:   # a result of the poisoned runs: nothing later may start from it
                st.dense_view(raw, lay)[...] = 1.0
                x.coef_dirty = x.coef_dirty or k[0] == VC
            st.fill_outside(raw, lay, 0.0)
            x.s.debug_raw_set(*k, raw)


def one(x, row, v, poisoned, ref, fails):
    """one variant on the handle of its descriptor -> (scalars, {key: dense output}); failure messages are appended"""
    tag = f"[{v['id']}]"
    reset(x)
    row.setup(x, v)
    x.fill_levels()
    before = poison(x, {(sp, idx) for sp, idx, _ in row.relies_on_zero}) if poisoned else snapshot(x)
    scalars = row.call(x, v)
    after = snapshot(x)
    written = row.writes(x, v)
    dense = {k: st.dense_view(after[k][1], after[k][0]).copy() for k in written if k in after}
    for k in written - set(after):
        fails.append(f"{tag} {name(k)} is in the written set but not allocated")
    for k, (lay, raw) in after.items():
        if k not in written:
            if k not in before:
                fails.append(f"{tag} {name(k)} was allocated by the call but is not in its written set")
            elif not np.array_equal(st.bits(raw), st.bits(before[k][1])):
                cnt, (z, y, xx) = first_diff(raw, before[k][1])
                fails.append(f"{tag} {name(k)} is not in the written set but changed: {cnt} words, first (z, y, x) = "
                             f"({z - lay.gh}, {y}, {xx})")
        if not poisoned:
            cnt, kind, at = st.first_outside_nonzero(raw, lay)
            if cnt:
                fails.append(f"{tag} {name(k)}: {cnt} words outside the dense grid are not +0, first in the {kind} at "
                             f"(z, y, x) = {at}: {raw[at[0] + lay.gh, at[1], at[2]]!r}")
            if k in written:
                got = dense_getter(x, k)
                if got is not None and not np.array_equal(st.bits(got), st.bits(dense[k].reshape(got.shape))):
                    fails.append(f"{tag} {name(k)}: the dense part of the raw copy is not what the getter returns")
    if poisoned:
        ref_scalars, ref_dense = ref
        if not same_scalars(scalars, ref_scalars):
            fails.append(f"{tag} returned scalars depend on what lies outside the dense grid: {scalars!r} != {ref_scalars!r}"[:400])
        for k in sorted(dense):
            if k in ref_dense and not np.array_equal(st.bits(dense[k]), st.bits(ref_dense[k])):
                cnt, at = first_diff(dense[k], ref_dense[k])
                fails.append(f"{tag} {name(k)} depends on what lies outside the dense grid: {cnt} words differ, first "
                             f"(z, y, x) = {at}: {dense[k][at]!r} != {ref_dense[k][at]!r}")
    return scalars, dense


# Creating a handle costs more than a row's calls on a small grid, so the handles of one (case, dtype) are shared by its rows
# (PARAMS is ordered by case): one per descriptor, closed when the next case begins.
_handles = {}


def close_handles():
    for x in _handles.values():
        x.s.close()
    _handles.clear()


def handle(case, dtype, d):
    if _handles and next(iter(_handles))[:2] != (case.id, dtype):
        close_handles()
    key = (case.id, dtype, tuple(sorted(d.items())))
    if key not in _handles:
        _handles[key] = Ctx(capi.Solver(capi.make_desc(**st.base_desc(case, dtype, **d))), case, dtype)
    return _handles[key]


@pytest.fixture(scope="module", autouse=True)
def _handles_closed_at_the_end():
    yield
    close_handles()


def run(row, case, dtype):
    """every variant of the row on the case: all of them clean, then all of them poisoned -> (failures of a, failures of b)"""
    fails_a, fails_b = [], []
    variants = row.variants(case, dtype)
    descs = []
    for v in variants:
        if v["desc"] not in descs:
            descs.append(v["desc"])
    for d in descs:
        x = handle(case, dtype, d)
        vs = [v for v in variants if v["desc"] == d]
        clean = [one(x, row, v, False, None, fails_a) for v in vs]
        try:
            for v, ref in zip(vs, clean):
                one(x, row, v, True, ref, fails_b)
        finally:
            scrub(x)
    return fails_a, fails_b


_last = {}   # the last pair run: check (b) of a pair follows its check (a)


def run_cached(p):
    key = st.pair_id(p)
    if key not in _last:
        _last.clear()
        _last[key] = run(*p)
    return _last[key]


PAIRS = sorted(st.pairs(), key=lambda p: (p[1].id, p[2]))   # stable: the rows of a case keep the table's order
PARAMS = [pytest.param(p, check, id=f"{st.pair_id(p)}-{check}") for p in PAIRS for check in "ab"]


@pytest.mark.parametrize("p,check", PARAMS)
def test_storage(p, check):
    """check a: the invariant from a clean state; check b: independence from what lies outside the dense grid"""
    fails = run_cached(p)["ab".index(check)]
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:12])


# ---------------------------------------------------------------- (c) the checker checks
@pytest.mark.parametrize("dtype", [capi.MG_F64, capi.MG_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("where", ["padding", "ghost-low", "ghost-high"])
def test_a_planted_word_is_found_at_its_coordinate(where, dtype):
    case = st.C(3, 35, 2)
    with capi.Solver(capi.make_desc(**st.base_desc(case, dtype))) as s:
        x = Ctx(s, case, dtype)
        x.fill_levels()
        lay = layouts(x)[(LEVEL, capi.ARR_E, 0)]
        assert lay.pitch > lay.nx and lay.gh == 1 and lay == st.layout_of(3, 35, 35, np.dtype(x.T).itemsize)
        raw = s.debug_raw_get(LEVEL, capi.ARR_E, 0)
        assert raw.shape == st.raw_shape(lay) and st.first_outside_nonzero(raw, lay) == (0, None, None)
        assert np.array_equal(st.dense_view(raw, lay), s.get_array(capi.ARR_E, 0))
        z, y, xx = {"padding": (7, 11, lay.nx), "ghost-low": (-1, 3, 5), "ghost-high": (lay.nz, 34, lay.pitch - 1)}[where]
        raw[z + lay.gh, y, xx] = -0.0 if where == "padding" else 3.0   # -0.0 is not +0
        s.debug_raw_set(LEVEL, capi.ARR_E, 0, raw)
        for k, (l2, got) in snapshot(x).items():
            want = (1, "padding" if where == "padding" else "ghost", (z, y, xx)) if k == (LEVEL, capi.ARR_E, 0) else (0, None, None)
            assert st.first_outside_nonzero(got, l2) == want, name(k)
        assert np.array_equal(s.get_array(capi.ARR_E, 0), x._fill[(capi.ARR_E, 0)])   # the dense part never saw it


def test_raw_window_refusals():
    import ctypes as C
    d = capi.make_desc(**st.base_desc(st.C(3, 17, 2), capi.MG_F32))
    with capi.Solver(d) as s:
        info = s.debug_raw_layout(st.MIXED, 1, 0)
        assert (info.allocated, info.elem_size, info.pitch, info.elems) == (0, 8, 32, 19 * 17 * 32)
        buf = np.zeros(19 * 17 * 32 + 1)
        ptr = buf.ctypes.data_as(C.c_void_p)
        for args, word in (((st.MIXED, 1, 0, ptr, 19 * 17 * 32 * 8, 0), "has not allocated"), ((LEVEL, 0, 0, ptr, 19 * 17 * 32 * 4 + 4, 0), "bytes"),
                           ((LEVEL, 4, 1, ptr, 8, 0), "has not allocated"), ((LEVEL, 5, 0, ptr, 8, 0), "index"), ((LEVEL, 0, 2, ptr, 8, 0), "level"),
                           ((st.KRYLOV, 0, 1, ptr, 8, 0), "level 0"), ((9, 0, 0, ptr, 8, 0), "space"), ((LEVEL, 0, 0, None, 19 * 17 * 32 * 4, 1), "null")):
            assert s.lib.mg_debug_raw_copy(s.h, *args) == -4
            msg = s.lib.mg_last_error().decode()
            assert msg.startswith("mg_debug_raw_copy: ") and word in msg, msg
    with capi.Solver(capi.make_desc(**st.base_desc(st.C(3, 33, 3), capi.MG_F64, dist_min_n=9)), device=0, rank=0, nranks=2, dry=True) as s:
        info = capi.MgDebugRawInfo()
        assert s.lib.mg_debug_raw_layout(s.h, LEVEL, 0, 0, C.byref(info)) == -4
        assert s.lib.mg_last_error().decode().startswith("mg_debug_raw_layout: distributed")
