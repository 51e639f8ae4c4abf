"""Device-resident array I/O on the caller's stream (mg_*_device, include/mg_hip.h; kernel: mg_io.hip) on the GPU.

Device arrays are torch tensors, and every one of them is a slice of a flat guard buffer: 8 sentinel elements (NaNs with a
recognisable payload) before the slice and 8 after it, the slice starting 0 .. 3 elements further into the buffer from
one array to the next, so that the dense base takes every residue modulo 16 bytes.

* round trips, bit for bit: device set -> host get, host set -> device get, device set -> device get, on every level of
  six hierarchies and the arrays U, RHS, TMP, in the handle's dtype and in the other one (against numpy.astype);
* the same bits downstream: cycles and solves of a handle fed by the device calls against one fed by the host calls;
* ordering against the caller's stream with no synchronisation in between;
* the heat-source and mixed-precision variants against their host twins; a distributed (dry-run) geometry; refusals.
"""

import numpy as np
import pytest
import torch

from multigrid_prj_amd import capi

pytestmark = pytest.mark.gpu

NP = {capi.MG_F64: np.float64, capi.MG_F32: np.float32}
TT = {np.float64: torch.float64, np.float32: torch.float32}
IT = {np.float64: np.int64, np.float32: np.int32}
SENTINEL = {np.float64: 0x7FF8DEADBEEF0001, np.float32: 0x7FC0BEEF}   # quiet NaNs with a payload
GUARD = 8
V22 = dict(cycle=capi.CYCLE_V, smoother=capi.SMOOTH_JACOBI, omega=6.0 / 7.0, nu_pre=2, nu_post=2, restriction=capi.RESTRICT_FULLW,
           outer_pre_gs=0, coarse_mode=capi.COARSE_FIXED, coarse_maxit=8)


class Guarded:
    """a dense device array of `shape` inside a flat buffer of sentinels, `off` + 8 elements in"""

    def __init__(self, shape, npdt, off, values=None):
        self.npdt, self.n, self.lo = npdt, int(np.prod(shape)), off + GUARD
        self.buf = torch.empty(self.lo + self.n + GUARD, dtype=TT[npdt], device="cuda")
        self.bits = self.buf.view(torch.int64 if npdt is np.float64 else torch.int32)
        self.bits.fill_(SENTINEL[npdt])
        self.t = self.buf[self.lo:self.lo + self.n].view(shape)
        assert self.t.data_ptr() % 16 == (self.lo * self.buf.element_size()) % 16
        if values is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(values, npdt)))

    def host(self):
        return self.t.cpu().numpy()

    def sentinels_intact(self):
        b = self.bits.cpu().numpy()
        return bool((b[:self.lo] == SENTINEL[self.npdt]).all() and (b[self.lo + self.n:] == SENTINEL[self.npdt]).all())

    def untouched(self):
        """nothing was written: the slice still holds the sentinels too"""
        return bool((self.bits.cpu().numpy() == SENTINEL[self.npdt]).all())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(IT[a.dtype.type]), b.view(IT[b.dtype.type]))


SPECIALS = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, 1e40, -1e40]


def field(rng, shape, npdt, specials=True):
    """random normals with the special values scattered in: signed zeros, infinities, a NaN, the two round-to-even cases of
    double -> float and a double that overflows to inf. No value whose float image is subnormal (the contract leaves the
    flush mode open): normals smaller than 1e-30 in magnitude are replaced."""
    a = rng.standard_normal(shape)
    a[np.abs(a) < 1e-30] = 1.0
    if specials:
        flat = a.reshape(-1)
        pos = rng.choice(flat.size, size=min(len(SPECIALS), flat.size), replace=False)
        flat[pos] = SPECIALS[:len(pos)]
        flat[0], flat[-1] = -0.0, 1.0 + 3.0 * 2.0 ** -24    # the ragged head and tail of the first / last chunk
    with np.errstate(over="ignore"):
        return a.astype(npdt)


def cast(a, npdt):
    with np.errstate(over="ignore"):
        return a.astype(npdt)


# ---------------------------------------------------------------- 1. round trips
HANDLES = [
    ("2d17-f64", dict(dim=2, n=17, levels=3, dtype=capi.MG_F64)),       # rows of 17, 9, 5: shorter than one vector group
    ("2d17-f32", dict(dim=2, n=17, levels=3, dtype=capi.MG_F32)),
    ("2d1025-f32", dict(dim=2, n=1025, levels=2, dtype=capi.MG_F32)),   # 4100-byte rows: the row starts walk all four residues
    ("3d33-f64", dict(dim=3, n=33, levels=3, dtype=capi.MG_F64)),       # pitch 48 != nx
    ("3d49-f32", dict(dim=3, n=49, levels=3, dtype=capi.MG_F32)),       # 49, 25, 13: off 2^k + 1
    ("3d65-semi-f64", dict(dim=3, n=65, levels=4, dtype=capi.MG_F64, semi_xy=2)),   # levels whose nz differs from n
    ("3d129-f64", dict(dim=3, n=129, levels=2, dtype=capi.MG_F64)),     # 537 chunks of 31 rows, the last one short: many workgroups, one chunk each
]


@pytest.mark.parametrize("kw", [h[1] for h in HANDLES], ids=[h[0] for h in HANDLES])
def test_round_trips_bit_for_bit(kw):
    rng = np.random.default_rng(kw["n"] * 10 + kw["dim"])
    kw = dict(kw, length=1.0, **(V22 if kw["dim"] == 3 else {}))
    count = 0
    with capi.Solver(capi.make_desc(**kw)) as s:
        own = s.np
        other = np.float32 if own is np.float64 else np.float64
        for level in range(kw["levels"]):
            shape = s.level_shape(level)
            for which in (capi.ARR_U, capi.ARR_RHS, capi.ARR_TMP):
                for dt in (own, other):
                    tag = (level, which, dt.__name__)
                    # device set -> host get
                    a = field(rng, shape, dt)
                    src = Guarded(shape, dt, count % 4, a); count += 1
                    s.set_array_device(which, level, src.t)
                    got = s.get_array(which, level)
                    assert same_bits(got, cast(a, own)), ("set_device/get_host", tag, int((got != cast(a, own)).sum()))
                    assert src.sentinels_intact() and same_bits(src.host(), a), tag
                    # host set -> device get
                    b = field(rng, shape, own)
                    s.set_array(which, level, b)
                    dst = Guarded(shape, dt, count % 4); count += 1
                    s.get_array_device(which, level, dst.t)
                    s.sync()
                    assert same_bits(dst.host(), cast(b, dt)), ("set_host/get_device", tag)
                    assert dst.sentinels_intact(), ("sentinels after get", tag)
                    # device set -> device get, source and destination at different residues
                    c = field(rng, shape, dt)
                    src = Guarded(shape, dt, count % 4, c); count += 1
                    dst = Guarded(shape, dt, (count + 1) % 4); count += 1
                    s.set_array_device(which, level, src.t)
                    s.get_array_device(which, level, dst.t)
                    torch.cuda.synchronize()
                    assert same_bits(dst.host(), cast(cast(c, own), dt)), ("set_device/get_device", tag)
                    assert dst.sentinels_intact() and src.sentinels_intact(), tag


# more chunks than the capped grid of 2048 workgroups takes in one stride: the chunk loop of k_io_copy runs more than once per
# workgroup (the image is refilled behind the closing barrier), as at every production size. 2-D 4097: rows longer than a
# chunk, cut into column segments (4096 + 1 columns: the last segment holds ONE dense element and 16 / 32 padded ones), 8194
# chunks; 3-D 257 is not needed beside it.
@pytest.mark.parametrize("dtype", [capi.MG_F64, capi.MG_F32], ids=["f64", "f32"])
def test_round_trips_beyond_one_grid_stride(dtype):
    rng = np.random.default_rng(4097)
    with capi.Solver(capi.make_desc(dim=2, n=4097, levels=2, dtype=dtype, length=1.0)) as s:
        own = s.np
        other = np.float32 if own is np.float64 else np.float64
        shape = s.level_shape(0)
        assert shape == (4097, 4097)
        for k, dt in enumerate((own, other)):
            tag = dt.__name__
            a = cast(rng.random(shape) - 0.5, dt)
            a[0, 0], a[-1, -1], a[1, 0], a[0, -1] = -0.0, 1.0 + 3.0 * 2.0 ** -24, np.inf, np.nan
            src = Guarded(shape, dt, k + 1, a)
            s.set_array_device(capi.ARR_U, 0, src.t)
            got = s.get_array(capi.ARR_U, 0)
            assert same_bits(got, cast(a, own)), ("set_device/get_host", tag, int((got != cast(a, own)).sum()))
            b = cast(rng.random(shape) - 0.5, own)
            b[0, 0], b[-1, -1], b[-1, 0] = 1.0 + 2.0 ** -24, -0.0, -np.inf
            s.set_array(capi.ARR_RHS, 0, b)
            dst = Guarded(shape, dt, k + 2)
            s.get_array_device(capi.ARR_RHS, 0, dst.t)
            s.sync()
            assert same_bits(dst.host(), cast(b, dt)), ("set_host/get_device", tag)
            assert dst.sentinels_intact() and src.sentinels_intact(), tag


def test_same_dtype_keeps_every_bit_pattern():
    """NaN payloads (quiet and signalling), -0.0, subnormals: with equal dtypes the copy moves bits"""
    for dtype in (capi.MG_F64, capi.MG_F32):
        npdt = NP[dtype]
        with capi.Solver(capi.make_desc(dim=3, n=17, levels=2, dtype=dtype, length=1.0, **V22)) as s:
            shape = s.level_shape(0)
            rng = np.random.default_rng(5)
            info = np.iinfo(IT[npdt])
            bits = rng.integers(info.min, info.max, size=shape, dtype=IT[npdt], endpoint=True)
            a = bits.view(npdt)
            src, dst = Guarded(shape, npdt, 1), Guarded(shape, npdt, 2)
            src.bits[src.lo:src.lo + src.n].copy_(torch.from_numpy(bits.reshape(-1)))
            s.set_array_device(capi.ARR_U, 0, src.t)
            assert same_bits(s.get_array(capi.ARR_U, 0), a)
            s.get_array_device(capi.ARR_U, 0, dst.t)
            s.sync()
            assert same_bits(dst.host(), a) and dst.sentinels_intact()


# ---------------------------------------------------------------- 2. the same bits downstream
@pytest.mark.parametrize("n,levels", [(65, 3), (129, 4)], ids=["65-small-levels", "129-pair-kernels"])
def test_same_bits_downstream(n, levels):
    """a corrupted padding column, a corrupted ghost plane or a stale rhs_halo_ok would show in the cycles that follow"""
    rng = np.random.default_rng(n)
    kw = dict(dim=3, n=n, levels=levels, length=1.0, **V22)
    with capi.Solver(capi.make_desc(**kw)) as a, capi.Solver(capi.make_desc(**kw)) as b:
        shape = a.level_shape(0)
        rhs, u0 = rng.standard_normal(shape), rng.standard_normal(shape)
        a.set_rhs(rhs); a.set_solution(u0)
        b.set_rhs_device(Guarded(shape, np.float64, 1, rhs).t); b.set_solution_device(Guarded(shape, np.float64, 2, u0).t)
        for s in (a, b):
            s.cycle(); s.cycle()
        ua, ub = a.get_solution(), b.get_solution()
        assert np.isfinite(ua).all() and np.array_equal(ua, ub)
        ha, _ = a.solve(0.0, 3)
        hb, _ = b.solve(0.0, 3)
        assert len(ha) == 4 and np.array_equal(ha, hb)
        out = Guarded(shape, np.float64, 3)
        b.get_solution_device(out.t)
        b.sync()
        assert np.array_equal(a.get_solution(), out.host()) and out.sentinels_intact()


# ---------------------------------------------------------------- 3. ordering against the caller's stream
def test_ordering_on_a_side_stream():
    n = 129
    kw = dict(dim=3, n=n, levels=4, length=1.0, **V22)
    rng = np.random.default_rng(3)
    with capi.Solver(capi.make_desc(**kw)) as s:
        shape = s.level_shape(0)
        start, rhs = rng.standard_normal(shape), rng.standard_normal(shape)
        expect = start.copy()
        for _ in range(20):
            expect *= 0.999
            expect += 0.25
        src, back, out = Guarded(shape, np.float64, 1, start), Guarded(shape, np.float64, 2), Guarded(shape, np.float64, 3)
        rhs_t = Guarded(shape, np.float64, 0, rhs)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(20):            # the producer: a chain of kernels the copy has to wait for
                src.t.mul_(0.999)
                src.t.add_(0.25)
            s.set_array_device(capi.ARR_U, 0, src.t, stream=side.cuda_stream)
            src.t.fill_(float("nan"))     # the caller reuses the array at once: the copy must have read it by then
            s.get_array_device(capi.ARR_U, 0, back.t, stream=side.cuda_stream)
            s.set_rhs_device(rhs_t.t, stream=side.cuda_stream)
            s.cycle_async(2)
            s.get_solution_device(out.t, stream=side.cuda_stream)
            clone = out.t.clone()          # the consumer: runs on the side stream after the copy
        torch.cuda.synchronize()           # the first synchronisation
        s.sync()
        assert np.array_equal(back.host(), expect)
        final = s.get_solution()
        assert np.isfinite(final).all() and not np.array_equal(final, expect)
        assert np.array_equal(clone.cpu().numpy(), final) and np.array_equal(out.host(), final)
        assert back.sentinels_intact() and out.sentinels_intact() and src.sentinels_intact()


# ---------------------------------------------------------------- 4. the driver variants
def test_heat_source_from_the_device():
    rng = np.random.default_rng(4)
    kw = dict(dim=3, n=33, levels=3, length=1.0, **V22)
    with capi.Solver(capi.make_desc(**kw)) as a, capi.Solver(capi.make_desc(**kw)) as b:
        shape = a.level_shape(0)
        u0, f = rng.standard_normal(shape), rng.standard_normal(shape) * 10.0
        base = a.device_bytes()
        assert b.device_bytes() == base
        a.set_solution(u0); b.set_solution_device(Guarded(shape, np.float64, 1, u0).t)
        b.heat_set_source_device(None)                      # nothing to remove, nothing allocated
        assert b.device_bytes() == base
        a.heat_set_source(f); b.heat_set_source_device(Guarded(shape, np.float64, 3, f).t)
        grown = a.device_bytes() - base
        assert grown > 0 and b.device_bytes() - base == grown
        sa, sb = a.heat_step(1e-3, 0.5, 2, 2), b.heat_step(1e-3, 0.5, 2, 2)
        ua = a.get_solution()
        assert np.array_equal(ua, b.get_solution()) and sa.relres == sb.relres
        b.heat_set_source_device(Guarded(shape, np.float32, 2, f).t)    # converted on the way in: the float image of f
        a.heat_set_source(f.astype(np.float32).astype(np.float64))
        assert b.device_bytes() - base == grown
        a.heat_step(1e-3, 0.5, 1, 2); b.heat_step(1e-3, 0.5, 1, 2)
        assert np.array_equal(a.get_solution(), b.get_solution())
        a.heat_set_source(None); b.heat_set_source_device(None)
        a.heat_step(1e-3, 0.5, 2, 2); b.heat_step(1e-3, 0.5, 2, 2)
        assert np.array_equal(a.get_solution(), b.get_solution())


def test_a_step_spelled_out_is_the_steppers_step():
    """INTEGRATION's worked example: under the shift 1 / (theta dt), mg_heat_rhs + one mg_cycle_async (outer_pre_gs = 0) per step
    with the source set from the device is mg_heat_step's step, bit for bit; the fp32 snapshot is the rounded solution"""
    rng = np.random.default_rng(14)
    kw = dict(dim=3, n=33, levels=3, length=1.0, **V22)
    dt, theta, nsteps = 1e-3, 0.5, 4
    with capi.Solver(capi.make_desc(**kw)) as a, capi.Solver(capi.make_desc(**kw)) as b:
        shape = a.level_shape(0)
        u0, f = rng.standard_normal(shape), rng.standard_normal(shape) * 10.0
        a.set_solution(u0); a.heat_set_source(f)
        a.heat_step(dt, theta, nsteps, 1)
        side = torch.cuda.Stream()
        f_t, u_t = Guarded(shape, np.float64, 1, f), Guarded(shape, np.float64, 2, u0)
        snap = Guarded(shape, np.float32, 3)
        work = torch.empty(shape, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            b.set_solution_device(u_t.t, stream=side.cuda_stream)
            b.set_shift(1.0 / (theta * dt))
            for _ in range(nsteps):
                torch.mul(f_t.t, 1.0, out=work)                    # the caller's kernel builds f(t_k) ...
                b.heat_set_source_device(work, stream=side.cuda_stream)
                work.fill_(float("nan"))                           # ... and reuses the array at once
                b.heat_rhs(dt, theta)
                b.cycle_async(1)
            b.get_solution_device(snap.t, stream=side.cuda_stream)
        torch.cuda.synchronize()
        ua = a.get_solution()
        assert np.isfinite(ua).all() and not np.array_equal(ua, u0)
        assert np.array_equal(ua, b.get_solution()) and a.get_shift() == b.get_shift()
        assert same_bits(snap.host(), ua.astype(np.float32)) and snap.sentinels_intact()


def test_mixed_from_the_device():
    rng = np.random.default_rng(6)
    kw = dict(dim=3, n=33, levels=3, length=1.0, dtype=capi.MG_F32, **V22)
    with capi.Solver(capi.make_desc(**kw)) as a, capi.Solver(capi.make_desc(**kw)) as b:
        shape = a.level_shape(0)
        rhs, u0 = rng.standard_normal(shape), rng.standard_normal(shape)
        base = a.device_bytes()
        a.mixed_set_rhs(rhs); b.mixed_set_rhs_device(Guarded(shape, np.float64, 1, rhs).t)
        grown = a.device_bytes() - base
        assert grown > 0 and b.device_bytes() - base == grown
        out = Guarded(shape, np.float64, 3)
        with pytest.raises(capi.MgError) as e:              # the host twin's rule: no solution yet
            b.mixed_get_solution_device(out.t)
        assert e.value.code == -4 and out.untouched()
        a.mixed_set_solution(u0); b.mixed_set_solution_device(Guarded(shape, np.float64, 2, u0).t)
        assert b.device_bytes() - base == grown
        ha, sta = a.mixed_solve(1e-12, 6, 2)
        hb, stb = b.mixed_solve(1e-12, 6, 2)
        assert len(ha) > 1 and ha[-1] < ha[0] and np.array_equal(ha, hb) and (sta.outer, sta.status) == (stb.outer, stb.status)
        b.mixed_get_solution_device(out.t)
        b.sync()
        ua = a.mixed_get_solution()
        assert np.array_equal(ua, out.host()) and np.array_equal(ua, b.mixed_get_solution()) and out.sentinels_intact()
        out32 = Guarded(shape, np.float32, 1)               # rounded on the way out
        b.mixed_get_solution_device(out32.t)
        b.sync()
        assert same_bits(out32.host(), ua.astype(np.float32)) and out32.sentinels_intact()


# ---------------------------------------------------------------- 5. distributed geometry
def test_dry_run_slab_geometry():
    """rank 1 of 3: local slabs with two ghost planes either side, a z offset, levels of different thickness"""
    rng = np.random.default_rng(7)
    desc = capi.make_desc(dim=3, n=65, levels=3, length=1.0, dist_min_n=17, **V22)
    with capi.Solver(desc, device=0, rank=1, nranks=3, dry=True) as s:
        for level in (0, 1):
            shape = s.level_shape(level)
            assert shape == (capi.plan_slab(desc, 3, 1, level)[1], s.level_n(level), s.level_n(level)) and shape[0] < shape[1]
            for which in (capi.ARR_U, capi.ARR_RHS):
                a = field(rng, shape, np.float64)
                src = Guarded(shape, np.float64, level + 1, a)
                s.set_array_device(which, level, src.t)
                assert same_bits(s.get_array(which, level), a)
                b = field(rng, shape, np.float64)
                s.set_array(which, level, b)
                dst = Guarded(shape, np.float64, level + 2)
                s.get_array_device(which, level, dst.t)
                s.sync()
                assert same_bits(dst.host(), b) and dst.sentinels_intact()


# ---------------------------------------------------------------- 6. refusals
def refused(call, *words):
    lib = capi.load()
    rc = call()
    msg = lib.mg_last_error().decode()
    assert rc == -4 and msg and all(w in msg for w in words), (rc, msg)


def test_refusals():
    rng = np.random.default_rng(8)
    lib = capi.load()
    with capi.Solver(capi.make_desc(dim=3, n=129, levels=2, length=1.0, **V22)) as s:
        shape = s.level_shape(0)
        ref = rng.standard_normal(shape)
        s.set_array(capi.ARR_U, 0, ref)
        good = Guarded(shape, np.float64, 1)
        small = torch.zeros(1024, dtype=torch.float64, device="cuda")      # a corner of a 2 MB allocator block; the level needs 17 MB
        host = np.zeros(shape)
        torch.cuda.synchronize()
        before = s.device_bytes()
        gp, sp, hp = good.t.data_ptr(), small.data_ptr(), host.ctypes.data
        for fn in (lib.mg_set_array_device, lib.mg_get_array_device):
            refused(lambda: fn(s.h, 7, 0, gp, capi.MG_F64, None), "no such array")
            refused(lambda: fn(s.h, capi.ARR_U, 2, gp, capi.MG_F64, None), "no such array")
            refused(lambda: fn(s.h, capi.ARR_RES, 1, gp, capi.MG_F64, None), "no such array")
            refused(lambda: fn(s.h, capi.ARR_U, 0, gp, 5, None), "dtype")
            refused(lambda: fn(s.h, capi.ARR_U, 0, None, capi.MG_F64, None), "null")
            refused(lambda: fn(s.h, capi.ARR_U, 0, gp + 4, capi.MG_F64, None), "aligned")
            refused(lambda: fn(s.h, capi.ARR_U, 0, hp, capi.MG_F64, None), "not device memory")
            refused(lambda: fn(s.h, capi.ARR_U, 0, sp, capi.MG_F64, None), "allocation ends before")
            refused(lambda: fn(s.h, capi.ARR_U, 0, sp, capi.MG_F32, None), "allocation ends before")
        refused(lambda: lib.mg_heat_set_source_device(s.h, hp, capi.MG_F64, None), "not device memory")
        refused(lambda: lib.mg_heat_set_source_device(s.h, sp, capi.MG_F64, None), "allocation ends before")
        refused(lambda: lib.mg_heat_set_source_device(s.h, None, 9, None), "dtype")
        assert s.device_bytes() == before                                    # nothing was allocated for a refused source
        for fn in (lib.mg_mixed_set_rhs_device, lib.mg_mixed_set_solution_device, lib.mg_mixed_get_solution_device):
            refused(lambda: fn(s.h, gp, capi.MG_F64, None), "MG_F32")
        assert s.device_bytes() == before
        torch.cuda.synchronize(); s.sync()
        assert good.untouched() and not small.any().item()
        assert np.array_equal(s.get_array(capi.ARR_U, 0), ref)
        # HIP's sticky error was cleared: the next calls work
        s.get_array_device(capi.ARR_U, 0, good.t)
        s.sync()
        assert np.array_equal(good.host(), ref) and good.sentinels_intact()
    with capi.Solver(capi.make_desc(dim=3, n=33, levels=2, length=1.0, dtype=capi.MG_F32, **V22)) as s32:
        before = s32.device_bytes()
        for fn in (lib.mg_mixed_set_rhs_device, lib.mg_mixed_set_solution_device):
            refused(lambda: fn(s32.h, hp, capi.MG_F64, None), "not device memory")
            refused(lambda: fn(s32.h, None, capi.MG_F64, None), "null")
        assert s32.device_bytes() == before                                  # nothing was allocated for a refused array
    desc = capi.make_desc(dim=3, n=65, levels=3, length=1.0, dist_min_n=17, dtype=capi.MG_F32, **V22)
    with capi.Solver(desc, device=0, rank=1, nranks=3, dry=True) as d:
        slab = Guarded(d.level_shape(0), np.float32, 0)
        p = slab.t.data_ptr()
        refused(lambda: lib.mg_heat_set_source_device(d.h, p, capi.MG_F32, None), "distributed")
        for fn in (lib.mg_mixed_set_rhs_device, lib.mg_mixed_set_solution_device, lib.mg_mixed_get_solution_device):
            refused(lambda: fn(d.h, p, capi.MG_F32, None), "distributed")
        torch.cuda.synchronize()
        assert slab.untouched()


def test_python_mirror_refuses_before_the_library():
    with capi.Solver(capi.make_desc(dim=2, n=17, levels=2, length=1.0)) as s:
        with pytest.raises(ValueError, match="shape"):
            s.set_array_device(capi.ARR_U, 0, torch.zeros(17, 16, dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError, match="strides"):
            s.set_array_device(capi.ARR_U, 0, torch.zeros(17, 17, dtype=torch.float64, device="cuda").t())
        with pytest.raises(ValueError, match="typestr"):
            s.get_array_device(capi.ARR_U, 0, torch.zeros(17, 17, dtype=torch.float16, device="cuda"))
        with pytest.raises(ValueError, match="__cuda_array_interface__"):
            s.set_array_device(capi.ARR_U, 0, np.zeros((17, 17)))
