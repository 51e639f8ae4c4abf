"""CPU-side checks of the variable-coefficient operator in mg_mixed_solve / mg_mixed_kernel (MG_MIXED_OPERATOR,
MG_MIXED_INNER_PCG, include/mg_hip.h): the ctypes binding agrees with the C header on the three constants, no entry point was
added for them, null-handle calls with the flags are refused before any device work, every kernel of mg_vc_mixed.hip compiles
for gfx950 without spilling to scratch, and the gate of its marching tile is mg_geom.h's march_ok with 8-byte elements."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from multigrid_prj_amd import build as mgbuild
from multigrid_prj_amd import capi
from tests import mixedvc_ref as mr
from tests import vcn_ref as vn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_constants_match_header(tmp_path):
    src = tmp_path / "flags.c"
    src.write_text('#include <stdio.h>\n#include "mg_hip.h"\n'
                   'int main(void){printf("%d %d %d %d %d\\n", MG_MIXED_ON_CONSTANT, MG_MIXED_ON_COEFFICIENT, MG_MIXED_INNER_PCG,'
                   ' MG_MIXED_OPERATOR(MG_MIXED_ON_COEFFICIENT), 7 | MG_MIXED_OPERATOR(MG_MIXED_ON_COEFFICIENT) | MG_MIXED_INNER_PCG);'
                   ' return 0;}\n')
    exe = tmp_path / "flags"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [capi.MIXED_ON_CONSTANT, capi.MIXED_ON_COEFFICIENT, capi.MIXED_INNER_PCG, capi.mixed_operator(capi.MIXED_ON_COEFFICIENT),
            7 | capi.mixed_operator(capi.MIXED_ON_COEFFICIENT) | capi.MIXED_INNER_PCG]
    assert got == want == [0, 2, 1 << 20, 2 << 16, 7 | (2 << 16) | (1 << 20)]


def test_no_new_entry_point():
    """flags in arguments the two calls already have: nothing named after the feature is exported or bound"""
    lib = capi.load(build_if_missing=True)
    assert not [e for e in capi.EXPORTS if "mixed_vc" in e or "vc_mixed" in e or "mixedvc" in e]
    for sym in ("mg_mixed_vc_solve", "mg_vc_mixed_solve", "mg_mixed_solve_vc"):
        assert not hasattr(lib, sym)
    import inspect
    assert list(inspect.signature(capi.Solver.mixed_solve).parameters)[-2:] == ["op", "inner_pcg"]
    assert list(inspect.signature(capi.Solver.mixed_kernel).parameters)[-1] == "op"


def test_null_handle_refused_with_flags():
    lib = capi.load()
    st = capi.MgMixedStats()
    n = C.c_int(0)
    op = capi.mixed_operator(capi.MIXED_ON_COEFFICIENT)
    for arg in (2 | op, 8 | op | capi.MIXED_INNER_PCG, 2 | capi.mixed_operator(1), 2 | capi.MIXED_INNER_PCG, op):
        assert lib.mg_mixed_solve(None, 1e-8, 10, arg, None, 0, C.byref(n), C.byref(st)) == -4
        assert b"null handle" in lib.mg_last_error()
    for k in (capi.MIXED_K_RESIDUAL, capi.MIXED_K_CORRECT_RESIDUAL):
        assert lib.mg_mixed_kernel(None, k | op, 1.0, 1.0, 0, 2, None) == -4
        assert b"null handle" in lib.mg_last_error()


def test_kernels_compile_without_scratch(tmp_path):
    """every kernel of mg_vc_mixed.hip: 0 bytes of scratch per lane (no register spills) with the library's own flags"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in mgbuild.FLAGS if f != "-shared"]
    assert "mg_vc_mixed.hip" in mgbuild.SOURCES
    r = subprocess.run([hipcc, *flags, "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(mgbuild.CSRC, "mg_vc_mixed.hip"), "-o", str(tmp_path / "mg_vc_mixed.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch)
    kernels = {n: s for n, s in zip(names, scratch)}
    # the tile (mask 0): first residual, correction by the reciprocal or by division; the plain form: the same in 2-D and 3-D
    assert sum("k_vc_mixed_march" in n for n in kernels) == 3 and sum("k_vc_mixed_plain" in n for n in kernels) == 6, names
    assert all(s == 0 for s in kernels.values()), kernels


MAIN = r"""
#include <cstdio>
#include "mg_geom.h"
int main()
{
    int dim, nx, ny, nz;
    while (scanf("%d %d %d %d", &dim, &nx, &ny, &nz) == 4) printf("%d\n", mg::vc_mixed_march_ok(dim, nx, ny, nz) ? 1 : 0);
    return 0;
}
"""


def test_tile_gate_is_march_ok_with_eight_byte_elements(tmp_path):
    """mg_geom.h's vc_mixed_march_ok against vcn_ref.march_ok(..., 8): the fp64 arrays decide, so 33^3 takes the tile on an fp32
    handle whose own vc kernels are plain there"""
    src, exe = tmp_path / "gate.cpp", tmp_path / "gate"
    src.write_text(MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + mgbuild.CSRC, str(src), "-o", str(exe)], check=True)
    cases = []
    for n in (3, 7, 9, 17, 25, 31, 32, 33, 34, 35, 63, 64, 65, 66, 67, 97, 129, 513):
        cases += [(3, n, n, n), (2, n, n, 1)]
    cases += [(3, 33, 33, 5), (3, 33, 5, 33), (3, 17, 17, 513), (3, 65, 9, 9)]
    text = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split()
    want = [int(vn.march_ok(*c, 8)) for c in cases]
    assert [int(v) for v in out] == want
    by = dict(zip(cases, want))
    assert by[3, 17, 17, 17] == 0 and by[3, 31, 31, 31] == 0 and by[3, 32, 32, 32] == 1 and by[3, 33, 33, 33] == 1 and by[2, 97, 97, 1] == 0
    assert not vn.march_ok(3, 33, 33, 33, 4)   # the fp32 handle's own vc kernels are plain at 33^3
    src_text = open(os.path.join(mgbuild.CSRC, "mg_vc_mixed.hip")).read()
    assert "vc_mixed_march_ok(g64.dim, g64.nx, g64.ny, g64.nz)" in src_text   # the launcher asks this function,
    assert "if (mask == 0 && vc_mixed_march_takes(g64, plain))" in src_text     # and a non-zero mask takes the plain form


def test_reference_loop_reproduces_the_table():
    """the numpy loop of tests/mixedvc_ref.py on the first row of the table in tests/test_mixedvc_gpu.py: 12 corrections of two
    float32 cycles to 3e-11 (8.6e-11 -> 1.1e-11); the float64 residual of the result is the last entry"""
    mask, sigma = vn.FACES["only-y-hi-dirichlet"]
    P64, P32 = mr.problems(vn.FIELDS["smooth"](33), mask, sigma)
    b = vn.convergence_rhs(P64.shape(0))
    u, hist, b_out, outer, relres = mr.mixed_loop(P64, P32, b, np.zeros_like(b), 2, False, 3e-11, 40)
    print(hist)
    assert outer == 12 and len(hist) == 13 and 7.5e-11 < hist[-2] < 1e-10 and 1e-11 < hist[-1] < 1.2e-11
    assert relres == hist[-1] and np.array_equal(b_out, b)
    dm = P64.dirichlet(b.shape)
    assert np.array_equal(u[dm], b[dm])
