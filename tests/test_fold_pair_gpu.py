"""tools/foldcheck (built by __graft_entry__.build() next to tools/pairbench): the wide-tile smoothing pairs of
mg_pair_wide.hip against k_jacobi2 -- the kernel the parity suite pins to the oracle -- through the product's launchers, on
the smallest geometries at which each path of the tile engages, every 32-bit word of the output allocation (ghost planes
and padding included).

Shapes (the gate wants rows of exactly 128 or 256 lanes, >= 200 rows, >= 8 planes): fp64 513 x 203 x 9 and x 23 (256 lanes,
34 tiles of 6 output rows, the last one partial; coarse 257 x 102 x 5 / x 12), fp64 257 x 201 x 9 (128 lanes, 8 groups),
fp32 1025 x 201 x 9 and 513 x 201 x 9; each with omega = 6/7 and omega = 1, as J(J(u + P e)), J(J(u)), J(J(0)), the
norm-carrying pair and the red-black sweeps. The folding pair also on slab pieces (two ghost planes, coarse planes by
global index; 10 to 13 planes: whole slab, interior, the two boundary pieces in one launch, two 8-plane pieces an odd and an
even number of planes apart) and, in child processes with MG_PW_ZC = 3 / 4 and MG_PW_MODE = 0, with chunks that start on odd
and on even planes and with workgroups that change tile inside a launch: wherever the kernel sets up its coarse rows anew."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EXE = os.path.join(ROOT, "tools", "foldcheck")

GROUPS = [
    ("f64-513", {}),
    ("f64-257", {}),
    ("f32-1025", {}),
    ("f32-513", {}),
    ("slab", {}),
    ("fold", {"MG_PW_ZC": "3"}),
    ("fold", {"MG_PW_ZC": "4"}),
    ("fold", {"MG_PW_MODE": "0"}),
]


@pytest.mark.parametrize("group,env", GROUPS, ids=[g + "".join("-%s=%s" % kv for kv in e.items()) for g, e in GROUPS])
def test_wide_tile_pairs_equal_k_jacobi2_bit_for_bit(group, env):
    assert os.path.exists(EXE), "tools/foldcheck is not built (python __graft_entry__.py build)"
    child = {k: v for k, v in os.environ.items() if k not in ("MG_PW_ZC", "MG_PW_MODE", "MG_PAIR_WIDE")}
    child.update(env)
    p = subprocess.run([EXE, group], capture_output=True, text=True, timeout=300, cwd=ROOT, env=child)
    tail = p.stdout[-4000:] + p.stderr[-2000:]
    assert p.returncode == 0, tail
    assert "foldcheck %s:" % group in p.stdout and "all bit-equal" in p.stdout and "MISMATCH" not in p.stdout, tail
    assert p.stdout.count("bit-equal") > 2, tail   # the cases ran
