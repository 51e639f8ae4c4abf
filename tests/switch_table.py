"""Reader of multigrid_prj_amd/csrc/mg_switches.def, the one table of the library's environment switches: the GPU tests take
the names of the switches they turn off from it, tests/test_switch_table.py checks the table against the sources and DESIGN.md."""
import os
import re
from collections import namedtuple

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEF = os.path.join(ROOT, "multigrid_prj_amd", "csrc", "mg_switches.def")

Switch = namedtuple("Switch", "field env kind default scope group desc")

_ROW = re.compile(r'^MG_SWITCH\(\s*(\w+)\s*,\s*"(MG_[A-Z0-9_]+)"\s*,\s*(ON|INT|REAL)(?:\(([^)]*)\))?\s*,\s*(PROCESS|HANDLE)\s*,\s*'
                  r'(FALLBACK|TUNING|POLICY)\s*,\s*"([^"]*)"\s*\)\s*$')


def rows():
    out = []
    with open(DEF) as f:
        for line in f:
            if not line.startswith("MG_SWITCH("):
                assert line.startswith("//") or not line.strip(), line
                continue
            m = _ROW.match(line)
            assert m, "unreadable row: " + line
            field, env, kind, default, scope, group, desc = m.groups()
            out.append(Switch(field, env, kind, "on" if kind == "ON" else default, scope, group, desc))
    assert len({s.env for s in out}) == len(out) == len({s.field for s in out})
    return out


def names(group=None):
    return {s.env for s in rows() if group in (None, s.group)}


def fallbacks(*envs):
    """the given names, checked to be FALLBACK rows of the table (a switch set to 0 that the library no longer reads proves nothing)"""
    unknown = set(envs) - names("FALLBACK")
    assert not unknown, f"not a FALLBACK row of mg_switches.def: {sorted(unknown)}"
    return tuple(envs)
