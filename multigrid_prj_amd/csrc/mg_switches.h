// The environment switches of the library as plain struct fields: mg_switches.def is the table, this header its only reader
// (no other file of csrc/ or include/ calls getenv). Header-only, so that the tools which compile single .hip files need
// no further source.
#pragma once

#include <cstdlib>

namespace mg {

#define MG_SW_TYPE_ON bool
#define MG_SW_TYPE_INT(d) int
#define MG_SW_TYPE_REAL(d) double
#define MG_SW_READ_ON !(e && e[0] == '0')
#define MG_SW_READ_INT(d) (e ? atoi(e) : (d))
#define MG_SW_READ_REAL(d) (e ? atof(e) : (d))
#define MG_SW_FIELD(field, env, kind) MG_SW_TYPE_##kind field;
#define MG_SW_READ(field, env, kind) { const char *e = getenv(env); field = MG_SW_READ_##kind; }
#define MG_SW_NONE(field, env, kind)

// PROCESS scope: read once, by the first caller of switches()
struct Switches {
#define MG_SWITCH(field, env, kind, scope, group, desc) MG_SW_##scope(field, env, kind)
#define MG_SW_HANDLE MG_SW_NONE
#define MG_SW_PROCESS MG_SW_FIELD
#include "mg_switches.def"
#undef MG_SW_PROCESS
#define MG_SW_PROCESS MG_SW_READ
    Switches() {
#include "mg_switches.def"
    }
#undef MG_SW_PROCESS
#undef MG_SW_HANDLE
};

// HANDLE scope: read by Solver::init() of every handle, so a process can create handles under different values
struct HandleSwitches {
#define MG_SW_PROCESS MG_SW_NONE
#define MG_SW_HANDLE MG_SW_FIELD
#include "mg_switches.def"
#undef MG_SW_HANDLE
#define MG_SW_HANDLE MG_SW_READ
    HandleSwitches() {
#include "mg_switches.def"
    }
#undef MG_SW_HANDLE
#undef MG_SW_PROCESS
#undef MG_SWITCH
};

#undef MG_SW_TYPE_ON
#undef MG_SW_TYPE_INT
#undef MG_SW_TYPE_REAL
#undef MG_SW_READ_ON
#undef MG_SW_READ_INT
#undef MG_SW_READ_REAL
#undef MG_SW_FIELD
#undef MG_SW_READ
#undef MG_SW_NONE

// (a function-local static: its initialisation is thread-safe, which ranks running as threads of one process rely on)
inline const Switches &switches()
{
    static const Switches s;
    return s;
}

}  // namespace mg
