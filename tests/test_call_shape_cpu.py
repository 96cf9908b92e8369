"""csrc/call_shape.h — what one call on a handle consists of — against the table it was transcribed from, row by row.  The header is
pure host code: tests/c_abi/call_shape_table.cpp includes it alone, is compiled with g++ and the address / undefined-behaviour
sanitizers, and prints one line per (route facts, mode); the rows below are literals, written from the table and not from the code.

  route, mode                pre-passes               kernel in / out            launch              expand                      last_vals
  Plain, any                 none                     caller's                   plain               none                        unchanged
  Direct, NEWTON             inertia unless count_d   caller's; d -> d2 unless   staged if staged    unless lean_rows: (d_outer  unchanged
                                                      d_outer                                        ? null : d2, success, 0)
  Direct, FACTOR             inertia unless count_d   caller's                   staged if staged    none                        set
  Direct, SOLVE, v2_solve    none                     last_vals, caller's        staged if staged    unless lean_rows:           needed
                                                                                                     (null, null, 0)
  Condensed, NEWTON          whole system, inertia    cbuf -> d2                 plain               (d2, success, 1)            unchanged
  Condensed, FACTOR          matrix only, inertia     cbuf                       plain               none                        set
  Condensed, SOLVE; Direct   rhs only                 cbuf -> d2                 plain               (d2, null, 0)               needed
    SOLVE without v2_solve
  GeneralDense               as Condensed             cbuf -> d2                 dense route         NEWTON (d2, success, 0),    FACTOR sets,
                                                                                                     SOLVE (d2, null, 0)         SOLVE needs
The extra inertia counts go to the launch exactly where the inertia pass runs.  Band: one band launch on the caller's arrays, FACTOR
sets and SOLVE needs last_vals (the band solve factorises them again); Dense: the dense backend keeps its own factor."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("NEWTON", "FACTOR", "SOLVE")

NOTHING = "condense=- inertia=0 in=caller d=caller extra=0 launch={launch} expand=- last_vals={last}"
PLAIN = [NOTHING.format(launch="kernel", last="unchanged")] * 3
DENSE = [NOTHING.format(launch="dense", last="unchanged")] * 3
BAND = [NOTHING.format(launch="band", last=last) for last in ("unchanged", "set", "needed")]
CONDENSED = ["condense=whole inertia=1 in=cbuf d=d2 extra=1 launch=kernel expand=d2,success,1 last_vals=unchanged",
             "condense=matrix inertia=1 in=cbuf d=caller extra=1 launch=kernel expand=- last_vals=set",
             "condense=rhs inertia=0 in=cbuf d=d2 extra=0 launch=kernel expand=d2,null,0 last_vals=needed"]
GENERAL_DENSE = ["condense=whole inertia=1 in=cbuf d=d2 extra=1 launch=general_dense expand=d2,success,0 last_vals=unchanged",
                 "condense=matrix inertia=1 in=cbuf d=caller extra=1 launch=general_dense expand=- last_vals=set",
                 "condense=rhs inertia=0 in=cbuf d=d2 extra=0 launch=general_dense expand=d2,null,0 last_vals=needed"]

# Direct: every reachable combination of (count_d, d_outer, v2_solve, lean_rows, staged) -> its NEWTON, FACTOR and SOLVE rows
SOLVE_GENERAL_KERNEL = CONDENSED[2]
DIRECT = {
    # the kernel neither counts the condensed pivots nor writes the kept components of d
    (0, 0, 0, 0, 0): ("condense=- inertia=1 in=caller d=d2 extra=1 launch=kernel expand=d2,success,0 last_vals=unchanged",
                      "condense=- inertia=1 in=caller d=caller extra=1 launch=kernel expand=- last_vals=set",
                      SOLVE_GENERAL_KERNEL),
    (1, 0, 0, 0, 0): ("condense=- inertia=0 in=caller d=d2 extra=0 launch=kernel expand=d2,success,0 last_vals=unchanged",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=kernel expand=- last_vals=set",
                      SOLVE_GENERAL_KERNEL),
    # d_outer without count_d: plain launches, a post-pass without the reduced solution
    (0, 1, 0, 0, 0): ("condense=- inertia=1 in=caller d=caller extra=1 launch=kernel expand=null,success,0 last_vals=unchanged",
                      "condense=- inertia=1 in=caller d=caller extra=1 launch=kernel expand=- last_vals=set",
                      SOLVE_GENERAL_KERNEL),
    (0, 1, 1, 0, 0): ("condense=- inertia=1 in=caller d=caller extra=1 launch=kernel expand=null,success,0 last_vals=unchanged",
                      "condense=- inertia=1 in=caller d=caller extra=1 launch=kernel expand=- last_vals=set",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=kernel expand=null,null,0 last_vals=needed"),
    # d_outer and count_d: v2_solve, lean_rows and staged are free
    (1, 1, 0, 0, 0): ("condense=- inertia=0 in=caller d=caller extra=0 launch=kernel expand=null,success,0 last_vals=unchanged",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=kernel expand=- last_vals=set",
                      SOLVE_GENERAL_KERNEL),
    (1, 1, 1, 0, 0): ("condense=- inertia=0 in=caller d=caller extra=0 launch=kernel expand=null,success,0 last_vals=unchanged",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=kernel expand=- last_vals=set",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=kernel expand=null,null,0 last_vals=needed"),
    (1, 1, 0, 1, 0): ("condense=- inertia=0 in=caller d=caller extra=0 launch=kernel expand=- last_vals=unchanged",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=kernel expand=- last_vals=set",
                      SOLVE_GENERAL_KERNEL),
    (1, 1, 1, 1, 0): ("condense=- inertia=0 in=caller d=caller extra=0 launch=kernel expand=- last_vals=unchanged",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=kernel expand=- last_vals=set",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=kernel expand=- last_vals=needed"),
    (1, 1, 0, 0, 1): ("condense=- inertia=0 in=caller d=caller extra=0 launch=staged expand=null,success,0 last_vals=unchanged",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=staged expand=- last_vals=set",
                      SOLVE_GENERAL_KERNEL),
    (1, 1, 1, 0, 1): ("condense=- inertia=0 in=caller d=caller extra=0 launch=staged expand=null,success,0 last_vals=unchanged",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=staged expand=- last_vals=set",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=staged expand=null,null,0 last_vals=needed"),
    (1, 1, 0, 1, 1): ("condense=- inertia=0 in=caller d=caller extra=0 launch=staged expand=- last_vals=unchanged",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=staged expand=- last_vals=set",
                      SOLVE_GENERAL_KERNEL),
    (1, 1, 1, 1, 1): ("condense=- inertia=0 in=caller d=caller extra=0 launch=staged expand=- last_vals=unchanged",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=staged expand=- last_vals=set",
                      "condense=- inertia=0 in=caller d=caller extra=0 launch=staged expand=- last_vals=needed"),
}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("call_shape") / "call_shape_table")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "c_abi", "call_shape_table.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr)
    out = {}
    for line in r.stdout.splitlines():
        key, shape = line.split(": ")
        route, *flags, mode = key.split()
        out[(route, tuple(int(f.split("=")[1]) for f in flags), mode)] = shape
    assert len(out) == (5 * 2 + 32) * 3
    return out


@pytest.mark.parametrize("route,rows", [("Plain", PLAIN), ("Dense", DENSE), ("Band", BAND), ("Condensed", CONDENSED), ("GeneralDense", GENERAL_DENSE)])
def test_routes_that_read_no_flag(table, route, rows):
    """All three modes; the flags only the Direct route reads change nothing, all clear or all set."""
    for flags in ((0,) * 5, (1,) * 5):
        for mode, row in zip(MODES, rows):
            assert table[(route, flags, mode)] == row, (route, flags, mode)


def test_direct_route_every_reachable_combination(table):
    """staged => d_outer and count_d, lean_rows => d_outer and count_d, v2_solve => d_outer: twelve combinations, three modes each."""
    reachable = [(c, o, v, l, s) for c in (0, 1) for o in (0, 1) for v in (0, 1) for l in (0, 1) for s in (0, 1)
                 if (not s or (o and c)) and (not l or (o and c)) and (not v or o)]
    assert sorted(reachable) == sorted(DIRECT)
    for flags in reachable:
        for mode, row in zip(MODES, DIRECT[flags]):
            assert table[("Direct", flags, mode)] == row, (flags, mode)


def test_extra_counts_exactly_where_the_inertia_pass_runs(table):
    for key, shape in table.items():
        assert ("inertia=1" in shape) == ("extra=1" in shape), key
