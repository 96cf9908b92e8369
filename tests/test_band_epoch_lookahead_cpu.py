"""The shapes tests/test_band_epoch_lookahead_gpu.py runs, checked from the plan alone (no GPU): the mover-table instance of the band
kernel (csrc/band.hip) takes every field of an epoch block from a register it loaded two epochs earlier, so its edges are the ends
of a sweep — the fewest epochs a part can have, a last epoch of one step and of a full eight, both parities of the step count of the
epoch the backward sweep starts with, parts of different lengths — and the batches that leave a workgroup partly or wholly idle.
Each property is asserted here for the shape that is there to cover it: a change of the plan generator that moves an edge fails
this file instead of silently thinning the GPU cases."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn

EPOCH = 8       # steps of a full epoch (csrc/band.h: BAND_EPOCH)
BE_NSTEP = 38   # the field of an epoch block that holds its step count (BE_NSTEP of the 15-piece layout)
# n, p, hw, batch, ladder climbers, [(steps, epochs, steps of the last epoch) of each part]
CASES = [
    dict(n=12, p=0, hw=2, B=33, ladder=(), parts=[(16, 2, 8)]),                        # smallest n, fewest epochs, last epoch full (even)
    dict(n=13, p=1, hw=2, B=31, ladder=(3,), parts=[(17, 3, 1)]),                      # one epoch more, last epoch of one step (odd)
    dict(n=20, p=4, hw=1, B=1, ladder=(), parts=[(24, 3, 8)]),                         # hw = 1, one problem
    dict(n=21, p=3, hw=1, B=65, ladder=(2, 40, 64), parts=[(25, 4, 1)]),               # hw = 1, three workgroups, the last with one problem
    dict(n=94, p=2, hw=2, B=65, ladder=(0, 7, 31), parts=[(49, 7, 1), (49, 7, 1)]),    # two parts; climbers in the first workgroup only
    dict(n=92, p=4, hw=1, B=33, ladder=(32,), parts=[(48, 6, 8), (48, 6, 8)]),         # two parts, hw = 1; the climber is the lone problem of the second workgroup
    dict(n=92, p=0, hw=2, B=31, ladder=(30,), parts=[(48, 6, 8), (48, 6, 8)]),         # two parts, hw = 2, no border
    dict(n=95, p=5, hw=2, B=33, ladder=(1,), parts=[(42, 6, 2), (57, 8, 1)]),          # two parts of different lengths: one wavefront ends two epochs early
]
IDS = [f"n{c['n']}-p{c['p']}-hw{c['hw']}-B{c['B']}" for c in CASES]
_plans = {}


def plan_of(n, p, hw):
    if (n, p, hw) not in _plans:
        s = syn.band_structure(n, p, hw=hw)
        rows, cols = s.kkt_pattern()
        _plans[n, p, hw] = (s, hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT)))
    return _plans[n, p, hw]


def table_and_parts(n, p, hw):
    """(table accepted, [(steps, epochs, steps of the last epoch)]) of the resident program the mover-table instance runs; (False, [])
    where the pattern has no such program"""
    _, pl = plan_of(n, p, hw)
    info = pl.array("bandr_info")
    if not info[0]:
        return False, []
    parts = []
    for q in range(int(info[1])):
        nsteps, nepochs = (int(v) for v in pl.array(f"bandr_part{q}")[:2])
        nst = pl.array(f"bandr_epochs{q}").reshape(nepochs, -1)[:, BE_NSTEP]
        assert nst.sum() == nsteps and (nst[:-1] == EPOCH).all() and 1 <= nst[-1] <= EPOCH
        parts.append((nsteps, nepochs, int(nst[-1])))
    return bool(pl.array("bandm_info")[0] == 1), parts


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_shape_has_the_table_and_the_edges_it_stands_for(built, case):
    ok, parts = table_and_parts(case["n"], case["p"], case["hw"])
    assert ok and parts == case["parts"]
    for nsteps, nepochs, last in parts:
        assert nepochs == -(-nsteps // EPOCH) and last == (nsteps - 1) % EPOCH + 1
    assert all(0 <= b < case["B"] for b in case["ladder"])


def test_no_shorter_chain_and_no_part_of_fewer_epochs(built):
    """n = 12 is the shortest chain with a program, its part of two epochs the shortest part: no accepted plan has a sweep of one epoch"""
    for n in range(4, 12):
        for p in (0, 1, 2, 4):
            if p and n % p:
                continue
            for hw in (1, 2):
                assert table_and_parts(n, p, hw) == (False, []), (n, p, hw)
    assert table_and_parts(12, 0, 2) == (True, [(16, 2, 8)])


def test_the_cases_cover_every_edge():
    last = {x[2] for c in CASES for x in c["parts"]}
    epochs = {x[1] for c in CASES for x in c["parts"]}
    assert {1, EPOCH} <= last and {l % 2 for l in last} == {0, 1}            # nsteps % 8 = 1 and 0; both parities in the first backward epoch
    assert min(epochs) == 2 and 3 in epochs                                 # the fewest epochs, and one more
    for nparts in (1, 2):
        assert {c["hw"] for c in CASES if len(c["parts"]) == nparts} == {1, 2}
        assert {1, EPOCH} <= {x[2] for c in CASES if len(c["parts"]) == nparts for x in c["parts"]}
    assert {c["B"] for c in CASES} == {1, 31, 33, 65}
    assert any(len({x[1] for x in c["parts"]}) == 2 for c in CASES)           # the two wavefronts of a workgroup run different epoch counts
    # a climber in the first workgroup and none in the second, which has finished when the first re-enters the forward sweep
    assert any(c["B"] > 32 and c["ladder"] and max(c["ladder"]) < 32 for c in CASES)
    assert any(not c["ladder"] for c in CASES) and any(c["p"] == 0 for c in CASES)
