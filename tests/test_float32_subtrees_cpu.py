"""The general kernel's subtree execution in float (tuning float32_subtrees), without a GPU: the key's rules, what vouches for the
inputs of tests/test_float32_subtrees_gpu.py (the oracle's pattern and the Float32 margin of every rung), the cut of the forced float
plans, their classic tables against the key-off plan, the plan run task by task in numpy.float32 against the classic walk, and the
routing rule as DESIGN section 9.11 states it."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl
from tests.support import dense_cases as dc
from tests.support import f32_subtrees_cases as FS

CNL_ERR_ARG = 1
CLASSIC = ("fronts", "inner_perm", "perm", "seg_ptr", "asm_pos", "asm_src", "child_idx", "rel_idx")
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def oracle_mod(built):
    from oracle import oracle as O
    O.build()
    return O


def _plan_rc(s, **opt):
    rows, cols = s.kkt_pattern()
    try:
        hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=7, options=hipldl.Options(**opt))
    except hipldl.CnlError as e:
        return e.code, str(e)
    return 0, ""


def _create_rc(s, dtype, **opt):
    """(code, message) of the creator for `dtype`; (0, "") where the handle was made (a machine with a device)"""
    rows, cols = s.kkt_pattern()
    try:
        hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=7, dtype=dtype, options=hipldl.Options(**opt)).close()
    except hipldl.CnlError as e:
        return e.code, str(e)
    return 0, ""


# ---- 1. the key's rules, decided before a device is looked for ----
def test_key_rules_without_a_device(built):
    s = FS.structure(FS.FOREST3)
    # accepted with float32_general, alone and with float32_blocked (the intended pairing), float32_condense and task_cap: the creator
    # gets past the option checks (with no device it then says so)
    for extra in ({}, dict(float32_blocked=1), dict(float32_condense=1, task_cap=4), dict(float32_subtrees=0), dict(float32_register_front=1)):
        rc, msg = _create_rc(s, f32, **dict(dict(float32_general=1, float32_subtrees=1), **extra))
        assert rc != CNL_ERR_ARG and "float32_subtrees" not in msg, (rc, msg)
        assert rc == 0 or "no HIP device" in msg, (rc, msg)
    # refused alone
    rc, msg = _create_rc(s, f32, float32_subtrees=1)
    assert rc == CNL_ERR_ARG and "float32_subtrees" in msg and "float32_general" in msg, (rc, msg)
    # refused at another value
    for bad in (2, -1):
        rc, msg = _create_rc(s, f32, float32_general=1, float32_subtrees=bad)
        assert rc == CNL_ERR_ARG and "float32_subtrees" in msg, (rc, msg)
    # refused with float32_refine, at plan and at handle creation; both are made without the key
    assert _plan_rc(s, float32_general=1, float32_refine=1)[0] == 0
    for rc, msg in (_plan_rc(s, float32_general=1, float32_refine=1, float32_subtrees=1),
                    _create_rc(s, f64, float32_general=1, float32_refine=1, float32_subtrees=1)):
        assert rc == CNL_ERR_ARG and "float32_subtrees" in msg and "float32_refine" in msg, (rc, msg)
    assert hipldl.lib().cnl_version() >= 507


def test_general_subtrees_is_still_refused_at_the_float32_creators(built):
    s = FS.structure(FS.FOREST3)
    for dtype, opt, word in ((f32, dict(float32_general=1, general_subtrees=1), "general_subtrees"),
                             (f32, dict(float32_general=1, general_subtrees=1, float32_subtrees=1), "general_subtrees"),
                             (f32, dict(float32_general=1, general_blocked=1, float32_subtrees=1), "general_blocked"),
                             (f64, dict(float32_general=1, float32_refine=1, general_subtrees=1), "general_subtrees")):
        rc, msg = _create_rc(s, dtype, **opt)
        assert rc == CNL_ERR_ARG and word in msg and "Float64 handles only" in msg, (rc, msg)
    rc, msg = _create_rc(s, f32, float32_general=1, general_subtrees=1)
    assert "the general kernel has no Float32 subtree instances" in msg, msg      # word for word


def test_a_float64_creator_reads_nothing_of_the_key(built):
    """neither rule nor value, as of float32_condense: the plan is the plan without the key, table for table"""
    s = FS.structure(FS.FOREST3)
    rows, cols = s.kkt_pattern()
    base = hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=7, options=hipldl.Options())
    for opt in (dict(float32_subtrees=1), dict(float32_subtrees=2), dict(float32_subtrees=1, float32_blocked=1)):
        assert _plan_rc(s, **opt)[0] == 0
        rc, msg = _create_rc(s, f64, **opt)
        assert rc != CNL_ERR_ARG and (rc == 0 or "no HIP device" in msg), (rc, msg)
        P = hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=7, options=hipldl.Options(**opt))
        assert P.info == base.info and len(P.array("gtasks")) == 0
        for name in CLASSIC:
            assert np.array_equal(P.array(name), base.array(name)), name


# ---- 2. what vouches for the inputs ----
MARGIN_CASES = [(sh, FS.MIX) for sh in FS.SHAPES] + [(FS.GRID12, 65)]


@pytest.mark.parametrize("shape,B", MARGIN_CASES, ids=[f"{FS.shape_id(sh)}-B{B}" for sh, B in MARGIN_CASES])
def test_pivot_margins(oracle_mod, shape, B):
    """Every decision of every rung of every problem the GPU tests run: the Schur complement onto the variables has its smallest
    eigenvalue at least MARGIN of the largest away from zero, with the sign the decision needs; the oracle's pattern is the mix's."""
    c = FS.case(shape, B)
    assert list(c["ok"]) == [FS.WANT_OK[b % 5] for b in range(B)], c["ok"]
    assert [int(x) for x in c["nf"]] == [FS.WANT_NF[b % 5] for b in range(B)]
    p = c["p32"].astype(np.float64)
    worst = np.inf
    for b in range(B):
        if b % 5 == 1:
            assert np.isnan(c["vals"][b]).any()
            continue
        assert c["rho"][b] == dc.rungs(float(c["rho_old"][b]), int(c["nf"][b]), p)[-1]
        for rho, rel, succeeds in FS.eig_margins(c, b):
            assert (rel >= FS.MARGIN) if succeeds else (rel <= -FS.MARGIN), (b, rho, rel, succeeds)
            worst = min(worst, abs(rel))
    print(f"{FS.shape_id(shape)} x {B}: smallest |lambda_min| / lambda_max over all rungs {worst:.3g}")
    assert worst >= FS.MARGIN


# ---- 3. the cut of the forced float plans, and their classic tables ----
CUTS = sorted(FS.CUT, key=str)


def _cid(v):
    shape, cond, cap = v
    return f"{FS.shape_id(shape)}-{'condensed' if cond else 'uncondensed'}-cap{cap}"


@pytest.mark.parametrize("key", CUTS, ids=[_cid(v) for v in CUTS])
def test_cut_of_the_forced_float_plan(built, key):
    shape, cond, cap = key
    for blocked in (0, 1):
        s, P = FS.make_plan(shape, cond, cap, blocked)
        gwork, ntasks, nstages, first, gcap = FS.ginfo(P)
        assert (ntasks, nstages, first) == FS.CUT[key] and gcap == cap
        assert P.info["fmax"] == FS.FMAX[shape][0 if cond else 1] and (P.info["ncond"] > 0) == cond
        t = P.array("gtasks").reshape(-1, 8).astype(np.int64)
        rows = 16 if blocked else 2
        end = t[:, 6] + rows * t[:, 7]      # wv_off + rows x fmax: the regions lie side by side and fill gwork
        assert t[0, 4] == 0 and np.array_equal(t[1:, 4], end[:-1]) and end[-1] == gwork and gwork % 2 == 0 and (t[:, 4] % 2 == 0).all()
        print(f"{_cid(key)} blocked {blocked}: gwork {gwork} elements = {gwork * FS.ESZ} bytes per problem")


CLASSIC_CASES = [(FS.GRID12, True, 4), (FS.GRID12, False, 8), (FS.GRID16, True, 8), (FS.FOREST3, False, 4), (FS.FOREST4, True, 4), (FS.GRID32, False, 8)]


@pytest.mark.parametrize("key", CLASSIC_CASES, ids=[_cid(v) for v in CLASSIC_CASES])
def test_classic_tables_are_those_of_the_key_off_plan(built, key):
    shape, cond, cap = key
    s, off = FS.make_plan(shape, cond, cap, subtrees=0)
    assert len(off.array("gtasks")) == 0
    for blocked in (0, 1):
        s, on = FS.make_plan(shape, cond, cap, blocked)
        for name in CLASSIC:
            assert np.array_equal(on.array(name), off.array(name)), name
        assert on.info == off.info
        g, fr = on.array("gfronts").reshape(-1, 16), on.array("fronts").reshape(-1, 16)
        same = [i for i, k in enumerate(FS.GS.HDR) if k not in FS.GS.MOVED]
        assert g.shape == fr.shape and np.array_equal(g[:, same], fr[:, same])


# ---- 4. execution in numpy.float32, task by task ----
EXEC = [(FS.GRID12, True, 4), (FS.GRID12, False, 4), (FS.GRID16, True, 8), (FS.FOREST4, True, 4), (FS.FOREST3, True, 4)]


@pytest.mark.parametrize("key", EXEC, ids=[_cid(v) for v in EXEC])
def test_task_by_task_in_float32_decides_as_the_classic_walk(built, key):
    """The mix through SubtreeSimF32 — gfronts task by task in numpy.float32, staging rows 2 and 16, the tasks of a stage forwards and
    reversed, every region NaN until its task has run, writes outside the running task's region refused — against PlanSim in float32
    on the classic table: ok, nfact, rho, rho_old equal (and the mix's pattern).  d is printed against the classic walk's: the
    per-front arithmetic is the same, so bit-equal is the expectation."""
    shape, cond, cap = key
    c_p32 = hipldl.default_params(np.float32)
    s = FS.structure(shape)
    vals, rhs, ro = FS.GD.values(s, FS.MIX)
    s, P2 = FS.make_plan(shape, cond, cap, 0)
    classic = FS.classic_sim(P2)
    classic.check_layout()
    want = [classic.newton_system(vals[b].copy(), rhs[b], s.nvar, s.nequ, s.ncon, ro[b], c_p32) for b in range(FS.MIX)]
    assert [(bool(w[1]), int(w[4])) for w in want] == list(zip(FS.WANT_OK, FS.WANT_NF)), [(w[1], w[4]) for w in want]
    for rows in (2, 16):
        s, P = FS.make_plan(shape, cond, cap, blocked=rows == 16)
        sims = [FS.SubtreeSimF32(P, reverse=False, rows=rows), FS.SubtreeSimF32(P, reverse=True, rows=rows)]
        assert sims[0].ntasks == FS.CUT[key][0] >= 2
        bit_equal = True
        for b in range(FS.MIX):
            for sim in sims:
                sim.check_writes = b == 0      # (the first attempt of the healthy problem; the other walks are the same walk at other values)
                got = sim.newton_system(vals[b].copy(), rhs[b], s.nvar, s.nequ, s.ncon, ro[b], c_p32)
                assert sorted(sim.trace) == list(range(sim.ntasks))
                assert (bool(got[1]), int(got[4])) == (bool(want[b][1]), int(want[b][4])), (rows, b, sim.reverse, got[1:], want[b][1:])
                assert np.array_equal(FS.bits([got[2], got[3]]), FS.bits([want[b][2], want[b][3]])), (rows, b)
                if got[1]:
                    assert got[0].dtype == np.float32 and np.isfinite(got[0]).all()
                    bit_equal &= bool(np.array_equal(FS.bits(got[0]), FS.bits(want[b][0])))
        assert sims[0].trace != sims[1].trace
        print(f"{_cid(key)} rows {rows}: {sims[0].ntasks} tasks, d bit-equal to the classic float32 walk: {bit_equal}")


# ---- 5. the routing rule ----
def test_routing_rule_on_the_host(built):
    """(a) the launch is the general kernel in float, (b) one problem per workgroup of 256 threads — there is no
    1 024-thread float instance —, (c) two tasks or more in the first stage, (d) batch x gwork x 4 <= 8e9 bytes."""
    for shape, cond, cap in CUTS:
        s, P = FS.make_plan(shape, cond, cap, 1)
        assert FS.takes_the_route(P, FS.MIX, 256) and FS.takes_the_route(P, 65, 256), (shape, cond, cap)
        assert not FS.takes_the_route(P, FS.MIX, 64) and not FS.takes_the_route(P, FS.MIX, 1024) and not FS.takes_the_route(P, FS.MIX, 256, ppb=4)
        assert not FS.takes_the_route(P, FS.MIX, 256, general_kernel=False)      # band, register-front, staged, dense routes
    s, P = FS.make_plan(FS.GRID12, True, 1000)
    assert FS.ginfo(P)[1:4] == [1, 1, 1] and not FS.takes_the_route(P, FS.MIX, 256)
    s, P = FS.make_plan(FS.GRID12, True, 8, subtrees=0)
    assert not FS.takes_the_route(P, FS.MIX, 256)
    # the memory rule on either side of the bound, in 4-byte elements: twice the problems of a Float64 handle on the same cut
    s, P = FS.make_plan(FS.GRID12, True, 8)
    gwork = FS.ginfo(P)[0]
    edge = int(FS.MEMORY_BOUND // (FS.ESZ * gwork))
    assert edge * gwork * FS.ESZ <= FS.MEMORY_BOUND < (edge + 1) * gwork * FS.ESZ and edge < (1 << 24)
    assert FS.takes_the_route(P, edge, 256) and not FS.takes_the_route(P, edge + 1, 256)
    assert edge // 2 == int(FS.MEMORY_BOUND // (8 * gwork))
