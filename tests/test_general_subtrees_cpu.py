"""The general kernel's subtree execution (tuning general_subtrees), without a GPU: the option's rules, the classic tables with the key
on, the cut, the layout of the task regions, the plan run task by task in numpy against the classic walk (bit for bit), the oracle's
decisions that vouch for the inputs of tests/test_general_subtrees_gpu.py, and the routing rule as DESIGN section 3.2 states it."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl
from tests.support import dense_general_cases as GC
from tests.support import general_subtrees_cases as GS
from tests.support.plan_sim import PlanSim, tri

CNL_ERR_ARG = 1
CLASSIC = ("fronts", "inner_perm", "perm", "seg_ptr", "asm_pos", "asm_src", "child_idx", "rel_idx")
# shape, extra options: every plan the tests below walk (the uncondensed grids have 44 and 84 fronts)
PLANS = [(sh, dict(task_cap=cap)) for sh in GS.SHAPES for cap in (4, 8)] + [(GS.GRID12, dict(task_cap=4, condense=0)), (GS.GRID16, dict(task_cap=8, condense=0)),
                                                                           (GS.GRID32, dict(task_cap=8, general_blocked=1))]


def _pid(v):
    return GS.shape_id(v) if isinstance(v, tuple) else "-".join(f"{k}{x}" for k, x in v.items())


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


# ---- 1. option rules ----
def test_option_rules(built):
    assert hipldl.lib().cnl_version() >= 506
    s = GS.structure(GS.FOREST3)
    assert _plan_rc(s, **GS.OPTS)[0] == 0
    assert _plan_rc(s, **GS.options(general_subtrees=0))[0] == 0
    assert _plan_rc(s, **GS.options(general_blocked=1))[0] == 0          # the intended pairing
    for bad in (2, -1):
        rc, msg = _plan_rc(s, **GS.options(general_subtrees=bad))
        assert rc == CNL_ERR_ARG and "general_subtrees" in msg, (rc, msg)
    assert _plan_rc(s, float32_general=1, float32_refine=1)[0] == 0
    rc, msg = _plan_rc(s, float32_general=1, float32_refine=1, general_subtrees=1)
    assert rc == CNL_ERR_ARG and "general_subtrees" in msg and "Float64" in msg, (rc, msg)


def test_float32_creators_refuse_the_key_before_they_look_for_a_device(built):
    s = GS.structure(GS.FOREST3)
    rows, cols = s.kkt_pattern()
    for dtype, opt in ((np.float32, dict(float32_general=1, general_subtrees=1)),
                       (np.float32, dict(general_subtrees=1)),
                       (np.float64, dict(float32_general=1, float32_refine=1, general_subtrees=1))):
        with pytest.raises(hipldl.CnlError) as e:
            hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=7, dtype=dtype, options=hipldl.Options(**opt))
        assert e.value.code == CNL_ERR_ARG and "general_subtrees" in str(e.value), str(e.value)


def test_plan_without_the_key_has_no_cut(built):
    s, P = GS.make_plan(GS.GRID12, general_subtrees=0)
    for name in ("gtasks", "gstage_ptr", "gfronts", "ginfo"):
        assert len(P.array(name)) == 0, name
    s, P = GS.make_plan(GS.GRID12)
    assert len(P.array("gtasks")) > 0 and len(P.array("tasks")) == 0 and len(P.array("stage_ptr")) == 0      # (the register-front kernel's stay empty)


# ---- 2. the classic tables with the key on ----
@pytest.mark.parametrize("shape,extra", PLANS, ids=_pid)
def test_classic_tables_are_those_of_the_key_off_plan(built, shape, extra):
    s, on = GS.make_plan(shape, **extra)
    s, off = GS.make_plan(shape, **dict(extra, general_subtrees=0))
    for name in CLASSIC:
        assert np.array_equal(on.array(name), off.array(name)), name
    assert on.info == off.info
    g, fr = on.array("gfronts").reshape(-1, 16), on.array("fronts").reshape(-1, 16)
    same = [i for i, k in enumerate(GS.HDR) if k not in GS.MOVED]
    assert g.shape == fr.shape and np.array_equal(g[:, same], fr[:, same])      # lptr included: the factor layout is the classic one


# ---- 3. the cut ----
@pytest.mark.parametrize("shape,extra", PLANS, ids=_pid)
def test_cut(built, shape, extra):
    s, P = GS.make_plan(shape, **extra)
    t, sp, g, gi = GS.cut_of(P)
    ns, nt, cap = len(g["npiv"]), len(t["f0"]), extra["task_cap"]
    assert gi[1] == nt and gi[2] == len(sp) - 1 and gi[3] == sp[1] and gi[4] == cap
    # every front in exactly one task
    owner = np.full(ns, -1)
    for k in range(nt):
        assert t["f0"][k] < t["f1"][k] and (owner[t["f0"][k]:t["f1"][k]] == -1).all()
        owner[t["f0"][k]:t["f1"][k]] = k
    assert (owner >= 0).all()
    parent = g["parent"]
    kids = [[] for _ in range(ns)]
    for f in range(ns):
        if parent[f] >= 0:
            kids[parent[f]].append(f)
    nsub = np.ones(ns, np.int64)
    for f in range(ns):     # post-order: children first
        assert parent[f] < 0 or parent[f] > f
        if parent[f] >= 0:
            nsub[parent[f]] += nsub[f]
    for k in range(nt):
        f0, f1 = t["f0"][k], t["f1"][k]
        root = f1 - 1
        if f1 - f0 > 1 or nsub[root] == 1:
            # a bottom subtree: a contiguous post-order range closed under descendants, of at most cap fronts, maximal
            assert nsub[root] == f1 - f0 <= cap and t["stage"][k] == 0
            assert all(f0 <= c < f1 for f in range(f0, f1) for c in kids[f])
            assert all(f0 <= parent[f] < f1 for f in range(f0, root))
            assert parent[root] < 0 or nsub[parent[root]] > cap
        else:
            assert nsub[root] > cap       # a single front above the cut
        child_tasks = {int(owner[c]) for c in kids[root]} - {k} if f1 - f0 == 1 else set()
        assert t["stage"][k] == (1 + max(t["stage"][c] for c in child_tasks) if child_tasks else 0)
        assert t["parent"][k] == (owner[parent[root]] if parent[root] >= 0 else -1)
    # stage pointers
    assert sp[0] == 0 and sp[-1] == nt and (np.diff(sp) > 0).all() and (np.diff(t["stage"]) >= 0).all()
    for st in range(len(sp) - 1):
        assert (t["stage"][sp[st]:sp[st + 1]] == st).all()
    if cap == 8 and shape in GS.CUT_CAP8 and "condense" not in extra:
        assert (nt, len(sp) - 1) == GS.CUT_CAP8[shape]
    if shape == GS.FOREST4:
        assert (parent < 0).sum() == 4
    if shape == GS.FOREST3:
        assert (parent < 0).sum() == 3
    print(f"{GS.shape_id(shape)} cap {cap}: {ns} fronts, {nt} tasks in {len(sp) - 1} stages, first stage {sp[1]}, gwork {gi[0]}")


# ---- 4. the layout ----
@pytest.mark.parametrize("shape,extra", PLANS, ids=_pid)
def test_layout(built, shape, extra):
    s, P = GS.make_plan(shape, **extra)
    t, sp, g, gi = GS.cut_of(P)
    rows = 16 if extra.get("general_blocked") else 2
    gwork, nt = int(gi[0]), len(t["f0"])
    assert P.info["fwd_peak"] > 0 and gwork < 2 ** 30
    child_idx = P.array("child_idx").astype(np.int64)
    end = t["wv_off"] + rows * t["fmax"]
    # regions pairwise disjoint and inside gwork (they are laid side by side in task order)
    assert t["base"][0] == 0 and (t["base"][1:] >= end[:-1]).all() and end[-1] <= gwork and (t["base"] < end).all()
    for k in range(nt):
        base, pb, wv = t["base"][k], t["pb_off"][k], t["wv_off"][k]
        fr = range(t["f0"][k], t["f1"][k])
        fs = np.array([1 + g["nupd"][f] + g["npiv"][f] for f in fr])
        panel = max(tri(1 + g["nupd"][f] + g["npiv"][f]) - tri(1 + g["nupd"][f]) for f in fr)
        assert base <= pb <= wv and pb + panel <= wv              # the panel buffer: behind the stack, in front of the staging rows
        assert t["fmax"][k] >= fs.max() and wv + rows * t["fmax"][k] <= end[k]
        for f in fr:
            f_ = 1 + g["nupd"][f] + g["npiv"][f]
            # PlanSim.check_layout's conditions, relative to the region: children of the task below the front, the stack inside [base, pb)
            for c in child_idx[g["child_begin"][f]:g["child_end"][f]]:
                if t["f0"][k] <= c < t["f1"][k]:
                    assert g["ubase"][c] + tri(1 + g["nupd"][c]) <= g["foff"][f], "child update overlaps the front"
            assert base <= g["ubase"][f] <= g["foff"][f]
            assert g["foff"][f] + tri(f_) <= pb
            # what another task reads later lies in the owner's region: the update matrix of the task's root, every solution vector
            assert g["ubase"][f] + tri(1 + g["nupd"][f]) <= pb
            assert base <= g["xoff"][f] and g["xoff"][f] + f_ <= pb


# ---- 5. execution, task by task ----
EXEC = [(GS.GRID12, dict(task_cap=4)), (GS.GRID12, dict(task_cap=4, condense=0)), (GS.GRID16, dict(task_cap=8)), (GS.FOREST4, dict(task_cap=4)), (GS.FOREST3, dict(task_cap=8))]


@pytest.mark.parametrize("shape,extra", EXEC, ids=_pid)
def test_task_by_task_is_the_classic_walk_bit_for_bit(built, shape, extra):
    """The mix through SubtreeSim — gfronts task by task, the tasks of a stage forwards and reversed, every region NaN until its
    task has run, writes outside the running task's region refused — against PlanSim on the classic table: the factor of the first
    attempt, its pivot counts, and d, ok, rho, rho_old, nfact of the whole newton_system, bit for bit in numpy."""
    s, P = GS.make_plan(shape, **extra)
    vals, rhs, ro = GC.values(s, GC.MIX)
    p = hipldl.default_params()
    classic = PlanSim(P)
    classic.check_layout()
    sims = [GS.SubtreeSim(P, reverse=False), GS.SubtreeSim(P, reverse=True)]
    assert sims[0].ntasks >= 2
    oks = []
    for b in range(GC.MIX):
        if classic.ncond:
            cb = classic.condense(vals[b], rhs[b])
            nmat = len(cb) - classic.N
            v, r = cb[:nmat].copy(), cb[nmat:]
        else:
            v, r = vals[b], rhs[b]
        L0, np0, nz0 = classic.factor(v, r, s.nvar, p[0])
        want = classic.newton_system(vals[b].copy(), rhs[b], s.nvar, s.nequ, s.ncon, ro[b], p)
        oks.append((bool(want[1]), int(want[4])))
        for sim in sims:
            sim.check_writes = True
            L1, np1, nz1 = sim.factor(v, r, s.nvar, p[0])
            assert sorted(sim.trace) == list(range(sim.ntasks))
            assert (np1, nz1) == (np0, nz0), (b, sim.reverse)
            assert np.array_equal(GC.bits64(L1), GC.bits64(L0)), (b, sim.reverse)
            sim.check_writes = False       # (the ladder's factorisations: the same walk at other values)
            got = sim.newton_system(vals[b].copy(), rhs[b], s.nvar, s.nequ, s.ncon, ro[b], p)
            assert (bool(got[1]), int(got[4])) == (bool(want[1]), int(want[4])), (b, got[1:], want[1:])
            assert np.array_equal(GC.bits64(got[0]), GC.bits64(want[0])), (b, sim.reverse)
            assert np.array_equal(GC.bits64([got[2], got[3]]), GC.bits64([want[2], want[3]]))
    assert sims[0].trace != sims[1].trace
    # never below one first-attempt success, one climber and one failure
    assert (True, 1) in oks and any(ok and nf > 1 for ok, nf in oks) and any(not ok for ok, nf in oks), oks
    print(f"{GS.shape_id(shape)} {extra}: {sims[0].ntasks} tasks, (ok, nfact) {oks}")


# ---- 6. decisions ----
# what the oracle makes of the mix per shape: kind 5 (one positive residual pivot) succeeds at once on grid_structure(12) and (32) and
# fails on the others; first-attempt successes, climbers (nfact 6 and 4) and failures (nfact 20) on every shape
WANT = {GS.GRID12: ([1, 0, 1, 1, 1, 1, 0], [1, 20, 6, 4, 1, 1, 20]), GS.GRID32: ([1, 0, 1, 1, 1, 1, 0], [1, 20, 6, 4, 1, 1, 20]),
        GS.GRID16: ([1, 0, 1, 1, 1, 0, 0], [1, 20, 6, 4, 1, 20, 20]), GS.FOREST4: ([1, 0, 1, 1, 1, 0, 0], [1, 20, 6, 4, 1, 20, 20]),
        GS.FOREST3: ([1, 0, 1, 1, 1, 0, 0], [1, 20, 6, 4, 1, 20, 20])}
DECISIONS = [(sh, {}) for sh in GS.SHAPES] + [(GS.GRID12, dict(condense=0)), (GS.GRID16, dict(condense=0))]


@pytest.mark.parametrize("shape,extra", DECISIONS, ids=_pid)
def test_decisions_on_both_orders(oracle_mod, shape, extra):
    """The oracle decides the mix the same way on the canonical order and on the plan's own, as WANT says, and the eigenvalues of
    the condensed matrix vouch for every rung of kinds 5 and 6 (dense_general_cases.rung_verdicts)."""
    c = GS.case(shape)
    s, P = GS.make_plan(shape, **extra)
    own = GC.oracle_on(P.array("perm").astype(np.int64), c)
    want_ok, want_nf = WANT[shape]
    for ref in (c, own):
        assert ref["ok"].astype(int).tolist() == want_ok and ref["nf"].tolist() == want_nf, (ref["ok"], ref["nf"])
        assert np.array_equal(GC.bits64(ref["rho"]), GC.bits64(c["rho"])) and np.array_equal(GC.bits64(ref["ro"]), GC.bits64(c["ro"]))
    if not extra and shape != GS.GRID32:        # (order-independent: once per shape; grid_structure(32) is test_general_blocked_cpu's)
        for k in (5, 6):
            for rho, determined, rel, how in GC.rung_verdicts(c, k):
                assert determined, (k, rho, rel, how)


# ---- 7. the routing rule ----
def test_routing_rule_on_the_host(built):
    """one problem per workgroup of 256 or 1024 threads, two tasks or more in the first stage, and
    batch x gwork x 8 <= 8e9 bytes.  Every shape of the tests takes the route at 256 threads with caps 4 and 8; 64 threads, several
    problems per workgroup and a single-task cut do not; the chain-like tree has 18 bottom subtrees and takes it by this rule."""
    for shape in GS.SHAPES:
        for cap in (4, 8):
            s, P = GS.make_plan(shape, task_cap=cap)
            assert GS.takes_the_route(P, GC.MIX, 256) and GS.takes_the_route(P, 65, 1024), (shape, cap)
            assert not GS.takes_the_route(P, GC.MIX, 64) and not GS.takes_the_route(P, GC.MIX, 256, ppb=4)
    s, P = GS.make_plan(GS.GRID12, task_cap=1000)
    assert P.array("ginfo")[1:4].tolist() == [1, 1, 1] and not GS.takes_the_route(P, GC.MIX, 256)
    s, P = GS.make_plan(GS.CHAIN)
    gi = P.array("ginfo")
    assert gi[3] == 18 and GS.takes_the_route(P, GC.MIX, 256), gi
    # the memory rule on either side of the bound
    s, P = GS.make_plan(GS.GRID12, task_cap=8)
    gwork = int(P.array("ginfo")[0])
    edge = int(GS.MEMORY_BOUND // (8 * gwork))
    assert edge * gwork * 8 <= GS.MEMORY_BOUND < (edge + 1) * gwork * 8 and edge < (1 << 24)
    assert GS.takes_the_route(P, edge, 256) and not GS.takes_the_route(P, edge + 1, 256)
