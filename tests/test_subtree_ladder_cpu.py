"""The staged rho ladder of subtree handles (tuning subtree_ladder = R), without a GPU: the key's rules, the staged
sequence restated in numpy (tests/support/subtree_ladder_cases.py: SubtreeLadderSim) against the sequential walk over the classic table
for every R that sits on an edge, the two further rhomax parameter sets, the ends the case set reaches — asserted from the oracle's
results —, the branch the mix does not reach pinned with hand-made inertia sequences, and the launch-count formula."""
import itertools

import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl
from tests.support import subtree_ladder_cases as SL

GS, FS, GC = SL.GS, SL.FS, SL.GC
CNL_ERR_ARG = 1
f32, f64 = np.float32, np.float64
CLASSIC = ("fronts", "inner_perm", "perm", "seg_ptr", "asm_pos", "asm_src", "child_idx", "rel_idx", "gtasks", "gstage_ptr", "gfronts", "ginfo")


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
    s = GS.structure(GS.FOREST3)
    assert hipldl.lib().cnl_version() >= 508
    for R in (0, 1, 64):
        # accepted with either subtree key, at the creator of its element type and at cnl_plan_create_ex
        for dtype, opt in ((f64, dict(general_subtrees=1)), (f32, dict(float32_general=1, float32_subtrees=1)),
                           (f32, dict(float32_general=1, float32_subtrees=1, float32_blocked=1, float32_condense=1))):
            rc, msg = _create_rc(s, dtype, **dict(opt, subtree_ladder=R))
            assert rc != CNL_ERR_ARG and "subtree_ladder" not in msg, (R, rc, msg)
            assert rc == 0 or "no HIP device" in msg, (rc, msg)
            assert _plan_rc(s, **dict(opt, subtree_ladder=R))[0] == 0
    # out of range
    for bad in (-1, 65):
        for rc, msg in (_create_rc(s, f64, general_subtrees=1, subtree_ladder=bad), _plan_rc(s, general_subtrees=1, subtree_ladder=bad),
                        _create_rc(s, f32, float32_general=1, float32_subtrees=1, subtree_ladder=bad)):
            assert rc == CNL_ERR_ARG and "subtree_ladder" in msg, (bad, rc, msg)
    # alone, and with the subtree key written out as 0
    for rc, msg in (_create_rc(s, f64, subtree_ladder=3), _plan_rc(s, subtree_ladder=3), _create_rc(s, f32, float32_general=1, subtree_ladder=3),
                    _create_rc(s, f64, general_subtrees=0, subtree_ladder=3), _create_rc(s, f32, float32_general=1, float32_subtrees=0, subtree_ladder=3)):
        assert rc == CNL_ERR_ARG and "subtree_ladder" in msg, (rc, msg)
    # at a creator whose own subtree key is off: the other element type's key does not count
    rc, msg = _create_rc(s, f64, float32_general=1, float32_subtrees=1, subtree_ladder=3)
    assert rc == CNL_ERR_ARG and "subtree_ladder" in msg and "general_subtrees" in msg, (rc, msg)
    # general_subtrees stays refused at a Float32 creator, with the ladder as without it
    for opt in (dict(general_subtrees=1), dict(general_subtrees=1, float32_subtrees=1)):
        rc, msg = _create_rc(s, f32, **dict(opt, float32_general=1, subtree_ladder=3))
        assert rc == CNL_ERR_ARG, (rc, msg)
    # float32_refine stays refused, at plan and at handle creation
    for opt in (dict(float32_subtrees=1), dict(general_subtrees=1), dict(float32_subtrees=1, general_subtrees=1)):
        for rc, msg in (_plan_rc(s, **dict(opt, float32_general=1, float32_refine=1, subtree_ladder=3)),
                        _create_rc(s, f64, **dict(opt, float32_general=1, float32_refine=1, subtree_ladder=3))):
            assert rc == CNL_ERR_ARG, (opt, rc, msg)


@pytest.mark.parametrize("shape,opt", [(GS.GRID12, dict(task_cap=4)), (GS.GRID12, dict(task_cap=8, condense=0, general_blocked=1)), (GS.FOREST3, {})],
                         ids=("grid12-cap4", "grid12-uncondensed-blocked", "forest3"))
def test_the_key_changes_no_plan(built, shape, opt):
    """array for array the plan without it, the cut and the task regions included"""
    s, off = GS.make_plan(shape, **opt)
    for R in (1, 64):
        s, on = GS.make_plan(shape, **dict(opt, subtree_ladder=R))
        assert on.info == off.info
        for name in CLASSIC:
            assert np.array_equal(on.array(name), off.array(name)), name
    assert len(off.array("gtasks")) > 0


# ---- 2. the launch-count formula ----
def test_launch_count_formula():
    for S in (1, 3, 8):
        assert SL.launches(0, S) == 2 * S + 2
        for R in (1, 3, 64):
            # first attempt S + 1, R rungs of S + 1, backward S, commit, climbers
            assert SL.launches(R, S) == (S + 1) + R * (S + 1) + S + 1 + 1 == (R + 2) * S + R + 3
        assert SL.launches(5, S, "try_to_factorize") == S + 1 and SL.launches(5, S, "solve_ldl") == 2 * S


# ---- 3. the staged state machine against the reference's loop, on hand-made inertia sequences ----
P64 = hipldl.default_params()
P32 = hipldl.default_params(np.float32)


@pytest.mark.parametrize("T,p0", [(f64, P64), (f32, P32)], ids=("double", "float"))
def test_staged_ladder_on_every_inertia_sequence(T, p0):
    """Every problem that first succeeds at attempt a = 0 .. 22 or never, from rho_old = 0 and rho_old = 2, under the three parameter sets,
    at every R of the sweep and at 64: the staged sequence gives the reference loop's (ok, rho, rho_old, nfact, last rho tried) bit for
    bit, tries the same rhos in the same order, and never tries one twice."""
    for name, ro, R in itertools.product(SL.PARAM_SETS, (0.0, 2.0), (1, 2, 3, 4, 5, 9, 19, 24, 64)):
        p = np.asarray(SL.PARAM_SETS[name](np.asarray(p0, T)), T)
        for first_ok in list(range(23)) + [None]:
            seen = []

            def verdict(a, rho):
                seen.append((a, rho))
                return first_ok is not None and a >= first_ok
            want = SL.reference_ladder(verdict, ro, p, T)
            ref_seen, seen = seen, []
            got, tried = SL.staged_ladder(verdict, ro, p, R, T)
            assert got[0] == want[0] and got[3] == want[3], (name, ro, R, first_ok, got, want)
            for g, w in zip(got[1:3] + got[4:], want[1:3] + want[4:]):
                assert (g is None and w is None) or SL.bits(np.array([g], T))[0] == SL.bits(np.array([w], T))[0], (name, ro, R, first_ok, got, want)
            assert [a for a, _ in seen] == list(range(want[3])) and len(seen) == len(ref_seen)
            assert all(a == b or SL.bits(np.array([a[1]], T))[0] == SL.bits(np.array([b[1]], T))[0] for a, b in zip(seen[1:], ref_seen[1:]))
            where = [w for _, _, w in tried]
            assert where == ["first"] + ["rung"] * min(R, want[3] - 1) + ["climbers"] * max(0, want[3] - 1 - R)


def test_success_at_rho_1_above_rhomax_keeps_rho_old():
    """The branch the mixes do not reach (under `below` every problem that fails the first attempt fails at rho_1 too: kinds 2 and 3 need
    the sixth and the fourth rho of their ladders): a success at rho_1 > rhomax records rho = rho_1 and leaves rho_old as it came, in the
    reference's loop and in the rung decide alike."""
    for T, p0 in ((f64, P64), (f32, P32)):
        p = np.asarray(SL.params_below(np.asarray(p0, T)), T)
        for ro in (0.0, 2.0):
            verdict = lambda a, rho: a >= 1
            want = SL.reference_ladder(verdict, ro, p, T)
            got, tried = SL.staged_ladder(verdict, ro, p, 3, T)
            assert want[0] and want[3] == 2 and want[1] > p[6] and want[2] == T(ro) and want[4] == want[1]
            assert got == want and [w for _, _, w in tried] == ["first", "rung"]


# ---- 4. the staged sequence on the mix against the sequential walk over the classic table ----
def _classic(plan, T):
    from tests.support.plan_sim import PlanSim
    return PlanSim(plan) if T is f64 else FS.classic_sim(plan)


_refs = {}


def _reference(tag, plan, c, p, T):
    """the sequential walk over the classic table, once per (plan, parameter set)"""
    if tag not in _refs:
        s = c["s"]
        _refs[tag] = SL.classic_reference(_classic(plan, T), c["vals"], c["rhs"], s.nvar, s.nequ, s.ncon, c["rho_old"], p, T)
    return _refs[tag]


def _sweep(tag, plan, c, p, T, Rs, rows, want_nf):
    s = c["s"]
    want = _reference(tag, plan, c, p, T)
    assert want["nf"].tolist() == list(want_nf), (tag, want["nf"])
    S = len(plan.array("gstage_ptr")) - 1
    cls = SL.SubtreeLadderSim if T is f64 else SL.SubtreeLadderSimF32
    for reverse in (False, True):
        sim = cls(plan, reverse=reverse, rows=rows, check_writes=False)
        memo = {}
        for R in Rs:
            vals = np.array(c["vals"], T)
            got = sim.call(vals, c["rhs"], s.nvar, c["rho_old"], p, R, memo=memo)
            SL.assert_same_outputs(got, want, (tag, reverse, R))
            # the rho slots of vals: the last rho tried where the first attempt failed, untouched elsewhere
            for b in range(len(vals)):
                tail = vals[b, -s.nvar:]
                if want["nf"][b] > 1:
                    assert (SL.bits(tail) == SL.bits(want["slots"][b:b + 1])[0]).all(), (tag, R, b)
                else:
                    assert np.array_equal(SL.bits(tail), SL.bits(np.asarray(c["vals"][b, -s.nvar:], T))), (tag, R, b)
            assert len(sim.passes) == SL.launches(R, S), (tag, R, len(sim.passes))
            kinds = [k for k, _, _ in sim.passes]
            if R:
                assert kinds == (["forward"] * S + ["decide"]) * (R + 1) + ["backward"] * S + ["commit", "climbers"]
                # a rung works on the problems still climbing and on nobody else; rungs beyond every ladder are empty launches
                for kind, k, who in sim.passes:
                    if kind in ("forward", "decide") and k >= 1:
                        assert who == [b for b in range(len(vals)) if want["nf"][b] > k], (tag, R, k, who)
                climbers = sim.passes[-1][2]
                assert climbers == [b for b in range(len(vals)) if want["nf"][b] > R + 1], (tag, R, climbers)
                assert sim.passes[-2][2] == [b for b in range(len(vals)) if 1 < want["nf"][b] <= R + 1]
            else:
                assert kinds == ["forward"] * S + ["decide"] + ["backward"] * S + ["climbers"]


DOUBLE_PLANS = [("grid12-cap4", GS.GRID12, dict(task_cap=4), 2), ("grid12-cap8-uncondensed", GS.GRID12, dict(task_cap=8, condense=0), 2),
                ("forest3", GS.FOREST3, dict(task_cap=4), 2)]


@pytest.mark.parametrize("name,shape,opt,rows", DOUBLE_PLANS, ids=[v[0] for v in DOUBLE_PLANS])
def test_sweep_of_R_in_double(oracle_mod, name, shape, opt, rows):
    """R = 0 the parent's sequence; 2: nobody finishes inside the rungs, all resume; 3: the nfact-4 climber finishes on the last rung;
    4: the nfact-6 climber resumes and succeeds on its first resumed attempt; 5: it finishes on the last rung and the failures resume;
    19: the failures' last attempt is rung 19, whose decide finds rho_20 > rhomax and leaves nothing for the climbers; 24: five idle rungs."""
    c = GS.case(shape)
    s, plan = GS.make_plan(shape, **opt)
    # (grid_structure(12) has the mix's pattern; on the forest kind 5 — one positive residual pivot — fails like kind 6, as the oracle says)
    assert c["nf"].tolist() == (GC.WANT_NF if shape == GS.GRID12 else [1, 20, 6, 4, 1, 20, 20])
    _sweep(("double", name, "default"), plan, c, c["params"], f64, SL.R_SWEEP, rows, c["nf"].tolist())
    want = _refs["double", name, "default"]
    assert np.array_equal(want["ok"], c["ok"]) and np.array_equal(want["nf"], c["nf"])      # (the oracle's decisions)
    assert np.array_equal(SL.bits(want["rho"]), SL.bits(c["rho"])) and np.array_equal(SL.bits(want["ro"]), SL.bits(c["ro"]))


@pytest.mark.parametrize("pset,want_nf", [("between", [1, 3, 3, 2, 1, 1, 3]), ("below", [1, 2, 2, 2, 1, 1, 2])], ids=("between", "below"))
def test_rhomax_parameter_sets_in_double(oracle_mod, pset, want_nf):
    """`between`: the rho_old = 0 failures exhaust at the decide of rung 2 (rho_3 > rhomax), and the problem that comes with rho_old = 2
    tries rho_1 = 2/3 > rhomax once.  `below`: every rung 1 is above rhomax and is tried all the same; the loop never runs."""
    c0 = GS.case(GS.GRID12)
    c = SL.case_with_params(c0, pset)
    assert c["nf"].tolist() == want_nf and c["params"][6] != c0["params"][6] and np.array_equal(np.delete(c["params"], 6), np.delete(c0["params"], 6))
    s, plan = GS.make_plan(GS.GRID12, task_cap=4)
    _sweep(("double", "grid12-cap4", pset), plan, c, c["params"], f64, (0, 1, 2, 3, 5), 2, want_nf)
    want = _refs["double", "grid12-cap4", pset]
    assert np.array_equal(want["ok"], c["ok"]) and np.array_equal(SL.bits(want["rho"]), SL.bits(c["rho"])) and np.array_equal(SL.bits(want["ro"]), SL.bits(c["ro"]))
    assert (want["rho"][~want["ok"]] > c["params"][6]).all()
    assert np.array_equal(want["ro"][~want["ok"]], c["rho_old"][~want["ok"]])      # rho_old of a failure is the incoming one


FLOAT_PLANS = [("grid12-cap4-condensed", GS.GRID12, True, 4), ("forest3-cap4-uncondensed", GS.FOREST3, False, 4)]


@pytest.mark.parametrize("name,shape,cond,cap", FLOAT_PLANS, ids=[v[0] for v in FLOAT_PLANS])
def test_sweep_of_R_in_float(oracle_mod, name, shape, cond, cap):
    """the five-kind float mix (nfact 1, 10, 5, 4, 1): R = 0, 2 (all resume), 3 (the nfact-4 climber finishes on the last rung) and 9,
    the rung whose decide exhausts the failure; every rho in float32"""
    c = FS.case(shape)
    s, plan = FS.make_plan(shape, cond, cap)
    _sweep(("float", name, "default"), plan, c, c["p32"], f32, (0, 2, 3, SL.R_EXHAUST[f32]), 2, FS.WANT_NF)
    want = _refs["float", name, "default"]
    assert np.array_equal(want["ok"], c["ok"]) and np.array_equal(want["nf"], c["nf"])
    assert np.array_equal(SL.bits(want["rho"]), SL.bits(c["rho"].astype(f32))) and np.array_equal(SL.bits(want["ro"]), SL.bits(c["ro"].astype(f32)))


@pytest.mark.parametrize("pset,want_nf", [("between", [1, 3, 3, 2, 1]), ("below", [1, 2, 2, 2, 1])], ids=("between", "below"))
def test_rhomax_parameter_sets_in_float(oracle_mod, pset, want_nf):
    c0 = FS.case(GS.GRID12)
    c = SL.case_with_params(c0, pset, f32=True)
    assert c["nf"].tolist() == want_nf and c["p32"].dtype == f32
    s, plan = FS.make_plan(GS.GRID12, True, 4)
    _sweep(("float", "grid12-cap4-condensed", pset), plan, c, c["p32"], f32, (0, 1, 3), 2, want_nf)


# ---- 5. the ends the case set reaches, from the oracle's results ----
def test_the_case_set_reaches_every_end(oracle_mod):
    """from the ORACLE's decisions and the parameters alone: which end each problem of each (parameter set, R) the tests run comes to"""
    seen = set()
    c0 = GS.case(GS.GRID12)
    for pset, Rs in (("default", SL.R_SWEEP[1:]), ("between", (1, 2, 3, 5)), ("below", (1, 3))):
        c = SL.case_with_params(c0, pset)
        for R in Rs:
            e = SL.ends(c, R)
            seen |= {(pset, x) for x in e}
            if pset == "default":
                # the edges the sweep's values sit on
                assert (R <= 2) == (set(e) == {"first", "resumed-ok", "resumed-failed"}), (R, e)
                assert (e[3] == "rung") == (R >= 3) and (e[2] == "rung") == (R >= 5), (R, e)
                assert (e[1] == "exhausted-at-R") == (R == 19) and (e[1] == "exhausted-inside") == (R > 19), (R, e)
    for end in ("first", "rung", "exhausted-inside", "exhausted-at-R", "resumed-ok", "resumed-failed"):
        assert any(x == end for _, x in seen), end
    assert ("between", "exhausted-inside") in seen and ("between", "exhausted-at-R") in seen and ("below", "exhausted-at-R") in seen
    # no mix problem succeeds at rho_1 > rhomax (test_success_at_rho_1_above_rhomax_keeps_rho_old pins that branch by hand)
    assert not any(x == "rung-above-rhomax" for _, x in seen)
    fe = set()
    cf = FS.case(GS.GRID12)
    for R in (2, 3, SL.R_EXHAUST[f32]):
        fe |= set(SL.ends(cf, R, f32=True))
    assert {"first", "rung", "exhausted-at-R", "resumed-ok", "resumed-failed"} <= fe
