"""Staged execution of Float32 general handles (tuning float32_staged), without a GPU: the tuning key and its refusals at
cnl_plan_create_ex, the ABI version, the latency plans cnl_create_f32_ex builds for the shapes the GPU tests name (task and stage
counts, front classes, what the staged record streams compute), the plans of the fallbacks, and the inputs the GPU tests name —
the fp64 oracle's decisions on them (with its pivot-margin assertion) reproduced by a numpy model in float32."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn
from oracle import oracle as O
from tests.support import f32_general as G
from tests.support import f32_staged as S
from tests.support.f32_direct import DIRECT_PLAN
from tests.support.rec_sim import StagedSim

EIG_TOL = 2.220446049250313e-16
CNL_ERR_ARG = 1


def _plan(s, batch, **opt):
    rows, cols = s.kkt_pattern()
    return hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=batch, options=hipldl.Options(**opt))


def test_tuning_key_and_version(built):
    s = S.structure(syn, "hw2")
    assert _plan(s, 13, **S.PLAN_KEYS).info["N"] == s.N
    assert _plan(s, 13, float32_general=1, float32_staged=0).info["N"] == s.N
    with pytest.raises(hipldl.CnlError) as e:
        _plan(s, 13, float32_general=1, float32_stage=1)
    assert e.value.code == CNL_ERR_ARG and "unknown key" in str(e.value)
    assert hipldl.lib().cnl_version() >= 501


@pytest.mark.parametrize("opt", [dict(float32_staged=1), dict(float32_general=1, float32_staged=2), dict(float32_general=1, float32_staged=-1),
                                 dict(float32_general=1, float32_staged=1, float32_refine=1)],
                         ids=["alone", "two", "negative", "with-refine"])
def test_refusals_name_the_key(built, opt):
    s = S.structure(syn, "hw2")
    with pytest.raises(hipldl.CnlError) as e:
        _plan(s, 13, **opt)
    assert e.value.code == CNL_ERR_ARG and "float32_staged" in str(e.value)


def test_latency_plan_needs_the_batch(built):
    s = S.structure(syn, "hw2")
    with pytest.raises(hipldl.CnlError) as e:
        _plan(s, None, plan_kind=hipldl.PLAN_LATENCY, **S.PLAN_KEYS)
    assert e.value.code == CNL_ERR_ARG


@pytest.mark.parametrize("shape,B", list(S.PLANS), ids=[f"{k[0]}-{k[1]}" for k in S.PLANS])
def test_staged_plans_of_the_named_shapes(built, shape, B):
    """the float plan has the task and stage counts the GPU tests rely on, direct records without backward rows (no lean instance),
    and StagedSim — the staged kernel's execution in numpy, tasks of a stage in either order — reproduces the oracle's inertia and
    solution on it"""
    ntasks, nstages, classes, v2_solve = S.PLANS[(shape, B)]
    s = S.structure(syn, shape)
    rows, cols = s.kkt_pattern()
    plan = _plan(s, B, **S.PLAN_KEYS)
    tasks, stage_ptr = plan.array("tasks").reshape(-1, 8), plan.array("stage_ptr")
    assert len(tasks) > 1 and stage_ptr[-1] == len(tasks)
    assert (len(tasks), len(stage_ptr) - 1) == (ntasks, nstages)
    v2 = plan.info["v2"]
    assert v2 is not None and plan.info["ncond"] == s.nequ
    assert (v2["fronts16"], v2["fronts32"], v2["fronts64"]) == classes
    assert v2_solve == (classes[1] == 0 and classes[2] == 0)
    assert not (plan.array("brec")[7] & 256)
    # which instance launch_newton2_staged's rule picks: cfg4's chain at 4 096 problems fills the slots but has 100 fronts for two
    # first-stage tasks, so it keeps the immediate stores; the "late" shape is the one the rule gives the LATE instance
    assert S.late_rule(B, stage_ptr, plan.info["nsuper"]) == (shape == "late")
    # the same plan whatever float32_* keys the caller writes out beside the key, and with plan_kind = LATENCY
    for more in (dict(S.UNSTAGED, float32_staged=1), dict(S.PLAN_KEYS, plan_kind=hipldl.PLAN_LATENCY)):
        other = _plan(s, B, **more)
        for name in ("perm", "rec", "brec", "tasks", "stage_ptr"):
            assert np.array_equal(other.array(name), plan.array(name)), name
    vals, rhs = syn.band_values(s, 78)
    off = s.offsets()
    vals[off[4]:off[5]] = -np.random.default_rng(2).uniform(0.5, 2.0, s.nequ)
    vals[off[6]:off[7]] = 0.125
    orc = O.Oracle(s.N, rows, cols, plan.array("perm").astype(np.int64))
    ok, pos0, zer0 = orc.try_to_factorize(vals, s.nvar, s.nequ, s.ncon, EIG_TOL, return_inertia=True)
    d0 = orc.solve_ldl(rhs)
    for reverse in (False, True):
        sim = StagedSim(plan, s.nnzNS, s.N)
        d, npos, nzer = sim.run(vals, rhs, EIG_TOL, s.N, reverse=reverse, dataflow=False)
        assert (npos, nzer) == (pos0, zer0)
        kept = ~np.isnan(d)
        assert kept.sum() == s.N - s.nequ and not kept[s.nvar:s.nvar + s.nequ].any()
        assert np.abs(d[kept] - d0[kept]).max() <= 1e-10 * np.abs(d0).max()


FALLBACKS = [("no-tasks", lambda: syn.random_structure(60, 80, 4, 0.1, seed=3), 8, {}),          # two fronts: nothing to cut into tasks
             ("batch-4097", lambda: S.structure(syn, "cfg4"), 4097, {}),
             ("throughput", lambda: S.structure(syn, "hw2"), 13, dict(plan_kind=hipldl.PLAN_THROUGHPUT)),
             # the lockstep test's pattern: its latency order gets no direct records (as for a Float64 handle, which falls back too)
             ("lockstep", lambda: syn.band_structure(300, 4, hw=3), 12, {})]


@pytest.mark.parametrize("name,make,B,opt", FALLBACKS, ids=[c[0] for c in FALLBACKS])
def test_fallbacks_have_the_plan_without_the_key(built, name, make, B, opt):
    s = make()
    a = _plan(s, B, **S.PLAN_KEYS, **opt)
    # (cnl_plan_create_ex makes a Float32 general handle's plan only behind the key: without it the plan cnl_create_f32_ex builds is
    #  written out as Plan options, tests/support/f32_direct.py)
    b = _plan(s, B, **DIRECT_PLAN)
    assert a.array("tasks").size == 0 and a.info == b.info
    for arr in ("perm", "rec", "brec", "tasks", "stage_ptr", "fronts"):
        assert np.array_equal(a.array(arr), b.array(arr)), arr


@pytest.mark.parametrize("shape", ["hw2", "hw3", "cfg4"])
@pytest.mark.parametrize("kind,rho_old", [("clean", 0.0), ("mixed", 0.0), ("mixed", 0.3)])
def test_float32_model_reproduces_the_oracle_on_the_named_inputs(built, shape, kind, rho_old):
    """every input the GPU tests name: the oracle's (success, nfact, rho, rho_old) — pivot margins asserted by oracle_newton — are
    those of an LDL' in float32 in the plan's order; the mixed batch has its climbers and its hopeless problem where the tests say"""
    s = S.structure(syn, shape)
    vals, rhs = S.distinct_inputs(syn, s, kind)
    p32 = S.params(hipldl, kind == "mixed")
    ref = G.oracle_newton(O, s, vals, rhs, np.full(S.NDISTINCT, rho_old, np.float32), p32)
    if kind == "clean":
        assert ref["ok"].all() and (ref["nf"] == 1).all()
    else:
        climbed = sorted(S.CLIMBERS + (S.HOPELESS,))
        assert [b for b in range(S.NDISTINCT) if ref["nf"][b] > 1] == climbed
        assert ref["ok"][list(S.CLIMBERS)].all() and bool(ref["ok"][S.HOPELESS]) == (rho_old != 0.0)
        if rho_old == 0.0:
            assert ref["rho"][S.HOPELESS] > S.RHO_MAX_SMALL and ref["ro"][S.HOPELESS] == 0.0
    perm = _plan(s, 13, **S.PLAN_KEYS).array("perm")
    for b in range(S.NDISTINCT):
        ok, nf, rho, ro = S.model_newton32(s, perm, vals[b], rho_old, p32)
        assert (ok, nf) == (bool(ref["ok"][b]), int(ref["nf"][b])), b
        assert np.float32(rho) == np.float32(ref["rho"][b]) and np.float32(ro) == np.float32(ref["ro"][b]), b
