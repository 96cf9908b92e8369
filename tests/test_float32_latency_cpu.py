"""The Float32 latency path (tuning float32_latency), without a GPU: the tuning key, its refusals at cnl_plan_create_ex and the ABI
version; the float plans, with the key, of every (shape, batch) the GPU tests use — tasks, stages, front classes, backward rows and
no product lists where the plan is lean — executed by rec_sim.StagedSim against the oracle, stage by stage with the tasks of a
stage in either order and in the dataflow order; the plan with every part switched off and the fallback plans equal to the plans
without the key; the smallest batch that needs more than one fused ladder launch; and the float32 numpy model of
tests/support/f32_staged.py reproducing the oracle's decisions on every input the GPU tests name, in the order of the plan with the key."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn
from oracle import oracle as O
from tests.support import f32_general as G
from tests.support import f32_latency as T
from tests.support import f32_staged as S
from tests.support.f32_direct import DIRECT_PLAN
from tests.support.rec_sim import StagedSim

EIG_TOL = 2.220446049250313e-16
CNL_ERR_ARG = 1


def _plan(s, batch, **opt):
    rows, cols = s.kkt_pattern()
    return hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=batch, options=hipldl.Options(**opt))


def _same_plan(a, b, names=("perm", "rec", "brec", "tasks", "stage_ptr", "fronts")):
    for name in names:
        assert np.array_equal(a.array(name), b.array(name)), name


def test_tuning_key_and_version(built):
    s = S.structure(syn, "hw2")
    assert _plan(s, 13, **T.PLAN_KEYS).info["N"] == s.N
    assert _plan(s, 13, float32_general=1, float32_latency=0).info["N"] == s.N
    with pytest.raises(hipldl.CnlError) as e:
        _plan(s, 13, float32_general=1, float32_latenc=1)
    assert e.value.code == CNL_ERR_ARG and "unknown key" in str(e.value)
    assert hipldl.lib().cnl_version() >= 502


@pytest.mark.parametrize("opt", [dict(float32_latency=1), dict(float32_general=1, float32_latency=2), dict(float32_general=1, float32_latency=-1),
                                 dict(float32_general=1, float32_latency=1, float32_refine=1)],
                         ids=["alone", "two", "negative", "with-refine"])
def test_refusals_name_the_key(built, opt):
    s = S.structure(syn, "hw2")
    with pytest.raises(hipldl.CnlError) as e:
        _plan(s, 13, **opt)
    assert e.value.code == CNL_ERR_ARG and "float32_latency" in str(e.value)


def test_float32_staged_keeps_its_own_refusal(built):
    """float32_staged = 2 is refused as before, with or without the new key beside it"""
    s = S.structure(syn, "hw2")
    for opt in (dict(float32_general=1, float32_staged=2), dict(float32_general=1, float32_staged=2, float32_latency=1)):
        with pytest.raises(hipldl.CnlError) as e:
            _plan(s, 13, **opt)
        assert e.value.code == CNL_ERR_ARG and "float32_staged" in str(e.value)


@pytest.mark.parametrize("shape,B", list(T.PLANS), ids=[f"{k[0]}-{k[1]}" for k in T.PLANS])
def test_latency_plans_of_the_named_shapes(built, shape, B):
    ntasks, nstages, classes, lean = T.PLANS[(shape, B)]
    s = S.structure(syn, shape)
    rows, cols = s.kkt_pattern()
    plan = _plan(s, B, **T.PLAN_KEYS)
    tasks, stage_ptr = plan.array("tasks").reshape(-1, 8), plan.array("stage_ptr")
    assert len(tasks) > 1 and stage_ptr[-1] == len(tasks)
    assert (len(tasks), len(stage_ptr) - 1) == (ntasks, nstages)
    v2 = plan.info["v2"]
    assert v2 is not None and plan.info["ncond"] == s.nequ
    assert (v2["fronts16"], v2["fronts32"], v2["fronts64"]) == classes
    # lean: every front of the fast class, none with product lists, and the backward records recover the residual rows
    assert lean == (classes[1] == 0 and classes[2] == 0)
    assert T.back_rows(plan.array) == lean
    if lean:
        assert T.listprod_fronts(plan.array, plan.info["nsuper"]) == 0
    # the same plan with float32_staged written out beside the key, and with plan_kind = LATENCY
    for more in (dict(T.PLAN_KEYS, float32_staged=1), dict(T.PLAN_KEYS, plan_kind=hipldl.PLAN_LATENCY)):
        _same_plan(_plan(s, B, **more), plan)
    # every part switched off: the plan of float32_staged = 1; a plan that is not lean is that plan anyway
    staged = _plan(s, B, **S.PLAN_KEYS)
    _same_plan(_plan(s, B, **T.PLAN_KEYS, **T.ALL_OFF), staged)
    assert not T.back_rows(staged.array)
    if not lean:
        _same_plan(plan, staged)
    # the dataflow and ladder switches do not touch the plan
    _same_plan(_plan(s, B, **T.PLAN_KEYS, dataflow=0, device_ladder=0), plan)
    vals, rhs = syn.band_values(s, 78)
    off = s.offsets()
    vals[off[4]:off[5]] = -np.random.default_rng(2).uniform(0.5, 2.0, s.nequ)
    vals[off[6]:off[7]] = 0.125
    orc = O.Oracle(s.N, rows, cols, plan.array("perm").astype(np.int64))
    ok, pos0, zer0 = orc.try_to_factorize(vals, s.nvar, s.nequ, s.ncon, EIG_TOL, return_inertia=True)
    d0 = orc.solve_ldl(rhs)
    for reverse, dataflow in ((False, False), (True, False), (False, True)):
        sim = StagedSim(plan, s.nnzNS, s.N)
        d, npos, nzer = sim.run(vals, rhs, EIG_TOL, s.N, reverse=reverse, dataflow=dataflow)
        assert (npos, nzer) == (pos0, zer0)
        kept = ~np.isnan(d)
        if lean:   # the backward rows give the residual components too: no post-pass
            assert kept.all()
        else:
            assert kept.sum() == s.N - s.nequ and not kept[s.nvar:s.nvar + s.nequ].any()
        assert np.abs(d[kept] - d0[kept]).max() <= 1e-10 * np.abs(d0).max()


def test_smallest_batch_with_more_than_one_fused_launch(built):
    """setup_v2's ladder rule on a device that holds 2 048 wavefronts: batches of cfg4's pattern below the recorded one take one fused
    launch, the recorded one two, with >= 16 tasks; cfg4 x 4 096 (three tasks, two launches) keeps the sequential launch"""
    shape, B = T.MULTI_LAUNCH
    s = S.structure(syn, shape)
    nt = lambda b: len(_plan(s, b, **T.PLAN_KEYS).array("tasks")) // 8
    assert nt(B) == T.PLANS[(shape, B)][0] >= 16
    assert T.fused_launches(nt(B), B, T.RESIDENT_FULL) == (1, 2)
    for b in (B - 1, B - 25, 256):
        assert T.fused_launches(nt(b), b, T.RESIDENT_FULL) == (1, 1), b
    assert T.fused_launches(T.PLANS[("cfg4", 4096)][0], 4096, T.RESIDENT_FULL) == (0, 2)
    assert T.fused_launches(T.PLANS[("hw3", 13)][0], 13, T.RESIDENT_FULL) == (1, 1)
    assert T.fused_launches(T.PLANS[("hw3", 13)][0], 13, T.RESIDENT_FULL, fused=1) == (2, 1)


FALLBACKS = [("no-tasks", lambda: syn.random_structure(60, 80, 4, 0.1, seed=3), 8, {}),          # two fronts: nothing to cut into tasks
             ("batch-4097", lambda: S.structure(syn, "cfg4"), 4097, {}),
             ("throughput", lambda: S.structure(syn, "hw2"), 13, dict(plan_kind=hipldl.PLAN_THROUGHPUT)),
             # a hw=3 latency order without direct records (as for a Float64 handle, which falls back too)
             ("hw3-no-direct", lambda: syn.band_structure(300, 4, hw=3), 12, {})]


@pytest.mark.parametrize("name,make,B,opt", FALLBACKS, ids=[c[0] for c in FALLBACKS])
def test_fallbacks_have_the_plan_without_the_key(built, name, make, B, opt):
    s = make()
    a = _plan(s, B, **T.PLAN_KEYS, **opt)
    b = _plan(s, B, **DIRECT_PLAN)
    c = _plan(s, B, **S.PLAN_KEYS, **opt)
    assert a.array("tasks").size == 0 and a.info == b.info == c.info
    _same_plan(a, b)
    _same_plan(a, c)


@pytest.mark.parametrize("shape", ["hw2", "hw3", "cfg4"])
@pytest.mark.parametrize("kind,rho_old", [("clean", 0.0), ("mixed", 0.0), ("mixed", 0.3)])
def test_float32_model_reproduces_the_oracle_on_the_named_inputs(built, shape, kind, rho_old):
    """every input the GPU tests name: the oracle's (success, nfact, rho, rho_old) — pivot margins asserted by oracle_newton — are
    those of an LDL' in float32 in the order of the plan WITH the key (cfg4: one front more than without it)"""
    s = S.structure(syn, shape)
    vals, rhs = S.distinct_inputs(syn, s, kind)
    p32 = S.params(hipldl, kind == "mixed")
    ref = G.oracle_newton(O, s, vals, rhs, np.full(S.NDISTINCT, rho_old, np.float32), p32)
    perm = _plan(s, 13, **T.PLAN_KEYS).array("perm")
    for b in range(S.NDISTINCT):
        ok, nf, rho, ro = S.model_newton32(s, perm, vals[b], rho_old, p32)
        assert (ok, nf) == (bool(ref["ok"][b]), int(ref["nf"][b])), b
        assert np.float32(rho) == np.float32(ref["rho"][b]) and np.float32(ro) == np.float32(ref["ro"][b]), b
