"""Float32 general handles on the condensed system (tuning float32_general = 1 with float32_condense = 1), without a GPU: the tuning
key, the sizes of the condensed plan against the uncondensed one, the condensed path restated in numpy float32
(tests/support/plan_sim_f32_cond.py: slots summed in list order, PlanSimF32's factor and backward sweep on the condensed plan, the
post-pass) against the fp64 oracle on the widened inputs within the project's Float32 tolerances (tests/support/f32_general.py), and
the pivot margin of every input set tests/test_float32_condense_gpu.py uses — shown here, before a GPU sees them."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn
from oracle import oracle as O
from tests.support import f32_general as G
from tests.support.plan_sim import PlanSim
from tests.support.plan_sim_f32_cond import PlanSimF32Cond

PATTERNS = {
    "dense-40-70": lambda: syn.dense_structure(40, 70),
    "dense-100-160": lambda: syn.dense_structure(100, 160),
    "random": lambda: syn.random_structure(60, 80, 4, 0.1, seed=3),
    "band-hw3": lambda: syn.band_structure(400, 4, hw=3),
    "band-hw4": lambda: syn.band_structure(400, 4, hw=4),
}
# the plan of a Float32 general handle with float32_condense = 1, as Plan options (cnl_create_f32_ex forces the same switches)
CONDENSED_PLAN = dict(G.GENERAL_PLAN, condense=1)


def _plan(s, **opt):
    rows, cols = s.kkt_pattern()
    return hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=24, options=hipldl.Options(**opt))


def test_tuning_key_is_known(built):
    """cnl_plan_create_ex accepts float32_condense = 1 (an unknown key is CNL_ERR_ARG: tuning_parse); the key alone changes no plan"""
    s = PATTERNS["random"]()
    pl = _plan(s, float32_condense=1)
    assert pl.info["N"] == s.N
    ref = _plan(s)
    assert {k: v for k, v in pl.info.items()} == {k: v for k, v in ref.info.items()}
    pl2 = _plan(s, float32_general=1, float32_condense=1)
    assert pl2.info == ref.info
    with pytest.raises(hipldl.CnlError) as e:
        _plan(s, float32_condensed=1)
    assert e.value.code == 1 and "unknown key" in str(e.value)


@pytest.mark.parametrize("name", ["dense-40-70", "dense-100-160", "random"])
def test_condensed_plan_sizes(built, name):
    """every residual node is condensed (ncond == nequ) and the work area of the forward pass shrinks"""
    s = PATTERNS[name]()
    on, off = _plan(s, **CONDENSED_PLAN), _plan(s, **G.GENERAL_PLAN)
    assert off.info["ncond"] == 0
    assert on.info["ncond"] == s.nequ
    assert on.info["fwd_peak"] < off.info["fwd_peak"], (on.info["fwd_peak"], off.info["fwd_peak"])
    print(f"{name}: fwd_peak {off.info['fwd_peak']} -> {on.info['fwd_peak']}, fmax {off.info['fmax']} -> {on.info['fmax']}, "
          f"flops {off.info['flops']} -> {on.info['flops']}")


# ---- the CPU model against the oracle ----
GEN = {"dense-40-70": G.dense_inputs, "dense-100-160": G.dense_inputs, "random": G.random_inputs, "band-hw3": G.band_inputs}
MODEL_CASES = ([("dense-40-70", seed, {}) for seed in (100, 101)] + [("dense-100-160", 100, {})] +
               [("random", seed, {}) for seed in (100, 101, 102)] + [("random", 200, dict(posdef=False)), ("random", 205, dict(posdef=False))] +
               [("band-hw3", 4000, {}), ("band-hw3", 7000, dict(stress="ladder"))])


@pytest.fixture(scope="module")
def sims(built):
    out = {}
    for name in GEN:
        s = PATTERNS[name]()
        out[name] = (s, PlanSimF32Cond(_plan(s, **CONDENSED_PLAN)))
    return out


@pytest.mark.parametrize("name,seed,kw", MODEL_CASES)
def test_condensed_path_in_float32_stays_within_the_tolerances(sims, name, seed, kw):
    s, sim = sims[name]
    vals, rhs = GEN[name](syn, s, [seed], **kw)
    p32 = hipldl.default_params(np.float32)
    ref = G.oracle_newton(O, s, vals, rhs, np.zeros(1, np.float32), p32)
    assert ref["ok"][0]
    v = vals.copy()
    d, ok, rho, ro, nf = sim.newton_system(v[0], rhs[0], s.nvar, s.nequ, s.ncon, 0.0, p32)
    assert d.dtype == np.float32
    be, fe = G.check_results(s, ref, v, rhs, d, [ok], [rho], [ro], [nf])
    print(f"{name} seed {seed}: nfact {nf}, backward error {be / G.EPS32:.1f} eps32, forward error {fe:.2e}")


def test_slots_are_summed_in_list_order(sims):
    """the rule the kernels follow: a slot is the float32 sum of its contributions one after the other, in list order — restated here
    with a scalar loop and compared bit for bit with the model's vectorised form"""
    s, sim = sims["random"]
    vals, rhs = G.random_inputs(syn, s, [100])
    got = sim.condense(vals[0], rhs[0])
    x = np.concatenate([vals[0], rhs[0]])
    F = np.float32
    for slot in range(sim.nslot):
        acc = F(0)
        for c in range(sim.c_ptr[slot], sim.c_ptr[slot + 1]):
            if sim.c_b[c] < 0:
                acc = F(acc + x[sim.c_a[c]])
            else:
                acc = F(acc - F(F(x[sim.c_a[c]] * x[sim.c_b[c]]) / x[sim.c_d[c]]))
        assert G.bits(acc) == G.bits(got[slot]), slot
    # ... and against the fp64 condensation of the same inputs: within a few roundings per contribution
    ref = PlanSim.condense(sim, vals[0].astype(np.float64), rhs[0].astype(np.float64))
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 4 * sim.c_len.max() * G.EPS32 * scale


# ---- the inputs of the GPU file keep the margin check_results' oracle demands ----
def _margin_sets():
    yield "dense-40-70", G.dense_inputs, range(100, 110), {}, (0.0,)
    yield "dense-100-160", G.dense_inputs, range(100, 104), {}, (0.0,)
    yield "random", G.random_inputs, range(100, 124), {}, (0.0,)
    yield "random", G.random_inputs, range(200, 224), dict(posdef=False), (0.0, 0.3)
    yield "random", G.random_inputs, [205], dict(posdef=False), (0.0,)
    for hw in ("band-hw3", "band-hw4"):
        yield hw, G.band_inputs, range(4000, 4024), {}, (0.0,)
        yield hw, G.band_inputs, range(7000, 7024), dict(stress="ladder"), (0.0,)


@pytest.mark.parametrize("name,gen,seeds,kw,rho_olds", list(_margin_sets()))
def test_gpu_inputs_keep_the_pivot_margin(built, name, gen, seeds, kw, rho_olds):
    """G.oracle_newton asserts, per problem, that every pivot of the last factorisation lies at least MARGIN * max|D| from eig_tol"""
    s = PATTERNS[name]()
    vals, rhs = gen(syn, s, seeds, **kw)
    p32 = hipldl.default_params(np.float32)
    for ro in rho_olds:
        ref = G.oracle_newton(O, s, vals, rhs, np.full(len(vals), ro, np.float32), p32)
        assert ref["ok"].all()
