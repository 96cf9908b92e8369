"""Float32 general handles on the Direct route (tuning float32_direct_records), without a GPU: the tuning key, the ABI version, and
the plan cnl_create_f32_ex builds for such a handle (tests/support/f32_direct.py: DIRECT_PLAN — the forced throughput analysis of
the condensed system with direct records, not shaped for a lean or solve-only instance) on the patterns the GPU tests name: which
of them get direct records, what those records compute, and which are refused and keep the records of the condensed form."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn
from oracle import oracle as O
from tests.support.f32_direct import CONDENSED_PLAN, DIRECT_PLAN
from tests.support.rec_sim import RecSim

EIG_TOL = 2.220446049250313e-16


def _plan(s, **opt):
    rows, cols = s.kkt_pattern()
    return hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(**opt))


def test_tuning_key_is_known(built):
    s = syn.random_structure(60, 80, 4, 0.1, seed=3)
    assert _plan(s, float32_direct_records=1).info["N"] == s.N
    with pytest.raises(hipldl.CnlError) as e:
        _plan(s, float32_direct_record=1)
    assert e.value.code == 1 and "unknown key" in str(e.value)


def test_version_is_0_4_2(built):
    assert hipldl.lib().cnl_version() >= 402


DIRECT = [
    ("chain", lambda: syn.band_structure(60, 2, hw=3), (7, 0, 0)),
    ("class32", lambda: syn.random_structure(30, 40, 2, 0.15, seed=1), (0, 2, 0)),
    ("class64", lambda: syn.random_structure(60, 80, 4, 0.1, seed=3), (0, 0, 2)),
    ("all-classes", lambda: syn.random_structure(40, 56, 2, 0.06, seed=3), (2, 3, 1)),
    ("lockstep", lambda: syn.band_structure(300, 4, hw=3), (38, 0, 0)),
    ("timing", lambda: syn.band_structure(1000, 10, hw=3), (126, 0, 0))]


@pytest.mark.parametrize("name,make,classes", DIRECT, ids=[c[0] for c in DIRECT])
def test_direct_records_of_the_named_patterns(built, name, make, classes):
    s = make()
    rows, cols = s.kkt_pattern()
    plan = _plan(s, **DIRECT_PLAN)
    v2 = plan.info["v2"]
    assert v2 is not None and plan.info["ncond"] == s.nequ, plan.info
    assert (v2["fronts16"], v2["fronts32"], v2["fronts64"]) == classes, v2
    nrec, nrec0 = plan.array("rec").size, _plan(s, **CONDENSED_PLAN).array("rec").size
    print(f"{name}: rec words {nrec0} -> {nrec}")
    assert nrec > nrec0
    assert not (plan.array("brec")[7] & 256)   # no backward rows: the post-pass recovers the residual components
    # one problem through the record streams, as tests/test_plan_cpu.py::test_record_streams_reproduce_the_oracle does
    vals, rhs = (syn.band_values if s.name == "band" else syn.random_values)(s, 77)
    off = s.offsets()
    vals[off[4]:off[5]] = -np.random.default_rng(1).uniform(0.5, 2.0, s.nequ)  # general residual pivots
    vals[off[6]:off[7]] = 0.25                                                  # some rho
    sim = RecSim(plan, s.nnzNS, s.N)
    L, npos, nzer = sim.forward(vals, rhs, EIG_TOL)
    assert sim.stats["products"] > 0 and sim.stats["raw"] > 0
    d = sim.backward(L, s.N, vals, rhs)
    orc = O.Oracle(s.N, rows, cols, plan.array("perm").astype(np.int64))
    ok, pos0, zer0 = orc.try_to_factorize(vals, s.nvar, s.nequ, s.ncon, EIG_TOL, return_inertia=True)
    d0 = orc.solve_ldl(rhs)
    dr = vals[off[4]:off[5]]
    assert sim.owned == s.nequ   # every condensed pivot is owned by exactly one front: the handle's count_d
    assert sim.own_pos == int((dr > EIG_TOL).sum()) and sim.own_zer == int((np.abs(dr) <= EIG_TOL).sum())
    assert npos + sim.own_pos == pos0 and nzer + sim.own_zer == zer0
    kept = ~np.isnan(d)
    assert kept.sum() == s.N - s.nequ and not kept[s.nvar:s.nvar + s.nequ].any()
    assert np.abs(d[kept] - d0[kept]).max() <= 1e-10 * np.abs(d0).max()


REFUSED = [
    ("class32-dense", lambda: syn.dense_structure(24, 40), (0, 1, 0)),          # more than 1 023 raw values
    ("chain-hw4", lambda: syn.band_structure(60, 2, hw=4), (9, 0, 0)),          # a fast front with more than 128 raw values
    ("class64-dense-70", lambda: syn.dense_structure(40, 70), None),
    ("class64-dense-90", lambda: syn.dense_structure(60, 90), None)]


@pytest.mark.parametrize("name,make,classes", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_patterns_keep_the_condensed_records(built, name, make, classes):
    s = make()
    plan, plan0 = _plan(s, **DIRECT_PLAN), _plan(s, **CONDENSED_PLAN)
    v2 = plan.info["v2"]
    assert v2 is not None
    if classes is not None:
        assert (v2["fronts16"], v2["fronts32"], v2["fronts64"]) == classes, v2
    else:
        assert (v2["fronts16"], v2["fronts32"], v2["fronts64"]) == (0, 0, 1), v2
    assert np.array_equal(plan.array("rec"), plan0.array("rec"))
    assert np.array_equal(plan.array("brec"), plan0.array("brec"))
