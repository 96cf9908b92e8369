"""Float32 general handles on the general form of the dense backend (tuning float32_general_dense), without a GPU: the tuning key and
the ABI version, the plan facts that decide the route for every shape of tests/support/f32_general_dense.py, and what vouches for the
inputs of tests/test_float32_general_dense_gpu.py — the oracle's (success, nfact) pattern and every decision of every ladder rung at
least EIG_MARGIN away from a flip, by eigenvalues (tests/support/f32_dense.py: eig_margins)."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn
from tests.support import dense_cases as dc
from tests.support import f32_general as G
from tests.support import f32_general_dense as GD

CNL_ERR_ARG = 1


def test_version_is_0_4_4(built):
    assert hipldl.lib().cnl_version() >= 404


def test_tuning_key_is_known(built):
    s = GD.structure(GD.NOT_TAKEN)
    rows, cols = s.kkt_pattern()
    for v in (1, 2):
        assert hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(float32_general=1, float32_general_dense=v)).info["N"] == s.N
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(float32_general_densee=1))
    assert e.value.code == CNL_ERR_ARG and "unknown key" in str(e.value)


def test_key_without_float32_general_is_an_argument_error(built):
    """refused before a device is asked for, with a message that names both keys"""
    s = GD.structure(GD.SMALLEST)
    rows, cols = s.kkt_pattern()
    for v in (1, 2):
        with pytest.raises(hipldl.CnlError) as e:
            hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=2, dtype=np.float32, options=hipldl.Options(float32_general_dense=v))
        assert e.value.code == CNL_ERR_ARG and "float32_general_dense" in str(e.value) and "float32_general = 1" in str(e.value)


def test_tolerances_are_the_projects():
    assert GD.BWD_TOL == G.BWD_TOL == 512 * G.EPS32 and GD.FWD_TOL == G.FWD_TOL == 1e-3 and GD.EIG_MARGIN == 1e-3


def test_the_largest_shape_is_the_float64_tests():
    assert list(GD.SHAPES)[-1] == dc.GENERAL


@pytest.mark.parametrize("shape", list(GD.SHAPES) + [GD.NOT_TAKEN], ids=GD.shape_id)
def test_plan_facts(built, shape):
    """condensed order and largest front of the condensed throughput plan, as the default analysis (register-front records allowed)
    and as the analysis a Float32 general handle is built on see them: every shape of the table has order 96 .. 4096 and a front
    above 64, which the register-front kernel refuses; the `not taken` pattern has neither (order 64, and a plan that kernel takes)"""
    s = GD.structure(shape)
    rows, cols = s.kkt_pattern()
    dflt = hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT)).info
    f32 = hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(**GD.COND_PLAN, **GD.OPTIONS)).info
    for info in (dflt, f32):
        assert s.N - info["ncond"] == s.nvar + s.ncon
    order, fmax = s.N - dflt["ncond"], dflt["fmax"]
    if shape == GD.NOT_TAKEN:
        assert (order, fmax) == (64, 63) and dflt["v2"] is not None
    else:
        assert (order, fmax) == GD.SHAPES[shape] == (s.N - f32["ncond"], f32["fmax"])
        assert 96 <= order <= 4096 and fmax > 64 and dflt["v2"] is None and f32["v2"] is None


@pytest.mark.parametrize("shape", list(GD.SHAPES), ids=GD.shape_id)
def test_oracle_pattern_and_eigenvalue_margins(built, shape):
    """(success, nfact) = ([1, 0, 1, 1, 1], [1, 10, 5, 4, 1]) on every shape, at B = 5 and (a second mix) B = 10 where the GPU tests
    use it; for every rung of every problem that is not hopeless lambda_min(M(rho)) is at least EIG_MARGIN of the largest
    |eigenvalue| away from zero, with the sign the decision needs."""
    worst = np.inf
    for B in (GD.MIX, 2 * GD.MIX) if shape == GD.SMALLEST else (GD.MIX,):
        c = GD.case(shape, B)
        reps = B // GD.MIX
        assert list(c["ok"]) == GD.WANT_OK * reps and list(c["nf"]) == GD.WANT_NF * reps, (c["ok"], c["nf"])
        p = c["p32"].astype(np.float64)
        for b in range(B):
            if b % 5 == 1:
                assert np.isnan(c["vals"][b]).any()
                continue
            assert c["rho"][b] == dc.rungs(float(c["rho_old"][b]), int(c["nf"][b]), p)[-1]   # the ladder replayed in double
            for rho, rel, succeeds in GD.eig_margins(c, b):
                assert (rel >= GD.EIG_MARGIN) if succeeds else (rel <= -GD.EIG_MARGIN), (b, rho, rel, succeeds)
                worst = min(worst, abs(rel))
    print(f"{GD.shape_id(shape)}: smallest |lambda_min| / lambda_max over all rungs {worst:.3g}")
