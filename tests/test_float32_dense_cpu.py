"""Float32 handles on the dense backend (tuning float32_dense), without a GPU: the tuning key and the ABI version, and what vouches
for the inputs of tests/test_float32_dense_gpu.py — every decision of every ladder rung far above float32 rounding by an
order-independent rule (tests/support/f32_dense.py: eig_margins), the oracle's (success, nfact) pattern, and a plain numpy float32
emulation of the backend's arithmetic as a sanity bound for the project's Float32 tolerances."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn
from tests.support import dense_cases as dc
from tests.support import f32_dense as FD
from tests.support import f32_general as G

ALL_CASES = [(shape, FD.MIX) for shape in FD.SHAPES] + [FD.GRAPH_CASE]


def _id(sc):
    return FD.shape_id(sc[0]) + f"-B{sc[1]}"


def test_version_is_0_4_3(built):
    assert hipldl.lib().cnl_version() >= 403


def test_tuning_key_is_known(built):
    s = syn.random_structure(60, 80, 4, 0.1, seed=3)
    rows, cols = s.kkt_pattern()
    assert hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(float32_general=1, float32_dense=1)).info["N"] == s.N
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(float32_densee=1))
    assert e.value.code == 1 and "unknown key" in str(e.value)


def test_tolerances_are_the_projects():
    assert FD.BWD_TOL == G.BWD_TOL == 512 * G.EPS32 and FD.FWD_TOL == G.FWD_TOL == 1e-3


@pytest.mark.parametrize("sc", ALL_CASES, ids=_id)
def test_oracle_pattern_and_eigenvalue_margins(built, sc):
    """(success, nfact) of the mix as the issue states them, and for every rung of every problem that is not hopeless
    |lambda_min(M(rho))| >= 1e-3 lambda_max with the sign the decision needs: no GPU test skips or reclassifies a problem."""
    shape, B = sc
    c = FD.case(shape, B)
    kinds = np.arange(B) % 5
    tall = shape == FD.TALL
    want_ok = [k != 1 for k in kinds]
    want_nf = [10 if k == 1 else 1 if (k in (0, 4) or tall) else 4 if k == 2 else 3 for k in kinds]
    assert list(c["ok"]) == want_ok and list(c["nf"]) == want_nf, (c["ok"], c["nf"])
    p = c["p32"].astype(np.float64)
    worst = np.inf
    for b in range(B):
        if kinds[b] == 1:
            assert np.isnan(c["vals"][b]).any()
            continue
        assert c["rho"][b] == dc.rungs(float(c["rho_old"][b]), int(c["nf"][b]), p)[-1]   # the ladder replayed in double
        if not tall and kinds[b] == 2:
            assert abs(c["rho"][b] - 20.1587) < 1e-3       # rho0 klarge^2
        if not tall and kinds[b] == 3:
            assert abs(c["rho"][b] - 16.0 / 3.0) < 1e-5    # kdec rho_old kinc
        for rho, rel, succeeds in FD.eig_margins(c, b):
            assert (rel >= FD.EIG_MARGIN) if succeeds else (rel <= -FD.EIG_MARGIN), (b, rho, rel, succeeds)
            worst = min(worst, abs(rel))
    print(f"{_id(sc)}: smallest |lambda_min| / lambda_max over all rungs {worst:.3g}")


@pytest.mark.parametrize("shape", FD.SHAPES, ids=FD.shape_id)
def test_float32_emulation_is_far_inside_the_tolerances(built, shape):
    """S formed in float32, LDL' without pivoting, both sweeps, r recovered — plain numpy, on the healthy problems: what float32 can
    do on these inputs lies orders of magnitude inside BWD_TOL and FWD_TOL, so the bars test the kernels, not the format."""
    c = FD.case(shape)
    s = c["s"]
    for b in (0, 4):
        d = FD.emulate32(s, c["vals"][b], c["rhs"][b])
        be = G.backward_error(s, c["vals"][b], c["rhs"][b], d)
        fe = np.abs(d - c["d"][b]).max() / np.abs(c["d"][b]).max()
        print(f"{FD.shape_id(shape)} problem {b}: backward {be / FD.EPS32:.2f} eps32, forward {fe:.2e}")
        assert be <= FD.BWD_TOL / 64 and fe <= FD.FWD_TOL / 64, (b, be, fe)
