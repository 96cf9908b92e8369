"""Tuning float32_refine on the host side: the key at cnl_plan_create_ex, the new symbols, the rows of the full KKT matrix
(cnl_plan_get "kkt_row_*") against synthetic.dense_kkt, and the numpy model of the refinement (tests/support/f32_refine.py)
against the two derived bounds for every input the GPU tests name.  No GPU."""
import os

import numpy as np
import pytest

from tests.support import f32_refine as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CNL_ERR_ARG = 1


def _mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    return hipldl, syn


def _plan(hipldl, s, **opt):
    rows, cols = s.kkt_pattern()
    return hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(**opt))


def test_plan_create_accepts_the_key(built):
    hipldl, syn = _mods()
    s = syn.random_structure(60, 80, 4, 0.1, 1)
    assert _plan(hipldl, s, float32_general=1, float32_refine=2).info["N"] == s.N
    # the plan is the inner Float32 handle's: float32_condense condenses it, the key alone does not
    assert _plan(hipldl, s, float32_general=1, float32_refine=2).info["ncond"] == 0
    assert _plan(hipldl, s, float32_general=1, float32_condense=1, float32_refine=2).info["ncond"] > 0


@pytest.mark.parametrize("opt, word", [(dict(float32_general=1, float32_refine=5), "0 (none) .. 4"), (dict(float32_general=1, float32_refine=-1), "0 (none) .. 4"),
                                       (dict(float32_refine=2), "float32_general"),
                                       (dict(float32_general=1, float32_refine=2, batch_layout=1), "INTERLEAVED"),
                                       (dict(float32_general=1, refine_rows=3), "refine_rows")])
def test_plan_create_refusals(built, opt, word):
    hipldl, syn = _mods()
    with pytest.raises(hipldl.CnlError) as e:
        _plan(hipldl, syn.dense_structure(6, 9), **opt)
    assert e.value.code == CNL_ERR_ARG and word in str(e.value), str(e.value)


def test_symbols_and_version(built):
    hipldl, _ = _mods()
    hdr = open(os.path.join(ROOT, "include", "cannoles_hip.h")).read()
    for sym in ("cnl_kkt_residual_dev", "cnl_get_refine_norms"):
        assert hasattr(hipldl.lib(), sym), sym
        assert f"int {sym}(" in hdr, sym
        assert sym in hipldl.ABI_SYMBOLS, sym
    assert hipldl.lib().cnl_version() >= 500


def _structures(syn):
    return [syn.random_structure(60, 80, 4, 0.1, 1), syn.dense_structure(40, 70), syn.model_band_structure(30, 3), syn.band_structure(30, 3, hw=3)]


@pytest.mark.parametrize("which", range(4))
def test_row_lists_apply_as_the_dense_matrix(built, which):
    hipldl, syn = _mods()
    s = _structures(syn)[which]
    pl = _plan(hipldl, s, plan_kind=hipldl.PLAN_THROUGHPUT)
    ptr, slot, col = (pl.array("kkt_row_" + k).astype(np.int64) for k in ("ptr", "slot", "col"))
    rows, cols = s.kkt_pattern()
    assert len(ptr) == s.N + 1 and ptr[0] == 0 and ptr[-1] == len(slot) == len(col)
    # each slot once if diagonal, twice if strictly lower; slots ascend within a row; the pairs are the entry and its mirror
    want = np.where(rows == cols, 1, 2)
    assert np.array_equal(np.bincount(slot, minlength=len(rows)), want)
    rowof = np.repeat(np.arange(s.N), np.diff(ptr))
    for i in range(s.N):
        assert (np.diff(slot[ptr[i]:ptr[i + 1]]) > 0).all(), i
    r0, c0 = rows[slot] - 1, cols[slot] - 1
    assert (((rowof == r0) & (col == c0)) | ((rowof == c0) & (col == r0))).all()
    assert int(np.diff(ptr).max()) == RF.max_row_entries(s)
    if which == 2:
        assert len(set(zip(rows.tolist(), cols.tolist()))) < len(rows)   # duplicates are exercised
    rng = np.random.default_rng(which)
    vals, d = rng.normal(size=s.nnzNS), rng.normal(size=s.N)
    got = np.zeros(s.N)
    np.add.at(got, rowof, vals[slot] * d[col])
    K = syn.dense_kkt(s, vals)
    m = RF.max_row_entries(s)
    assert (np.abs(got - K @ d) <= (m + 2) * RF.EPS64 * (np.abs(K) @ np.abs(d))).all()


@pytest.mark.parametrize("name", RF.INPUT_NAMES)
def test_model_meets_the_bounds(built, name):
    """the unpivoted float32 LDL' with a float64 residual, k = 2: both bounds, and a contraction above 1000 per step, for every
    positive-definite input the GPU tests name"""
    _, syn = _mods()
    s, vals, rhs = RF.inputs(syn, name)
    for b in range(vals.shape[0]):
        d, norms = RF.refine_model(s, vals[b], rhs[b], 2)
        RF.check_bounds(s, vals[b], rhs[b], d, f"{name}[{b}]")
        assert norms[1] < norms[0] / RF.CONTRACTION, (name, b, norms)


def test_model_on_the_ladder_input(built):
    """the mixed batch through the fp64 oracle on the demoted data (tests/support/f32_general.py: no pivot near eig_tol): problem 5
    climbs, problem 6 fails below RHO_MAX_SMALL, the others need no rho; the model meets the bounds at the rho problem 5 reaches"""
    hipldl, syn = _mods()
    from oracle import oracle as O
    from tests.support import f32_general as G
    s, vals, rhs = RF.mixed_ladder_inputs(syn)
    _, p32 = RF.demoted_params(hipldl, RF.RHO_MAX_SMALL)
    ref = G.oracle_newton(O, s, vals.astype(np.float32), rhs.astype(np.float32), np.zeros(len(vals), np.float32), p32)
    assert not ref["ok"][RF.FAILS] and ref["ok"][RF.CLIMBS] and ref["nf"][RF.CLIMBS] > 1 and 0 < ref["rho"][RF.CLIMBS] <= RF.RHO_MAX_SMALL
    assert np.delete(ref["ok"], RF.FAILS).all() and (np.delete(ref["nf"], [RF.FAILS, RF.CLIMBS]) == 1).all()
    v = vals[RF.CLIMBS].copy()
    v[-s.nvar:] = np.float64(np.float32(ref["rho"][RF.CLIMBS]))
    d, norms = RF.refine_model(s, v, rhs[RF.CLIMBS], 2)
    RF.check_bounds(s, v, rhs[RF.CLIMBS], d, "mixed[5]")
    assert norms[1] < norms[0] / RF.CONTRACTION, norms
