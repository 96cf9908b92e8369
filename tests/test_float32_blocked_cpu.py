"""The blocked general kernel in float (tuning float32_blocked), without a GPU: the key's rules, the plan facts the GPU tests rely
on for the Float32 plans cnl_create_f32_ex builds, the blocked elimination restated in numpy.float32 with the lane maps of
v_mfma_f32_16x16x4_f32 against the pivot-by-pivot loop in float64, and what vouches for the inputs of
tests/test_float32_blocked_gpu.py: every decision of every rung of every case it uses has the project's margin in float."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl
from tests.support import dense_cases as dc
from tests.support import f32_blocked_cases as FB
from tests.support import general_blocked_cases as GB

CNL_ERR_ARG = 1
# Blocked elimination in float32 against the rank-1 loop in float64, one front of order f, relative to the largest entry the
# elimination meets (the assembled front or the result, whichever is larger).  An entry receives at most f updates, each a product
# and a sum rounded once (unit roundoff eps32 / 2 each): to first order f eps32 times the largest partial sum, which these
# fronts — quasi-definite, or positive definite at the ladder's last rung — keep at the size of the largest entry.  So the bar is
# 1.0 eps32 f max|F|, the first-order worst case without growth.  Measured on every front of the plans below and on the isolated
# fronts (printed by the tests): worst 0.095 on the plans, 0.118 on the isolated fronts — a margin of 8 to the bar; the f64 result map
# misses it by a factor of 400 to 2 000 (test_the_f64_result_map_fails).
L_FACTOR = 1.0


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
    s = FB.structure(FB.random_shape(33))
    f32, f64 = np.float32, np.float64
    # (a) accepted with float32_general: the plan is made; the creator gets past the option checks (with no device it then says so)
    assert _plan_rc(s, float32_general=1, float32_blocked=1)[0] == 0
    for extra in ({}, dict(float32_condense=1), dict(float32_blocked=0)):
        rc, msg = _create_rc(s, f32, **dict(dict(float32_general=1, float32_blocked=1), **extra))
        assert rc != CNL_ERR_ARG and "float32_blocked" not in msg, (rc, msg)
        assert rc == 0 or "no HIP device" in msg, (rc, msg)
    # (b) refused alone
    rc, msg = _create_rc(s, f32, float32_blocked=1)
    assert rc == CNL_ERR_ARG and "float32_blocked" in msg and "float32_general" in msg, (rc, msg)
    # (c) refused at another value
    for bad in (2, -1):
        rc, msg = _create_rc(s, f32, float32_general=1, float32_blocked=bad)
        assert rc == CNL_ERR_ARG and "float32_blocked" in msg, (rc, msg)
    # (d) refused with float32_refine, at plan and at handle creation; both are made without the key
    assert _plan_rc(s, float32_general=1, float32_refine=1)[0] == 0
    for rc, msg in (_plan_rc(s, float32_general=1, float32_refine=1, float32_blocked=1),
                    _create_rc(s, f64, float32_general=1, float32_refine=1, float32_blocked=1)):
        assert rc == CNL_ERR_ARG and "float32_blocked" in msg and "float32_refine" in msg, (rc, msg)
    # (e) general_blocked at the Float32 creators is still refused, with or without the new key
    for dtype, opt in ((f32, dict(float32_general=1, general_blocked=1)), (f32, dict(float32_general=1, general_blocked=1, float32_blocked=1)),
                       (f64, dict(float32_general=1, float32_refine=1, general_blocked=1))):
        rc, msg = _create_rc(s, dtype, **opt)
        assert rc == CNL_ERR_ARG and "general_blocked" in msg, (rc, msg)
    # a Float64 creator without float32_refine reads nothing of the key, as of float32_condense: neither rule nor value
    for opt in (dict(float32_blocked=1), dict(float32_blocked=2), dict(float32_condense=1)):
        assert _plan_rc(s, **opt)[0] == 0
        rc, msg = _create_rc(s, f64, **opt)
        assert rc != CNL_ERR_ARG and (rc == 0 or "no HIP device" in msg), (rc, msg)
    # (f)
    assert hipldl.lib().cnl_version() >= 505


# ---- 2. plan facts ----
def _pid(v):
    return FB.shape_id(v[0]) + ("-condensed" if "float32_condense" in v[1] else "-uncondensed")


@pytest.mark.parametrize("shape,hopt,popt", FB.GPU_CASES, ids=[_pid(v) for v in FB.GPU_CASES])
def test_float32_plan_facts(built, shape, hopt, popt):
    """The Float32 plan of every handle the GPU tests make: the fronts of GB.FRONT_TABLE, the largest front, and the threads per
    problem choose_config takes from it (64 up to order 96, else 256)."""
    cond = "float32_condense" in hopt
    s, P = FB.make_plan(shape, popt)
    fr = GB.fronts_of(P)
    fmax = P.info["fmax"]
    assert fmax == FB.FMAX[FB.shape_id(shape), cond] == max(1 + f[0] + f[1] for f in fr), (fmax, fr)
    assert (P.info["ncond"] > 0) == cond
    for sh, extra, want in GB.FRONT_TABLE:
        if sh == shape and (not extra) == cond:
            if len(fr) == 1:
                assert fr[0][:2] == want[0][:2], (fr, want)      # (one front of n pivots; FRONT_TABLE leaves its indep open)
            else:
                for w in want:
                    assert w in fr or w[0] < FB.PANEL, (w, fr)
    if shape == FB.COND0:
        assert fr[-1] == (60, 0, 23)
    if shape == FB.G450:
        assert fr[-2:] == [(19, 355, 0), (356, 0, 0)]
    if shape == FB.GRID and not cond:
        assert (16, 13, 11) in fr
    assert max(f[0] for f in fr) >= FB.PANEL
    # 64 threads per problem by default up to order 96: only these shapes run a blocked instance without v1_tpp
    assert (fmax > 96) == (shape in (FB.F97, FB.F130, FB.G450))


# ---- 3. the algorithm ----
def _front_ratio(before32, f, nupd, indep, eig_tol, row=FB.row_f32):
    """(ratio of the largest difference to eps32 f max|F|, counts agree) of the float32 blocked elimination against rank-1 in float64"""
    ref = before32.astype(np.float64)
    c1 = GB.eliminate_rank1(ref, f, nupd, indep, float(np.float32(eig_tol)))
    Fb, npos, nzer = FB.eliminate_blocked_f32(before32.copy(), f, nupd, indep, eig_tol, row)
    scale = max(np.abs(ref).max(), np.abs(before32).max())
    return np.abs(Fb.astype(np.float64) - ref).max() / (FB.EPS32 * f * scale), (npos, nzer) == c1


ALGO = [v for v in FB.GPU_CASES if v[0] != FB.F96]


@pytest.mark.parametrize("shape,hopt,popt", ALGO, ids=[_pid(v) for v in ALGO])
def test_blocked_elimination_f32_against_rank1(built, shape, hopt, popt):
    """On every front with 16 pivots or more of the plan, as the float64 walk over the plan assembles it (rounded to float32): the
    healthy problem as given and the first climber at the rho its ladder ends on (failing rungs are unpivoted factorisations of
    indefinite matrices: growth times eps, and nothing reads those factors).  Counts equal, fronts within L_FACTOR eps32 f max|F|."""
    s, P = FB.make_plan(shape, popt)
    sim = GB.BlockedSim(P)
    c = FB.case(shape)
    eig_tol = float(c["p32"][0])
    worst, nblocked = 0.0, 0

    def on_front(k, before, after, cnt):
        nonlocal worst, nblocked
        npiv, nupd, indep = int(sim.fr["npiv"][k]), int(sim.fr["nupd"][k]), int(sim.fr["indep"][k])
        if npiv < FB.PANEL:
            return
        nblocked += 1
        f = 1 + nupd + npiv
        ratio, same = _front_ratio(before.astype(np.float32), f, nupd, indep, eig_tol)
        assert same, (k, npiv, nupd, indep)
        worst = max(worst, ratio)
        assert ratio <= L_FACTOR, (k, npiv, nupd, indep, ratio)

    for b, rho in ((0, None), (2, float(c["rho"][2]))):
        v, r = sim.inner_inputs(c["vals"][b].astype(np.float64), c["rhs"][b].astype(np.float64))
        _, npos, nzer = sim.factor_with(v, r, s.nvar, eig_tol, rho, blocked=False, on_front=on_front)
    assert nblocked > 0
    print(f"{_pid((shape, hopt))}: {nblocked} blocked fronts, worst difference {worst:.3f} eps32 f max|F|")


def _isolated(rng, npiv, nupd, indep):
    f = 1 + nupd + npiv
    idep = f - indep
    A = rng.uniform(-1, 1, (f, f))
    A = A + A.T + np.diag(rng.choice([-1.0, 1.0], f) * (f + rng.uniform(0, 1, f)))
    A[idep:, idep:] = np.diag(np.diag(A)[idep:])      # independent pivots: no entries between them
    ti, tj = np.tril_indices(f)
    return A[ti, tj].astype(np.float32), f


def test_narrow_and_independent_panels_in_isolation_f32():
    """random symmetric fronts at the panel edges: npiv = 16 k - 1, 16 k, 16 k + 1, with and without update rows, 0 .. all pivots
    independent"""
    rng = np.random.default_rng(7)
    worst = 0.0
    for npiv in (15, 16, 17, 31, 32, 33, 47, 48, 49):
        for nupd in (0, 5, 40):
            for indep in sorted({0, 1, 15, 16, 17, npiv} & set(range(npiv + 1))):
                F0, f = _isolated(rng, npiv, nupd, indep)
                ratio, same = _front_ratio(F0, f, nupd, indep, 1e-6)
                assert same and ratio <= L_FACTOR, (npiv, nupd, indep, ratio, same)
                worst = max(worst, ratio)
    print(f"isolated fronts: worst difference {worst:.3f} eps32 f max|F|")


def test_the_f64_result_map_fails():
    """the accumulator loaded and stored by the f64 instruction's result map (row lg + 4 r) — what copying the double code gives —
    is a wrong factor by orders of magnitude more than the bar, on a front with one panel and one tile already"""
    rng = np.random.default_rng(7)
    for npiv, nupd, indep in ((16, 5, 0), (33, 40, 0), (32, 0, 16)):
        F0, f = _isolated(rng, npiv, nupd, indep)
        good, _ = _front_ratio(F0, f, nupd, indep, 1e-6)
        bad, _ = _front_ratio(F0, f, nupd, indep, 1e-6, row=FB.row_f64)
        print(f"npiv {npiv} nupd {nupd} indep {indep}: f32 map {good:.3f}, f64 map {bad:.3g} eps32 f max|F|")
        assert good <= L_FACTOR < 100 * L_FACTOR < bad


# ---- 4. pivot margins ----
MARGIN_CASES = sorted({(v[0], B) for v in FB.GPU_CASES for B in ((FB.MIX, 65) if v[0] == FB.random_shape(33) else (FB.MIX,))}, key=str)


@pytest.mark.parametrize("shape,B", MARGIN_CASES, ids=[f"{FB.shape_id(sh)}-B{B}" for sh, B in MARGIN_CASES])
def test_pivot_margins(oracle_mod, shape, B):
    """Every decision of every rung of every problem the GPU tests run (the mix, and the 65 problems of the batch test): the Schur
    complement onto the variables has its smallest eigenvalue at least MARGIN of the largest away from zero, with the sign the
    decision needs; the oracle's pattern is that of the mix."""
    c = FB.case(shape, B)
    assert list(c["ok"]) == [FB.WANT_OK[b % 5] for b in range(B)], c["ok"]
    assert [int(x) for x in c["nf"][:FB.MIX]] == FB.WANT_NF
    p = c["p32"].astype(np.float64)
    worst = np.inf
    for b in range(B):
        if b % 5 == 1:
            assert np.isnan(c["vals"][b]).any()
            continue
        assert c["rho"][b] == dc.rungs(float(c["rho_old"][b]), int(c["nf"][b]), p)[-1]
        for rho, rel, succeeds in FB.eig_margins(c, b):
            assert (rel >= FB.MARGIN) if succeeds else (rel <= -FB.MARGIN), (b, rho, rel, succeeds)
            worst = min(worst, abs(rel))
    print(f"{FB.shape_id(shape)} x {B}: smallest |lambda_min| / lambda_max over all rungs {worst:.3g}")
