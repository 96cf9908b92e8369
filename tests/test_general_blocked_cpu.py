"""The blocked general kernel (tuning general_blocked), without a GPU: the option's rules, the front tables the GPU tests rely on,
the blocked elimination restated in numpy against the pivot-by-pivot loop of tests/support/plan_sim.py, and what vouches for the
inputs of tests/test_general_blocked_gpu.py (the oracle's decisions on the canonical order and on the plan's own)."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl
from tests.support import dense_general_cases as GC
from tests.support import general_blocked_cases as GB

CNL_ERR_ARG = 1
L_TOL = 1e-12      # blocked against rank-1 on one front, relative to the front's largest entry


@pytest.fixture(scope="module")
def oracle_mod(built):
    from oracle import oracle as O
    O.build()
    return O


def _plan_rc(s, **opt):
    """(code, message) of cnl_plan_create_ex at batch 7 under the given options"""
    rows, cols = s.kkt_pattern()
    try:
        hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=7, options=hipldl.Options(**opt))
    except hipldl.CnlError as e:
        return e.code, str(e)
    return 0, ""


# ---- 1. option rules ----
def test_option_rules(built):
    assert hipldl.lib().cnl_version() >= 504
    s = GB.structure(GB.random_shape(33))
    assert _plan_rc(s, **GB.OPTS)[0] == 0
    assert _plan_rc(s, **dict(GB.OPTS, general_blocked=0))[0] == 0
    for bad in (2, -1):
        rc, msg = _plan_rc(s, **dict(GB.OPTS, general_blocked=bad))
        assert rc == CNL_ERR_ARG and "general_blocked" in msg, (rc, msg)
    # a refined handle's plan is its inner Float32 handle's: refused with the key, made without it
    assert _plan_rc(s, float32_general=1, float32_refine=1)[0] == 0
    rc, msg = _plan_rc(s, float32_general=1, float32_refine=1, general_blocked=1)
    assert rc == CNL_ERR_ARG and "general_blocked" in msg and "Float64" in msg, (rc, msg)


def test_float32_creators_refuse_the_key_before_they_look_for_a_device(built):
    """cnl_create_f32_ex and cnl_create_ex with float32_refine answer CNL_ERR_ARG about the key whether or not a device is there:
    the option checks come first."""
    s = GB.structure(GB.random_shape(33))
    rows, cols = s.kkt_pattern()
    for dtype, opt in ((np.float32, dict(float32_general=1, general_blocked=1)),
                       (np.float32, dict(general_blocked=1)),
                       (np.float64, dict(float32_general=1, float32_refine=1, general_blocked=1))):
        with pytest.raises(hipldl.CnlError) as e:
            hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=7, dtype=dtype, options=hipldl.Options(**opt))
        assert e.value.code == CNL_ERR_ARG and "general_blocked" in str(e.value), str(e.value)


# ---- 2. front tables ----
@pytest.mark.parametrize("shape,extra,want", GB.FRONT_TABLE, ids=[GB.shape_id(sh) + ("-condense0" if ex else "") for sh, ex, _ in GB.FRONT_TABLE])
def test_front_tables(built, shape, extra, want):
    s, P = GB.make_plan(shape, **extra)
    fr = GB.fronts_of(P)
    if shape in [GB.random_shape(n) for n in GB.RANDOM_N]:
        assert len(fr) == 1 and fr[0][:2] == want[0][:2] and P.info["fmax"] == shape[0] + 1, fr
    else:
        for w in want:
            assert w in fr, (w, fr)
    if shape == GB.GRID:
        assert P.info["fmax"] == 95 and s.nvar == 1024
    if shape == GB.G450:
        assert fr[-2:] == want
    assert max(f[0] for f in fr) >= GB.PANEL


def test_grid_structure_is_the_five_point_family(built):
    """J_F: one row per grid point on the point and its neighbours, row-major; H_F: every pair of a stencil once, lower triangle;
    the plan figures of the three grids the measurements use."""
    from cannoles_jl_amd import synthetic as syn
    s = syn.grid_structure(5, p=2)
    assert (s.nvar, s.nequ, s.ncon) == (25, 25, 2)
    jr, jc = np.asarray(s.jF[0]) - 1, np.asarray(s.jF[1]) - 1
    assert (np.diff(jr) >= 0).all() and len(jr) == 5 * 25 - 4 * 5
    assert sorted(jc[jr == 12]) == [7, 11, 12, 13, 17] and sorted(jc[jr == 0]) == [0, 1, 5]
    hr, hc = np.asarray(s.hF[0]) - 1, np.asarray(s.hF[1]) - 1
    assert (hr >= hc).all() and len(set(zip(hr, hc))) == len(hr)
    A = np.zeros((25, 25), bool)
    A[jr, jc] = True
    assert set(zip(hr, hc)) == set(zip(*np.nonzero(np.tril((A.T.astype(int) @ A.astype(int)) > 0))))
    assert sorted(np.asarray(s.jc[1])[np.asarray(s.jc[0]) == 2] - 1) == list(range(10, 15))
    v, r = syn.random_values(s, 3)
    assert len(v) == s.nnzNS and len(r) == s.N
    for G, n, fmax, nfronts in ((24, 576, 71, 101), (48, 2304, 143, 340)):
        s, P = GB.make_plan(("grid", G))
        assert (s.nvar, P.info["fmax"], len(GB.fronts_of(P))) == (n, fmax, nfronts)


# ---- 3. the algorithm ----
ALGO = [(sh, ex) for sh, ex, _ in GB.FRONT_TABLE]


@pytest.mark.parametrize("shape,extra", ALGO, ids=[GB.shape_id(sh) + ("-condense0" if ex else "") for sh, ex in ALGO])
def test_blocked_elimination_against_rank1(built, shape, extra):
    """On every front of the plan, with the mix's values as given (the first attempt) and, for the climbers, at rho = 605.5 (about
    where their ladder ends: the variable block is positive definite there): the blocked elimination and the rank-1 loop, from
    the same assembled front, give the same npos / nzer and the same front — L panel and update matrix — to L_TOL of the front's
    largest entry; the whole factor of the blocked walk agrees with PlanSim.factor's likewise.  (The failing rungs in between are
    unpivoted factorisations of indefinite matrices with element growth of 10 .. 100 and more: any two summation orders differ by
    growth x eps there, and nothing reads those factors.)"""
    s, P = GB.make_plan(shape, **extra)
    sim = GB.BlockedSim(P)
    B = 4 if shape in (GB.GRID, GB.G450) else GC.MIX       # (kinds 0 .. 3: healthy, NaN, the two climbers)
    vals, rhs, _ = GC.values(s, B)
    eig_tol = hipldl.default_params()[0]
    worst, nblocked = 0.0, 0

    def on_front(k, before, after, cnt):
        nonlocal worst, nblocked
        npiv, nupd, indep = int(sim.fr["npiv"][k]), int(sim.fr["nupd"][k]), int(sim.fr["indep"][k])
        if npiv < GB.PANEL:
            return
        nblocked += 1
        ref = before.copy()
        cnt1 = GB.eliminate_rank1(ref, 1 + nupd + npiv, nupd, indep, eig_tol)
        if np.isnan(before).any():
            assert np.isnan(after).any() and cnt[0] < npiv and cnt1[0] < npiv
            return
        assert cnt == cnt1, (k, cnt, cnt1)
        err = np.abs(after - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err <= L_TOL, (k, npiv, nupd, indep, err)

    for b in range(B):
        for rho in (None,) if b % GC.MIX in (0, 1, 4, 5) else (None, 605.5):
            v, r = sim.inner_inputs(vals[b], rhs[b])
            Lb, npos, nzer = sim.factor_with(v, r, s.nvar, eig_tol, rho, blocked=True, on_front=on_front)
            L1, npos1, nzer1 = sim.factor(v, r, s.nvar, eig_tol, rho)
            if b % GC.MIX == 1:
                assert npos != s.nvar and npos1 != s.nvar
                continue
            assert (npos, nzer) == (npos1, nzer1)
            live = ~np.isnan(L1)
            assert np.array_equal(live, ~np.isnan(Lb))
            assert np.abs(Lb[live] - L1[live]).max() <= L_TOL * np.abs(L1[live]).max()
    assert nblocked > 0
    print(f"{GB.shape_id(shape)}: {nblocked} blocked fronts, worst front difference {worst:.2e}")


def test_narrow_and_independent_panels_in_isolation():
    """random symmetric fronts at the panel edges: npiv = 16 k - 1, 16 k, 16 k + 1, with and without update rows, with independent
    leading pivots up to all of them; the blocked result is the rank-1 result"""
    rng = np.random.default_rng(7)
    for npiv in (15, 16, 17, 31, 32, 33, 48):
        for nupd in (0, 5, 40):
            for indep in sorted({0, 1, 15, 16, 17, npiv} & set(range(npiv + 1))):
                f = 1 + nupd + npiv
                idep = f - indep
                A = rng.uniform(-1, 1, (f, f))
                A = A + A.T + np.diag(rng.choice([-1.0, 1.0], f) * (f + rng.uniform(0, 1, f)))
                A[idep:, idep:] = np.diag(np.diag(A)[idep:])      # independent pivots: no entries between them
                ti, tj = np.tril_indices(f)
                F0 = A[ti, tj]
                Fb, F1 = F0.copy(), F0.copy()
                cb = GB.eliminate_blocked(Fb, f, nupd, indep, 1e-12)
                c1 = GB.eliminate_rank1(F1, f, nupd, indep, 1e-12)
                assert cb == c1 and cb[0] + cb[1] <= npiv
                assert np.abs(Fb - F1).max() <= L_TOL * np.abs(F1).max(), (npiv, nupd, indep)


# ---- 4. decisions ----
DECISIONS = [(GB.random_shape(n), {}) for n in GB.RANDOM_N] + [(GB.COND0, {}), (GB.COND0, dict(condense=0)), (GB.GRID, {}), (GB.GRID, dict(condense=0)),
                                                                (GB.GRID48, {}), (GB.F130, {}), (GB.G125, {}), (GB.G450, {}), (GC.SECOND, {}), (GC.SMALLEST, {})]


@pytest.mark.parametrize("shape,extra", DECISIONS, ids=[GB.shape_id(sh) + ("-condense0" if ex else "") for sh, ex in DECISIONS])
def test_decisions_on_both_orders(oracle_mod, shape, extra):
    """The oracle decides the mix the same way on the canonical order and on the plan's own, as WANT_OK / WANT_NF say, and the
    eigenvalues of the condensed matrix vouch for every rung of kinds 5 and 6 — except n = 16, where kind 5 fails in the oracle
    too: the GPU test uses kinds 0 .. 4 there."""
    kinds = range(5) if shape == GB.random_shape(16) else range(GC.MIX)
    c = GB.case(shape, kinds=kinds)
    s, P = GB.make_plan(shape, **extra)
    own = GC.oracle_on(P.array("perm").astype(np.int64), c)
    want_ok, want_nf = [GC.WANT_OK[k] for k in kinds], [GC.WANT_NF[k] for k in kinds]
    for ref in (c, own):
        assert list(ref["ok"]) == want_ok and list(ref["nf"]) == want_nf, (ref["ok"], ref["nf"])
        assert np.array_equal(GC.bits64(ref["rho"]), GC.bits64(c["rho"])) and np.array_equal(GC.bits64(ref["ro"]), GC.bits64(c["ro"]))
    if shape == GB.random_shape(16):
        full = GB.case(shape)
        assert not full["ok"][5]
    for k, kind in enumerate(kinds):
        if kind in (5, 6):
            for rho, determined, rel, how in GC.rung_verdicts(c, k):
                assert determined, (kind, rho, rel, how)
