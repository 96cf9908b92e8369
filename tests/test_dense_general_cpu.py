"""The general form of the dense backend in double (Route::GeneralDense), without a GPU: the plan facts that decide the route for every
shape of tests/support/dense_general_cases.py, and what vouches for every input of tests/test_dense_general_gpu.py, so that the GPU
file skips and reclassifies nothing —
  * the oracle's decision table of the seven-kind mix, exactly;
  * for kinds 0, 2, 3 and 4 every rung refactorised by the oracle with min|D| > NOISE max|D| (the rule of
    tests/test_dense_cases_cpu.py);
  * for kinds 5 and 6 (a positive residual pivot, counted outside the dense factor) every rung's decision determined by the
    eigenvalues of the condensed matrix K_kk - K_kr D_r^-1 K_rk in numpy (dense_general_cases.rung_verdict);
  * the same for the inputs of the prefer_dense test and of the route table, Float32 roundings included."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl
from tests.support import dense_cases as dc
from tests.support import dense_general_cases as GC
from tests.support import f32_general_dense as GD32
from tests.test_dense_cases_cpu import NOISE, _rung_margins


@pytest.fixture(scope="module")
def oracle_mod(built):
    from oracle import oracle as O
    O.build()
    return O


def test_shapes_are_the_float_tables_and_one_more():
    assert list(GC.SHAPES)[:-1] == list(GD32.SHAPES) and list(GC.SHAPES)[-1] == GC.BIG == (800, 900, 0, 0.05, 1)
    assert GC.SMALLEST == GD32.SMALLEST and GC.SECOND in GC.SHAPES and GC.MIX == 7
    assert GC.EIG_MARGIN == 1e-6 and GC.EIG_MARGIN32 == GD32.EIG_MARGIN == 1e-3
    assert NOISE == 4096.0 * np.finfo(float).eps


@pytest.mark.parametrize("shape", list(GC.SHAPES), ids=GC.shape_id)
def test_plan_facts(built, shape):
    """Under default options, at the batches the GPU tests create (1, 7, 14, 256): the condensed order and the largest front agree
    with the shared table, the order is within 96 .. 4096, a front exceeds 64 and there is no register-front plan — what puts a
    default Float64 handle on the route.  The 800 shape has more condensed slots than one trip of dn_scatter_general's loop covers:
    the PLAN's own count (the condensed buffer holds [slots | nvar rho | order rhs] sums, so c_ptr has slots + nvar + order + 1
    entries), which the numpy count of the lower triangle of pattern(K_kk) + pattern(J'J) confirms."""
    s = GC.structure(shape)
    rows, cols = s.kkt_pattern()
    for B in (1, 7, 14, 256):
        P = hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=B)
        info = P.info
        order, fmax = s.N - info["ncond"], info["fmax"]
        assert order == s.nvar + s.ncon == GC.SHAPES[shape][0]
        if shape in GD32.SHAPES:
            assert (order, fmax) == GD32.SHAPES[shape]
        assert 96 <= order <= 4096 and fmax > 64 and info["v2"] is None
        slots = len(P.array("c_ptr")) - 1 - s.nvar - order
        assert slots == GC.condensed_slots(s)
        if shape == GC.BIG:
            assert slots == 292243 > GC.SCATTER_TRIP and order <= 800
    print(f"{GC.shape_id(shape)}: order {order}, largest front {fmax}, {slots} condensed slots")


@pytest.mark.parametrize("shape", list(GC.SHAPES), ids=GC.shape_id)
def test_decisions_and_margins(oracle_mod, shape):
    """ok = [1, 0, 1, 1, 1, 1, 0], nfact = [1, 20, 6, 4, 1, 1, 20] on every shape (B = 7, and B = 14 on the smallest, where the GPU
    tests use two mixes); rho as dc.rungs replays it, the rho slots of vals as the ladder leaves them; then the margins."""
    O = oracle_mod
    params = O.default_params()
    worst_d, worst_e, by_count = np.inf, np.inf, 0
    for B in (GC.MIX, 2 * GC.MIX) if shape == GC.SMALLEST else (GC.MIX,):
        c = GC.case(shape, B)
        s, reps = c["s"], B // GC.MIX
        n = s.nvar
        assert list(c["ok"]) == GC.WANT_OK * reps and list(c["nf"]) == GC.WANT_NF * reps, (c["ok"], c["nf"])
        for b in range(B):
            kind = b % GC.MIX
            rr = dc.rungs(float(c["rho_old"][b]), int(c["nf"][b]), params)
            assert len(rr) == c["nf"][b] and c["rho"][b] == (params[4] * rr[-1] if kind in (1, 6) else rr[-1])
            if kind in (0, 4, 5):
                assert c["rho"][b] == 0.0 and c["ro"][b] == 0.0 and (c["vals_after"][b, -n:] == 0.0).all()
            elif kind in (1, 6):     # the ladder runs out (the rho returned is the first above rhomax): rho_old stays, the slots hold the last rho tried
                assert c["rho"][b] > params[6] and c["ro"][b] == 0.0 and (c["vals_after"][b, -n:] == rr[-1]).all()
            else:
                assert c["ro"][b] == c["rho"][b] == rr[-1] and (c["vals_after"][b, -n:] == rr[-1]).all()
            assert np.array_equal(c["vals_after"][b, :-n], c["vals"][b, :-n], equal_nan=True)
        assert abs(c["rho"][2] - 605.545) < 1e-3 and abs(c["rho"][3] - 128.0 / 3.0) < 1e-12
        orc = O.Oracle(s.N, c["rows"], c["cols"], O.canonical_perm(s.nvar, s.nequ, s.ncon))
        plain = [b for b in range(B) if b % GC.MIX in (0, 2, 3, 4)]
        worst_d = min(worst_d, _rung_margins(O, orc, s, c["vals"], c["rho_old"], c["nf"], c["rho"], params, plain))
        for b in [b for b in range(B) if b % GC.MIX in (5, 6)]:
            lam, dr = GC.condensed_eigs(s, c["vals"][b], 0.0)
            assert int((dr > 0).sum()) == 1
            if b % GC.MIX == 5:
                assert int((lam > 0).sum()) == n - 1      # the call succeeds only with the positive pivot counted outside
            for rho, determined, rel, how in GC.rung_verdicts(c, b):
                assert determined, (b, rho, rel, how)
                by_count += how == "count"
                if how == "all":
                    worst_e = min(worst_e, rel)
            # the inertia the two-call test compares with numpy's: no eigenvalue of K near zero
            npos, nzero, rel = GC.numpy_inertia(c, b)
            assert nzero == 0 and rel >= GC.EIG_MARGIN and (npos == n if b % GC.MIX == 5 else npos != n), (b, npos, nzero, rel)
            ref = orc.try_to_factorize(np.array(c["vals"][b]), s.nvar, s.nequ, s.ncon, params[0], return_inertia=True)
            assert ref == (b % GC.MIX == 5, npos, 0)
    print(f"{GC.shape_id(shape)}: kinds 0 2 3 4 min|D| / max|D| >= {worst_d:.2e}; kinds 5 6 smallest relative |eigenvalue| of a rung decided "
          f"by all eigenvalues {worst_e:.2e}, {by_count} failing rungs decided by the count of nvar eigenvalues above the margin")


def test_repeated_call_inputs(oracle_mod):
    """the eight problems the 256-problem test repeats: healthy (nfact 1), pivots far above the noise"""
    O = oracle_mod
    c = GC.healthy_case((129, 150, 0, 0.06, 5))
    s = c["s"]
    assert len(c["vals"]) == 8 and c["ok"].all() and (c["nf"] == 1).all() and not c["rho"].any()
    orc = O.Oracle(s.N, c["rows"], c["cols"], O.canonical_perm(s.nvar, s.nequ, s.ncon))
    worst = _rung_margins(O, orc, s, c["vals"], c["rho_old"], c["nf"], c["rho"], O.default_params(), range(8))
    print(f"eight healthy problems of order 129: min|D| / max|D| >= {worst:.2e}")


def test_prefer_dense_pattern(oracle_mod):
    """The pattern of the 16 / 17 test: a latency plan (batches 16 and 17 get the same one) whose register-front records hold a
    front of the 64 class on a condensed system of order 96 .. 512 — capi_plan.cpp's prefer_dense; kinds 0, 2 and 5 decide as the
    table says, with the margins above."""
    O = oracle_mod
    c = GC.prefer_case()
    s = c["s"]
    assert (s.nvar, s.nequ, s.ncon) == (135, 154, 2)
    infos = [hipldl.Plan(s.N, c["rows"], c["cols"], s.nvar, s.nequ, s.ncon, batch=B).info for B in (16, 17)]
    assert infos[0] == infos[1]
    info = infos[0]
    assert info["v2"] is not None and info["v2"]["fronts64"] > 0 and 32 < info["fmax"] <= 64
    assert s.N - info["ncond"] == 137 and 96 <= 137 <= 512
    assert list(c["kinds"]) == [0, 2, 5] and list(c["ok"]) == [True, True, True] and list(c["nf"]) == [1, 6, 1]
    params = O.default_params()
    orc = O.Oracle(s.N, c["rows"], c["cols"], O.canonical_perm(s.nvar, s.nequ, s.ncon))
    worst = _rung_margins(O, orc, s, c["vals"], c["rho_old"], c["nf"], c["rho"], params, [0, 1])
    (rho, determined, rel, how), = GC.rung_verdicts(c, 2)
    assert determined and how == "all"
    print(f"prefer_dense pattern: min|D| / max|D| >= {worst:.2e}, kind 5 smallest relative |eigenvalue| {rel:.2e}")


@pytest.mark.parametrize("route", list(GC.ROUTES))
def test_route_table_inputs(oracle_mod, route):
    """Kinds 0, 5 and 6 on the pattern of every row of the route table, in the row's element type (Float32: inputs rounded, the
    oracle on the widened data with ParamCaNNOLeS(Float32) widened; margin 1e-3, the Float32 tests' own): ok = [1, 1, 0], nfact
    = [1, 1, 20] (10 in Float32), every rung of kinds 5 and 6 determined, the healthy problem far above the noise, and an inertia
    for numpy to state.  Every pattern passes with the pivot off[4] + m // 2 and the seeds 40 + kind: nothing else was picked."""
    O = oracle_mod
    T, opt, pattern = GC.ROUTES[route]
    f32 = np.dtype(T) == np.float32
    c = GC.route_case(pattern, T)
    s = c["s"]
    margin = GC.EIG_MARGIN32 if f32 else GC.EIG_MARGIN
    assert c["vals"].dtype == np.dtype(T) and list(c["kinds"]) == [0, 5, 6]
    assert list(c["ok"]) == [True, True, False] and list(c["nf"]) == [1, 1, 10 if f32 else 20], (c["ok"], c["nf"])
    p = np.array(c["params"], np.float64)
    orc = O.Oracle(s.N, c["rows"], c["cols"], O.canonical_perm(s.nvar, s.nequ, s.ncon))
    assert orc.try_to_factorize(np.array(c["vals"][0], np.float64), s.nvar, s.nequ, s.ncon, p[0])
    D = np.abs(orc.D)
    assert D.min() > (margin if f32 else NOISE) * D.max()
    worst = np.inf
    for b in (1, 2):
        assert int((np.array(c["vals"][b, s.offsets()[4]:s.offsets()[5]]) > 0).sum()) == 1
        for rho, determined, rel, how in GC.rung_verdicts(c, b, margin):
            assert determined, (b, rho, rel, how)
            if how == "all":
                worst = min(worst, rel)
        npos, nzero, rel = GC.numpy_inertia(c, b, margin)
        assert nzero == 0 and rel >= margin and (npos == s.nvar) == (b == 1)
    print(f"{route}: smallest relative |eigenvalue| of a rung decided by all eigenvalues {worst:.2e}")
    # the plan facts the row's route rests on, where the analysis alone shows them
    if pattern == "smallest":
        assert s.N - hipldl.Plan(s.N, c["rows"], c["cols"], s.nvar, s.nequ, s.ncon, batch=3).info["ncond"] == 96
    elif pattern == "records":
        info = hipldl.Plan(s.N, c["rows"], c["cols"], s.nvar, s.nequ, s.ncon, batch=3).info
        assert info["v2"] is not None and info["ncond"] == s.nequ and info["fmax"] <= 64
    elif pattern == "resblock":
        assert (s.nvar, s.nequ, s.ncon) == (65, 130, 0) and s.nnzjF == 65 * 130
