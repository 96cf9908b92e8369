"""Pins the oracle against the reference's own known answers (CPU, no GPU).

The reference asserts final solutions of `cannoles(nls, linsolve = :ldlfactorizations)` at atol = 1e-4
(/root/reference/test/runtests.jl:56-100, 116-171).  Here the restated outer loop
(tests/support/outer_loop.py) drives the ORACLE's newton_system! on the same problems and must reach
the same solutions; this is the only way the reference's tests constrain the linear-solver boundary.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests.support.outer_loop import SymNLS, solve


def oracle_solver(N, rows, cols, vals, nvar, nequ, ncon):
    return O.Oracle(N, rows, cols, O.canonical_perm(nvar, nequ, ncon))


def oracle_newton(LDLT, nvar, nequ, ncon, rhs, vals, rho_old, params):
    return O.newton_system(LDLT, nvar, nequ, ncon, rhs, vals, rho_old, params)


F_linear = lambda x: [x[0] - 2, x[1] - 3]
F_Rosen = lambda x: [x[0] - 1, 10 * (x[1] - x[0] ** 2)]


def F_larger(n):
    return lambda x: [10 * (x[i + 1] - x[i] ** 2) for i in range(n - 1)] + [x[i] - 1 for i in range(n - 1)]


def F_under(n):
    return lambda x: [x[0] - x[i] for i in range(1, n)]


c_linear = lambda x: [sum(x) - 1]


def c_quad(x):
    prod = 1
    for xi in x:
        prod = prod * xi
    return [sum(xi ** 2 for xi in x) - 5, prod - 2]


UNCONSTRAINED = [  # test/runtests.jl:63-78
    (F_linear, [-1.0, -1.0], [2.0, 3.0]),
    (F_Rosen, [-1.2, 1.0], [1.0, 1.0]),
    (F_larger(10), [0.9] * 10, [1.0] * 10),
] + [(F_under(10), [float(i)] * 10, [float(i)] * 10) for i in range(1, 6)]

CONSTRAINED = [  # test/runtests.jl:82-99
    (F_linear, c_linear, [-1.0, -1.0], [0.0, 1.0]),
    (F_Rosen, c_linear, [-1.2, 1.0], [0.6188, 0.3812]),
    (F_under(10), c_linear, [j / 10 for j in range(1, 11)], [0.1] * 10),
    (F_linear, c_quad, [0.9, 1.9], [1.0, 2.0]),
    (F_Rosen, c_quad, [0.9, 1.9], [1.0, 2.0]),
    (F_larger(3), c_quad, [0.5, 1.0, 1.5], [1.0647, 1.215, 1.546]),
]


@pytest.mark.parametrize("case", range(len(UNCONSTRAINED)))
def test_unconstrained_known_answers(params, case):
    F, x0, xf = UNCONSTRAINED[case]
    nls = SymNLS(F, x0)
    out = solve(nls, oracle_solver, oracle_newton, params)
    assert out["status"] in ("first_order", "small_residual")
    assert np.allclose(out["solution"], xf, atol=1e-4)


@pytest.mark.parametrize("case", range(len(CONSTRAINED)))
def test_constrained_known_answers(params, case):
    F, c, x0, xf = CONSTRAINED[case]
    nls = SymNLS(F, x0, c)
    out = solve(nls, oracle_solver, oracle_newton, params)
    assert out["status"] in ("first_order", "small_residual")
    assert np.allclose(out["solution"], xf, atol=1e-4)


def test_hs6_resolve_and_small_residual(params):
    """test/runtests.jl:116-171: HS6 from two starting points, and the small-residual stop"""
    F = lambda x: [x[0] - 1]
    c = lambda x: [10 * (x[1] - x[0] ** 2)]
    for x0 in ([-1.2, 1.0], [10.0, 10.0]):
        out = solve(SymNLS(F, x0, c), oracle_solver, oracle_newton, params)
        assert out["status"] == "first_order"
        assert np.allclose(out["solution"], [1.0, 1.0], atol=1e-6)
    out = solve(SymNLS(F, [-1.2, 1.0], c), oracle_solver, oracle_newton, params, atol=1e-15, rtol=0.0, Fatol=1e-6, Frtol=0.0)
    assert out["status"] == "small_residual" and abs(out["objective"]) < 1e-6


def test_gauss_newton_variant(params):
    """method = :Newton_noFHess (test/runtests.jl:205-214): empty H_F segment, still reaches [1, 1]"""
    out = solve(SymNLS(F_Rosen, [-1.2, 1.0]), oracle_solver, oracle_newton, params, method="Newton_noFHess")
    assert np.allclose(out["solution"], [1.0, 1.0], atol=1e-6)


# ---- batched outer loop (host threads + one batched Newton call per round) ---------------------
def _oracle_batched(rows, cols, dims, rhs, vals, rho_old, params):
    """stand-in for the batched device call on machines without a GPU: the oracle, slot by slot"""
    N, n, m, p = dims
    orc = O.Oracle(N, rows, cols, O.canonical_perm(n, m, p))
    B = rhs.shape[0]
    d = np.zeros((B, N)); ok = np.zeros(B, bool); rho = np.zeros(B); ro = np.zeros(B); nf = np.zeros(B, int)
    for b in range(B):
        d[b], ok[b], rho[b], ro[b], nf[b] = O.newton_system(orc, n, m, p, rhs[b], vals[b], rho_old[b], params)
    return d, ok, rho, ro, nf


def test_batched_outer_loop_matches_single_runs(params):
    """cannoles_jl_amd.batch_solve: B outer loops over one batched linear solver give the same answers as B separate
    runs (reference known answers with n = 2, nequ = 2, ncon = 1 — one dense pattern — from several starting points)."""
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import batch_solve
    (F0, c0, x00, xf0), (F1, c1, x01, xf1) = CONSTRAINED[0], CONSTRAINED[1]
    cases = [(F0, c0, x00, xf0), (F1, c1, x01, xf1), (F1, c1, [-1.0, 0.5], xf1), (F0, c0, [3.0, -2.0], xf0), (F1, c1, [0.0, 0.0], xf1)]
    models = [SymNLS(F, x0, c) for F, c, x0, xf in cases]
    res, ncalls = batch_solve.solve_batch(models, params, executor=_oracle_batched)
    singles = [solve(SymNLS(F, x0, c), oracle_solver, oracle_newton, params) for F, c, x0, xf in cases]
    for k, (F, c, x0, xf) in enumerate(cases):
        assert res[k]["status"] == singles[k]["status"] and res[k]["iter"] == singles[k]["iter"]
        assert res[k]["nlinsolve"] == singles[k]["nlinsolve"] and res[k]["nfact"] == singles[k]["nfact"]
        assert np.array_equal(res[k]["solution"], singles[k]["solution"])
        assert np.allclose(res[k]["solution"], xf, atol=1e-4)
    # batching works: as many device calls as the longest problem needs, fewer than the Newton systems solved
    assert ncalls == max(r["nlinsolve"] for r in res) and ncalls < sum(r["nlinsolve"] for r in res)


def test_batched_outer_loop_rejects_mixed_patterns(params):
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import batch_solve
    F0, c0, x0, _ = CONSTRAINED[0]
    F2, c2, x2, _ = CONSTRAINED[2]
    with pytest.raises(ValueError):
        batch_solve.solve_batch([SymNLS(F0, x0, c0), SymNLS(F2, x2, c2)], params, executor=_oracle_batched)


# ---- the inner-iteration limit is `stalled`, the evaluation count `max_eval` (src/CaNNOLeS.jl:843, 846) ------------------------------------
def test_inner_iteration_limit_reports_stalled_and_the_evaluation_count_max_eval(params):
    """max_inner = 1 on the rough band family (300, 4), seed 304: problems 0, 1 and 3 leave an inner loop at the limit and end `stalled`
    (the reference hands `inner_iter > max_inner >= 0` to get_status as `stalled`; `max_eval` there is the evaluation count alone), with
    the counters of the run; problem 2 never reaches the limit.  A small max_eval still gives `max_eval`, with or without the limit."""
    import torch
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import device_loop as DL, synthetic as syn
    fam = DL.BandQuadFamily(syn.band_structure(300, 4), 12, seed=304, torch=torch, device="cpu", curvature=3.0, start=2.0, noise=0.5)
    want = {0: ("stalled", 10, 10, 26, 2), 1: ("stalled", 7, 7, 19, 2), 3: ("stalled", 34, 34, 83, 3), 2: ("first_order", 30, 30, 69, 0)}
    for b, w in want.items():
        one = solve(fam.host_model(b), oracle_solver, oracle_newton, params, max_inner=1)
        assert (one["status"], one["iter"], one["nlinsolve"], one["nfact"], one["nbk"]) == w, b
    for kw in (dict(max_eval=5), dict(max_eval=5, max_inner=1)):
        model = fam.host_model(0)
        one = solve(model, oracle_solver, oracle_newton, params, **kw)
        assert one["status"] == "max_eval" and model.neval > 5, kw
    assert solve(fam.host_model(0), oracle_solver, oracle_newton, params)["status"] == "first_order"
