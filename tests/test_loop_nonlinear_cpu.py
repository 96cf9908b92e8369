"""The inputs of tests/test_loop_nonlinear_gpu.py, vouched for without a GPU: BandQuadConFamily's callbacks against central differences
and against each other (numpy twin and torch on the CPU), the hand-written closed forms of tests/support/ref_problem_family.py against
the sympy models, what the chosen seed is chosen for, and that the comparison with the host mirror can see the feature: the same scalar
runs on a model without constraint Hessian, or with a constraint Jacobian that is never re-evaluated, take other decisions."""
import numpy as np
import pytest
import torch

from tests.support import loop_nonlinear_cases as K
from tests.support import ref_problem_family as RP


def _central(f, x, h=1e-5):
    """d f / d x by central differences: [len(f), len(x)]"""
    cols = []
    for j in range(len(x)):
        e = np.zeros(len(x))
        e[j] = h
        cols.append((f(x + e) - f(x - e)) / (2 * h))
    return np.stack(cols, axis=1)


def _dense_lower(model, vals):
    H = np.zeros((model.nvar, model.nvar))
    H[np.asarray(model.h_rows) - 1, np.asarray(model.h_cols) - 1] = vals
    return H + np.tril(H, -1).T


@pytest.mark.parametrize("b", [0, 5, 11])
def test_host_model_derivatives_against_central_differences(built, b):
    """c is quadratic, so central differences are exact up to rounding: jac to 1e-9, and the Hessian of lam'c — the central difference
    of x -> jac(x)' lam — to 1e-8"""
    fam = K.family()
    M = fam.host_model(b)
    rng = np.random.default_rng(b)
    x, lam = rng.normal(size=M.nvar), rng.normal(size=M.ncon)
    assert np.abs(M.jac(x) - _central(M.cons, x)).max() <= 1e-9
    H = _dense_lower(M, M.hess_coord_cons(x, lam))
    assert np.abs(H - _central(lambda y: M.jac(y).T @ lam, x)).max() <= 1e-8
    assert np.abs(np.diag(H)).min() > 0 and np.count_nonzero(H - np.diag(np.diag(H))) == 0   # every variable is in a block; diagonal
    assert np.abs(M.cons(x) - fam.host_model(b).cons(x)).max() == 0


def test_constraints_vanish_at_the_generating_point(built):
    """e is such that c(xs) = 0; xs is not kept, but x0 = xs + start * noise: with start = 0 the start point is xs"""
    fam = K.family(start=0.0)
    for b in range(K.BL):
        assert np.abs(fam.host_model(b).cons(fam.h["x0"][b])).max() <= 1e-12


def test_base_data_are_those_of_the_linear_family(built):
    """g is drawn behind every draw of the base class: the data both have are equal, and the base family is still linear"""
    from cannoles_jl_amd import device_loop as DL, synthetic as syn
    fam = K.family()
    kind = {k: v for k, v in K.KIND.items() if k != "con_curvature"}
    base = DL.BandQuadFamily(syn.band_structure(K.N, K.P), K.BL, K.SEED, torch=torch, device="cpu", **kind)
    for k in ("A", "q", "Cv", "x0", "y"):
        assert np.array_equal(fam.h[k], base.h[k]), k
    assert not np.array_equal(fam.h["e"], base.h["e"]) and "g" not in base.h and "g" in fam.per_problem_tensors()
    assert np.abs(fam.h["g"]).max() <= K.KIND["con_curvature"] and np.abs(fam.h["g"]).min() > 0
    assert getattr(base, "linear_constraints", True) is True and fam.linear_constraints is False
    assert not hasattr(base, "hess_cons_vals")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_torch_callbacks_against_the_host_twins(built, dtype):
    """cons, jacc_vals and hess_cons_vals on CPU tensors against host_model(b), on the family and on a head / take of it.  Float64: a few
    ulps (other summation order); Float32: the same data, computed in float"""
    fam = K.family(dtype=dtype)
    rng = np.random.default_rng(3)
    X, LAM = rng.normal(size=(K.BL, K.N)).astype(dtype), rng.normal(size=(K.BL, K.P)).astype(dtype)
    tol = 64 * float(np.finfo(dtype).eps)
    for sub, idx in ((fam, range(K.BL)), (fam.head(5), range(5)), (fam.take([7, 2]), [7, 2])):
        idx = list(idx)
        tX, tL = torch.as_tensor(X[idx]), torch.as_tensor(LAM[idx])
        c, Jc, Hc = sub.cons(tX).numpy(), sub.jacc_vals(tX).numpy(), sub.hess_cons_vals(tX, tL).numpy()
        assert c.dtype == Jc.dtype == Hc.dtype == np.dtype(dtype)
        for i, b in enumerate(idx):
            M = fam.host_model(b)
            x, lam = X[b].astype(np.float64), LAM[b].astype(np.float64)
            J = M.jac(x)[fam.cr, fam.cc]
            assert np.abs(c[i] - M.cons(x)).max() <= tol * K.N, b
            assert np.abs(Jc[i] - J).max() <= tol * max(1.0, np.abs(J).max()), b
            assert np.abs(Hc[i] - M.hess_coord_cons(x, lam)).max() <= tol, b


@pytest.mark.parametrize("name", list(RP.PROBLEMS))
def test_reference_problem_closed_forms(built, name):
    """the hand-written torch closed forms against the sympy model, at the start points and at a random point; row 0 is the reference's
    start point, the others are within PERTURBATION of it"""
    fam = RP.RefProblemFamily(name, 8, 1, torch, "cpu")
    s = fam.s
    assert np.array_equal(fam.h["x0"][0], RP.PROBLEMS[name][4]) and np.abs(fam.h["x0"] - fam.h["x0"][0]).max() <= RP.PERTURBATION
    assert len({tuple(r) for r in fam.h["x0"]}) == 8
    rng = np.random.default_rng(5)
    for X in (fam.h["x0"], rng.normal(size=(8, s.nvar))):
        R, LAM = rng.normal(size=(8, s.nequ)), rng.normal(size=(8, s.ncon))
        tX, tR, tL = (torch.as_tensor(a) for a in (X, R, LAM))
        got = [f.numpy() for f in (fam.residual(tX), fam.jac_vals(tX), fam.hess_vals(tX, tR), fam.cons(tX), fam.jacc_vals(tX), fam.hess_cons_vals(tX, tL))]
        for b in range(8):
            M = fam.host_model(b)
            assert (tuple(M.h_rows), tuple(M.h_cols)) == (tuple(s.hF[0]), tuple(s.hF[1]))
            assert (tuple(M.jF_rows), tuple(M.jF_cols)) == (tuple(s.jF[0]), tuple(s.jF[1]))
            assert (tuple(M.jc_rows), tuple(M.jc_cols)) == (tuple(s.jc[0]), tuple(s.jc[1]))
            want = [M.residual(X[b]), M.jac_residual(X[b]).ravel(), M.hess_coord_residual(X[b], R[b]), M.cons(X[b]), M.jac(X[b]).ravel(),
                    M.hess_coord_cons(X[b], LAM[b])]
            for k, (g, w) in enumerate(zip(got, want)):
                assert g[b].shape == w.shape and np.abs(g[b] - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), (name, b, k)


def test_the_chosen_seed_does_what_it_is_chosen_for(built):
    fam = K.family()
    ones = K.scalar_runs(fam, "nonlinear")
    K.assert_chosen_for(ones)
    rejecting = [b for b, o in enumerate(ones) if o["rejected"] > 0]
    print("iter", K.col(ones, "iter"), "nbk", K.col(ones, "nbk"), "rejected", K.col(ones, "rejected"),
          "ladder", [o["nfact"] - o["nlinsolve"] for o in ones])
    assert rejecting == [0, 9] and all(ones[b]["nbk"] > 0 for b in rejecting)


def test_the_float32_seed_is_chosen_for_decisions_that_survive_float32_rounding(built):
    """the Float32 comparison: the host mirror on the rounded data, with the Float32 run's tolerances and parameters, does what the
    Float64 seed is chosen for, and takes the same decisions on every problem when the callbacks work in Float32"""
    from cannoles_jl_amd import hipldl
    fam = K.family(dtype=np.float32, seed=K.F32_SEED)
    ones = K.scalar_runs(fam, "nonlinear f32", **K.f32_run(hipldl))
    K.assert_chosen_for(ones)
    assert [b for b, o in enumerate(ones) if o["rejected"] > 0 and o["nbk"] > 0] == [0, 1, 10]
    assert K.float32_stable(fam, "nonlinear f32", ones, **K.f32_run(hipldl)) == []


@pytest.mark.parametrize("seed, problems", [(48, [5]), (53, [4, 7])])
def test_the_float32_criterion_sees_the_seeds_it_is_meant_to_refuse(built, seed, problems):
    """seeds with three rejecting problems in front of F32_SEED: decisions move under a perturbation of Float32 size, on the problems on
    which a Float32 run on the device left the mirror's counters (tests/test_loop_nonlinear_gpu.py)"""
    from cannoles_jl_amd import hipldl
    fam = K.family(dtype=np.float32, seed=seed)
    ones = K.scalar_runs(fam, ("nonlinear f32", seed), **K.f32_run(hipldl))
    K.assert_chosen_for(ones)
    assert K.float32_stable(fam, ("nonlinear f32", seed), ones, **K.f32_run(hipldl)) == problems


@pytest.mark.parametrize("method", ["Newton_noFHess", "Newton_vanishing"])
def test_the_other_methods_end_too(built, method):
    ones = K.scalar_runs(K.family(**K.METHOD_KINDS[method]), ("nonlinear", method), method=method)
    assert set(K.col(ones, "status")) <= {"first_order", "small_residual"}, K.col(ones, "status")
    assert any(o["rejected"] > 0 and o["nbk"] > 0 for o in ones)
    if method == "Newton_vanishing":
        assert K.col(ones, "hess_skipped") == [1, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0]


@pytest.mark.parametrize("wrap", [K.NoConstraintHessian, K.StaleConstraintJacobian], ids=["zero H_c", "stale J_c"])
def test_the_comparison_can_see_the_feature(built, wrap):
    """without the constraint Hessian, or with a constraint Jacobian that is never evaluated again, the scalar loop takes other decisions
    on at least one problem: a device loop that did either could not match the host mirror's counters"""
    fam = K.family()
    ones = K.scalar_runs(fam, "nonlinear")
    crippled = K.scalar_runs(fam, ("nonlinear", wrap.__name__), wrap=wrap, max_iter=60)
    differ = [b for b in range(K.BL) if (ones[b]["iter"], ones[b]["nfact"]) != (crippled[b]["iter"], crippled[b]["nfact"])]
    print(wrap.__name__, "differs on", differ)
    assert differ


def test_reference_problems_on_the_host_mirror(built):
    """row 0 of every reference problem reaches the reference's answer on the host mirror (what tests/test_oracle_pinning.py pins), and so
    do the perturbed rows"""
    for name in RP.PROBLEMS:
        fam = RP.RefProblemFamily(name, 8, 1, torch, "cpu")
        ones = K.scalar_runs(fam, ("ref", name))
        assert set(K.col(ones, "status")) <= {"first_order", "small_residual"}, (name, K.col(ones, "status"))
        assert np.allclose(ones[0]["solution"], fam.answer, atol=RP.REF_ATOL), name


def test_framework_restatement_refuses_nonlinear_constraints(built):
    from cannoles_jl_amd import device_loop as DL
    with pytest.raises(ValueError, match="nonlinear"):
        DL.solve_batch_device_framework(K.family())


def test_wide_shape(built):
    """the shape of the test of both gaps together: 1 025 constraints, the smallest number above the LDS instance's 1 024 that
    band_structure takes with n = 2 p; the family's callbacks agree with the host twin there too.  (Its scalar runs take seconds: the GPU
    test makes them, and asserts what it needs of them, before it touches the device.)"""
    fam = K.wide_family()
    assert fam.s.ncon == 1025 and fam.s.nvar == 2 * fam.s.ncon and fam.B == K.WIDE_B
    M = fam.host_model(1)
    rng = np.random.default_rng(9)
    X, LAM = rng.normal(size=(K.WIDE_B, K.WIDE_N)), rng.normal(size=(K.WIDE_B, K.WIDE_P))
    tX, tL = torch.as_tensor(X), torch.as_tensor(LAM)
    assert np.abs(fam.cons(tX).numpy()[1] - M.cons(X[1])).max() <= 1e-13
    assert np.abs(fam.jacc_vals(tX).numpy()[1] - M.jac(X[1])[fam.cr, fam.cc]).max() <= 1e-14
    assert np.abs(fam.hess_cons_vals(tX, tL).numpy()[1] - M.hess_coord_cons(X[1], LAM[1])).max() <= 1e-14
