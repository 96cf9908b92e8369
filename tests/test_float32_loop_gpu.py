"""The lockstep outer loop in Float32 on the device (device_loop.solve_batch_device with a Float32 family: a Float32 band handle, the
`_f32_dev` passes, cnl_outer_state_f32 and the cnl_outer_*_f32_dev kernels).  -m gpu.

`solve!` is generic in T and the reference's suite runs it in Float32 (test/runtests.jl:102-113, "Multiprecision") with the tolerance
atol = max(1e-4, eps(T)^(1/4)); that tolerance holds the mild family here against the Float64 loop with the CPU oracle.  The rough
family (the rho ladder is climbed, the line search backtracks) is non-convex — two precisions may end at different stationary points —
so its results are held to an independent Float64 evaluation of the optimality measure at the returned point instead."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
MULTIPRECISION_ATOL = max(1e-4, EPS32 ** 0.25)   # test/runtests.jl:110; 1.86e-2
COUNTERS = ("iter", "nlinsolve", "nfact", "nbk")
MILD = dict()                                     # the class defaults: curvature=0.3, start=0.3, noise=0.01
ROUGH = dict(curvature=3.0, start=2.0, noise=0.5)
B = 12


def _mods():
    import torch
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import device_loop as DL, hipldl, synthetic as syn
    return torch, DL, hipldl, syn


def _family(shape, kind, dtype=np.float32, batch=B):
    torch, DL, hipldl, syn = _mods()
    n, p = shape
    return DL.BandQuadFamily(syn.band_structure(n, p), batch, seed=n + p, torch=torch, device="cuda:0", dtype=dtype, **kind)


_runs = {}


def _solved(shape, kind_name):
    """one Float32 run per (shape, family) for the tests that look at the same batch"""
    key = (shape, kind_name)
    if key not in _runs:
        torch, DL, hipldl, syn = _mods()
        fam = _family(shape, {"mild": MILD, "rough": ROUGH}[kind_name])
        _runs[key] = (fam, DL.solve_batch_device(fam))
    return _runs[key]


def _close32(a, b):
    return bool((np.abs(a - b) <= 16 * EPS32 * np.maximum(1.0, np.abs(b))).all())


@pytest.mark.parametrize("shape", [(300, 4), (1000, 10)])
def test_mild_family_against_the_float64_loop(built, shape):
    """(a) every problem ends first_order on the band kernels, and x, lambda are within the reference's multiprecision tolerance of the
    Float64 single-problem loop with the CPU oracle on the same (float32-representable) data.  Counters are not compared: Float32
    legitimately takes fewer iterations (its tolerances are those of eps(Float32)).
    A CPU emulation of the Float32 loop gave max |dx| = 2.2e-6, max |dlambda| = 4.8e-7; the measured maxima are printed."""
    torch, DL, hipldl, syn = _mods()
    from cannoles_jl_amd import outer_loop
    from tests.test_oracle_pinning import oracle_newton, oracle_solver
    fam, got = _solved(shape, "mild")
    assert got["dtype"] == "float32" and got["solution"].dtype == np.float32 and got["r"].shape == (B, fam.s.nequ)
    assert got["kernel"] == "band"
    assert got["status"] == ["first_order"] * B
    prm = hipldl.default_params()
    dx = dl = 0.0
    for b in range(B):
        one = outer_loop.solve(fam.host_model(b), oracle_solver, oracle_newton, prm)
        assert one["status"] == "first_order"
        dx = max(dx, float(np.abs(got["solution"][b].astype(np.float64) - one["solution"]).max()))
        dl = max(dl, float(np.abs(got["multipliers"][b].astype(np.float64) - one["multipliers"]).max()))
    print(f"float32 lockstep loop, mild {shape}: max|dx| = {dx:.3e}, max|dlambda| = {dl:.3e}, steps = {got['steps']}, "
          f"iter = {got['iter'].tolist()}, vals_layout = {got['vals_layout']}")
    assert dx <= MULTIPRECISION_ATOL and dl <= MULTIPRECISION_ATOL


def _optimality64(fam, got, b):
    """(measure, rounding bound) of problem b in float64 from the widened outputs: max(|J'r - Jc'lam|_inf / ds, |[F - r; c]|_inf) with
    ds = max(100, sum|lam| / p) / 100, and 2 K eps32 S — the standard bound of the float32 evaluation of those sums (K: the longest sum,
    S: the largest sum of magnitudes)."""
    M = fam.host_model(b)
    p = fam.s.ncon
    x, r = got["solution"][b].astype(np.float64), got["r"][b].astype(np.float64)
    lam = got["multipliers"][b].astype(np.float64)
    J, F = M.jac_residual(x), M.residual(x)
    Jc, c = (M.jac(x), M.cons(x)) if p else (np.zeros((0, len(x))), np.zeros(0))
    dual = J.T @ r - Jc.T @ lam
    primal = np.concatenate([F - r, c])
    ds = max(100.0, np.abs(lam).sum() / p) / 100.0 if p else 1.0
    measure = max(np.abs(dual).max() / ds, np.abs(primal).max())
    JJ = np.vstack([J, Jc])
    K = max(int((JJ != 0).sum(axis=0).max()), int((J != 0).sum(axis=1).max())) + 3
    S = max((np.abs(J).T @ np.abs(r) + np.abs(Jc).T @ np.abs(lam)).max(), (np.abs(J) @ np.abs(x) + np.abs(F) + np.abs(r)).max())
    return measure, 2 * K * EPS32 * S


@pytest.mark.parametrize("shape", [(300, 4), (300, 0)])
def test_rough_family_climbs_backtracks_and_ends_optimal(built, shape):
    """(b) every problem ends first_order, the rho ladder is climbed (more factorisations than Newton systems) and the line-search
    kernels backtrack; the optimality measure recomputed in float64 at the returned (x, r, lambda) is within the loop's own tolerance
    plus the rounding bound of its float32 evaluation.  Not compared with the Float64 solution: the problem is non-convex."""
    fam, got = _solved(shape, "rough")
    assert got["kernel"] == "band"
    assert got["status"] == ["first_order"] * B
    print(f"float32 lockstep loop, rough {shape}: steps = {got['steps']}, nlinsolve = {got['nlinsolve'].tolist()}, nfact = {got['nfact'].tolist()}, "
          f"nbk = {got['nbk'].tolist()}")
    assert got["nfact"].sum() > got["nlinsolve"].sum()
    assert got["nbk"].sum() > 0
    ratios = []
    for b in range(B):
        measure, slack = _optimality64(fam, got, b)
        own = max(got["normdual"][b] / (max(100.0, np.abs(got["multipliers"][b].astype(np.float64)).sum() / shape[1]) / 100.0 if shape[1] else 1.0),
                  got["normprimal"][b])
        ratios.append((measure / got["epstol"][b], own / got["epstol"][b], slack / got["epstol"][b]))
        assert measure <= got["epstol"][b] + slack, (b, measure, got["epstol"][b], slack)
    print("  (float64 measure, the loop's own measure, rounding bound) / epstol per problem: " + ", ".join(f"({a:.2f}, {o:.2f}, {s_:.2f})" for a, o, s_ in ratios))


def test_each_problem_decides_alone(built):
    """(c) sub-batches of the rough (300, 4) family — three single problems and the first five — take the decisions of the batch of 12"""
    torch, DL, hipldl, syn = _mods()
    fam, got = _solved((300, 4), "rough")
    picks = [[int(b)] for b in np.sort(np.random.default_rng(304).choice(B, 3, replace=False))] + [list(range(5))]
    for idx in picks:
        sub = DL.solve_batch_device(fam.take(idx))
        assert sub["status"] == [got["status"][b] for b in idx], idx
        for k in COUNTERS:
            assert np.array_equal(sub[k], got[k][idx]), (idx, k)
        assert _close32(sub["solution"], got["solution"][idx]), idx
        print(f"  sub-batch {idx}: solutions bit-equal to the batch's: {np.array_equal(sub['solution'], got['solution'][idx])}")


@pytest.mark.parametrize("kind", ["rough", "mild"])
def test_kernels_against_the_framework_form(built, kind):
    """(d) the nine Float32 kernels against the loop written as framework expressions in float32 (decision sums: double terms, summed,
    rounded once — as the kernels)"""
    torch, DL, hipldl, syn = _mods()
    fam, got = _solved((300, 4), kind)
    old = DL.solve_batch_device_framework(fam, dtype=np.float32)
    assert old["dtype"] == "float32" and old["solution"].dtype == np.float32
    assert old["steps"] == got["steps"] and old["status"] == got["status"]
    for k in COUNTERS:
        assert np.array_equal(old[k], got[k]), k
    assert _close32(old["solution"], got["solution"])
    print(f"  framework form, {kind}: max |dx| = {np.abs(old['solution'] - got['solution']).max():.3e}")


def test_layouts_agree_and_element_types_do_not_mix(built):
    """(e) problem-major `vals` give what interleaved ones give, bit for bit; a family of the other element type is refused by the driver
    (the C side cannot tell a Float64 state from a Float32 one)"""
    torch, DL, hipldl, syn = _mods()
    fam, got = _solved((300, 4), "rough")
    assert got["vals_layout"] == "interleaved"
    pm = DL.solve_batch_device(fam, layout="problem-major")
    assert pm["kernel"] == "band" and pm["vals_layout"] == "problem-major"
    assert pm["steps"] == got["steps"] and pm["status"] == got["status"]
    for k in COUNTERS:
        assert np.array_equal(pm[k], got[k]), k
    assert np.array_equal(pm["solution"].view(np.uint32), got["solution"].view(np.uint32))
    fam64 = _family((300, 4), ROUGH, dtype=np.float64, batch=2)
    with pytest.raises(TypeError):
        DL.solve_batch_device(fam64, dtype=np.float32)
    with pytest.raises(TypeError):
        DL.solve_batch_device(fam.take([0, 1]), dtype=np.float64)


def test_a_finite_objective_never_breaks_a_float32_problem(built):
    """(f) T(1e60) is Inf32: cnl_outer_newton_done_f32_dev on a hand-built state of two problems that took a Newton system — fx = 3e38
    stays active, fx = inf is `broken`"""
    torch, DL, hipldl, syn = _mods()
    dev = torch.device("cuda", 0)
    nb, n, m, p = 2, 3, 3, 1
    N = n + m + p
    st = hipldl.cnl_outer_state_f32()
    scalars = dict(B=nb, n=n, m=m, p=p, P=1, N=N, nnzjF=5, nnzjc=2, max_inner=10, dmin=1e-8, rhomax=1e10, delta_dec=0.1, smax=100.0, gammaA=1e-2,
                   eps2=EPS32 ** 2)
    for k, v in scalars.items():
        setattr(st, k, v)
    keep = {}
    for k, ty in st._fields_:
        if k in scalars:
            continue
        if k in ("status", "it", "flags", "nf_new", "ok_new"):
            a = torch.zeros(16, dtype=torch.int32, device=dev)
        elif k in ("inner", "nfact", "nlin", "nbk"):
            a = torch.zeros(16, dtype=torch.int64, device=dev)
        elif k in ("phase0", "act", "need", "brk", "ext", "lsm", "rej", "chk", "done_in", "tired", "small_res", "bt"):
            a = torch.zeros(16, dtype=torch.uint8, device=dev)
        else:
            a = torch.zeros(nb * 16, dtype=torch.float32, device=dev)   # rows of at most N = 7 < 16 entries
        keep[k] = a
        setattr(st, k, a.data_ptr())
    keep["act"][:nb] = 1
    keep["need"][:nb] = 1
    keep["ok_new"][:nb] = 1
    keep["nf_new"][:nb] = 1
    keep["delta"][:nb] = 1.0
    keep["epsk"][:nb] = 1e3
    keep["d_new"][:nb * N] = 0.5
    keep["fx"][0], keep["fx"][1] = 3e38, float("inf")
    stream = torch.cuda.current_stream(dev).cuda_stream
    hipldl._check(hipldl.lib().cnl_outer_newton_done_f32_dev(C.byref(st), 1, stream))
    torch.cuda.synchronize(dev)
    assert keep["brk"][:nb].tolist() == [0, 1]
    assert keep["act"][:nb].tolist() == [1, 0]
    assert keep["ext"][:nb].tolist() == [1, 0]
    assert keep["nlin"][:nb].tolist() == [1, 1] and keep["nfact"][:nb].tolist() == [1, 1]
    assert keep["d"][:N].tolist() == [0.5] * N
