"""The lockstep loop on models with NONLINEAR constraints, on the GPU (-m gpu): H_c = sum_k lam_k Hess c_k in front of every Newton
system and a constraint Jacobian of its own at the trial point (device_loop.solve_batch_device with a family whose `linear_constraints`
is False).  tests/test_loop_nonlinear_cpu.py vouches for the inputs and shows that the host mirror's counters change when either is
left out; every test here asserts again what its inputs are chosen for before it touches the device.

Against the host mirror: outer_loop.solve with the CPU oracle on tests/support/counting_model.CountingModel, problem by problem —
status, iter, nlinsolve, nfact, nbk and neval equal.  Solutions, Float64: the bars of tests/test_loop_keywords_gpu._close_solutions
(atol = rtol = 1e-7 on x, 1e-6 on the multipliers, 1e-9 relative on the objective).  Float32: the host mirror runs in Float64 on the
rounded data with the Float32 run's tolerances (sqrt(eps32), eps32) and ParamCaNNOLeS(Float32); both end where dual and primal
residual are below epstol = sqrt(eps32) (1 + ||dual_0||), so the bars are those of Float64 scaled by the ratio of the two stopping
tolerances, sqrt(eps32) / sqrt(eps64) = 2.3e4 (x: 2.3e-3, multipliers: 2.3e-2): what separates two runs that stop at the same
threshold scales with the threshold.  The counters of a Float32 run are held to that Float64-arithmetic mirror at a seed chosen on the
CPU for decisions that survive perturbations of Float32 size in every callback and every Newton system
(tests/support/loop_nonlinear_cases.F32_SEED).
"""
import numpy as np
import pytest

from tests.support import loop_nonlinear_cases as K
from tests.support import ref_problem_family as RP

pytestmark = pytest.mark.gpu

EXACT = ("solution", "multipliers", "r", "objective", "normdual", "normprimal", "epstol", "iter", "nfact", "nlinsolve", "nbk", "neval")
F32_SCALE = float(np.sqrt(np.finfo(np.float32).eps) / np.sqrt(np.finfo(np.float64).eps))


def _mods():
    import torch
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import device_loop as DL, hipldl, synthetic as syn
    return torch, DL, hipldl, syn


def _same_decisions(got, ones, tag):
    print(f"{tag}: device {got['status']}, " + ", ".join(f"{k} = {got[k].tolist()}" for k in K.DECISIONS))
    print(f"{tag}: mirror {K.col(ones, 'status')}, " + ", ".join(f"{k} = {K.col(ones, k)}" for k in K.DECISIONS))
    assert got["status"] == K.col(ones, "status"), tag
    for k in K.DECISIONS:
        assert got[k].tolist() == K.col(ones, k), (tag, k, got[k].tolist(), K.col(ones, k))


def _distances(got, ones, tag):
    dx = max(float(np.abs(got["solution"][b] - o["solution"]).max()) for b, o in enumerate(ones))
    dl = max(float(np.abs(got["multipliers"][b] - o["multipliers"]).max()) for b, o in enumerate(ones))
    print(f"{tag}: max|dx| = {dx:.3e}, max|dlambda| = {dl:.3e} against the host mirror")


def _close_solutions(got, ones, tag, scale=1.0):
    _distances(got, ones, tag)
    for b, o in enumerate(ones):
        assert np.allclose(got["solution"][b], o["solution"], atol=1e-7 * scale, rtol=1e-7 * scale), (tag, b)
        assert np.allclose(got["multipliers"][b], o["multipliers"], atol=1e-6 * scale, rtol=1e-6 * scale), (tag, b)
        assert abs(got["objective"][b] - o["objective"]) <= 1e-9 * scale * max(1.0, o["objective"]), (tag, b)


def _bit_equal(a, b, tag):
    for k in EXACT + (("hess_skipped",) if "hess_skipped" in b else ()):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (tag, k)
    assert a["status"] == b["status"] and a["steps"] == b["steps"], tag


def test_loop_against_the_host_mirror_f64(built):
    """fails on a loop that hands `prepare` a zero H_c or keeps one constraint-Jacobian array"""
    torch, DL, hipldl, syn = _mods()
    ones = K.scalar_runs(K.family(), "nonlinear")
    K.assert_chosen_for(ones)
    got = DL.solve_batch_device(K.family("cuda:0"))
    assert got["dtype"] == "float64" and got["jct_shared"] is False
    _same_decisions(got, ones, "nonlinear f64")
    _close_solutions(got, ones, "nonlinear f64")


def test_loop_against_the_host_mirror_f32(built):
    """The Float32 run against the host mirror, which computes in Float64 (there is no Float32 mirror): counters equal, solutions at the
    scaled bars of the module docstring.  The mirror's decisions bind a Float32 run only where they do not hang on the last bits, so the
    seed is chosen on the CPU for decisions that survive perturbations of Float32 size in every callback and every Newton system
    (tests/support/loop_nonlinear_cases.F32_SEED; asserted here again before the device is touched).  Measured on an MI355X: all twelve
    problems take the mirror's decisions, max|dx| = 1.5e-6, max|dlambda| = 4.5e-7.  At seeds 48 and 53, which that criterion refuses,
    the run left the mirror's counters on problem 5 (iter 13 against 14), and on problems 4 and 7 — the problems the criterion names."""
    torch, DL, hipldl, syn = _mods()
    fam_h = K.family(dtype=np.float32, seed=K.F32_SEED)    # (host_model: the Float64 twin of the rounded data)
    ones = K.scalar_runs(fam_h, "nonlinear f32", **K.f32_run(hipldl))
    K.assert_chosen_for(ones)
    assert K.float32_stable(fam_h, "nonlinear f32", ones, **K.f32_run(hipldl)) == []   # (what F32_SEED is chosen for)
    got = DL.solve_batch_device(K.family("cuda:0", dtype=np.float32, seed=K.F32_SEED))
    assert got["dtype"] == "float32" and got["solution"].dtype == np.float32 and got["jct_shared"] is False
    _distances(got, ones, "nonlinear f32")
    _same_decisions(got, ones, "nonlinear f32")
    _close_solutions(got, ones, "nonlinear f32", scale=F32_SCALE)


def test_loop_float32_sub_batches_and_compaction(built):
    """Float32 at the bars tests/test_loop_keywords_gpu.test_loop_float32 holds a Float32 run to: every problem decides alone (sub-batches
    take the same decisions, solutions within 16 eps32), compact on / off bit-equal, every problem ends first_order"""
    torch, DL, hipldl, syn = _mods()
    fam = K.family("cuda:0", dtype=np.float32, seed=K.F32_SEED)
    got = DL.solve_batch_device(fam)
    assert got["dtype"] == "float32" and set(got["status"]) == {"first_order"} and got["nbk"].any() and (got["nfact"] > got["nlinsolve"]).any()
    packed = DL.solve_batch_device(fam, compact=True, compact_min_finished=1)
    assert packed["compactions"] >= 1
    _bit_equal(packed, got, "float32 compact")
    eps32 = float(np.finfo(np.float32).eps)
    for idx in ([5], [0, 1, 2, 3, 4], [11, 10]):
        sub = DL.solve_batch_device(fam.take(idx))
        assert sub["status"] == [got["status"][b] for b in idx], idx
        for k in K.DECISIONS:
            assert np.array_equal(sub[k], got[k][idx]), (idx, k)
        assert (np.abs(sub["solution"] - got["solution"][idx]) <= 16 * eps32 * np.maximum(1.0, np.abs(got["solution"][idx]))).all(), idx


def _compact_against(fam, got, tag, shrinks, **kw):
    torch, DL, hipldl, syn = _mods()
    packed = DL.solve_batch_device(fam, compact=True, compact_min_finished=1, **kw)
    print(f"  {tag}, compact: kernel {packed['kernel']}, compactions = {packed['compactions']}, handle_shrunk = {packed['handle_shrunk']}")
    assert packed["compactions"] >= 1 and packed["handle_shrunk"] is shrinks and packed["jct_shared"] is False
    _bit_equal(packed, got, tag)


@pytest.mark.parametrize("method", list(K.METHOD_KINDS))
def test_loop_methods_and_compaction(built, method):
    """every method against the host mirror, and compact = True, compact_min_finished = 1 bit-equal to compact = False in every output, on
    a throughput handle, which follows the working batch (cnl_set_active_batch)"""
    torch, DL, hipldl, syn = _mods()
    kind = K.METHOD_KINDS[method]
    ones = K.scalar_runs(K.family(**kind), ("nonlinear", method), method=method)
    assert set(K.col(ones, "status")) <= {"first_order", "small_residual"} and any(o["rejected"] > 0 and o["nbk"] > 0 for o in ones)
    assert len(set(K.col(ones, "iter"))) > 1                     # problems finish at different steps: there is something to compact
    fam = K.family("cuda:0", **kind)
    kw = dict(method=method, tuning={"plan_kind": hipldl.PLAN_THROUGHPUT})
    got = DL.solve_batch_device(fam, **kw)
    _same_decisions(got, ones, method)
    _close_solutions(got, ones, method)
    if method == "Newton_vanishing":
        assert got["hess_skipped"].tolist() == K.col(ones, "hess_skipped") and any(K.col(ones, "hess_skipped"))
    _compact_against(fam, got, method, True, **kw)


def test_loop_compaction_on_a_handle_that_keeps_its_batch(built):
    """300 variables, 4 constraints: the default handle of twelve problems runs staged and refuses cnl_set_active_batch, so behind a
    compaction it reads an H_c (and H_F) row for every problem it was created with — the padded arrays.  Against the host mirror, and
    compact on / off bit-equal."""
    torch, DL, hipldl, syn = _mods()
    ones = K.scalar_runs(K.staged_family(), "staged")
    assert set(K.col(ones, "status")) == {"first_order"} and len(set(K.col(ones, "iter"))) > 1
    assert any(o["rejected"] > 0 and o["nbk"] > 0 for o in ones)
    fam = K.staged_family("cuda:0")
    got = DL.solve_batch_device(fam)
    assert got["kernel"] == "v2-staged", got["kernel"]
    _same_decisions(got, ones, "staged")
    _close_solutions(got, ones, "staged")
    _compact_against(fam, got, "staged", False)


@pytest.mark.parametrize("name", list(RP.PROBLEMS))
def test_loop_on_the_reference_problems(built, name):
    """(F_linear, c_quad), (F_Rosen, c_quad), (F_larger(3), c_quad) and HS6 from both of its start points, as batches of 8 on the default
    Float64 handle: row 0 from the reference's start point reaches the answer the reference holds at its own atol = 1e-4, and every row
    takes the decisions of its host-mirror run"""
    torch, DL, hipldl, syn = _mods()
    ones = K.scalar_runs(RP.RefProblemFamily(name, 8, 1, torch, "cpu"), ("ref", name))
    assert set(K.col(ones, "status")) <= {"first_order", "small_residual"} and np.allclose(ones[0]["solution"], RP.PROBLEMS[name][5], atol=RP.REF_ATOL)
    fam = RP.RefProblemFamily(name, 8, 1, torch, "cuda:0")
    got = DL.solve_batch_device(fam)
    _same_decisions(got, ones, name)
    print(f"{name}: row 0 ends at {got['solution'][0].tolist()}, the reference holds {fam.answer}")
    assert np.allclose(got["solution"][0], fam.answer, atol=RP.REF_ATOL)
    assert got["jct_shared"] is False


def test_linear_family_keeps_one_constraint_jacobian(built):
    """a family without `linear_constraints` (BandQuadFamily) runs as before: Jct aliased to Jcv, and no callback beyond the old ones"""
    torch, DL, hipldl, syn = _mods()
    fam = DL.BandQuadFamily(syn.band_structure(K.N, K.P), K.BL, K.SEED, torch=torch, device="cuda:0")
    assert not hasattr(fam, "linear_constraints") and not hasattr(fam, "hess_cons_vals")
    got = DL.solve_batch_device(fam)
    assert got["jct_shared"] is True and set(got["status"]) == {"first_order"}
    assert DL.solve_batch_device(fam, compact=True, compact_min_finished=1)["jct_shared"] is True
    free = DL.BandQuadFamily(syn.band_structure(K.N, 0), K.BL, K.SEED, torch=torch, device="cuda:0")
    assert DL.solve_batch_device(free)["jct_shared"] is True
