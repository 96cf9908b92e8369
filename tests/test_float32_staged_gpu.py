"""Staged execution of Float32 general handles (cnl_create_f32 with tuning float32_general = 1, float32_staged = 1, band_kernel = 0:
a latency plan on direct records, run stage by stage on the staged float instances of csrc/kernels2.hip — one launch per stage, no
dataflow, no in-kernel ladder; the problems that fail the first attempt climb the rho ladder in the classic float launch behind it)
against the fp64 oracle on the widened float32 inputs with ParamCaNNOLeS(Float32) widened.  -m gpu.

`check` (tests/support/f32_staged.py) means, through hipldl.newton_system_: (success, nfact) identical to the oracle; rho, rho_old and
the rho slots of vals bit-equal to the oracle's rounded to float32; backward error <= 512 eps(Float32) and forward error <= 1e-3
(tests/support/f32_general.py: oracle_newton with its per-problem pivot-margin assertion, check_results; unchanged); a failed problem
leaves d untouched; the handle reports float32, "v2-staged", direct and info["ncond"] > 0; the call counts one launch of the
register-front family (the launch behind the stages) and none of the general kernel.  Staged and unstaged handles sum in different
orders: between them only decisions are compared, never d.  Every test here fails on a library without the tuning key.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.support import f32_general as G
from tests.support import f32_register_front as R
from tests.support import f32_staged as S
from tests.test_float32_general_gpu import MULTIPRECISION_ATOL

pytestmark = pytest.mark.gpu

CNL_ERR_ARG, CNL_ERR_STATE = 1, 5
bits = G.bits


def _facts(L, shape, B):
    ntasks, nstages, classes, v2_solve = S.PLANS[(shape, B)]
    assert len(L.plan_array("tasks")) // 8 == ntasks and len(L.plan_array("stage_ptr")) - 1 == nstages
    assert (L.info["v2"]["fronts16"], L.info["v2"]["fronts32"], L.info["v2"]["fronts64"]) == classes
    assert L.config["v2_solve"] == v2_solve and L.config["wpb"] >= 1 and L.config["lds2_bytes"] > 0


# ---- parity against the oracle: every shape and batch ----
@pytest.mark.parametrize("shape,B", [k for k in S.PLANS if k[1] <= 256], ids=[f"{k[0]}-{k[1]}" for k in S.PLANS if k[1] <= 256])
def test_clean_and_mixed_batches(built, shape, B):
    """a clean batch (nfact = 1 everywhere), then — same handle — the batch with climbers and a hopeless problem inside the wavefront
    of problems 0 - 3 and a climber in another wavefront: the follow-up launch (skip_done) takes them through the ladder from its
    first rung; B = 1 and B = 13 leave lanes of the last wavefront without a problem, 256 fills whole wavefronts"""
    hipldl, syn, O = S.mods()
    s = S.structure(syn, shape)
    L = S.handle(hipldl, s, B)
    _facts(L, shape, B)
    _, ref, _, _ = S.check(shape, "clean", B, L=L)
    assert ref["ok"].all() and (ref["nf"] == 1).all()
    _, ref, _, _ = S.check(shape, "mixed", B, L=L)
    if B > S.HOPELESS:
        assert not ref["ok"][S.HOPELESS] and ref["nf"][S.HOPELESS] == 4 and ref["ok"][list(S.CLIMBERS[:2])].all() and (ref["nf"][1:3] == 4).all()
        assert ref["ok"].sum() == B - (B + S.NDISTINCT - 1 - S.HOPELESS) // S.NDISTINCT
    _, ref, _, _ = S.check(shape, "clean", B, L=L)   # ... and the clean batch again behind it
    L.close()


@pytest.mark.parametrize("shape", ["hw2", "hw3"])
def test_rho_old_positive(built, shape):
    _, ref, _, _ = S.check(shape, "mixed", 13, rho_old=0.3)
    assert ref["ok"].all() and (ref["nf"][[1, 2, 3, 9]] == 5).all()


@pytest.mark.parametrize("shape,B", [("cfg4", 4096), ("late", 3840)])
def test_bidirectional_chain(built, shape, B):
    """three tasks in two stages; launch_newton2_staged's rule (S.late_rule, from the host's facts) keeps the immediate stores for
    cfg4's 100 fronts and picks the LATE instance for the 260 fronts of the "late" shape"""
    hipldl, syn, O = S.mods()
    s = S.structure(syn, shape)
    L = S.handle(hipldl, s, B)
    _facts(L, shape, B)
    assert S.late_rule(B, L.plan_array("stage_ptr"), L.info["nsuper"]) == (shape == "late")
    _, ref, _, _ = S.check(shape, "clean", B, L=L)
    assert ref["ok"].all() and (ref["nf"] == 1).all()
    if shape == "cfg4":
        _, ref, _, (ok, nf, _) = S.check(shape, "mixed", B, L=L)
        assert int((~ok).sum()) == len(range(S.HOPELESS, B, S.NDISTINCT))
    L.close()


# ---- two calls ----
@pytest.mark.parametrize("shape", ["hw2", "hw3"])
def test_two_call_sequence(built, shape):
    """try_to_factorize with the inertia counts (staged_decide_kernel) against the oracle's, then two solve_ldl_ calls with different
    right-hand sides: staged on the shape whose fronts are all of the fast class (no launch counted), on the general kernel's float
    instance where class-32 fronts keep v2_solve false; failed problems keep their fill"""
    hipldl, syn, O = S.mods()
    s = S.structure(syn, shape)
    vals, rhs = S.distinct_inputs(syn, s, "mixed")
    B = vals.shape[0]
    p32 = S.params(hipldl)
    L = S.handle(hipldl, s, B)
    v2_solve = S.PLANS[(shape, B)][3]
    assert L.config["v2_solve"] == v2_solve
    c0 = hipldl.launch_counts()
    ok, npos, nzer = hipldl.try_to_factorize(L, vals, s.nvar, s.nequ, s.ncon, p32[0], return_inertia=True)
    R.launches(hipldl, c0)   # the stages and the decision: no launch of the three counted families
    orc = G.oracle_of(O, s)
    for b in range(B):
        ok0, np0, nz0 = orc.try_to_factorize(vals[b].astype(np.float64), s.nvar, s.nequ, s.ncon, float(p32[0]), return_inertia=True)
        assert (bool(ok[b]), int(npos[b]), int(nzer[b])) == (ok0, np0, nz0), b
    failed = sorted(S.CLIMBERS + (S.HOPELESS,))
    assert [b for b in range(B) if not ok[b]] == failed
    rhs2 = np.ascontiguousarray(rhs[::-1] * np.float32(0.5))
    for r in (rhs, rhs2):
        d = np.full((B, s.N), 7.0, np.float32)
        c0 = hipldl.launch_counts()
        assert hipldl.solve_ldl_(r, L.factor, d) is True
        R.launches(hipldl, c0, **({} if v2_solve else dict(general=1)))
        for b in range(B):
            if b in failed:
                assert np.all(d[b] == 7.0), b
                continue
            d0 = -np.linalg.solve(syn.dense_kkt(s, vals[b].astype(np.float64)), r[b].astype(np.float64))
            assert G.backward_error(s, vals[b], r[b], d[b]) <= G.BWD_TOL, b
            assert np.abs(d[b] - d0).max() <= G.FWD_TOL * np.abs(d0).max(), b
    L.close()


# ---- device entry ----
def _dev_run(hipldl, torch, s, L, vals, rhs, p, dtype=np.float32):
    B = vals.shape[0]
    dev = torch.device("cuda", 0)
    tt = torch.float32 if dtype == np.float32 else torch.float64
    t = dict(v=torch.from_numpy(vals.astype(dtype)).to(dev), r=torch.from_numpy(rhs.astype(dtype)).to(dev),
             d=torch.full((B, s.N), 5.0, dtype=tt, device=dev), ro=torch.zeros(B, dtype=tt, device=dev), rho=torch.zeros(B, dtype=tt, device=dev),
             nf=torch.zeros(B, dtype=torch.int32, device=dev), ok=torch.zeros(B, dtype=torch.int32, device=dev))
    c0 = hipldl.launch_counts()
    hipldl.newton_system_dev(L, t["v"], t["r"], t["d"], t["ro"], t["rho"], t["nf"], t["ok"], p)
    torch.cuda.synchronize()
    c1 = hipldl.launch_counts()
    return {k: x.cpu().numpy() for k, x in t.items()}, tuple(c1[k] - c0[k] for k in ("band", "register_front", "general"))


@pytest.mark.parametrize("shape", ["hw2", "hw3"])
def test_host_and_device_entry_points_agree(built, shape):
    import torch
    hipldl, syn, O = S.mods()
    s = S.structure(syn, shape)
    vals, rhs = S.distinct_inputs(syn, s, "mixed")
    B = vals.shape[0]
    p32 = S.params(hipldl, True)
    L = S.handle(hipldl, s, B)
    v, d, ok, rho, ro, nf = S.newton(hipldl, s, L, vals, rhs, np.zeros(B, np.float32), p32, fill=5.0)
    g, counts = _dev_run(hipldl, torch, s, L, vals, rhs, p32)
    L.close()
    assert counts == (0, 1, 0)
    assert np.array_equal(bits(g["d"]), bits(d)) and np.array_equal(bits(g["v"]), bits(v))
    assert np.array_equal(bits(g["rho"]), bits(rho)) and np.array_equal(bits(g["ro"]), bits(ro))
    assert np.array_equal(g["nf"], nf) and np.array_equal(g["ok"].astype(bool), ok)


@pytest.mark.parametrize("shape,B", [("hw2", 13), ("hw3", 64), ("cfg4", 256)])
def test_launch_counts_are_those_of_a_float64_staged_handle(built, shape, B):
    """newton_system! and try_to_factorize: no general-kernel launch, and the register-front family counts what a Float64 handle
    running one launch per stage (dataflow = 0, device_ladder = 0, lean_kernel = 0) counts for the same call, pattern and batch"""
    import torch
    hipldl, syn, O = S.mods()
    s = S.structure(syn, shape)
    v13, r13 = S.distinct_inputs(syn, s, "mixed")
    vals, rhs = S.tiled(v13, B), S.tiled(r13, B)
    rows, cols = s.kkt_pattern()
    L = S.handle(hipldl, s, B)
    L64 = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B,
                              options=hipldl.Options(dataflow=0, device_ladder=0, lean_kernel=0, band_kernel=0))
    assert L64.config["kernel"] == "v2-staged" and not L64.config["float32"] and not L64.config["lean"], L64.config
    got = []
    for H, dt in ((L, np.float32), (L64, np.float64)):
        p = hipldl.default_params(dt)
        p[6] = S.RHO_MAX_SMALL
        out, counts = _dev_run(hipldl, torch, s, H, vals, rhs, p, dt)
        dev = torch.device("cuda", 0)
        tv = torch.from_numpy(vals.astype(dt)).to(dev)
        tok = torch.zeros(B, dtype=torch.int32, device=dev)
        c0 = hipldl.launch_counts()
        hipldl.factorize_dev(H, tv, p[0], tok)
        torch.cuda.synchronize()
        c1 = hipldl.launch_counts()
        got.append((counts, tuple(c1[k] - c0[k] for k in ("band", "register_front", "general")), out["ok"].astype(bool), tok.cpu().numpy()))
    L.close()
    L64.close()
    assert got[0][0] == got[1][0] == (0, 1, 0) and got[0][1] == got[1][1] == (0, 0, 0)
    assert np.array_equal(got[0][3], got[1][3])   # try_to_factorize at rho = 0: the same decisions in both precisions


# ---- the same call twice, another case in between ----
@pytest.mark.parametrize("shape", ["hw2", "hw3"])
def test_repeated_call_is_bit_equal(built, shape):
    hipldl, syn, O = S.mods()
    s = S.structure(syn, shape)
    B = 13
    L = S.handle(hipldl, s, B)
    vm, rm = S.distinct_inputs(syn, s, "mixed")
    vc, rc = S.distinct_inputs(syn, s, "clean")
    pm, pc = S.params(hipldl, True), S.params(hipldl)
    a = S.newton(hipldl, s, L, vm, rm, np.zeros(B, np.float32), pm, fill=5.0)
    S.newton(hipldl, s, L, vc[::-1].copy(), rc[::-1].copy(), np.full(B, 0.3, np.float32), pc, fill=1.0)
    c = S.newton(hipldl, s, L, vm, rm, np.zeros(B, np.float32), pm, fill=5.0)
    L.close()
    for x, y in zip(a, c):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


def test_results_do_not_depend_on_what_earlier_kernels_left(built):
    """four cases in a child process (tests/support/f32_staged.py as a script), once as it is and once with kernels in front of every
    launch that leave a byte pattern in LDS, scratch memory and the vector registers: the digests of every output are the same"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for fill in (None, "0xffffffff"):
        env = dict(os.environ)
        if fill:
            env.update(CNL_DBG_SCRATCHFILL="1", CNL_DBG_LDSFILL=fill)
        r = subprocess.run([sys.executable, "-m", "tests.support.f32_staged"], env=env, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
        lines = [ln for ln in r.stdout.splitlines() if ln and not ln.startswith("[")]
        assert lines[-1] == "done" and len(lines) == len(S.CASES) + 1, r.stdout[-1500:]
        outs.append(lines)
    assert outs[0] == outs[1], outs


# ---- fallbacks: the handle without the key, bit for bit ----
FALLBACKS = [("no-tasks", "class64", 13, {}), ("batch-4097", "hw2", 4097, {}), ("throughput", "hw2", 13, dict(plan_kind=1))]


@pytest.mark.parametrize("name,shape,B,opt", FALLBACKS, ids=[c[0] for c in FALLBACKS])
def test_fallbacks_are_the_handle_without_the_key(built, name, shape, B, opt):
    hipldl, syn, O = S.mods()
    if shape == "class64":
        s = R.class64(syn)
        vals, rhs = R.mixed_batch(syn, s)
        vals, rhs = vals[:B].copy(), rhs[:B].copy()
    else:
        s = S.structure(syn, shape)
        v13, r13 = S.distinct_inputs(syn, s, "mixed")
        vals, rhs = S.tiled(v13, B), S.tiled(r13, B)
    p32 = S.params(hipldl, True)
    outs, cfgs = [], []
    for keys in (S.KEYS, S.UNSTAGED):
        L = S.handle(hipldl, s, B, staged=False, keys=keys, **opt)
        cfgs.append((L.config, L.info))
        outs.append(S.newton(hipldl, s, L, vals, rhs, np.zeros(B, np.float32), p32, fill=5.0))
        L.close()
    assert cfgs[0] == cfgs[1]
    for x, y in zip(*outs):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


# ---- refusals ----
def test_refusals_launch_nothing(built):
    hipldl, syn, O = S.mods()
    s = S.structure(syn, "hw2")
    rows, cols = s.kkt_pattern()
    L = S.handle(hipldl, s, 13)
    c0 = hipldl.launch_counts()
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.set_active_batch(L, 5)
    assert e.value.code == CNL_ERR_STATE and hipldl.get_active_batch(L) == 13
    hipldl.set_active_batch(L, 13)   # the created batch: nothing to change
    L.close()

    def create(dtype=np.float32, **opt):
        return hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=13, dtype=dtype, options=hipldl.Options(**opt))

    for dtype, opt in ((np.float32, dict(S.KEYS, batch_layout=hipldl.LAYOUT_INTERLEAVED)), (np.float32, dict(float32_staged=1, band_kernel=0)),
                       (np.float32, dict(float32_staged=1)), (np.float64, dict(float32_staged=1)),
                       (np.float64, dict(S.KEYS, float32_refine=1)), (np.float32, dict(S.KEYS, float32_staged=2))):
        with pytest.raises(hipldl.CnlError) as e:
            create(dtype, **opt)
        assert e.value.code == CNL_ERR_ARG, opt
        if "batch_layout" not in opt:
            assert "float32_staged" in str(e.value), opt
    assert hipldl.launch_counts() == c0
    sb = syn.band_structure(400, 4)   # band kernels first: a pattern they serve keeps its band handle
    rb, cb = sb.kkt_pattern()
    Lb = hipldl.HIPLDLStruct(sb.N, rb, cb, None, sb.nvar, sb.nequ, sb.ncon, batch=4, dtype=np.float32,
                             options=hipldl.Options(float32_general=1, float32_staged=1))
    assert Lb.config["band"] and Lb.config["kernel"] == "band"
    Lb.close()


# ---- the lockstep loop ----
def test_lockstep_loop(built):
    """BandQuadFamily(band_structure(300, 4, hw=3), 12) with the key: the latency order of this pattern gets no direct records (the
    CPU test asserts it, and that a Float64 handle falls back alike), so the loop runs on the handle without the key ("v2") —
    unchanged, which is the property; the staged handle in the loop is the next test"""
    import torch
    hipldl, syn, O = S.mods()
    from cannoles_jl_amd import device_loop as DL, outer_loop
    from tests.test_oracle_pinning import oracle_newton, oracle_solver
    B = 12
    tuning = dict(float32_general=1, float32_staged=1)
    fam = DL.BandQuadFamily(syn.band_structure(300, 4, hw=3), B, seed=304, torch=torch, device="cuda:0", dtype=np.float32)
    got = DL.solve_batch_device(fam, tuning=tuning)
    assert got["dtype"] == "float32" and got["kernel"] == "v2" and got["vals_layout"] == "problem-major"
    assert got["status"] == ["first_order"] * B
    prm = hipldl.default_params()
    dx = dl = 0.0
    for b in range(B):
        one = outer_loop.solve(fam.host_model(b), oracle_solver, oracle_newton, prm)
        assert one["status"] == "first_order"
        dx = max(dx, float(np.abs(got["solution"][b].astype(np.float64) - one["solution"]).max()))
        dl = max(dl, float(np.abs(got["multipliers"][b].astype(np.float64) - one["multipliers"]).max()))
    print(f"float32 lockstep loop with the key: max|dx| = {dx:.3e}, max|dlambda| = {dl:.3e}, steps = {got['steps']}")
    assert dx <= MULTIPRECISION_ATOL and dl <= MULTIPRECISION_ATOL
    cp = DL.solve_batch_device(fam, tuning=tuning, compact=True, compact_min_finished=1)
    assert cp["kernel"] == "v2" and cp["status"] == got["status"]
    assert np.array_equal(bits(cp["solution"]), bits(got["solution"]))
    assert np.array_equal(bits(cp["multipliers"]), bits(got["multipliers"]))


def test_lockstep_loop_on_a_staged_handle(built):
    """[added] the same loop where the handle really runs staged (band_structure(300, 4, hw=2), band_kernel = 0): it refuses to
    shrink, and compact=True goes on with the whole batch — bit-equal solutions"""
    import torch
    hipldl, syn, O = S.mods()
    from cannoles_jl_amd import device_loop as DL, outer_loop
    from tests.test_oracle_pinning import oracle_newton, oracle_solver
    B = 12
    tuning = dict(S.KEYS)
    fam = DL.BandQuadFamily(syn.band_structure(300, 4, hw=2), B, seed=304, torch=torch, device="cuda:0", dtype=np.float32)
    got = DL.solve_batch_device(fam, tuning=tuning)
    assert got["dtype"] == "float32" and got["kernel"] == "v2-staged" and got["vals_layout"] == "problem-major"
    assert got["status"] == ["first_order"] * B
    prm = hipldl.default_params()
    dx = dl = 0.0
    for b in range(B):
        one = outer_loop.solve(fam.host_model(b), oracle_solver, oracle_newton, prm)
        assert one["status"] == "first_order"
        dx = max(dx, float(np.abs(got["solution"][b].astype(np.float64) - one["solution"]).max()))
        dl = max(dl, float(np.abs(got["multipliers"][b].astype(np.float64) - one["multipliers"]).max()))
    print(f"float32 lockstep loop on the staged handle: max|dx| = {dx:.3e}, max|dlambda| = {dl:.3e}, steps = {got['steps']}")
    assert dx <= MULTIPRECISION_ATOL and dl <= MULTIPRECISION_ATOL
    cp = DL.solve_batch_device(fam, tuning=tuning, compact=True, compact_min_finished=1)
    assert cp["kernel"] == "v2-staged" and cp["status"] == got["status"]
    assert np.array_equal(bits(cp["solution"]), bits(got["solution"]))
    assert np.array_equal(bits(cp["multipliers"]), bits(got["multipliers"]))
