"""The Float32 latency path (cnl_create_f32 with tuning float32_general = 1, float32_latency = 1, band_kernel = 0: the latency plan
of float32_staged shaped and run as a Float64 handle's — lean instances with backward rows, dataflow execution, the fused in-kernel
rho ladder and its commit / redo launch — on the float instances named last in csrc/kernels2.hip) against the fp64 oracle on the
widened float32 inputs with ParamCaNNOLeS(Float32) widened.  -m gpu.

`S.check` (tests/support/f32_staged.py) means, through hipldl.newton_system_: (success, nfact) identical to the oracle; rho, rho_old
and the rho slots of vals bit-equal to the oracle's rounded to float32; backward error <= 512 eps(Float32) and forward error <= 1e-3
(tests/support/f32_general.py: oracle_newton with its per-problem pivot-margin assertion, check_results; unchanged); a failed problem
leaves d untouched; every copy of a problem gives the bits of its first copy; the call counts one launch of the register-front
family (the commit / redo / skip_done launch behind the attempt) and none of the general kernel.  Every test here fails on a
library without the tuning key."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.support import f32_general as G
from tests.support import f32_latency as T
from tests.support import f32_staged as S
from tests.test_float32_general_gpu import MULTIPRECISION_ATOL

pytestmark = pytest.mark.gpu

CNL_ERR_ARG, CNL_ERR_STATE = 1, 5
bits = G.bits


def _facts(L, shape, B):
    ntasks, nstages, classes, lean = T.PLANS[(shape, B)]
    assert len(L.plan_array("tasks")) // 8 == ntasks and len(L.plan_array("stage_ptr")) - 1 == nstages
    assert (L.info["v2"]["fronts16"], L.info["v2"]["fronts32"], L.info["v2"]["fronts64"]) == classes
    assert T.back_rows(L.plan_array) == lean
    return ntasks


def _lad_mode(L, ntasks, B, fused=0):
    import torch
    return T.fused_launches(ntasks, B, T.resident_waves(torch, L.config), fused)


def _same_bits(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


# ---- parity against the oracle: lean plans, non-lean plans ----
CASES = [("hw2", 1), ("hw2", 13), ("hw2", 256), ("cfg4", 32), ("cfg4", 256), ("hw3", 13), ("hw3", 64)]


@pytest.mark.parametrize("shape,B", CASES, ids=[f"{k[0]}-{k[1]}" for k in CASES])
def test_clean_mixed_clean(built, shape, B):
    """hw2 and cfg4: lean plans (staged lean instances, the lean fused ladder, backward rows: no post-pass); hw3: class-32 fronts, so
    the non-lean instances with dataflow and the non-lean fused ladder.  A clean batch, then — same handle — climbers and a
    hopeless problem in one wavefront and a climber in another, then the clean batch again"""
    hipldl, syn, O = S.mods()
    s = S.structure(syn, shape)
    lean = T.PLANS[(shape, B)][3]
    L = T.handle(hipldl, s, B, lean)
    ntasks = _facts(L, shape, B)
    mode, launches = _lad_mode(L, ntasks, B)
    assert L.config["lad_mode"] == mode and (mode, launches) == (1, 1), (L.config, mode, launches)
    T.three_batches(hipldl, shape, B, L)
    L.close()


@pytest.mark.parametrize("shape", ["hw2", "hw3"])
def test_rho_old_positive(built, shape):
    hipldl, syn, O = S.mods()
    L = T.handle(hipldl, S.structure(syn, shape), 13, shape == "hw2", lad_mode=1)
    _, ref, _, _ = S.check(shape, "mixed", 13, rho_old=0.3, L=L)
    L.close()
    assert ref["ok"].all() and (ref["nf"][[1, 2, 3, 9]] == 5).all()


@pytest.mark.parametrize("shape,B", [("hw2", 13), ("hw3", 13)])
def test_first_attempt_inside_the_fused_launch(built, shape, B):
    """device_ladder_fused = 1 (lad_mode 2): first attempt, ladder and backward sweeps of the smallest batches in ONE launch of the
    fused float instance, lean and not; the same results, bit for bit, as the default (the fused ladder behind a staged attempt)"""
    hipldl, syn, O = S.mods()
    s = S.structure(syn, shape)
    lean = T.PLANS[(shape, B)][3]
    L = T.handle(hipldl, s, B, lean, device_ladder_fused=1)
    assert (L.config["lad_mode"], 1) == _lad_mode(L, _facts(L, shape, B), B, fused=1) == (2, 1)
    L1 = T.handle(hipldl, s, B, lean, lad_mode=1)
    a = S.check(shape, "mixed", B, L=L)
    b = S.check(shape, "mixed", B, L=L1)
    S.check(shape, "clean", B, L=L)
    L.close()
    L1.close()
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[2]), bits(b[2]))


# ---- the ladder rule ----
@pytest.mark.parametrize("shape,B", [("cfg4", 4096), ("late", 3840)])
def test_three_tasks_keep_the_sequential_ladder(built, shape, B):
    """cfg4 x 4 096: three tasks, and 1 024 groups of problems do not fit one fused launch — lad_mode 0, the problems that fail the
    attempt climb in the classic LEAN launch behind it (skip_done).  [added] band_structure(2600, 4) x 3 840: the chain the launch
    rule gives the LATE setting of the staged lean instance"""
    hipldl, syn, O = S.mods()
    L = T.handle(hipldl, S.structure(syn, shape), B, True, lad_mode=0)
    ntasks = _facts(L, shape, B)
    assert _lad_mode(L, ntasks, B)[0] == 0
    assert S.late_rule(B, L.plan_array("stage_ptr"), L.info["nsuper"]) == (shape == "late")
    _, ref, _, _ = S.check(shape, "clean", B, L=L)
    assert ref["ok"].all() and (ref["nf"] == 1).all()
    if shape == "cfg4":
        _, ref, _, (ok, nf, _) = S.check(shape, "mixed", B, L=L)
        assert int((~ok).sum()) == len(range(S.HOPELESS, B, S.NDISTINCT))
    L.close()


def test_more_than_one_fused_launch(built):
    """cfg4 x 281 (tests/support/f32_latency.py: the smallest such batch, found on the CPU): 29 tasks, 71 groups of problems — two
    fused launches on a device that holds 2 048 wavefronts; the expected count comes from this device's CU count"""
    hipldl, syn, O = S.mods()
    shape, B = T.MULTI_LAUNCH
    L = T.handle(hipldl, S.structure(syn, shape), B, True)
    ntasks = _facts(L, shape, B)
    mode, launches = _lad_mode(L, ntasks, B)
    if launches == 1:
        L.close()
        pytest.skip(f"this device holds the {ntasks} tasks of all {(B + 3) // 4} groups of problems in one fused launch")
    assert ntasks >= 16 and 2 <= launches <= 4 and mode == 1 and L.config["lad_mode"] == 1, (launches, L.config)
    print(f"cfg4 x {B}: {ntasks} tasks, {launches} fused launches")
    T.three_batches(hipldl, shape, B, L)
    L.close()


# ---- the switches ----
@pytest.mark.parametrize("shape", ["hw2", "hw3"])
def test_every_part_switched_off_is_the_float32_staged_handle(built, shape):
    hipldl, syn, O = S.mods()
    s = S.structure(syn, shape)
    B = 13
    vals, rhs = S.distinct_inputs(syn, s, "mixed")
    p32 = S.params(hipldl, True)
    off = T.handle(hipldl, s, B, False, df=False, lad_mode=0, **T.ALL_OFF)
    ref = S.handle(hipldl, s, B)
    assert off.config == ref.config and off.info == ref.info
    for name in ("perm", "rec", "brec", "tasks", "stage_ptr"):
        assert np.array_equal(off.plan_array(name), ref.plan_array(name)), name
    outs = []
    for H in (off, ref):
        c0 = hipldl.launch_counts()
        a = S.newton(hipldl, s, H, vals, rhs, np.zeros(B, np.float32), p32, fill=5.0)
        ok = hipldl.try_to_factorize(H, vals, s.nvar, s.nequ, s.ncon, p32[0])
        d = np.full((B, s.N), 7.0, np.float32)
        assert hipldl.solve_ldl_(rhs, H.factor, d) is True
        c1 = hipldl.launch_counts()
        outs.append((a + (np.asarray(ok), d), tuple(c1[k] - c0[k] for k in ("band", "register_front", "general"))))
        H.close()
    assert outs[0][1] == outs[1][1]
    _same_bits(outs[0][0], outs[1][0])


@pytest.mark.parametrize("shape,B", [("hw2", 13), ("hw3", 13), ("cfg4", 32)])
def test_dataflow_and_ladder_do_not_change_a_bit(built, shape, B):
    """dataflow = 0, device_ladder = 0 against both on: the same plan (asserted on its arrays), so every launch form runs the same
    arithmetic per front — one launch per stage and the classic ladder launch give the bits of dataflow and the fused ladder"""
    hipldl, syn, O = S.mods()
    s = S.structure(syn, shape)
    lean = T.PLANS[(shape, B)][3]
    v13, r13 = S.distinct_inputs(syn, s, "mixed")
    vals, rhs = S.tiled(v13, B), S.tiled(r13, B)
    p32 = S.params(hipldl, True)
    on = T.handle(hipldl, s, B, lean, lad_mode=1)
    off = T.handle(hipldl, s, B, lean, False, 0, **dict(dataflow=0, device_ladder=0))
    for name in ("perm", "rec", "brec", "tasks", "stage_ptr"):
        assert np.array_equal(on.plan_array(name), off.plan_array(name)), name
    outs = []
    for H in (on, off):
        a = S.newton(hipldl, s, H, vals, rhs, np.full(B, 0.0, np.float32), p32, fill=5.0)
        b = S.newton(hipldl, s, H, vals, rhs, np.full(B, 0.3, np.float32), p32, fill=5.0)
        outs.append(a + b)
        H.close()
    _same_bits(outs[0], outs[1])


# ---- two calls ----
@pytest.mark.parametrize("shape", ["hw2", "hw3"])
def test_factorize_then_two_solves(built, shape):
    """try_to_factorize with the inertia counts against the oracle's, then two solve_ldl_ with different right-hand sides: hw2 on the
    staged lean solve instance (backward rows, no post-pass), hw3 — class-32 fronts — off the register-front kernel; the device
    entries give the bits of the host entries; the first solve again behind the second gives its bits again"""
    import torch
    hipldl, syn, O = S.mods()
    s = S.structure(syn, shape)
    vals, rhs = S.distinct_inputs(syn, s, "mixed")
    B = vals.shape[0]
    p32 = S.params(hipldl)
    lean = shape == "hw2"
    L = T.handle(hipldl, s, B, lean)
    assert L.config["v2_solve"] == lean
    ok, npos, nzer = hipldl.try_to_factorize(L, vals, s.nvar, s.nequ, s.ncon, p32[0], return_inertia=True)
    orc = G.oracle_of(O, s)
    for b in range(B):
        ok0, np0, nz0 = orc.try_to_factorize(vals[b].astype(np.float64), s.nvar, s.nequ, s.ncon, float(p32[0]), return_inertia=True)
        assert (bool(ok[b]), int(npos[b]), int(nzer[b])) == (ok0, np0, nz0), b
    failed = sorted(S.CLIMBERS + (S.HOPELESS,))
    assert [b for b in range(B) if not ok[b]] == failed
    rhs2 = np.ascontiguousarray(rhs[::-1] * np.float32(0.5))
    host = []
    for r in (rhs, rhs2, rhs):
        d = np.full((B, s.N), 7.0, np.float32)
        assert hipldl.solve_ldl_(r, L.factor, d) is True
        host.append(d)
        for b in range(B):
            if b in failed:
                assert np.all(d[b] == 7.0), b
                continue
            d0 = -np.linalg.solve(syn.dense_kkt(s, vals[b].astype(np.float64)), r[b].astype(np.float64))
            assert G.backward_error(s, vals[b], r[b], d[b]) <= G.BWD_TOL, b
            assert np.abs(d[b] - d0).max() <= G.FWD_TOL * np.abs(d0).max(), b
    assert np.array_equal(bits(host[0]), bits(host[2]))
    # the device entries
    dev = torch.device("cuda", 0)
    tv = torch.from_numpy(vals).to(dev)
    tok = torch.zeros(B, dtype=torch.int32, device=dev)
    hipldl.factorize_dev(L, tv, p32[0], tok)
    torch.cuda.synchronize()
    assert np.array_equal(tok.cpu().numpy().astype(bool), np.asarray(ok, bool))
    for r, dh in ((rhs, host[0]), (rhs2, host[1])):
        tr = torch.from_numpy(r).to(dev)
        td = torch.full((B, s.N), 7.0, dtype=torch.float32, device=dev)
        hipldl.solve_dev(L, tr, td)
        torch.cuda.synchronize()
        # (solve_ldl! follows a successful factorisation: the device entry does not know which problems hold a factor, the host entry
        #  copies back only those that do)
        held = np.asarray(ok, bool)
        assert np.array_equal(bits(td.cpu().numpy()[held]), bits(dh[held]))
    L.close()


def _dev_newton(hipldl, torch, s, L, vals, rhs, p):
    B = vals.shape[0]
    dev = torch.device("cuda", 0)
    t = dict(v=torch.from_numpy(vals).to(dev), r=torch.from_numpy(rhs).to(dev), d=torch.full((B, s.N), 5.0, dtype=torch.float32, device=dev),
             ro=torch.zeros(B, dtype=torch.float32, device=dev), rho=torch.zeros(B, dtype=torch.float32, device=dev),
             nf=torch.zeros(B, dtype=torch.int32, device=dev), ok=torch.zeros(B, dtype=torch.int32, device=dev))
    hipldl.newton_system_dev(L, t["v"], t["r"], t["d"], t["ro"], t["rho"], t["nf"], t["ok"], p)
    torch.cuda.synchronize()
    return {k: x.cpu().numpy() for k, x in t.items()}


@pytest.mark.parametrize("shape", ["hw2", "hw3"])
def test_host_and_device_newton_agree_and_repeat(built, shape):
    """newton_system: the device entry gives the bits of the host entry, and the same call behind another one gives its bits again"""
    import torch
    hipldl, syn, O = S.mods()
    s = S.structure(syn, shape)
    vm, rm = S.distinct_inputs(syn, s, "mixed")
    vc, rc = S.distinct_inputs(syn, s, "clean")
    B = vm.shape[0]
    pm, pc = S.params(hipldl, True), S.params(hipldl)
    L = T.handle(hipldl, s, B, shape == "hw2", lad_mode=1)
    a = S.newton(hipldl, s, L, vm, rm, np.zeros(B, np.float32), pm, fill=5.0)
    g = _dev_newton(hipldl, torch, s, L, vm, rm, pm)
    S.newton(hipldl, s, L, vc[::-1].copy(), rc[::-1].copy(), np.full(B, 0.3, np.float32), pc, fill=1.0)
    c = S.newton(hipldl, s, L, vm, rm, np.zeros(B, np.float32), pm, fill=5.0)
    L.close()
    _same_bits(a, c)
    v, d, ok, rho, ro, nf = a
    assert np.array_equal(bits(g["d"]), bits(d)) and np.array_equal(bits(g["v"]), bits(v))
    assert np.array_equal(bits(g["rho"]), bits(rho)) and np.array_equal(bits(g["ro"]), bits(ro))
    assert np.array_equal(g["nf"], nf) and np.array_equal(g["ok"].astype(bool), ok)


# ---- the redo path ----
def test_a_wait_that_gives_up_is_counted_and_redone(built):
    """dataflow_spin_limit = 1 (as tests/test_gpu_parity.py does in Float64): practically every wait of the fused launch gives up —
    a bounded give-up handled in software: the waits are counted, nothing is committed, and the classic lean launch behind it
    (only_if_status) redoes the call from the caller's untouched inputs; then a normal call on a fresh handle"""
    hipldl, syn, O = S.mods()
    shape, B = "hw2", 13
    s = S.structure(syn, shape)
    L = T.handle(hipldl, s, B, True, lad_mode=1, dataflow_spin_limit=1)
    S.check(shape, "mixed", B, L=L)
    t1 = L.dataflow_timeouts()
    assert t1 > 0, "spin limit 1 did not make a single wait give up: the test does not test anything"
    # the two-call sequence on the same handle: the redo of try_to_factorize and of solve_ldl! (the classic lean solve instance)
    vals, rhs = S.distinct_inputs(syn, s, "clean")
    ok = hipldl.try_to_factorize(L, vals, s.nvar, s.nequ, s.ncon, S.params(hipldl)[0])
    assert np.asarray(ok, bool).all()
    d = np.full((B, s.N), 7.0, np.float32)
    assert hipldl.solve_ldl_(rhs, L.factor, d) is True
    for b in range(B):
        assert G.backward_error(s, vals[b], rhs[b], d[b]) <= G.BWD_TOL, b
    assert L.dataflow_timeouts() > t1
    L.close()
    L = T.handle(hipldl, s, B, True, lad_mode=1)
    S.check(shape, "mixed", B, L=L)
    assert L.dataflow_timeouts() == 0
    L.close()


# ---- leftover state ----
def test_results_do_not_depend_on_what_earlier_kernels_left(built):
    """two cases in a child process (tests/support/f32_latency.py as a script), once as it is and once with kernels in front of every
    launch that leave a byte pattern in LDS, scratch memory and the vector registers: the digests of every output are the same"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for fill in (None, "0xffffffff"):
        env = dict(os.environ)
        if fill:
            env.update(CNL_DBG_SCRATCHFILL="1", CNL_DBG_LDSFILL=fill)
        r = subprocess.run([sys.executable, "-m", "tests.support.f32_latency"], env=env, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
        lines = [ln for ln in r.stdout.splitlines() if ln and not ln.startswith("[")]
        assert lines[-1] == "done" and len(lines) == len(T.CASES) + 1, r.stdout[-1500:]
        outs.append(lines)
    assert outs[0] == outs[1], outs


# ---- fallbacks: the handle without the key, bit for bit ----
FALLBACKS = [("hw3-no-direct", (300, 4, 3), 12, {}), ("batch-4097", "hw2", 4097, {}), ("dense", "dense", 5, dict(float32_dense=1))]


@pytest.mark.parametrize("name,shape,B,opt", FALLBACKS, ids=[c[0] for c in FALLBACKS])
def test_fallbacks_are_the_handle_without_the_key(built, name, shape, B, opt):
    """a hw = 3 latency order without direct records, a batch above staged_max_batch, and a dense pattern float32_dense takes: the
    handle of float32_staged = 1 (whose fallbacks are the handle without either key), configuration and every output bit"""
    hipldl, syn, O = S.mods()
    ro = np.zeros(B, np.float32)
    if shape == "dense":   # the smallest case of the Float32 dense backend's tests
        from tests.support import f32_dense as FD
        c = FD.case(FD.SHAPES[0])
        s, vals, rhs, ro = c["s"], c["vals"][:B].copy(), c["rhs"][:B].copy(), c["rho_old"][:B].copy()
    elif isinstance(shape, tuple):
        s = syn.band_structure(shape[0], shape[1], hw=shape[2])
        vals, rhs = G.band_inputs(syn, s, range(4000, 4000 + B))
    else:
        s = S.structure(syn, shape)
        v13, r13 = S.distinct_inputs(syn, s, "mixed")
        vals, rhs = S.tiled(v13, B), S.tiled(r13, B)
    rows, cols = s.kkt_pattern()
    p32 = S.params(hipldl, True)
    outs, cfgs = [], []
    for keys in (T.KEYS, S.KEYS):
        L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32, options=hipldl.Options(**keys, **opt))
        assert L.config["float32"] and L.config["kernel"] != "v2-staged" and not L.config["lean"] and not L.config["dataflow"], L.config
        cfgs.append((L.config, L.info))
        v = vals.copy()
        outs.append((v,) + tuple(hipldl.newton_system_(np.full((B, s.N), 5.0, np.float32), s.nvar, s.nequ, s.ncon, rhs, v, L, ro, p32)))
        L.close()
    assert cfgs[0] == cfgs[1] and (cfgs[0][0]["kernel"] == "dense") == (shape == "dense")
    _same_bits(outs[0], outs[1])


# ---- refusals ----
def test_refusals_launch_nothing(built):
    hipldl, syn, O = S.mods()
    s = S.structure(syn, "hw2")
    rows, cols = s.kkt_pattern()
    L = T.handle(hipldl, s, 13, True)
    c0 = hipldl.launch_counts()
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.set_active_batch(L, 5)
    assert e.value.code == CNL_ERR_STATE and hipldl.get_active_batch(L) == 13
    L.close()

    def create(dtype=np.float32, **opt):
        return hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=13, dtype=dtype, options=hipldl.Options(**opt))

    for dtype, opt in ((np.float32, dict(float32_latency=1, band_kernel=0)), (np.float32, dict(float32_latency=1)),
                       (np.float64, dict(float32_latency=1)), (np.float64, dict(T.KEYS, float32_refine=1)),
                       (np.float32, dict(T.KEYS, float32_latency=2))):
        with pytest.raises(hipldl.CnlError) as e:
            create(dtype, **opt)
        assert e.value.code == CNL_ERR_ARG and "float32_latency" in str(e.value), opt
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.MultiHIPLDLStruct(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=13, devices=[0], options=hipldl.Options(float32_latency=1))
    assert e.value.code == CNL_ERR_ARG and "float32_latency" in str(e.value)
    assert hipldl.launch_counts() == c0


# ---- the lockstep loop ----
def test_lockstep_loop(built):
    """solve_batch_device on band_structure(300, 4, hw=2) with the key: per-problem status and iteration counts as without it, the
    solutions within the multiprecision tolerance of the reference loop"""
    import torch
    hipldl, syn, O = S.mods()
    from cannoles_jl_amd import device_loop as DL
    B = 12
    fam = DL.BandQuadFamily(syn.band_structure(300, 4, hw=2), B, seed=304, torch=torch, device="cuda:0", dtype=np.float32)
    got = DL.solve_batch_device(fam, tuning=dict(T.KEYS))
    base = DL.solve_batch_device(fam, tuning=dict(S.UNSTAGED))
    assert got["dtype"] == "float32" and got["kernel"] == "v2-staged" and base["kernel"] == "v2"
    assert got["status"] == base["status"] == ["first_order"] * B
    assert np.array_equal(got["iter"], base["iter"])
    dx = float(np.abs(got["solution"].astype(np.float64) - base["solution"].astype(np.float64)).max())
    dl = float(np.abs(got["multipliers"].astype(np.float64) - base["multipliers"].astype(np.float64)).max())
    print(f"float32 lockstep loop with float32_latency: max|dx| = {dx:.3e}, max|dlambda| = {dl:.3e} against the handle without the key, steps = {got['steps']}")
    assert dx <= MULTIPRECISION_ATOL and dl <= MULTIPRECISION_ATOL
