"""The general kernel's subtree execution in float (tuning float32_subtrees: csrc/kernels.hip, newton_subtrees instantiated for float —
on a Float32 general handle one workgroup per problem and task of the elimination tree, a launch per stage) against the fp64 oracle on
the widened float data and against the same handle with the key off.  -m gpu.

Inputs, reference and bars are those of tests/support/f32_subtrees_cases.py: the Float32 five-kind mix of
tests/support/f32_general_dense.py on the shapes of tests/support/general_subtrees_cases.py, the oracle on the canonical order and on
the handle's own, BWD_TOL / FWD_TOL of tests/support/f32_general.py; tests/test_float32_subtrees_cpu.py vouches for the cut of every
plan used here and for the Float32 margin of every rung, so no test skips or reclassifies a problem.  Everything goes through
cnl_newton_system_f32_dev with sentinels in d unless the test says otherwise.  Decisions (success, nfact, rho, rho_old, the rho slots)
are compared bit for bit; d within the bars."""
import numpy as np
import pytest

from tests.support import f32_general as G
from tests.support import f32_subtrees_cases as FS

pytestmark = pytest.mark.gpu
CNL_ERR_ARG = 1


def _mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    return hipldl, syn


def _base(cond):
    return FS.COND if cond else FS.UNCOND


def _stages(L):
    return len(L.plan_array("gstage_ptr")) - 1


def _call(hipldl, c, L, idx):
    A = FS.GD.Args(c["s"], len(idx))
    A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
    A.call(hipldl, L, c["p32"])
    return A.read()


def _assert_on_the_route(L, blocked):
    cfg = L.config
    assert cfg["kernel"] == "v1" and cfg["float32"] and not cfg["band"], cfg
    assert cfg["float32_subtrees"] and not cfg["general_subtrees"] and not cfg["general_blocked"], cfg      # (bits 49 / 47 stay Float64-only)
    assert cfg["tpp"] == 256 and cfg["ppb"] == 1 and not cfg["lds_work"] and cfg["lds_bytes"] == 16 * 4, cfg
    assert cfg["float32_blocked"] == bool(blocked), cfg


def _run_mix(hipldl, c, L, blocked=0, idxs=None):
    """one cnl_newton_system_f32_dev call per order of the case's problems (forwards and reversed), each against the oracle on the
    canonical order and on the handle's own; the configuration is asserted FIRST, the launch count 2 S + 2 on every call.  Returns the
    outputs of the forward call."""
    B = len(c["vals"])
    _assert_on_the_route(L, blocked)
    refs = [c, FS.oracle_on(L.plan_array("perm").astype(np.int64), c)]
    first = None
    for idx in (idxs or (np.arange(B), np.arange(B)[::-1])):
        before = hipldl.launch_counts()["general"]
        out = _call(hipldl, c, L, idx)
        assert hipldl.launch_counts()["general"] - before == 2 * _stages(L) + 2      # S forward, decide, S backward, the climbers
        for ref in refs:
            be, fe = FS.check_outputs(ref, out, idx, c["vals"][idx])
        print(f"stages {_stages(L)} blocked {blocked}: ok {out['ok'].tolist()} nfact {out['nf'].tolist()} backward {be / FS.EPS32:.1f} eps32 forward {fe:.2e}")
        first = first or out
    return first


def _handle(hipldl, c, B, cond, cap, blocked=0, forced=True, **extra):
    opt = dict(_base(cond), **FS.KEY, float32_blocked=blocked, **extra)
    if cap:
        opt["task_cap"] = cap
    if forced:
        opt.update(FS.FORCED)
    return FS.handle(hipldl, c, B, **opt)


def _assert_cut(L, shape, cond, cap):
    assert tuple(FS.ginfo(L)[1:4]) == FS.CUT[shape, cond, cap] and L.info["fmax"] == FS.FMAX[shape][0 if cond else 1], (FS.ginfo(L), L.info["fmax"])


# ---- 1. the mix against the oracle ----
@pytest.mark.parametrize("cond", (True, False), ids=("condensed", "uncondensed"))
@pytest.mark.parametrize("cap", (4, 8))
@pytest.mark.parametrize("shape", (FS.GRID12, FS.GRID16), ids=FS.shape_id)
def test_grids(built, shape, cap, cond):
    hipldl, syn = _mods()
    c = FS.case(shape)
    L = _handle(hipldl, c, FS.MIX, cond, cap)
    _assert_cut(L, shape, cond, cap)
    _run_mix(hipldl, c, L)
    L.close()


@pytest.mark.parametrize("cond", (True, False), ids=("condensed", "uncondensed"))
@pytest.mark.parametrize("blocked", (0, 1), ids=("unblocked", "blocked"))
def test_grid32_with_and_without_blocked_panels(built, blocked, cond):
    """grid_structure(32) at cap 8: the separator fronts (21, 62), (31, 63) and the root (93, 0) are single-front tasks above the cut,
    eliminated in panels on the f32 matrix cores where float32_blocked = 1; uncondensed, (16, 13, 11) is a blocked front INSIDE a
    bottom task"""
    hipldl, syn = _mods()
    c = FS.case(FS.GRID32)
    L = _handle(hipldl, c, FS.MIX, cond, 8, blocked)
    _assert_cut(L, FS.GRID32, cond, 8)
    fr = [tuple(int(x) for x in f[[0, 1, 14]]) for f in L.plan_array("fronts").reshape(-1, 16)]
    for w in [(21, 62, 0), (31, 63, 0), (93, 0, 0)] + ([] if cond else [(16, 13, 11)]):
        assert w in fr, w
    t = L.plan_array("gtasks").reshape(-1, 8)

    def fronts_of_the_task_of(w):
        k = fr.index(w)
        f0, f1 = t[(t[:, 1] <= k) & (k < t[:, 2])][0, 1:3]
        return int(f1 - f0)

    assert fronts_of_the_task_of((93, 0, 0)) == 1 and (cond or fronts_of_the_task_of((16, 13, 11)) > 1)
    _run_mix(hipldl, c, L, blocked)
    L.close()


@pytest.mark.parametrize("shape,cond,cap,blocked", [(FS.FOREST3, True, 4, 0), (FS.FOREST3, False, 8, 0), (FS.FOREST4, True, 4, 0), (FS.FOREST4, False, 8, 1)],
                         ids=lambda v: FS.shape_id(v) if isinstance(v, tuple) else str(v))
def test_forests(built, shape, cond, cap, blocked):
    """three and four roots: several tasks without a parent, the last stages short"""
    hipldl, syn = _mods()
    c = FS.case(shape)
    L = _handle(hipldl, c, FS.MIX, cond, cap, blocked)
    _assert_cut(L, shape, cond, cap)
    fr = L.plan_array("fronts").reshape(-1, 16)
    assert (fr[:, 11] < 0).sum() == (4 if shape == FS.FOREST4 else 3)
    _run_mix(hipldl, c, L, blocked)
    L.close()


def test_chain_like_tree_under_the_default_configuration(built):
    """(450, 300, 4, 0.02, 1), float32_blocked = 1: largest front 375, so 256 threads per problem by choose_config itself; 18 bottom
    subtrees under eight more stages"""
    hipldl, syn = _mods()
    c = FS.case(FS.CHAIN)
    L = _handle(hipldl, c, FS.MIX, True, 0, 1, forced=False)
    _assert_cut(L, FS.CHAIN, True, 8)
    _run_mix(hipldl, c, L, 1)
    L.close()


# ---- 2. key on against key off ----
@pytest.mark.parametrize("shape,cond,cap,blocked", [(FS.GRID16, True, 8, 0), (FS.GRID16, False, 4, 0), (FS.FOREST4, True, 4, 0), (FS.GRID32, True, 8, 1)],
                         ids=lambda v: FS.shape_id(v) if isinstance(v, tuple) else str(v))
def test_key_on_against_key_off(built, shape, cond, cap, blocked):
    """the same shape, 256 threads per problem and the work area in global scratch on both sides: decisions bit-equal, d within
    FWD_TOL of each other; the per-front arithmetic is the same source, and the test prints whether d is bit-equal"""
    hipldl, syn = _mods()
    c = FS.case(shape)
    s, B = c["s"], FS.MIX
    outs = []
    for key in (1, 0):
        L = FS.handle(hipldl, c, B, **_base(cond), **FS.FORCED, v1_lds=0, task_cap=cap, float32_blocked=blocked, float32_subtrees=key)
        cfg = L.config
        assert cfg["float32_subtrees"] == bool(key) and cfg["kernel"] == "v1" and cfg["tpp"] == 256 and not cfg["lds_work"] and cfg["float32_blocked"] == bool(blocked), cfg
        outs.append(_call(hipldl, c, L, np.arange(B)))
        FS.check_outputs(c, outs[-1], np.arange(B), c["vals"])
        L.close()
    on, off = outs
    for k in ("ok", "nf"):
        assert np.array_equal(on[k], off[k]), k
    for k in ("rho", "ro", "vals"):
        assert np.array_equal(FS.bits(on[k]), FS.bits(off[k])), k
    worst, bit_equal = 0.0, True
    for b in range(B):
        if not on["ok"][b]:
            assert (on["d"][b] == 7.0).all() and (off["d"][b] == 7.0).all()
            continue
        bit_equal &= bool(np.array_equal(FS.bits(on["d"][b]), FS.bits(off["d"][b])))
        fe = np.abs(on["d"][b].astype(np.float64) - off["d"][b]).max() / np.abs(off["d"][b]).max()
        worst = max(worst, fe)
        assert fe <= FS.FWD_TOL, (b, fe)
    print(f"{FS.shape_id(shape)} cond {cond} cap {cap} blocked {blocked}: d with the key on against off: bit-equal {bit_equal}, worst {worst:.2e}")


# ---- 3. the two-call sequence ----
@pytest.mark.parametrize("cond", (True, False), ids=("condensed", "uncondensed"))
def test_two_call_sequence_inertia_and_failed_rows(built, cond):
    """cnl_factorize_f32_dev (S + 1 launches: the stages and the decide kernel), then cnl_solve_f32_dev twice with different right-hand
    sides on that factor (2 S launches each): the solutions within BWD_TOL, vals untouched, the rows of d of the problems without a
    factor — the hopeless one and the two climbers, which try_to_factorize does not repair — at their 7.0 sentinel; then the host
    try_to_factorize with the inertia, equal to the oracle's counts on the widened data."""
    import torch
    from oracle import oracle as O
    hipldl, syn = _mods()
    c = FS.case(FS.GRID12)
    s, B = c["s"], FS.MIX
    eig_tol = float(c["p32"][0])
    orc = G.oracle_of(O, s)
    ref = [orc.try_to_factorize(c["vals"][b].astype(np.float64), s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True) for b in range(B)]
    want = [bool(r[0]) for r in ref]
    assert want == [True, False, False, False, True]
    L = _handle(hipldl, c, B, cond, 4)
    _assert_on_the_route(L, 0)
    S = _stages(L)
    dev = "cuda:0"
    t_vals = torch.from_numpy(np.array(c["vals"])).to(dev)
    t_ok = torch.full((B,), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    n0 = hipldl.launch_counts()["general"]
    hipldl.factorize_dev(L, t_vals, eig_tol, t_ok, stream=stream)
    assert hipldl.launch_counts()["general"] - n0 == S + 1
    for k in range(2):
        r = np.ascontiguousarray(c["rhs"] * np.float32(k + 1.5))
        t_r = torch.from_numpy(r).to(dev)
        t_d = torch.full((B, s.N), 7.0, dtype=torch.float32, device=dev)
        n0 = hipldl.launch_counts()["general"]
        hipldl.solve_dev(L, t_r, t_d, stream=stream)
        assert hipldl.launch_counts()["general"] - n0 == 2 * S
        torch.cuda.synchronize()
        assert t_ok.cpu().numpy().tolist() == [int(w) for w in want]
        d = t_d.cpu().numpy()
        for b in range(B):
            if want[b]:
                be = G.backward_error(s, c["vals"][b], r[b], d[b])
                assert be <= FS.BWD_TOL, (b, k, be)
            else:
                assert (d[b] == 7.0).all(), b      # no factor: the rows stay untouched
    assert np.array_equal(FS.bits(t_vals.cpu().numpy()), FS.bits(c["vals"]))
    ok, npos, nzer = hipldl.try_to_factorize(L, np.array(c["vals"]), s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True)
    assert list(ok) == want
    for b in range(B):
        if b % 5 != 1:     # (the hopeless problem's pivots are NaN: its counts mean nothing in either arithmetic)
            assert (int(npos[b]), int(nzer[b])) == (int(ref[b][1]), int(ref[b][2])), b
    L.close()


# ---- 4. batches ----
def test_batch_of_one(built):
    """one problem, one workgroup per task: the healthy problem and the first climber"""
    hipldl, syn = _mods()
    c = FS.case(FS.GRID12)
    L = _handle(hipldl, c, 1, True, 4)
    out = _run_mix(hipldl, c, L, idxs=(np.array([0]), np.array([2])))
    assert out["ok"].tolist() == [1] and out["nf"].tolist() == [1]
    L.close()


def test_batch_of_65_and_an_active_prefix(built):
    """65 different problems (thirteen mixes); then cnl_set_active_batch on the first 20: the calls run on the prefix and leave the
    arrays of the others alone, the flags kept behind the factorisation are those of the prefix, and solve leaves its failed rows
    untouched"""
    import torch
    hipldl, syn = _mods()
    c = FS.case(FS.GRID12, 65)
    s, B, nb = c["s"], 65, 20
    L = _handle(hipldl, c, B, True, 4)
    out = _run_mix(hipldl, c, L)
    assert out["ok"].tolist() == [int(FS.WANT_OK[b % 5]) for b in range(B)] and out["nf"].tolist() == [FS.WANT_NF[b % 5] for b in range(B)]
    hipldl.set_active_batch(L, nb)
    part = _call(hipldl, c, L, np.arange(B))      # (arrays of the whole batch, sentinels everywhere)
    FS.check_outputs(c, {k: v[:nb] for k, v in part.items()}, np.arange(nb), c["vals"][:nb])
    assert (part["d"][nb:] == 7.0).all() and (part["ok"][nb:] == -1).all() and (part["nf"][nb:] == -1).all() and (part["rho"][nb:] == -1.0).all()
    assert np.array_equal(FS.bits(part["vals"][nb:]), FS.bits(c["vals"][nb:]))
    for k in ("ok", "nf", "rho", "ro", "d"):
        assert np.ascontiguousarray(part[k][:nb]).tobytes() == np.ascontiguousarray(out[k][:nb]).tobytes(), k
    dev = "cuda:0"
    stream = torch.cuda.current_stream().cuda_stream
    t_vals = torch.from_numpy(np.array(c["vals"])).to(dev)
    t_ok = torch.full((B,), -1, dtype=torch.int32, device=dev)
    hipldl.factorize_dev(L, t_vals, float(c["p32"][0]), t_ok, stream=stream)
    t_r = torch.from_numpy(np.array(c["rhs"])).to(dev)
    t_d = torch.full((B, s.N), 7.0, dtype=torch.float32, device=dev)
    hipldl.solve_dev(L, t_r, t_d, stream=stream)
    torch.cuda.synchronize()
    ok, d = t_ok.cpu().numpy(), t_d.cpu().numpy()
    assert ok.tolist() == [[1, 0, 0, 0, 1][b % 5] for b in range(nb)] + [-1] * (B - nb)
    for b in range(B):
        if b < nb and ok[b] == 1:
            assert G.backward_error(s, c["vals"][b], c["rhs"][b], d[b]) <= FS.BWD_TOL, b
        else:
            assert (d[b] == 7.0).all(), b
    hipldl.set_active_batch(L, B)
    L.close()


def test_host_entry_on_a_batch_of_the_chunking_size(built):
    """The host-pointer cnl_newton_system_f32 on the mix on grid_structure(12) repeated to the size at which the host entry of a
    Float64 handle cuts a batch into sub-batch views (96 MB and more of input — counted here with 4-byte elements —, at least 32
    problems): every problem at its own offset into the factor panels, the task regions and the tasks' count slots.  The first mix
    against the oracle; every repetition bit-equal to the first.  The call runs stage by stage however many views it is cut into: the
    launches are a multiple of 2 S + 2, and the test prints how many views there were (a Float32 host-pointer call is the device
    entry behind one upload: one)."""
    hipldl, syn = _mods()
    c = FS.case(FS.GRID12)
    s = c["s"]
    per = (s.nnzNS + s.N) * FS.ESZ
    reps = -(-(96 << 20) // (FS.MIX * per))
    B = FS.MIX * reps
    assert B >= 32 and B * per >= (96 << 20) and max(16, ((B // 8) + 3) & ~3) < B       # the rule of cnl_newton_system
    L = _handle(hipldl, c, B, True, 4)
    _assert_on_the_route(L, 0)
    vals, rhs, ro = (np.ascontiguousarray(np.tile(c[k], (reps,) + (1,) * (c[k].ndim - 1))) for k in ("vals", "rhs", "rho_old"))
    before = hipldl.launch_counts()["general"]
    d, ok, rho, ro_out, nf = hipldl.newton_system_(np.full((B, s.N), 7.0, np.float32), s.nvar, s.nequ, s.ncon, rhs, vals, L, ro, c["p32"])
    launches, per_call = hipldl.launch_counts()["general"] - before, 2 * _stages(L) + 2
    assert launches >= per_call and launches % per_call == 0, (launches, per_call)
    print(f"{B} problems, {B * per >> 20} MB of input: {launches // per_call} view(s), {launches} launches")
    out = dict(vals=vals, d=d, ok=np.asarray(ok).astype(np.int32), rho=rho, ro=ro_out, nf=np.asarray(nf))
    FS.check_outputs(c, {k: v[:FS.MIX] for k, v in out.items()}, np.arange(FS.MIX), c["vals"])
    for k, v in out.items():
        rep = np.asarray(v).reshape((reps, FS.MIX) + np.asarray(v).shape[1:])
        assert np.ascontiguousarray(rep).tobytes() == np.ascontiguousarray(np.broadcast_to(rep[:1], rep.shape)).tobytes(), k
    L.close()


# ---- 5. what earlier launches left in the task regions ----
def test_results_do_not_depend_on_what_the_scratch_holds(built):
    """The mix, then a call on OTHER values (every problem's kind shifted by three and scaled, so that every region of every problem —
    stack, panel buffer, staging rows, count slots — holds another problem's numbers, NaN among them), then the mix again: bit-equal
    to the first call in every output."""
    hipldl, syn = _mods()
    c = FS.case(FS.GRID16)
    s, B = c["s"], FS.MIX
    L = _handle(hipldl, c, B, True, 4, 1)
    first = _run_mix(hipldl, c, L, 1)        # (its second call ran the problems in reversed order)
    A = FS.GD.Args(s, B)
    idx = (np.arange(B) + 3) % B
    A.fill(c["vals"][idx] * np.float32(3.0), c["rhs"][idx], c["rho_old"][idx])
    A.call(hipldl, L, c["p32"])
    A.read()
    again = _call(hipldl, c, L, np.arange(B))
    for k in first:
        assert np.ascontiguousarray(first[k]).tobytes() == np.ascontiguousarray(again[k]).tobytes(), k
    L.close()


# ---- 6. handles the key does not act on run as without it, and say so ----
@pytest.mark.parametrize("name,opt,tpp", [("64-threads", dict(task_cap=4), 64), ("single-task", dict(FS.FORCED, task_cap=1000), 256)])
def test_general_kernel_handles_the_key_does_not_act_on(built, name, opt, tpp):
    """grid_structure(12), fmax 34: 64 threads per problem by choose_config (no float subtree instance), and a cut of one task at
    256 threads — one classic launch per call, the same configuration word for word, the same bits"""
    hipldl, syn = _mods()
    c = FS.case(FS.GRID12)
    B = FS.MIX
    outs, cfgs = [], []
    for key in (1, 0):
        L = FS.handle(hipldl, c, B, **FS.COND, **opt, float32_subtrees=key)
        assert not L.config["float32_subtrees"] and L.config["kernel"] == "v1" and L.config["tpp"] == tpp, L.config
        cfgs.append(L.config)
        before = hipldl.launch_counts()["general"]
        outs.append(_call(hipldl, c, L, np.arange(B)))
        assert hipldl.launch_counts()["general"] - before == 1
        FS.check_outputs(c, outs[-1], np.arange(B), c["vals"])
        L.close()
    assert cfgs[0] == cfgs[1]
    for k in outs[0]:
        assert np.ascontiguousarray(outs[0][k]).tobytes() == np.ascontiguousarray(outs[1][k]).tobytes(), k


def _same_with_and_without(hipldl, s, vals, rhs, base, kernel):
    rows, cols = s.kkt_pattern()
    B = vals.shape[0]
    p32 = hipldl.default_params(np.float32)
    res, cfgs = [], []
    for extra in ({}, FS.KEY):
        L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32, options=hipldl.Options(**base, **extra))
        assert not L.config["float32_subtrees"] and L.config["kernel"] == kernel, L.config
        cfgs.append(L.config)
        v = vals.copy()
        d, ok, rho, ro_out, nf = hipldl.newton_system_(np.full((B, s.N), 7.0, np.float32), s.nvar, s.nequ, s.ncon, rhs.copy(), v, L, np.zeros(B, np.float32), p32)
        res.append(dict(vals=v, d=d, ok=np.asarray(ok).astype(np.int32), rho=rho, ro=ro_out, nf=np.asarray(nf)))
        L.close()
    assert cfgs[0] == cfgs[1] and res[0]["ok"].all()
    for name, a in res[0].items():
        b = res[1][name]
        assert a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), name


def test_other_routes_are_what_they_are_without_the_key(built):
    """a band pattern stays on the band kernels, a pattern float32_general_dense takes stays on the dense route, a plan the
    register-front kernel serves stays on it: float32_subtrees False, the same configuration, the same bits"""
    from tests.support import f32_blocked_cases as FB
    hipldl, syn = _mods()
    sb = syn.band_structure(200, 4)
    _same_with_and_without(hipldl, sb, *G.band_inputs(syn, sb, range(4000, 4008)), FS.COND, "band")
    c = FB.case(FB.F97)
    healthy = [0, 4]
    _same_with_and_without(hipldl, c["s"], c["vals"][healthy], c["rhs"][healthy], dict(FS.COND, float32_general_dense=1), "dense")
    sr = syn.random_structure(60, 80, 4, 0.1, seed=3)
    _same_with_and_without(hipldl, sr, *G.random_inputs(syn, sr, range(100, 108)), dict(FS.COND, float32_register_front=1), "v2")


# ---- 7. a float32_register_front handle that fell back ----
def test_register_front_handle_that_fell_back_takes_the_route(built):
    """(450, 300, 4, 0.02, 1) with float32_register_front = 1: a front above order 64, so the handle is the float32_condense handle —
    and runs its subtrees"""
    hipldl, syn = _mods()
    c = FS.case(FS.CHAIN)
    L = _handle(hipldl, c, FS.MIX, True, 0, 1, forced=False, float32_register_front=1)
    _assert_cut(L, FS.CHAIN, True, 8)
    _run_mix(hipldl, c, L, 1, idxs=(np.arange(FS.MIX),))
    L.close()


# ---- 8. the rules with a device, and the lockstep loop's tuning ----
def test_rules_with_a_device(built):
    """the rules of tests/test_float32_subtrees_cpu.py hold on a machine with a device, where the accepted combinations make a handle"""
    from tests import test_float32_subtrees_cpu as cpu
    cpu.test_key_rules_without_a_device(True)
    cpu.test_general_subtrees_is_still_refused_at_the_float32_creators(True)
    cpu.test_a_float64_creator_reads_nothing_of_the_key(True)


def test_lockstep_loop_passes_the_key_through(built):
    """solve_batch_device(fam, tuning = {...}) hands the key to the handle: a value the library refuses is refused there, and with the
    key at 1 the run is the run without it on a band family (a chain: one task per stage, so the key does not act), bit for bit"""
    import torch
    hipldl, syn = _mods()
    from cannoles_jl_amd import device_loop as DL
    fam = DL.BandQuadFamily(syn.band_structure(60, 2, hw=3), 8, seed=62, torch=torch, device="cuda:0", dtype=np.float32)
    with pytest.raises(hipldl.CnlError) as e:
        DL.solve_batch_device(fam, tuning={"float32_general": 1, "float32_subtrees": 2})
    assert e.value.code == CNL_ERR_ARG and "float32_subtrees" in str(e.value), str(e.value)
    runs = [DL.solve_batch_device(fam, tuning=dict({"float32_general": 1, "v1_tpp": 256, "v1_ppb": 1}, **key)) for key in ({"float32_subtrees": 1}, {})]
    assert runs[0]["status"] == runs[1]["status"] == ["first_order"] * 8 and runs[0]["kernel"] == runs[1]["kernel"] == "v1"
    for k in ("solution", "multipliers"):
        assert np.asarray(runs[0][k]).tobytes() == np.asarray(runs[1][k]).tobytes(), k
