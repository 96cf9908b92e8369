"""The general kernel's subtree execution (tuning general_subtrees: csrc/kernels.hip, newton_subtrees — one workgroup per problem and
task of the elimination tree, a launch per stage) against the CPU oracle and against the same handle with the key off.  -m gpu.

Inputs and reference: the seven-kind mix of tests/support/dense_general_cases.py on the shapes of
tests/support/general_subtrees_cases.py, the oracle on the canonical order and on the handle's own; tests/test_general_subtrees_cpu.py
vouches for the cut, the layout and the oracle's decisions.  Tolerances are those of tests/test_gpu_parity.py: BWD_TOL = 1e-13,
FWD_TOL = 1e-9 on problems with nfact 1.  Decisions (ok, nfact, rho, rho_old, the rho slots of vals) are compared bit for bit; a
failed problem keeps its d = 7.0 sentinel."""
import numpy as np
import pytest

from tests.support import dense_general_cases as GC
from tests.support import general_subtrees_cases as GS
from tests.test_gpu_parity import BWD_TOL, FWD_TOL, backward_error

pytestmark = pytest.mark.gpu


def _mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    from oracle import oracle as O
    return hipldl, syn, O


def _handle(hipldl, c, B, shape, **opt):
    s = c["s"]
    if shape[0] == "grid":
        opt = dict(dict(plan_kind=hipldl.PLAN_THROUGHPUT), **opt)
    return hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(**GS.options(**opt)))


def _stages(L):
    return len(L.plan_array("gstage_ptr")) - 1


def _run_mix(hipldl, c, L, subtrees=True, tpp=256):
    """one cnl_newton_system_dev call on the case's problems, forwards and reversed, checked on both orders; returns the outputs of
    the forward call"""
    s, B = c["s"], len(c["vals"])
    cfg = L.config
    assert cfg["kernel"] == "v1" and cfg["general_subtrees"] == subtrees and not cfg["float32"], cfg
    assert cfg["tpp"] == tpp and (cfg["ppb"] == 1 or not subtrees), cfg
    if subtrees:
        assert not cfg["lds_work"], cfg
    refs = [c, GC.oracle_on(L.plan_array("perm").astype(np.int64), c)]
    A = GC.Args(s, B)
    first = None
    for idx in (np.arange(B), np.arange(B)[::-1]):
        A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
        before = hipldl.launch_counts()["general"]
        A.call(hipldl, L, hipldl.default_params())
        out = A.read()
        if subtrees:
            assert hipldl.launch_counts()["general"] - before == 2 * _stages(L) + 2      # S forward, decide, S backward, the climbers — DESIGN 3.2
        be, fe = GC.check_outputs(out, refs, c, c["rhs"][idx], idx, BWD_TOL, FWD_TOL, backward_error)
        print(f"tpp {cfg['tpp']} subtrees {cfg['general_subtrees']}: ok {out['ok'].tolist()} nfact {out['nf'].tolist()} backward {be:.2e} forward {fe:.2e}")
        first = first or out
    return first


# ---- 1. the mix against the oracle ----
@pytest.mark.parametrize("condense", (1, 0), ids=("condensed", "uncondensed"))
@pytest.mark.parametrize("cap", (4, 8))
@pytest.mark.parametrize("shape", (GS.GRID12, GS.GRID16), ids=GS.shape_id)
def test_grids(built, shape, cap, condense):
    hipldl, syn, O = _mods()
    c = GS.case(shape)
    L = _handle(hipldl, c, GC.MIX, shape, v1_tpp=256, task_cap=cap, condense=condense)
    assert _stages(L) >= 3 and L.plan_array("ginfo")[3] >= 2
    _run_mix(hipldl, c, L)
    L.close()


@pytest.mark.parametrize("blocked,condense", [(0, 1), (1, 1), (1, 0)], ids=("unblocked", "blocked", "blocked-uncondensed"))
def test_grid32_with_and_without_blocked_panels(built, blocked, condense):
    """grid_structure(32), 50 tasks in 6 stages at cap 8: the separator fronts (21, 62), (31, 63) and the root (93, 0) are single-front
    tasks above the cut, eliminated in panels where general_blocked = 1 (uncondensed also (16, 13, 11))"""
    hipldl, syn, O = _mods()
    c = GS.case(GS.GRID32)
    L = _handle(hipldl, c, GC.MIX, GS.GRID32, v1_tpp=256, general_blocked=blocked, condense=condense)
    fr = [tuple(int(x) for x in f[[0, 1, 14]]) for f in L.plan_array("fronts").reshape(-1, 16)]
    for w in [(21, 62, 0), (31, 63, 0), (93, 0, 0)] + ([] if condense else [(16, 13, 11)]):
        assert w in fr, w
    assert L.config["general_blocked"] == bool(blocked)
    if condense:
        assert (len(L.plan_array("gtasks")) // 8, _stages(L)) == GS.CUT_CAP8[GS.GRID32]
    _run_mix(hipldl, c, L)
    L.close()


def test_1024_threads(built):
    hipldl, syn, O = _mods()
    c = GS.case(GS.GRID12)
    L = _handle(hipldl, c, GC.MIX, GS.GRID12, v1_tpp=1024, task_cap=4, general_blocked=1)
    _run_mix(hipldl, c, L, tpp=1024)
    L.close()


@pytest.mark.parametrize("shape,cap", [(GS.FOREST4, 4), (GS.FOREST3, 8)], ids=lambda v: GS.shape_id(v) if isinstance(v, tuple) else str(v))
def test_forests(built, shape, cap):
    """four and three roots: several tasks without a parent, the last stages short"""
    hipldl, syn, O = _mods()
    c = GS.case(shape)
    L = _handle(hipldl, c, GC.MIX, shape, v1_tpp=256, task_cap=cap)
    fr = L.plan_array("fronts").reshape(-1, 16)
    assert (fr[:, 11] < 0).sum() == (4 if shape == GS.FOREST4 else 3)
    _run_mix(hipldl, c, L)
    L.close()


def test_chain_like_tree_takes_the_route(built):
    """(450, 300, 4, 0.02, 1): 18 bottom subtrees under eight more stages, the last six of one task each — by the documented rule
    (two tasks or more in the first stage) it takes the route, at its default configuration (fmax 375: 256 threads), and measured
    faster there; tests/test_general_blocked_cpu.py vouches for the oracle's decisions on this shape"""
    hipldl, syn, O = _mods()
    c = GS.case(GS.CHAIN)
    L = _handle(hipldl, c, GC.MIX, GS.CHAIN, general_blocked=1)
    assert L.plan_array("ginfo")[1:4].tolist() == [31, 9, 18] and L.config["general_blocked"], L.config
    _run_mix(hipldl, c, L)
    L.close()


# ---- 2. key on against key off ----
@pytest.mark.parametrize("shape,opt", [(GS.GRID16, dict(task_cap=8)), (GS.GRID16, dict(task_cap=4, condense=0)), (GS.FOREST4, dict(task_cap=4)),
                                       (GS.GRID32, dict(general_blocked=1))], ids=lambda v: GS.shape_id(v) if isinstance(v, tuple) else "-".join(v))
def test_key_on_against_key_off(built, shape, opt):
    """the same shape, thread count and work area in global scratch: decisions bit-equal, d within FWD_TOL — the per-front arithmetic
    is the same source, so bit-equal d is the expectation; the test prints whether it holds"""
    hipldl, syn, O = _mods()
    c = GS.case(shape)
    s, B = c["s"], GC.MIX
    outs = []
    for key in (1, 0):
        L = _handle(hipldl, c, B, shape, **dict(opt, v1_tpp=256, v1_lds=0, general_subtrees=key))
        assert L.config["general_subtrees"] == bool(key) and L.config["kernel"] == "v1" and L.config["tpp"] == 256 and not L.config["lds_work"], L.config
        A = GC.Args(s, B)
        A.fill(c["vals"], c["rhs"], c["rho_old"])
        A.call(hipldl, L, hipldl.default_params())
        outs.append(A.read())
        L.close()
    on, off = outs
    for k in ("ok", "nf"):
        assert np.array_equal(on[k], off[k]), k
    for k in ("rho", "ro"):
        assert np.array_equal(GC.bits64(on[k]), GC.bits64(off[k])), k
    assert np.array_equal(GC.bits64(on["vals"][:, -s.nvar:]), GC.bits64(off["vals"][:, -s.nvar:]))
    worst, bit_equal = 0.0, True
    for b in range(B):
        if not on["ok"][b]:
            assert (on["d"][b] == 7.0).all() and (off["d"][b] == 7.0).all()
            continue
        bit_equal &= bool(np.array_equal(GC.bits64(on["d"][b]), GC.bits64(off["d"][b])))
        fe = np.abs(on["d"][b] - off["d"][b]).max() / np.abs(off["d"][b]).max()
        worst = max(worst, fe)
        assert fe <= FWD_TOL, (b, fe)
    print(f"{GS.shape_id(shape)} {opt}: d with the key on against off: bit-equal {bit_equal}, worst {worst:.2e}")


# ---- 3. the two-call sequence ----
@pytest.mark.parametrize("condense", (1, 0), ids=("condensed", "uncondensed"))
def test_two_call_sequence_inertia_and_failed_rows(built, condense):
    """cnl_factorize_dev (S + 1 launches: the stages and the decide kernel), then cnl_solve_dev twice with different right-hand sides
    on that factor (2 S launches each): the solutions against cnl_newton_system_dev's backward error bound, vals untouched, the rows
    of d of the problems without a factor at their 7.0 sentinel (the handle keeps the flags of its last factorisation); then the host
    try_to_factorize with the inertia, equal to the oracle's counts."""
    import torch
    hipldl, syn, O = _mods()
    c = GS.case(GS.GRID12)
    s, B = c["s"], GC.MIX
    eig_tol = O.default_params()[0]
    orc = O.Oracle(s.N, c["rows"], c["cols"], O.canonical_perm(s.nvar, s.nequ, s.ncon))
    ref = [orc.try_to_factorize(np.array(c["vals"][b]), s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True) for b in range(B)]
    want = [bool(r[0]) for r in ref]
    assert want == [True, False, False, False, True, True, False]
    L = _handle(hipldl, c, B, GS.GRID12, v1_tpp=256, task_cap=4, condense=condense)
    assert L.config["general_subtrees"] and L.config["kernel"] == "v1", L.config
    S = _stages(L)
    dev = "cuda:0"
    t_vals = torch.from_numpy(np.array(c["vals"])).to(dev)
    t_ok = torch.full((B,), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    n0 = hipldl.launch_counts()["general"]
    hipldl.factorize_dev(L, t_vals.data_ptr(), eig_tol, t_ok.data_ptr(), stream=stream)
    assert hipldl.launch_counts()["general"] - n0 == S + 1
    for k in range(2):
        r = np.ascontiguousarray(c["rhs"] * (k + 1.5))
        t_r = torch.from_numpy(r).to(dev)
        t_d = torch.full((B, s.N), 7.0, dtype=torch.float64, device=dev)
        n0 = hipldl.launch_counts()["general"]
        hipldl.solve_dev(L, t_r.data_ptr(), t_d.data_ptr(), stream=stream)
        assert hipldl.launch_counts()["general"] - n0 == 2 * S
        torch.cuda.synchronize()
        assert t_ok.cpu().numpy().tolist() == [int(w) for w in want]
        d = t_d.cpu().numpy()
        for b in range(B):
            if want[b]:
                be = backward_error(s, c["vals"][b], r[b], d[b])
                assert be <= BWD_TOL, (b, k, be)
            else:
                assert (d[b] == 7.0).all(), b      # no factor: the rows stay untouched
    assert np.array_equal(GC.bits64(t_vals.cpu().numpy()), GC.bits64(c["vals"]))
    # the solve at the right-hand side of the mix is newton_system's d of the problems that succeed at once
    A = GC.Args(s, B)
    A.fill(c["vals"], c["rhs"], c["rho_old"])
    A.call(hipldl, L, hipldl.default_params())
    out = A.read()
    hipldl.factorize_dev(L, t_vals.data_ptr(), eig_tol, t_ok.data_ptr(), stream=stream)
    t_r = torch.from_numpy(np.array(c["rhs"])).to(dev)
    t_d = torch.full((B, s.N), 7.0, dtype=torch.float64, device=dev)
    hipldl.solve_dev(L, t_r.data_ptr(), t_d.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    d = t_d.cpu().numpy()
    for b in range(B):
        if want[b]:
            assert np.abs(d[b] - out["d"][b]).max() <= FWD_TOL * np.abs(out["d"][b]).max(), b
    ok, npos, nzer = hipldl.try_to_factorize(L, np.array(c["vals"]), s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True)
    assert list(ok) == want
    for b in range(B):
        if b % GC.MIX != 1:     # (the hopeless problem's pivots are NaN: its counts mean nothing in either arithmetic)
            assert (int(npos[b]), int(nzer[b])) == (int(ref[b][1]), int(ref[b][2])), b
    L.close()


# ---- 4. batches ----
def test_batch_of_one(built):
    hipldl, syn, O = _mods()
    for kind in (0, 2):
        c = GS.case(GS.GRID12, kinds=(kind,))
        L = _handle(hipldl, c, 1, GS.GRID12, v1_tpp=256, task_cap=4)
        out = _run_mix(hipldl, c, L)
        assert out["ok"].tolist() == [1] and out["nf"].tolist() == [GC.WANT_NF[kind]]
        L.close()


def test_batch_of_65_and_an_active_prefix(built):
    """65 problems (nine mixes and two); then cnl_set_active_batch on the first 20: the later problems' outputs stay untouched"""
    hipldl, syn, O = _mods()
    c = GS.case(GS.GRID12, B=65)
    s = c["s"]
    L = _handle(hipldl, c, 65, GS.GRID12, v1_tpp=256, task_cap=4)
    out = _run_mix(hipldl, c, L)
    # (checked against the oracle by _run_mix; kind 5 — one positive residual pivot — depends on the values: it fails at some seeds)
    assert [out["ok"][b] for b in range(65) if b % GC.MIX != 5] == [int(GC.WANT_OK[b % GC.MIX]) for b in range(65) if b % GC.MIX != 5]
    assert [out["nf"][b] for b in range(65) if b % GC.MIX != 5] == [GC.WANT_NF[b % GC.MIX] for b in range(65) if b % GC.MIX != 5]
    nb = 20
    hipldl.set_active_batch(L, nb)
    A = GC.Args(s, 65)
    A.fill(c["vals"], c["rhs"], c["rho_old"])
    A.call(hipldl, L, hipldl.default_params())
    part = A.read()
    assert (part["d"][nb:] == 7.0).all() and (part["nf"][nb:] == -1).all() and (part["ok"][nb:] == -1).all()
    for k in ("ok", "nf"):
        assert np.array_equal(part[k][:nb], out[k][:nb]), k
    for k in ("rho", "ro", "d"):
        assert np.array_equal(GC.bits64(part[k][:nb]), GC.bits64(out[k][:nb])), k
    hipldl.set_active_batch(L, 65)
    L.close()


def test_sub_batch_views(built):
    """The host-pointer cnl_newton_system cuts a batch of 96 MB and more of input into chunks of at least 16 MB, each a view of the
    handle at its own offset into the factor panels, the task regions and the tasks' count slots: the mix on grid_structure(12)
    repeated to that size.  The first mix against the oracle; every repetition bit-equal to the first."""
    hipldl, syn, O = _mods()
    c = GS.case(GS.GRID12)
    s = c["s"]
    per = (s.nnzNS + s.N) * 8
    reps = -(-(96 << 20) // (GC.MIX * per))
    B = GC.MIX * reps
    assert B >= 32 and B * per >= (96 << 20) and max(16, ((B // 8) + 3) & ~3) < B       # the rule of cnl_newton_system
    L = _handle(hipldl, c, B, GS.GRID12, v1_tpp=256, v1_ppb=1, task_cap=4)     # (a batch this large gets several problems per workgroup by default)
    assert L.config["general_subtrees"] and L.config["kernel"] == "v1", L.config
    vals, rhs, ro = (np.ascontiguousarray(np.tile(c[k], (reps,) + (1,) * (c[k].ndim - 1))) for k in ("vals", "rhs", "rho_old"))
    before = hipldl.launch_counts()["general"]
    d, ok, rho, ro_out, nf = hipldl.newton_system_(np.full((B, s.N), 7.0), s.nvar, s.nequ, s.ncon, rhs, vals, L, ro, hipldl.default_params())
    chunk = max(16, ((B // 8) + 3) & ~3)
    while chunk * per < (16 << 20):
        chunk += 4
    nviews, per_call = -(-B // chunk), 2 * _stages(L) + 2
    launches = hipldl.launch_counts()["general"] - before
    assert nviews >= 2 and launches >= nviews * per_call and launches % per_call == 0, (nviews, launches)     # every view runs stage by stage
    out = dict(vals=vals, d=d, ok=np.asarray(ok).astype(np.int32), rho=rho, ro=ro_out, nf=np.asarray(nf))
    first = {k: v[:GC.MIX] for k, v in out.items()}
    refs = [c, GC.oracle_on(L.plan_array("perm").astype(np.int64), c)]
    GC.check_outputs(first, refs, c, c["rhs"], np.arange(GC.MIX), BWD_TOL, FWD_TOL, backward_error)
    for k, v in out.items():
        rep = v.reshape((reps, GC.MIX) + v.shape[1:])
        assert np.array_equal(rep, np.broadcast_to(rep[:1], rep.shape), equal_nan=True), k
    L.close()


# ---- 5. what earlier launches left in the task regions ----
def test_results_do_not_depend_on_what_the_scratch_holds(built):
    """The mix, then a call on OTHER values (every problem's kind shifted by three, so that every region of every problem — stack,
    panel buffer, staging rows, count slots — holds another problem's numbers, NaN among them), then the mix again: bit-equal to the
    first call in every output.  (The garbage-fill aid of tools/fuzz_parity.py fills LDS, private memory and registers; the task
    regions are global memory of the handle, which only a call of the handle itself reaches.)"""
    hipldl, syn, O = _mods()
    c = GS.case(GS.GRID16)
    s, B = c["s"], GC.MIX
    L = _handle(hipldl, c, B, GS.GRID16, v1_tpp=256, task_cap=4, general_blocked=1)
    first = _run_mix(hipldl, c, L)        # (its second call ran the problems in reversed order)
    A = GC.Args(s, B)
    idx = (np.arange(B) + 3) % B
    A.fill(c["vals"][idx] * 3.0, c["rhs"][idx], c["rho_old"][idx])
    A.call(hipldl, L, hipldl.default_params())
    A.read()
    A.fill(c["vals"], c["rhs"], c["rho_old"])
    A.call(hipldl, L, hipldl.default_params())
    again = A.read()
    for k in first:
        assert np.array_equal(first[k], again[k], equal_nan=True), k
    L.close()


# ---- 6. handles that run as without the key, and say so ----
@pytest.mark.parametrize("name,shape,opt", [("64-threads", GS.GRID12, dict(v1_tpp=64, task_cap=4)), ("single-task", GS.GRID12, dict(v1_tpp=256, task_cap=1000))])
def test_handles_the_key_does_not_act_on(built, name, shape, opt):
    hipldl, syn, O = _mods()
    c = GS.case(shape)
    s, B = c["s"], GC.MIX
    outs, cfgs = [], []
    for key in (1, 0):
        L = _handle(hipldl, c, B, shape, **dict(opt, general_subtrees=key))
        assert not L.config["general_subtrees"] and L.config["kernel"] == "v1", L.config
        cfgs.append(L.config)
        before = hipldl.launch_counts()["general"]
        outs.append(_run_mix(hipldl, c, L, subtrees=False, tpp=opt["v1_tpp"]))
        assert hipldl.launch_counts()["general"] - before == 2         # one classic launch per call
        L.close()
    assert cfgs[0] == cfgs[1]
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k
