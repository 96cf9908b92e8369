"""The staged rho ladder of subtree handles (tuning subtree_ladder = R: csrc/capi_run.cpp — launch_subtrees —, csrc/kernels.hip —
subtree_ladder_kernel, the first decide, the rung decide, the commit) against the CPU oracle and against the same handle with R = 0.
-m gpu.

Inputs, references and bars are those of tests/support/subtree_ladder_cases.py: the seven-kind mix in double and the five-kind mix in
float on the shapes of tests/support/general_subtrees_cases.py, the oracle on the canonical order and on the handle's own, FWD_TOL /
BWD_TOL of tests/test_gpu_parity.py in double and the Float32 bars of tests/support/f32_subtrees_cases.py;
tests/test_subtree_ladder_cpu.py vouches for the sequence and for the ends the cases reach.  Everything goes through
cnl_newton_system_dev with sentinels unless the test says otherwise.  Decisions are compared bit for bit against the oracle, and EVERY
output bit for bit against the same handle with R = 0."""
import numpy as np
import pytest

from tests.support import subtree_ladder_cases as SL
from tests.test_gpu_parity import BWD_TOL, FWD_TOL, backward_error

GS, FS, GC = SL.GS, SL.FS, SL.GC
pytestmark = pytest.mark.gpu
CNL_ERR_ARG = 1
f32, f64 = np.float32, np.float64


def _mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl
    return hipldl


def _stages(L):
    return len(L.plan_array("gstage_ptr")) - 1


def _handle64(hipldl, c, B, shape, **opt):
    s = c["s"]
    if shape[0] == "grid":
        opt = dict(dict(plan_kind=hipldl.PLAN_THROUGHPUT), **opt)
    return hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(**GS.options(**opt)))


def _handle32(hipldl, c, B, cond, cap, blocked=0, **extra):
    opt = dict(FS.COND if cond else FS.UNCOND, **FS.KEY, float32_blocked=blocked, task_cap=cap, **FS.FORCED, **extra)
    return FS.handle(hipldl, c, B, **opt)


def _call(hipldl, c, L, idx, f32_=False, params=None):
    A = (FS.GD.Args if f32_ else GC.Args)(c["s"], len(idx))
    A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
    A.call(hipldl, L, (c["p32"] if f32_ else c["params"]) if params is None else params)
    return A.read()


def _check(hipldl, c, L, out, idx, f32_):
    """one call's outputs against the oracle on the canonical order and on the handle's own"""
    perm = L.plan_array("perm").astype(np.int64)
    if f32_:
        for ref in (c, FS.oracle_on(perm, c)):
            be, fe = FS.check_outputs(ref, out, idx, c["vals"][idx])
        return be, fe
    return GC.check_outputs(out, [c, GC.oracle_on(perm, c)], c, c["rhs"][idx], idx, BWD_TOL, FWD_TOL, backward_error)


def _same(a, b, what=""):
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(SL.bits(a[k]) if a[k].dtype.kind == "f" else a[k], SL.bits(b[k]) if b[k].dtype.kind == "f" else b[k]), (what, k)


_r0 = {}


def _mix(hipldl, c, make, R, f32_=False, tag=None, key_cfg="general_subtrees"):
    """The case through a handle with subtree_ladder = R, its problems forwards and reversed: the configuration, the launch count
    (R + 2) S + R + 3, the oracle on both orders, and every output bit-equal to the same handle with R = 0 (made once per `tag`)."""
    B = len(c["vals"])
    orders = (np.arange(B), np.arange(B)[::-1])
    if tag not in _r0:
        L0 = make(0)
        assert L0.config[key_cfg] and L0.config["subtree_ladder"] == 0, L0.config
        _r0[tag] = [_call(hipldl, c, L0, idx, f32_) for idx in orders]
        L0.close()
    L = make(R)
    cfg = L.config
    assert cfg["kernel"] == "v1" and cfg[key_cfg] and cfg["subtree_ladder"] == R and cfg["ppb"] == 1 and not cfg["lds_work"], cfg
    S = _stages(L)
    outs = []
    for idx, ref in zip(orders, _r0[tag]):
        before = hipldl.launch_counts()["general"]
        out = _call(hipldl, c, L, idx, f32_)
        assert hipldl.launch_counts()["general"] - before == SL.launches(R, S) == (R + 2) * S + R + 3
        be, fe = _check(hipldl, c, L, out, idx, f32_)
        _same(out, ref, (tag, R))
        outs.append(out)
    print(f"{tag} R {R}: {S} stages, {SL.launches(R, S)} launches, ok {outs[0]['ok'].tolist()} nfact {outs[0]['nf'].tolist()} backward {be:.2e} forward {fe:.2e}; "
          f"every output bit-equal to R = 0")
    return L, outs[0]


# ---- 1. the mix, double ----
@pytest.mark.parametrize("R", (1, 3, 5, 19, 24))
@pytest.mark.parametrize("condense", (1, 0), ids=("condensed", "uncondensed"))
@pytest.mark.parametrize("cap", (4, 8))
def test_grid12_double(built, cap, condense, R):
    hipldl = _mods()
    c = GS.case(GS.GRID12)
    assert c["nf"].tolist() == GC.WANT_NF
    L, out = _mix(hipldl, c, lambda r: _handle64(hipldl, c, GC.MIX, GS.GRID12, v1_tpp=256, task_cap=cap, condense=condense, subtree_ladder=r), R,
                  tag=("grid12", cap, condense))
    if condense:
        assert (len(L.plan_array("gtasks")) // 8, _stages(L)) == {4: (12, 4), 8: (6, 3)}[cap]
    L.close()


@pytest.mark.parametrize("R", (3, 19))
@pytest.mark.parametrize("shape", (GS.GRID16, GS.FOREST3), ids=GS.shape_id)
def test_grid16_and_forest_double(built, shape, R):
    hipldl = _mods()
    c = GS.case(shape)
    L, out = _mix(hipldl, c, lambda r: _handle64(hipldl, c, GC.MIX, shape, v1_tpp=256, task_cap=4, subtree_ladder=r), R, tag=(shape,))
    L.close()


@pytest.mark.parametrize("blocked", (0, 1), ids=("unblocked", "blocked"))
def test_grid32_double(built, blocked):
    """grid_structure(32) at 256 threads per problem (its largest front, order 95, takes 64 by itself: forced, as in
    tests/test_general_subtrees_gpu.py), the separator fronts in panels where general_blocked = 1"""
    hipldl = _mods()
    c = GS.case(GS.GRID32)
    L, out = _mix(hipldl, c, lambda r: _handle64(hipldl, c, GC.MIX, GS.GRID32, v1_tpp=256, general_blocked=blocked, subtree_ladder=r), 5, tag=("grid32", blocked))
    assert L.config["tpp"] == 256 and L.config["general_blocked"] == bool(blocked), L.config
    L.close()


def test_1024_threads(built):
    hipldl = _mods()
    c = GS.case(GS.GRID12)
    L, out = _mix(hipldl, c, lambda r: _handle64(hipldl, c, GC.MIX, GS.GRID12, v1_tpp=1024, task_cap=4, general_blocked=1, subtree_ladder=r), 3, tag=("1024",))
    assert L.config["tpp"] == 1024, L.config
    L.close()


# ---- 2. the mix, float ----
FLOAT_CASES = [(GS.GRID12, True, 0), (GS.GRID12, False, 0), (GS.GRID12, True, 1), (GS.GRID12, False, 1), (GS.FOREST3, True, 0), (GS.FOREST3, False, 1)]


@pytest.mark.parametrize("R", (2, 3, SL.R_EXHAUST[f32]))
@pytest.mark.parametrize("shape,cond,blocked", FLOAT_CASES, ids=[f"{GS.shape_id(sh)}-{'condensed' if cd else 'uncondensed'}-{'blocked' if bl else 'unblocked'}" for sh, cd, bl in FLOAT_CASES])
def test_mix_float(built, shape, cond, blocked, R):
    hipldl = _mods()
    c = FS.case(shape)
    assert c["nf"].tolist() == FS.WANT_NF
    L, out = _mix(hipldl, c, lambda r: _handle32(hipldl, c, FS.MIX, cond, 4, blocked, subtree_ladder=r), R, f32_=True, tag=("f32", shape, cond, blocked),
                  key_cfg="float32_subtrees")
    assert L.config["float32"] and L.config["tpp"] == 256 and L.config["float32_blocked"] == bool(blocked) and not L.config["general_subtrees"], L.config
    L.close()


# ---- 3. the two rhomax parameter sets ----
@pytest.mark.parametrize("pset", ("between", "below"))
@pytest.mark.parametrize("f32_", (False, True), ids=("double", "float"))
def test_rhomax_parameter_sets(built, f32_, pset):
    """`between`: failures exhaust at the decide of rung 2, inside R = 3; `below`: rung 1 is tried above rhomax and nothing follows"""
    hipldl = _mods()
    c = SL.case_with_params((FS if f32_ else GS).case(GS.GRID12), pset, f32=f32_)
    assert c["nf"].tolist() == ({"between": [1, 3, 3, 2, 1], "below": [1, 2, 2, 2, 1]} if f32_ else {"between": [1, 3, 3, 2, 1, 1, 3], "below": [1, 2, 2, 2, 1, 1, 2]})[pset]
    if f32_:
        make = lambda r: _handle32(hipldl, c, FS.MIX, True, 4, 0, subtree_ladder=r)
    else:
        make = lambda r: _handle64(hipldl, c, GC.MIX, GS.GRID12, v1_tpp=256, task_cap=4, subtree_ladder=r)
    L, out = _mix(hipldl, c, make, 3, f32_=f32_, tag=("pset", f32_, pset), key_cfg="float32_subtrees" if f32_ else "general_subtrees")
    fails = ~c["ok"]
    assert (out["rho"][fails] > (c["p32"] if f32_ else c["params"])[6]).all() and np.array_equal(out["ro"][fails], c["rho_old"][fails])
    L.close()


# ---- 4. failures and factors ----
@pytest.mark.parametrize("R", (3, 19))
def test_solve_on_the_factor_the_last_rung_left(built, R):
    """Behind a call with R > 0, cnl_solve_dev solves the successes with the factor their LAST attempt left — a rung's for the problems
    that finished inside the rungs, the resumed climbers' for the others — at the rho that attempt tried (the rho slots the call left in
    vals), and leaves the rows of d of the failures at their sentinel."""
    import torch
    hipldl = _mods()
    c = GS.case(GS.GRID12)
    s, B = c["s"], GC.MIX
    L, out = _mix(hipldl, c, lambda r: _handle64(hipldl, c, B, GS.GRID12, v1_tpp=256, task_cap=4, subtree_ladder=r), R, tag=("grid12", 4, 1))
    A = GC.Args(s, B)       # (the last call of _mix ran the problems reversed; a condensed handle condenses later right-hand sides
    A.fill(c["vals"], c["rhs"], c["rho_old"])       #  with the vals of this call: they stay alive as long as the solves run)
    A.call(hipldl, L, c["params"])
    out = A.read()
    ok = c["ok"]
    assert (out["d"][~ok] == 7.0).all()
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(2):
        r = np.ascontiguousarray(c["rhs"] * (k + 1.5))
        t_r = torch.from_numpy(r).to("cuda:0")
        t_d = torch.full((B, s.N), 7.0, dtype=torch.float64, device="cuda:0")
        n0 = hipldl.launch_counts()["general"]
        hipldl.solve_dev(L, t_r.data_ptr(), t_d.data_ptr(), stream=stream)
        assert hipldl.launch_counts()["general"] - n0 == 2 * _stages(L)
        torch.cuda.synchronize()
        d = t_d.cpu().numpy()
        for b in range(B):
            if ok[b]:
                be = backward_error(s, out["vals"][b], r[b], d[b])      # K at the rho of the last attempt
                assert be <= BWD_TOL, (b, k, be)
            else:
                assert (d[b] == 7.0).all(), b
    t_r = torch.from_numpy(np.array(c["rhs"])).to("cuda:0")
    t_d = torch.full((B, s.N), 7.0, dtype=torch.float64, device="cuda:0")
    hipldl.solve_dev(L, t_r.data_ptr(), t_d.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    d = t_d.cpu().numpy()
    own = GC.oracle_on(L.plan_array("perm").astype(np.int64), c)
    for b in range(B):
        if ok[b]:
            # the solve at the right-hand side of the mix is newton_system's d (the bar of tests/test_general_subtrees_gpu.py), and the
            # oracle's where the problem succeeded at once
            assert np.abs(d[b] - out["d"][b]).max() <= FWD_TOL * np.abs(out["d"][b]).max(), b
            if c["nf"][b] == 1:
                assert np.abs(d[b] - own["d"][b]).max() <= FWD_TOL * np.abs(own["d"][b]).max(), b
        else:
            assert (d[b] == 7.0).all(), b
    # try_to_factorize and solve_ldl! are untouched by the key: S + 1 launches
    t_vals = torch.from_numpy(np.array(c["vals"])).to("cuda:0")
    t_ok = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
    n0 = hipldl.launch_counts()["general"]
    hipldl.factorize_dev(L, t_vals.data_ptr(), c["params"][0], t_ok.data_ptr(), stream=stream)
    assert hipldl.launch_counts()["general"] - n0 == _stages(L) + 1
    torch.cuda.synchronize()
    assert t_ok.cpu().numpy().tolist() == [1, 0, 0, 0, 1, 1, 0]
    L.close()


# ---- 5. batch sizes and views ----
@pytest.mark.parametrize("R", (3, 5))
def test_batch_of_one_climber(built, R):
    """one problem of kind 2 (nfact 6): at R = 3 it resumes in the climbers' launch, at R = 5 it finishes on the last rung"""
    hipldl = _mods()
    c = GS.case(GS.GRID12, kinds=(2,))
    assert c["nf"].tolist() == [6] and c["ok"].tolist() == [True]
    L, out = _mix(hipldl, c, lambda r: _handle64(hipldl, c, 1, GS.GRID12, v1_tpp=256, task_cap=4, subtree_ladder=r), R, tag=("one",))
    assert out["ok"].tolist() == [1] and out["nf"].tolist() == [6]
    L.close()


def test_batch_of_65_and_an_active_prefix(built):
    hipldl = _mods()
    c = GS.case(GS.GRID12, B=65)
    s = c["s"]
    L, out = _mix(hipldl, c, lambda r: _handle64(hipldl, c, 65, GS.GRID12, v1_tpp=256, task_cap=4, subtree_ladder=r), 3, tag=("65",))
    nb = 20
    hipldl.set_active_batch(L, nb)
    A = GC.Args(s, 65)
    A.fill(c["vals"], c["rhs"], c["rho_old"])
    before = hipldl.launch_counts()["general"]
    A.call(hipldl, L, hipldl.default_params())
    assert hipldl.launch_counts()["general"] - before == SL.launches(3, _stages(L))
    part = A.read()
    assert (part["d"][nb:] == 7.0).all() and (part["nf"][nb:] == -1).all() and (part["ok"][nb:] == -1).all() and (part["rho"][nb:] == -1.0).all()
    assert np.array_equal(GC.bits64(part["vals"][nb:]), GC.bits64(c["vals"][nb:])) and np.array_equal(part["ro"][nb:], c["rho_old"][nb:])
    for k in part:
        assert np.array_equal(SL.bits(part[k][:nb]) if part[k].dtype.kind == "f" else part[k][:nb], SL.bits(out[k][:nb]) if out[k].dtype.kind == "f" else out[k][:nb]), k
    hipldl.set_active_batch(L, 65)
    L.close()


def test_sub_batch_views(built):
    """The host-pointer cnl_newton_system cuts 96 MB of input into views of the handle, each at its own offset into the factor panels,
    the task regions, the count slots and the ladder state: every view runs the whole staged sequence, the first mix against the
    oracle, every repetition bit-equal to the first."""
    hipldl = _mods()
    R = 3
    c = GS.case(GS.GRID12)
    s = c["s"]
    per = (s.nnzNS + s.N) * 8
    reps = -(-(96 << 20) // (GC.MIX * per))
    B = GC.MIX * reps
    assert B >= 32 and B * per >= (96 << 20) and max(16, ((B // 8) + 3) & ~3) < B       # the rule of cnl_newton_system
    L = _handle64(hipldl, c, B, GS.GRID12, v1_tpp=256, v1_ppb=1, task_cap=4, subtree_ladder=R)
    assert L.config["general_subtrees"] and L.config["subtree_ladder"] == R, L.config
    vals, rhs, ro = (np.ascontiguousarray(np.tile(c[k], (reps,) + (1,) * (c[k].ndim - 1))) for k in ("vals", "rhs", "rho_old"))
    before = hipldl.launch_counts()["general"]
    d, ok, rho, ro_out, nf = hipldl.newton_system_(np.full((B, s.N), 7.0), s.nvar, s.nequ, s.ncon, rhs, vals, L, ro, hipldl.default_params())
    chunk = max(16, ((B // 8) + 3) & ~3)
    while chunk * per < (16 << 20):
        chunk += 4
    nviews, per_call = -(-B // chunk), SL.launches(R, _stages(L))
    launches = hipldl.launch_counts()["general"] - before
    assert nviews >= 2 and launches >= nviews * per_call and launches % per_call == 0, (nviews, launches)
    out = dict(vals=vals, d=d, ok=np.asarray(ok).astype(np.int32), rho=rho, ro=ro_out, nf=np.asarray(nf))
    first = {k: v[:GC.MIX] for k, v in out.items()}
    GC.check_outputs(first, [c, GC.oracle_on(L.plan_array("perm").astype(np.int64), c)], c, c["rhs"], np.arange(GC.MIX), BWD_TOL, FWD_TOL, backward_error)
    for k, v in out.items():
        rep = v.reshape((reps, GC.MIX) + v.shape[1:])
        assert np.array_equal(rep, np.broadcast_to(rep[:1], rep.shape), equal_nan=True), k
    L.close()


@pytest.mark.parametrize("f32_", (False, True), ids=("double", "float"))
def test_results_do_not_depend_on_what_the_state_holds(built, f32_):
    """The mix, then a call on OTHER values (every problem's kind shifted by three: every region, count slot, done flag and rho of the
    ladder state holds another problem's numbers), then the mix again: bit-equal to the first call in every output."""
    hipldl = _mods()
    c = (FS if f32_ else GS).case(GS.GRID16)
    s, B = c["s"], len(c["vals"])
    L = _handle32(hipldl, c, B, True, 4, 1, subtree_ladder=3) if f32_ else _handle64(hipldl, c, B, GS.GRID16, v1_tpp=256, task_cap=4, general_blocked=1, subtree_ladder=3)
    assert L.config["subtree_ladder"] == 3, L.config
    idx = np.arange(B)
    first = _call(hipldl, c, L, idx, f32_)
    _check(hipldl, c, L, first, idx, f32_)
    A = (FS.GD.Args if f32_ else GC.Args)(s, B)
    sh = (idx + 3) % B
    A.fill(c["vals"][sh] * (c["vals"].dtype.type(3)), c["rhs"][sh], c["rho_old"][sh])
    A.call(hipldl, L, c["p32"] if f32_ else c["params"])
    A.read()
    again = _call(hipldl, c, L, idx, f32_)
    for k in first:
        assert np.array_equal(first[k], again[k], equal_nan=True), k
    L.close()


# ---- 6. R = 0, and handles the subtree key does not act on ----
def test_R_0_is_the_parent_sequence(built):
    hipldl = _mods()
    c = GS.case(GS.GRID12)
    outs = []
    for opt in (dict(subtree_ladder=0), {}):
        L = _handle64(hipldl, c, GC.MIX, GS.GRID12, v1_tpp=256, task_cap=4, **opt)
        assert L.config["general_subtrees"] and L.config["subtree_ladder"] == 0, L.config
        before = hipldl.launch_counts()["general"]
        outs.append(_call(hipldl, c, L, np.arange(GC.MIX)))
        assert hipldl.launch_counts()["general"] - before == 2 * _stages(L) + 2
        L.close()
    _same(outs[0], outs[1])


@pytest.mark.parametrize("name,opt", [("64-threads", dict(v1_tpp=64, task_cap=4)), ("single-task", dict(v1_tpp=256, task_cap=1000))])
def test_handles_the_subtree_key_does_not_act_on(built, name, opt):
    """given R = 5 such a handle runs one classic launch per call, reports 0 and is the handle with both keys off"""
    hipldl = _mods()
    c = GS.case(GS.GRID12)
    outs, cfgs = [], []
    for keys in (dict(general_subtrees=1, subtree_ladder=5), dict(general_subtrees=0)):
        L = _handle64(hipldl, c, GC.MIX, GS.GRID12, **dict(opt, **keys))
        assert not L.config["general_subtrees"] and L.config["subtree_ladder"] == 0 and L.config["kernel"] == "v1", L.config
        cfgs.append(L.config)
        before = hipldl.launch_counts()["general"]
        outs.append(_call(hipldl, c, L, np.arange(GC.MIX)))
        assert hipldl.launch_counts()["general"] - before == 1
        _check(hipldl, c, L, outs[-1], np.arange(GC.MIX), False)
        L.close()
    assert cfgs[0] == cfgs[1]
    _same(outs[0], outs[1])


# ---- 7. the refusals, through the C ABI ----
def test_refusals(built):
    hipldl = _mods()
    s = GS.structure(GS.FOREST3)
    rows, cols = s.kkt_pattern()

    def rc(dtype, **opt):
        try:
            hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=7, dtype=dtype, options=hipldl.Options(**opt)).close()
        except hipldl.CnlError as e:
            return e.code, str(e)
        return 0, ""

    assert rc(f64, general_subtrees=1, subtree_ladder=64)[0] == 0 and rc(f32, float32_general=1, float32_subtrees=1, subtree_ladder=64)[0] == 0
    for dtype, opt in ((f64, dict(subtree_ladder=3)), (f64, dict(general_subtrees=1, subtree_ladder=65)), (f64, dict(general_subtrees=1, subtree_ladder=-1)),
                       (f32, dict(float32_general=1, subtree_ladder=3)), (f32, dict(float32_general=1, general_subtrees=1, subtree_ladder=3)),
                       (f32, dict(float32_general=1, float32_subtrees=1, subtree_ladder=65)),
                       (f64, dict(float32_general=1, float32_subtrees=1, subtree_ladder=3)),
                       (f64, dict(float32_general=1, float32_refine=1, float32_subtrees=1, subtree_ladder=3)),
                       (f64, dict(float32_general=1, float32_refine=1, general_subtrees=1, subtree_ladder=3))):
        code, msg = rc(dtype, **opt)
        assert code == CNL_ERR_ARG, (opt, code, msg)
