"""The blocked general kernel in float (tuning float32_blocked: csrc/kernels.hip — on a Float32 general handle fronts with 16 pivots
or more leave in panels of 16, the trailing updates run on v_mfma_f32_16x16x4_f32) against the fp64 oracle on the widened float data.
-m gpu.

Inputs, reference, tolerances and the per-call bar are those of tests/support/f32_blocked_cases.py (the Float32 five-kind mix and
check_outputs of tests/support/f32_general_dense.py on the shapes of tests/support/general_blocked_cases.py; BWD_TOL, FWD_TOL of
tests/support/f32_general.py); tests/test_float32_blocked_cpu.py vouches for the fronts these shapes have in the Float32 plans and for
every decision of every rung, so no test skips or reclassifies a problem.  Everything goes through cnl_newton_system_f32_dev with
sentinels in d.  Decisions (success, nfact, rho, rho_old, the rho slots) are compared bit for bit — with the oracle's, and between
key on and key off; d is compared with the oracle only, within the bars: in float the blocked and the rank-1 summation orders round
differently."""
import numpy as np
import pytest

from tests.support import f32_blocked_cases as FB
from tests.support import f32_general as G

pytestmark = pytest.mark.gpu
CNL_ERR_ARG = 1
LDS_LIMIT = 160 * 1024      # what choose_config allows a workgroup


def _mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    return hipldl, syn


def _call(hipldl, c, L, idx):
    A = FB.GD.Args(c["s"], len(idx))
    A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
    A.call(hipldl, L, c["p32"])
    return A.read()


def _run_mix(hipldl, c, L, blocked=True, tpp=None, lds=None):
    """one cnl_newton_system_f32_dev call on the case's problems, forwards and reversed, each against the oracle; the handle's
    configuration is asserted FIRST.  Returns the outputs of the forward call."""
    B = len(c["vals"])
    cfg = L.config
    assert cfg["kernel"] == "v1" and cfg["float32"] and not cfg["band"] and cfg["float32_blocked"] == blocked and not cfg["general_blocked"], cfg
    if tpp is not None:
        assert cfg["tpp"] == tpp and cfg["ppb"] == 1, cfg
    if lds is not None:
        assert cfg["lds_work"] == lds, cfg
    first = None
    for idx in (np.arange(B), np.arange(B)[::-1]):
        out = _call(hipldl, c, L, idx)
        be, fe = FB.check_outputs(c, out, idx, c["vals"][idx])
        print(f"tpp {cfg['tpp']} lds_work {cfg['lds_work']}: ok {out['ok'].tolist()} nfact {out['nf'].tolist()} backward {be / FB.EPS32:.1f} eps32 forward {fe:.2e}")
        first = first or out
    return first


def _decisions_equal(s, a, b):
    for k in ("ok", "nf"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("rho", "ro"):
        assert np.array_equal(FB.bits(a[k]), FB.bits(b[k])), k
    assert np.array_equal(FB.bits(a["vals"]), FB.bits(b["vals"]))      # (the rho slots, and the rest untouched)


# ---- 1. smallest shapes, panel edges; independent pivots ----
@pytest.mark.parametrize("lds", (1, 0), ids=("lds", "global"))
@pytest.mark.parametrize("n", FB.RANDOM_N)
def test_panel_edges(built, n, lds):
    """one front of n = 16 k - 1, 16 k, 16 k + 1 pivots on the float32_condense handle, 256 threads per problem, the work area in
    LDS and in global scratch"""
    hipldl, syn = _mods()
    c = FB.case(FB.random_shape(n))
    L = FB.handle(hipldl, c, FB.MIX, **FB.COND, **FB.KEY, **FB.FORCED, v1_lds=lds)
    assert L.config["float32_blocked"], L.config
    fr = L.plan_array("fronts").reshape(-1, 16)
    assert fr.shape[0] == 1 and fr[0, 0] == n and L.info["ncond"] > 0
    _run_mix(hipldl, c, L, tpp=256, lds=lds)
    L.close()


@pytest.mark.parametrize("lds", (1, 0), ids=("lds", "global"))
def test_independent_pivots(built, lds):
    """COND0 on the uncondensed Float32 general handle: the last front has 60 pivots, the leading 23 independent (one full panel of
    independent pivots and a narrow one, then dependent panels)"""
    hipldl, syn = _mods()
    c = FB.case(FB.COND0)
    L = FB.handle(hipldl, c, FB.MIX, **FB.UNCOND, **FB.KEY, **FB.FORCED, v1_lds=lds)
    assert L.config["float32_blocked"], L.config
    fr = L.plan_array("fronts").reshape(-1, 16)
    assert tuple(fr[-1, [0, 1, 14]]) == (60, 0, 23) and L.info["ncond"] == 0
    _run_mix(hipldl, c, L, tpp=256, lds=lds)
    L.close()


# ---- 2. fronts with update rows ----
@pytest.mark.parametrize("base", (FB.COND, FB.UNCOND), ids=("condensed", "uncondensed"))
def test_grid(built, base):
    """grid_structure(32): fronts with update rows — (21, 62), (31, 63), the root (93, 0) — and, uncondensed, a blocked front whose
    leading pivots are independent ((16, 13, 11)); fmax 95, so 256 threads per problem are forced"""
    hipldl, syn = _mods()
    c = FB.case(FB.GRID)
    L = FB.handle(hipldl, c, FB.MIX, **base, **FB.KEY, **FB.FORCED)
    fr = [tuple(int(x) for x in f[[0, 1, 14]]) for f in L.plan_array("fronts").reshape(-1, 16)]
    for w in [(21, 62, 0), (31, 63, 0), (93, 0, 0)] + ([] if "float32_condense" in base else [(16, 13, 11)]):
        assert w in fr, w
    _run_mix(hipldl, c, L, tpp=256)
    L.close()


# ---- 3. default configurations ----
def _placement(L):
    """work area in LDS or global scratch, read from the configuration and checked against the sizes it states"""
    cfg, fmax = L.config, L.info["fmax"]
    if cfg["lds_work"]:
        assert 16 * 4 + 16 * fmax * 4 < cfg["lds_bytes"] <= LDS_LIMIT, cfg      # (the header, the W panel and more)
    else:
        assert cfg["lds_bytes"] == 16 * 4, cfg
    return cfg["lds_work"]


@pytest.mark.parametrize("shape,extra,lds", [(FB.F97, {}, 1), (FB.F130, {}, 1), (FB.G450, {}, 0), (FB.F130, dict(float32_register_front=1), 1)],
                         ids=["fmax97", "fmax130", "fmax375", "fmax130-register-front-fell-back"])
def test_default_configurations(built, shape, extra, lds):
    """what choose_config picks with the key: 256 threads per problem above order 96, the work area — W panel included — in LDS at
    fmax 97 and 130, in global scratch at fmax 375; a float32_register_front handle whose front is above order 64 fell back to the
    float32_condense handle and is blocked like it"""
    hipldl, syn = _mods()
    c = FB.case(shape)
    L = FB.handle(hipldl, c, FB.MIX, **FB.COND, **FB.KEY, **extra)
    print(f"{FB.shape_id(shape)}: fmax {L.info['fmax']} config {L.config}")
    assert L.config["float32_blocked"], L.config
    assert _placement(L) == lds
    _run_mix(hipldl, c, L, tpp=256, lds=lds)
    L.close()


def test_fmax_96_runs_unblocked(built):
    """fmax 96: 64 threads per problem, no blocked instance — the handle is made, says so, and gives what the handle without the key
    gives, bit for bit"""
    hipldl, syn = _mods()
    c = FB.case(FB.F96)
    outs = []
    for key in (FB.KEY, {}):
        L = FB.handle(hipldl, c, FB.MIX, **FB.COND, **key)
        assert L.info["fmax"] == 96 and L.config["tpp"] == 64 and not L.config["float32_blocked"], L.config
        outs.append(_run_mix(hipldl, c, L, blocked=False))
        L.close()
    for k, a in outs[0].items():
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(outs[1][k]).tobytes(), k


# ---- 4. the two-call sequence ----
@pytest.mark.parametrize("shape,opt", [(FB.random_shape(33), FB.FORCED), (FB.F130, {}), (FB.G450, {})], ids=["n33", "fmax130", "fmax375"])
def test_two_call_sequence_and_inertia(built, shape, opt):
    """cnl_factorize_f32_dev (the blocked instance), then cnl_solve_f32_dev twice with different right-hand sides on that factor,
    vals untouched; then the host try_to_factorize with the inertia, equal to the oracle's counts on the widened data"""
    import torch
    from oracle import oracle as O
    hipldl, syn = _mods()
    c = FB.case(shape)
    s, B = c["s"], FB.MIX
    eig_tol = float(c["p32"][0])
    orc = G.oracle_of(O, s)
    ref = [orc.try_to_factorize(c["vals"][b].astype(np.float64), s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True) for b in range(B)]
    want = [bool(r[0]) for r in ref]
    assert want == [True, False, False, False, True]
    L = FB.handle(hipldl, c, B, **FB.COND, **FB.KEY, **opt)
    assert L.config["float32_blocked"] and L.config["kernel"] == "v1", L.config
    dev = "cuda:0"
    t_vals = torch.from_numpy(np.array(c["vals"])).to(dev)
    t_ok = torch.full((B,), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    hipldl.factorize_dev(L, t_vals, eig_tol, t_ok, stream=stream)
    for k in range(2):
        r = np.ascontiguousarray(c["rhs"] * np.float32(k + 1.5))
        t_r = torch.from_numpy(r).to(dev)
        t_d = torch.full((B, s.N), 7.0, dtype=torch.float32, device=dev)
        hipldl.solve_dev(L, t_r, t_d, stream=stream)
        torch.cuda.synchronize()
        assert t_ok.cpu().numpy().tolist() == [int(w) for w in want]
        d = t_d.cpu().numpy()
        for b in range(B):
            if want[b]:
                be = G.backward_error(s, c["vals"][b], r[b], d[b])
                assert be <= FB.BWD_TOL, (b, k, be)
            else:
                assert (d[b] == 7.0).all(), b      # no factor: the rows stay untouched
    assert np.array_equal(FB.bits(t_vals.cpu().numpy()), FB.bits(c["vals"]))
    ok, npos, nzer = hipldl.try_to_factorize(L, np.array(c["vals"]), s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True)
    assert list(ok) == want
    for b in range(B):
        if b % 5 != 1:     # (the hopeless problem's pivots are NaN: its counts mean nothing in either arithmetic)
            assert (int(npos[b]), int(nzer[b])) == (int(ref[b][1]), int(ref[b][2])), b
    L.close()


def test_solve_leaves_failed_rows_untouched(built):
    """The two-call sequence at n = 33 behind a device-pointer factorisation, condensed and uncondensed: with the key on the rows of d
    of a problem whose factorisation failed (the hopeless one and the two climbers, which try_to_factorize does not repair) stay at
    their 7.0 sentinel — the handle keeps the success flags of its last factorisation, the blocked float instance's MODE_SOLVE and the
    float expand pass read them.  With the key off the handle runs what it always ran; the test prints both counts."""
    import torch
    hipldl, syn = _mods()
    c = FB.case(FB.random_shape(33))
    s, B = c["s"], FB.MIX
    dev = "cuda:0"
    stream = torch.cuda.current_stream().cuda_stream
    touched = {}
    for key, base in ((0, FB.COND), (1, FB.COND), (1, FB.UNCOND)):
        L = FB.handle(hipldl, c, B, **base, **FB.FORCED, float32_blocked=key)
        assert L.config["float32_blocked"] == bool(key), L.config
        t_vals = torch.from_numpy(np.array(c["vals"])).to(dev)
        t_ok = torch.full((B,), -1, dtype=torch.int32, device=dev)
        hipldl.factorize_dev(L, t_vals, float(c["p32"][0]), t_ok, stream=stream)
        t_r = torch.from_numpy(np.array(c["rhs"])).to(dev)
        t_d = torch.full((B, s.N), 7.0, dtype=torch.float32, device=dev)
        hipldl.solve_dev(L, t_r, t_d, stream=stream)
        torch.cuda.synchronize()
        ok, d = t_ok.cpu().numpy(), t_d.cpu().numpy()
        assert ok.tolist() == [1, 0, 0, 0, 1]
        name = (key, "float32_condense" in base)
        touched[name] = {b: int((d[b] != 7.0).sum()) for b in range(B) if not ok[b]}
        print(f"float32_blocked={key} condensed={name[1]}: entries of d overwritten per failed problem {touched[name]} of {s.N}")
        for b in range(B):
            if ok[b]:
                assert G.backward_error(s, c["vals"][b], c["rhs"][b], d[b]) <= FB.BWD_TOL, (name, b)
        L.close()
    assert all(n == 0 for k in ((1, True), (1, False)) for n in touched[k].values()), touched


# ---- 5. key on against key off ----
@pytest.mark.parametrize("shape,base,opt", [(FB.random_shape(33), FB.COND, FB.FORCED), (FB.COND0, FB.UNCOND, FB.FORCED), (FB.F130, FB.COND, {})],
                         ids=["n33", "cond0-uncondensed", "fmax130"])
def test_key_on_against_key_off(built, shape, base, opt):
    """the same handle with and without the key: decisions bit-equal; d of either against the oracle within the bars, never against
    each other bit for bit"""
    hipldl, syn = _mods()
    c = FB.case(shape)
    B = FB.MIX
    outs = []
    for key in (1, 0):
        L = FB.handle(hipldl, c, B, **base, **opt, float32_blocked=key)
        assert L.config["float32_blocked"] == bool(key) and L.config["kernel"] == "v1" and L.config["tpp"] == 256, L.config
        outs.append(_call(hipldl, c, L, np.arange(B)))
        FB.check_outputs(c, outs[-1], np.arange(B), c["vals"])
        L.close()
    on, off = outs
    _decisions_equal(c["s"], on, off)
    ok = on["ok"].astype(bool)
    worst = np.abs(on["d"][ok].astype(np.float64) - off["d"][ok]).max() / np.abs(off["d"][ok]).max()
    print(f"{FB.shape_id(shape)}: d with the key on against off, largest difference {worst:.2e} of the largest entry (printed, not asserted)")


# ---- 6. batch effects ----
def test_batch_of_65(built):
    """65 different problems (thirteen mixes), one workgroup each"""
    hipldl, syn = _mods()
    c = FB.case(FB.random_shape(33), 65)
    L = FB.handle(hipldl, c, 65, **FB.COND, **FB.KEY, **FB.FORCED)
    assert L.config["grid"] == 65
    out = _run_mix(hipldl, c, L, tpp=256)
    assert out["ok"].tolist() == [int(FB.WANT_OK[b % 5]) for b in range(65)]
    L.close()


def test_host_entry_on_a_repeated_mix(built):
    """The host-pointer cnl_newton_system_f32 on the mix at n = 33 repeated thirteen times, work area in global scratch (every problem
    at its own offset into the enlarged work area and the factor panels): the first mix against the oracle, every repetition bit-equal
    to the first.  (A Float32 handle's host-pointer call is the device entry behind one upload: the chunked pipeline that runs a
    Float64 handle's large batches as sub-batch views does not exist in float, so no view of a Float32 handle is ever made; the
    shift of the kept flags for views is exercised by tests/test_general_blocked_gpu.py: test_sub_batch_slices.)"""
    hipldl, syn = _mods()
    c = FB.case(FB.random_shape(33))
    s, reps = c["s"], 13
    B = FB.MIX * reps
    L = FB.handle(hipldl, c, B, **FB.COND, **FB.KEY, **FB.FORCED, v1_lds=0)
    assert L.config["float32_blocked"] and not L.config["lds_work"] and L.config["grid"] == B, L.config
    vals, rhs, ro = (np.ascontiguousarray(np.tile(c[k], (reps,) + (1,) * (c[k].ndim - 1))) for k in ("vals", "rhs", "rho_old"))
    d, ok, rho, ro_out, nf = hipldl.newton_system_(np.full((B, s.N), 7.0, np.float32), s.nvar, s.nequ, s.ncon, rhs, vals, L, ro, c["p32"])
    out = dict(vals=vals, d=d, ok=np.asarray(ok).astype(np.int32), rho=rho, ro=ro_out, nf=np.asarray(nf))
    FB.check_outputs(c, {k: v[:FB.MIX] for k, v in out.items()}, np.arange(FB.MIX), c["vals"])
    for k, v in out.items():
        rep = np.asarray(v).reshape((reps, FB.MIX) + np.asarray(v).shape[1:])
        assert np.ascontiguousarray(rep).tobytes() == np.ascontiguousarray(np.broadcast_to(rep[:1], rep.shape)).tobytes(), k
    L.close()


def test_active_batch_prefix(built):
    """cnl_set_active_batch on a prefix of two mixes: the calls run on the first 7 problems and leave the arrays of the others
    alone; the flags kept behind the factorisation are those of the prefix, and solve leaves its failed rows untouched"""
    import torch
    hipldl, syn = _mods()
    c = FB.case(FB.random_shape(33), 2 * FB.MIX)
    s, B, nb = c["s"], 2 * FB.MIX, 7
    L = FB.handle(hipldl, c, B, **FB.COND, **FB.KEY, **FB.FORCED)
    assert L.config["float32_blocked"], L.config
    full = _call(hipldl, c, L, np.arange(B))
    FB.check_outputs(c, full, np.arange(B), c["vals"])
    hipldl.set_active_batch(L, nb)
    out = _call(hipldl, c, L, np.arange(B))      # (arrays of the whole batch, sentinels everywhere)
    FB.check_outputs(c, {k: v[:nb] for k, v in out.items()}, np.arange(nb), c["vals"][:nb])
    assert (out["d"][nb:] == 7.0).all() and (out["ok"][nb:] == -1).all() and (out["nf"][nb:] == -1).all() and (out["rho"][nb:] == -1.0).all()
    assert np.array_equal(FB.bits(out["vals"][nb:]), FB.bits(c["vals"][nb:]))
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
    assert ok.tolist() == [1, 0, 0, 0, 1, 1, 0] + [-1] * (B - nb)
    for b in range(B):
        if b < nb and ok[b] == 1:
            assert G.backward_error(s, c["vals"][b], c["rhs"][b], d[b]) <= FB.BWD_TOL, b
        else:
            assert (d[b] == 7.0).all(), b
    L.close()


# ---- 7. the key changes nothing elsewhere ----
def _same_with_and_without(hipldl, s, vals, rhs, base, kernel):
    rows, cols = s.kkt_pattern()
    B = vals.shape[0]
    p32 = hipldl.default_params(np.float32)
    res = []
    for extra in ({}, FB.KEY):
        L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32, options=hipldl.Options(**base, **extra))
        assert not L.config["float32_blocked"] and L.config["kernel"] == kernel, L.config
        v = vals.copy()
        d, ok, rho, ro_out, nf = hipldl.newton_system_(np.full((B, s.N), 7.0, np.float32), s.nvar, s.nequ, s.ncon, rhs.copy(), v, L, np.zeros(B, np.float32), p32)
        res.append(dict(vals=v, d=d, ok=np.asarray(ok).astype(np.int32), rho=rho, ro=ro_out, nf=np.asarray(nf)))
        L.close()
    assert res[0]["ok"].all()
    for name, a in res[0].items():
        b = res[1][name]
        assert a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), name


def test_key_changes_nothing_elsewhere(built):
    """a band pattern stays on the band kernels, a plan the register-front kernel serves stays on it, a pattern
    float32_general_dense takes stays on the dense route: float32_blocked False, the same kernel, the same bits"""
    hipldl, syn = _mods()
    sb = syn.band_structure(200, 4)
    _same_with_and_without(hipldl, sb, *G.band_inputs(syn, sb, range(4000, 4008)), FB.COND, "band")
    sr = syn.random_structure(60, 80, 4, 0.1, seed=3)
    _same_with_and_without(hipldl, sr, *G.random_inputs(syn, sr, range(100, 108)), dict(FB.COND, float32_register_front=1), "v2")
    c = FB.case(FB.F97)
    healthy = [0, 4]
    _same_with_and_without(hipldl, c["s"], c["vals"][healthy], c["rhs"][healthy], dict(FB.COND, float32_general_dense=1), "dense")


# ---- 8. refusals ----
def test_refusals_with_a_device(built):
    """the rules of tests/test_float32_blocked_cpu.py hold on a machine with a device, where the accepted combinations make a handle"""
    from tests import test_float32_blocked_cpu as cpu
    hipldl, syn = _mods()
    cpu.test_key_rules_without_a_device(True)
    c = FB.case(FB.random_shape(33))
    for base in (FB.COND, FB.UNCOND):
        L = FB.handle(hipldl, c, FB.MIX, **base, **FB.KEY)
        assert L.config["float32"] and L.config["kernel"] == "v1" and L.config["tpp"] == 64 and not L.config["float32_blocked"], L.config
        L.close()
    s = c["s"]
    for opt in (dict(float32_blocked=1), dict(float32_general=1, float32_blocked=2), dict(float32_general=1, general_blocked=1)):
        with pytest.raises(hipldl.CnlError) as e:
            FB.handle(hipldl, c, FB.MIX, **opt)
        assert e.value.code == CNL_ERR_ARG, str(e.value)
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=FB.MIX, options=hipldl.Options(float32_general=1, float32_refine=1, float32_blocked=1))
    assert e.value.code == CNL_ERR_ARG and "float32_blocked" in str(e.value), str(e.value)
