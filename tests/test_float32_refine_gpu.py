"""Refined handles (tuning float32_refine = k: a Float64 handle on an inner Float32 general handle, d corrected k times with a Float64
residual) and the residual kernel on its own (cnl_kkt_residual_dev).  -m gpu.

Bounds, notation and inputs: tests/support/f32_refine.py.  Both bounds are derived (a Float64 residual of m + 2 terms, converged
fixed-precision refinement, a factor 2 each) and asserted per problem against K from the caller's Float64 vals AS RETURNED, formed
in longdouble.  Decisions (success, nfact, rho, rho_old) are compared, widened and bit for bit, with the bare Float32 handle — the
code that existed before this feature — on the demoted inputs."""
import numpy as np
import pytest

from tests.support import f32_general as G
from tests.support import f32_refine as RF

pytestmark = pytest.mark.gpu

CNL_ERR_ARG, CNL_ERR_STATE = 1, 5
SENTINEL = np.frombuffer(np.uint64(0x7FF8DEADBEEF0001).tobytes(), np.float64)[0]   # a NaN with a payload


def _mods():
    import torch
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    return torch, hipldl, syn


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _handle(hipldl, s, B, dtype, **opt):
    rows, cols = s.kkt_pattern()
    return hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=dtype, options=hipldl.Options(**opt) if opt else None)


def _refined(hipldl, s, B, k=2, **opt):
    L = _handle(hipldl, s, B, np.float64, float32_general=1, float32_refine=k, **opt)
    assert L.config["refine"] == k and not L.config["float32"] and not L.config["band"], L.config
    return L


def _bare(hipldl, s, B, **opt):
    return _handle(hipldl, s, B, np.float32, float32_general=1, band_kernel=0, **opt)


def _newton_dev(L, vals, rhs, params, d0=None, rho_old=0.0):
    """newton_system! on device pointers, in the handle's element type; returns host arrays (vals: as the call left them)"""
    torch, hipldl, _ = _mods()
    T = L.dtype
    B, N = rhs.shape
    tv, tr = _dev(torch, vals.astype(T)), _dev(torch, rhs.astype(T))
    td = _dev(torch, np.full((B, N), SENTINEL if T == np.float64 else np.nan, T) if d0 is None else d0.astype(T))
    tro, trho = _dev(torch, np.full(B, rho_old, T)), _dev(torch, np.zeros(B, T))
    tnf, tok = _dev(torch, np.zeros(B, np.int32)), _dev(torch, np.zeros(B, np.int32))
    hipldl.newton_system_dev(L, tv, tr, td, tro, trho, tnf, tok, params, 0)
    torch.cuda.synchronize()
    return {"d": td.cpu().numpy(), "vals": tv.cpu().numpy(), "ok": tok.cpu().numpy(), "rho": trho.cpu().numpy(), "ro": tro.cpu().numpy(),
            "nf": tnf.cpu().numpy()}


def _same_decisions(got, bare):
    assert np.array_equal(got["ok"], bare["ok"]) and np.array_equal(got["nf"], bare["nf"]), (got["ok"], bare["ok"], got["nf"], bare["nf"])
    assert got["rho"].dtype == np.float64 and bare["rho"].dtype == np.float32
    assert np.array_equal(_bits(got["rho"]), _bits(bare["rho"].astype(np.float64)))
    assert np.array_equal(_bits(got["ro"]), _bits(bare["ro"].astype(np.float64)))


# ---- 1. the residual kernel alone ----
@pytest.mark.parametrize("rows_mode", [1, 2])
@pytest.mark.parametrize("name, B", RF.RESIDUAL_CASES)
def test_residual_kernel(built, name, B, rows_mode):
    torch, hipldl, syn = _mods()
    s, vals, rhs, d = RF.residual_inputs(syn, name, B)
    # (a Float64 handle without the key; the throughput plan off the dense backend, so that cnl_set_active_batch is served below —
    #  the dense backend and the staged execution of small batches refuse it, and the residual kernel does not care what factorises)
    L = _handle(hipldl, s, B, np.float64, refine_rows=rows_mode, plan_kind=hipldl.PLAN_THROUGHPUT, dense_backend=0)
    assert not L.config["refine"] and L.config["kernel"] != "dense"
    tv, tr, td = _dev(torch, vals), _dev(torch, rhs), _dev(torch, d)
    tg, tn = _dev(torch, np.full((B, s.N), SENTINEL)), _dev(torch, np.full(B, SENTINEL))
    hipldl.kkt_residual_dev(L, tv, tr, td, tg, tn)
    torch.cuda.synchronize()
    g, norms = tg.cpu().numpy(), tn.cpu().numpy()
    m = RF.max_row_entries(s)
    for b in range(B):
        ref, scale = RF.residual_long(s, vals[b], rhs[b], d[b])
        assert (np.abs(g[b].astype(np.longdouble) - ref) <= (m + 2) * RF.EPS64 * scale).all(), (name, b)
        assert norms[b] == np.abs(g[b]).max()
    # two calls are bit-equal; a null norms pointer is allowed
    tg2 = _dev(torch, np.zeros((B, s.N)))
    hipldl.kkt_residual_dev(L, tv, tr, td, tg2, None)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(tg2.cpu().numpy()), _bits(g))
    # fewer active problems: the rows beyond keep a sentinel bit for bit
    nb = B - 1
    hipldl.set_active_batch(L, nb)
    tg3, tn3 = _dev(torch, np.full((B, s.N), SENTINEL)), _dev(torch, np.full(B, SENTINEL))
    hipldl.kkt_residual_dev(L, tv, tr, td, tg3, tn3)
    torch.cuda.synchronize()
    g3, n3 = tg3.cpu().numpy(), tn3.cpu().numpy()
    assert np.array_equal(_bits(g3[:nb]), _bits(g[:nb])) and np.array_equal(_bits(n3[:nb]), _bits(norms[:nb]))
    assert (_bits(g3[nb:]) == _bits(SENTINEL)).all() and (_bits(n3[nb:]) == _bits(SENTINEL)).all()
    L.close()


def test_residual_kernel_refusals(built):
    torch, hipldl, syn = _mods()
    lib = hipldl.lib()
    assert lib.cnl_kkt_residual_dev(None, 8, 8, 8, 8, None, None) == CNL_ERR_ARG
    s = syn.band_structure(200, 4)
    Li = _handle(hipldl, s, 40, np.float64, plan_kind=hipldl.PLAN_THROUGHPUT, batch_layout=hipldl.LAYOUT_INTERLEAVED)
    assert Li.config["batch_layout"] == 1
    t = _dev(torch, np.zeros(hipldl.layout_len(Li, 0)))
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.kkt_residual_dev(Li, t, t, t, t, None)
    assert e.value.code == CNL_ERR_STATE
    Li.close()
    with pytest.raises(hipldl.CnlError) as e:   # a handle made without the key has no refinement norms
        Lp = _handle(hipldl, syn.dense_structure(6, 9), 2, np.float64)
        try:
            hipldl.refine_norms(Lp)
        finally:
            Lp.close()
    assert e.value.code == CNL_ERR_STATE


# ---- 2. refined newton_system!, one case per inner route ----
ROUTES = [("general", "random", {}), ("condense", "random", dict(float32_condense=1)),
          ("register_front", "band", dict(float32_register_front=1)),
          ("direct_records", "band", dict(float32_register_front=1, float32_direct_records=1)),
          ("dense", "dense", dict(float32_dense=1)), ("general_dense", "random-large-front", dict(float32_general_dense=2))]


@pytest.mark.parametrize("route, name, opt", ROUTES, ids=[r[0] for r in ROUTES])
def test_refined_newton_system(built, route, name, opt):
    torch, hipldl, syn = _mods()
    s, vals, rhs = RF.inputs(syn, name)
    B = vals.shape[0]
    p64, p32 = RF.demoted_params(hipldl)
    Lb = _bare(hipldl, s, B, **opt)
    bare = _newton_dev(Lb, vals, rhs, p32)
    assert bare["ok"].all()
    L = _refined(hipldl, s, B, 2, **opt)
    # the route is the bare Float32 handle's
    for key in ("kernel", "direct", "v2_solve", "cond_resident", "tpp", "ppb", "wpb"):
        assert L.config[key] == Lb.config[key], (key, L.config, Lb.config)
    assert L.info["ncond"] == Lb.info["ncond"]
    got = _newton_dev(L, vals, rhs, p64)
    _same_decisions(got, bare)
    assert np.array_equal(_bits(got["vals"]), _bits(vals))   # nothing climbed: vals untouched
    worst = [max(r) for r in zip(*(RF.check_bounds(s, got["vals"][b], rhs[b], got["d"][b], f"{route}[{b}]") for b in range(B)))]
    norms = hipldl.refine_norms(L)
    print(f"{route}: worst omega / bound {worst[0]:.3f}, worst forward / bound {worst[1]:.2e}, norms {norms.max(axis=0)}")
    assert norms.shape == (B, 2) and (norms[:, 1] < norms[:, 0] / RF.CONTRACTION).all(), norms
    L.close()
    # one step already gains more than 1000 on the raw Float32 solution
    L1 = _refined(hipldl, s, B, 1, **opt)
    one = _newton_dev(L1, vals, rhs, p64)
    for b in range(B):
        w1, w0 = RF.omega(s, vals[b], rhs[b], one["d"][b]), RF.omega(s, vals[b], rhs[b], bare["d"][b].astype(np.float64))
        assert w1 <= w0 / 1000, (route, b, w1, w0)
    L1.close()
    Lb.close()


# ---- 3. ladder and failure inside one workgroup ----
def test_ladder_and_failure_in_one_workgroup(built):
    torch, hipldl, syn = _mods()
    from oracle import oracle as O
    s, vals, rhs = RF.mixed_ladder_inputs(syn)
    B = vals.shape[0]
    p64, p32 = RF.demoted_params(hipldl, RF.RHO_MAX_SMALL)
    # (the MARGIN discipline: no oracle pivot near eig_tol, so float rounding cannot flip a decision)
    ref = G.oracle_newton(O, s, vals.astype(np.float32), rhs.astype(np.float32), np.zeros(B, np.float32), p32)
    Lb = _bare(hipldl, s, B, v1_ppb=4)
    bare = _newton_dev(Lb, vals, rhs, p32)
    L = _refined(hipldl, s, B, 2, v1_ppb=4)   # problems 4 .. 7 share a workgroup
    got = _newton_dev(L, vals, rhs, p64)
    _same_decisions(got, bare)
    assert np.array_equal(got["ok"].astype(bool), ref["ok"]) and np.array_equal(got["nf"], ref["nf"])
    c, f = RF.CLIMBS, RF.FAILS
    assert got["nf"][c] > 1 and got["rho"][c] > 0 and got["ok"][c] == 1
    assert (got["vals"][c, -s.nvar:] == got["rho"][c]).all()
    others = [b for b in range(B) if b not in (c, f)]
    assert np.array_equal(_bits(got["vals"][others]), _bits(vals[others]))
    norms = hipldl.refine_norms(L)
    for b in range(B):
        if b != f:
            RF.check_bounds(s, got["vals"][b], rhs[b], got["d"][b], f"mixed[{b}]")
            assert norms[b, 1] < norms[b, 0] / RF.CONTRACTION
    assert got["ok"][f] == 0 and (_bits(got["d"][f]) == _bits(SENTINEL)).all() and (norms[f] == -1).all()
    L.close()
    Lb.close()


# ---- 4. two-call sequence ----
def test_factorize_then_two_solves(built):
    torch, hipldl, syn = _mods()
    s, vals, rhs = RF.inputs(syn, "random")
    B = vals.shape[0]
    p64, _ = RF.demoted_params(hipldl)
    L = _refined(hipldl, s, B, 2, float32_condense=1)
    tr, td = _dev(torch, rhs), _dev(torch, np.zeros((B, s.N)))
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.solve_dev(L, tr, td)
    assert e.value.code == CNL_ERR_STATE
    tv, tok = _dev(torch, vals), _dev(torch, np.zeros(B, np.int32))
    hipldl.factorize_dev(L, tv, p64[0], tok)
    for seed in (1, 2):
        r2 = rhs if seed == 1 else np.random.default_rng(seed).normal(size=rhs.shape)
        tr = _dev(torch, r2)
        hipldl.solve_dev(L, tr, td)
        torch.cuda.synchronize()
        assert tok.cpu().numpy().all()
        d = td.cpu().numpy()
        for b in range(B):
            RF.check_bounds(s, vals[b], r2[b], d[b], f"solve {seed}[{b}]")
    # a factorisation of fewer problems, then the handle widened again: the solve is refused, as on every handle
    hipldl.set_active_batch(L, 5)
    hipldl.factorize_dev(L, tv, p64[0], tok)
    hipldl.set_active_batch(L, B)
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.solve_dev(L, tr, td)
    assert e.value.code == CNL_ERR_STATE
    L.close()


# ---- 5. host-pointer calls ----
def test_host_pointer_calls_equal_device_pointer_calls(built):
    torch, hipldl, syn = _mods()
    s, vals, rhs = RF.mixed_ladder_inputs(syn)
    B = vals.shape[0]
    p64, _ = RF.demoted_params(hipldl, RF.RHO_MAX_SMALL)
    L = _refined(hipldl, s, B, 2)
    dev = _newton_dev(L, vals, rhs, p64)
    v, d0 = vals.copy(), np.full((B, s.N), SENTINEL)
    d, ok, rho, ro, nf = hipldl.newton_system_(d0, s.nvar, s.nequ, s.ncon, rhs, v, L, np.zeros(B), p64)
    assert np.array_equal(_bits(d), _bits(dev["d"])) and np.array_equal(_bits(rho), _bits(dev["rho"])) and np.array_equal(_bits(ro), _bits(dev["ro"]))
    assert np.array_equal(nf, dev["nf"]) and np.array_equal(ok, dev["ok"].astype(bool))
    assert np.array_equal(_bits(v), _bits(dev["vals"]))
    # try_to_factorize / solve_ldl! on host pointers: the solution of the newton call for every problem that needed no rho
    ok2, npos, nzer = hipldl.try_to_factorize(L, vals, s.nvar, s.nequ, s.ncon, p64[0], return_inertia=True)
    plain = [b for b in range(B) if dev["nf"][b] == 1]
    assert ok2[plain].all() and not ok2[RF.CLIMBS] and (npos[plain] == s.nvar).all() and (nzer[plain] == 0).all()
    d2 = np.full((B, s.N), SENTINEL)
    hipldl.solve_ldl_(rhs, L.factor, d2)
    assert np.array_equal(_bits(d2[plain]), _bits(dev["d"][plain]))
    assert (_bits(d2[RF.CLIMBS]) == _bits(SENTINEL)).all()
    L.close()


# ---- 6. refusals ----
def test_refusals(built):
    torch, hipldl, syn = _mods()
    s = syn.random_structure(60, 80, 4, 0.1, 1)
    rows, cols = s.kkt_pattern()
    for dtype, opt, word in [(np.float64, dict(float32_refine=2), "float32_general"), (np.float64, dict(float32_general=1, float32_refine=5), "0 (none) .. 4"),
                             (np.float32, dict(float32_general=1, float32_refine=2), "cnl_create_ex"),
                             (np.float64, dict(float32_general=1, float32_refine=2, batch_layout=hipldl.LAYOUT_INTERLEAVED), "INTERLEAVED")]:
        with pytest.raises(hipldl.CnlError) as e:
            _handle(hipldl, s, 4, dtype, **opt)
        assert e.value.code == CNL_ERR_ARG and word in str(e.value), str(e.value)
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.MultiHIPLDLStruct(s.N, rows, cols, s.nvar, s.nequ, s.ncon, 4, [0], options=hipldl.Options(float32_general=1, float32_refine=2))
    assert e.value.code == CNL_ERR_ARG and "cnl_multi_create_ex" in str(e.value)
    # every _f32 entry point on a refined handle: CNL_ERR_STATE, nothing launched
    L = _refined(hipldl, s, 4, 2)
    lib = hipldl.lib()
    t = _dev(torch, np.zeros(4 * s.nnzNS, np.float32))
    ti = _dev(torch, np.zeros(4, np.int32))
    p, ip = t.data_ptr(), ti.data_ptr()
    p32 = hipldl.default_params(np.float32)
    c0 = hipldl.launch_counts()
    host = np.zeros(4 * s.nnzNS, np.float32).ctypes.data
    hosti = np.zeros(8, np.int64).ctypes.data
    assert lib.cnl_factorize_f32_dev(L._h, p, 1e-7, ip, None) == CNL_ERR_STATE
    assert lib.cnl_solve_f32_dev(L._h, p, p, None) == CNL_ERR_STATE
    assert lib.cnl_newton_system_f32_dev(L._h, p, p, p, p, p, ip, ip, p32.ctypes.data, None) == CNL_ERR_STATE
    assert lib.cnl_factorize_f32(L._h, host, 1e-7, hosti, None, None) == CNL_ERR_STATE
    assert lib.cnl_solve_f32(L._h, host, host) == CNL_ERR_STATE
    assert lib.cnl_newton_system_f32(L._h, host, host, host, host, p32.ctypes.data, host, host, hosti, hosti) == CNL_ERR_STATE
    assert lib.cnl_residual_vectors_f32_dev(L._h, p, p, p, p, p, p, p, None) == CNL_ERR_STATE
    assert lib.cnl_cgls_multipliers_f32_dev(L._h, p, p, p, p, 1e-6, 1e-6, 10, 0, ip, None) == CNL_ERR_STATE
    assert lib.cnl_trial_point_f32_dev(L._h, p, p, p, p, 1.0, p, p, p, p, None) == CNL_ERR_STATE
    assert lib.cnl_prepare_newton_system_f32_dev(L._h, 0, 0, 0, 0, p, p, p, p, p, p, None) == CNL_ERR_STATE
    assert lib.cnl_interleave_f32_dev(L._h, 0, p, p, None) == CNL_ERR_STATE
    torch.cuda.synchronize()
    assert hipldl.launch_counts() == c0
    L.close()


# ---- 7. active batch ----
def test_active_batch(built):
    torch, hipldl, syn = _mods()
    s, vals, rhs = RF.inputs(syn, "random")
    B = vals.shape[0]
    p64, _ = RF.demoted_params(hipldl)
    L = _refined(hipldl, s, B, 2)
    full = _newton_dev(L, vals, rhs, p64)
    hipldl.set_active_batch(L, 5)
    assert hipldl.get_active_batch(L) == 5
    part = _newton_dev(L, vals, rhs, p64)
    assert np.array_equal(_bits(part["d"][:5]), _bits(full["d"][:5])) and np.array_equal(part["nf"][:5], full["nf"][:5])
    assert (_bits(part["d"][5:]) == _bits(SENTINEL)).all() and (part["ok"][5:] == 0).all()
    L.close()
    sd, _, _ = RF.inputs(syn, "dense")
    Ld = _refined(hipldl, sd, 3, 2, float32_dense=1)
    assert Ld.config["kernel"] == "dense"
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.set_active_batch(Ld, 2)
    assert e.value.code == CNL_ERR_STATE
    Ld.close()


# ---- 8. the lockstep loop in Float64 on a refined handle ----
def test_lockstep_loop_on_a_refined_handle(built):
    torch, hipldl, syn = _mods()
    from cannoles_jl_amd import device_loop as DL
    B, p = 16, 2
    fam = DL.BandQuadFamily(syn.band_structure(60, p, hw=3), B, seed=62, torch=torch, device="cuda:0", dtype=np.float64)
    got = DL.solve_batch_device(fam, tuning={"float32_general": 1, "float32_register_front": 1, "float32_refine": 2})
    assert got["dtype"] == "float64" and got["vals_layout"] == "problem-major"
    assert got["status"] == ["first_order"] * B, got["status"]
    for b in range(B):
        M = fam.host_model(b)
        x, r, lam = got["solution"][b], got["r"][b], got["multipliers"][b]
        J, F, Jc, c = M.jac_residual(x), M.residual(x), M.jac(x), M.cons(x)
        normdual, normprimal = np.abs(J.T @ r - Jc.T @ lam).max(), np.abs(np.concatenate([F - r, c])).max()
        ds = max(100.0, np.abs(lam).sum() / p) / 100.0
        # (self-certifying: the optimality measure at the returned point, recomputed in numpy, within the tolerance of the call; the
        #  two evaluations differ by Float64 rounding of sums of at most N terms)
        slack = 2 * fam.s.N * RF.EPS64 * max(1.0, np.abs(J).sum(axis=0).max() * max(np.abs(r).max(), 1.0))
        assert max(normdual / ds, normprimal) <= got["epstol"][b] + slack, (b, normdual / ds, normprimal, got["epstol"][b])
