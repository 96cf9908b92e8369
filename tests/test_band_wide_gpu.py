"""The wide band kernel instances (csrc/band.hip: band_newton_kernel<T, NL, 20>) on the GPU.  -m gpu.

Model-shaped patterns — the H_c segment filled with the model's whole Hessian structure, as the reference's src/CaNNOLeS.jl:256,
:288-291 fills it: synthetic.model_band_structure — reach the band kernels through the wide form of the band program, in Float64
and in Float32 (where cnl_create_f32 used to refuse them).  Bounds: those of tests/test_gpu_parity.py for the band kernels (FWD_TOL,
BWD_TOL, decisions identical to the oracle's) and of tests/test_float32_gpu.py (BWD_TOL, FWD_TOL, MARGIN), unchanged.  On a pattern
fifteen pieces serve the wide instances must reproduce the 15-piece ones bit for bit (tuning band_pieces = 20 against default)."""
import numpy as np
import pytest

from tests.support import f32_rows as R
from tests.test_gpu_parity import BWD_TOL, FWD_TOL, _band_opts, _mods, backward_error, run_case
from tests import test_float32_gpu as F32
from tests import test_float32_rows_gpu as F32R

pytestmark = pytest.mark.gpu

CNL_ERR_ARG = 1


def _model_values(syn, s, B, cfg=4, ladder=(), hopeless=None):
    vals, rhs = syn.batch_values(s, B, cfg=cfg, gen=syn.model_band_values)
    for b in ladder:
        vals[b], rhs[b] = syn.model_band_values(s, 5000 + b, stress="ladder")
    if hopeless is not None:
        vals[hopeless, s.offsets()[0]] = -1e300
    return vals, rhs


def _model_batch(syn, s, B, seed):
    """vectorised values of B problems of model_band_structure: bench.band_batch on the band_structure twin (H_c diagonal), moved into the
    model-shaped layout, small entries on the off-diagonal H_c positions"""
    import bench as BM
    twin = syn.band_structure(s.nvar, s.ncon, hw=s.meta["hw"])
    v0, rhs = BM.band_batch(twin, B, seed)
    o0, o1 = twin.offsets(), s.offsets()
    vals = np.zeros((B, s.nnzNS))
    vals[:, o1[0]:o1[1]] = v0[:, o0[0]:o0[1]]
    r, c = np.asarray(s.hc[0]), np.asarray(s.hc[1])
    hcv = np.random.default_rng(seed + 1).uniform(-0.01, 0.01, (B, len(r)))
    hcv[:, r == c] = v0[:, o0[1]:o0[2]]
    vals[:, o1[1]:o1[2]] = hcv
    vals[:, o1[2]:] = v0[:, o0[2]:]
    return vals, rhs


def _run_dev(s, vals, rhs, ro_h, dtype=np.float64, keep=None, **opt):
    """try_to_factorize -> solve_ldl!, then newton_system!, device-resident on one handle; `vals` interleaved when the handle's layout
    is.  Returns the handle's config and [success of the factorisation, d of the two calls, d, rho_old, rho, nfact, success, vals after];
    keep = problem indices: vals after = those rows and, behind them, everybody's rho slots (large batches of large problems)."""
    import torch
    hipldl, syn, O = _mods()
    rows, cols = s.kkt_pattern()
    B = vals.shape[0]
    dev = torch.device("cuda", 0)
    tt = torch.float64 if dtype == np.float64 else torch.float32
    L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=dtype, options=hipldl.Options(**opt) if opt else None)
    cfg = dict(L.config)
    p_ = hipldl.default_params(dtype)
    tv = torch.from_numpy(np.ascontiguousarray(vals, dtype)).to(dev)
    tr = torch.from_numpy(np.ascontiguousarray(rhs, dtype)).to(dev)
    tin = tv
    if cfg["batch_layout"]:
        assert hipldl.layout_len(L, 0) == hipldl.il_len(B, s.nnzNS)
        tin = torch.full((hipldl.layout_len(L, 0),), 9.0, dtype=tt, device=dev)
        hipldl.interleave_dev(L, 0, tv, tin)
    su = torch.zeros(B, dtype=torch.int32, device=dev)
    d2 = torch.full((B, s.N), 7.0, dtype=tt, device=dev)
    hipldl.factorize_dev(L, tin, float(p_[0]), su)
    hipldl.solve_dev(L, tr, d2)
    d = torch.full((B, s.N), 3.0, dtype=tt, device=dev)
    ro, rho = torch.from_numpy(np.ascontiguousarray(ro_h, dtype)).to(dev), torch.zeros(B, dtype=tt, device=dev)
    nf, ok = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    hipldl.newton_system_dev(L, tin, tr, d, ro, rho, nf, ok, p_)
    if cfg["batch_layout"]:
        hipldl.deinterleave_dev(L, 0, tin, tv)
    torch.cuda.synchronize()
    if keep is not None:
        tv = torch.cat([tv[torch.from_numpy(np.asarray(keep)).to(dev)].reshape(-1), tv[:, -s.nvar:].reshape(-1)])
    out = [x.cpu().numpy() for x in (su, d2, d, ro, rho, nf, ok, tv)]
    L.close()
    return cfg, out


def _bit_equal(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ---- Float64, model-shaped patterns --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,p,B,nl", [(300, 4, 5, 16), (1000, 10, 37, 8), (1000, 10, 70, 16), (1000, 10, 37, 0), (10000, 50, 33, 16), (10000, 50, 20, 8)])
def test_wide_kernels_against_the_oracle(built, n, p, B, nl):
    """a small batch with the throughput plan forced: decisions identical to the oracle's on the product's order and on the canonical
    one, d within the forward / backward bar of the band kernels; 8 and 16 problems per workgroup (Float64 has no wide instance of 32)"""
    hipldl, syn, O = _mods()
    s = syn.model_band_structure(n, p)
    vals, rhs = _model_values(syn, s, B)
    info, cfg = run_case(s, vals, rhs, options=_band_opts(hipldl, band_pieces=20, band_problems_per_group=nl))
    assert cfg["band"] and cfg["band_pieces"] == 20 and cfg["band_nl"] == (nl or 16)


def test_wide_kernels_ladder_hopeless_and_rho_old(built):
    """ladder climbers (nfact = 6), a problem no rho rescues (d untouched, rho_old kept), starts from rho_old > 0 — mixed with convex
    problems in one workgroup"""
    hipldl, syn, O = _mods()
    s = syn.model_band_structure(600, 6)
    B = 21
    vals, rhs = _model_values(syn, s, B, ladder=(1, 5, 17, 20), hopeless=9)
    ro = np.zeros(B)
    ro[5] = 0.3
    ro[2] = 1e-3
    info, cfg = run_case(s, vals, rhs, rho_old=ro, options=_band_opts(hipldl, band_pieces=20))
    assert cfg["band"] and cfg["band_pieces"] == 20


def test_no_wide_float64_instance_of_32_problems(built):
    """the Float64 instance of 32 problems per workgroup would spill: asking for it is CNL_ERR_ARG, not a slower kernel"""
    hipldl, syn, O = _mods()
    s = syn.model_band_structure(300, 4)
    rows, cols = s.kkt_pattern()
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=64, options=_band_opts(hipldl, band_pieces=20, band_problems_per_group=32))
    assert e.value.code == CNL_ERR_ARG
    # Float64 runs the wide program on request only — the register-front kernel measured faster on this pattern:
    # default options and band_pieces = 15 keep it, as before
    for opt in ({}, {"band_pieces": 15}):
        L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=64, options=_band_opts(hipldl, **opt))
        assert not L.config["band"] and L.config["band_pieces"] == 0 and L.config["kernel"] == "v2"
        L.close()


@pytest.mark.parametrize("n,p,B", [(1000, 10, 8192 + 72), (10000, 50, 8192 + 40)])
def test_wide_kernels_large_batch_both_layouts(built, n, p, B):
    """a batch above 8 192 problems through cnl_newton_system_dev: a random sample of 32 problems against the oracle (one climbs the rho
    ladder inside a workgroup of convex ones, one is hopeless), `vals` interleaved bit-equal to problem-major in every output, and
    try_to_factorize -> solve_ldl! bit-equal in d to the fused call where nothing climbed"""
    hipldl, syn, O = _mods()
    s = syn.model_band_structure(n, p)
    rng = np.random.default_rng(5)
    pick = np.sort(rng.choice(B, 32, replace=False))
    vals, rhs = np.empty((B, s.nnzNS)), np.empty((B, s.N))
    for b0 in range(0, B, 512):
        nb = min(512, B - b0)
        vals[b0:b0 + nb], rhs[b0:b0 + nb] = _model_batch(syn, s, nb, seed=9000 + b0)
    climber, hopeless = int(pick[7]), int(pick[20])
    vals[climber], rhs[climber] = syn.model_band_values(s, 5000 + climber, stress="ladder")
    vals[hopeless, s.offsets()[0]] = -1e300
    ro_h = np.zeros(B)
    ro_h[int(pick[3])] = 0.3
    cfg_pm, pm = _run_dev(s, vals, rhs, ro_h, keep=pick, band_pieces=20)
    cfg_il, il = _run_dev(s, vals, rhs, ro_h, keep=pick, band_pieces=20, batch_layout=hipldl.LAYOUT_INTERLEAVED)
    for cfg, layout in ((cfg_pm, 0), (cfg_il, 1)):
        assert cfg["band"] and cfg["band_pieces"] == 20 and cfg["band_nl"] == 16 and cfg["batch_layout"] == layout and not cfg["float32"]
    assert _bit_equal(pm, il)
    su, d_two, d, ro_o, rho, nf, ok, v_kept = pm
    v_after = dict(zip((int(b) for b in pick), v_kept[:32 * s.nnzNS].reshape(32, s.nnzNS)))
    assert ok.sum() == B - 1 and not ok[hopeless] and np.all(d[hopeless] == 3.0) and np.all(d_two[hopeless] == 7.0)
    assert nf[climber] == 6 and not su[climber] and int((nf > 1).sum()) == 2
    quiet = np.ones(B, bool)
    quiet[[climber, hopeless]] = False
    assert su[quiet].all() and np.array_equal(d_two[quiet], d[quiet])
    rows, cols = s.kkt_pattern()
    orc = O.Oracle(s.N, rows, cols, O.canonical_perm(s.nvar, s.nequ, s.ncon))
    for b in pick:
        v0 = vals[b].copy()
        d0, ok0, rho0, ro0, nf0 = O.newton_system(orc, s.nvar, s.nequ, s.ncon, rhs[b], v0, float(ro_h[b]), O.default_params())
        assert bool(ok[b]) == bool(ok0) and nf[b] == nf0 and rho[b] == rho0 and ro_o[b] == ro0, b
        assert np.array_equal(v_after[int(b)][-s.nvar:], v0[-s.nvar:])
        if ok0:
            assert np.abs(d[b] - d0).max() <= FWD_TOL * np.abs(d0).max()
            assert backward_error(s, v0, rhs[b], d[b]) <= BWD_TOL


# ---- bit-equality of the wide instances on patterns both forms run -----------------------------------------------------------------------

# (Float64 has no wide instance of 32 problems per workgroup: test_no_wide_float64_instance_of_32_problems)
BIT_EQUAL_CASES = [(n, p, B, nl, dt) for dt in (np.float64, np.float32)
                   for n, p, B, nl in [(1000, 10, 75, 8), (1000, 10, 75, 16), (1000, 10, 75, 32), (10000, 50, 70, 16), (10000, 50, 70, 32), (1000, 10, 8192 + 40, 0)]
                   if not (dt == np.float64 and nl == 32)]


@pytest.mark.parametrize("n,p,B,nl,dtype", BIT_EQUAL_CASES)
def test_wide_instances_are_bit_equal_to_the_fifteen_piece_ones(built, n, p, B, nl, dtype):
    """band_structure with band_pieces = 20 against default options: same steps, same arithmetic, so every output — flags, d of both
    call sequences, rho, rho_old, nfact, the rho slots — is identical, in both layouts.  (Above 8 192 problems the 15-piece Float64
    handle runs 32 problems per workgroup and the wide one 16: the instances differ in how records travel, not in arithmetic.)"""
    hipldl, syn, O = _mods()
    s = syn.band_structure(n, p)
    if B > 1000:
        v8, r8 = syn.batch_values(s, 8, cfg=3)
        rng = np.random.default_rng(5)
        vals = np.tile(v8, (B // 8 + 1, 1))[:B] * (1.0 + 1e-3 * rng.standard_normal((B, 1)))
        rhs = np.tile(r8, (B // 8 + 1, 1))[:B] + 1e-3 * np.arange(B)[:, None]
        vals[:, s.offsets()[4]:s.offsets()[5]] = -1.0
    else:
        vals, rhs = syn.batch_values(s, B, cfg=4)
    for b in (1, 36, B - 1):
        vals[b], rhs[b] = syn.band_values(s, 5000 + b, stress="ladder")
    vals[3, s.offsets()[0]] = -1e300 if dtype == np.float64 else -1e30   # hopeless in either type (rho_max = eps^-2)
    ro_h = np.zeros(B)
    ro_h[4] = 0.3
    for layout in (0, 1):
        kw = dict(plan_kind=hipldl.PLAN_THROUGHPUT, batch_layout=layout)
        if nl:
            kw["band_problems_per_group"] = nl
        c15, o15 = _run_dev(s, vals, rhs, ro_h, dtype, **kw)
        c20, o20 = _run_dev(s, vals, rhs, ro_h, dtype, band_pieces=20, **kw)
        assert c15["band"] and c15["band_pieces"] == 15 and c20["band"] and c20["band_pieces"] == 20
        assert c15["batch_layout"] == c20["batch_layout"] == layout
        assert _bit_equal(o15, o20)
        assert o20[5][1] > 1 and not o20[6][3] and o20[6].sum() == B - 1


# ---- Float32, model-shaped patterns --------------------------------------------------------------------------------------------------

def _f32_model_inputs(syn, s, B, stress=None):
    vr = [syn.model_band_values(s, (7000 if stress else 4000) + b, stress=stress) for b in range(B)]
    return (np.ascontiguousarray(np.stack([v for v, _ in vr]), np.float32), np.ascontiguousarray(np.stack([r for _, r in vr]), np.float32))


@pytest.mark.parametrize("B,stress", [(1, None), (24, "ladder"), (256, None)])
def test_float32_model_shaped_against_the_oracle(built, B, stress):
    """cnl_create_f32 accepts the model-shaped pattern (it used to answer CNL_ERR_ARG) and the handle is held to
    tests/test_float32_gpu.py's check, unchanged"""
    hipldl, syn, O = _mods()
    s = syn.model_band_structure(1000, 10) if stress is None else syn.model_band_structure(400, 4)
    vals, rhs = _f32_model_inputs(syn, s, B, stress)
    rows, cols = s.kkt_pattern()
    L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32)
    assert L.config["float32"] and L.config["band"] and L.config["band_pieces"] == 20
    L.close()
    ok, nf = F32.check_against_oracle(hipldl, syn, O, s, vals, rhs, bwd_rows=range(0, B, 5))
    assert ok.all() and ((nf > 1).all() if stress else (nf == 1).all())


@pytest.mark.parametrize("nl", [8, 16, 32])
def test_float32_wide_instances(built, nl):
    hipldl, syn, O = _mods()
    s = syn.model_band_structure(1000, 10)
    vals, rhs = _f32_model_inputs(syn, s, 70)
    F32.check_against_oracle(hipldl, syn, O, s, vals, rhs, options=hipldl.Options(band_problems_per_group=nl), expect_nl=nl, bwd_rows=[0, 7, 8, 31, 32, 69])


def test_float32_device_twins_in_both_layouts(built):
    """the `_dev` twins on a model-shaped Float32 handle: interleaved `vals` bit-equal to problem-major in every output, the two-call
    sequence bit-equal in d to the fused call"""
    hipldl, syn, O = _mods()
    s = syn.model_band_structure(1000, 10)
    B = 100
    vals, rhs = _f32_model_inputs(syn, s, B)
    lad = _f32_model_inputs(syn, syn.model_band_structure(1000, 10), 2, "ladder")
    vals[[5, 40]], rhs[[5, 40]] = lad
    ro_h = np.zeros(B, np.float32)
    cfg_pm, pm = _run_dev(s, vals, rhs, ro_h, np.float32)
    cfg_il, il = _run_dev(s, vals, rhs, ro_h, np.float32, batch_layout=hipldl.LAYOUT_INTERLEAVED)
    assert cfg_pm["float32"] and cfg_pm["band_pieces"] == 20 and cfg_il["band_pieces"] == 20 and cfg_il["batch_layout"] == 1
    assert _bit_equal(pm, il)
    su, d_two, d, ro_o, rho, nf, ok, v_after = pm
    assert ok.all() and (nf[[5, 40]] > 1).all() and int((nf > 1).sum()) == 2
    quiet = nf == 1
    assert su[quiet].all() and np.array_equal(d_two[quiet].view(np.uint32), d[quiet].view(np.uint32))
    F32R._check_newton_against_oracle(O, s, vals, rhs, d, ok, nf, rho, ro_o, v_after)


def test_float32_device_resident_inner_iteration_model_shaped(built):
    """tests/test_float32_rows_gpu.py's inner iteration — prepare -> f1 (`_jac`) -> newton_system_f32_dev -> trial point -> f1 at the
    trial point — on the model-shaped pattern (row f2 fills an H_c segment as long as H_F), problem-major and interleaved: every
    output bit-equal between the two, the Newton outputs held to the oracle"""
    torch, hipldl, syn, O = F32R._mods()
    s = syn.model_band_structure(1000, 10)
    B = 96
    rows, cols = s.kkt_pattern()
    vals64, _ = syn.batch_values(s, B, cfg=4, gen=syn.model_band_values)
    vals32 = vals64.astype(np.float32)
    off = s.offsets()
    m = F32R._model(s, B, 6)
    m.update(hF=vals32[:, off[0]:off[1]], hc=-vals32[:, off[1]:off[2]], Jx=vals32[:, off[2]:off[3]], Jcx=vals32[:, off[3]:off[4]],
             delta=-vals32[:, off[5]])
    m["d"] = None
    scrambled = np.full_like(vals32, 3.0)
    scrambled[:, off[4]:off[5]] = -1.0   # the -I segment: prepare leaves it alone
    t = {k: F32R._dev(torch, np.ascontiguousarray(v)) for k, v in m.items() if v is not None}
    dev = t["x"].device
    p32 = hipldl.default_params(np.float32)
    z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)   # noqa: E731
    runs = []
    for layout in (0, 1):
        L = F32R._handle(hipldl, s, B, batch_layout=layout)
        assert L.config["band_pieces"] == 20 and L.config["batch_layout"] == layout
        vin = F32R._dev(torch, scrambled)
        if layout:
            v = torch.zeros(hipldl.layout_len(L, 0), dtype=torch.float32, device=dev)
            hipldl.interleave_dev(L, 0, vin, v)
        else:
            v = vin
        rhs, nrm, d = z(B, s.N), z(B, 2), z(B, s.N)
        ro, rho = z(B), z(B)
        nf, ok = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        xt, rt, lt, dl = z(B, s.nvar), z(B, s.nequ), z(B, s.ncon), z(B, s.ncon)
        rhs_t, nrm_t = z(B, s.N), z(B, 2)
        hipldl.prepare_newton_system_dev(L, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, t["hF"], t["hc"], t["Jx"], t["Jcx"], t["delta"], v)
        hipldl.residual_vectors_jac_dev(L, s.nnzjF, s.nnzjc, t["Jx"], t["Jcx"], t["r"], t["lam"], t["Fx"], t["cx"], rhs, nrm)
        hipldl.newton_system_dev(L, v, rhs, d, ro, rho, nf, ok, p32)
        hipldl.trial_point_dev(L, t["x"], t["r"], t["lam"], d, 1e4, xt, rt, lt, dl)
        hipldl.residual_vectors_jac_dev(L, s.nnzjF, s.nnzjc, t["Jx"], t["Jcx"], rt, lt, t["Fx"], t["cx"], rhs_t, nrm_t)
        if layout:
            vout = torch.zeros((B, s.nnzNS), dtype=torch.float32, device=dev)
            hipldl.deinterleave_dev(L, 0, v, vout)
        else:
            vout = v
        torch.cuda.synchronize()
        runs.append([x.cpu().numpy() for x in (vout, rhs, nrm, d, ro, rho, nf, ok, xt, rt, lt, dl, rhs_t, nrm_t)])
        L.close()
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    vout, rhs, nrm, d, ro, rho, nf, ok = runs[0][:8]
    want_rhs, want_nrm = R.residual_vectors(rows, cols, vals32, s.nvar, s.nequ, s.ncon, m["r"], m["lam"], m["Fx"], m["cx"])
    assert F32R._same(rhs, want_rhs) and F32R._same(nrm, want_nrm)
    assert ok.all() and (nf == 1).all()
    F32R._check_newton_against_oracle(O, s, vals32, rhs, d, ok, nf, rho, ro, vout)
    assert np.array_equal(vout.view(np.uint32), vals32.view(np.uint32))   # prepare reproduced the generator's values


# ---- the lockstep loop ---------------------------------------------------------------------------------------------------------------

def test_lockstep_loop_of_a_constrained_family_runs_on_the_band_kernels(built):
    """device_loop.solve_batch_device hands over kkt_pattern_of's pattern: where a throughput handle is chosen a constrained family
    gets a band handle and interleaved `vals` with layout = "auto" once the wide program is asked for (tuning band_pieces = 20: Float64
    takes it on request only).  Eight sampled problems against outer_loop.solve with the oracle
    (tolerances of tests/test_gpu_parity.py::test_f3_device_resident_lockstep_outer_loop), and layout = "problem-major" gives the same
    counters for all.
    B: with default options a CONSTRAINED band pattern between 4 097 and 7 680 problems is served by the split plan (bidirectional chain
    + single stream, "v2-staged": csrc/capi_plan.cpp, split_mode) — band_structure(300, 4) with its diagonal H_c just as the model-shaped
    pattern — and the wide form is offered only where the register-front throughput handle runs, so the first batch a band handle serves is
    7 681; only unconstrained families get one from 4 097 on."""
    import torch
    hipldl, syn, O = _mods()
    from cannoles_jl_amd import device_loop as DL, outer_loop
    from tests.test_oracle_pinning import oracle_newton, oracle_solver
    s = syn.band_structure(300, 4)
    B = 7680 + 40
    fam = DL.BandQuadFamily(s, B, seed=304, torch=torch, device="cuda:0", curvature=1.5, start=1.0, noise=0.5)
    prm = hipldl.default_params()
    got = DL.solve_batch_device(fam, prm, tuning={"band_pieces": 20})
    assert got["kernel"] == "band" and got["vals_layout"] == "interleaved"
    for b in np.sort(np.random.default_rng(9).choice(B, 8, replace=False)):
        one = outer_loop.solve(fam.host_model(int(b)), oracle_solver, oracle_newton, prm)
        assert got["status"][b] == one["status"], b
        assert (got["iter"][b], got["nlinsolve"][b], got["nfact"][b], got["nbk"][b]) == (one["iter"], one["nlinsolve"], one["nfact"], one["nbk"]), b
        assert np.allclose(got["solution"][b], one["solution"], atol=1e-7, rtol=1e-7)
        assert np.allclose(got["multipliers"][b], one["multipliers"], atol=1e-6, rtol=1e-6)
        assert abs(got["objective"][b] - one["objective"]) <= 1e-9 * max(1.0, one["objective"])
    pm = DL.solve_batch_device(fam, prm, layout="problem-major", tuning={"band_pieces": 20})
    assert pm["kernel"] == "band" and pm["vals_layout"] == "problem-major"
    assert pm["steps"] == got["steps"] and pm["status"] == got["status"]
    for k in ("iter", "nlinsolve", "nfact", "nbk"):
        assert np.array_equal(pm[k], got[k]), k
