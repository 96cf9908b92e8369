"""Float32 Newton systems on the band kernels (cnl_create_f32 and the `_f32` entry points) against the fp64 oracle.  -m gpu.

Reference: the oracle (oracle/, LDLFactStruct restated) run on the Float32 inputs widened to double with ParamCaNNOLeS(Float32)
widened to double.  Then:
  * (success, npos, nzero, nfact) identical;
  * rho and rho_old bit-equal to the oracle's rounded to float32 (the rungs are rho0 * 2^k or one rounded kdec * rho_old product);
  * backward error (fp64, on the float32 values) <= 512 eps(Float32); forward error <= 1e-3.
Decision parity needs the oracle's pivots far from eig_tol: every case asserts that margin, so a change of seed cannot pass silently.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
BWD_TOL = 512 * EPS32
FWD_TOL = 1e-3
MARGIN = 1e-3


def _mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    from oracle import oracle as O
    return hipldl, syn, O


def backward_error(s, vals, rhs, d):
    import scipy.sparse as sp
    rows, cols = s.kkt_pattern()
    Kl = sp.coo_matrix((np.asarray(vals, np.float64), (rows - 1, cols - 1)), shape=(s.N, s.N)).tocsr()
    K = Kl + sp.tril(Kl, -1).T
    d, rhs = np.asarray(d, np.float64), np.asarray(rhs, np.float64)
    res = K @ d + rhs
    return np.abs(res).max() / (abs(K).sum(axis=1).max() * np.abs(d).max() + np.abs(rhs).max())


def f32_inputs(syn, s, B, cfg=4, stress=None):
    """generator values rounded to float32"""
    if stress is None:
        vals, rhs = syn.batch_values(s, B, cfg=cfg)
    else:
        vr = [syn.band_values(s, 7000 + b, stress=stress) for b in range(B)]
        vals, rhs = np.stack([v for v, _ in vr]), np.stack([r for _, r in vr])
    return np.ascontiguousarray(vals, np.float32), np.ascontiguousarray(rhs, np.float32)


def oracle_newton(O, s, vals32, rhs32, rho_old32, p32):
    """the fp64 oracle on the widened Float32 data, with the pivot margin of every problem's last factorisation"""
    rows, cols = s.kkt_pattern()
    orc = O.Oracle(s.N, rows, cols, O.canonical_perm(s.nvar, s.nequ, s.ncon))
    p64 = p32.astype(np.float64)
    B = vals32.shape[0]
    out = {"d": np.zeros((B, s.N)), "ok": np.zeros(B, bool), "rho": np.zeros(B), "ro": np.zeros(B), "nf": np.zeros(B, np.int64),
           "vals": vals32.astype(np.float64)}
    for b in range(B):
        d, ok, rho, ro, nf = O.newton_system(orc, s.nvar, s.nequ, s.ncon, rhs32[b].astype(np.float64), out["vals"][b], float(rho_old32[b]), p64)
        D = orc.D
        margin = np.abs(np.abs(D) - p64[0]).min()
        assert margin >= MARGIN * np.abs(D).max(), f"problem {b}: an oracle pivot lies within {margin:.3g} of eig_tol"
        out["d"][b], out["ok"][b], out["rho"][b], out["ro"][b], out["nf"][b] = d, ok, rho, ro, nf
    return out


def check_against_oracle(hipldl, syn, O, s, vals32, rhs32, rho_old=0.0, options=None, expect_nl=None, bwd_rows=None):
    rows, cols = s.kkt_pattern()
    B = vals32.shape[0]
    p32 = hipldl.default_params(np.float32)
    ro32 = np.broadcast_to(np.asarray(rho_old, np.float32), (B,)).copy()
    L = hipldl.HIPLDLStruct(s.N, rows, cols, vals32.copy(), s.nvar, s.nequ, s.ncon, batch=B, options=options)
    assert L.dtype == np.float32 and L.config["float32"] and L.config["band"]
    if expect_nl is not None:
        assert L.config["band_nl"] == expect_nl
    v = vals32.copy()
    d = np.zeros((B, s.N), np.float32)
    d, ok, rho, ro, nf = hipldl.newton_system_(d, s.nvar, s.nequ, s.ncon, rhs32, v, L, ro32, p32)
    if B == 1:
        ok, rho, ro, nf = np.array([ok]), np.array([rho], np.float32), np.array([ro], np.float32), np.array([nf])
    d = np.asarray(d).reshape(B, s.N)
    ref = oracle_newton(O, s, vals32, rhs32, ro32, p32)
    assert np.array_equal(np.asarray(ok, bool), ref["ok"])
    assert np.array_equal(np.asarray(nf, np.int64), ref["nf"])
    assert np.asarray(rho).dtype == np.float32 and np.asarray(ro).dtype == np.float32
    assert np.array_equal(np.asarray(rho).view(np.uint32), ref["rho"].astype(np.float32).view(np.uint32))
    assert np.array_equal(np.asarray(ro).view(np.uint32), ref["ro"].astype(np.float32).view(np.uint32))
    # the rho slots: written where the ladder climbed, as the reference writes them (src/CaNNOLeS.jl:1031,1038)
    assert np.array_equal(v[:, -s.nvar:].view(np.uint32), ref["vals"][:, -s.nvar:].astype(np.float32).view(np.uint32))
    for b in (range(B) if bwd_rows is None else bwd_rows):
        if ref["ok"][b]:
            assert backward_error(s, v[b], rhs32[b], d[b]) <= BWD_TOL, b
            assert np.abs(d[b] - ref["d"][b]).max() <= FWD_TOL * np.abs(ref["d"][b]).max(), b
    L.close()
    return ok, nf


def test_cfg4_batch(built):
    hipldl, syn, O = _mods()
    s = syn.band_structure(1000, 10)
    vals, rhs = f32_inputs(syn, s, 256)
    ok, nf = check_against_oracle(hipldl, syn, O, s, vals, rhs, bwd_rows=range(0, 256, 5))
    assert ok.all() and (nf == 1).all()


@pytest.mark.parametrize("rho_old", [0.0, 0.3])
def test_ladder_climbs_the_float32_rungs(built, rho_old):
    """cfg5's ladder on Float32 data: kappa_largeinc = 64 (sizeof(Float32) * 16) from rho0, or the kdec rung from rho_old > 0"""
    hipldl, syn, O = _mods()
    s = syn.band_structure(400, 4)
    vals, rhs = f32_inputs(syn, s, 24, stress="ladder")
    ok, nf = check_against_oracle(hipldl, syn, O, s, vals, rhs, rho_old=rho_old)
    assert ok.all() and (nf > 1).all()


@pytest.mark.parametrize("B", [64, 100])
def test_headline_pattern(built, B):
    """band_structure(10000, 50); B = 100: the last workgroup is partial"""
    hipldl, syn, O = _mods()
    s = syn.band_structure(10000, 50)
    vals, rhs = f32_inputs(syn, s, B, cfg=3)
    check_against_oracle(hipldl, syn, O, s, vals, rhs, bwd_rows=[0, 1, 15, 16, 63, B - 1])


def test_one_problem(built):
    """B = 1, the drop-in case: scalars come back as the reference returns them"""
    hipldl, syn, O = _mods()
    s = syn.band_structure(1000, 10)
    vals, rhs = f32_inputs(syn, s, 1)
    check_against_oracle(hipldl, syn, O, s, vals, rhs)


@pytest.mark.parametrize("opt,nl", [({"band_problems_per_group": 8}, 8), ({"band_problems_per_group": 16}, 16),
                                    ({"band_problems_per_group": 32}, 32), ({"band_kernel": 2}, 16)])
def test_every_instantiation(built, opt, nl):
    hipldl, syn, O = _mods()
    s = syn.band_structure(1000, 10)
    vals, rhs = f32_inputs(syn, s, 70)
    vals[5], rhs[5] = f32_inputs(syn, s, 1, stress="ladder")[0][0], f32_inputs(syn, s, 1, stress="ladder")[1][0]
    check_against_oracle(hipldl, syn, O, s, vals, rhs, options=hipldl.Options(**opt), expect_nl=nl, bwd_rows=[0, 5, 31, 32, 69])


def test_two_call_sequence(built):
    """try_to_factorize -> solve_ldl! on a Float32 handle: inertia as the oracle's, d bit-equal to the fused call's where that
    succeeded at rho = 0, band launches only"""
    hipldl, syn, O = _mods()
    s = syn.band_structure(800, 8)
    B = 20
    vals, rhs = f32_inputs(syn, s, B)
    lv, lr = f32_inputs(syn, s, 1, stress="ladder")
    vals[3], rhs[3] = lv[0], lr[0]
    rows, cols = s.kkt_pattern()
    p32 = hipldl.default_params(np.float32)
    L = hipldl.HIPLDLStruct(s.N, rows, cols, vals.copy(), s.nvar, s.nequ, s.ncon, batch=B)
    c0 = hipldl.launch_counts()
    ok, npos, nzer = hipldl.try_to_factorize(L, vals, s.nvar, s.nequ, s.ncon, p32[0], return_inertia=True)
    orc = O.Oracle(s.N, rows, cols, O.canonical_perm(s.nvar, s.nequ, s.ncon))
    for b in range(B):
        ok0, np0, nz0 = orc.try_to_factorize(vals[b].astype(np.float64), s.nvar, s.nequ, s.ncon, float(p32[0]), return_inertia=True)
        assert (bool(ok[b]), int(npos[b]), int(nzer[b])) == (ok0, np0, nz0), b
    assert not ok[3] and ok.sum() == B - 1
    d1 = np.full((B, s.N), 7.0, np.float32)
    assert hipldl.solve_ldl_(rhs, L.factor, d1) is True
    assert np.all(d1[3] == 7.0)
    v = vals.copy()
    d = np.zeros((B, s.N), np.float32)
    d, ok2, rho, ro, nf = hipldl.newton_system_(d, s.nvar, s.nequ, s.ncon, rhs, v, L, np.zeros(B, np.float32), p32)
    assert ok2.all() and nf[3] > 1
    keep = np.nonzero(nf == 1)[0]
    assert len(keep) == B - 1
    assert np.array_equal(d1[keep].view(np.uint32), np.asarray(d).reshape(B, s.N)[keep].view(np.uint32))
    c1 = hipldl.launch_counts()
    assert c1["band"] - c0["band"] == 3 and c1["register_front"] == c0["register_front"] and c1["general"] == c0["general"]
    L.close()
    # one problem whose factorisation failed: solve_ldl! is a call-sequence error (CNL_ERR_STATE), refused before anything is uploaded
    # or launched, and d stays as passed (the Float32 twin of test_gpu_parity.test_solve_after_a_failed_factorisation)
    L1 = hipldl.HIPLDLStruct(s.N, rows, cols, lv[0].copy(), s.nvar, s.nequ, s.ncon, batch=1)
    assert L1.config["float32"]
    assert not hipldl.try_to_factorize(L1, lv[0], s.nvar, s.nequ, s.ncon, p32[0])
    d7 = np.full(s.N, 7.0, np.float32)
    c2 = hipldl.launch_counts()
    with pytest.raises(hipldl.CnlError) as ei:
        hipldl.solve_ldl_(lr[0], L1.factor, d7)
    assert ei.value.code == 5 and (d7 == 7.0).all()
    assert hipldl.launch_counts() == c2
    L1.close()


@pytest.mark.parametrize("layout", [0, 1])
def test_device_twins_in_both_layouts(built, layout):
    """the `_dev` twins with torch float32 tensors: every output bit-equal to the host-pointer call; interleave -> deinterleave is
    the identity"""
    import torch
    hipldl, syn, O = _mods()
    s = syn.band_structure(1000, 10)
    B = 45
    vals, rhs = f32_inputs(syn, s, B)
    lv, lr = f32_inputs(syn, s, 2, stress="ladder")
    vals[[4, 40]], rhs[[4, 40]] = lv, lr
    rows, cols = s.kkt_pattern()
    p32 = hipldl.default_params(np.float32)
    host = hipldl.HIPLDLStruct(s.N, rows, cols, vals.copy(), s.nvar, s.nequ, s.ncon, batch=B)
    vh = vals.copy()
    dh, okh, rhoh, roh, nfh = hipldl.newton_system_(np.zeros((B, s.N), np.float32), s.nvar, s.nequ, s.ncon, rhs, vh, host,
                                                    np.zeros(B, np.float32), p32)
    assert nfh[4] > 1 and nfh[40] > 1
    host.close()
    opts = hipldl.Options(batch_layout=layout, band_rhs_interleaved=1) if layout else None
    L = hipldl.HIPLDLStruct(s.N, rows, cols, vals.copy(), s.nvar, s.nequ, s.ncon, batch=B, options=opts)
    assert L.config["batch_layout"] == layout
    dev = torch.device("cuda", 0)
    tv, tr = torch.from_numpy(vals).to(dev), torch.from_numpy(rhs).to(dev)
    if layout:
        iv = torch.full((hipldl.layout_len(L, 0),), 5.0, dtype=torch.float32, device=dev)
        ir = torch.full((hipldl.layout_len(L, 1),), 5.0, dtype=torch.float32, device=dev)
        hipldl.interleave_dev(L, 0, tv, iv)
        hipldl.interleave_dev(L, 1, tr, ir)
        back = torch.zeros_like(tv)
        hipldl.deinterleave_dev(L, 0, iv, back)
        torch.cuda.synchronize()
        assert torch.equal(back, tv)
        idx = hipldl.il_index(np.arange(B)[:, None], np.arange(s.nnzNS)[None, :], s.nnzNS)
        assert np.array_equal(iv.cpu().numpy()[idx], vals)
        tv_run, tr_run = iv, ir
    else:
        tv_run, tr_run = tv, tr
    td = torch.zeros((B, s.N), dtype=torch.float32, device=dev)
    ro, rho = torch.zeros(B, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.float32, device=dev)
    nf, ok = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    hipldl.newton_system_dev(L, tv_run, tr_run, td, ro, rho, nf, ok, p32)
    torch.cuda.synchronize()
    assert np.array_equal(ok.cpu().numpy().astype(bool), okh)
    assert np.array_equal(nf.cpu().numpy(), nfh)
    for got, want in ((td, np.asarray(dh).reshape(B, s.N)), (rho, rhoh), (ro, roh)):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), np.asarray(want, np.float32).view(np.uint32))
    if layout:
        vout = torch.zeros_like(tv)
        hipldl.deinterleave_dev(L, 0, tv_run, vout)
        torch.cuda.synchronize()
    else:
        vout = tv_run
    assert np.array_equal(vout.cpu().numpy().view(np.uint32), vh.view(np.uint32))   # rho slots as the host call left them
    # the two-call sequence on device pointers: d bit-equal to the fused call's where nothing climbed
    su = torch.zeros(B, dtype=torch.int32, device=dev)
    td2 = torch.full((B, s.N), 7.0, dtype=torch.float32, device=dev)
    tv2 = tv if not layout else torch.zeros_like(iv)
    if layout:
        hipldl.interleave_dev(L, 0, tv, tv2)
    hipldl.factorize_dev(L, tv2, p32[0], su)
    hipldl.solve_dev(L, tr_run, td2)
    torch.cuda.synchronize()
    keep = np.nonzero(nfh == 1)[0]
    assert np.array_equal(su.cpu().numpy()[keep], np.ones(len(keep), np.int32))
    assert np.array_equal(td2.cpu().numpy()[keep].view(np.uint32), np.asarray(dh).reshape(B, s.N)[keep].view(np.uint32))
    L.close()


def test_errors_and_mixed_types(built):
    hipldl, syn, O = _mods()
    lib = hipldl.lib()
    # a pattern the band kernels do not serve: no Float32 handle (the caller stays on the CPU)
    r = syn.random_structure(60, 80, 4, 0.1, seed=3)
    rr, rc = r.kkt_pattern()
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.HIPLDLStruct(r.N, rr, rc, None, r.nvar, r.nequ, r.ncon, batch=4, dtype=np.float32)
    assert e.value.code == 1 and "build_band_plan" in str(e.value)
    s = syn.band_structure(400, 4)
    rows, cols = s.kkt_pattern()
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=4, dtype=np.float32, options=hipldl.Options(band_kernel=0))
    assert e.value.code == 1
    B = 4
    v32, r32 = f32_inputs(syn, s, B)
    L32 = hipldl.HIPLDLStruct(s.N, rows, cols, v32.copy(), s.nvar, s.nequ, s.ncon, batch=B)
    L64 = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B)
    p32, p64 = hipldl.default_params(np.float32), hipldl.default_params()
    v64, r64 = v32.astype(np.float64), r32.astype(np.float64)
    c0 = hipldl.launch_counts()
    # Python surface: arrays of the other type are a TypeError, either way round
    with pytest.raises(TypeError):
        hipldl.try_to_factorize(L32, v64, s.nvar, s.nequ, s.ncon, p32[0])
    with pytest.raises(TypeError):
        hipldl.try_to_factorize(L64, v32, s.nvar, s.nequ, s.ncon, p64[0])
    with pytest.raises(TypeError):
        hipldl.newton_system_(np.zeros((B, s.N)), s.nvar, s.nequ, s.ncon, r64, v64.copy(), L32, 0.0, p64)
    with pytest.raises(TypeError):
        hipldl.newton_system_(np.zeros((B, s.N), np.float32), s.nvar, s.nequ, s.ncon, r32, v32.copy(), L64, 0.0, p32)
    # C ABI: every Float64 entry point refuses a Float32 handle and every `_f32` one a Float64 handle (CNL_ERR_STATE), launching nothing
    buf = np.zeros((B, max(s.nnzNS, s.N) * 2), np.float64)
    ib = np.zeros(4 * B, np.int64)
    a, i = buf.ctypes.data, ib.ctypes.data
    STATE = 5
    f64_calls = [
        lambda h: lib.cnl_factorize(h, a, 1e-8, i, None, None),
        lambda h: lib.cnl_solve(h, a, a),
        lambda h: lib.cnl_newton_system(h, a, a, a, a, p64.ctypes.data, a, a, i, i),
        lambda h: lib.cnl_factorize_dev(h, a, 1e-8, i, None),
        lambda h: lib.cnl_solve_dev(h, a, a, None),
        lambda h: lib.cnl_newton_system_dev(h, a, a, a, a, a, i, i, p64.ctypes.data, None),
        lambda h: lib.cnl_residual_vectors_dev(h, a, a, a, a, a, a, a, None),
        lambda h: lib.cnl_residual_vectors_jac_dev(h, 1, 1, a, a, a, a, a, a, a, a, None),
        lambda h: lib.cnl_cgls_multipliers_dev(h, a, a, a, None, 1e-8, 1e-8, 0, 1, None, None),
        lambda h: lib.cnl_cgls_multipliers_jac_dev(h, 1, 1, a, a, a, a, None, 1e-8, 1e-8, 0, 1, None, None),
        lambda h: lib.cnl_trial_point_dev(h, a, a, a, a, 1e4, a, a, a, a, None),
        lambda h: lib.cnl_prepare_newton_system_dev(h, 0, 0, 0, 0, None, None, a, a, a, a, None),
        lambda h: lib.cnl_interleave_dev(h, 0, a, a + 8, None),
        lambda h: lib.cnl_deinterleave_dev(h, 0, a, a + 8, None),
    ]
    for call in f64_calls:
        assert call(L32._h) == STATE, lib.cnl_last_error()
    f32_calls = [
        lambda h: lib.cnl_factorize_f32(h, a, 1e-4, i, None, None),
        lambda h: lib.cnl_solve_f32(h, a, a),
        lambda h: lib.cnl_newton_system_f32(h, a, a, a, a, p32.ctypes.data, a, a, i, i),
        lambda h: lib.cnl_factorize_f32_dev(h, a, 1e-4, i, None),
        lambda h: lib.cnl_solve_f32_dev(h, a, a, None),
        lambda h: lib.cnl_newton_system_f32_dev(h, a, a, a, a, a, i, i, p32.ctypes.data, None),
        lambda h: lib.cnl_interleave_f32_dev(h, 0, a, a + 8, None),
        lambda h: lib.cnl_deinterleave_f32_dev(h, 0, a, a + 8, None),
    ]
    for call in f32_calls:
        assert call(L64._h) == STATE, lib.cnl_last_error()
    assert hipldl.launch_counts() == c0
    assert hipldl.layout_len(L32, 0) == hipldl.il_len(B, L32.nnz) and hipldl.layout_len(L32, 1) == hipldl.il_len(B, s.N)   # (elements)
    L32.close()
    L64.close()


def test_float64_handle_beside_a_float32_one(built):
    """a Float64 handle created beside a Float32 one of the same pattern computes what a Float64 handle made alone computes"""
    hipldl, syn, O = _mods()
    s = syn.band_structure(1000, 10)
    B = 40
    vals, rhs = syn.batch_values(s, B, cfg=4)
    vals[7], rhs[7] = syn.band_values(s, 77, stress="ladder")
    rows, cols = s.kkt_pattern()
    p = hipldl.default_params()

    def run(L):
        v = vals.copy()
        d, ok, rho, ro, nf = hipldl.newton_system_(np.zeros((B, s.N)), s.nvar, s.nequ, s.ncon, rhs, v, L, np.zeros(B), p)
        return [np.asarray(x).copy() for x in (d, ok, rho, ro, nf, v)]

    alone = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B)
    r_alone = run(alone)
    alone.close()
    f32 = hipldl.HIPLDLStruct(s.N, rows, cols, vals.astype(np.float32), s.nvar, s.nequ, s.ncon, batch=B)
    beside = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B)
    assert not beside.config["float32"] and f32.config["float32"]
    hipldl.newton_system_(np.zeros((B, s.N), np.float32), s.nvar, s.nequ, s.ncon, rhs.astype(np.float32), vals.astype(np.float32), f32,
                          np.zeros(B, np.float32), hipldl.default_params(np.float32))
    r_beside = run(beside)
    for x, y in zip(r_alone, r_beside):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    beside.close()
    f32.close()
