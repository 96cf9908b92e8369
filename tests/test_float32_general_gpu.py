"""Float32 handles on the general multifrontal kernel (cnl_create_f32 with tuning float32_general = 1: the float instantiation of
csrc/kernels.hip) against the fp64 oracle on the widened float32 inputs with ParamCaNNOLeS(Float32) widened.  -m gpu.

`check` means, through hipldl.newton_system_ on such a handle: (success, nfact) identical to the oracle; rho, rho_old and the rho slots
of vals bit-equal to the oracle's rounded to float32; backward error <= 512 eps(Float32) and forward error <= 1e-3 (the project's
Float32 tolerances, tests/test_float32_gpu.py); the oracle's pivots at least 1e-3 max|D| from eig_tol, asserted per problem; the handle
reports float32, no band kernels, kernel "v1"; and the call is exactly one launch of the general kernel family.
"""
import ctypes as C

import numpy as np
import pytest

from tests.support import f32_general as G
from tests.support import f32_rows as R

pytestmark = pytest.mark.gpu

EPS32 = G.EPS32
CNL_ERR_ARG, CNL_ERR_DIM, CNL_ERR_STATE = 1, 2, 5
MULTIPRECISION_ATOL = max(1e-4, EPS32 ** 0.25)   # the reference's own multiprecision tolerance (test/runtests.jl:110)
# the (threads per problem, problems per workgroup, work area in LDS) instances compiled for float (csrc/kernels.hip, CNL_F32_CASES)
F32_INSTANCES = [(64, 1, 1), (64, 4, 1), (32, 2, 1), (16, 4, 1), (256, 1, 1), (64, 4, 0), (256, 1, 0)]


def _mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    from oracle import oracle as O
    return hipldl, syn, O


def _handle(hipldl, s, B, vals=None, **opt):
    rows, cols = s.kkt_pattern()
    L = hipldl.HIPLDLStruct(s.N, rows, cols, vals, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32,
                            options=hipldl.Options(float32_general=1, **opt))
    assert L.dtype == np.float32
    assert L.config["float32"] and not L.config["band"] and L.config["kernel"] == "v1", L.config
    return L


def _general_only(hipldl, c0, n=1):
    c1 = hipldl.launch_counts()
    assert c1["general"] - c0["general"] == n and c1["band"] == c0["band"] and c1["register_front"] == c0["register_front"], (c0, c1)


_refs = {}


def _ref(O, hipldl, key, s, vals, rhs, ro32):
    """one oracle run per named input set, shared by the tests that use it (never modified)"""
    if key not in _refs:
        _refs[key] = G.oracle_newton(O, s, vals, rhs, ro32, hipldl.default_params(np.float32))
    return _refs[key]


def check(key, s, vals, rhs, rho_old=0.0, L=None, **opt):
    hipldl, syn, O = _mods()
    B = vals.shape[0]
    p32 = hipldl.default_params(np.float32)
    ro32 = np.full(B, rho_old, np.float32)
    own = L is None
    if own:
        L = _handle(hipldl, s, B, **opt)
    v = vals.copy()
    c0 = hipldl.launch_counts()
    d, ok, rho, ro, nf = hipldl.newton_system_(np.zeros((B, s.N) if B > 1 else s.N, np.float32), s.nvar, s.nequ, s.ncon,
                                               rhs if B > 1 else rhs[0], v if B > 1 else v[0], L, ro32 if B > 1 else ro32[0], p32)
    _general_only(hipldl, c0)
    if B == 1:   # the drop-in case: scalars, as the reference returns them
        assert isinstance(ok, bool) and isinstance(rho, float) and isinstance(ro, float) and isinstance(nf, int)
    ref = _ref(O, hipldl, (key, float(rho_old)), s, vals, rhs, ro32)
    be, fe = G.check_results(s, ref, v, rhs, d, ok, rho, ro, nf)
    print(f"{key}: backward error {be / EPS32:.1f} eps32, forward error {fe:.2e}, nfact {sorted(set(ref['nf'].tolist()))}, "
          f"tpp {L.config['tpp']} ppb {L.config['ppb']} lds {L.config['lds_work']}")
    out = (np.asarray(d).reshape(B, s.N).copy(), ref, v)
    if own:
        L.close()
    return out


def _random_case():
    hipldl, syn, O = _mods()
    return syn.random_structure(60, 80, 4, 0.1, seed=3)


def _mixed_batch(syn, s):
    """the posdef batch with problem 5 replaced by an indefinite one: a mixed ladder inside one workgroup"""
    vals, rhs = G.random_inputs(syn, s, range(100, 124))
    v5, r5 = G.random_inputs(syn, s, [205], posdef=False)
    vals[5], rhs[5] = v5[0], r5[0]
    return vals, rhs


# ---- 1. irregular pattern ----
def test_irregular_pattern_first_attempt(built):
    hipldl, syn, O = _mods()
    s = _random_case()
    vals, rhs = G.random_inputs(syn, s, range(100, 124))
    _, ref, _ = check("random-posdef", s, vals, rhs)
    assert ref["ok"].all() and (ref["nf"] == 1).all()


@pytest.mark.parametrize("rho_old", [0.0, 0.3])
def test_irregular_pattern_ladder(built, rho_old):
    hipldl, syn, O = _mods()
    s = _random_case()
    vals, rhs = G.random_inputs(syn, s, range(200, 224), posdef=False)
    _, ref, _ = check("random-indefinite", s, vals, rhs, rho_old=rho_old)
    assert ref["ok"].all()
    assert (ref["nf"] == 4).all() if rho_old == 0.0 else set(ref["nf"].tolist()) <= {3, 4}


def test_irregular_pattern_mixed_ladder_in_one_workgroup(built):
    hipldl, syn, O = _mods()
    s = _random_case()
    vals, rhs = _mixed_batch(syn, s)
    _, ref, _ = check("random-mixed", s, vals, rhs, v1_ppb=4)   # problems 4 .. 7 share a workgroup
    assert ref["nf"][5] > 1 and (np.delete(ref["nf"], 5) == 1).all()


def test_irregular_pattern_one_problem(built):
    hipldl, syn, O = _mods()
    s = _random_case()
    vals, rhs = G.random_inputs(syn, s, [100])
    check("random-one", s, vals, rhs)
    vals, rhs = G.random_inputs(syn, s, [200], posdef=False)
    check("random-one-indefinite", s, vals, rhs)


# ---- 2. band half-widths the band program refuses ----
@pytest.mark.parametrize("hw", [3, 4])
def test_band_half_widths_the_band_program_refuses(built, hw):
    hipldl, syn, O = _mods()
    s = syn.band_structure(400, 4, hw=hw)
    rows, cols = s.kkt_pattern()
    with pytest.raises(hipldl.CnlError) as e:   # without the option: refused, as before
        hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=24, dtype=np.float32)
    assert e.value.code == CNL_ERR_ARG and "build_band_plan" in str(e.value)
    L = _handle(hipldl, s, 24)
    vals, rhs = G.band_inputs(syn, s, range(4000, 4024))
    _, ref, _ = check(f"band-hw{hw}", s, vals, rhs, L=L)
    assert (ref["nf"] == 1).all()
    vals, rhs = G.band_inputs(syn, s, range(7000, 7024), stress="ladder")
    _, ref, _ = check(f"band-hw{hw}-ladder", s, vals, rhs, L=L)
    assert ref["ok"].all() and (ref["nf"] == 4).all()
    L.close()


# ---- 3. dense block: one large front ----
def test_dense_block(built):
    hipldl, syn, O = _mods()
    s = syn.dense_structure(40, 70)
    vals, rhs = G.dense_inputs(syn, s, range(100, 110))
    L = _handle(hipldl, s, 10)
    assert (L.config["tpp"], L.config["ppb"], L.config["lds_work"]) == (256, 1, 1)   # front of order 111: a workgroup per problem, LDS
    check("dense-40-70", s, vals, rhs, L=L)
    L.close()


def test_dense_block_beyond_lds_runs_on_global_scratch(built):
    """dense_structure(100, 160): one front of order 261, a work area of 276 kB in float — the global-scratch instance serves it
    (DESIGN section 9); CNL_ERR_DIM is left to work areas of 2^30 elements and to forced configurations that exceed LDS"""
    hipldl, syn, O = _mods()
    s = syn.dense_structure(100, 160)
    vals, rhs = G.dense_inputs(syn, s, range(100, 104))
    L = _handle(hipldl, s, 4)
    assert (L.config["tpp"], L.config["ppb"], L.config["lds_work"]) == (256, 1, 0)
    check("dense-100-160", s, vals, rhs, L=L)
    L.close()
    rows, cols = s.kkt_pattern()
    with pytest.raises(hipldl.CnlError) as e:   # the same work area forced into LDS: refused, the front order named
        hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=4, dtype=np.float32,
                            options=hipldl.Options(float32_general=1, v1_lds=1))
    assert e.value.code == CNL_ERR_DIM and "front of order 261" in str(e.value)


# ---- 4. a band pattern on the general kernel, against the Float32 band handle ----
def test_band_pattern_on_the_general_kernel(built):
    hipldl, syn, O = _mods()
    s = syn.band_structure(400, 4)
    rows, cols = s.kkt_pattern()
    B = 24
    vals, rhs = G.band_inputs(syn, s, range(4000, 4024))
    lv, lr = G.band_inputs(syn, s, [7003], stress="ladder")
    vals[3], rhs[3] = lv[0], lr[0]
    d, ref, v = check("band-on-general", s, vals, rhs, band_kernel=0)
    assert ref["nf"][3] > 1
    p32 = hipldl.default_params(np.float32)
    Lb = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32, options=hipldl.Options(float32_general=1))
    assert Lb.config["band"] and Lb.config["kernel"] == "band"   # the option changes nothing where the band kernels serve the handle
    vb = vals.copy()
    db, okb, rhob, rob, nfb = hipldl.newton_system_(np.zeros((B, s.N), np.float32), s.nvar, s.nequ, s.ncon, rhs, vb, Lb, np.zeros(B, np.float32), p32)
    Lb.close()
    assert np.array_equal(okb, ref["ok"]) and np.array_equal(nfb, ref["nf"])
    assert np.array_equal(G.bits(rhob), G.bits(ref["rho"])) and np.array_equal(G.bits(rob), G.bits(ref["ro"]))
    assert np.array_equal(G.bits(vb[:, -s.nvar:]), G.bits(v[:, -s.nvar:]))
    for b in range(B):   # both are within FWD_TOL of the oracle
        assert np.abs(db[b] - d[b]).max() <= 2 * G.FWD_TOL * np.abs(ref["d"][b]).max(), b


# ---- 5. every compiled instance ----
@pytest.mark.parametrize("tpp,ppb,lds", F32_INSTANCES)
def test_every_compiled_instance(built, tpp, ppb, lds):
    hipldl, syn, O = _mods()
    s = _random_case()
    vals, rhs = _mixed_batch(syn, s)
    B = vals.shape[0]
    L = _handle(hipldl, s, B, v1_tpp=tpp, v1_ppb=ppb, v1_lds=lds)
    cfg = np.zeros(8, np.int64)
    hipldl._check(hipldl.lib().cnl_get_config(L._h, cfg))
    work = (L.info["fwd_peak"] + 1 & ~1 if L.info["fwd_peak"] >= L.info["bwd_peak"] else L.info["bwd_peak"] + 1 & ~1) + (L.info["panel_max"] + 1 & ~1) + \
        2 * (L.info["fmax"] + 1 & ~1)
    assert cfg[:5].tolist() == [tpp, ppb, 4 * (16 + (ppb * work if lds else 0)), lds, (B + ppb - 1) // ppb]
    assert int(cfg[5]) & ~128 == 1 + (1 << 27)   # the general kernel, Float32, bit 6 (band) clear; bit 7: row f1 on column tiles
    check("random-mixed", s, vals, rhs, L=L)
    L.close()


def test_instances_not_compiled_for_float_are_refused(built):
    hipldl, syn, O = _mods()
    s = _random_case()
    rows, cols = s.kkt_pattern()
    for tpp, ppb, lds in [(64, 2, 1), (1024, 1, 1), (1024, 1, 0)]:   # Float64 has them (csrc/kernels.hip, CNL_CASE)
        assert (tpp, ppb, lds) not in F32_INSTANCES
        with pytest.raises(hipldl.CnlError) as e:
            hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=24, dtype=np.float32,
                                options=hipldl.Options(float32_general=1, v1_tpp=tpp, v1_ppb=ppb, v1_lds=lds))
        assert e.value.code == CNL_ERR_ARG and "no Float32 instance" in str(e.value)


# ---- 6. two-call sequence and the kept factor ----
def test_two_call_sequence_and_kept_factor(built):
    import torch
    hipldl, syn, O = _mods()
    s = _random_case()
    rows, cols = s.kkt_pattern()
    vals, rhs = _mixed_batch(syn, s)
    B = vals.shape[0]
    p32 = hipldl.default_params(np.float32)
    L = _handle(hipldl, s, B)
    c0 = hipldl.launch_counts()
    ok, npos, nzer = hipldl.try_to_factorize(L, vals, s.nvar, s.nequ, s.ncon, p32[0], return_inertia=True)
    _general_only(hipldl, c0)
    orc = G.oracle_of(O, s)
    for b in range(B):
        ok0, np0, nz0 = orc.try_to_factorize(vals[b].astype(np.float64), s.nvar, s.nequ, s.ncon, float(p32[0]), return_inertia=True)
        assert (bool(ok[b]), int(npos[b]), int(nzer[b])) == (ok0, np0, nz0), b
    assert not ok[5] and ok.sum() == B - 1
    # two solves with different right-hand sides on the stored factor: one launch each, failed rows untouched
    rhs2 = np.ascontiguousarray(rhs[::-1] * np.float32(0.5))
    d_host = []
    for r in (rhs, rhs2):
        d = np.full((B, s.N), 7.0, np.float32)
        c0 = hipldl.launch_counts()
        assert hipldl.solve_ldl_(r, L.factor, d) is True
        _general_only(hipldl, c0)
        assert np.all(d[5] == 7.0)
        for b in range(B):
            if b == 5:
                continue
            d0 = -np.linalg.solve(syn.dense_kkt(s, vals[b].astype(np.float64)), r[b].astype(np.float64))
            assert G.backward_error(s, vals[b], r[b], d[b]) <= G.BWD_TOL, b
            assert np.abs(d[b] - d0).max() <= G.FWD_TOL * np.abs(d0).max(), b
        d_host.append(d)
    # device pointers: the factor is the handle's own — the caller may overwrite d_vals between factorisation and solve
    dev = torch.device("cuda", 0)
    tv, tr = torch.from_numpy(vals).to(dev), torch.from_numpy(rhs).to(dev)
    su = torch.zeros(B, dtype=torch.int32, device=dev)
    d_keep = torch.zeros((B, s.N), dtype=torch.float32, device=dev)
    d_over = torch.zeros((B, s.N), dtype=torch.float32, device=dev)
    hipldl.factorize_dev(L, tv, p32[0], su)
    hipldl.solve_dev(L, tr, d_keep)
    torch.cuda.synchronize()
    tv2 = tv.clone()
    hipldl.factorize_dev(L, tv2, p32[0], su)
    torch.cuda.synchronize()
    tv2.fill_(float("nan"))
    hipldl.solve_dev(L, tr, d_over)
    torch.cuda.synchronize()
    keep = np.nonzero(ok)[0]
    assert np.array_equal(su.cpu().numpy().astype(bool), ok)
    assert np.array_equal(G.bits(d_over.cpu().numpy()[keep]), G.bits(d_keep.cpu().numpy()[keep]))
    assert np.array_equal(G.bits(d_keep.cpu().numpy()[keep]), G.bits(d_host[0][keep]))   # (host and device calls run the same launch)
    L.close()
    # one problem whose factorisation failed: solve_ldl! is a call-sequence error, refused before anything is uploaded or launched
    L1 = _handle(hipldl, s, 1)
    assert not hipldl.try_to_factorize(L1, vals[5], s.nvar, s.nequ, s.ncon, p32[0])
    d7 = np.full(s.N, 7.0, np.float32)
    c2 = hipldl.launch_counts()
    with pytest.raises(hipldl.CnlError) as ei:
        hipldl.solve_ldl_(rhs[5], L1.factor, d7)
    assert ei.value.code == CNL_ERR_STATE and (d7 == 7.0).all()
    assert hipldl.launch_counts() == c2
    L1.close()


# ---- 7. determinism and prefix ----
def test_determinism_and_active_prefix(built):
    import torch
    hipldl, syn, O = _mods()
    s = _random_case()
    vals, rhs = _mixed_batch(syn, s)
    B = vals.shape[0]
    p32 = hipldl.default_params(np.float32)
    dev = torch.device("cuda", 0)
    L = _handle(hipldl, s, B)

    def run(fill=0.0):
        t = dict(v=torch.from_numpy(vals).to(dev), r=torch.from_numpy(rhs).to(dev), d=torch.full((B, s.N), fill, dtype=torch.float32, device=dev),
                 ro=torch.zeros(B, dtype=torch.float32, device=dev), rho=torch.full((B,), fill, dtype=torch.float32, device=dev),
                 nf=torch.full((B,), int(fill), dtype=torch.int32, device=dev), ok=torch.full((B,), int(fill), dtype=torch.int32, device=dev))
        c0 = hipldl.launch_counts()
        hipldl.newton_system_dev(L, t["v"], t["r"], t["d"], t["ro"], t["rho"], t["nf"], t["ok"], p32)
        torch.cuda.synchronize()
        _general_only(hipldl, c0)
        return {k: x.cpu().numpy() for k, x in t.items()}

    a, b = run(), run()
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert a["nf"][5] > 1 and a["ok"].all()
    hipldl.set_active_batch(L, 5)
    assert hipldl.get_active_batch(L) == 5
    c = run(fill=9.0)
    for k in ("d", "rho", "nf", "ok", "ro"):
        assert np.array_equal(c[k][:5].view(np.uint8), a[k][:5].view(np.uint8)), k
    assert np.array_equal(c["v"][:5].view(np.uint8), a["v"][:5].view(np.uint8))
    assert (c["d"][5:] == 9.0).all() and (c["rho"][5:] == 9.0).all() and (c["nf"][5:] == 9).all() and (c["ok"][5:] == 9).all()
    assert np.array_equal(c["v"][5:].view(np.uint8), vals[5:].view(np.uint8))    # rows 5 .. 23: untouched (problem 5 did not climb)
    with pytest.raises(hipldl.CnlError) as e:   # host-pointer calls take the arrays of the created batch
        hipldl.newton_system_(np.zeros((B, s.N), np.float32), s.nvar, s.nequ, s.ncon, rhs, vals.copy(), L, np.zeros(B, np.float32), p32)
    assert e.value.code == CNL_ERR_STATE
    hipldl.set_active_batch(L, B)
    e2 = run()
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), e2[k].view(np.uint8)), k
    L.close()


# ---- 8. rows f1 / f2 / f4 and the trial point on a non-band Float32 handle ----
def test_rows_on_a_non_band_handle(built):
    import torch
    hipldl, syn, O = _mods()
    s = _random_case()
    rows, cols = s.kkt_pattern()
    B = 7
    rng = np.random.default_rng(8)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)   # noqa: E731
    m = {"hF": f(B, s.nnzhF), "hc": f(B, s.nnzhc), "Jx": f(B, s.nnzjF), "Jcx": f(B, s.nnzjc), "delta": np.abs(f(B)),
         "x": f(B, s.nvar), "r": f(B, s.nequ), "lam": f(B, s.ncon), "Fx": f(B, s.nequ), "cx": f(B, s.ncon), "d": f(B, s.N)}
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in m.items()}
    same = lambda a, b: np.array_equal(G.bits(a), G.bits(b))   # noqa: E731
    old = rng.standard_normal((B, s.nnzNS)).astype(np.float32)
    want_vals = R.prepare(old, s.nvar, s.nequ, s.ncon, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, m["hF"], m["hc"], m["Jx"], m["Jcx"], m["delta"])
    want_rhs, want_nrm = R.residual_vectors(rows, cols, want_vals, s.nvar, s.nequ, s.ncon, m["r"], m["lam"], m["Fx"], m["cx"])
    outs = []
    for tiles in (1, 0):   # (0: the gather form of row f1, in float on an irregular pattern)
        L = _handle(hipldl, s, B, f1_tiles=tiles)
        if not tiles:
            assert not L.config["f1_tiles"]
        tv = torch.from_numpy(old).to(dev)
        hipldl.prepare_newton_system_dev(L, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, t["hF"], t["hc"], t["Jx"], t["Jcx"], t["delta"], tv)
        rhs = torch.full((B, s.N), 9.0, dtype=torch.float32, device=dev)
        nrm = torch.full((B, 2), -1.0, dtype=torch.float32, device=dev)
        hipldl.residual_vectors_dev(L, tv, t["r"], t["lam"], t["Fx"], t["cx"], rhs, nrm)
        rhs2, nrm2 = torch.zeros_like(rhs), torch.zeros_like(nrm)
        hipldl.residual_vectors_jac_dev(L, s.nnzjF, s.nnzjc, t["Jx"], t["Jcx"], t["r"], t["lam"], t["Fx"], t["cx"], rhs2, nrm2)
        torch.cuda.synchronize()
        assert same(tv.cpu().numpy(), want_vals)
        got = [x.cpu().numpy() for x in (rhs, nrm, rhs2, nrm2)]
        assert same(got[0], want_rhs) and same(got[1], want_nrm), tiles
        assert same(got[2], got[0]) and same(got[3], got[1]), tiles
        outs.append(got)
        if tiles:
            L.close()
    assert all(same(a, b) for a, b in zip(outs[0], outs[1]))
    # CGLS (row f4) and its `_jac` twin: the restated recurrence's iteration counts (every stopping test MARGIN away from its threshold)
    lam, jt, it = (torch.zeros((B, s.ncon), dtype=torch.float32, device=dev), torch.zeros((B, s.nvar), dtype=torch.float32, device=dev),
                   torch.zeros(B, dtype=torch.int32, device=dev))
    hipldl.cgls_multipliers_dev(L, tv, t["r"], lam, jt, iters_ptr=it)
    lam2, jt2, it2 = torch.zeros_like(lam), torch.zeros_like(jt), torch.zeros_like(it)
    hipldl.cgls_multipliers_jac_dev(L, s.nnzjF, s.nnzjc, t["Jx"], t["Jcx"], t["r"], lam2, jt2, iters_ptr=it2)
    torch.cuda.synchronize()
    lam, jt, it, lam2, jt2, it2 = (x.cpu().numpy() for x in (lam, jt, it, lam2, jt2, it2))
    assert same(lam, lam2) and same(jt, jt2) and np.array_equal(it, it2)
    off = s.offsets()
    i0, j0 = rows - 1, cols - 1
    for b in range(B):
        lam0, jt0, it0, margin = R.cgls_multipliers(rows, cols, want_vals[b], s.nvar, s.nequ, s.ncon, m["r"][b])
        assert margin > G.MARGIN, f"problem {b}: a stopping test lies within {margin:.3g} of its threshold"
        assert same(jt[b], jt0) and it[b] == it0, (b, it[b], it0)
        A = np.zeros((s.nvar, s.ncon))
        k = np.arange(off[3], off[4])
        A[j0[k], i0[k] - s.nvar - s.nequ] = want_vals[b, k]
        g = jt0.astype(np.float64)
        ls = np.linalg.lstsq(A, g, rcond=None)[0]
        assert np.linalg.norm(A.T @ (A @ lam[b].astype(np.float64) - g)) <= 2e-3 * np.linalg.norm(A.T @ g), b
        assert np.linalg.norm(lam[b] - ls) <= 1e-3 * np.linalg.norm(ls), b
    # trial point
    d = m["d"].copy()
    d[2, s.nvar + s.nequ:] *= 1e4   # over the cap
    want = R.trial_point(s.nvar, s.nequ, s.ncon, m["x"], m["r"], m["lam"], d, 1e4)
    out = [torch.full(a.shape, 5.0, dtype=torch.float32, device=dev) for a in want]
    hipldl.trial_point_dev(L, t["x"], t["r"], t["lam"], torch.from_numpy(d).to(dev), 1e4, *out)
    torch.cuda.synchronize()
    xt, rt, lt, dl = (x.cpu().numpy() for x in out)
    assert same(xt, want[0]) and same(rt, want[1])
    assert np.all(np.abs(dl - want[3]) <= 4 * EPS32 * np.abs(want[3]))
    assert np.all(np.abs(lt - want[2]) <= 4 * EPS32 * (np.abs(m["lam"]) + np.abs(want[3])))
    assert np.array_equal(dl[0], -d[0, s.nvar + s.nequ:])
    L.close()


# ---- 9. errors ----
def test_errors(built):
    hipldl, syn, O = _mods()
    lib = hipldl.lib()
    s = _random_case()
    rows, cols = s.kkt_pattern()
    B = 4
    with pytest.raises(hipldl.CnlError) as e:   # the interleaved layout is the band kernels'
        hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32,
                            options=hipldl.Options(float32_general=1, batch_layout=hipldl.LAYOUT_INTERLEAVED))
    assert e.value.code == CNL_ERR_ARG
    with pytest.raises(hipldl.CnlError) as e:   # without the option: as before
        hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32)
    assert e.value.code == CNL_ERR_ARG and "build_band_plan" in str(e.value)
    L = _handle(hipldl, s, B)
    p64 = hipldl.default_params()
    buf = np.full((B, max(s.nnzNS, s.N) * 2), 3.0, np.float64)
    ib = np.full(4 * B, 3, np.int64)
    a, i = buf.ctypes.data, ib.ctypes.data
    c0 = hipldl.launch_counts()
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
        assert call(L._h) == CNL_ERR_STATE, lib.cnl_last_error()
    assert hipldl.launch_counts() == c0
    assert (buf == 3.0).all() and (ib == 3).all()
    L.close()


def test_layout_conversions_still_work(built):
    """cnl_interleave_f32_dev / cnl_deinterleave_f32_dev are pure layout conversions: served on any Float32 handle"""
    import torch
    hipldl, syn, O = _mods()
    s = _random_case()
    B = 5
    L = _handle(hipldl, s, B)
    dev = torch.device("cuda", 0)
    v = torch.from_numpy(np.random.default_rng(1).standard_normal((B, s.nnzNS)).astype(np.float32)).to(dev)
    iv = torch.full((hipldl.layout_len(L, 0),), 5.0, dtype=torch.float32, device=dev)
    back = torch.zeros_like(v)
    hipldl.interleave_dev(L, 0, v, iv)
    hipldl.deinterleave_dev(L, 0, iv, back)
    torch.cuda.synchronize()
    assert torch.equal(back, v)
    idx = hipldl.il_index(np.arange(B)[:, None], np.arange(s.nnzNS)[None, :], s.nnzNS)
    assert np.array_equal(iv.cpu().numpy()[idx], v.cpu().numpy())
    L.close()


# ---- 10. the lockstep loop in Float32 off the band kernels ----
def test_lockstep_loop_off_the_band_kernels(built):
    import torch
    hipldl, syn, O = _mods()
    from cannoles_jl_amd import device_loop as DL, outer_loop
    from tests.test_oracle_pinning import oracle_newton, oracle_solver
    B = 12
    fam = DL.BandQuadFamily(syn.band_structure(300, 4, hw=3), B, seed=304, torch=torch, device="cuda:0", dtype=np.float32)
    got = DL.solve_batch_device(fam, tuning={"float32_general": 1})
    assert got["dtype"] == "float32" and got["kernel"] == "v1" and got["vals_layout"] == "problem-major"
    assert got["status"] == ["first_order"] * B
    prm = hipldl.default_params()
    dx = dl = 0.0
    for b in range(B):
        one = outer_loop.solve(fam.host_model(b), oracle_solver, oracle_newton, prm)
        assert one["status"] == "first_order"
        dx = max(dx, float(np.abs(got["solution"][b].astype(np.float64) - one["solution"]).max()))
        dl = max(dl, float(np.abs(got["multipliers"][b].astype(np.float64) - one["multipliers"]).max()))
    print(f"float32 lockstep loop on the general kernel: max|dx| = {dx:.3e}, max|dlambda| = {dl:.3e}, steps = {got['steps']}, iter = {got['iter'].tolist()}")
    assert dx <= MULTIPRECISION_ATOL and dl <= MULTIPRECISION_ATOL
    # (compact_min_finished = 1: the default threshold, max(32, working batch // 8), is never reached by twelve problems)
    cp = DL.solve_batch_device(fam, tuning={"float32_general": 1}, compact=True, compact_min_finished=1)
    print(f"  compact: handle_shrunk = {cp['handle_shrunk']}, compactions = {cp.get('compactions')}")
    assert cp["kernel"] == "v1" and cp["status"] == got["status"] and cp["handle_shrunk"] is True
    for k in ("iter", "nlinsolve", "nfact", "nbk"):
        assert np.array_equal(cp[k], got[k]), k
    assert np.array_equal(G.bits(cp["solution"]), G.bits(got["solution"]))
    assert np.array_equal(G.bits(cp["multipliers"]), G.bits(got["multipliers"]))
