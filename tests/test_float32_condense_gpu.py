"""Float32 general handles on the condensed system (cnl_create_f32 with tuning float32_general = 1 and float32_condense = 1: the float
instantiations of the condensation passes of csrc/kernels_aux.hip around the float general kernel) against the fp64 oracle on the
widened float32 inputs with ParamCaNNOLeS(Float32) widened.  -m gpu.

`check` means, through hipldl.newton_system_ on such a handle: (success, nfact) identical to the oracle; rho, rho_old and the rho slots
of vals bit-equal to the oracle's rounded to float32; backward error <= 512 eps(Float32) and forward error <= 1e-3
(tests/support/f32_general.py: oracle_newton / check_results, unchanged); the handle reports float32, no band kernels, kernel "v1"
and info["ncond"] > 0; and the call is exactly one launch of the general kernel family and none of the other two.  The inputs' pivot
margins are asserted without a GPU in tests/test_float32_condense_cpu.py.
"""
import numpy as np
import pytest

from tests.support import f32_general as G
from tests.test_float32_general_gpu import MULTIPRECISION_ATOL

pytestmark = pytest.mark.gpu

EPS32 = G.EPS32
CNL_ERR_ARG, CNL_ERR_STATE = 1, 5


def _mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    from oracle import oracle as O
    return hipldl, syn, O


def _handle(hipldl, s, B, condense=1, **opt):
    rows, cols = s.kkt_pattern()
    L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32,
                            options=hipldl.Options(float32_general=1, float32_condense=condense, **opt))
    assert L.dtype == np.float32
    assert L.config["float32"] and not L.config["band"] and L.config["kernel"] == "v1", L.config
    assert (L.info["ncond"] > 0) == bool(condense), L.info
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


def _newton(hipldl, s, L, vals, rhs, ro32, fill=0.0):
    B = vals.shape[0]
    p32 = hipldl.default_params(np.float32)
    v = vals.copy()
    c0 = hipldl.launch_counts()
    d, ok, rho, ro, nf = hipldl.newton_system_(np.full((B, s.N) if B > 1 else s.N, fill, np.float32), s.nvar, s.nequ, s.ncon,
                                               rhs if B > 1 else rhs[0], v if B > 1 else v[0], L, ro32 if B > 1 else ro32[0], p32)
    _general_only(hipldl, c0)
    return v, d, ok, rho, ro, nf


def check(key, s, vals, rhs, rho_old=0.0, L=None, **opt):
    hipldl, syn, O = _mods()
    B = vals.shape[0]
    ro32 = np.full(B, rho_old, np.float32)
    own = L is None
    if own:
        L = _handle(hipldl, s, B, **opt)
    v, d, ok, rho, ro, nf = _newton(hipldl, s, L, vals, rhs, ro32)
    if B == 1:   # the drop-in case: scalars, as the reference returns them
        assert isinstance(ok, bool) and isinstance(rho, float) and isinstance(ro, float) and isinstance(nf, int)
    ref = _ref(O, hipldl, (key, float(rho_old)), s, vals, rhs, ro32)
    be, fe = G.check_results(s, ref, v, rhs, d, ok, rho, ro, nf)
    print(f"{key}: backward error {be / EPS32:.1f} eps32, forward error {fe:.2e}, nfact {sorted(set(ref['nf'].tolist()))}, "
          f"tpp {L.config['tpp']} ppb {L.config['ppb']} lds {L.config['lds_work']}, tiled condense {int(L.plan_array('cond_info')[0])}")
    out = (np.asarray(d).reshape(B, s.N).copy(), ref, v, (np.asarray(ok).reshape(B), np.asarray(nf).reshape(B), np.asarray(rho).reshape(B)))
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


# ---- 1. dense block, largest front 41 ----
def test_dense_block(built):
    hipldl, syn, O = _mods()
    s = syn.dense_structure(40, 70)
    vals, rhs = G.dense_inputs(syn, s, range(100, 110))
    L = _handle(hipldl, s, 10)
    assert L.info["fmax"] == 41 and L.info["ncond"] == 70
    # a dense Jacobian: the resident condense kernel (the tiled kernel's chunks would each stage the whole Jacobian); the post-pass
    # takes its row-per-thread loop (2 800 entries)
    assert L.config["cond_resident"] and L.plan_array("cond_info")[0] == 1
    check("dense-40-70", s, vals, rhs, L=L)
    L.close()


# ---- 2. the order-261 front becomes an order-101 front in LDS ----
def test_dense_block_moves_into_lds(built):
    hipldl, syn, O = _mods()
    s = syn.dense_structure(100, 160)
    vals, rhs = G.dense_inputs(syn, s, range(100, 104))
    L = _handle(hipldl, s, 4)
    assert L.config["lds_work"] == 1 and L.info["fmax"] == 101, (L.config, L.info)
    assert L.config["cond_resident"] and L.plan_array("cond_info")[0] == 0   # (no tiled kernel: a dense J'J chunk exceeds its LDS)
    check("dense-100-160", s, vals, rhs, L=L)
    L.close()
    Lu = _handle(hipldl, s, 4, condense=0)     # uncondensed: global scratch
    assert (Lu.config["tpp"], Lu.config["ppb"], Lu.config["lds_work"]) == (256, 1, 0)
    Lu.close()


# ---- 3. irregular pattern ----
def test_irregular_pattern_first_attempt(built):
    hipldl, syn, O = _mods()
    s = _random_case()
    vals, rhs = G.random_inputs(syn, s, range(100, 124))
    _, ref, _, _ = check("random-posdef", s, vals, rhs)
    assert ref["ok"].all() and (ref["nf"] == 1).all()


@pytest.mark.parametrize("rho_old", [0.0, 0.3])
def test_irregular_pattern_ladder(built, rho_old):
    hipldl, syn, O = _mods()
    s = _random_case()
    vals, rhs = G.random_inputs(syn, s, range(200, 224), posdef=False)
    _, ref, _, _ = check("random-indefinite", s, vals, rhs, rho_old=rho_old)
    assert ref["ok"].all() and (ref["nf"] > 1).all()


def test_irregular_pattern_mixed_ladder_in_one_workgroup(built):
    hipldl, syn, O = _mods()
    s = _random_case()
    vals, rhs = _mixed_batch(syn, s)
    L = _handle(hipldl, s, 24, v1_ppb=4)   # problems 4 .. 7 share a workgroup
    assert L.config["ppb"] == 4 and not L.config["cond_resident"]
    _, ref, _, _ = check("random-mixed", s, vals, rhs, L=L)
    L.close()
    assert ref["nf"][5] > 1 and (np.delete(ref["nf"], 5) == 1).all()


def test_irregular_pattern_one_problem(built):
    hipldl, syn, O = _mods()
    s = _random_case()
    vals, rhs = G.random_inputs(syn, s, [100])
    check("random-one", s, vals, rhs)
    vals, rhs = G.random_inputs(syn, s, [200], posdef=False)
    check("random-one-indefinite", s, vals, rhs)


# ---- 4. band half-widths the band program refuses ----
@pytest.mark.parametrize("hw", [3, 4])
def test_band_half_widths(built, hw):
    hipldl, syn, O = _mods()
    s = syn.band_structure(400, 4, hw=hw)
    L = _handle(hipldl, s, 24)
    assert not L.config["cond_resident"] and L.plan_array("cond_info")[0] == 1   # sparse Jacobian: the tiled kernel
    vals, rhs = G.band_inputs(syn, s, range(4000, 4024))
    _, ref, _, _ = check(f"band-hw{hw}", s, vals, rhs, L=L)
    assert (ref["nf"] == 1).all()
    vals, rhs = G.band_inputs(syn, s, range(7000, 7024), stress="ladder")
    _, ref, _, _ = check(f"band-hw{hw}-ladder", s, vals, rhs, L=L)
    assert ref["ok"].all() and (ref["nf"] == 4).all()
    L.close()


# ---- 5. a hopeless problem in a batch ----
def test_hopeless_problem_in_a_batch(built):
    """Problem 2 gets an H entry of -1e20: no rho up to rhomax (2^46) rescues it, so it climbs the whole ladder and fails; its d is
    untouched and its rho slots hold the last rho tried, as the oracle leaves them.  The oracle's margin assertion measures pivots
    against max|D| = 1e20 and so cannot hold for this one problem; it is run through the same oracle call without that assertion, and
    its decision does not hang on a margin: the pivot of that entry stays below -1e19 on every rung."""
    hipldl, syn, O = _mods()
    s = _random_case()
    vals, rhs = G.random_inputs(syn, s, range(100, 108))
    B, bad = vals.shape[0], 2
    vals[bad, s.offsets()[0]] = np.float32(-1e20)
    p32 = hipldl.default_params(np.float32)
    keep = [b for b in range(B) if b != bad]
    part = G.oracle_newton(O, s, vals[keep], rhs[keep], np.zeros(B - 1, np.float32), p32)
    ref = {k: np.zeros((B,) + part[k].shape[1:], part[k].dtype) for k in part}
    for k in part:
        ref[k][keep] = part[k]
    v64 = vals[bad].astype(np.float64)
    d0, ok0, rho0, ro0, nf0 = O.newton_system(G.oracle_of(O, s), s.nvar, s.nequ, s.ncon, rhs[bad].astype(np.float64), v64, 0.0, p32.astype(np.float64))
    assert not ok0 and nf0 > 2 and rho0 > float(p32[6])
    ref["ok"][bad], ref["rho"][bad], ref["ro"][bad], ref["nf"][bad], ref["vals"][bad] = ok0, rho0, ro0, nf0, v64
    L = _handle(hipldl, s, B)
    v, d, ok, rho, ro, nf = _newton(hipldl, s, L, vals, rhs, np.zeros(B, np.float32), fill=7.0)
    L.close()
    G.check_results(s, ref, v, rhs, d, ok, rho, ro, nf)
    assert not ok[bad] and (d[bad] == 7.0).all()
    assert ok[keep].all() and (nf[keep] == 1).all()


# ---- 6. two-call sequence: try_to_factorize, then two solves on the kept factor ----
def test_two_call_sequence(built):
    hipldl, syn, O = _mods()
    s = _random_case()
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
    rhs2 = np.ascontiguousarray(rhs[::-1] * np.float32(0.5))
    for r in (rhs, rhs2):   # one launch each: the second solve factorises nothing
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
    L.close()


# ---- 7. ragged batches: the last partial group of the condense kernels and of the post-pass ----
@pytest.mark.parametrize("B", [5, 1])
def test_ragged_batches_tiled_kernel(built, B):
    hipldl, syn, O = _mods()
    s = _random_case()
    vals, rhs = _mixed_batch(syn, s)
    L = _handle(hipldl, s, B)
    assert L.plan_array("cond_info")[0] == 1 and not L.config["cond_resident"]
    check(f"random-ragged-{B}", s, vals[6 - B:6].copy(), rhs[6 - B:6].copy(), L=L)   # (the indefinite problem 5 is the last one)
    L.close()


@pytest.mark.parametrize("name", ["dense-40-70", "dense-100-160"])
def test_list_kernels_on_a_dense_jacobian_agree_with_the_resident_kernel(built, name):
    """float32_condense = 2 keeps the list kernels where 1 takes the resident one: the tiled kernel at dense_structure(40, 70), the
    plain slot kernel at (100, 160) — there on five problems, one full group of CPB = 4 and one more.  All three sum a slot's
    contributions in list order with the same operations, so the results are bit-equal."""
    hipldl, syn, O = _mods()
    if name == "dense-40-70":
        s = syn.dense_structure(40, 70)
        vals, rhs = G.dense_inputs(syn, s, range(100, 110))
    else:
        s = syn.dense_structure(100, 160)
        vals, rhs = G.dense_inputs(syn, s, range(100, 104))
        vals, rhs = np.concatenate([vals, vals[:1]]), np.concatenate([rhs, rhs[:1]])
    B = vals.shape[0]
    L = _handle(hipldl, s, B, condense=2)
    assert not L.config["cond_resident"] and L.plan_array("cond_info")[0] == (1 if name == "dense-40-70" else 0)
    d, _, _, _ = check(name + "-lists", s, vals, rhs, L=L)
    L.close()
    Lr = _handle(hipldl, s, B)
    assert Lr.config["cond_resident"]
    dr, _, _, _ = check(name + "-lists", s, vals, rhs, L=Lr)
    Lr.close()
    assert np.array_equal(G.bits(d), G.bits(dr))
    if name == "dense-100-160":
        assert np.array_equal(G.bits(d[4]), G.bits(d[0]))


# ---- 8. cnl_set_active_batch ----
@pytest.mark.parametrize("nb", [7, 6])
def test_active_prefix(built, nb):
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
                 ro=torch.full((B,), fill, dtype=torch.float32, device=dev), rho=torch.full((B,), fill, dtype=torch.float32, device=dev),
                 nf=torch.full((B,), int(fill), dtype=torch.int32, device=dev), ok=torch.full((B,), int(fill), dtype=torch.int32, device=dev))
        t["ro"][:nb] = 0.0
        c0 = hipldl.launch_counts()
        hipldl.newton_system_dev(L, t["v"], t["r"], t["d"], t["ro"], t["rho"], t["nf"], t["ok"], p32)
        torch.cuda.synchronize()
        _general_only(hipldl, c0)
        return {k: x.cpu().numpy() for k, x in t.items()}

    a = run()
    assert a["nf"][5] > 1 and a["ok"].all()
    hipldl.set_active_batch(L, nb)
    assert hipldl.get_active_batch(L) == nb
    c = run(fill=9.0)
    for k in ("d", "rho", "nf", "ok", "ro", "v"):
        assert np.array_equal(c[k][:nb].view(np.uint8), a[k][:nb].view(np.uint8)), k
    assert (c["d"][nb:] == 9.0).all() and (c["rho"][nb:] == 9.0).all() and (c["ro"][nb:] == 9.0).all()
    assert (c["nf"][nb:] == 9).all() and (c["ok"][nb:] == 9).all()
    assert np.array_equal(c["v"][nb:].view(np.uint8), vals[nb:].view(np.uint8))
    hipldl.set_active_batch(L, B)
    e2 = run()
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), e2[k].view(np.uint8)), k
    L.close()


# ---- 9. condensed against uncondensed ----
@pytest.mark.parametrize("name", ["dense-40-70", "random-mixed"])
def test_condensed_against_uncondensed(built, name):
    hipldl, syn, O = _mods()
    if name == "dense-40-70":
        s = syn.dense_structure(40, 70)
        vals, rhs = G.dense_inputs(syn, s, range(100, 110))
    else:
        s = _random_case()
        vals, rhs = _mixed_batch(syn, s)
    B = vals.shape[0]
    ro32 = np.zeros(B, np.float32)
    got = []
    for condense in (1, 0):
        L = _handle(hipldl, s, B, condense=condense)
        got.append(_newton(hipldl, s, L, vals, rhs, ro32))
        L.close()
    (v1, d1, ok1, rho1, _, nf1), (v0, d0, ok0, rho0, _, nf0) = got
    assert np.array_equal(ok1, ok0) and np.array_equal(nf1, nf0) and np.array_equal(G.bits(rho1), G.bits(rho0))
    assert np.array_equal(G.bits(v1[:, -s.nvar:]), G.bits(v0[:, -s.nvar:]))
    ref = _ref(O, hipldl, (name, 0.0), s, vals, rhs, ro32)
    for b in range(B):   # both are within FWD_TOL of the oracle
        assert np.abs(d1[b] - d0[b]).max() <= 2 * G.FWD_TOL * np.abs(ref["d"][b]).max(), b


# ---- 10. host-pointer and device-pointer entry points ----
def test_host_and_device_entry_points_agree(built):
    import torch
    hipldl, syn, O = _mods()
    s = syn.dense_structure(40, 70)
    vals, rhs = G.dense_inputs(syn, s, range(100, 110))
    B = vals.shape[0]
    p32 = hipldl.default_params(np.float32)
    L = _handle(hipldl, s, B)
    v, d, ok, rho, ro, nf = _newton(hipldl, s, L, vals, rhs, np.zeros(B, np.float32))
    dev = torch.device("cuda", 0)
    t = dict(v=torch.from_numpy(vals).to(dev), r=torch.from_numpy(rhs).to(dev), d=torch.zeros((B, s.N), dtype=torch.float32, device=dev),
             ro=torch.zeros(B, dtype=torch.float32, device=dev), rho=torch.zeros(B, dtype=torch.float32, device=dev),
             nf=torch.zeros(B, dtype=torch.int32, device=dev), ok=torch.zeros(B, dtype=torch.int32, device=dev))
    c0 = hipldl.launch_counts()
    hipldl.newton_system_dev(L, t["v"], t["r"], t["d"], t["ro"], t["rho"], t["nf"], t["ok"], p32)
    torch.cuda.synchronize()
    _general_only(hipldl, c0)
    L.close()
    g = {k: x.cpu().numpy() for k, x in t.items()}
    assert np.array_equal(G.bits(g["d"]), G.bits(d)) and np.array_equal(G.bits(g["v"]), G.bits(v))
    assert np.array_equal(G.bits(g["rho"]), G.bits(rho)) and np.array_equal(G.bits(g["ro"]), G.bits(ro))
    assert np.array_equal(g["nf"], nf) and np.array_equal(g["ok"].astype(bool), ok)


# ---- 11. the lockstep loop ----
def test_lockstep_loop(built):
    import torch
    hipldl, syn, O = _mods()
    from cannoles_jl_amd import device_loop as DL, outer_loop
    from tests.test_oracle_pinning import oracle_newton, oracle_solver
    B = 12
    tuning = {"float32_general": 1, "float32_condense": 1}
    fam = DL.BandQuadFamily(syn.band_structure(300, 4, hw=3), B, seed=304, torch=torch, device="cuda:0", dtype=np.float32)
    got = DL.solve_batch_device(fam, tuning=tuning)
    assert got["dtype"] == "float32" and got["kernel"] == "v1" and got["vals_layout"] == "problem-major"
    assert got["status"] == ["first_order"] * B
    prm = hipldl.default_params()
    dx = dl = 0.0
    for b in range(B):
        one = outer_loop.solve(fam.host_model(b), oracle_solver, oracle_newton, prm)
        assert one["status"] == "first_order"
        dx = max(dx, float(np.abs(got["solution"][b].astype(np.float64) - one["solution"]).max()))
        dl = max(dl, float(np.abs(got["multipliers"][b].astype(np.float64) - one["multipliers"]).max()))
    print(f"float32 lockstep loop on the condensed general handle: max|dx| = {dx:.3e}, max|dlambda| = {dl:.3e}, steps = {got['steps']}, "
          f"iter = {got['iter'].tolist()}")
    assert dx <= MULTIPRECISION_ATOL and dl <= MULTIPRECISION_ATOL
    cp = DL.solve_batch_device(fam, tuning=tuning, compact=True, compact_min_finished=1)
    assert cp["kernel"] == "v1" and cp["status"] == got["status"] and cp["handle_shrunk"] is True
    for k in ("iter", "nlinsolve", "nfact", "nbk"):
        assert np.array_equal(cp[k], got[k]), k
    assert np.array_equal(G.bits(cp["solution"]), G.bits(got["solution"]))
    assert np.array_equal(G.bits(cp["multipliers"]), G.bits(got["multipliers"]))


# ---- 12. refusals: nothing launched ----
def test_refusals(built):
    hipldl, syn, O = _mods()
    lib = hipldl.lib()
    s = _random_case()
    rows, cols = s.kkt_pattern()
    B = 4
    c0 = hipldl.launch_counts()
    with pytest.raises(hipldl.CnlError) as e:   # the key alone serves no pattern the band kernels refuse
        hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32, options=hipldl.Options(float32_condense=1))
    assert e.value.code == CNL_ERR_ARG and "build_band_plan" in str(e.value)
    with pytest.raises(hipldl.CnlError) as e:   # the interleaved layout is the band kernels'
        hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32,
                            options=hipldl.Options(float32_general=1, float32_condense=1, batch_layout=hipldl.LAYOUT_INTERLEAVED))
    assert e.value.code == CNL_ERR_ARG
    L = _handle(hipldl, s, B)
    p64 = hipldl.default_params()
    buf = np.full((B, max(s.nnzNS, s.N) * 2), 3.0, np.float64)
    ib = np.full(4 * B, 3, np.int64)
    a, i = buf.ctypes.data, ib.ctypes.data
    for call in (lambda h: lib.cnl_factorize(h, a, 1e-8, i, None, None), lambda h: lib.cnl_solve(h, a, a),
                 lambda h: lib.cnl_newton_system(h, a, a, a, a, p64.ctypes.data, a, a, i, i),
                 lambda h: lib.cnl_newton_system_dev(h, a, a, a, a, a, i, i, p64.ctypes.data, None)):
        assert call(L._h) == CNL_ERR_STATE, lib.cnl_last_error()
    assert lib.cnl_solve_f32(L._h, a, a) == CNL_ERR_STATE and b"before cnl_factorize" in lib.cnl_last_error()
    assert hipldl.launch_counts() == c0
    assert (buf == 3.0).all() and (ib == 3).all()
    L.close()
    # a band pattern keeps its band handle whatever the two keys say
    sb = syn.band_structure(400, 4)
    rb, cb = sb.kkt_pattern()
    Lb = hipldl.HIPLDLStruct(sb.N, rb, cb, None, sb.nvar, sb.nequ, sb.ncon, batch=B, dtype=np.float32,
                             options=hipldl.Options(float32_general=1, float32_condense=1))
    assert Lb.config["band"] and Lb.config["kernel"] == "band"
    Lb.close()
