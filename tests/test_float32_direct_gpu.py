"""Float32 general handles on the Direct route (cnl_create_f32 with tuning float32_general = 1, float32_register_front = 1 and
float32_direct_records = 1: the float instantiation of csrc/kernels2.hip on direct records — it condenses on the fly from the
caller's vals and writes the kept components of d itself) against the fp64 oracle on the widened float32 inputs with
ParamCaNNOLeS(Float32) widened.  -m gpu.

`check` means, through hipldl.newton_system_ on such a handle: (success, nfact) identical to the oracle; rho, rho_old and the rho slots
of vals bit-equal to the oracle's rounded to float32; backward error <= 512 eps(Float32) and forward error <= 1e-3
(tests/support/f32_general.py: oracle_newton with its per-problem pivot-margin assertion, check_results; unchanged); the handle
reports float32, no band kernels, kernel "v2", config["direct"] and info["ncond"] > 0; and the call is exactly one launch of the
register-front kernel family and none of the other two.  The inputs are those of tests/test_float32_register_front_gpu.py.  Direct
and condensed handles sum the condensation products in different orders: between the two kinds only decisions are compared, never d.
Every test here fails on a library without the tuning key.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.support import f32_direct as D
from tests.support import f32_general as G
from tests.support import f32_register_front as R
from tests.test_float32_general_gpu import MULTIPRECISION_ATOL

pytestmark = pytest.mark.gpu

CNL_ERR_ARG = 1
bits = G.bits


def _classes(L):
    return (L.info["v2"]["fronts16"], L.info["v2"]["fronts32"], L.info["v2"]["fronts64"])


# ---- parity against the oracle ----
def test_chain_of_class16_fronts(built):
    hipldl, syn, O = D.mods()
    s = R.chain(syn)
    L = D.handle(hipldl, s, 13)
    assert _classes(L) == (7, 0, 0) and L.config["v2_solve"]
    assert L.config["wpb"] >= 1 and L.config["lds2_bytes"] > 0
    _, ref, _, _ = D.check("chain", s, *R.chain_inputs(syn, s), L=L)
    assert ref["ok"].all() and (ref["nf"] == 1).all()
    _, ref, _, _ = D.check("chain-ladder", s, *R.chain_inputs(syn, s, ladder=True), L=L)
    assert ref["ok"].all() and (ref["nf"] == 4).all()
    L.close()


def test_chain_update_matrices_in_global_scratch(built):
    hipldl, syn, O = D.mods()
    s = R.chain(syn)
    vals, rhs = R.chain_inputs(syn, s)
    L = D.handle(hipldl, s, 13, ubig=4)
    assert L.info["v2"]["ustack"] == 2, L.info
    dg, _, _, _ = D.check("chain", s, vals, rhs, L=L)
    L.close()
    d, _, _, _ = D.check("chain", s, vals, rhs)
    assert np.array_equal(bits(dg), bits(d))


def test_drop_in_one_problem(built):
    hipldl, syn, O = D.mods()
    s = R.chain(syn)
    vals, rhs = R.chain_inputs(syn, s)
    D.check("chain-one", s, vals[:1].copy(), rhs[:1].copy())


def test_class32_first_attempt(built):
    hipldl, syn, O = D.mods()
    s = R.class32(syn)
    L = D.handle(hipldl, s, 13)
    assert _classes(L) == (0, 2, 0) and not L.config["v2_solve"]
    _, ref, _, _ = D.check("class32", s, *G.random_inputs(syn, s, range(100, 113)), L=L)
    L.close()
    assert ref["ok"].all() and (ref["nf"] == 1).all()


@pytest.mark.parametrize("rho_old", [0.0, 0.3])
def test_class32_ladder(built, rho_old):
    hipldl, syn, O = D.mods()
    s = R.class32(syn)
    _, ref, _, _ = D.check("class32-indefinite", s, *G.random_inputs(syn, s, range(200, 213), posdef=False), rho_old=rho_old)
    assert ref["ok"].all()
    if rho_old == 0.0:
        assert (ref["nf"] == 4).all()
    else:
        assert set(ref["nf"].tolist()) <= {3, 4}


def test_class64_first_attempt(built):
    hipldl, syn, O = D.mods()
    s = R.class64(syn)
    L = D.handle(hipldl, s, 13)
    assert _classes(L) == (0, 0, 2) and not L.config["v2_solve"]
    _, ref, _, _ = D.check("class64-13", s, *G.random_inputs(syn, s, range(100, 113)), L=L)
    L.close()
    assert ref["ok"].all() and (ref["nf"] == 1).all()


@pytest.mark.parametrize("rho_old", [0.0, 0.3])
def test_class64_ladder(built, rho_old):
    hipldl, syn, O = D.mods()
    s = R.class64(syn)
    _, ref, _, _ = D.check("class64-indefinite-13", s, *G.random_inputs(syn, s, range(200, 213), posdef=False), rho_old=rho_old)
    assert ref["ok"].all() and (ref["nf"] > 1).all()


def test_class64_mixed_ladder_inside_a_wavefront(built):
    hipldl, syn, O = D.mods()
    s = R.class64(syn)
    _, ref, _, _ = D.check("random-mixed", s, *R.mixed_batch(syn, s))
    assert ref["nf"][5] > 1 and (np.delete(ref["nf"], 5) == 1).all()


def test_all_three_classes_in_one_tree(built):
    hipldl, syn, O = D.mods()
    s = R.mixed_classes(syn)
    L = D.handle(hipldl, s, 13)
    assert _classes(L) == (2, 3, 1)
    _, ref, _, _ = D.check("classes-posdef", s, *G.random_inputs(syn, s, range(100, 113)), L=L)
    assert ref["ok"].all() and (ref["nf"] == 1).all()
    _, ref, _, _ = D.check("classes-indefinite", s, *G.random_inputs(syn, s, range(200, 213), posdef=False), L=L)
    assert ref["ok"].all() and (ref["nf"] == 4).all()
    L.close()


# ---- bit-equality inside the handle kind: where a problem sits, how the wavefronts are grouped, which instance runs ----
def _cases(syn):
    s64 = R.class64(syn)
    smix = R.mixed_classes(syn)
    s = R.chain(syn)
    return [("chain",) + (s,) + R.chain_inputs(syn, s), ("classes",) + (smix,) + G.random_inputs(syn, smix, range(100, 113)),
            ("class64",) + (s64,) + G.random_inputs(syn, s64, range(100, 113))]


def test_lane_group_of_a_problem(built):
    """one problem at each of the four positions of a wavefront, and alone: a bit-equal d"""
    hipldl, syn, O = D.mods()
    for key, s, vals, rhs in _cases(syn):
        L1 = D.handle(hipldl, s, 1)
        _, d1, ok1, *_ = D.newton(hipldl, s, L1, vals[:1].copy(), rhs[:1].copy(), np.zeros(1, np.float32))
        L1.close()
        assert ok1 is True
        L = D.handle(hipldl, s, 4)
        for pos in range(4):
            idx = [1, 2, 3]
            idx.insert(pos, 0)
            _, d, ok, *_ = D.newton(hipldl, s, L, vals[idx].copy(), rhs[idx].copy(), np.zeros(4, np.float32))
            assert ok.all()
            assert np.array_equal(bits(d[pos]), bits(d1)), (key, pos)
        L.close()


def test_wavefronts_per_workgroup(built):
    hipldl, syn, O = D.mods()
    for key, s, vals, rhs in _cases(syn):
        got = []
        for wpb in (1, 2, 4):
            L = D.handle(hipldl, s, 13, waves_per_block=wpb)
            assert L.config["wpb"] == wpb, L.config
            got.append(D.newton(hipldl, s, L, vals, rhs, np.zeros(13, np.float32))[1])
            L.close()
        assert np.array_equal(bits(got[0]), bits(got[1])) and np.array_equal(bits(got[0]), bits(got[2])), key


def test_late_instance_on_a_large_batch(built):
    """4 096 problems are 1 024 wavefronts: the launcher takes the instance that stores its L rows one front late"""
    hipldl, syn, O = D.mods()
    s = R.chain(syn)
    for ladder in (False, True):
        vals, rhs = R.chain_inputs(syn, s, ladder=ladder)
        L13 = D.handle(hipldl, s, 13)
        v13, d13, ok13, rho13, ro13, nf13 = D.newton(hipldl, s, L13, vals, rhs, np.zeros(13, np.float32))
        L13.close()
        B = 4096
        idx = np.arange(B) % 13
        L = D.handle(hipldl, s, B)
        v, d, ok, rho, ro, nf = D.newton(hipldl, s, L, vals[idx], rhs[idx], np.zeros(B, np.float32))
        L.close()
        assert np.array_equal(bits(d), bits(d13[idx])) and np.array_equal(bits(v), bits(v13[idx]))
        assert np.array_equal(ok, ok13[idx]) and np.array_equal(nf, nf13[idx])
        assert np.array_equal(bits(rho), bits(rho13[idx])) and np.array_equal(bits(ro), bits(ro13[idx]))


def _dev_run(hipldl, torch, s, L, vals, rhs, fill=0.0, nb=None):
    B = vals.shape[0]
    dev = torch.device("cuda", 0)
    t = dict(v=torch.from_numpy(vals).to(dev), r=torch.from_numpy(rhs).to(dev), d=torch.full((B, s.N), fill, dtype=torch.float32, device=dev),
             ro=torch.full((B,), fill, dtype=torch.float32, device=dev), rho=torch.full((B,), fill, dtype=torch.float32, device=dev),
             nf=torch.full((B,), int(fill), dtype=torch.int32, device=dev), ok=torch.full((B,), int(fill), dtype=torch.int32, device=dev))
    t["ro"][:B if nb is None else nb] = 0.0
    c0 = hipldl.launch_counts()
    hipldl.newton_system_dev(L, t["v"], t["r"], t["d"], t["ro"], t["rho"], t["nf"], t["ok"], hipldl.default_params(np.float32))
    torch.cuda.synchronize()
    D.launches(hipldl, c0, register_front=1)
    return {k: x.cpu().numpy() for k, x in t.items()}


def test_host_and_device_entry_points_agree(built):
    import torch
    hipldl, syn, O = D.mods()
    s = R.mixed_classes(syn)
    vals, rhs = G.random_inputs(syn, s, range(200, 213), posdef=False)
    B = vals.shape[0]
    L = D.handle(hipldl, s, B)
    v, d, ok, rho, ro, nf = D.newton(hipldl, s, L, vals, rhs, np.zeros(B, np.float32))
    g = _dev_run(hipldl, torch, s, L, vals, rhs)
    L.close()
    assert np.array_equal(bits(g["d"]), bits(d)) and np.array_equal(bits(g["v"]), bits(v))
    assert np.array_equal(bits(g["rho"]), bits(rho)) and np.array_equal(bits(g["ro"]), bits(ro))
    assert np.array_equal(g["nf"], nf) and np.array_equal(g["ok"].astype(bool), ok)


# ---- active batch ----
def test_active_batch(built):
    import torch
    hipldl, syn, O = D.mods()
    s = R.chain(syn)
    vals, rhs = R.chain_inputs(syn, s, ladder=True)
    B, nb = 13, 5
    L = D.handle(hipldl, s, B)
    a = _dev_run(hipldl, torch, s, L, vals, rhs)
    assert a["ok"].all() and (a["nf"] == 4).all()
    hipldl.set_active_batch(L, nb)
    assert hipldl.get_active_batch(L) == nb
    c = _dev_run(hipldl, torch, s, L, vals, rhs, fill=9.0, nb=nb)
    for k in ("d", "rho", "nf", "ok", "ro", "v"):
        assert np.array_equal(c[k][:nb].view(np.uint8), a[k][:nb].view(np.uint8)), k
    assert (c["d"][nb:] == 9.0).all() and (c["rho"][nb:] == 9.0).all() and (c["ro"][nb:] == 9.0).all()
    assert (c["nf"][nb:] == 9).all() and (c["ok"][nb:] == 9).all()
    assert np.array_equal(c["v"][nb:].view(np.uint8), vals[nb:].view(np.uint8))   # the caller's vals beyond nb: untouched
    hipldl.set_active_batch(L, B)
    e2 = _dev_run(hipldl, torch, s, L, vals, rhs)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), e2[k].view(np.uint8)), k
    L.close()


# ---- two calls ----
def _two_calls(hipldl, syn, O, s, vals, rhs, L, solve_launch, failed=()):
    """try_to_factorize against the oracle's (success, npos, nzero) with one launch of family 1; two right-hand sides through
    solve_ldl_, each the launch `solve_launch` names; d within the bar against a dense fp64 solve; failed problems keep their fill"""
    B = vals.shape[0]
    p32 = hipldl.default_params(np.float32)
    c0 = hipldl.launch_counts()
    ok, npos, nzer = hipldl.try_to_factorize(L, vals, s.nvar, s.nequ, s.ncon, p32[0], return_inertia=True)
    D.launches(hipldl, c0, register_front=1)
    orc = G.oracle_of(O, s)
    for b in range(B):
        ok0, np0, nz0 = orc.try_to_factorize(vals[b].astype(np.float64), s.nvar, s.nequ, s.ncon, float(p32[0]), return_inertia=True)
        assert (bool(ok[b]), int(npos[b]), int(nzer[b])) == (ok0, np0, nz0), b
    assert [b for b in range(B) if not ok[b]] == list(failed)
    rhs2 = np.ascontiguousarray(rhs[::-1] * np.float32(0.5))
    for r in (rhs, rhs2):
        d = np.full((B, s.N), 7.0, np.float32)
        c0 = hipldl.launch_counts()
        assert hipldl.solve_ldl_(r, L.factor, d) is True
        D.launches(hipldl, c0, **solve_launch)
        for b in range(B):
            if b in failed:
                assert np.all(d[b] == 7.0), b
                continue
            d0 = -np.linalg.solve(syn.dense_kkt(s, vals[b].astype(np.float64)), r[b].astype(np.float64))
            assert G.backward_error(s, vals[b], r[b], d[b]) <= G.BWD_TOL, b
            assert np.abs(d[b] - d0).max() <= G.FWD_TOL * np.abs(d0).max(), b


def test_two_call_sequence_on_the_same_kernel(built):
    """every front of the chain is of the fast class: solve_ldl! runs the forward substitution and the backward sweep of the
    register-front kernel's float solve instance, from the factorisation's vals (alive and unmodified: the Direct handles' contract)"""
    hipldl, syn, O = D.mods()
    s = R.chain(syn)
    vals, rhs = R.chain_inputs(syn, s)
    L = D.handle(hipldl, s, vals.shape[0])
    assert L.config["v2_solve"]
    _two_calls(hipldl, syn, O, s, vals, rhs, L, dict(register_front=1))
    L.close()


def test_two_call_sequence_with_out_of_line_fronts(built):
    hipldl, syn, O = D.mods()
    s = R.class64(syn)
    vals, rhs = R.mixed_batch(syn, s)
    L = D.handle(hipldl, s, vals.shape[0])
    assert not L.config["v2_solve"]
    _two_calls(hipldl, syn, O, s, vals, rhs, L, dict(general=1), failed=(5,))
    L.close()


# ---- refusals and defaults ----
@pytest.mark.parametrize("name", ["dense-24-40", "chain-hw4"])
def test_refused_direct_records_keep_todays_handle(built, name):
    hipldl, syn, O = D.mods()
    if name == "chain-hw4":
        s = syn.band_structure(60, 2, hw=4)
        vals, rhs = G.band_inputs(syn, s, range(4000, 4005))
    else:
        s = syn.dense_structure(24, 40)
        vals, rhs = G.dense_inputs(syn, s, range(100, 105))
    B = vals.shape[0]
    L = D.handle(hipldl, s, B, direct=False)
    assert not L.config["v2_solve"]
    a = D.newton(hipldl, s, L, vals, rhs, np.zeros(B, np.float32))
    L.close()
    L0 = R.handle(hipldl, s, B)
    c = R.newton(hipldl, s, L0, vals, rhs, np.zeros(B, np.float32))
    L0.close()
    for x, y in zip(a, c):   # vals, d, flags, rho, rho_old, nfact
        x, y = np.asarray(x), np.asarray(y)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_defaults(built):
    hipldl, syn, O = D.mods()
    s = R.chain(syn)
    rows, cols = s.kkt_pattern()
    L0 = R.handle(hipldl, s, 4)   # without the key: the condensation passes around the launch
    assert not L0.config["direct"] and not L0.config["v2_solve"]
    L0.close()
    Lg = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=4, dtype=np.float32,
                             options=hipldl.Options(float32_general=1, float32_condense=1, float32_direct_records=1))
    assert Lg.config["kernel"] == "v1" and Lg.config["float32"] and not Lg.config["direct"]   # the key without float32_register_front: nothing
    Lg.close()
    with pytest.raises(hipldl.CnlError) as e:   # the interleaved layout is the band kernels'
        hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=4, dtype=np.float32,
                            options=hipldl.Options(batch_layout=hipldl.LAYOUT_INTERLEAVED, **D.KEYS))
    assert e.value.code == CNL_ERR_ARG
    sb = syn.band_structure(400, 4)   # a pattern the band kernels serve keeps its band handle
    rb, cb = sb.kkt_pattern()
    Lb = hipldl.HIPLDLStruct(sb.N, rb, cb, None, sb.nvar, sb.nequ, sb.ncon, batch=4, dtype=np.float32, options=hipldl.Options(**D.KEYS))
    assert Lb.config["band"] and Lb.config["kernel"] == "band" and not Lb.config["direct"]
    Lb.close()
    Ld = hipldl.HIPLDLStruct(sb.N, rb, cb, None, sb.nvar, sb.nequ, sb.ncon, batch=4,   # the bits are correct for Float64 handles too
                             options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT))
    assert Ld.config["band"] and not Ld.config["direct"] and not Ld.config["v2_solve"]
    Ld.close()
    Lf = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=4, options=hipldl.Options(band_kernel=0))
    assert Lf.config["direct"] and Lf.config["v2_solve"] and not Lf.config["float32"], Lf.config
    Lf.close()


# ---- garbage left by earlier kernels ----
def test_results_do_not_depend_on_what_earlier_kernels_left(built):
    """Five cases in a child process (tests/support/f32_direct.py as a script), once as it is and once each with kernels in front
    of every launch that leave a byte pattern in LDS, scratch memory and the vector registers: the digests of every output are the
    same in the three runs."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for fill in (None, "0x7fc00000", "0xffffffff"):
        env = dict(os.environ)
        if fill:
            env.update(CNL_DBG_SCRATCHFILL="1", CNL_DBG_LDSFILL=fill)
        r = subprocess.run([sys.executable, "-m", "tests.support.f32_direct"], env=env, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
        lines = [ln for ln in r.stdout.splitlines() if ln and not ln.startswith("[")]
        assert lines[-1] == "done" and len(lines) == 6, r.stdout[-1500:]
        outs.append(lines)
    assert outs[0] == outs[1] == outs[2], outs


# ---- the lockstep loop ----
def test_lockstep_loop(built):
    import torch
    hipldl, syn, O = D.mods()
    from cannoles_jl_amd import device_loop as DL, outer_loop
    from tests.test_oracle_pinning import oracle_newton, oracle_solver
    B = 12
    tuning = dict(D.KEYS)
    fam = DL.BandQuadFamily(syn.band_structure(300, 4, hw=3), B, seed=304, torch=torch, device="cuda:0", dtype=np.float32)
    got = DL.solve_batch_device(fam, tuning=tuning)
    assert got["dtype"] == "float32" and got["kernel"] == "v2" and got["vals_layout"] == "problem-major"
    assert got["status"] == ["first_order"] * B
    prm = hipldl.default_params()
    dx = dl = 0.0
    for b in range(B):
        one = outer_loop.solve(fam.host_model(b), oracle_solver, oracle_newton, prm)
        assert one["status"] == "first_order"
        dx = max(dx, float(np.abs(got["solution"][b].astype(np.float64) - one["solution"]).max()))
        dl = max(dl, float(np.abs(got["multipliers"][b].astype(np.float64) - one["multipliers"]).max()))
    print(f"float32 lockstep loop on the direct handle: max|dx| = {dx:.3e}, max|dlambda| = {dl:.3e}, steps = {got['steps']}")
    assert dx <= MULTIPRECISION_ATOL and dl <= MULTIPRECISION_ATOL
    cp = DL.solve_batch_device(fam, tuning=tuning, compact=True, compact_min_finished=1)
    assert cp["kernel"] == "v2" and cp["status"] == got["status"]
    assert np.array_equal(bits(cp["solution"]), bits(got["solution"]))
    assert np.array_equal(bits(cp["multipliers"]), bits(got["multipliers"]))
