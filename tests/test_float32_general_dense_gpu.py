"""Float32 general handles on the general form of the dense backend (cnl_create_f32 with tuning float32_general = 1,
float32_general_dense = 1: an irregular condensed system with a front above order 64 as ONE dense matrix on the float kernels of
csrc/dense_f32.hip) against the fp64 oracle on the widened float32 inputs with ParamCaNNOLeS(Float32) widened.  -m gpu.

Inputs, reference, tolerances and the per-call bar are those of tests/support/f32_general_dense.py (the bar: f32_dense.check_outputs);
tests/test_float32_general_dense_cpu.py vouches for the inputs — every decision of every rung at least 1e-3 away from a flip, by
eigenvalues — so no problem is skipped or reclassified here."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.support import f32_general as G
from tests.support import f32_general_dense as GD

pytestmark = pytest.mark.gpu

CNL_ERR_ARG, CNL_ERR_STATE = 1, 5


def _mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    return hipldl, syn


def _route_handle(hipldl, c, B, **opt):
    L = GD.handle(hipldl, c, B, **opt)
    assert L.config["kernel"] == "dense" and L.config["float32"] and L.info["ncond"] > 0 and not L.config["band"], L.config
    return L


def _captured(capfd):
    """n where the call just made captured its sequence as the handle's n-th cached graph (the line csrc/dense_impl.h prints under
    CNL_VERBOSE), 0 where it replayed a cached graph or ran plain launches"""
    err = capfd.readouterr().err
    return next((n for n in range(1, 10) if f"captured as a graph ({n} cached)" in err), 0)


def _host_newton(hipldl, s, L, vals, rhs, ro, p32):
    B = vals.shape[0]
    v = vals.copy()
    d, ok, rho, ro_out, nf = hipldl.newton_system_(np.full((B, s.N), 7.0, np.float32), s.nvar, s.nequ, s.ncon, rhs.copy(), v, L, ro.copy(), p32)
    return dict(vals=v, d=d, ok=np.asarray(ok).astype(np.int32), rho=rho, ro=ro_out, nf=np.asarray(nf))


# ---- 1. device entry, every shape, both panel kernels ----
@pytest.mark.parametrize("panel_blocks", [0, 1])
@pytest.mark.parametrize("shape", list(GD.SHAPES), ids=GD.shape_id)
def test_shapes_and_panel_kernels(built, shape, panel_blocks):
    """cnl_newton_system_f32_dev at every shape of the table; dense_panel_blocks = 0: dnf_panel, 1: dnf_panel2 (batch x tiles <= 512).
    The second call, batch reversed, finds nothing stale from the first; cnl_solve_f32_dev then uses the factor and the rho the
    ladder ended on."""
    import torch
    hipldl, syn = _mods()
    c = GD.case(shape)
    s, B = c["s"], GD.MIX
    L = _route_handle(hipldl, c, B, dense_panel_blocks=panel_blocks)
    A = GD.Args(s, B)
    for idx in (np.arange(B), np.arange(B)[::-1]):
        A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
        A.call(hipldl, L, c["p32"])
        out = A.read()
        be, fe = GD.check_outputs(c, out, idx, c["vals"][idx])
        print(f"{GD.shape_id(shape)} panel_blocks {panel_blocks}: backward error {be / GD.EPS32:.1f} eps32, forward error {fe:.2e}")
    rhs2 = np.random.default_rng(5).standard_normal((B, s.N)).astype(np.float32)
    t_rhs2 = torch.from_numpy(rhs2).to("cuda:0")
    t_x = torch.zeros_like(t_rhs2)
    hipldl.solve_dev(L, t_rhs2, t_x, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    x = t_x.cpu().numpy()
    for k, b in enumerate(idx):
        if c["ok"][b]:
            be = G.backward_error(s, out["vals"][k], rhs2[k], x[k])
            assert be <= GD.BWD_TOL, (b, be)
    L.close()


# ---- 2. the two-call sequence ----
@pytest.mark.parametrize("shape", list(GD.SHAPES), ids=GD.shape_id)
def test_two_call_sequence(built, shape):
    """cnl_factorize_f32_dev, then cnl_solve_f32_dev twice with different right-hand sides on the one factor: success as the
    oracle's try_to_factorize on the widened data, every d of a factorised problem within BWD_TOL.  The host entry (the device entry
    behind an upload) also hands back the inertia: npos and nzero as the oracle's — the CPU test's eigenvalue margins make the
    inertia of every problem that is not hopeless a property of the matrix, not of the order or the precision."""
    import torch
    from oracle import oracle as O
    hipldl, syn = _mods()
    c = GD.case(shape)
    s, B = c["s"], GD.MIX
    orc = G.oracle_of(O, s)
    eig_tol = float(c["p32"][0])
    ref = [orc.try_to_factorize(c["vals"][b].astype(np.float64), s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True) for b in range(B)]
    want = [bool(r[0]) for r in ref]
    assert want == [True, False, False, False, True]
    L = _route_handle(hipldl, c, B)
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
                assert be <= GD.BWD_TOL, (b, k, be)
    assert np.array_equal(GD.bits(t_vals.cpu().numpy()), GD.bits(c["vals"]))      # try_to_factorize and solve_ldl! leave vals alone
    ok, npos, nzer = hipldl.try_to_factorize(L, np.array(c["vals"]), s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True)
    print(f"{GD.shape_id(shape)}: npos {list(npos)} nzero {list(nzer)}; oracle {[(int(r[1]), int(r[2])) for r in ref]}")
    assert list(ok) == want
    for b in range(B):
        if b % 5 != 1:     # (the hopeless problem's pivots are NaN: it fails, and its counts mean nothing in either arithmetic)
            assert (int(npos[b]), int(nzer[b])) == (int(ref[b][1]), int(ref[b][2])), b
    L.close()


# ---- 3. host-pointer call = device call ----
@pytest.mark.parametrize("shape", [(92, 110, 4, 0.08, 2), (129, 150, 0, 0.06, 5)], ids=GD.shape_id)
def test_host_entry_equals_dev_entry(built, shape):
    hipldl, syn = _mods()
    c = GD.case(shape)
    s, B = c["s"], GD.MIX
    L = _route_handle(hipldl, c, B)
    A = GD.Args(s, B)
    A.fill(c["vals"], c["rhs"], c["rho_old"])
    A.call(hipldl, L, c["p32"])
    dev = A.read()
    GD.check_outputs(c, dev, np.arange(B), c["vals"])
    host = _host_newton(hipldl, s, L, c["vals"], c["rhs"], c["rho_old"], c["p32"])
    L.close()
    assert np.array_equal(host["ok"], dev["ok"]) and np.array_equal(host["nf"], dev["nf"])
    for name in ("rho", "ro", "vals", "d"):     # bit for bit, the untouched rows of the hopeless problem included
        assert np.array_equal(GD.bits(host[name]), GD.bits(dev[name])), name


# ---- 4. graph replay ----
def test_graph_replay(built, monkeypatch, capfd):
    """One argument set called twice (capture, then replay), a second set of pointers with another right-hand side, the first set
    again with another rho0 in params, and the second set again (replay): every output bit-equal to what a handle without graphs
    returns for the same call, so a replay of a stale graph — old pointers, old params — shows.  Two mixes (B = 10).  The handle
    with dense_graph = 1 really captures and replays: the states of its cache are read off the CNL_VERBOSE line of
    csrc/dense_impl.h, as tests/test_dense_gpu.py::test_dense_graph_cache_states does for the double form — calls 0, 2 and 3
    capture graphs 1, 2 and 3, calls 1 and 4 replay; the handle with dense_graph = 0 never captures."""
    hipldl, syn = _mods()
    B = 2 * GD.MIX
    c = GD.case(GD.SMALLEST, B)
    s = c["s"]
    p2 = c["p32"].copy()
    p2[5] *= np.float32(3.0)
    rhs2 = np.ascontiguousarray(c["rhs"] * np.float32(1.25))
    calls = [(0, c["rhs"], c["p32"]), (0, c["rhs"], c["p32"]), (1, rhs2, c["p32"]), (0, c["rhs"], p2), (1, rhs2, c["p32"])]
    outs, seen = {}, {}
    monkeypatch.setenv("CNL_VERBOSE", "1")
    for graph in (0, 1):
        L = _route_handle(hipldl, c, B, dense_graph=graph)
        sets = [GD.Args(s, B), GD.Args(s, B)]
        assert sets[0].vals.data_ptr() != sets[1].vals.data_ptr()
        outs[graph], seen[graph] = [], []
        capfd.readouterr()
        for k, rhs, p in calls:
            sets[k].fill(c["vals"], rhs, c["rho_old"])
            sets[k].call(hipldl, L, p)
            outs[graph].append(sets[k].read())
            seen[graph].append(_captured(capfd))
        L.close()
    monkeypatch.delenv("CNL_VERBOSE")
    assert seen[0] == [0, 0, 0, 0, 0] and seen[1] == [1, 0, 2, 3, 0], seen
    GD.check_outputs(c, outs[0][0], np.arange(B), c["vals"])
    for name in ("vals", "d", "ro", "rho", "nf", "ok"):
        for call in range(len(calls)):
            assert outs[1][call][name].tobytes() == outs[0][call][name].tobytes(), (name, call)
        assert outs[1][1][name].tobytes() == outs[1][0][name].tobytes(), name
        assert outs[1][4][name].tobytes() == outs[1][2][name].tobytes(), name
    climbers = np.arange(B) % 5 == 2       # rho_old = 0: the ladder starts at rho0
    assert (outs[1][3]["rho"][climbers] != outs[1][0]["rho"][climbers]).all()      # the changed params were honoured
    healthy = np.arange(B) % 5 == 0
    assert not np.array_equal(outs[1][2]["d"][healthy], outs[1][0]["d"][healthy])  # ... and so were the changed pointers


def _small_copies(t, n=16):
    """a burst of small device-to-host copies between two calls: host-side traffic of the kind that stood between a capture and the
    replay that went wrong"""
    for _ in range(n):
        t[:1].cpu()


def test_repeated_calls_at_256_problems(built, monkeypatch, capfd):
    """The sequence on which a replayed graph of this route answered success = 0, nfact = 10 for every problem while S0 was zeroed
    by a captured hipMemsetAsync (the replayed memset node left S0 full of values near 1e36; dn_zero16 zeroes
    it now): 256 healthy problems of order 129, one argument set, four calls with device-to-host copies between them.  The first
    call captures, the others replay; every call decides as the oracle does for the eight problems the batch repeats, and hands
    back the same bits as the first."""
    from oracle import oracle as O
    hipldl, syn = _mods()
    shape, B, nbase = (129, 150, 0, 0.06, 5), 256, 8
    c = GD.case(shape)
    s = c["s"]
    vals8, rhs8 = G.random_inputs(syn, s, range(40, 40 + 5 * nbase, 5))
    d_ref, ok_ref, _, _, nf_ref = O.newton_system_batch(G.oracle_of(O, s), nbase, s.nvar, s.nequ, s.ncon, rhs8.astype(np.float64),
                                                        vals8.astype(np.float64), np.zeros(nbase), c["p32"].astype(np.float64))
    assert np.asarray(ok_ref).all() and (np.asarray(nf_ref) == 1).all()
    idx = np.arange(B) % nbase
    L = _route_handle(hipldl, c, B)
    A = GD.Args(s, B)
    A.fill(vals8[idx], rhs8[idx], np.zeros(B, np.float32))
    first = None
    monkeypatch.setenv("CNL_VERBOSE", "1")
    capfd.readouterr()
    for call in range(4):
        A.call(hipldl, L, c["p32"])
        out = A.read()
        assert _captured(capfd) == (1 if call == 0 else 0), call
        _small_copies(A.ok)
        assert (out["ok"] == 1).all() and (out["nf"] == 1).all(), (call, int(out["ok"].sum()), int(out["nf"].max()))
        if first is None:
            first = out
            assert not out["rho"].any() and not out["ro"].any() and np.array_equal(GD.bits(out["vals"]), GD.bits(vals8[idx]))
            for b in range(nbase):
                be = G.backward_error(s, vals8[b], rhs8[b], out["d"][b])
                fe = np.abs(out["d"][b] - d_ref[b]).max() / np.abs(d_ref[b]).max()
                assert be <= GD.BWD_TOL and fe <= GD.FWD_TOL, (b, be, fe)
        for name in ("vals", "d", "ro", "rho"):
            assert out[name].tobytes() == first[name].tobytes(), (call, name)
    monkeypatch.delenv("CNL_VERBOSE")
    L.close()


def test_calls_behind_later_handles(built, monkeypatch, capfd):
    """... and the other one: one problem of order 129, a first call (capture), then a float32_condense handle and a Float64 default
    handle created and called — their creation is a long row of hipMemset and hipMemcpy calls —, then the first handle again, twice
    (replays)."""
    import torch
    hipldl, syn = _mods()
    c = GD.case((129, 150, 0, 0.06, 5))
    s = c["s"]
    L = _route_handle(hipldl, c, 1)
    A = GD.Args(s, 1)
    A.fill(c["vals"][:1], c["rhs"][:1], c["rho_old"][:1])
    monkeypatch.setenv("CNL_VERBOSE", "1")
    capfd.readouterr()
    A.call(hipldl, L, c["p32"])
    first = A.read()
    assert _captured(capfd) == 1
    GD.check_outputs(c, first, np.arange(1), c["vals"][:1])
    others = []
    for T, opt in ((np.float32, GD.BASE), (np.float64, {})):
        Lo = hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=1, dtype=T, options=hipldl.Options(**opt))
        v, r = c["vals"][:1].astype(T), c["rhs"][:1].astype(T)
        d, ok, *_ = hipldl.newton_system_(np.zeros(s.N, T), s.nvar, s.nequ, s.ncon, r[0].copy(), v[0].copy(), Lo, T(0), hipldl.default_params(T))
        assert ok
        others.append(Lo)
    capfd.readouterr()     # (the Float64 handle captured a graph of its own)
    for call in range(2):
        A.fill(c["vals"][:1], c["rhs"][:1], c["rho_old"][:1])
        A.call(hipldl, L, c["p32"])
        out = A.read()
        assert _captured(capfd) == 0, call     # the graph of the first call, replayed
        for name in ("vals", "d", "ro", "rho", "nf", "ok"):
            assert out[name].tobytes() == first[name].tobytes(), (call, name)
    monkeypatch.delenv("CNL_VERBOSE")
    torch.cuda.synchronize()
    for Lo in others:
        Lo.close()
    L.close()


def test_residual_block_form_on_the_same_sequences(built, monkeypatch, capfd):
    """The Float32 residual-block form (tuning float32_dense) shares the panel, update, ladder and solve kernels with this route and
    replays its graph too; its captured sequence has no memset node (dnf_assemble writes every element of S0).  The two sequences
    above on that handle: 256 healthy problems of order 129, three calls with copies between them, then one problem behind two
    later handles — every replay hands back the bits of the capturing call."""
    import torch
    hipldl, syn = _mods()
    from tests.support import f32_dense as FD
    cd = FD.case((129, 70, 0))
    s = cd["s"]
    opt = hipldl.Options(float32_general=1, float32_dense=1)
    monkeypatch.setenv("CNL_VERBOSE", "1")
    for B in (256, 1):
        idx = np.array([0, 4])[np.arange(B) % 2]
        L = hipldl.HIPLDLStruct(s.N, cd["rows"], cd["cols"], None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32, options=opt)
        assert L.config["kernel"] == "dense" and L.config["float32"] and L.info["ncond"] == 0, L.config
        A = GD.Args(s, B)
        A.fill(cd["vals"][idx], cd["rhs"][idx], np.zeros(B, np.float32))
        capfd.readouterr()
        first, others = None, []
        for call in range(3):
            A.call(hipldl, L, cd["p32"])
            out = A.read()
            assert _captured(capfd) == (1 if call == 0 else 0), (B, call)
            assert (out["ok"] == 1).all() and (out["nf"] == 1).all(), (B, call, int(out["ok"].sum()), int(out["nf"].max()))
            if first is None:
                first = out
                for b in range(min(B, 2)):
                    assert G.backward_error(s, cd["vals"][idx[b]], cd["rhs"][idx[b]], out["d"][b]) <= GD.BWD_TOL, (B, b)
            for name in ("vals", "d", "ro", "rho"):
                assert out[name].tobytes() == first[name].tobytes(), (B, call, name)
            _small_copies(A.ok)
            if B == 1 and call == 0:
                c9 = GD.case((129, 150, 0, 0.06, 5))
                s9 = c9["s"]
                for T, o in ((np.float32, GD.BASE), (np.float64, {})):
                    Lo = hipldl.HIPLDLStruct(s9.N, c9["rows"], c9["cols"], None, s9.nvar, s9.nequ, s9.ncon, batch=1, dtype=T, options=hipldl.Options(**o))
                    v, r = c9["vals"][:1].astype(T), c9["rhs"][:1].astype(T)
                    d, ok, *_ = hipldl.newton_system_(np.zeros(s9.N, T), s9.nvar, s9.nequ, s9.ncon, r[0].copy(), v[0].copy(), Lo, T(0), hipldl.default_params(T))
                    assert ok
                    others.append(Lo)
                capfd.readouterr()
        torch.cuda.synchronize()
        for Lo in others:
            Lo.close()
        L.close()
    monkeypatch.delenv("CNL_VERBOSE")


# ---- 5. the batch rule ----
def test_batch_rule(built):
    """order 96 is two tiles per side: S0, S and G take 3 x 16 384 x 4 bytes per problem, so 8e9 bytes hold 40 690 problems.  With
    value 1 the batch above that keeps the float32_condense handle, the batch at the limit takes the route.
    (Memory: the heaviest allocation of the suite for a decision made on the host — the handle at the limit allocates and zero-fills
    8 GB of tiles plus the general kernel's unused factor panels, the one above it the panels alone; both are closed before the next
    is created.  On a shared card it needs that much free.)"""
    hipldl, syn = _mods()
    c = GD.case(GD.SMALLEST)
    limit = int(8e9 // (3 * 16384 * 4))
    assert limit == 40690
    L = GD.handle(hipldl, c, limit + 1)
    assert L.config["kernel"] == "v1" and L.config["float32"] and L.info["ncond"] > 0, L.config
    L.close()
    L = GD.handle(hipldl, c, limit)
    assert GD.on_the_route(L), L.config
    L.close()


# ---- 6. the key changes nothing elsewhere ----
def _same_with_and_without(hipldl, s, vals, rhs, base, kernel):
    rows, cols = s.kkt_pattern()
    B = vals.shape[0]
    p32 = hipldl.default_params(np.float32)
    res = []
    for extra in ({}, dict(float32_general_dense=1)):
        L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32, options=hipldl.Options(**base, **extra))
        out = _host_newton(hipldl, s, L, vals, rhs, np.zeros(B, np.float32), p32)
        res.append((L.config, L.info, out))
        L.close()
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and res[0][0]["kernel"] == kernel, (res[0][0], res[1][0])
    assert res[0][2]["ok"].all()
    for name, a in res[0][2].items():
        b = res[1][2][name]
        assert a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), name


def test_key_changes_nothing_elsewhere(built):
    hipldl, syn = _mods()
    from tests.support import f32_dense as FD
    # a band pattern stays on the band kernels
    sb = syn.band_structure(200, 4)
    _same_with_and_without(hipldl, sb, *G.band_inputs(syn, sb, range(4000, 4008)), GD.BASE, "band")
    # condensed order 64: below what the route takes
    sn = GD.structure(GD.NOT_TAKEN)
    _same_with_and_without(hipldl, sn, *G.random_inputs(syn, sn, range(100, 108)), GD.BASE, "v1")
    # a plan the register-front kernel serves (fronts of the 64 class) stays on it with float32_register_front = 1
    sr = syn.random_structure(60, 80, 4, 0.1, seed=3)
    _same_with_and_without(hipldl, sr, *G.random_inputs(syn, sr, range(100, 108)), dict(GD.BASE, float32_register_front=1), "v2")
    # a dense residual block that float32_dense = 1 took (order 129: in the range of this route); its two healthy problems
    cd = FD.case((129, 70, 0))
    _same_with_and_without(hipldl, cd["s"], cd["vals"][[0, 4]], cd["rhs"][[0, 4]], dict(GD.BASE, float32_dense=1), "dense")
    # value 2: the order-96 pattern takes the route whatever its fronts, also where the register-front kernel is asked for
    c = GD.case(GD.SMALLEST)
    for extra in ({}, dict(float32_register_front=1)):
        L = GD.handle(hipldl, c, GD.MIX, options=dict(float32_general=1, float32_general_dense=2, **extra))
        assert GD.on_the_route(L), L.config
        A = GD.Args(c["s"], GD.MIX)
        A.fill(c["vals"], c["rhs"], c["rho_old"])
        A.call(hipldl, L, c["p32"])
        GD.check_outputs(c, A.read(), np.arange(GD.MIX), c["vals"])
        L.close()


# ---- 7. refusals ----
def test_refusals(built):
    import torch
    hipldl, syn = _mods()
    c = GD.case(GD.SMALLEST)
    s, B = c["s"], GD.MIX
    with pytest.raises(hipldl.CnlError) as e:     # the interleaved layout is the band kernels'
        GD.handle(hipldl, c, B, batch_layout=hipldl.LAYOUT_INTERLEAVED)
    assert e.value.code == CNL_ERR_ARG
    L = _route_handle(hipldl, c, B)
    with pytest.raises(hipldl.CnlError) as e:     # the dense backend is sized by the created batch
        hipldl.set_active_batch(L, 2)
    assert e.value.code == CNL_ERR_STATE
    # a Float64 entry point on the handle
    t64 = torch.zeros((B, s.N), dtype=torch.float64, device="cuda:0")
    t32 = torch.zeros((B,), dtype=torch.int32, device="cuda:0")
    assert hipldl.lib().cnl_solve_dev(L._h, t64.data_ptr(), t64.data_ptr(), 0) == CNL_ERR_STATE
    assert hipldl.lib().cnl_factorize_dev(L._h, t64.data_ptr(), 1e-7, t32.data_ptr(), 0) == CNL_ERR_STATE
    # cnl_solve_f32_dev before a factorisation
    f32 = torch.zeros((B, s.N), dtype=torch.float32, device="cuda:0")
    assert hipldl.lib().cnl_solve_f32_dev(L._h, f32.data_ptr(), f32.data_ptr(), 0) == CNL_ERR_STATE
    # ... none of which left anything behind: the handle serves the call
    A = GD.Args(s, B)
    A.fill(c["vals"], c["rhs"], c["rho_old"])
    A.call(hipldl, L, c["p32"])
    GD.check_outputs(c, A.read(), np.arange(B), c["vals"])
    L.close()


# ---- 8. garbage left by earlier kernels ----
def test_results_do_not_depend_on_what_earlier_kernels_left(built):
    """The two smallest shapes in a child process (tests/support/f32_general_dense.py as a script), once as it is and once with
    kernels in front of every launch that leave a byte pattern in LDS, scratch memory and the vector registers (all ones: a NaN in
    every float, -1 in every counter): the digests of every output are the same in both runs."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for fill in (None, "0xffffffff"):
        env = dict(os.environ)
        if fill:
            env.update(CNL_DBG_SCRATCHFILL="1", CNL_DBG_LDSFILL=fill)
        r = subprocess.run([sys.executable, "-m", "tests.support.f32_general_dense"], env=env, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
        lines = [ln for ln in r.stdout.splitlines() if ln and not ln.startswith("[")]
        assert lines[-1] == "done" and len(lines) == 3, r.stdout[-1500:]
        outs.append(lines)
    assert outs[0] == outs[1], outs
