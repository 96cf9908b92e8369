"""The general form of the dense backend in double (Route::GeneralDense: what a default Float64 handle on an irregular pattern with a
front above order 64 and condensed order 96 .. 4096 runs — csrc/dense.hip: dense_enqueue_general) against the CPU oracle, on the
edges its Float32 twin is tested on (tests/test_float32_general_dense_gpu.py), and a positive residual pivot on every route that
counts residual pivots outside its factor.  -m gpu.

Inputs and reference are those of tests/support/dense_general_cases.py: a seven-kind mix per shape (healthy, hopeless, two climbers,
a positive residual pivot that the call needs to succeed, and one with which no rho can succeed), the oracle with its own default
params on the canonical order and on the handle's own.  tests/test_dense_general_cpu.py vouches for every input — pivots above the
noise at every rung, and for the positive-pivot kinds every decision determined by eigenvalues — so no problem is skipped or
reclassified here.  Tolerances are those of tests/test_gpu_parity.py: BWD_TOL = 1e-13, FWD_TOL = 1e-9 on problems with nfact 1.

Decisions (ok, nfact, rho, rho_old, the rho slots of vals) are compared bit for bit; a failed problem keeps its d = 7.0 sentinel."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests.support import dense_general_cases as GC
from tests.support import f32_general_dense as GD32
from tests.test_gpu_parity import BWD_TOL, FWD_TOL, backward_error

pytestmark = pytest.mark.gpu

ORDER_129 = (129, 150, 0, 0.06, 5)


def _mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    from oracle import oracle as O
    return hipldl, syn, O


def _handle(hipldl, c, B, dtype=np.float64, **opt):
    s = c["s"]
    return hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B, dtype=dtype,
                               options=hipldl.Options(**opt) if opt else None)


def _route_handle(hipldl, c, B, **opt):
    L = _handle(hipldl, c, B, **opt)
    assert L.config["kernel"] == "dense" and L.info["ncond"] > 0 and not L.config["float32"] and not L.config["band"], L.config
    return L


def _refs(L, c):
    """the oracle's results on the canonical order and on the handle's own"""
    return [c, GC.oracle_on(L.plan_array("perm").astype(np.int64), c)]


def _check(out, refs, c, rhs, idx):
    return GC.check_outputs(out, refs, c, rhs, idx, BWD_TOL, FWD_TOL, backward_error)


def _captured(capfd):
    """n where the call just made captured its sequence as the handle's n-th cached graph (the line csrc/dense_impl.h prints under
    CNL_VERBOSE), 0 where it replayed a cached graph or ran plain launches"""
    err = capfd.readouterr().err
    return next((n for n in range(1, 10) if f"captured as a graph ({n} cached)" in err), 0)


def _host_newton(hipldl, s, L, vals, rhs, ro, p):
    B = vals.shape[0]
    v = np.array(vals)
    d, ok, rho, ro_out, nf = hipldl.newton_system_(np.full((B, s.N), 7.0, vals.dtype), s.nvar, s.nequ, s.ncon, np.array(rhs), v, L, np.array(ro), p)
    return dict(vals=v, d=d, ok=np.asarray(ok).astype(np.int32), rho=rho, ro=ro_out, nf=np.asarray(nf))


# ---- 1. device entry, every shape, both panel kernels ----
# dense_panel_blocks = 0: dn_panel; 1 (the default): dn_panel2 while batch x tiles <= 512, which holds at every shape (7 x 13 = 91 at
# order 800, which runs with that value alone)
@pytest.mark.parametrize("shape,panel_blocks", [(sh, pb) for sh in GC.SHAPES for pb in (0, 1) if sh != GC.BIG or pb == 1],
                         ids=lambda v: GC.shape_id(v) if isinstance(v, tuple) else f"panel{v}")
def test_shapes_and_panel_kernels(built, shape, panel_blocks):
    """cnl_newton_system_dev at every shape of the table (order 800: more condensed slots than one trip of dn_scatter_general's
    grid-stride loop covers).  The second call, batch reversed, finds nothing stale from the first (pivot counters, the counts
    handed over by dn_set_counts, ladder state, S and G); cnl_solve_dev then uses the factor and the rho the ladder ended on."""
    import torch
    hipldl, syn, O = _mods()
    c = GC.case(shape)
    s, B = c["s"], GC.MIX
    L = _route_handle(hipldl, c, B, dense_panel_blocks=panel_blocks)
    assert 7 * -(-(s.nvar + s.ncon) // 64) <= 512
    refs = _refs(L, c)
    p = hipldl.default_params()
    A = GC.Args(s, B)
    for idx in (np.arange(B), np.arange(B)[::-1]):
        A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
        A.call(hipldl, L, p)
        out = A.read()
        print(f"{GC.shape_id(shape)} panel_blocks {panel_blocks}: ok {out['ok'].tolist()} nfact {out['nf'].tolist()}")
        be, fe = _check(out, refs, c, c["rhs"][idx], idx)
        print(f"{GC.shape_id(shape)} panel_blocks {panel_blocks}: backward error {be:.2e}, forward error {fe:.2e} = {fe / FWD_TOL:.3f} FWD_TOL")
    rhs2 = np.random.default_rng(5).standard_normal((B, s.N))
    t_rhs2 = torch.from_numpy(rhs2).to("cuda:0")
    t_x = torch.zeros_like(t_rhs2)
    hipldl.solve_dev(L, t_rhs2, t_x, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    x = t_x.cpu().numpy()
    for k, b in enumerate(idx):
        if c["ok"][b]:
            be = backward_error(s, out["vals"][k], rhs2[k], x[k])
            assert be <= BWD_TOL, (b, be)
    L.close()


# ---- 2. the two-call sequence ----
@pytest.mark.parametrize("shape", list(GC.SHAPES), ids=GC.shape_id)
def test_two_call_sequence_and_inertia(built, shape):
    """cnl_factorize_dev, then cnl_solve_dev twice with different right-hand sides on the one factor, vals untouched; then the host
    try_to_factorize with the inertia: npos and nzero are the sum of what the dense factor counts and what cond_inertia_kernel
    counts outside it (dn_set_counts hands it over, dn_decide adds it).  Success and counts as the oracle's for every kind but the
    hopeless one; for the positive-pivot kinds also as numpy's eigenvalues of K state them (kind 5: (nvar, 0))."""
    import torch
    hipldl, syn, O = _mods()
    c = GC.case(shape)
    s, B = c["s"], GC.MIX
    eig_tol = O.default_params()[0]
    orc = O.Oracle(s.N, c["rows"], c["cols"], O.canonical_perm(s.nvar, s.nequ, s.ncon))
    ref = [orc.try_to_factorize(np.array(c["vals"][b]), s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True) for b in range(B)]
    want = [bool(r[0]) for r in ref]
    assert want == [True, False, False, False, True, True, False]
    L = _route_handle(hipldl, c, B)
    dev = "cuda:0"
    t_vals = torch.from_numpy(np.array(c["vals"])).to(dev)
    t_ok = torch.full((B,), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    hipldl.factorize_dev(L, t_vals.data_ptr(), hipldl.default_params()[0], t_ok.data_ptr(), stream=stream)
    for k in range(2):
        r = np.ascontiguousarray(c["rhs"] * (k + 1.5))
        t_r = torch.from_numpy(r).to(dev)
        t_d = torch.full((B, s.N), 7.0, dtype=torch.float64, device=dev)
        hipldl.solve_dev(L, t_r.data_ptr(), t_d.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        assert t_ok.cpu().numpy().tolist() == [int(w) for w in want]
        d = t_d.cpu().numpy()
        for b in range(B):
            if want[b]:
                be = backward_error(s, c["vals"][b], r[b], d[b])
                assert be <= BWD_TOL, (b, k, be)
    assert np.array_equal(GC.bits64(t_vals.cpu().numpy()), GC.bits64(c["vals"]))      # try_to_factorize and solve_ldl! leave vals alone
    ok, npos, nzer = hipldl.try_to_factorize(L, np.array(c["vals"]), s.nvar, s.nequ, s.ncon, hipldl.default_params()[0], return_inertia=True)
    print(f"{GC.shape_id(shape)}: npos {list(npos)} nzero {list(nzer)}; oracle {[(int(r[1]), int(r[2])) for r in ref]}")
    assert list(ok) == want
    for b in range(B):
        if b % GC.MIX != 1:     # (the hopeless problem's pivots are NaN: it fails, and its counts mean nothing in either arithmetic)
            assert (int(npos[b]), int(nzer[b])) == (int(ref[b][1]), int(ref[b][2])), b
        if b % GC.MIX in (5, 6):
            assert (int(npos[b]), int(nzer[b])) == GC.numpy_inertia(c, b)[:2], b
    assert (int(npos[5]), int(nzer[5])) == (s.nvar, 0)
    L.close()


# ---- 3. host-pointer call = device call ----
@pytest.mark.parametrize("shape", [GC.SECOND, ORDER_129], ids=GC.shape_id)
def test_host_entry_equals_dev_entry(built, shape):
    hipldl, syn, O = _mods()
    c = GC.case(shape)
    s, B = c["s"], GC.MIX
    p = hipldl.default_params()
    L = _route_handle(hipldl, c, B)
    A = GC.Args(s, B)
    A.fill(c["vals"], c["rhs"], c["rho_old"])
    A.call(hipldl, L, p)
    dev = A.read()
    _check(dev, _refs(L, c), c, c["rhs"], np.arange(B))
    host = _host_newton(hipldl, s, L, c["vals"], c["rhs"], c["rho_old"], p)
    L.close()
    assert np.array_equal(host["ok"], dev["ok"]) and np.array_equal(host["nf"], dev["nf"])
    for name in ("rho", "ro", "vals", "d"):     # bit for bit, the untouched rows of the failed problems included
        assert np.array_equal(GC.bits64(host[name]), GC.bits64(dev[name])), name


# ---- 4. graph replay ----
def test_graph_replay(built, monkeypatch, capfd):
    """The captured sequence of the general form (GraphKey mode 16 + mode; S0 zeroed by a kernel, not by a memset node).  One argument
    set called twice (capture, then replay), a second set of pointers with another right-hand side, the first set again with another
    rho0 in params, and the second set again (replay): every output bit-equal to what a handle without graphs returns for the same
    call, so a replay of a stale graph — old pointers, old params — shows.  Two mixes (B = 14).  The states of the cache are read off
    the CNL_VERBOSE line of csrc/dense_impl.h, as tests/test_dense_gpu.py::test_dense_graph_cache_states does: calls 0, 2 and 3
    capture graphs 1, 2 and 3, calls 1 and 4 replay; the handle with dense_graph = 0 never captures."""
    hipldl, syn, O = _mods()
    B = 2 * GC.MIX
    c = GC.case(GC.SMALLEST, B)
    s = c["s"]
    p = hipldl.default_params()
    p2 = p.copy()
    p2[5] *= 3.0
    rhs2 = np.ascontiguousarray(c["rhs"] * 1.25)
    calls = [(0, c["rhs"], p), (0, c["rhs"], p), (1, rhs2, p), (0, c["rhs"], p2), (1, rhs2, p)]
    outs, seen = {}, {}
    monkeypatch.setenv("CNL_VERBOSE", "1")
    for graph in (0, 1):
        L = _route_handle(hipldl, c, B, dense_graph=graph)
        refs = _refs(L, c)
        sets = [GC.Args(s, B), GC.Args(s, B)]
        assert sets[0].vals.data_ptr() != sets[1].vals.data_ptr()
        outs[graph], seen[graph] = [], []
        capfd.readouterr()
        for k, rhs, pk in calls:
            sets[k].fill(c["vals"], rhs, c["rho_old"])
            sets[k].call(hipldl, L, pk)
            outs[graph].append(sets[k].read())
            seen[graph].append(_captured(capfd))
        L.close()
    monkeypatch.delenv("CNL_VERBOSE")
    assert seen[0] == [0, 0, 0, 0, 0] and seen[1] == [1, 0, 2, 3, 0], seen
    _check(outs[0][0], refs, c, c["rhs"], np.arange(B))
    for name in ("vals", "d", "ro", "rho", "nf", "ok"):
        for call in range(len(calls)):
            assert outs[1][call][name].tobytes() == outs[0][call][name].tobytes(), (name, call)
        assert outs[1][1][name].tobytes() == outs[1][0][name].tobytes(), name
        assert outs[1][4][name].tobytes() == outs[1][2][name].tobytes(), name
    climbers = np.arange(B) % GC.MIX == 2      # rho_old = 0: the ladder starts at rho0
    assert (outs[1][3]["rho"][climbers] != outs[1][0]["rho"][climbers]).all()      # the changed params were honoured
    healthy = np.arange(B) % GC.MIX == 0
    assert not np.array_equal(outs[1][2]["d"][healthy], outs[1][0]["d"][healthy])  # ... and so were the changed pointers


def _small_copies(t, n=16):
    """a burst of small device-to-host copies between two calls: host-side traffic of the kind that stood between a capture and the
    replay that went wrong"""
    for _ in range(n):
        t[:1].cpu()


def test_repeated_calls_at_256_problems(built, monkeypatch, capfd):
    """The sequence on which a replayed graph of the Float32 form answered failure for every problem while S0 was zeroed by a captured
    hipMemsetAsync (dense_enqueue_general zeroes S0 with dn::zero_async since): 256 healthy problems of order
    129, one argument set, four calls with device-to-host copies between them.  The first call captures, the others replay; every
    call decides as the oracle does for the eight problems the batch repeats, and hands back the same bits as the first."""
    hipldl, syn, O = _mods()
    B = 256
    c8 = GC.healthy_case(ORDER_129)
    s, nbase = c8["s"], len(c8["vals"])
    assert c8["ok"].all() and (c8["nf"] == 1).all() and nbase == 8
    idx = np.arange(B) % nbase
    p = hipldl.default_params()
    L = _route_handle(hipldl, c8, B)
    A = GC.Args(s, B)
    A.fill(c8["vals"][idx], c8["rhs"][idx], np.zeros(B))
    first = None
    monkeypatch.setenv("CNL_VERBOSE", "1")
    capfd.readouterr()
    for call in range(4):
        A.call(hipldl, L, p)
        out = A.read()
        assert _captured(capfd) == (1 if call == 0 else 0), call
        _small_copies(A.ok)
        assert (out["ok"] == 1).all() and (out["nf"] == 1).all(), (call, int(out["ok"].sum()), int(out["nf"].max()))
        if first is None:
            first = out
            _check({k: v[:nbase] for k, v in out.items()}, [c8], c8, c8["rhs"], np.arange(nbase))
        for name in ("vals", "d", "ro", "rho"):
            assert out[name].tobytes() == first[name].tobytes(), (call, name)
    monkeypatch.delenv("CNL_VERBOSE")
    L.close()


def test_calls_behind_later_handles(built, monkeypatch, capfd):
    """... and the other one: one problem of order 129, a first call (capture), then a float32_condense handle and a Float32
    general-dense handle created and called — their creation is a long row of hipMemset and hipMemcpy calls —, then the first handle
    again, twice (replays)."""
    import torch
    hipldl, syn, O = _mods()
    c = GC.subcase(GC.case(ORDER_129), [0])
    s = c["s"]
    p = hipldl.default_params()
    L = _route_handle(hipldl, c, 1)
    refs = _refs(L, c)
    A = GC.Args(s, 1)
    A.fill(c["vals"], c["rhs"], c["rho_old"])
    monkeypatch.setenv("CNL_VERBOSE", "1")
    capfd.readouterr()
    A.call(hipldl, L, p)
    first = A.read()
    assert _captured(capfd) == 1
    _check(first, refs, c, c["rhs"], np.arange(1))
    others = []
    v32, r32 = c["vals"][0].astype(np.float32), c["rhs"][0].astype(np.float32)
    for opt in (GD32.BASE, GD32.OPTIONS):
        Lo = _handle(hipldl, c, 1, dtype=np.float32, **opt)
        assert Lo.config["float32"] and Lo.info["ncond"] > 0 and Lo.config["kernel"] == ("dense" if opt is GD32.OPTIONS else "v1"), Lo.config
        d, ok, *_ = hipldl.newton_system_(np.zeros(s.N, np.float32), s.nvar, s.nequ, s.ncon, r32.copy(), v32.copy(), Lo, np.float32(0),
                                          hipldl.default_params(np.float32))
        assert ok
        others.append(Lo)
    capfd.readouterr()     # (the Float32 general-dense handle captured a graph of its own)
    for call in range(2):
        A.fill(c["vals"], c["rhs"], c["rho_old"])
        A.call(hipldl, L, p)
        out = A.read()
        assert _captured(capfd) == 0, call     # the graph of the first call, replayed
        for name in ("vals", "d", "ro", "rho", "nf", "ok"):
            assert out[name].tobytes() == first[name].tobytes(), (call, name)
    monkeypatch.delenv("CNL_VERBOSE")
    torch.cuda.synchronize()
    for Lo in others:
        Lo.close()
    L.close()


# ---- 5. the batch rule ----
def test_batch_rule(built):
    """order 96 is two tiles per side: S0, S and G take 3 x 32 768 x 4 bytes per problem, so 8e9 bytes hold 20 345 problems.  The
    batch above that keeps the general kernel on the condensed system, the batch at the limit takes the route.
    (Memory: a decision made on the host, and as heavy as its Float32 twin — the handle at the limit allocates and zero-fills 8 GB
    of tiles plus the general kernel's unused factor panels, the one above it the panels alone; both are closed before the next is
    created.  On a shared card it needs that much free.)"""
    hipldl, syn, O = _mods()
    c = GC.case(GC.SMALLEST)
    limit = int(8e9 // (3 * 32768 * 4))
    assert limit == 20345
    L = _handle(hipldl, c, limit + 1)
    assert L.config["kernel"] == "v1" and not L.config["float32"] and L.info["ncond"] > 0, L.config
    L.close()
    L = _handle(hipldl, c, limit)
    assert GC.on_the_route(L), L.config
    L.close()


# ---- 6. prefer_dense: 16 / 17 ----
@pytest.mark.parametrize("B", [16, 17])
def test_prefer_dense_takes_small_batches_only(built, B):
    """A latency plan with a front of the 64 class on a condensed system of order 137 (tests/test_dense_general_cpu.py states the
    plan facts): up to 16 problems run as one dense LDL', 17 on the register-front kernel.  Kinds 0, 2 and 5 repeated over the batch,
    either handle against the oracle."""
    hipldl, syn, O = _mods()
    c = GC.prefer_case()
    s = c["s"]
    L = _handle(hipldl, c, B)
    if B <= 16:
        assert GC.on_the_route(L), L.config
    else:
        assert L.config["kernel"] in ("v2", "v2-staged") and not L.config["float32"] and L.info["ncond"] > 0, L.config
    idx = np.arange(B) % len(c["vals"])
    A = GC.Args(s, B)
    A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
    A.call(hipldl, L, hipldl.default_params())
    out = A.read()
    print(f"B {B}: kernel {L.config['kernel']}, ok {out['ok'].tolist()} nfact {out['nf'].tolist()}")
    _check(out, _refs(L, c), c, c["rhs"][idx], idx)
    L.close()


# ---- 7. positive residual pivots on every route that counts them outside the factor ----
def _on_route(route, L):
    cfg, info = L.config, L.info
    f32 = cfg["float32"]
    return {
        "general-dense": cfg["kernel"] == "dense" and info["ncond"] > 0 and not f32,
        "condensed-general-kernel": cfg["kernel"] == "v1" and info["ncond"] > 0 and not f32,
        "register-front-direct": cfg["kernel"] in ("v2", "v2-staged") and cfg["direct"] and not f32 and not cfg["band"],
        "v2-staged": cfg["kernel"] == "v2-staged" and not f32 and not cfg["band"],
        # (a Float64 plan states the condensed residual rows on this route too; order 65 is below what the general form takes)
        "dense-residual-block": cfg["kernel"] == "dense" and info["N"] - info["ncond"] == 65 and not f32,
        "band": cfg["band"] and not f32,
        "float32-condense": cfg["kernel"] == "v1" and info["ncond"] > 0 and f32,
        "float32-general-dense": cfg["kernel"] == "dense" and info["ncond"] > 0 and f32,
        "float32-dense": cfg["kernel"] == "dense" and info["ncond"] == 0 and f32,
    }[route]


@pytest.mark.parametrize("route", list(GC.ROUTES))
def test_positive_residual_pivot_on_every_route(built, route):
    """B = 3: a healthy problem, one whose condensed matrix has nvar - 1 positive eigenvalues and ONE positive residual pivot (the
    call succeeds at once only where that pivot is counted), and one that no rho repairs for the same reason (a route that forgets
    the count behind the first rung answers success near the sixth).  Host newton_system! and try_to_factorize with the inertia,
    against the oracle (Float32: on the widened data with ParamCaNNOLeS(Float32) widened, tolerances of tests/support/f32_general.py)
    and, for the counts of the two problems with the positive pivot, numpy's eigenvalues."""
    hipldl, syn, O = _mods()
    T, opt, pattern = GC.ROUTES[route]
    f32 = np.dtype(T) == np.float32
    c = GC.route_case(pattern, T)
    s, B = c["s"], len(c["vals"])
    L = _handle(hipldl, c, B, dtype=T, **opt)
    print(f"{route}: config {L.config}")
    assert _on_route(route, L), (route, L.config, L.info)
    p = hipldl.default_params(T)
    assert np.array_equal(np.asarray(p, np.float64), np.asarray(c["params"], np.float64))
    out = _host_newton(hipldl, s, L, c["vals"], c["rhs"], c["rho_old"], p)
    print(f"{route}: ok {out['ok'].tolist()} nfact {out['nf'].tolist()} rho {out['rho'].tolist()}")
    if f32:
        GD32.check_outputs(c, out, np.arange(B), c["vals"])
    else:
        _check(out, _refs(L, c), c, c["rhs"], np.arange(B))
    orc = O.Oracle(s.N, c["rows"], c["cols"], O.canonical_perm(s.nvar, s.nequ, s.ncon))
    eig_tol = float(p[0])
    ref = [orc.try_to_factorize(np.array(c["vals"][b], np.float64), s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True) for b in range(B)]
    ok, npos, nzer = hipldl.try_to_factorize(L, np.array(c["vals"]), s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True)
    print(f"{route}: npos {list(npos)} nzero {list(nzer)}; oracle {[(int(r[1]), int(r[2])) for r in ref]}")
    assert list(ok) == [bool(r[0]) for r in ref] == [True, True, False]
    margin = GC.EIG_MARGIN32 if f32 else GC.EIG_MARGIN
    for b in range(B):
        assert (int(npos[b]), int(nzer[b])) == (int(ref[b][1]), int(ref[b][2])), b
        if b > 0:
            assert (int(npos[b]), int(nzer[b])) == GC.numpy_inertia(c, b, margin)[:2], b
    assert (int(npos[1]), int(nzer[1])) == (s.nvar, 0)
    L.close()


# ---- 8. garbage left by earlier kernels ----
def test_results_do_not_depend_on_what_earlier_kernels_left(built):
    """The two smallest shapes in a child process (tests/support/dense_general_cases.py as a script), once as it is and once with
    kernels in front of every launch that leave a byte pattern in LDS, scratch memory and the vector registers (all ones: a NaN in
    every double, -1 in every counter): the digests of every output are the same in both runs.  (A child's time is the start of the
    interpreter and of the runtime: the script itself runs for 0.1 s.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for fill in (None, "0xffffffff"):
        env = dict(os.environ)
        if fill:
            env.update(CNL_DBG_SCRATCHFILL="1", CNL_DBG_LDSFILL=fill)
        t0 = time.time()
        r = subprocess.run([sys.executable, "-m", "tests.support.dense_general_cases"], env=env, cwd=root, capture_output=True, text=True, timeout=300)
        print(f"child with fill {fill}: {time.time() - t0:.1f} s")
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
        lines = [ln for ln in r.stdout.splitlines() if ln and not ln.startswith("[")]
        assert lines[-1] == "done" and len(lines) == 3, r.stdout[-1500:]
        outs.append(lines)
    assert outs[0] == outs[1], outs
