"""The blocked general kernel (tuning general_blocked: csrc/kernels.hip — fronts with 16 pivots or more leave in panels of 16, the
trailing updates run on the f64 matrix cores) against the CPU oracle.  -m gpu.

Inputs and reference: the seven-kind mix of tests/support/dense_general_cases.py on the shapes of
tests/support/general_blocked_cases.py, the oracle on the canonical order and on the handle's own; tests/test_general_blocked_cpu.py
vouches for the fronts these shapes have and for the oracle's decisions.  Tolerances are those of tests/test_gpu_parity.py: BWD_TOL =
1e-13, FWD_TOL = 1e-9 on problems with nfact 1.  Decisions (ok, nfact, rho, rho_old, the rho slots of vals) are compared bit for bit; a
failed problem keeps its d = 7.0 sentinel."""
import numpy as np
import pytest

from tests.support import dense_general_cases as GC
from tests.support import general_blocked_cases as GB
from tests.test_gpu_parity import BWD_TOL, FWD_TOL, backward_error

pytestmark = pytest.mark.gpu
CNL_ERR_ARG = 1


def _mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    from oracle import oracle as O
    return hipldl, syn, O


def _handle(hipldl, c, B, **opt):
    s = c["s"]
    return hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(**dict(GB.OPTS, **opt)))


def _kinds(shape):
    return range(5) if shape == GB.random_shape(16) else range(GC.MIX)     # (n = 16: kind 5 fails in the oracle too)


def _run_mix(hipldl, c, L, blocked=True, tpp=None, lds=None):
    """one cnl_newton_system_dev call on the case's problems, forwards and reversed, checked on both orders; returns the outputs of
    the forward call"""
    s, B = c["s"], len(c["vals"])
    cfg = L.config
    assert cfg["kernel"] == "v1" and cfg["general_blocked"] == blocked and not cfg["float32"], cfg
    if tpp is not None:
        assert cfg["tpp"] == tpp and cfg["ppb"] == 1, cfg
    if lds is not None:
        assert cfg["lds_work"] == lds, cfg
    refs = [c, GC.oracle_on(L.plan_array("perm").astype(np.int64), c)]
    A = GC.Args(s, B)
    first = None
    for idx in (np.arange(B), np.arange(B)[::-1]):
        A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
        A.call(hipldl, L, hipldl.default_params())
        out = A.read()
        be, fe = GC.check_outputs(out, refs, c, c["rhs"][idx], idx, BWD_TOL, FWD_TOL, backward_error)
        print(f"tpp {cfg['tpp']} lds_work {cfg['lds_work']}: ok {out['ok'].tolist()} nfact {out['nf'].tolist()} backward {be:.2e} forward {fe:.2e}")
        first = first or out
    return first


# ---- 1. the mix against the oracle ----
SMALL = [GB.random_shape(n) for n in GB.RANDOM_N] + [GB.COND0]


@pytest.mark.parametrize("lds", (1, 0), ids=("lds", "global"))
@pytest.mark.parametrize("condense", (1, 0), ids=("condensed", "uncondensed"))
@pytest.mark.parametrize("shape", SMALL, ids=GB.shape_id)
def test_panel_edges(built, shape, condense, lds):
    """one front of n = 16 k - 1, 16 k, 16 k + 1 pivots (condensed) resp. the uncondensed plan's last front with its independent
    leading pivots, 256 threads per problem, work area in LDS and in global scratch"""
    hipldl, syn, O = _mods()
    c = GB.case(shape, kinds=_kinds(shape))
    L = _handle(hipldl, c, len(c["vals"]), v1_tpp=256, v1_lds=lds, condense=condense)
    fr = L.plan_array("fronts").reshape(-1, 16)
    assert fr[:, 0].max() >= GB.PANEL
    if condense:
        assert fr.shape[0] == 1 and fr[0, 0] == c["s"].nvar + c["s"].ncon
    elif shape == GB.COND0:
        assert tuple(fr[-1, [0, 1, 14]]) == (60, 0, 23)
    _run_mix(hipldl, c, L, tpp=256, lds=lds)
    L.close()


@pytest.mark.parametrize("n", (33, 49))
def test_panel_edges_1024_threads(built, n):
    hipldl, syn, O = _mods()
    c = GB.case(GB.random_shape(n))
    L = _handle(hipldl, c, GC.MIX, v1_tpp=1024)
    _run_mix(hipldl, c, L, tpp=1024)
    L.close()


@pytest.mark.parametrize("condense", (1, 0), ids=("condensed", "uncondensed"))
def test_grid(built, condense):
    """grid_structure(32) on the large-batch plan: fronts with update rows — (21, 62), (31, 63), the root (93, 0) — and, uncondensed,
    fronts whose leading pivots are independent, one of them ((16, 13, 11)) blocked"""
    hipldl, syn, O = _mods()
    c = GB.case(GB.GRID)
    L = _handle(hipldl, c, GC.MIX, v1_tpp=256, condense=condense, plan_kind=hipldl.PLAN_THROUGHPUT)
    fr = [tuple(int(x) for x in f[[0, 1, 14]]) for f in L.plan_array("fronts").reshape(-1, 16)]
    for w in [(21, 62, 0), (31, 63, 0), (93, 0, 0)] + ([] if condense else [(16, 13, 11), (15, 27, 9)]):
        assert w in fr, w
    _run_mix(hipldl, c, L, tpp=256)
    L.close()


@pytest.mark.parametrize("shape,lds,tpp", [(GC.SECOND, 1, 256), (GB.F130, 1, 256), (GB.G125, 0, 256), (GB.G450, 0, 256)], ids=lambda v: GB.shape_id(v) if isinstance(v, tuple) else str(v))
def test_default_configurations(built, shape, lds, tpp):
    """the configuration choose_config picks: fmax 97 and 130 with the work area (W panel included) in LDS, 182 KB and the 450
    shape in global scratch"""
    hipldl, syn, O = _mods()
    c = GB.case(shape)
    L = _handle(hipldl, c, GC.MIX)
    print(f"{GB.shape_id(shape)}: fmax {L.info['fmax']} config {L.config}")
    _run_mix(hipldl, c, L, tpp=tpp, lds=lds)
    L.close()


def test_big_1024_threads_default(built):
    """order 800 (fmax 798): 1024 threads per problem by default; kinds 0 and 5"""
    hipldl, syn, O = _mods()
    c = GB.case(GC.BIG, kinds=(0, 5))
    L = _handle(hipldl, c, 2)
    assert L.info["fmax"] == 798
    _run_mix(hipldl, c, L, tpp=1024, lds=0)
    L.close()


# ---- 2. a configuration without a blocked instance ----
def test_smallest_runs_unblocked(built):
    """fmax 96: 64 threads per problem, no blocked instance — the handle is created, says so, and passes the same check"""
    hipldl, syn, O = _mods()
    c = GB.case(GC.SMALLEST)
    L = _handle(hipldl, c, GC.MIX)
    assert L.info["fmax"] == 96 and L.config["tpp"] == 64
    _run_mix(hipldl, c, L, blocked=False)
    L.close()


# ---- 3. the two-call sequence ----
@pytest.mark.parametrize("shape,opt", [(GB.random_shape(33), dict(v1_tpp=256)), (GB.F130, {}), (GB.G450, {})], ids=lambda v: GB.shape_id(v) if isinstance(v, tuple) else "")
def test_two_call_sequence_and_inertia(built, shape, opt):
    """cnl_factorize_dev (the blocked instance), then cnl_solve_dev twice with different right-hand sides on that factor (the plain
    instance's sweeps), vals untouched; then the host try_to_factorize with the inertia, equal to the oracle's counts"""
    import torch
    hipldl, syn, O = _mods()
    c = GB.case(shape)
    s, B = c["s"], GC.MIX
    eig_tol = O.default_params()[0]
    orc = O.Oracle(s.N, c["rows"], c["cols"], O.canonical_perm(s.nvar, s.nequ, s.ncon))
    ref = [orc.try_to_factorize(np.array(c["vals"][b]), s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True) for b in range(B)]
    want = [bool(r[0]) for r in ref]
    assert want == [True, False, False, False, True, True, False]
    L = _handle(hipldl, c, B, **opt)
    assert L.config["general_blocked"] and L.config["kernel"] == "v1", L.config
    dev = "cuda:0"
    t_vals = torch.from_numpy(np.array(c["vals"])).to(dev)
    t_ok = torch.full((B,), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    hipldl.factorize_dev(L, t_vals.data_ptr(), eig_tol, t_ok.data_ptr(), stream=stream)
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
            else:
                assert (d[b] == 7.0).all(), b      # no factor: the rows stay untouched
    assert np.array_equal(GC.bits64(t_vals.cpu().numpy()), GC.bits64(c["vals"]))
    ok, npos, nzer = hipldl.try_to_factorize(L, np.array(c["vals"]), s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True)
    assert list(ok) == want
    for b in range(B):
        if b % GC.MIX != 1:     # (the hopeless problem's pivots are NaN: its counts mean nothing in either arithmetic)
            assert (int(npos[b]), int(nzer[b])) == (int(ref[b][1]), int(ref[b][2])), b
    L.close()


def test_solve_leaves_failed_rows_untouched(built):
    """The two-call sequence at n = 33, condensed and uncondensed: behind cnl_solve_dev the rows of d of a problem whose
    factorisation failed stay at their 7.0 sentinel on a blocked handle — it keeps the success flags of its last factorisation, the
    blocked instance's MODE_SOLVE and the expand pass read them.  With the key off the handle runs what it always ran: the sweeps of
    every problem (all 76 entries of d of each failed problem overwritten); the test prints both counts."""
    import torch
    hipldl, syn, O = _mods()
    c = GB.case(GB.random_shape(33))
    s, B = c["s"], GC.MIX
    dev = "cuda:0"
    stream = torch.cuda.current_stream().cuda_stream
    touched = {}
    for key, condense in ((0, 1), (1, 1), (1, 0)):
        L = _handle(hipldl, c, B, v1_tpp=256, general_blocked=key, condense=condense)
        assert L.config["general_blocked"] == bool(key)
        t_vals = torch.from_numpy(np.array(c["vals"])).to(dev)
        t_ok = torch.full((B,), -1, dtype=torch.int32, device=dev)
        hipldl.factorize_dev(L, t_vals.data_ptr(), O.default_params()[0], t_ok.data_ptr(), stream=stream)
        t_r = torch.from_numpy(np.array(c["rhs"])).to(dev)
        t_d = torch.full((B, s.N), 7.0, dtype=torch.float64, device=dev)
        hipldl.solve_dev(L, t_r.data_ptr(), t_d.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        ok, d = t_ok.cpu().numpy(), t_d.cpu().numpy()
        assert ok.tolist() == [1, 0, 0, 0, 1, 1, 0]
        touched[key, condense] = {b: int((d[b] != 7.0).sum()) for b in range(B) if not ok[b]}
        print(f"general_blocked={key} condense={condense}: entries of d overwritten per failed problem {touched[key, condense]} of {s.N}")
        for b in range(B):
            if ok[b]:
                assert backward_error(s, c["vals"][b], c["rhs"][b], d[b]) <= BWD_TOL, (key, condense, b)
        L.close()
    assert all(n == 0 for k in ((1, 1), (1, 0)) for n in touched[k].values()), touched


# ---- 4. key on against key off ----
@pytest.mark.parametrize("shape,opt", [(GB.random_shape(33), dict(v1_tpp=256)), (GB.COND0, dict(v1_tpp=256, condense=0)), (GB.F130, {})],
                         ids=lambda v: GB.shape_id(v) if isinstance(v, tuple) else "")
def test_key_on_against_key_off(built, shape, opt):
    hipldl, syn, O = _mods()
    c = GB.case(shape)
    s, B = c["s"], GC.MIX
    outs = []
    for key in (1, 0):
        L = _handle(hipldl, c, B, **dict(opt, general_blocked=key))
        assert L.config["general_blocked"] == bool(key) and L.config["kernel"] == "v1" and L.config["tpp"] == 256, L.config
        A = GC.Args(s, B)
        A.fill(c["vals"], c["rhs"], c["rho_old"])
        A.call(hipldl, L, hipldl.default_params())
        outs.append(A.read())
        L.close()
    on, off = outs
    for k in ("ok", "nf"):
        assert np.array_equal(on[k], off[k]), k
    for k in ("rho", "ro"):
        assert np.array_equal(GC.bits64(on[k]), GC.bits64(off[k])), k
    assert np.array_equal(GC.bits64(on["vals"][:, -s.nvar:]), GC.bits64(off["vals"][:, -s.nvar:]))
    worst = 0.0
    for b in range(B):
        if not on["ok"][b]:
            assert (on["d"][b] == 7.0).all() and (off["d"][b] == 7.0).all()
        elif on["nf"][b] == 1:
            fe = np.abs(on["d"][b] - off["d"][b]).max() / np.abs(off["d"][b]).max()
            worst = max(worst, fe)
            assert fe <= FWD_TOL, (b, fe)
    print(f"{GB.shape_id(shape)}: d with the key on against off, worst {worst:.2e}")


# ---- 5. more problems than one mix ----
def test_batch_of_65(built):
    """65 problems (nine mixes and two), one workgroup each"""
    hipldl, syn, O = _mods()
    c = GB.case(GB.random_shape(33), B=65)
    L = _handle(hipldl, c, 65, v1_tpp=256)
    assert L.config["grid"] == 65
    out = _run_mix(hipldl, c, L, tpp=256)
    assert out["ok"].tolist() == [int(GC.WANT_OK[b % GC.MIX]) for b in range(65)]
    L.close()


def test_sub_batch_slices(built):
    """The host-pointer cnl_newton_system cuts a batch of 96 MB and more of input into chunks of at least 16 MB, each a view of the
    handle at its own offset into the factor panels and the global work area (which the key enlarged): the mix at n = 33 repeated
    to that size, work area in global scratch.  The first mix against the oracle; every repetition bit-equal to the first."""
    hipldl, syn, O = _mods()
    c = GB.case(GB.random_shape(33))
    s = c["s"]
    per = (s.nnzNS + s.N) * 8
    reps = -(-(96 << 20) // (GC.MIX * per))
    B = GC.MIX * reps
    assert B >= 32 and B * per >= (96 << 20) and max(16, ((B // 8) + 3) & ~3) < B       # the rule of cnl_newton_system
    L = _handle(hipldl, c, B, v1_tpp=256, v1_ppb=1, v1_lds=0)     # (a batch this large gets several problems per workgroup by default)
    assert L.config["general_blocked"] and L.config["kernel"] == "v1" and not L.config["lds_work"], {k: L.config[k] for k in ("general_blocked", "kernel", "tpp", "ppb", "lds_work")}
    vals, rhs, ro = (np.ascontiguousarray(np.tile(c[k], (reps,) + (1,) * (c[k].ndim - 1))) for k in ("vals", "rhs", "rho_old"))
    before = hipldl.launch_counts()["general"]
    d, ok, rho, ro_out, nf = hipldl.newton_system_(np.full((B, s.N), 7.0), s.nvar, s.nequ, s.ncon, rhs, vals, L, ro, hipldl.default_params())
    chunk = max(16, ((B // 8) + 3) & ~3)
    while chunk * per < (16 << 20):
        chunk += 4
    assert hipldl.launch_counts()["general"] - before >= -(-B // chunk) >= 6       # one launch per chunk at least
    out = dict(vals=vals, d=d, ok=np.asarray(ok).astype(np.int32), rho=rho, ro=ro_out, nf=np.asarray(nf))
    first = {k: v[:GC.MIX] for k, v in out.items()}
    refs = [c, GC.oracle_on(L.plan_array("perm").astype(np.int64), c)]
    GC.check_outputs(first, refs, c, c["rhs"], np.arange(GC.MIX), BWD_TOL, FWD_TOL, backward_error)
    for k, v in out.items():
        rep = v.reshape((reps, GC.MIX) + v.shape[1:])
        assert np.array_equal(rep, np.broadcast_to(rep[:1], rep.shape), equal_nan=True), k
    L.close()


# ---- 6. refusals ----
def test_float32_creators_refuse_the_key(built):
    hipldl, syn, O = _mods()
    c = GB.case(GB.random_shape(33))
    s = c["s"]
    for dtype, opt in ((np.float32, dict(float32_general=1, general_blocked=1)),
                       (np.float64, dict(float32_general=1, float32_refine=1, general_blocked=1))):
        with pytest.raises(hipldl.CnlError) as e:
            hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=GC.MIX, dtype=dtype, options=hipldl.Options(**opt))
        assert e.value.code == CNL_ERR_ARG and "general_blocked" in str(e.value), str(e.value)
    # ... and without the key both are made
    for dtype, opt in ((np.float32, dict(float32_general=1)), (np.float64, dict(float32_general=1, float32_refine=1))):
        hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=GC.MIX, dtype=dtype, options=hipldl.Options(**opt)).close()
