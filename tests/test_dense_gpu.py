"""Dense backend (csrc/dense.hip) on the edges of its tiles, through the entries no other deterministic test takes.  -m gpu.

  * cnl_newton_system_dev on a residual-block handle: the on-device rho ladder (dn_ladder), the gated solve kernels and the
    scalars dn_out writes from the ladder's state — at every shape of tests/support/dense_cases.py, with both panel kernels;
  * the two-call sequence and its inertia counts (pad rows of the last tile are no pivots);
  * the panel kernel a large batch picks by itself;
  * the hipGraph cache of a handle: capture, replay, the miss limit, a hit behind it, eviction;
  * the general form at an order that takes the ladder's second pass over the row tiles.

The inputs are vouched for by tests/test_dense_cases_cpu.py (every decision far above the rounding noise): no problem is skipped
or reclassified here.  Tolerances are those of tests/test_gpu_parity.py."""
import numpy as np
import pytest

from tests.support import dense_cases as dc
from tests.test_gpu_parity import BWD_TOL, FWD_TOL, _mods, backward_error, run_case

pytestmark = pytest.mark.gpu

_own = {}


def _oracle_on(perm, shape, c):
    """the oracle's results for the case on the elimination order `perm` (the handle's), once per (shape, order)"""
    key = (shape, len(c["vals"]), perm.tobytes())
    if key not in _own:
        from oracle import oracle as O
        s = c["s"]
        B = len(c["vals"])
        orc = O.Oracle(s.N, c["rows"], c["cols"], perm)
        v = c["vals"].copy()
        d, ok, rho, ro, nf = O.newton_system_batch(orc, B, s.nvar, s.nequ, s.ncon, c["rhs"], v, c["rho_old"], O.default_params())
        _own[key] = dict(d=d, ok=ok, rho=rho, ro=ro, nf=nf, vals_after=v)
    return _own[key]


class _Args:
    """one argument set of cnl_newton_system_dev on the device"""

    def __init__(self, s, B):
        import torch
        dev = torch.device("cuda:0")
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        self.vals, self.rhs, self.d = torch.zeros((B, s.nnzNS), **f64), torch.zeros((B, s.N), **f64), torch.zeros((B, s.N), **f64)
        self.ro, self.rho = torch.zeros(B, **f64), torch.zeros(B, **f64)
        self.nf, self.ok = torch.zeros(B, **i32), torch.zeros(B, **i32)

    def fill(self, vals, rhs, ro):
        import torch
        self.vals.copy_(torch.from_numpy(np.array(vals)))   # (copies: the shared cases are read-only)
        self.rhs.copy_(torch.from_numpy(np.array(rhs)))
        self.ro.copy_(torch.from_numpy(np.array(ro)))
        self.d.fill_(7.0)
        self.rho.fill_(-1.0)
        self.nf.fill_(-1)
        self.ok.fill_(-1)
        torch.cuda.synchronize()

    def call(self, hipldl, L, p):
        import torch
        hipldl.newton_system_dev(L, self.vals.data_ptr(), self.rhs.data_ptr(), self.d.data_ptr(), self.ro.data_ptr(), self.rho.data_ptr(),
                                 self.nf.data_ptr(), self.ok.data_ptr(), p, stream=torch.cuda.current_stream().cuda_stream)

    def read(self):
        import torch
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("vals", "d", "ro", "rho", "nf", "ok")}


def _check_dev_outputs(out, refs, s, rhs, idx):
    """one call's outputs against the oracle's on every order of `refs`, for the problems `idx` of the case"""
    for ref in refs:
        ok0, nf0 = ref["ok"][idx], ref["nf"][idx]
        assert np.array_equal(out["ok"], ok0.astype(np.int32))
        assert np.array_equal(out["nf"], nf0)
        assert np.array_equal(out["rho"], ref["rho"][idx]) and np.array_equal(out["ro"], ref["ro"][idx])
        assert np.array_equal(out["vals"], ref["vals_after"][idx], equal_nan=True)    # only the rho slots change, as the reference leaves them
        for b in range(len(idx)):
            d, d0 = out["d"][b], ref["d"][idx[b]]
            if not ok0[b]:
                assert (d == 7.0).all()
            elif nf0[b] == 1:
                assert np.abs(d - d0).max() <= FWD_TOL * np.abs(d0).max()
    for b in range(len(idx)):   # (the decisions are those of every order by now)
        if out["ok"][b]:
            assert backward_error(s, out["vals"][b], rhs[b], out["d"][b]) <= BWD_TOL


def _solve_dev_check(hipldl, L, s, vals_left, ok0, seed):
    """cnl_solve_dev with a fresh rhs uses the factorisation (and the rho) the ladder ended on"""
    import torch
    B = len(ok0)
    rhs2 = np.random.default_rng(seed).standard_normal((B, s.N))
    t_rhs2 = torch.from_numpy(rhs2).to("cuda:0")
    t_x = torch.zeros_like(t_rhs2)
    hipldl.solve_dev(L, t_rhs2, t_x, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    x = t_x.cpu().numpy()
    for b in range(B):
        if ok0[b]:
            assert backward_error(s, vals_left[b], rhs2[b], x[b]) <= BWD_TOL


@pytest.mark.parametrize("panel_blocks", [0, 2])
@pytest.mark.parametrize("shape", dc.SHAPES, ids=dc.shape_id)
def test_dense_dev_entry_against_the_oracle(built, shape, panel_blocks):
    """cnl_newton_system_dev on a residual-block dense handle: decisions, rho slots and scalars as the oracle's on two orders, d
    untouched for the problem no rho repairs; a second call with the batch reversed finds nothing stale from the first (pivot
    counters, ladder state, S and G); cnl_solve_dev then solves with what the ladder left."""
    hipldl, syn, O = _mods()
    c = dc.oracle_case(shape)
    s, B = c["s"], dc.MIX
    L = hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(dense_panel_blocks=panel_blocks))
    assert L.config["kernel"] == "dense"
    refs = [c, _oracle_on(L.plan_array("perm").astype(np.int64), shape, c)]
    if shape != dc.TALL:
        assert c["nf"].max() == 20 and sorted(c["nf"])[-2] >= 3
    p = hipldl.default_params()
    A = _Args(s, B)
    for idx in (np.arange(B), np.arange(B)[::-1]):
        A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
        A.call(hipldl, L, p)
        out = A.read()
        _check_dev_outputs(out, refs, s, c["rhs"][idx], idx)
    _solve_dev_check(hipldl, L, s, out["vals"], c["ok"][idx], seed=5)
    L.close()


@pytest.mark.parametrize("shape", [(129, 70, 0), (126, 150, 4), (470, 64, 3)], ids=dc.shape_id)
def test_dense_host_entry_device_ladder_equals_dev_entry(built, shape):
    """The host-pointer call with cnl_options.host_ladder = 0 is the device entry behind an upload: the same outputs bit for bit.
    The default host-pointer call (the ladder driven from the host, a multi-kernel factorisation per rung) decides the same."""
    hipldl, syn, O = _mods()
    c = dc.oracle_case(shape)
    s, B = c["s"], dc.MIX
    p = hipldl.default_params()
    L = hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B)
    assert L.config["kernel"] == "dense"
    A = _Args(s, B)
    A.fill(c["vals"], c["rhs"], c["rho_old"])
    A.call(hipldl, L, p)
    dev = A.read()
    assert np.array_equal(dev["ok"], c["ok"].astype(np.int32)) and np.array_equal(dev["nf"], c["nf"])

    def host_call(handle):
        v, d = c["vals"].copy(), np.full((B, s.N), 7.0)
        _, ok, rho, ro, nf = hipldl.newton_system_(d, s.nvar, s.nequ, s.ncon, c["rhs"].copy(), v, handle, c["rho_old"].copy(), p)
        return dict(vals=v, d=d, ok=ok, rho=rho, ro=ro, nf=nf)

    L0 = hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(host_ladder=0))
    h0 = host_call(L0)
    L0.close()
    assert np.array_equal(h0["ok"], dev["ok"].astype(bool)) and np.array_equal(h0["nf"], dev["nf"])
    assert np.array_equal(h0["rho"], dev["rho"]) and np.array_equal(h0["ro"], dev["ro"])
    assert np.array_equal(h0["vals"], dev["vals"], equal_nan=True)
    assert np.array_equal(h0["d"], dev["d"])                     # bit for bit, the untouched rows of the hopeless problem included
    h1 = host_call(L)
    L.close()
    assert np.array_equal(h1["ok"], dev["ok"].astype(bool)) and np.array_equal(h1["nf"], dev["nf"])
    assert np.array_equal(h1["rho"], dev["rho"]) and np.array_equal(h1["ro"], dev["ro"])
    assert np.array_equal(h1["vals"], dev["vals"], equal_nan=True)
    for b in range(B):
        if not c["ok"][b]:
            assert (h1["d"][b] == 7.0).all()
        elif c["nf"][b] == 1:
            assert np.abs(h1["d"][b] - dev["d"][b]).max() <= FWD_TOL * np.abs(dev["d"][b]).max()


@pytest.mark.parametrize("shape", dc.SHAPES, ids=dc.shape_id)
def test_dense_two_call_inertia(built, shape):
    """try_to_factorize with the inertia counts on the healthy and the indefinite problems: success as the oracle's; the counts
    are the oracle's too (Sylvester: they do not depend on the order while no pivot is near zero) — n positive pivots and no
    zero one where the problem is healthy, so the unit pad rows of the last tile are not counted.  Then solve_ldl! twice."""
    hipldl, syn, O = _mods()
    c = dc.oracle_case(shape)
    s = c["s"]
    idx = np.array([0, 2, 3, 4])
    B = len(idx)
    vals = np.ascontiguousarray(c["vals"][idx])
    eig_tol = hipldl.default_params()[0]
    orc = O.Oracle(s.N, c["rows"], c["cols"], O.canonical_perm(s.nvar, s.nequ, s.ncon))
    ref = [orc.try_to_factorize(vals[b], s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True) for b in range(B)]
    L = hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B)
    assert L.config["kernel"] == "dense"
    ok, npos, nzer = hipldl.try_to_factorize(L, vals, s.nvar, s.nequ, s.ncon, eig_tol, return_inertia=True)
    assert list(ok) == [r[0] for r in ref]
    assert list(ok) == ([True] * 4 if shape == dc.TALL else [True, False, False, True])
    assert list(npos) == [r[1] for r in ref] and list(nzer) == [r[2] for r in ref]
    for b in (0, 3):
        assert npos[b] == s.nvar and nzer[b] == 0
    for k in range(2):
        r = np.ascontiguousarray(c["rhs"][idx] * (k + 1.5))
        d = np.full((B, s.N), 7.0)
        hipldl.solve_ldl_(r, L.factor, d)
        for b in range(B):
            if ok[b]:
                assert backward_error(s, vals[b], r[b], d[b]) <= BWD_TOL
            else:
                assert (d[b] == 7.0).all()     # no factor: the rows stay as the caller passed them
    L.close()


def test_dense_auto_panel_choice_large_batch(built):
    """batch x tiles = 180 x 3 > 512: the handle picks the one-wavefront-per-tile panel kernel by itself (default options).  The
    five-problem mix tiled 36 times, the assertions of the device-entry test."""
    hipldl, syn, O = _mods()
    shape, rep = (129, 70, 0), 36
    c = dc.oracle_case(shape)
    s, B = c["s"], dc.MIX * rep
    L = hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B)
    assert L.config["kernel"] == "dense"
    refs = [c, _oracle_on(L.plan_array("perm").astype(np.int64), shape, c)]
    idx = np.tile(np.arange(dc.MIX), rep)
    A = _Args(s, B)
    A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
    A.call(hipldl, L, hipldl.default_params())
    _check_dev_outputs(A.read(), refs, s, c["rhs"][idx], idx)
    L.close()


def test_dense_graph_cache_states(built, monkeypatch, capfd):
    """The launch sequence of a call is replayed as a hipGraph cached per argument set (csrc/dense.hip, run_cached): captured on
    a miss, plain launches from the fifth miss in a row on, a hit resets that count, the ninth graph evicts the oldest.  Ten
    argument sets in an order that visits every state; every call must return what a handle without graphs returns, bit for
    bit (fixed summation order everywhere, atomics on integer counters only).  The captures are read off the library's own
    CNL_VERBOSE line, so a cache that never captured (or always did) does not pass on equal numbers alone."""
    import torch
    hipldl, syn, O = _mods()
    shape, B = dc.GRAPH_CASE
    c = dc.oracle_case(shape, B)
    s = c["s"]
    p = hipldl.default_params()
    assert list(c["ok"]) == [True, False, True] and list(c["nf"]) == [1, 20, 5]
    nsets = 10
    rhs_of = [np.ascontiguousarray(c["rhs"] * (1.0 + 0.25 * k)) for k in range(nsets)]   # the sets differ: a replay of the wrong graph shows
    Lref = hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(dense_graph=0))
    assert Lref.config["kernel"] == "dense"
    Aref = _Args(s, B)
    ref = []
    for k in range(nsets):
        Aref.fill(c["vals"], rhs_of[k], c["rho_old"])
        Aref.call(hipldl, Lref, p)
        ref.append(Aref.read())
    Lref.close()
    _check_dev_outputs(ref[0], [c], s, rhs_of[0], np.arange(B))
    L = hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B)
    sets = [_Args(s, B) for _ in range(nsets)]    # all alive at once: ten distinct sets of addresses
    assert len({a.vals.data_ptr() for a in sets}) == nsets
    #        capture, replay | captures 2..5 | 5th, 6th miss: plain | hit | captures 6..8 | 9th graph evicts set 0's | 5th miss in a row: plain | hit
    order = [0, 0, 1, 2, 3, 4, 5, 6, 0, 6, 7, 8, 9, 0, 1]
    cached = [1, 0, 2, 3, 4, 5, 0, 0, 0, 6, 7, 8, 8, 0, 0]   # graphs cached behind a call that captured, 0 where it did not
    # ... and behind that hit, with eight graphs held: set 0, whose graph was evicted, is captured again (evicts set 1's), then set 1
    order += [0, 1]
    cached += [8, 8]
    monkeypatch.setenv("CNL_VERBOSE", "1")
    capfd.readouterr()
    seen = []
    for call, k in enumerate(order):
        A = sets[k]
        A.fill(c["vals"], rhs_of[k], c["rho_old"])
        A.call(hipldl, L, p)
        out = A.read()
        err = capfd.readouterr().err
        seen.append(next((n for n in range(1, 10) if f"captured as a graph ({n} cached)" in err), 0))
        for name in ("d", "rho", "ro", "nf", "ok"):
            assert np.array_equal(out[name], ref[k][name]), (call, k, name)
        assert np.array_equal(out["vals"], ref[k]["vals"], equal_nan=True), (call, k)
    monkeypatch.delenv("CNL_VERBOSE")
    L.close()
    assert seen == cached


def test_dense_general_form_multi_pass_ladder(built):
    """An irregular pattern served as ONE dense matrix of order 454 (cnl_options general_dense = 2): eight tiles per side, so the
    ladder's workgroup takes the row tiles of a panel step in two passes.  Newton step with and without the ladder."""
    hipldl, syn, O = _mods()
    s, vals, rhs = dc.general_case(3)
    opts = hipldl.Options(general_dense=2)
    info, cfg = run_case(s, vals, rhs, options=opts)
    assert cfg["kernel"] == "dense" and s.N - info["ncond"] >= 449
    v2 = vals.copy()
    off = s.offsets()
    v2[:, off[0]:off[1]] *= -20.0   # indefinite top-left block: the ladder climbs to nfact = 6
    run_case(s, v2, rhs, check_fwd=False, options=opts)
