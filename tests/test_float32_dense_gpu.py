"""Float32 handles on the dense backend (cnl_create_f32 with tuning float32_general = 1, float32_dense = 1: the float kernels of
csrc/dense_f32.hip) against the fp64 oracle on the widened float32 inputs with ParamCaNNOLeS(Float32) widened.  -m gpu.

Inputs, reference, tolerances and the per-call assertions are those of tests/support/f32_dense.py; tests/test_float32_dense_cpu.py
vouches for the inputs (every decision of every rung at least 1e-3 away from a flip, by eigenvalues), so no problem is skipped or
reclassified here.  The asymmetric places a wrong C / D lane map of the f32 matrix instruction would show in — w != 1 in J'WJ, the
off-diagonal tiles of S, the G tiles — are all on the way to d: a misplaced row fails the backward error."""
import numpy as np
import pytest

from tests.support import f32_dense as FD
from tests.support import f32_general as G

pytestmark = pytest.mark.gpu

CNL_ERR_ARG = 1


def _mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    return hipldl, syn


def _handle(hipldl, c, B, **opt):
    s = c["s"]
    L = hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32,
                            options=hipldl.Options(**FD.OPTIONS, **opt))
    assert L.config["kernel"] == "dense" and L.config["float32"] and not L.config["band"], L.config
    return L


class _Args:
    """one argument set of cnl_newton_system_f32_dev on the device"""

    def __init__(self, s, B):
        import torch
        dev = torch.device("cuda:0")
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self.vals, self.rhs, self.d = torch.zeros((B, s.nnzNS), **f32), torch.zeros((B, s.N), **f32), torch.zeros((B, s.N), **f32)
        self.ro, self.rho = torch.zeros(B, **f32), torch.zeros(B, **f32)
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
        hipldl.newton_system_dev(L, self.vals, self.rhs, self.d, self.ro, self.rho, self.nf, self.ok, p,
                                 stream=torch.cuda.current_stream().cuda_stream)

    def read(self):
        import torch
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("vals", "d", "ro", "rho", "nf", "ok")}


def _solve_dev_check(hipldl, L, s, vals_left, ok0, seed):
    """cnl_solve_f32_dev with a fresh rhs uses the factorisation (and the rho) the ladder ended on"""
    import torch
    B = len(ok0)
    rhs2 = np.random.default_rng(seed).standard_normal((B, s.N)).astype(np.float32)
    t_rhs2 = torch.from_numpy(rhs2).to("cuda:0")
    t_x = torch.zeros_like(t_rhs2)
    hipldl.solve_dev(L, t_rhs2, t_x, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    x = t_x.cpu().numpy()
    for b in range(B):
        if ok0[b]:
            be = G.backward_error(s, vals_left[b], rhs2[b], x[b])
            assert be <= FD.BWD_TOL, (b, be)


# ---- 1. device entry, every shape, both panel kernels ----
@pytest.mark.parametrize("panel_blocks", [0, 2])
@pytest.mark.parametrize("shape", FD.SHAPES, ids=FD.shape_id)
def test_dev_entry_against_the_oracle(built, shape, panel_blocks):
    hipldl, syn = _mods()
    c = FD.case(shape)
    s, B = c["s"], FD.MIX
    L = _handle(hipldl, c, B, dense_panel_blocks=panel_blocks)
    A = _Args(s, B)
    for idx in (np.arange(B), np.arange(B)[::-1]):     # the second call, batch reversed, finds nothing stale from the first
        A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
        A.call(hipldl, L, c["p32"])
        out = A.read()
        be, fe = FD.check_outputs(c, out, idx, c["vals"][idx])
        print(f"{FD.shape_id(shape)} panel_blocks {panel_blocks}: backward error {be / FD.EPS32:.1f} eps32, forward error {fe:.2e}")
    _solve_dev_check(hipldl, L, s, out["vals"], c["ok"][idx], seed=5)
    L.close()


# ---- 2. the two-call sequence ----
@pytest.mark.parametrize("shape", FD.SHAPES, ids=FD.shape_id)
def test_two_call_sequence(built, shape):
    """try_to_factorize: success as the oracle's on problems 0, 2, 3, 4; on the healthy ones n positive pivots and no zero one (the
    unit pad rows of the last tile are no pivots); the indefinite ones only fail — M(0) may have interior eigenvalues near zero, so
    the float counts are not pinned.  Then solve_ldl! twice; no factor, no change of d."""
    hipldl, syn = _mods()
    c = FD.case(shape)
    s = c["s"]
    idx = np.array([0, 2, 3, 4])
    B = len(idx)
    vals = np.ascontiguousarray(c["vals"][idx])
    want = [True] * 4 if shape == FD.TALL else [True, False, False, True]
    assert want == [bool(c["ok"][b] and c["nf"][b] == 1) for b in idx]     # the oracle's first attempt
    L = _handle(hipldl, c, B)
    ok, npos, nzer = hipldl.try_to_factorize(L, vals, s.nvar, s.nequ, s.ncon, float(c["p32"][0]), return_inertia=True)
    assert list(ok) == want
    for b in range(B):
        if want[b]:
            assert npos[b] == s.nvar and nzer[b] == 0
    for k in range(2):
        r = np.ascontiguousarray(c["rhs"][idx] * np.float32(k + 1.5))
        d = np.full((B, s.N), 7.0, np.float32)
        hipldl.solve_ldl_(r, L.factor, d)
        for b in range(B):
            if ok[b]:
                be = G.backward_error(s, vals[b], r[b], d[b])
                assert be <= FD.BWD_TOL, (b, be)
            else:
                assert (d[b] == 7.0).all()
    L.close()


# ---- 3. host-pointer call = device call ----
@pytest.mark.parametrize("shape", [(129, 70, 0), (126, 150, 4)], ids=FD.shape_id)
def test_host_entry_equals_dev_entry(built, shape):
    hipldl, syn = _mods()
    c = FD.case(shape)
    s, B = c["s"], FD.MIX
    L = _handle(hipldl, c, B)
    A = _Args(s, B)
    A.fill(c["vals"], c["rhs"], c["rho_old"])
    A.call(hipldl, L, c["p32"])
    dev = A.read()
    FD.check_outputs(c, dev, np.arange(B), c["vals"])
    v, d = c["vals"].copy(), np.full((B, s.N), 7.0, np.float32)
    _, ok, rho, ro, nf = hipldl.newton_system_(d, s.nvar, s.nequ, s.ncon, c["rhs"].copy(), v, L, c["rho_old"].copy(), c["p32"])
    L.close()
    assert np.array_equal(ok, dev["ok"].astype(bool)) and np.array_equal(nf, dev["nf"])
    assert np.array_equal(FD.bits(rho), FD.bits(dev["rho"])) and np.array_equal(FD.bits(ro), FD.bits(dev["ro"]))
    assert np.array_equal(FD.bits(v), FD.bits(dev["vals"]))
    assert np.array_equal(FD.bits(d), FD.bits(dev["d"]))     # bit for bit, the untouched rows of the hopeless problem included


# ---- 4. graph replay ----
def test_graph_replay(built):
    """The same argument set called twice (capture, then replay) against a handle without graphs: every output bit-equal, and call 1
    equals call 2."""
    hipldl, syn = _mods()
    shape, B = FD.GRAPH_CASE
    c = FD.case(shape, B)
    s = c["s"]
    outs = {}
    for graph in (0, 1):
        L = _handle(hipldl, c, B, dense_graph=graph)
        A = _Args(s, B)
        outs[graph] = []
        for _ in range(2):
            A.fill(c["vals"], c["rhs"], c["rho_old"])
            A.call(hipldl, L, c["p32"])
            outs[graph].append(A.read())
        L.close()
    FD.check_outputs(c, outs[0][0], np.arange(B), c["vals"])
    for name in ("vals", "d", "ro", "rho", "nf", "ok"):
        for graph, call in ((0, 1), (1, 0), (1, 1)):
            assert outs[graph][call][name].tobytes() == outs[0][0][name].tobytes(), (name, graph, call)


# ---- 5. large batch ----
def test_large_batch_picks_its_panel_kernel(built):
    """batch x tiles = 180 x 3 > 512: the handle picks the one-wavefront-per-tile panel kernel by itself.  The five-problem mix tiled
    36 times, the assertions of the device-entry test."""
    hipldl, syn = _mods()
    shape, rep = (129, 70, 0), 36
    c = FD.case(shape)
    s, B = c["s"], FD.MIX * rep
    L = _handle(hipldl, c, B)
    idx = np.tile(np.arange(FD.MIX), rep)
    A = _Args(s, B)
    A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
    A.call(hipldl, L, c["p32"])
    FD.check_outputs(c, A.read(), idx, c["vals"][idx])
    L.close()


# ---- 6. the key changes nothing elsewhere ----
def test_key_changes_nothing_elsewhere(built):
    hipldl, syn = _mods()
    s = syn.random_structure(60, 80, 4, 0.1, seed=3)
    rows, cols = s.kkt_pattern()
    vals, rhs = G.random_inputs(syn, s, range(100, 108))
    B = vals.shape[0]
    p32 = hipldl.default_params(np.float32)
    res = []
    for extra in ({}, dict(float32_dense=1)):
        L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32,
                                options=hipldl.Options(float32_general=1, **extra))
        v = vals.copy()
        d, ok, rho, ro, nf = hipldl.newton_system_(np.zeros((B, s.N), np.float32), s.nvar, s.nequ, s.ncon, rhs, v, L, np.zeros(B, np.float32), p32)
        res.append((L.config, v, d, ok, rho, ro, nf))
        L.close()
    assert res[0][0] == res[1][0] and res[0][0]["kernel"] == "v1"
    for a, b in zip(res[0][1:], res[1][1:]):
        assert a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    # a band pattern stays on the band kernels
    sb = syn.band_structure(200, 4)
    rb, cb = sb.kkt_pattern()
    Lb = hipldl.HIPLDLStruct(sb.N, rb, cb, None, sb.nvar, sb.nequ, sb.ncon, batch=8, dtype=np.float32, options=hipldl.Options(**FD.OPTIONS))
    assert Lb.config["kernel"] == "band" and Lb.config["float32"]
    Lb.close()
    # the key alone is an argument error that names both keys
    c = FD.case((129, 70, 0))
    sd = c["s"]
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.HIPLDLStruct(sd.N, c["rows"], c["cols"], None, sd.nvar, sd.nequ, sd.ncon, batch=2, dtype=np.float32, options=hipldl.Options(float32_dense=1))
    assert e.value.code == CNL_ERR_ARG and "float32_dense" in str(e.value) and "float32_general" in str(e.value)
    # dense_backend = 0: the handle without the key
    L0 = hipldl.HIPLDLStruct(sd.N, c["rows"], c["cols"], None, sd.nvar, sd.nequ, sd.ncon, batch=2, dtype=np.float32,
                             options=hipldl.Options(dense_backend=0, **FD.OPTIONS))
    assert L0.config["kernel"] == "v1" and L0.config["float32"]
    L0.close()


# ---- 7. against the existing Float32 path on the same inputs ----
def test_against_the_condense_handle(built):
    """d of the dense handle and of the float32_condense handle ("v1") on the healthy problems: within 2 FWD_TOL max|d_oracle| of each
    other, the bar tests/test_float32_general_gpu.py::test_band_pattern_on_the_general_kernel sets between two float handles."""
    hipldl, syn = _mods()
    c = FD.case((129, 70, 0))
    s = c["s"]
    idx = np.array([0, 4])
    B = len(idx)
    vals, rhs = np.ascontiguousarray(c["vals"][idx]), np.ascontiguousarray(c["rhs"][idx])
    ds = []
    for opt, kernel in ((FD.OPTIONS, "dense"), (dict(float32_general=1, float32_condense=1), "v1")):
        L = hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32, options=hipldl.Options(**opt))
        assert L.config["kernel"] == kernel and L.config["float32"], L.config
        v = vals.copy()
        d, ok, rho, ro, nf = hipldl.newton_system_(np.zeros((B, s.N), np.float32), s.nvar, s.nequ, s.ncon, rhs, v, L, np.zeros(B, np.float32), c["p32"])
        assert ok.all() and (nf == 1).all()
        ds.append(d.astype(np.float64))
        L.close()
    for k, b in enumerate(idx):
        diff = np.abs(ds[0][k] - ds[1][k]).max()
        assert diff <= 2 * FD.FWD_TOL * np.abs(c["d"][b]).max(), (b, diff)
