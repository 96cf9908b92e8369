"""The per-stage launch shapes of subtree handles (tuning subtree_wide = W: 1 024-thread factorising stages on a 256-thread handle;
subtree_lds_panels = M: dependent pivot panels eliminated in LDS) against the same handle with both keys off, bit for
bit, and against the CPU oracle.  -m gpu.

Shapes, handle options, mixes, oracles and bars are those of tests/support/general_subtrees_cases.py (the seven-kind mix in double)
and tests/support/f32_subtrees_cases.py (the five-kind mix in float); tests/support/subtree_wide_cases.py restates the stage rule from
the plan's arrays, and tests/test_subtree_wide_cpu.py vouches for it and for the bounds of the LDS areas.  Every device call goes through
arrays with a sentinel row in front of and behind the rows of the call, all of which must come back untouched."""
import ctypes

import numpy as np
import pytest

from tests.support import subtree_ladder_cases as SL
from tests.support import subtree_wide_cases as SW
from tests.test_gpu_parity import BWD_TOL, FWD_TOL, backward_error

GS, FS, GC = SL.GS, SL.FS, SL.GC
pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
CAP = {GS.GRID12: 4, GS.FOREST3: 4}      # task_cap by shape (8 elsewhere): the cuts of the existing subtree tests
TYPES = pytest.mark.parametrize("T", (f64, f32), ids=("double", "float"))


def _mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl
    return hipldl


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(shape, T, B=None):
    if T is f32:
        return FS.case(shape) if B is None else FS.case(shape, B=B)
    return GS.case(shape) if B is None else GS.case(shape, B=B)


def _handle(hipldl, c, T, shape, B, cond=True, blocked=1, W=0, M=0, **extra):
    """the handle of the existing subtree tests for this element type — 256 threads per workgroup, forced —, with the two keys"""
    keys = dict(SW.key_options(W, M), task_cap=CAP.get(shape, 8), **extra)
    if T is f32:
        L = FS.handle(hipldl, c, B, **dict(FS.COND if cond else FS.UNCOND, **FS.KEY, float32_blocked=blocked, **FS.FORCED, **keys))
        assert L.config["float32_subtrees"] and L.config["float32_blocked"] == bool(blocked) and L.config["tpp"] == 256, L.config
        return L
    s = c["s"]
    opt = dict(v1_tpp=256, condense=int(cond), general_blocked=blocked, **keys)
    if shape[0] == "grid":
        opt = dict(plan_kind=hipldl.PLAN_THROUGHPUT, **opt)
    L = hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(**GS.options(**opt)))
    assert L.config["general_subtrees"] and L.config["general_blocked"] == bool(blocked) and L.config["tpp"] == 256, L.config
    return L


def _expected(L, T, W, M, batch):
    blocked = L.config["float32_blocked" if T is f32 else "general_blocked"]
    return SW.stage_rule(SW.stage_table(L), L.config["tpp"], blocked, 4 if T is f32 else 8, W, M, batch, _cus())


def _check_table(hipldl, L, T, W, M, batch):
    """cnl_subtree_stage_shape against the numpy rule at `batch` (the handle's active batch); returns the table"""
    tpp, lds = hipldl.subtree_stage_shape(L)
    want_tpp, want_lds = _expected(L, T, W, M, batch)
    assert tpp.dtype == np.int32 and lds.dtype == np.int32 and len(tpp) == len(lds) == len(L.plan_array("gstage_ptr")) - 1
    assert np.array_equal(tpp, want_tpp) and np.array_equal(lds, want_lds), (W, M, batch, tpp, want_tpp, lds, want_lds)
    return tpp, lds


class Guarded:
    """argument arrays of the device entries with one sentinel row in front of and behind the B rows of the call"""
    G = 1

    def __init__(self, s, B, T):
        import torch
        self.B, self.T, self.s = B, T, s
        dev = torch.device("cuda:0")
        ft = torch.float32 if T is f32 else torch.float64
        n = B + 2 * self.G
        self.a = dict(vals=torch.zeros((n, s.nnzNS), dtype=ft, device=dev), rhs=torch.zeros((n, s.N), dtype=ft, device=dev),
                      d=torch.zeros((n, s.N), dtype=ft, device=dev), ro=torch.zeros(n, dtype=ft, device=dev), rho=torch.zeros(n, dtype=ft, device=dev),
                      nf=torch.zeros(n, dtype=torch.int32, device=dev), ok=torch.zeros(n, dtype=torch.int32, device=dev))

    def ptr(self, k):
        return self.a[k][self.G:].data_ptr()

    def fill(self, vals, rhs, ro):
        import torch
        for k, v in (("vals", 3.0), ("rhs", 3.0), ("d", 7.0), ("ro", 3.0), ("rho", -1.0), ("nf", -1), ("ok", -1)):
            self.a[k].fill_(v)
        for k, v in (("vals", vals), ("rhs", rhs), ("ro", ro)):
            self.a[k][self.G:self.G + self.B].copy_(torch.from_numpy(np.array(v, self.T)))
        torch.cuda.synchronize()

    def stream(self):
        import torch
        return torch.cuda.current_stream().cuda_stream

    def newton(self, hipldl, L, p):
        hipldl.newton_system_dev(L, self.ptr("vals"), self.ptr("rhs"), self.ptr("d"), self.ptr("ro"), self.ptr("rho"), self.ptr("nf"), self.ptr("ok"), p,
                                 stream=self.stream())

    def factorize(self, hipldl, L, eig_tol):
        hipldl.factorize_dev(L, self.ptr("vals"), float(eig_tol), self.ptr("ok"), stream=self.stream())

    def solve(self, hipldl, L):
        hipldl.solve_dev(L, self.ptr("rhs"), self.ptr("d"), stream=self.stream())

    def read(self):
        """the B rows of every array; the sentinel rows must be what fill() left"""
        import torch
        torch.cuda.synchronize()
        out = {}
        for k, v in (("vals", 3.0), ("rhs", 3.0), ("d", 7.0), ("ro", 3.0), ("rho", -1.0), ("nf", -1), ("ok", -1)):
            h = self.a[k].cpu().numpy()
            assert (h[:self.G] == v).all() and (h[self.G + self.B:] == v).all(), k
            out[k] = h[self.G:self.G + self.B].copy()
        return out


def _bits(a):
    return SL.bits(a) if a.dtype.kind == "f" else a


def _same(a, b, what=""):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _params(c, T):
    return c["p32"] if T is f32 else c["params"]


def _run_all(hipldl, c, L, T, idx, counts=None):
    """The three calls of the plugin surface on the problems `idx` of the case, each through guarded arrays: newton_system_dev;
    factorize_dev and solve_dev; the host-pointer factorize with its inertia.  counts: the launches per call that are asserted.
    Returns every output as one dict."""
    s, B = c["s"], len(idx)
    p = _params(c, T)
    A = Guarded(s, B, T)
    out = {}
    A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
    n0 = hipldl.launch_counts()["general"]
    A.newton(hipldl, L, p)
    n1 = hipldl.launch_counts()["general"]
    r = A.read()
    out.update({"newton_" + k: r[k] for k in ("vals", "d", "ro", "rho", "nf", "ok")})
    assert (r["d"][r["ok"] == 0] == 7.0).all() and np.array_equal(_bits(r["rhs"]), _bits(np.array(c["rhs"][idx], T)))
    A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
    n2 = hipldl.launch_counts()["general"]
    A.factorize(hipldl, L, p[0])
    n3 = hipldl.launch_counts()["general"]
    A.solve(hipldl, L)
    n4 = hipldl.launch_counts()["general"]
    r = A.read()
    out.update(factor_ok=r["ok"], solve_d=r["d"])
    assert (r["d"][r["ok"] == 0] == 7.0).all() and (r["nf"] == -1).all() and (r["rho"] == -1.0).all()
    assert np.array_equal(_bits(r["vals"]), _bits(np.array(c["vals"][idx], T)))
    if counts is not None:
        assert (n1 - n0, n3 - n2, n4 - n3) == counts, ((n1 - n0, n3 - n2, n4 - n3), counts)
    ok, npos, nzer = hipldl.try_to_factorize(L, np.array(c["vals"][idx], T), s.nvar, s.nequ, s.ncon, p[0], return_inertia=True)
    out.update(host_ok=np.asarray(ok), npos=np.asarray(npos), nzero=np.asarray(nzer))
    return out


def _oracle(hipldl, c, L, T, out, idx):
    """the newton_system outputs of _run_all against the oracle on the canonical order and on the handle's own"""
    o = {k: out["newton_" + k] for k in ("vals", "d", "ro", "rho", "nf", "ok")}
    perm = L.plan_array("perm").astype(np.int64)
    if T is f32:
        for ref in (c, FS.oracle_on(perm, c)):
            FS.check_outputs(ref, o, idx, c["vals"][idx])
        return
    GC.check_outputs(o, [c, GC.oracle_on(perm, c)], c, c["rhs"][idx], idx, BWD_TOL, FWD_TOL, backward_error)


def _mixed_M(L):
    """an M between the F_s of two stages that both have a front of 16 pivots: LPAN for some of them, not for all (None: no such pair)"""
    F, tasks, has = SW.stage_table(L)
    fs = sorted(set(int(x) for x in F[has]))
    return fs[0] if len(fs) >= 2 else None


# ---- 1. the stage table ----
@TYPES
@pytest.mark.parametrize("shape", SW.GPU_SHAPES, ids=GS.shape_id)
def test_stage_table(built, shape, T):
    hipldl = _mods()
    c = _case(shape, T)
    B = len(c["vals"])
    L0 = _handle(hipldl, c, T, shape, B)
    F, tasks, has = SW.stage_table(L0)
    tpp, lds = _check_table(hipldl, L0, T, 0, 0, B)
    esz = 4 if T is f32 else 8
    assert (tpp == 256).all() and (lds == 16 * esz).all() and not L0.config["subtree_wide"] and not L0.config["subtree_lds_panels"]
    n = ctypes.c_int64(-1)
    assert hipldl.lib().cnl_subtree_stage_shape(L0._h, None, None, ctypes.byref(n)) == 0 and n.value == len(F)      # null arrays: the count alone
    mixed = _mixed_M(L0)
    L0.close()
    settings = [(1, 0), (int(F[-1]), 0), (int(F.max()) + 1, 0), (0, 4096), (0, 16), (1, 4096)]
    if mixed is not None:
        settings += [(0, mixed), (int(F[-1]), mixed)]
    if shape == GS.GRID32:
        assert mixed is not None      # fronts (21, 64) and (93, 0): panels on two levels of the tree, F_s 86 and 94
    for W, M in settings:
        L = _handle(hipldl, c, T, shape, B, W=W, M=M)
        tpp, lds = _check_table(hipldl, L, T, W, M, B)
        assert L.config["subtree_wide"] == bool((tpp == 1024).any()) and L.config["subtree_lds_panels"] == bool((lds > 16 * esz).any()), (W, M, L.config)
        if (W, M) == (1, 0):
            assert (tpp == 1024).all()           # (7 problems: no stage of these shapes reaches 2 x CUs workgroups)
        if W == int(F[-1]) and W > 1:
            assert tpp[-1] == 1024 and np.array_equal(tpp == 1024, F >= W)
        if W > F.max():
            assert (tpp == 256).all() and not L.config["subtree_wide"]
        if M == 4096:
            assert np.array_equal(lds > 16 * esz, has) and np.array_equal(lds[has], SW.need_bytes(F[has], esz))
        if M == 16:
            assert (lds == 16 * esz).all() and not L.config["subtree_lds_panels"]
        if mixed is not None and M == mixed:
            assert (lds > 16 * esz).any() and (lds[has] == 16 * esz).any()
        L.close()
    # an unblocked handle: M is refused at the creator (tests/test_subtree_wide_cpu.py); W acts
    L = _handle(hipldl, c, T, shape, B, blocked=0, W=1)
    tpp, lds = _check_table(hipldl, L, T, 1, 0, B)
    assert (tpp == 1024).all() and (lds == 16 * esz).all()
    L.close()


@TYPES
def test_batch_bound_and_active_prefix(built, T):
    """At a batch where the workgroups of stage 0 exceed twice the CU count stage 0 keeps 256 threads while the root is wide (bit 58 is
    set: it speaks of the created batch); on a small active prefix stage 0 becomes wide; the outputs of the prefix are those of keys off."""
    hipldl = _mods()
    shape = GS.GRID12
    probe = _handle(hipldl, _case(shape, T), T, shape, 1)
    F, tasks, has = SW.stage_table(probe)
    probe.close()
    B = 2 * _cus() // int(tasks[0]) + 1
    assert tasks[0] * B > 2 * _cus() >= tasks[-1] * B and tasks[-1] == 1
    c = _case(shape, T, B=B)
    L = _handle(hipldl, c, T, shape, B, W=1, M=4096)
    tpp, lds = _check_table(hipldl, L, T, 1, 4096, B)
    assert tpp[0] == 256 and tpp[-1] == 1024 and L.config["subtree_wide"]
    nb = 5
    idx = np.arange(nb)
    full = _run_all(hipldl, c, L, T, np.arange(B))
    hipldl.set_active_batch(L, nb)
    tpp, lds = _check_table(hipldl, L, T, 1, 4096, nb)
    assert (tpp == 1024).all()
    L0 = _handle(hipldl, c, T, shape, B)
    hipldl.set_active_batch(L0, nb)
    A, A0 = Guarded(c["s"], nb, T), Guarded(c["s"], nb, T)
    outs = []
    for a, h in ((A, L), (A0, L0)):
        a.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
        a.newton(hipldl, h, _params(c, T))
        outs.append(a.read())
    _same(outs[0], outs[1], "prefix")
    for k in ("vals", "d", "ro", "rho", "nf", "ok"):      # ... and those of the same problems in the full batch (stage 0 at 256 threads there)
        assert np.array_equal(_bits(outs[0][k]), _bits(full["newton_" + k][:nb])), k
    hipldl.set_active_batch(L, B)
    hipldl.set_active_batch(L0, B)
    L.close()
    L0.close()


# ---- 2, 3, 6. every output bit-equal to keys off; the oracle; the launch counts ----
@TYPES
@pytest.mark.parametrize("cond", (True, False), ids=("condensed", "uncondensed"))
@pytest.mark.parametrize("shape", SW.GPU_SHAPES, ids=GS.shape_id)
def test_bit_equal_to_keys_off(built, shape, cond, T):
    hipldl = _mods()
    c = _case(shape, T)
    B = len(c["vals"])
    orders = (np.arange(B), np.arange(B)[::-1].copy())
    for blocked in (1, 0):
        L0 = _handle(hipldl, c, T, shape, B, cond=cond, blocked=blocked)
        S = len(L0.plan_array("gstage_ptr")) - 1
        counts = (2 * S + 2, S + 1, 2 * S)
        F, tasks, has = SW.stage_table(L0)
        ref = [_run_all(hipldl, c, L0, T, idx, counts) for idx in orders]
        for idx, r in zip(orders, ref):
            _oracle(hipldl, c, L0, T, r, idx)
        settings = [(1, 0)]
        if blocked:
            settings += [(0, 4096), (1, 4096)]
            if _mixed_M(L0) is not None:
                settings.append((int(F[-1]), _mixed_M(L0)))      # the mixed tables: the widest stages alone wide, LPAN on the smaller panels alone
        L0.close()
        esz = 4 if T is f32 else 8
        for W, M in settings:
            L = _handle(hipldl, c, T, shape, B, cond=cond, blocked=blocked, W=W, M=M)
            tpp, lds = _check_table(hipldl, L, T, W, M, B)
            assert (tpp == 1024).any() == (W > 0) and (lds > 16 * esz).any() == bool(M > 0 and has.any() and M >= F[has].min()), (W, M, tpp, lds)
            for idx, r in zip(orders, ref):
                out = _run_all(hipldl, c, L, T, idx, counts)
                _same(out, r, (GS.shape_id(shape), cond, blocked, W, M))
                if (W, M) == settings[-1]:
                    _oracle(hipldl, c, L, T, out, idx)
            L.close()
        print(f"{GS.shape_id(shape)} {'float' if T is f32 else 'double'} cond {cond} blocked {blocked}: F_s {F.tolist()} panels {has.tolist()} settings {settings}: "
              f"every output bit-equal to keys off on both orders")


# ---- 4. with the staged ladder ----
@TYPES
@pytest.mark.parametrize("shape", (GS.GRID12, GS.GRID32), ids=GS.shape_id)
def test_with_subtree_ladder(built, shape, T):
    """R = 3 with the keys against R = 3 without, bit for bit; (R + 2) S + R + 3 launches"""
    hipldl = _mods()
    R = 3
    c = _case(shape, T)
    B = len(c["vals"])
    idx = np.arange(B)
    L0 = _handle(hipldl, c, T, shape, B, subtree_ladder=R)
    S = len(L0.plan_array("gstage_ptr")) - 1
    counts = ((R + 2) * S + R + 3, S + 1, 2 * S)
    ref = _run_all(hipldl, c, L0, T, idx, counts)
    _oracle(hipldl, c, L0, T, ref, idx)
    L0.close()
    for W, M in ((1, 0), (0, 4096), (1, 4096)):
        L = _handle(hipldl, c, T, shape, B, W=W, M=M, subtree_ladder=R)
        assert L.config["subtree_ladder"] == R and L.config["subtree_wide"] == (W > 0) and L.config["subtree_lds_panels"] == (M > 0), L.config
        _same(_run_all(hipldl, c, L, T, idx, counts), ref, (W, M))
        L.close()


# ---- 5. nothing depends on what LDS or the task regions held ----
@TYPES
def test_results_do_not_depend_on_what_the_state_holds(built, T):
    """The mix, then a call on OTHER values (every problem's kind shifted by three, values tripled), then the mix again: bit-equal to
    the first call in every output."""
    hipldl = _mods()
    shape = GS.GRID16
    c = _case(shape, T)
    B = len(c["vals"])
    idx = np.arange(B)
    L = _handle(hipldl, c, T, shape, B, W=1, M=4096)
    assert L.config["subtree_wide"] and L.config["subtree_lds_panels"], L.config
    first = _run_all(hipldl, c, L, T, idx)
    _oracle(hipldl, c, L, T, first, idx)
    sh = (idx + 3) % B
    A = Guarded(c["s"], B, T)
    A.fill(c["vals"][sh] * T(3), c["rhs"][sh], c["rho_old"][sh])
    A.newton(hipldl, L, _params(c, T))
    A.read()
    _same(_run_all(hipldl, c, L, T, idx), first)
    L.close()


# ---- handles on which a key does not act ----
def test_1024_thread_handle_and_non_subtree_handle(built):
    """A Float64 handle configured with 1 024 threads: subtree_wide does not act (bit 58 clear, every stage at the handle's count).  A
    handle that is no subtree handle (64 threads per problem): cnl_subtree_stage_shape is CNL_ERR_ARG."""
    hipldl = _mods()
    c = GS.case(GS.GRID12)
    s = c["s"]
    mk = lambda **o: hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=GC.MIX,
                                         options=hipldl.Options(**GS.options(plan_kind=hipldl.PLAN_THROUGHPUT, task_cap=4, **o)))
    L = mk(v1_tpp=1024, general_blocked=1, subtree_wide=1, subtree_lds_panels=4096)
    assert L.config["tpp"] == 1024 and L.config["general_subtrees"] and not L.config["subtree_wide"], L.config
    tpp, lds = _check_table(hipldl, L, f64, 1, 4096, GC.MIX)
    assert (tpp == 1024).all() and L.config["subtree_lds_panels"] == bool((lds > 128).any())
    L0 = mk(v1_tpp=1024, general_blocked=1)
    idx = np.arange(GC.MIX)
    _same(_run_all(hipldl, c, L, f64, idx), _run_all(hipldl, c, L0, f64, idx))
    L.close()
    L0.close()
    L = mk(v1_tpp=64, subtree_wide=1)
    assert not L.config["general_subtrees"] and not L.config["subtree_wide"] and not L.config["subtree_lds_panels"], L.config
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.subtree_stage_shape(L)
    assert e.value.code == 1
    L.close()
