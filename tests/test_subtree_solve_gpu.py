"""The solve sweeps of subtree handles in panels of 16 pivots (tuning subtree_solve_panels = P: bit 0 the backward stage launches, bit 1
the forward stage launches of solve_ldl!) against the same handle with the key off and against the CPU oracle.  -m gpu.

Shapes, handle options, mixes, oracles and bars are those of tests/support/general_subtrees_cases.py (the seven-kind mix in double)
and tests/support/f32_subtrees_cases.py (the five-kind mix in float) at the cuts of the existing subtree tests; the handles, the guarded
argument arrays (a sentinel row in front of and behind the rows of a call, all of which must come back untouched) and the three-call
runner are those of tests/test_subtree_wide_gpu.py.  tests/test_subtree_solve_cpu.py vouches for the panel cut and the LDS bounds.

What is asserted: P = 2 leaves every output of every call bit-equal to P = 0 (the forward substitution in panels performs the
operations of the unpanelled loop on every element in their order).  P = 1 and P = 3 leave every decision and the factor's verdicts
bit-equal, d within the existing bars against the oracle on both problem orders (BWD_TOL / FWD_TOL of tests/test_gpu_parity.py in
double, of tests/support/f32_general.py in float) and within FWD_TOL of the key-off d, the rows of d of failed problems at their
sentinel; and d is a fixed function of the front: bit-equal between calls, batches and active prefixes."""
import numpy as np
import pytest

from tests import test_subtree_wide_gpu as WG
from tests.support import subtree_solve_cases as SP

GS, FS, GC = WG.GS, WG.FS, WG.GC
pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
TYPES = pytest.mark.parametrize("T", (f64, f32), ids=("double", "float"))
DECISIONS = ("newton_ok", "newton_nf", "newton_rho", "newton_ro", "newton_vals", "factor_ok", "host_ok", "npos", "nzero")
CASES = [(shape, cond) for shape in SP.GPU_SHAPES for cond in (True, False)] + [(SP.CHAIN, True)]
CASE_IDS = [f"{GS.shape_id(s)}-{'condensed' if c else 'uncondensed'}" for s, c in CASES]


def _handle(hipldl, c, T, shape, B, P=0, **kw):
    L = WG._handle(hipldl, c, T, shape, B, **dict(kw, **SP.key_options(P)))
    assert L.config["subtree_solve_panels"] == P, L.config
    return L


def _fwd_tol(T):
    return FS.FWD_TOL if T is f32 else WG.FWD_TOL


def _close_d(on, off, ok, tol, what):
    """d of the problems that hold a solution within tol of the key-off d, problem by problem (max norm); the others at the sentinel"""
    worst, equal = 0.0, True
    for b in range(len(ok)):
        if not ok[b]:
            assert (on[b] == 7.0).all() and (off[b] == 7.0).all(), (what, b)
            continue
        fe = float(np.abs(on[b].astype(f64) - off[b].astype(f64)).max() / np.abs(off[b].astype(f64)).max())
        worst = max(worst, fe)
        equal &= bool(np.array_equal(WG._bits(on[b]), WG._bits(off[b])))
        assert fe <= tol, (what, b, fe, tol)
    return worst, equal


def _two_solves(hipldl, c, L, T, idx):
    """factorize_dev once, solve_dev twice on that factor with different right-hand sides, through guarded arrays"""
    A = WG.Guarded(c["s"], len(idx), T)
    A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
    A.factorize(hipldl, L, WG._params(c, T)[0])
    A.solve(hipldl, L)
    first = A.read()
    import torch
    A.a["rhs"][A.G:A.G + len(idx)].copy_(torch.from_numpy(np.array(c["rhs"][idx][::-1] * 1.5 + 0.25, T)))
    A.a["d"].fill_(7.0)
    n0 = hipldl.launch_counts()["general"]
    A.solve(hipldl, L)
    assert hipldl.launch_counts()["general"] - n0 == 2 * (len(L.plan_array("gstage_ptr")) - 1)
    torch.cuda.synchronize()
    second = A.a["d"].cpu().numpy()
    assert (second[:A.G] == 7.0).all() and (second[A.G + len(idx):] == 7.0).all()
    return dict(ok=first["ok"], d1=first["d"], d2=second[A.G:A.G + len(idx)].copy())


def _compare(hipldl, c, L, T, P, idx, ref, ref2, counts, what):
    """one handle with mask P on the problems idx against the key-off outputs ref (three calls) and ref2 (two solves on one factor)"""
    out = WG._run_all(hipldl, c, L, T, idx, counts)
    two = _two_solves(hipldl, c, L, T, idx)
    if P == 2:
        WG._same(out, ref, what)
        WG._same(two, ref2, what)
        return out, (0.0, True)
    for k in DECISIONS:
        assert out[k].dtype == ref[k].dtype and np.array_equal(WG._bits(out[k]), WG._bits(ref[k])), (what, k)
    assert np.array_equal(two["ok"], ref2["ok"])
    tol = _fwd_tol(T)
    w = [_close_d(out["newton_d"], ref["newton_d"], ref["newton_ok"], tol, (what, "newton")),
         _close_d(out["solve_d"], ref["solve_d"], ref["factor_ok"], tol, (what, "solve")),
         _close_d(two["d1"], ref2["d1"], ref2["ok"], tol, (what, "solve 1 of 2")),
         _close_d(two["d2"], ref2["d2"], ref2["ok"], tol, (what, "solve 2 of 2"))]
    WG._oracle(hipldl, c, L, T, out, idx)
    return out, (max(x[0] for x in w), all(x[1] for x in w))


# ---- 1. every mask against the key off, both orders, blocked and not; the oracle; the launch counts ----
@TYPES
@pytest.mark.parametrize("shape,cond", CASES, ids=CASE_IDS)
def test_masks_against_key_off(built, shape, cond, T):
    hipldl = WG._mods()
    c = WG._case(shape, T)
    B = len(c["vals"])
    orders = (np.arange(B), np.arange(B)[::-1].copy())
    for blocked in (1, 0):
        L0 = _handle(hipldl, c, T, shape, B, cond=cond, blocked=blocked)
        S = len(L0.plan_array("gstage_ptr")) - 1
        counts = (2 * S + 2, S + 1, 2 * S)
        ref = [WG._run_all(hipldl, c, L0, T, idx, counts) for idx in orders]
        ref2 = [_two_solves(hipldl, c, L0, T, idx) for idx in orders]
        fronts = sorted({f[:2] for st in SP.fronts_by_stage(L0) for f in st})
        L0.close()
        for P in (2, 1, 3):
            L = _handle(hipldl, c, T, shape, B, P, cond=cond, blocked=blocked)
            for idx, r, r2 in zip(orders, ref, ref2):
                out, (worst, equal) = _compare(hipldl, c, L, T, P, idx, r, r2, counts, (GS.shape_id(shape), cond, blocked, P))
            L.close()
            print(f"{GS.shape_id(shape)} {'float' if T is f32 else 'double'} cond {cond} blocked {blocked} P {P}: stages {S}, largest pivot count "
                  f"{max(f[0] for f in fronts)}, d against key off: worst {worst:.2e}, bit-equal {equal}")


# ---- 2. with the staged ladder ----
@TYPES
def test_with_subtree_ladder(built, T):
    """R = 3 with the key against R = 3 without: (R + 2) S + R + 3 launches, the decisions bit for bit, d within the bars"""
    hipldl = WG._mods()
    R, shape = 3, GS.GRID12
    c = WG._case(shape, T)
    B = len(c["vals"])
    idx = np.arange(B)
    L0 = _handle(hipldl, c, T, shape, B, subtree_ladder=R)
    S = len(L0.plan_array("gstage_ptr")) - 1
    counts = ((R + 2) * S + R + 3, S + 1, 2 * S)
    ref, ref2 = WG._run_all(hipldl, c, L0, T, idx, counts), _two_solves(hipldl, c, L0, T, idx)
    WG._oracle(hipldl, c, L0, T, ref, idx)
    L0.close()
    for P in (2, 1, 3):
        L = _handle(hipldl, c, T, shape, B, P, subtree_ladder=R)
        assert L.config["subtree_ladder"] == R, L.config
        _compare(hipldl, c, L, T, P, idx, ref, ref2, counts, ("ladder", P))
        L.close()


# ---- 3. what the handle reports ----
def test_config_reports_the_mask_where_it_acts(built):
    hipldl = WG._mods()
    c = GS.case(GS.GRID12)
    s = c["s"]
    mk = lambda **o: hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=GC.MIX,
                                         options=hipldl.Options(**GS.options(plan_kind=hipldl.PLAN_THROUGHPUT, **o)))
    for P in SP.MASKS:
        L = mk(v1_tpp=256, task_cap=4, subtree_solve_panels=P)
        assert L.config["general_subtrees"] and L.config["subtree_solve_panels"] == P, L.config
        L.close()
    for name, opt in (("64 threads", dict(v1_tpp=64, task_cap=4)), ("a single task", dict(v1_tpp=256, task_cap=1000))):
        L = mk(subtree_solve_panels=3, **opt)
        assert not L.config["general_subtrees"] and L.config["subtree_solve_panels"] == 0, (name, L.config)
        L0 = mk(**opt)
        outs = []
        for h in (L, L0):      # ... and runs as without the key
            A = WG.Guarded(s, GC.MIX, f64)
            A.fill(c["vals"], c["rhs"], c["rho_old"])
            n0 = hipldl.launch_counts()["general"]
            A.newton(hipldl, h, c["params"])
            assert hipldl.launch_counts()["general"] - n0 == 1
            outs.append(A.read())
        WG._same(outs[0], outs[1], name)
        L.close()
        L0.close()


# ---- 4. d is a fixed function of the front ----
@TYPES
def test_results_do_not_depend_on_what_lds_and_the_scratch_hold(built, T):
    """P = 3: the mix, then a call on OTHER values (every problem's kind shifted by three, values tripled: every task region and the LDS
    of every compute unit the call used hold another problem's numbers), then the mix again: bit-equal in every output of every call."""
    hipldl = WG._mods()
    shape = GS.GRID16
    c = WG._case(shape, T)
    B = len(c["vals"])
    idx = np.arange(B)
    L = _handle(hipldl, c, T, shape, B, 3)
    first, first2 = WG._run_all(hipldl, c, L, T, idx), _two_solves(hipldl, c, L, T, idx)
    WG._oracle(hipldl, c, L, T, first, idx)
    sh = (idx + 3) % B
    A = WG.Guarded(c["s"], B, T)
    A.fill(c["vals"][sh] * T(3), c["rhs"][sh], c["rho_old"][sh])
    A.newton(hipldl, L, WG._params(c, T))
    A.solve(hipldl, L)
    A.read()
    WG._same(WG._run_all(hipldl, c, L, T, idx), first)
    WG._same(_two_solves(hipldl, c, L, T, idx), first2)
    L.close()


@TYPES
def test_results_do_not_depend_on_batch_grid_or_active_prefix(built, T):
    """P = 3: the rows of d of a problem are bit-equal in the full batch, in an active prefix of 5 and in a handle of batch 1"""
    hipldl = WG._mods()
    shape = GS.GRID16
    c = WG._case(shape, T)
    B = len(c["vals"])
    def calls(L, idx):
        """newton_system_dev, then factorize_dev and solve_dev, on the problems idx through guarded arrays"""
        A = WG.Guarded(c["s"], len(idx), T)
        A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
        A.newton(hipldl, L, WG._params(c, T))
        r = A.read()
        out = {"newton_" + k: r[k] for k in ("d", "ok", "nf", "rho", "ro", "vals")}
        A.fill(c["vals"][idx], c["rhs"][idx], c["rho_old"][idx])
        A.factorize(hipldl, L, WG._params(c, T)[0])
        A.solve(hipldl, L)
        r = A.read()
        return dict(out, factor_ok=r["ok"], solve_d=r["d"])

    L = _handle(hipldl, c, T, shape, B, 3)
    full = calls(L, np.arange(B))
    assert full["newton_ok"].sum() >= 2 and full["factor_ok"].sum() >= 2
    nb = 5
    hipldl.set_active_batch(L, nb)
    part = calls(L, np.arange(nb))
    for k in full:
        assert np.array_equal(WG._bits(part[k]), WG._bits(full[k][:nb])), k
    hipldl.set_active_batch(L, B)
    perm = L.plan_array("perm")
    L.close()
    L1 = _handle(hipldl, c, T, shape, 1, 3)
    assert np.array_equal(L1.plan_array("perm"), perm)
    for b in (0, int(np.flatnonzero(full["newton_ok"])[-1])):
        one = calls(L1, np.array([b]))
        for k in full:
            assert np.array_equal(WG._bits(one[k][0]), WG._bits(full[k][b])), (b, k)
    L1.close()


# ---- 5. with the launch shapes of the factorising stages, and on a 1 024-thread handle ----
@TYPES
@pytest.mark.parametrize("shape", (GS.GRID32, GS.FOREST4), ids=GS.shape_id)
def test_with_wide_stages_and_lds_panels(built, shape, T):
    hipldl = WG._mods()
    c = WG._case(shape, T)
    B = len(c["vals"])
    idx = np.arange(B)
    L0 = _handle(hipldl, c, T, shape, B, W=1, M=4096)
    S = len(L0.plan_array("gstage_ptr")) - 1
    counts = (2 * S + 2, S + 1, 2 * S)
    assert L0.config["subtree_wide"] and L0.config["subtree_lds_panels"], L0.config
    ref, ref2 = WG._run_all(hipldl, c, L0, T, idx, counts), _two_solves(hipldl, c, L0, T, idx)
    L0.close()
    for P in (2, 3):
        L = _handle(hipldl, c, T, shape, B, P, W=1, M=4096)
        assert L.config["subtree_wide"] and L.config["subtree_lds_panels"], L.config
        _compare(hipldl, c, L, T, P, idx, ref, ref2, counts, ("wide", P))
        L.close()


def test_1024_thread_handle(built):
    """a Float64 handle configured with 1 024 threads: rows of a panel on whole wavefronts"""
    hipldl = WG._mods()
    c = GS.case(GS.GRID32)
    s = c["s"]
    idx = np.arange(GC.MIX)
    mk = lambda **o: hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=GC.MIX,
                                         options=hipldl.Options(**GS.options(plan_kind=hipldl.PLAN_THROUGHPUT, v1_tpp=1024, general_blocked=1, **o)))
    L0 = mk()
    assert L0.config["tpp"] == 1024 and L0.config["general_subtrees"] and L0.config["subtree_solve_panels"] == 0, L0.config
    S = len(L0.plan_array("gstage_ptr")) - 1
    counts = (2 * S + 2, S + 1, 2 * S)
    ref, ref2 = WG._run_all(hipldl, c, L0, f64, idx, counts), _two_solves(hipldl, c, L0, f64, idx)
    L0.close()
    for P in (2, 1, 3):
        L = mk(subtree_solve_panels=P)
        assert L.config["tpp"] == 1024 and L.config["subtree_solve_panels"] == P, L.config
        _compare(hipldl, c, L, f64, P, idx, ref, ref2, counts, ("1024 threads", P))
        L.close()
