"""Row f4 with its ncon-vectors in the handle's workspace (`cgls_kernel<T, true>`, tuning cgls_wide), on the patterns and against the
restated recurrence of tests/support/rows_f4_cases.py, with the device helpers of tests/test_rows_f4_trial_gpu.py.  -m gpu.

Bit equality.  The wide instance does the operations of the LDS instance in the same order; only the address space of x, sv and pv
differs.  So a handle with cgls_wide = 2 returns lambda, Jxtr and the iteration counts of the default handle bit for bit, on the shapes
the f4 tests name for the loops over the ncon-vectors (p = 255, 256, 257, 1024), nvar < 256 and nvar + nequ odd, in both element types,
from `vals` and from the model's arrays, ones_if_zero on and off, itmax = 1, itmax above INT_MAX, beside a zero residual and a NaN
in r.  No tolerance applies.

Above 1 024 constraints (over-1025, over-1100, cgls_wide = 1) there is no LDS instance to compare with: iteration counts against the
restatement of the element type, lambda at the bars of tests/test_rows_f4_trial_gpu._check_lambda, after asserting on the CPU what makes
the count comparable: every stopping test at least 1e-3 away from its threshold, and no more steps than live constraints unless the
last test saw at most NOISE_ROOM of the threshold."""
import numpy as np
import pytest

from tests.support import loop_nonlinear_cases as LK
from tests.support import rows_f4_cases as K
from tests.test_rows_f4_trial_gpu import GUARD, IDS, IGUARD, Guarded, _cgls, _check_lambda, _dev, _mods, _same

pytestmark = pytest.mark.gpu
both_types = pytest.mark.parametrize("dtype", K.DTYPES, ids=[IDS[t] for t in K.DTYPES])
MARGIN = 1e-3     # (tests/test_rows_f4_trial_cpu.py)
CNL_ERR_ARG, CNL_ERR_DIM = 1, 2


def _handle(hipldl, s, B, dtype, **opt):
    rows, cols = s.kkt_pattern()
    if dtype == np.float32:
        opt = dict(opt, float32_general=1)
    return hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=dtype, options=hipldl.Options(**opt) if opt else None)


def _batch(shape, dtype, B=4):
    """problems 0 and 2 ordinary, problem 1 with r = 0 (no step; lambda = 1 under ones_if_zero), problem 3 with a NaN in r"""
    s = K.pattern(shape)
    m = K.model(s, B, 1, dtype)
    m["r"][1] = 0
    m["r"][3, 1] = np.nan     # (column 2: constraint rows 1 and 2 of every pattern have an entry there)
    return s, m, K.vals_of(s, m)


@both_types
@pytest.mark.parametrize("shape", ["p-255", "p-256", "p-257", "p-1024", "few-vars", "rect"])
def test_wide_instance_is_bit_equal_to_the_lds_instance(built, shape, dtype):
    torch, hipldl = _mods()
    s, m, vals = _batch(shape, dtype)
    B = vals.shape[0]
    lds, wide = _handle(hipldl, s, B, dtype), _handle(hipldl, s, B, dtype, cgls_wide=2)
    assert lds.config["cgls_wide"] == 0 and wide.config["cgls_wide"] == 2
    for kw in ({}, dict(ones_if_zero=False), dict(itmax=1), dict(itmax=K.HUGE_ITMAX[0]), dict(itmax=K.HUGE_ITMAX[1])):
        want = _cgls(torch, hipldl, lds, s, m, vals, dtype, **kw)      # (both value sources, guard rows checked)
        got = _cgls(torch, hipldl, wide, s, m, vals, dtype, **kw)
        assert _same(got[0], want[0]), (kw, "lambda")
        assert _same(got[1], want[1]), (kw, "Jxtr")
        assert np.array_equal(got[2], want[2]), (kw, got[2], want[2])
        it = want[2]
        assert it[1] == 0 and it[3] == 0 and (it[[0, 2]] == 1 if kw.get("itmax") == 1 else it[[0, 2]] > 1).all(), (kw, it)
        fill = np.zeros(s.ncon, dtype) if kw.get("ones_if_zero") is False else np.ones(s.ncon, dtype)
        assert _same(want[0][1], fill) and np.isnan(want[1][3]).any() and np.isfinite(want[0][[0, 2]]).all()
    lds.close()
    wide.close()


def _over_case(shape, dtype, B=2, seed=1):
    """the model of tests/test_rows_f4_trial_gpu.test_cgls_above_the_limit_is_refused and the restatement's results, with what makes an
    iteration count comparable asserted here, on the CPU"""
    s = K.pattern(shape)
    m = K.model(s, B, seed, dtype)
    vals = K.vals_of(s, m)
    ref = []
    for b in range(B):
        tr = []
        lam, jt, it, margin = K.restated(s, vals[b], m["r"][b], dtype, trace=tr)
        live = int((np.bincount(np.asarray(s.jc[0]) - 1, minlength=s.ncon) > 0).sum())
        assert margin > MARGIN, (shape, b, margin)
        assert 0 < it <= live and (it < live or tr[-1] <= K.NOISE_ROOM), (shape, b, it, live, tr[-1])
        ref.append((lam, jt, it, margin))
    return s, m, vals, ref


@both_types
@pytest.mark.parametrize("shape", ["over-1025", "over-1100"])
def test_above_1024_constraints_on_the_wide_instance(built, shape, dtype):
    """cgls_wide = 1: the handle runs what the default refuses (on a library without the key the handle is not created)"""
    torch, hipldl = _mods()
    s, m, vals, ref = _over_case(shape, dtype)
    B = vals.shape[0]
    L = _handle(hipldl, s, B, dtype, cgls_wide=1)
    assert L.config["cgls_wide"] == 1
    lam, jt, it = _cgls(torch, hipldl, L, s, m, vals, dtype)
    L.close()
    print(f"{shape} {IDS[dtype]}: iterations {it.tolist()}, restated {[r[2] for r in ref]}")
    for b in range(B):
        assert _same(jt[b], ref[b][1]), b
        assert it[b] == ref[b][2], (b, it[b], ref[b][2])
        _check_lambda(shape, dtype, s, m, {}, b, lam[b], ref[b])


@both_types
def test_wide_on_request_only(built, dtype):
    """cgls_wide = 0 is the default: over-1025 is CNL_ERR_DIM with nothing written; cgls_wide = 1 keeps the LDS instance up to 1024
    constraints (bit-equal either way, so the choice shows in nothing but the workspace); 3 is refused at creation"""
    torch, hipldl = _mods()
    s = K.pattern("over-1025")
    B = 2
    m = K.model(s, B, 1, dtype)
    vals = K.vals_of(s, m)
    tv, tr, tJ, tJc = (_dev(torch, a) for a in (vals, m["r"], m["Jx"], m["Jcx"]))
    for opt in ({}, dict(cgls_wide=0)):
        L = _handle(hipldl, s, B, dtype, **opt)
        assert L.config["cgls_wide"] == 0
        lam, jt, it = Guarded(torch, B, s.ncon, dtype), Guarded(torch, B, s.nvar, dtype), Guarded(torch, B, 1, np.int32, IGUARD)
        with pytest.raises(hipldl.CnlError) as e:
            hipldl.cgls_multipliers_dev(L, tv, tr, lam.t, jt.t, iters_ptr=it.t)
        assert e.value.code == CNL_ERR_DIM
        with pytest.raises(hipldl.CnlError) as e:
            hipldl.cgls_multipliers_jac_dev(L, s.nnzjF, s.nnzjc, tJ, tJc, tr, lam.t, jt.t, iters_ptr=it.t)
        assert e.value.code == CNL_ERR_DIM
        torch.cuda.synchronize()
        L.close()
        assert (lam.get() == GUARD).all() and (jt.get() == GUARD).all() and (it.get() == IGUARD).all()
    for bad in (3, -1):
        with pytest.raises(hipldl.CnlError) as e:
            _handle(hipldl, s, B, dtype, cgls_wide=bad)
        assert e.value.code == CNL_ERR_ARG and "cgls_wide" in str(e.value)
    s2, m2, vals2 = _batch("p-1024", dtype)
    L0, L1 = _handle(hipldl, s2, 4, dtype), _handle(hipldl, s2, 4, dtype, cgls_wide=1)
    a, b = _cgls(torch, hipldl, L0, s2, m2, vals2, dtype), _cgls(torch, hipldl, L1, s2, m2, vals2, dtype)
    L0.close()
    L1.close()
    assert _same(a[0], b[0]) and _same(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_loop_with_1025_nonlinear_constraints(built):
    """both gaps together: solve_batch_device on BandQuadConFamily(band_structure(2050, 1025), 2, seed) in Float64 against the host mirror,
    max_iter lowered on both sides (the mirror's factorisations of order 5 125 take a second each).  The loop asks for the wide instance
    itself; without it the first multiplier estimate is CNL_ERR_DIM."""
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import device_loop as DL
    ones = LK.scalar_runs(LK.wide_family(), "wide", max_iter=LK.WIDE_MAX_ITER)
    assert all(o["status"] == "max_iter" and o["nlinsolve"] == LK.WIDE_MAX_ITER + 1 for o in ones), [(o["status"], o["nlinsolve"]) for o in ones]
    got = DL.solve_batch_device(LK.wide_family("cuda:0"), max_iter=LK.WIDE_MAX_ITER)
    print(f"1025 constraints: device {got['status']}, " + ", ".join(f"{k} = {got[k].tolist()}" for k in LK.DECISIONS) + f"; kernel {got['kernel']}")
    assert got["cgls_wide"] == 1 and got["jct_shared"] is False
    assert got["status"] == LK.col(ones, "status")
    for k in LK.DECISIONS:
        assert got[k].tolist() == LK.col(ones, k), (k, got[k].tolist(), LK.col(ones, k))
    for b, o in enumerate(ones):   # the iterates after two Newton steps, at the bars of tests/test_loop_keywords_gpu._close_solutions
        assert np.allclose(got["solution"][b], o["solution"], atol=1e-7, rtol=1e-7), b
        assert np.allclose(got["multipliers"][b], o["multipliers"], atol=1e-6, rtol=1e-6), b
