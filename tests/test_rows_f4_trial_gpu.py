"""Row f4 (`cgls_kernel`) and the trial point (`trial_point_kernel`) at every loop edge, in both element types, through hipldl's
wrappers on the cases of tests/support/rows_f4_cases.py (tests/test_rows_f4_trial_cpu.py checks those inputs without a GPU).  -m gpu.

CGLS: the LDS loops over the ncon-vectors in one, exactly one and two to four passes (p = 1, 3, 255, 256, 257, 1024 = CGLS_PMAX) and
the refusal above; constraint rows of 0, 1, 63, 64, 65, 128, 129 and 200 entries for the wavefront loop of `at_res`; rows that share
columns, so that a wrong beta or p update changes the answer; nvar < 256; itmax, atol, rtol, ones_if_zero away from their defaults,
itmax above INT_MAX; null Jxtr / iters; the per-handle workspace from one call to the next; problems of a batch kept apart.
Trial point: one chunk, exactly one chunk, one element in the second chunk, the x / r boundary inside a chunk, ncon = 0, 3, 130,
255, 256, 257, 1024, 1100, and the cap at equality (also beside entries that a scaling by 1e4 / 1e4 would change: on 1e4 and zeros
alone `>=` gives the bits of `>`), one ulp above it, far above it, at zero and with a NaN.  Every output array has a
guard row either side.

What is held to what.  Bit-equal: Jxtr, xt, rt, the `_jac` twins, everything a case calls bit-equal.  Iteration counts: the
restatement's of the same element type (its stopping margins are asserted >= 1e-3 on the CPU).  lambda against the restatement:
Float64 rtol 1e-10, atol 1e-12; Float32 the normal-equation residual <= 2e-3 ||Jc b|| and the distance to the least-squares solution
<= 1e-3 relative (the figures of the two older tests, which belong to the default tolerances); a Float32 run with itmax = 3 or with
rtol = 1e-3 is not near the least-squares solution, it is held to the restatement: k steps, each with two dot products of at most
nvar terms whose worst-case relative error is nvar eps32, so 2 k nvar eps32 of ||lambda|| (itmax = 3: 2.1e-4, where the second or
fourth iterate is 0.9 ||lambda|| away).  dlambda, lambdat: 4 eps.  And two judges formed in longdouble
from the inputs alone (rows_f4_cases.Judge), which a mistake shared by kernel and restatement does not pass:
  1. ||A'(A lambda - b)|| <= 2 max(threshold, the restatement's own value of it)   (the same number of steps, another reduction order;
     the factor 2 is over the reference, never over the kernel's output);
  2. ||lambda - lambda_ls|| <= ||A'(A lambda - b)|| / sigma_min(A)^2 (1 + 1e-6)   (derived; holds for any vector).
"""
import numpy as np
import pytest

from tests.support import rows_f4_cases as K

pytestmark = pytest.mark.gpu

IDS = {np.float64: "f64", np.float32: "f32"}
both_types = pytest.mark.parametrize("dtype", K.DTYPES, ids=[IDS[t] for t in K.DTYPES])
GUARD, IGUARD = 7.5, 77


def _mods():
    import torch
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl
    return torch, hipldl


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _same(a, b):
    """bit-equal arrays of one element type, NaN where the other has NaN (any payload)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    z = a.dtype.type(0)
    return np.array_equal(np.where(np.isnan(a), z, a).view(u), np.where(np.isnan(b), z, b).view(u))


def _handle(hipldl, s, B, dtype):
    """a handle of the element type (Float32: the general kernels, the band kernels do not serve these patterns)"""
    rows, cols = s.kkt_pattern()
    if dtype == np.float32:
        return hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32,
                                   options=hipldl.Options(float32_general=1))
    return hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B)


class Guarded:
    """a device array [B][n] with a guard row either side"""

    def __init__(self, torch, B, n, dtype, fill=GUARD):
        tt = {np.float64: torch.float64, np.float32: torch.float32, np.int32: torch.int32}[dtype]
        self.B, self.fill = B, fill
        self.all = torch.full((B + 2, max(n, 1)), fill, dtype=tt, device=torch.device("cuda", 0))
        self.t = self.all[1:B + 1]

    def get(self):
        """the rows of the batch, after checking that the guard rows are intact"""
        a = self.all.cpu().numpy()
        assert (a[0] == self.fill).all() and (a[-1] == self.fill).all(), "a guard row was written"
        return a[1:self.B + 1]


def _cgls(torch, hipldl, L, s, m, vals, dtype, outputs=True, **kw):
    """row f4 on `vals` and, through the `_jac` twin, on the model's arrays: bit-equal; returns (lambda, Jxtr, iterations)"""
    B = vals.shape[0]
    tv, tr, tJ, tJc = (_dev(torch, a) for a in (vals, m["r"], m["Jx"], m["Jcx"]))
    runs = []
    for jac in (False, True):
        lam, jt, it = Guarded(torch, B, s.ncon, dtype), Guarded(torch, B, s.nvar, dtype), Guarded(torch, B, 1, np.int32, IGUARD)
        o = dict(Jxtr_ptr=jt.t, iters_ptr=it.t) if outputs else {}
        if jac:
            hipldl.cgls_multipliers_jac_dev(L, s.nnzjF, s.nnzjc, tJ, tJc, tr, lam.t, **o, **kw)
        else:
            hipldl.cgls_multipliers_dev(L, tv, tr, lam.t, **o, **kw)
        torch.cuda.synchronize()
        runs.append((lam.get()[:, :s.ncon], jt.get()[:, :s.nvar], it.get()[:, 0]))
    for a, b in zip(runs[0], runs[1]):
        assert _same(a, b) if a.dtype != np.int32 else np.array_equal(a, b), "the `_jac` twin differs"
    return runs[0]


def _check_lambda(name, dtype, s, m, kw, b, lam, ref):
    """lambda of a problem that took steps: against the restatement, and against the least-squares problem itself"""
    lam0 = ref[0]
    J = K.Judge(s, m, b, dtype, **kw)
    assert np.array_equal(lam[J.dead], np.zeros(int(J.dead.sum()), dtype)), b     # a row without entries: lambda stays 0
    res, res0 = J.ne_residual(lam), J.ne_residual(lam0)
    print(f"{name} {IDS[dtype]} problem {b}: residual / threshold: kernel {res / J.threshold:.3g}, restatement {res0 / J.threshold:.3g}")
    if dtype == np.float64:
        np.testing.assert_allclose(lam, lam0, rtol=1e-10, atol=1e-12)
    elif 0 < kw.get("itmax", 0) < 100 or "rtol" in kw:
        assert np.linalg.norm(lam.astype(np.float64) - lam0) <= 2 * ref[2] * s.nvar * float(np.finfo(np.float32).eps) * np.linalg.norm(lam0), b
    else:
        dist, nls = J.distance(lam)
        assert res <= 2e-3 * J.s0, b
        assert dist <= 1e-3 * nls, b
    assert res <= 2 * max(J.threshold, res0), (b, res, res0, J.threshold)
    assert J.distance(lam)[0] <= J.distance_bound(lam), b


def _check_case(name, dtype, lam, jt, it):
    s, m, vals, kw = K.cgls_case(name, dtype)
    ref = K.cgls_reference(name, dtype)
    one = np.ones(s.ncon, dtype) if kw.get("ones_if_zero", True) else np.zeros(s.ncon, dtype)
    for b, (lam0, jt0, it0, _) in enumerate(ref):
        assert _same(jt[b], jt0), b
        assert it[b] == it0, (b, it[b], it0)
        if it0 == 0:     # r = 0, J_c = 0 or a NaN in r: no step, lambda = 1 (or the zeros it started from)
            assert _same(lam[b], one), b
        else:
            _check_lambda(name, dtype, s, m, kw, b, lam[b], ref[b])


@both_types
@pytest.mark.parametrize("name", list(K.CGLS_CASES))
def test_cgls_case(built, name, dtype):
    torch, hipldl = _mods()
    s, m, vals, kw = K.cgls_case(name, dtype)
    L = _handle(hipldl, s, vals.shape[0], dtype)
    lam, jt, it = _cgls(torch, hipldl, L, s, m, vals, dtype, **kw)
    L.close()
    _check_case(name, dtype, lam, jt, it)
    if name == "isolation":
        assert it[3] == 0 and np.array_equal(np.isnan(jt[3]), np.isnan(K.cgls_reference(name, dtype)[3][1])) and np.isnan(jt[3]).any()
        assert np.isfinite(lam).all() and np.isfinite(jt[[0, 1, 2, 4]]).all()


@both_types
def test_cgls_itmax_above_int_max(built, dtype):
    """itmax is an int64_t: typemax(Int64) and 2^32 mean "no limit", not the -1 and 0 their low 32 bits spell"""
    torch, hipldl = _mods()
    s, m, vals, _ = K.cgls_case("long-300", dtype)
    L = _handle(hipldl, s, vals.shape[0], dtype)
    want = _cgls(torch, hipldl, L, s, m, vals, dtype, itmax=0)
    assert (want[2] > 0).all()
    for itmax in K.HUGE_ITMAX + (2 ** 31, 2 ** 31 - 1):
        got = _cgls(torch, hipldl, L, s, m, vals, dtype, itmax=itmax)
        assert np.array_equal(got[2], want[2]) and _same(got[0], want[0]) and _same(got[1], want[1]), itmax
    L.close()


@both_types
def test_cgls_problems_of_a_batch_do_not_mix(built, dtype):
    """problems 0, 2, 4 beside a zero residual and a NaN: bit-equal to their run in a batch of three"""
    torch, hipldl = _mods()
    s, m, vals, _ = K.cgls_case("isolation", dtype)
    L5 = _handle(hipldl, s, 5, dtype)
    lam5, jt5, it5 = _cgls(torch, hipldl, L5, s, m, vals, dtype)
    L5.close()
    keep = [0, 2, 4]
    m3 = {k: np.ascontiguousarray(v[keep]) for k, v in m.items()}
    L3 = _handle(hipldl, s, 3, dtype)
    lam3, jt3, it3 = _cgls(torch, hipldl, L3, s, m3, np.ascontiguousarray(vals[keep]), dtype)
    L3.close()
    assert _same(lam5[keep], lam3) and _same(jt5[keep], jt3) and np.array_equal(it5[keep], it3) and (it3 > 0).all()


@both_types
def test_cgls_null_outputs(built, dtype):
    torch, hipldl = _mods()
    s, m, vals, _ = K.cgls_case("long-300", dtype)
    L = _handle(hipldl, s, vals.shape[0], dtype)
    lam, _, it = _cgls(torch, hipldl, L, s, m, vals, dtype)
    lam_only, _, _ = _cgls(torch, hipldl, L, s, m, vals, dtype, outputs=False)   # (the unused guarded arrays: checked untouched)
    L.close()
    assert (it > 0).all() and _same(lam_only, lam)


@both_types
def test_cgls_workspace_carries_nothing(built, dtype):
    """two calls on one handle with different r: the second one bit-equal to the same call on a fresh handle"""
    torch, hipldl = _mods()
    s, m, vals, _ = K.cgls_case("few-vars", dtype)
    B = vals.shape[0]
    m2 = dict(m, r=np.ascontiguousarray(3 * m["r"][::-1] + 1))
    used = _handle(hipldl, s, B, dtype)
    first = _cgls(torch, hipldl, used, s, m, vals, dtype)
    second = _cgls(torch, hipldl, used, s, m2, vals, dtype)
    used.close()
    fresh = _handle(hipldl, s, B, dtype)
    alone = _cgls(torch, hipldl, fresh, s, m2, vals, dtype)
    fresh.close()
    assert not _same(first[0], second[0])
    assert _same(second[0], alone[0]) and _same(second[1], alone[1]) and np.array_equal(second[2], alone[2])


@both_types
@pytest.mark.parametrize("shape", ["over-1100", "over-1025"])
def test_cgls_above_the_limit_is_refused(built, shape, dtype):
    torch, hipldl = _mods()
    s = K.pattern(shape)
    B = 2
    m = K.model(s, B, 1, dtype)
    vals = K.vals_of(s, m)
    L = _handle(hipldl, s, B, dtype)
    tv, tr, tJ, tJc = (_dev(torch, a) for a in (vals, m["r"], m["Jx"], m["Jcx"]))
    lam, jt, it = Guarded(torch, B, s.ncon, dtype), Guarded(torch, B, s.nvar, dtype), Guarded(torch, B, 1, np.int32, IGUARD)
    with pytest.raises(hipldl.CnlError):
        hipldl.cgls_multipliers_dev(L, tv, tr, lam.t, jt.t, iters_ptr=it.t)
    with pytest.raises(hipldl.CnlError):
        hipldl.cgls_multipliers_jac_dev(L, s.nnzjF, s.nnzjc, tJ, tJc, tr, lam.t, jt.t, iters_ptr=it.t)
    torch.cuda.synchronize()
    L.close()
    assert (lam.get() == GUARD).all() and (jt.get() == GUARD).all() and (it.get() == IGUARD).all()


@both_types
def test_cgls_without_constraints(built, dtype):
    torch, hipldl = _mods()
    s = K.pattern("no-constraints")
    B = 2
    m = K.model(s, B, 1, dtype)
    L = _handle(hipldl, s, B, dtype)
    tv, tr, tJ = (_dev(torch, a) for a in (K.vals_of(s, m), m["r"], m["Jx"]))
    hipldl.cgls_multipliers_dev(L, tv, tr, 0)
    hipldl.cgls_multipliers_jac_dev(L, s.nnzjF, 0, tJ, 0, tr, 0)
    torch.cuda.synchronize()
    L.close()


@both_types
@pytest.mark.parametrize("shape", K.TRIAL_SHAPES)
def test_trial_point_shape(built, shape, dtype):
    torch, hipldl = _mods()
    s = K.pattern(shape)
    x, r, lam, d, nan_slot = K.trial_batch(s, dtype)
    B, p = d.shape[0], s.ncon
    want = K.trial_reference(s, x, r, lam, d, dtype)
    L = _handle(hipldl, s, B, dtype)
    out = [Guarded(torch, B, n, dtype) for n in (s.nvar, s.nequ, p, p)]
    tx, tr, tl, td = (_dev(torch, a) for a in (x, r, lam, d))
    hipldl.trial_point_dev(L, tx, tr, tl if p else 0, td, K.MAX_DLAMBDA, out[0].t, out[1].t, out[2].t if p else 0, out[3].t if p else 0)
    torch.cuda.synchronize()
    L.close()
    xt, rt, lt, dl = (o.get()[:, :n] for o, n in zip(out, (s.nvar, s.nequ, p, p)))
    assert _same(xt, want[0]) and _same(rt, want[1])
    if not p:
        assert (out[2].all.cpu().numpy() == GUARD).all() and (out[3].all.cpu().numpy() == GUARD).all()
        return
    eps = float(np.finfo(dtype).eps)
    minus_d = -d[:, s.nvar + s.nequ:]
    v = {name: i for i, name in enumerate(K.TRIAL_VARIANTS)}
    nan = np.isnan(want[3])
    assert np.array_equal(np.isnan(dl), nan) and np.array_equal(np.isnan(lt), nan) and nan.sum() == 1 and nan[v["nan"], nan_slot]
    with np.errstate(invalid="ignore"):
        assert np.all((np.abs(dl - want[3]) <= 4 * eps * np.abs(want[3])) | nan)
        assert np.all((np.abs(lt - want[2]) <= 4 * eps * (np.abs(lam) + np.abs(want[3]))) | nan)
    for name in ("under", "exact", "exact-dust", "zero", "nan"):      # not capped: dlambda = -d, bit for bit
        assert _same(dl[v[name]], minus_d[v[name]]), name
    T = np.dtype(dtype).type
    assert dl[v["exact"], -1] == T(K.MAX_DLAMBDA)
    above = ("one-ulp-above", "far-above") + (("overflow",) if dtype == np.float32 else ())
    for name in above:                                    # capped
        assert not _same(dl[v[name]], minus_d[v[name]]), name
        assert np.isfinite(dl[v[name]]).all() and np.linalg.norm(dl[v[name]].astype(np.float64)) <= K.MAX_DLAMBDA * (1 + 4 * eps), name
    assert dl[v["one-ulp-above"], -1] == T(K.MAX_DLAMBDA)
