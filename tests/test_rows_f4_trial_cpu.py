"""The inputs of tests/test_rows_f4_trial_gpu.py, checked without a GPU (tests/support/rows_f4_cases.py): the GPU tests must neither
fail on their inputs nor pass on them.

For every CGLS case and both element types: every stopping test of the restated recurrence lies at least MARGIN from its threshold (so
the kernel's differently ordered reductions cannot change an iteration count), cond(Jc') <= 100, and the restatement's own normal-
equation residual, formed in longdouble from the inputs, is at most its stopping threshold (a case that stops by its iteration limit
instead: its residual is above it), and no problem takes more steps than it has constraints or ends on rounding noise near the
threshold.  The float64 restatement is oracle.cgls_multipliers bit for bit; outer_loop.cgls, the host mirror of the loop (a third
copy of the recurrence), takes the oracle's number of steps and gives its lambda to 1e-12.  The trial-point restatements give the
variants at the cap and with a NaN as the cases specify them.
"""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import outer_loop
from oracle import oracle as O
from tests.support import rows_f4_cases as K

MARGIN = 1e-3
IDS = {np.float64: "f64", np.float32: "f32"}
both_types = pytest.mark.parametrize("dtype", K.DTYPES, ids=[IDS[t] for t in K.DTYPES])


def _same(a, b):
    """bit-equal arrays of one element type, NaN where the other has NaN (any payload)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    z = a.dtype.type(0)
    return np.array_equal(np.where(np.isnan(a), z, a).view(u), np.where(np.isnan(b), z, b).view(u))


@both_types
@pytest.mark.parametrize("name", list(K.CGLS_CASES))
def test_cgls_case_inputs(name, dtype):
    s, m, vals, kw = K.cgls_case(name, dtype)
    ref = K.cgls_reference(name, dtype)
    limit = kw.get("itmax", 0)
    for b, (lam, jt, it, margin) in enumerate(ref):
        assert lam.dtype == dtype and jt.dtype == dtype
        assert margin > MARGIN, f"problem {b}: a stopping test lies within {margin:.3g} of its threshold"
        if not m["Jcx"][b].any():
            assert it == 0
            continue
        J = K.Judge(s, m, b, dtype, **kw)
        assert J.cond <= 100, (b, J.cond)
        if np.isnan(m["r"][b]).any():
            assert it == 0 and np.isnan(jt).any() and np.array_equal(lam, np.ones(s.ncon, dtype))   # the recurrence ends at once
        elif not m["r"][b].any():
            assert it == 0 and J.s0 == 0
        elif 0 < limit < 100:
            assert it == limit and J.ne_residual(lam) > J.threshold, b    # stopped by the limit, not by the threshold
        else:
            assert it > 0 and J.ne_residual(lam) <= J.threshold, (b, J.ne_residual(lam), J.threshold)
            # finite termination: the test after step p sees rounding noise, which must lie well below the threshold (rows_f4_cases)
            live = int(J.live.sum())
            assert it <= live and (it < live or K.cgls_last_ratio(name, dtype)[b] <= K.NOISE_ROOM), (b, it, live)
            assert np.array_equal(lam[J.dead], np.zeros(J.dead.sum(), dtype))      # a row without entries keeps lambda = 0


def test_rtol_case_stops_earlier_than_the_defaults():
    """the case is about the threshold atol + rtol ||s0||: with the looser one some problem must take fewer steps"""
    for dtype in K.DTYPES:
        s, m, vals, kw = K.cgls_case("rtol", dtype)
        loose = [x[2] for x in K.cgls_reference("rtol", dtype)]
        tight = [K.restated(s, vals[b], m["r"][b], dtype)[2] for b in range(len(loose))]
        assert all(a <= b for a, b in zip(loose, tight)) and any(a < b for a, b in zip(loose, tight)), (loose, tight)


@pytest.mark.parametrize("name", list(K.CGLS_CASES))
def test_float64_restatement_is_the_oracle_and_the_host_mirror_agrees(built, name):
    s, m, vals, kw = K.cgls_case(name, np.float64)
    rows, cols = s.kkt_pattern()
    for b, (lam, jt, it, _) in enumerate(K.cgls_reference(name, np.float64)):
        with np.errstate(invalid="ignore"):
            lam0, jt0, it0 = O.cgls_multipliers(rows, cols, vals[b], s.nvar, s.nequ, s.ncon, m["r"][b], **kw)
        assert _same(lam, lam0) and _same(jt, jt0) and it == it0, b
        if np.isnan(jt0).any():
            continue
        # outer_loop.cgls returns lambda only: it took k steps when a limit of k changes nothing and a limit of k - 1 does
        A = np.zeros((s.nvar, s.ncon))
        A[np.asarray(s.jc[1]) - 1, np.asarray(s.jc[0]) - 1] = m["Jcx"][b]
        tol = {k: v for k, v in kw.items() if k in ("atol", "rtol")}
        free = outer_loop.cgls(A, jt0, itmax=kw.get("itmax", 0), **tol)
        assert np.array_equal(outer_loop.cgls(A, jt0, itmax=max(it0, 1), **tol), free), b
        if it0 > 0:
            assert not np.array_equal(outer_loop.cgls(A, jt0, itmax=it0 - 1, **tol) if it0 > 1 else np.zeros(s.ncon), free), b
            plain = O.cgls_multipliers(rows, cols, vals[b], s.nvar, s.nequ, s.ncon, m["r"][b], **{**kw, "ones_if_zero": False})[0]
            assert np.linalg.norm(free - plain) <= 1e-12 * np.linalg.norm(plain), b
        else:
            assert not free.any()


@both_types
@pytest.mark.parametrize("shape", [n for n in K.TRIAL_SHAPES if n != "no-constraints"])
def test_trial_point_variants(shape, dtype):
    s = K.pattern(shape)
    x, r, lam, d, nan_slot = K.trial_batch(s, dtype)
    xt, rt, lt, dl = K.trial_reference(s, x, r, lam, d, dtype)
    c0 = s.nvar + s.nequ
    minus_d = -d[:, c0:]
    T = np.dtype(dtype).type
    assert all(a.dtype == dtype for a in (xt, rt, lt, dl))
    v = {name: i for i, name in enumerate(K.TRIAL_VARIANTS)}
    assert _same(dl[v["under"]], minus_d[v["under"]])
    # norm exactly max_dlambda: `>` is false, nothing is scaled (the zeros stay -0.0)
    assert _same(dl[v["exact"]], minus_d[v["exact"]]) and dl[v["exact"], -1] == T(K.MAX_DLAMBDA) and np.signbit(dl[v["exact"], :-1]).all()
    # the same norm after rounding, beside entries that scaling by 1e4 / 1e4 would change: only `>` leaves them alone
    e = v["exact-dust"]
    M = T(K.MAX_DLAMBDA)
    assert T(np.sqrt(np.sum(minus_d[e].astype(np.float64) ** 2))) == M and _same(dl[e], minus_d[e])
    assert ((minus_d[e] * M) / M != minus_d[e])[:-1].all()
    # one ulp above: scaled back onto the cap
    assert minus_d[v["one-ulp-above"], -1] > T(K.MAX_DLAMBDA) and dl[v["one-ulp-above"], -1] == T(K.MAX_DLAMBDA)
    assert not _same(dl[v["far-above"]], minus_d[v["far-above"]])
    assert np.linalg.norm(dl[v["far-above"]].astype(np.float64)) <= K.MAX_DLAMBDA * (1 + 4 * float(np.finfo(dtype).eps))
    assert not dl[v["zero"]].any() and _same(lt[v["zero"]], lam[v["zero"]] + dl[v["zero"]])
    # a NaN makes the norm NaN and `>` false: not scaled, the NaN stays where it was
    only = np.zeros(s.ncon, bool)
    only[nan_slot] = True
    assert _same(dl[v["nan"]], minus_d[v["nan"]]) and np.array_equal(np.isnan(dl[v["nan"]]), only)
    assert np.array_equal(np.isnan(lt[v["nan"]]), only)
    if dtype == np.float32:
        with np.errstate(over="ignore"):
            assert np.isfinite(dl[v["overflow"]]).all() and np.isinf(minus_d[v["overflow"]] * minus_d[v["overflow"]]).any()
    assert _same(xt, x + d[:, :s.nvar]) and _same(rt, r + d[:, s.nvar:c0])
